"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for the two entries that carry a ViT encoder
block on fp16 / bf16 activations: mi355_layernorm16_x16_fwd (csrc/layernorm.hip) and mi355_linear16_res_fwd (csrc/gemm16_res.hip), each
in both I/O types.  The LayerNorm at a packed width with a ragged last wave and at a width off the packed kernel; the GEMM at a shape
ragged in every dimension (row, column and wave tails of a single tile) and at one with several tiles, in the three (residual, result)
type pairs.

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_vit_io16_cpu.py, tests/test_vit_io16_arena_gpu.py); the latter runs them through the harness."""
import torch

import arena_cases
from arena_cases import TOL, _gen, _rn, gelu64, ln64, row

IDS = []
PAIRS = (("r16_o32", True, False), ("r32_o16", False, True), ("r16_o16", True, True))


def _register():
    for dt, p in ((torch.float16, 1), (torch.bfloat16, 2)):
        tname = "f16" if p == 1 else "bf16"
        for rows_, cols in ((33, 384), (9, 52)):
            IDS.append(f"layernorm16_x16_{rows_}x{cols}_p{p}")

            def make_ln(seed, rows_=rows_, cols=cols, dt=dt):
                g = _gen(seed)
                return dict(x=(_rn(g, rows_, cols) * 2 + 0.5).to(dt), w=0.5 + torch.rand(cols, generator=g), b=_rn(g, cols, s=0.2))
            row(id=IDS[-1], entries=("mi355_layernorm16_x16_fwd",), prec=p, tol=TOL[p], make=make_ln,
                run=lambda F, d: F.layernorm16_x16(d["x"], d["w"], d["b"], 1e-5),
                ref=lambda d: ln64(d["x"], d["w"], d["b"], 1e-5), tags=(f"layernorm_x16_kernel<{tname}>",))
        for (M, N, K, gelu) in ((77, 72, 192, False), (394, 256, 256, True)):
            for pname, r16, o16 in PAIRS:
                IDS.append(f"linear16_res_{M}x{N}x{K}_{pname}_p{p}")

                def make_mm(seed, M=M, N=N, K=K, r16=r16, dt=dt):
                    g = _gen(seed)
                    r = _rn(g, M, N, s=1.5)
                    return dict(x=_rn(g, M, K).to(dt), w=(_rn(g, N, K) / K ** 0.5).to(dt), b=_rn(g, N, s=0.1), r=r.to(dt) if r16 else r)

                def ref_mm(d, gelu=gelu):
                    z = d["x"].double() @ d["w"].double().t() + d["b"].double()
                    return d["r"].double() + (gelu64(z) if gelu else z)
                row(id=IDS[-1], entries=("mi355_linear16_res_fwd",), prec=p, tol=TOL[p], make=make_mm, ref=ref_mm,
                    run=lambda F, d, gelu=gelu, o16=o16, dt=dt, p=p: F.linear16_res(d["x"], d["w"], d["b"], d["r"], act=1 if gelu else 0,
                                                                                     out_dtype=dt if o16 else torch.float32, precision=p),
                    tags=(f"gemm16_res_kernel<{tname},{'r16' if r16 else 'r32'},{'o16' if o16 else 'o32'}>",))
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
