"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for the three entries that carry an XCABlock on
fp16 / bf16 activations: mi355_linear16_res_scale_fwd (csrc/gemm16_res.hip), mi355_linear16_stats_r16_fwd (csrc/gemm16_wreg.hip) and
mi355_mlp_fused_o16_fwd (csrc/mlp_fused.hip), each at precision 1 and 2 = in both I/O types, at a ragged shape (M = 105: three images of
5 x 7 tokens, a partial last tile of every kernel) and at a model-sized one (M = 6272 = 256 x 196 / 8).  The LayerScale GEMM in the two
(residual, result) pairs a block uses -- a 16-bit residual into an fp32 stream (proj) and an fp32 residual into a 16-bit store (fc2) --
with a gamma and, once, without; the fused MLP at C = 64 (also under mlp_tt4 = 1) and at C = 128.

The two GEMM entries take row strides (ldx, ldy).  The table of tests/gemm_ld_cases.py and its one `invoke` are not this feature's to
extend, so they are entered in that table's ELSEWHERE list here, with the place that runs them strided:
tests/test_xcit_io16_gpu.py::test_gemm_entries_on_strided_rows (the "pad" and "block" patterns of that table, in a poisoned buffer,
bit for bit against the dense call).

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_xcit_io16_cpu.py, tests/test_xcit_io16_arena_gpu.py); the latter runs them through the harness."""
import torch

import arena_cases
import gemm_ld_cases
from arena_cases import TOL, _gen, _rn, gelu64, ln64, row

IDS = []
# (M, N, K, 16-bit residual, 16-bit result, gamma)
SCALE_SHAPES = ((105, 192, 192, True, False, True), (105, 256, 1024, False, True, True), (105, 192, 192, True, True, False),
                (6272, 384, 384, True, False, True), (6272, 384, 1536, False, True, True))
STATS_SHAPES = ((105, 256), (105, 384), (6272, 256), (6272, 384))                                       # (M, N = K)
MLP_SHAPES = ((105, 64, {}), (105, 64, dict(mlp_tt4=1)), (6272, 64, {}), (105, 128, {}), (6272, 128, {}))     # (M, C, options)


def _ln(C, g):
    ln = torch.nn.LayerNorm(C)
    with torch.no_grad():
        ln.weight.copy_(0.5 + torch.rand(C, generator=g))
        ln.bias.copy_(_rn(g, C, s=0.2))
    return ln.requires_grad_(False)


def _linear(K, N, g):
    lin = torch.nn.Linear(K, N)
    with torch.no_grad():
        lin.weight.copy_(_rn(g, N, K) / K ** 0.5)
        lin.bias.copy_(_rn(g, N, s=0.1))
    return lin.requires_grad_(False)


def _register():
    for dt, p in ((torch.float16, 1), (torch.bfloat16, 2)):
        tname = "f16" if p == 1 else "bf16"
        for (M, N, K, r16, o16, scaled) in SCALE_SHAPES:
            IDS.append(f"linear16_res_scale_{M}x{N}x{K}_{'r16' if r16 else 'r32'}_{'o16' if o16 else 'o32'}{'' if scaled else '_nogamma'}_p{p}")

            def make_mm(seed, M=M, N=N, K=K, r16=r16, scaled=scaled, dt=dt):
                g = _gen(seed)
                r = _rn(g, M, N, s=1.5)
                return dict(x=_rn(g, M, K).to(dt), w=(_rn(g, N, K) / K ** 0.5).to(dt), b=_rn(g, N, s=0.1), r=r.to(dt) if r16 else r,
                            g=0.5 + torch.rand(N, generator=g) if scaled else None)

            def ref_mm(d):
                z = d["x"].double() @ d["w"].double().t() + d["b"].double()
                return d["r"].double() + (z if d["g"] is None else z * d["g"].double())
            row(id=IDS[-1], entries=("mi355_linear16_res_scale_fwd",), prec=p, tol=TOL[p], make=make_mm, ref=ref_mm,
                run=lambda F, d, o16=o16, dt=dt, p=p: F.linear16_res_scale(d["x"], d["w"], d["b"], d["g"], d["r"],
                                                                          out_dtype=dt if o16 else torch.float32, precision=p),
                tags=(f"gemm16_res_kernel<{tname},{'r16' if r16 else 'r32'},{'o16' if o16 else 'o32'}{',scale' if scaled else ''}>",))
        for (M, N) in STATS_SHAPES:
            IDS.append(f"linear16_stats_r16_{M}x{N}_p{p}")

            def make_st(seed, M=M, N=N, dt=dt):
                g = _gen(seed)
                return dict(x=_rn(g, M, N).to(dt), w=(_rn(g, N, N) / N ** 0.5).to(dt), b=_rn(g, N, s=0.1), r=_rn(g, M, N, s=1.5).to(dt))

            def ref_st(d):
                y = d["r"].double() + d["x"].double() @ d["w"].double().t() + d["b"].double()
                return y, torch.stack([y.mean(-1), 1.0 / torch.sqrt(y.var(-1, unbiased=False) + 1e-6)], dim=-1)
            row(id=IDS[-1], entries=("mi355_linear16_stats_r16_fwd",), prec=p, tol=TOL[p], make=make_st, ref=ref_st,
                run=lambda F, d, p=p: F.linear16_stats_r16(d["x"], d["w"], d["b"], d["r"], 1e-6, precision=p),
                tags=(f"gemm16_wreg_kernel<{tname},resid16+stats>",))
        for (M, C, opts) in MLP_SHAPES:
            IDS.append(f"mlp_fused_o16_{M}x{C}{'_tt4' if opts else ''}_p{p}")

            def make_mlp(seed, M=M, C=C):
                g = _gen(seed)
                return dict(x=_rn(g, M, C) * 1.3 + 0.2, ln=_ln(C, g), fc1=_linear(C, 4 * C, g), fc2=_linear(4 * C, C, g),
                            g=0.5 + torch.rand(C, generator=g))

            def ref_mlp(d):
                lin = lambda t, m: t @ m.weight.double().t() + m.bias.double()      # noqa: E731
                x = d["x"].double()
                u = ln64(x, d["ln"].weight, d["ln"].bias, d["ln"].eps)
                return x + d["g"].double() * lin(gelu64(lin(u, d["fc1"])), d["fc2"])
            row(id=IDS[-1], entries=("mi355_mlp_fused_o16_fwd",), prec=p, tol=TOL[p], opts=dict(opts), make=make_mlp, ref=ref_mlp,
                run=lambda F, d, p=p: F.mlp_fused_o16(d["x"], d["ln"], d["fc1"], d["fc2"], gamma=d["g"], precision=p),
                tags=(f"mlp_fused_kernel<C={C},o16>",))
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})
    for entry in ("mi355_linear16_res_scale_fwd", "mi355_linear16_stats_r16_fwd"):
        gemm_ld_cases.ELSEWHERE.setdefault(entry, "a GEMM entry of the XCiT 16-bit path: run on padded and column-block strides, in a poisoned buffer, "
                                                  "by tests/test_xcit_io16_gpu.py::test_gemm_entries_on_strided_rows")


_register()
