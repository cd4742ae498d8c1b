"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for the entries of csrc/dual_attn_io16.hip: CAM
and the two x-touching steps of PAM on fp16 / bf16 activations (mi355_cam_x16_fwd, mi355_conv1x1_tokens16_fwd,
mi355_tokens_to_nchw_axpy_x16_fwd).  Each forward at one aligned shape (2,64,8,8: 16-byte rows) and one ragged shape (3,30,9,7: C off every
multiple, odd H*W) in both I/O types; the ragged projection has Cout = 90 (no multiple of 4) and the ragged axpy reads the first C columns
of token rows that are 12 wider (ld_tokens = C + 12).

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_dual_io16_cpu.py, tests/test_dual_io16_arena_gpu.py); the latter runs them through the harness."""
import torch

import arena_cases
import oracle.axis_attn as OA
from arena_cases import TOL, _gen, _rn, row

IDS = []
SHAPES = ((2, 64, 8, 8), (3, 30, 9, 7))


def _rows_of(w):
    """(Cout, Cin) -> the (Cout, ldw) operand rows of mi355_conv2d_tokens_fwd: ldw % 4 == 0, zero padding beyond Cin."""
    out = torch.zeros(w.shape[0], (w.shape[1] + 3) // 4 * 4)
    out[:, :w.shape[1]] = w
    return out


def _register():
    for shape in SHAPES:
        B, C, H, W = shape
        sid = "x".join(map(str, shape))
        for dt, p in ((torch.float16, 1), (torch.bfloat16, 2)):
            IDS.append(f"cam16_{sid}_p{p}")
            row(id=IDS[-1], entries=("mi355_cam_x16_fwd",), prec=p, tol=TOL[p],
                make=lambda seed, s=shape, dt=dt: dict(x=(_rn(_gen(seed), *s, s=3.0) / (s[2] * s[3]) ** 0.5).to(dt), beta=torch.tensor([0.7])),
                run=lambda F, d: F.cam_forward(d["x"], d["beta"]),
                ref=lambda d: OA.cam_forward(d["x"].double(), {"beta": d["beta"]}, torch.float64))
            cout = 3 * C
            IDS.append(f"conv1x1_tokens16_{sid}_o{cout}_p{p}")

            def make_conv(seed, s=shape, dt=dt, cout=cout):
                g = _gen(seed)
                return dict(x=_rn(g, *s, s=0.5).to(dt), w=_rows_of(_rn(g, cout, s[1]) / s[1] ** 0.5), bias=_rn(g, cout, s=0.1))
            row(id=IDS[-1], entries=("mi355_conv1x1_tokens16_fwd",), prec=0, tol=TOL[0], make=make_conv,
                run=lambda F, d: F.conv1x1_tokens16(d["x"], d["w"], d["bias"]),
                ref=lambda d, C=C: torch.einsum("bcp,oc->bpo", d["x"].double().flatten(2), d["w"][:, :C].double()) + d["bias"].double())
            extra = 0 if shape == SHAPES[0] else 12
            IDS.append(f"axpy16_{sid}_ld{C + extra}_p{p}")

            def make_axpy(seed, s=shape, dt=dt, extra=extra):
                g = _gen(seed)
                return dict(wide=_rn(g, s[0], s[2] * s[3], s[1] + extra), x=_rn(g, *s).to(dt), alpha=torch.tensor([0.7]))
            row(id=IDS[-1], entries=("mi355_tokens_to_nchw_axpy_x16_fwd",), prec=p, tol=TOL[p], make=make_axpy,
                run=lambda F, d, C=C: F.tokens_to_nchw_axpy(d["wide"][:, :, :C], d["x"], d["alpha"]),
                ref=lambda d, s=shape: (d["alpha"].double() * d["wide"][:, :, :s[1]].double().transpose(1, 2).reshape(s) + d["x"].double()))
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
