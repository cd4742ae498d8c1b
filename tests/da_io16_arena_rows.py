"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for mi355_double_attn16_fwd
(csrc/double_attn.hip): DoubleAttention on fp16 / bf16 activations.  One shape per route -- the one-kernel path (2,64,32,32) c 32, the
two-pass path (2,256,8,8) c 128, the general route (2,64,10,10) c 32 -- in both I/O types, with option "da_fused" at 1 and at 0 (0 sends
every shape down the general route).

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_da_io16_cpu.py, tests/test_da_io16_arena_gpu.py); the latter runs them through the harness."""
import math

import torch

import arena_cases
import oracle.chan_attn as OC
from arena_cases import TOL, _gen, _rn, row

IDS = []
SHAPES = (((2, 64, 32, 32), 32), ((2, 256, 8, 8), 128), ((2, 64, 10, 10), 32))
NAMES = ("wA", "bA", "wB", "bB", "wV", "bV", "wP", "bP")


def _register():
    for shape, c in SHAPES:
        C = shape[1]
        sid = "x".join(map(str, shape))
        for dt, p in ((torch.float16, 1), (torch.bfloat16, 2)):
            def make(seed, shape=shape, dt=dt, C=C, c=c):
                g = _gen(seed)
                return dict(x=_rn(g, *shape).to(dt), wA=_rn(g, c, C) / math.sqrt(C), bA=_rn(g, c, s=0.1), wB=_rn(g, c, C) / math.sqrt(C),
                            bB=_rn(g, c, s=0.1), wV=_rn(g, c, C) / math.sqrt(C), bV=_rn(g, c, s=0.1), wP=_rn(g, C, c) / math.sqrt(c),
                            bP=_rn(g, C, s=0.1))
            for fused in (1, 0):
                IDS.append(f"da16_{sid}_c{c}_f{fused}_p{p}")
                row(id=IDS[-1], entries=("mi355_double_attn16_fwd",), opts=dict(da_fused=fused), prec=p, tol=TOL[p], make=make,
                    run=lambda F, d: F.double_attention_forward(d["x"], *(d[k] for k in NAMES)),
                    ref=lambda d: OC.double_attention_forward(d["x"].double(), *(d[k] for k in NAMES), dtype=torch.float64))
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
