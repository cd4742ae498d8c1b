"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for the six 16-bit entries of the CNN SE variants
and the channel-statistics gates: mi355_se16_ex_fwd (csrc/chan_io16.hip) and mi355_simam16_fwd .. mi355_gct16_fwd
(csrc/chan_stat_io16.hip).  A single-read shape and a ragged one, both I/O types, both forms.

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_zoo_io16_cpu.py, tests/test_zoo_io16_arena_gpu.py); the latter runs them through the harness."""
import math

import torch

import arena_cases
import oracle as O
from arena_cases import TOL, _gen, _rn, row

IDS = []


def _register():
    for shape in ((2, 64, 32, 32), (3, 72, 7, 7)):
        B, C, H, W = shape
        sid = "x".join(map(str, shape))
        forms = (1, 0) if H * W % 8 == 0 else (1,)
        for dt, p in ((torch.float16, 1), (torch.bfloat16, 2)):
            def make(seed, shape=shape, dt=dt, C=C):
                g = _gen(seed)
                return dict(x=_rn(g, *shape).to(dt), w1=_rn(g, C // 4, C) / math.sqrt(C), b1=_rn(g, C // 4), w2=_rn(g, C, C // 4) / math.sqrt(C // 4),
                            b2=_rn(g, C), cfc=_rn(g, C, 1, 2), bw=0.5 + torch.rand(C, generator=g), bb=_rn(g, C, s=0.5), bm=_rn(g, C, s=0.3),
                            bv=0.5 + torch.rand(C, generator=g), lw=_rn(g, C), lb=_rn(g, C), al=0.5 + torch.rand(C, generator=g), ga=_rn(g, C),
                            be=_rn(g, C, s=0.5))
            x64 = lambda d: d["x"].double()
            f64 = torch.float64
            gates = (
                ("simam16", "mi355_simam16_fwd", lambda F, d: F.simam_forward(d["x"], 1e-4), lambda d: O.simam_forward(x64(d), 1e-4, f64)),
                ("srm16", "mi355_srm16_fwd", lambda F, d: F.srm_forward(d["x"], d["cfc"], d["bw"], d["bb"], d["bm"], d["bv"], 1e-5),
                 lambda d: O.srm_forward(x64(d), d["cfc"], d["bw"], d["bb"], d["bm"], d["bv"], 1e-5, f64)),
                ("gctg16", "mi355_gct_gauss16_fwd", lambda F, d: F.gct_gauss_forward(d["x"], 2, 1e-5), lambda d: O.gct_gauss_forward(x64(d), 2, 1e-5, f64)),
                ("lct16", "mi355_lct16_fwd", lambda F, d: F.lct_forward(d["x"], d["lw"], d["lb"], 4, 1e-5),
                 lambda d: O.lct_forward(x64(d), d["lw"], d["lb"], 4, 1e-5, f64)),
                ("gct16_l2", "mi355_gct16_fwd", lambda F, d: F.gct_forward(d["x"], d["al"], d["ga"], d["be"], 1e-5, "l2"),
                 lambda d: O.gct_forward(x64(d), d["al"], d["ga"], d["be"], 1e-5, "l2", False, f64)),
                ("gct16_l1", "mi355_gct16_fwd", lambda F, d: F.gct_forward(d["x"], d["al"], d["ga"], d["be"], 1e-5, "l1"),
                 lambda d: O.gct_forward(x64(d), d["al"], d["ga"], d["be"], 1e-5, "l1", False, f64)),
            )
            for name, sym, run, ref in gates:
                for single in forms:
                    IDS.append(f"{name}_{sid}_s{single}_p{p}")
                    row(id=IDS[-1], entries=(sym,), opts=dict(zoo_single=single), prec=p, tol=TOL[p], make=make, run=run, ref=ref)
            for gate in ("sigmoid", "hard_sigmoid"):
                for single in forms:
                    IDS.append(f"se16_ex_{gate}_{sid}_s{single}_p{p}")
                    row(id=IDS[-1], entries=("mi355_se16_ex_fwd",), opts=dict(se_single=single), prec=p, tol=TOL[p], make=make,
                        run=lambda F, d, gate=gate: F.se_ex_forward(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], gate=gate),
                        ref=lambda d, gate=gate: O.se_ex_forward(x64(d), d["w1"], d["b1"], d["w2"], d["b2"], gate, f64))
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
