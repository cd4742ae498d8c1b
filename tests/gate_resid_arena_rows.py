"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for the three entries of the residual (+ ReLU)
epilogue of SELayer / ECALayer / CBAM: mi355_se_res_fwd, mi355_eca_res_fwd, mi355_cbam_res_fwd (csrc/chan_attn.hip, chan_fused.hip,
cbam_single.hip, chan_io16.hip).  A single-read shape and a ragged one, all three I/O types, both forms, relu on and off.

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_gate_resid_cpu.py, tests/test_gate_resid_arena_gpu.py); the latter runs them through the harness."""
import math

import torch

import arena_cases
import oracle as O
from arena_cases import TOL, VEC, _gen, _rn, row

IDS = []
SHAPES = ((2, 64, 32, 32), (3, 72, 7, 7))
TYPES = ((torch.float32, 0), (torch.float16, 1), (torch.bfloat16, 2))
ENTRIES = {"se": "mi355_se_res_fwd", "eca": "mi355_eca_res_fwd", "cbam": "mi355_cbam_res_fwd"}


def _register():
    f64 = torch.float64
    for shape in SHAPES:
        B, C, H, W = shape
        sid = "x".join(map(str, shape))
        for dt, p in TYPES:
            forms = (1, 0) if H * W % (8 if p else 4) == 0 else (1,)     # a ragged map takes the general form under either option value
            def make(seed, shape=shape, dt=dt, C=C):
                g = _gen(seed)
                return dict(x=_rn(g, *shape).to(dt), r=_rn(g, *shape, s=0.7).to(dt), w1=_rn(g, C // 4, C) / math.sqrt(C),
                            w2=_rn(g, C, C // 4) / math.sqrt(C // 4), wc=_rn(g, 1, 2, 7, 7, s=0.2), we=_rn(g, 3, s=0.5))
            gates = (
                ("se", "se_single", lambda F, d, relu: F.se_forward(d["x"], d["w1"], d["w2"], resid=d["r"], relu=relu),
                 lambda d: O.se_forward(d["x"].double(), d["w1"], d["w2"], f64)),
                ("eca", "eca_single", lambda F, d, relu: F.eca_forward(d["x"], d["we"], resid=d["r"], relu=relu),
                 lambda d: O.eca_forward(d["x"].double(), d["we"].reshape(1, 1, -1), f64)),
                ("cbam", "cbam_single", lambda F, d, relu: F.cbam_forward(d["x"], d["w1"], d["w2"], d["wc"], resid=d["r"], relu=relu),
                 lambda d: O.cbam_forward(d["x"].double(), d["w1"], d["w2"], d["wc"], f64)),
            )
            for name, option, run, gate in gates:
                for single in forms:
                    for relu in (False, True):
                        IDS.append(f"{name}_res_{sid}_s{single}_p{p}_relu{int(relu)}")
                        def ref(d, gate=gate, relu=relu):
                            s = gate(d) + d["r"].double()
                            return torch.relu(s) if relu else s
                        row(id=IDS[-1], entries=(ENTRIES[name],), opts={option: single}, prec=p, tol=TOL[p] if p else VEC, make=make,
                            run=lambda F, d, run=run, relu=relu: run(F, d, relu), ref=ref)
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
