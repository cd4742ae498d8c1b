"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for mi355_sk_fwd on the matrix-core branch
kernel (sk_wide_kernel of csrc/sk_wide.hip): the 32 x 32-group row with ragged row ends, the row whose input channels are staged in
chunks, the 3-in / 5-out row whose channel octet and output tile are mostly padding, and one shape the FMA kernels cover run with
options(sk_wide=1).  Module rows: parameters, buffers, x, y and the workspace of mi355_sk_ws_bytes (u1 / u2 planes, pooled sums, packed
weights) all live in the poisoned arena at 16-byte alignment.

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py: every kernel-selecting option of csrc/options.h is set by some row) see them in any run
that collects the test files that import it (tests/test_sk_wide_cpu.py, tests/test_sk_wide_arena_gpu.py); the latter runs them through
the harness."""
import torch

import arena_cases
import oracle as O
import sk_wide_cases as S
from arena_cases import TOL, row

IDS = []
ROW_CASES = (("g32x32_ragged", {}), ("chunked_512", {}), ("g3x5", {}), ("covered_ragged", dict(sk_wide=1)))


def _register():
    for cid, opts in ROW_CASES:
        case = S.BY_ID[cid]

        def make(seed, case=case):
            return dict(m=S.module(case), x=S.input_of(case))

        def run(F, d):
            return d["m"](d["x"])

        def ref(d, case=case):
            return O.sk_forward(d["x"].float(), d["m"].state_dict(), case[2], torch.float64)

        IDS.append(f"sk_wide_{cid}")
        row(id=IDS[-1], entries=("mi355_sk_fwd",), opts=dict(opts), prec=0, tol=TOL[0], tags=(S.WIDE_TAG,), make=make, run=run, ref=ref,
            module=True)
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
