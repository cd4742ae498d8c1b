"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for mi355_sdpa_general_fwd on the wide-head
kernel (sdpa_wide_kernel of csrc/sdpa_general.hip): one head of width 320 (two value slices of 192 + 128 columns) and 640 (three slices
of 256 + 256 + 128), precision 0 / 1 / 2, N_q = 70 (a whole query block and a partial one) against N_kv = 35 (one partial key tile).
q, k and v are slices of one fused (B, N, 3 * width) projection; the output is a (B, N_q, width) view into rows of width + 12 floats
that start out as zeros, and the whole buffer is returned: the kernel must leave the gap columns -- and everything outside `out` --
untouched.

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_pam_any_width_cpu.py, tests/test_pam_wide_arena_gpu.py); the latter runs them through the harness."""
import torch

import arena_cases
from arena_cases import TOL, _gen, _rn, row, sdpa64

IDS = []
WIDTHS = (320, 640)
B, NQ, NKV, GAP = 2, 70, 35, 12
WIDE_TAG = "sdpa_wide_kernel<d=%d,prec %d>"


def _register():
    for width in WIDTHS:
        def make(seed, width=width):
            g = _gen(seed)
            return dict(q=_rn(g, B, NQ, width), kv=_rn(g, B, NKV, 2 * width))

        def ref(dd, width=width):
            q, k, v = dd["q"].double()[:, None], dd["kv"].double()[:, None, :, :width], dd["kv"].double()[:, None, :, width:]
            out = torch.zeros(B, NQ, width + GAP, dtype=torch.float64)
            out[:, :, :width] = sdpa64(q, k, v, width ** -0.5)[:, 0]
            return out

        def run(F, dd, p, width=width):
            buf = F.torch.zeros(B, NQ, width + GAP, dtype=torch.float32, device=dd["q"].device)
            F.sdpa_general(dd["q"], dd["kv"][..., :width], dd["kv"][..., width:], 1, width ** -0.5, precision=p, out=buf[:, :, :width])
            return buf

        for p in (0, 1, 2):
            IDS.append(f"sdpa_wide_{width}_p{p}")
            row(id=IDS[-1], entries=("mi355_sdpa_general_fwd",), prec=p, tol=TOL[p], tags=(WIDE_TAG % (width, p),), make=make, ref=ref,
                run=lambda F, dd, p=p, run=run: run(F, dd, p))
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
