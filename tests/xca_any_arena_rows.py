"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for the run-time-width XCiT kernels:
mi355_xca_fwd (precision 0 / 1 / 2) and mi355_xca16_fwd (1 / 2, from 16-bit and from fp32 qkv) on xca_any_kernel at head widths 5
(unaligned heads, element-wise accesses, two token chunks with the last partial) and 72 (three row blocks, the last of 8 live rows),
and mi355_class_attn_fwd on class_attn_any_kernel at width 5.  A head that starts or ends inside a 16-byte unit must write nothing
beside its own columns: the poisoned arena shows it.

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_xca_any_cpu.py, tests/test_xca_any_arena_gpu.py); the latter runs them through the harness."""
import torch

import arena_cases
import xca_any_cases as X
from arena_cases import TOL, _gen, _rn, dt16, row

IDS = []
XCA_TAG = "xca_any_kernel<d=%d"
CLS_TAG = "class_attn_any_kernel<d=%d"


def _xca_ref(dd, h):
    from test_ops_gpu import _xca_core_ref
    return _xca_core_ref(dd["qkv"].double(), dd["t"].double(), h)


def _register():
    for B, N, h, d in X.ARENA_XCA:
        def make(seed, s=(B, N, h, d)):
            B_, N_, h_, d_ = s
            g = _gen(seed)
            return dict(qkv=_rn(g, B_, N_, 3 * h_ * d_), t=torch.rand(h_, generator=g) + 0.5)

        def make16(seed, p, make=make):
            dd = make(seed)
            return dict(dd, qkv=dd["qkv"].to(dt16(p)))
        sid = f"{B}x{N}x{h}x{d}"
        for p in (0, 1, 2):
            IDS.append(f"xca_any_{sid}_p{p}")
            row(id=IDS[-1], entries=("mi355_xca_fwd",), prec=p, tol=TOL[p], tags=(XCA_TAG % d + ">",), make=make, ref=lambda dd, h=h: _xca_ref(dd, h),
                run=lambda F, dd, h=h, p=p: F.xca_core(dd["qkv"], dd["t"], h, precision=p))
        for p in (1, 2):
            IDS.append(f"xca16_any_{sid}_p{p}")
            row(id=IDS[-1], entries=("mi355_xca16_fwd",), prec=p, tol=TOL[p], tags=(XCA_TAG % d + ",in16,out16>",), ref=lambda dd, h=h: _xca_ref(dd, h),
                make=lambda seed, p=p, make16=make16: make16(seed, p),
                run=lambda F, dd, h=h, p=p: F.xca_core(dd["qkv"], dd["t"], h, precision=p, out16=True))
            IDS.append(f"xca16_any_from32_{sid}_p{p}")
            row(id=IDS[-1], entries=("mi355_xca16_fwd",), prec=p, tol=TOL[p], tags=(XCA_TAG % d + ",out16>",), make=make, ref=lambda dd, h=h: _xca_ref(dd, h),
                run=lambda F, dd, h=h, p=p: F.xca_core(dd["qkv"], dd["t"], h, precision=p, out16=True))
    for B, N, h, d in X.ARENA_CLASS_ATTN:
        C = h * d

        def make(seed, s=(B, N, 3 * C)):
            return dict(qkv=_rn(_gen(seed), *s))

        def ref(dd, B=B, N=N, h=h, d=d, C=C):
            qkv = dd["qkv"].double()
            q = qkv[:, 0, :C].reshape(B, h, 1, d)
            k = qkv[:, :, C:2 * C].reshape(B, N, h, d).permute(0, 2, 1, 3)
            v = qkv[:, :, 2 * C:].reshape(B, N, h, d).permute(0, 2, 1, 3)
            a = torch.softmax((q * k).sum(-1) * d ** -0.5, dim=-1)
            return (a.unsqueeze(2) @ v).transpose(1, 2).reshape(B, C)

        def run(F, dd, N=N, h=h, d=d, C=C):
            t = dd["qkv"]
            return F.class_attention(t[:, 0, :C], t[:, :, C:2 * C], t[:, :, 2 * C:], h, d ** -0.5, N, N * 3 * C, 3 * C)
        IDS.append(f"class_attn_any_{B}x{N}x{h}x{d}")
        row(id=IDS[-1], entries=("mi355_class_attn_fwd",), prec=0, tol=TOL[0], tags=(CLS_TAG % d,), make=make, ref=ref, run=run)
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
