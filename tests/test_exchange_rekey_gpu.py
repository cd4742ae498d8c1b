"""GPU test (-m gpu): one caller-owned workspace whose layout changes between calls, for the six users of the granule exchange
(csrc/api.hip xch_begin / xch_zero / xch_launched): mi355_se_fwd, mi355_se16_fwd, mi355_cbam_fwd, mi355_cbam16_fwd, mi355_gct_fwd and
mi355_gct16_fwd, called through the C ABI with "ws_persistent" on.

Each user runs shape A, shape B and shape A again on ONE buffer that is sized for the larger shape and starts out as 0xFF bytes: an
exchange area is zeroed when its history is unknown (first use, another layout key) and not otherwise, and a launch's granules are told
from an earlier launch's by the epoch in the area itself.  Every result must equal, bit for bit, the same call on a fresh zeroed buffer,
and no poll may have run out.  The shapes are the smallest that still take the single-read kernels: the 16-bit entries show it in the
kernel trace, the fp32 entries are compared with their multi-pass form at the bounds of
tests/test_chan_attn_gpu.py (1e-6 SE, 2e-6 CBAM and GCT)."""
import ctypes

import pytest
import torch

from conftest import assert_parity

pytestmark = pytest.mark.gpu

SE_SHAPES = ((2, 16, 8, 8), (3, 32, 4, 8))
CBAM_SHAPES = ((2, 16, 8, 8), (2, 32, 16, 16))       # one band per image; two bands at segment width 32
TORCH_TYPE = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class _User:
    """One entry pair: `io` 0 calls the fp32 entry, 1 / 2 the 16-bit one; params(C) are fp32 device tensors."""

    def __init__(self, kind, io):
        self.kind, self.io = kind, io
        self.shapes = CBAM_SHAPES if kind == "cbam" else SE_SHAPES
        self.off_option = {"se": "se_single", "cbam": "cbam_single", "gct": "zoo_single"}[kind]
        self.tol = 1e-6 if kind == "se" else 2e-6
        self.tag = {"se": "se16_single_kernel", "cbam": "cbam16_single_kernel", "gct": "stat16_single_kernel"}[kind]

    def params(self, C):
        g = torch.Generator().manual_seed(100 + C)
        r = lambda *s: (torch.randn(*s, generator=g) * 0.5).cuda()
        if self.kind == "se":
            return [r(C // 4, C), r(C, C // 4)]
        if self.kind == "cbam":
            return [r(C // 4, C), r(C, C // 4), r(1, 2, 7, 7)]
        return [1.0 + r(C), r(C), r(C)]                                  # alpha, gamma, beta

    def ws_bytes(self, lib, shape):
        B, C, H, W = shape
        if self.kind == "se":
            return lib.mi355_se_workspace_bytes(B, C, H, W)
        if self.kind == "cbam":
            return (lib.mi355_cbam16_workspace_bytes if self.io else lib.mi355_cbam_workspace_bytes)(B, C, H, W)
        return lib.mi355_chan_stat_workspace_bytes(B, C)

    def call(self, lib, x, par, ws):
        from mi355attn._ffi import stream_ptr
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        tail = (_p(ws), ws.numel(), stream_ptr(x.device))
        io = (self.io,) if self.io else ()
        if self.kind == "se":
            fn = lib.mi355_se16_fwd if self.io else lib.mi355_se_fwd
            rc = fn(_p(x), _p(par[0]), _p(par[1]), _p(y), B, C, C // 4, H, W, *io, *tail)
        elif self.kind == "cbam":
            fn = lib.mi355_cbam16_fwd if self.io else lib.mi355_cbam_fwd
            rc = fn(_p(x), _p(par[0]), _p(par[1]), _p(par[2]), _p(y), B, C, C // 4, 7, H, W, 0, *io, *tail)
        else:
            fn = lib.mi355_gct16_fwd if self.io else lib.mi355_gct_fwd
            rc = fn(_p(x), _p(par[0]), _p(par[1]), _p(par[2]), _p(y), B, C, H, W, 1e-5, 0, 0, *io, *tail)
        assert rc == 0, (self.kind, self.io, tuple(x.shape), lib.mi355_last_error())
        return y


@pytest.mark.parametrize("io", [0, 1, 2], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("kind", ["se", "cbam", "gct"])
def test_one_workspace_changing_layout(kind, io):
    import mi355attn
    from mi355attn._ffi import lib as _lib
    lib = _lib()
    u = _User(kind, io)
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(*s, generator=g).to(TORCH_TYPE[io]).cuda() for s in u.shapes]
    pars = [u.params(s[1]) for s in u.shapes]
    sizes = [u.ws_bytes(lib, s) for s in u.shapes]
    shared = torch.full((max(sizes),), 0xFF, dtype=torch.uint8, device="cuda")
    fresh = []
    try:
        with mi355attn.options(ws_persistent=1):
            ref = []
            for x, par, n in zip(xs, pars, sizes):
                fresh.append(torch.zeros(n, dtype=torch.uint8, device="cuda"))
                if io:
                    rows = mi355attn.kernel_trace(lambda: ref.append(u.call(lib, x, par, fresh[-1])))
                    assert any(r[0].startswith(u.tag) for r in rows), [r[0] for r in rows]
                else:
                    ref.append(u.call(lib, x, par, fresh[-1]))
                    with mi355attn.options(**{u.off_option: 0}):
                        fresh.append(torch.zeros(n, dtype=torch.uint8, device="cuda"))
                        multi = u.call(lib, x, par, fresh[-1])
                    assert_parity(ref[-1].cpu(), multi.cpu(), u.tol, f"{kind} {tuple(x.shape)}: single read vs multi-pass")
            for i in (0, 1, 0):
                y = u.call(lib, xs[i], pars[i], shared)
                assert torch.equal(y, ref[i]), f"{kind} io={io}: shape {u.shapes[i]} on the shared workspace differs from a fresh one"
            torch.cuda.synchronize()
            assert lib.mi355_sync_status() == 0, lib.mi355_last_error()
    finally:
        torch.cuda.synchronize()
        for t in fresh + [shared]:                                       # before the buffers are freed (include/mi355attn.h, "ws_persistent")
            lib.mi355_workspace_forget(_p(t), t.numel())
