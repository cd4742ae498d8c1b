"""GPU tests (-m gpu): DoubleAttention and CAM on maps whose H*W or channel counts are no multiples of 4 -- the ragged routes behind
mi355_double_attn_fwd, mi355_double_attn16_fwd and mi355_cam_fwd (csrc/ragged_maps.hip, csrc/double_attn.hip, csrc/sk_dual.hip).

Reference: the fp64 oracle (oracle.chan_attn.double_attention_forward, oracle.axis_attn.cam_forward) through conftest.assert_parity at the
project's bars TOL = {0: 5e-5, 1: 1e-3, 2: 1.2e-2} (tests/arena_cases.py).  Shapes, inputs and CAM's input scale: tests/ragged_cases.py;
tests/test_ragged_maps_cpu.py pins the oracle on these shapes and shows that CAM's scale leaves a factor ten to the strict bar."""
import ctypes
import warnings

import pytest
import torch

import ragged_cases as R
from conftest import assert_parity, max_abs_ratio, rel_fro
from io16_common import DTYPES, IO, _status

pytestmark = pytest.mark.gpu

RAGGED_TAGS = ("ragged_stage_kernel", "ragged_softmax_rows_kernel", "da_pack_ragged_kernel", "da_round16_ragged_kernel")


def _cam(precision=None):
    from mi355attn.modules import CAM
    m = CAM().eval()
    with torch.no_grad():
        m.beta.fill_(R.CAM_BETA)
    m.precision = precision
    return m


def _trace(fn):
    import mi355attn
    out = []
    with torch.no_grad():
        rows = mi355attn.kernel_trace(lambda: out.append(fn()))
    return out[0], sorted((tag, count) for tag, count, *_ in rows)


# ---- parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("case", R.DA, ids=R.da_id)
def test_double_attention_parity_against_fp64(case, prec):
    m = R.da_module(case, precision=prec).cuda()
    ref = R.da_ref(case)
    with torch.no_grad():
        y = m(R.da_input(case).cuda())                                 # Mi355Error without the ragged route
    assert y.dtype == torch.float32
    y = y.cpu()
    print(f"[ragged] DA {R.da_id(case)} p{prec}: rel_fro {rel_fro(y, ref):.2e} max-abs ratio {max_abs_ratio(y, ref):.2e} (bar {R.TOL[prec]:g})")
    assert_parity(y, ref, R.TOL[prec], f"DoubleAttention {R.da_id(case)} precision {prec}")
    _status()


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("shape", R.CAM, ids=R.cam_id)
def test_cam_parity_against_fp64(shape, prec):
    m = _cam(prec).cuda()
    ref = R.cam_ref(shape)
    with torch.no_grad():
        y = m(R.cam_input(shape).cuda()).cpu()                         # Mi355Error without the ragged route
    print(f"[ragged] CAM {R.cam_id(shape)} p{prec}: rel_fro {rel_fro(y, ref):.2e} max-abs ratio {max_abs_ratio(y, ref):.2e} (bar {R.TOL[prec]:g})")
    assert_parity(y, ref, R.TOL[prec], f"CAM {R.cam_id(shape)} precision {prec}")
    _status()


# ---- 16-bit I/O -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", R.DA, ids=R.da_id)
def test_double_attention_16bit_io_is_the_fp32_entry_rounded_once(case, dtype):
    """The header's contract of the 16-bit entry on the new route: y = mi355_double_attn_fwd(precision = io) on the widened x, rounded
    once -- element for element.  Precision 0 on an fp16 x is the wrapper's widen, run, round."""
    m = R.da_module(case).cuda()
    m32 = R.da_module(case, precision=IO[dtype]).cuda()               # the same seed: the same weights
    x16 = R.da_input(case).to(dtype).cuda()
    with torch.no_grad():
        y16 = m(x16)
        want = m32(x16.float()).to(dtype)
    assert y16.dtype == dtype and tuple(y16.shape) == case[0]
    assert torch.equal(y16, want), f"{int((y16 != want).sum())} of {y16.numel()} elements differ"
    assert_parity(y16.float().cpu(), R.da_ref(case, x16), R.TOL[IO[dtype]], f"DoubleAttention {R.da_id(case)} {dtype}")
    if dtype == torch.float16:
        m0 = R.da_module(case, precision=0).cuda()
        with torch.no_grad():
            assert torch.equal(m0(x16), m0(x16.float()).half())
    _status()


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------
BAND = 64                                                              # elements on each side: 256 / 128 bytes, so the views are 16-byte aligned


def _banded(t, poison):
    """t copied into the middle of a flat buffer filled with `poison`: (buffer, view)."""
    buf = torch.full((t.numel() + 2 * BAND,), poison, dtype=t.dtype, device="cuda")
    view = buf[BAND:BAND + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _bands(buf):
    return torch.cat([buf[:BAND], buf[-BAND:]]).view(torch.uint8).clone()


GUARD = [R.DA[3], R.DA[4]]                                             # (2, 30, 9, 7) c 10/6 and (1, 5, 3, 3) c 3/1


@pytest.mark.parametrize("io", [0, 1, 2], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("case", GUARD, ids=R.da_id)
def test_double_attention_guard_bands(case, io):
    """x and y are views inside larger poisoned buffers: what lies around x never reaches the result (a 16-byte load past a row end or
    an image end would bring it in), and nothing is written around y (a 16-byte store past a row end would leave the tensor there)."""
    from mi355attn import _ffi
    from mi355attn import functional as F
    dtype = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[io]
    prec = io if io else 1
    m = R.da_module(case, precision=prec).cuda()
    p = [m.convA.weight, m.convA.bias, m.convB.weight, m.convB.bias, m.convV.weight, m.convV.bias, m.proj.weight, m.proj.bias]
    x = R.da_input(case).to(dtype)
    (B, C, H, W), cm, cn = case
    with torch.no_grad():
        _, xa = _banded(x, 3.0e4)
        _, xb = _banded(x, -7.0)
        ya = F.double_attention_forward(xa, *p, precision=prec)
        yb = F.double_attention_forward(xb, *p, precision=prec)
        assert torch.equal(ya, yb) and torch.isfinite(ya).all()
        # y through the C entry
        ybuf, yv = _banded(torch.zeros(case[0], dtype=dtype), 123.0)
        before = _bands(ybuf)
        lib = _ffi.lib()
        flat = [t.detach().reshape(t.shape[0], -1).contiguous() for t in p]
        if io:
            n = lib.mi355_double_attn16_ws_bytes(B, C, cm, cn, H, W, io)
            entry, slot = lib.mi355_double_attn16_fwd, io
        else:
            n = lib.mi355_double_attn_ws_bytes(B, C, cm, cn, H, W, prec)
            entry, slot = lib.mi355_double_attn_fwd, prec
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        rc = entry(_ffi.dptr(xa), *[_ffi.dptr(t) for t in flat], _ffi.dptr(yv), B, C, cm, cn, H, W, slot, _ffi.dptr(ws), ws.numel(),
                   _ffi.stream_ptr(yv.device))
        assert rc == 0, lib.mi355_last_error().decode()
        torch.cuda.synchronize()
        assert torch.equal(_bands(ybuf), before), "bytes around y were written"
        assert torch.equal(yv, ya)
    _status()


@pytest.mark.parametrize("shape", [R.CAM[1], R.CAM[2]], ids=R.cam_id)
def test_cam_guard_bands(shape):
    from mi355attn import _ffi
    from mi355attn import functional as F
    beta = torch.tensor([R.CAM_BETA], device="cuda")
    x = R.cam_input(shape)
    B, C, H, W = shape
    _, xa = _banded(x, 3.0e4)
    _, xb = _banded(x, -7.0)
    ya = F.cam_forward(xa, beta, 1)
    yb = F.cam_forward(xb, beta, 1)
    assert torch.equal(ya, yb) and torch.isfinite(ya).all()
    ybuf, yv = _banded(torch.zeros(shape), 123.0)
    before = _bands(ybuf)
    lib = _ffi.lib()
    ws = torch.empty(lib.mi355_cam_ws_bytes(B, C, H, W), dtype=torch.uint8, device="cuda")
    rc = lib.mi355_cam_fwd(_ffi.dptr(xa), _ffi.dptr(beta), _ffi.dptr(yv), B, C, H, W, 1, _ffi.dptr(ws), ws.numel(), _ffi.stream_ptr(yv.device))
    assert rc == 0, lib.mi355_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(_bands(ybuf), before), "bytes around y were written"
    assert torch.equal(yv, ya)
    _status()


# ---- nothing moved for the shapes the entries took before ----------------------------------------------------------------------------------
# kernel_trace tags (sorted, with counts) recorded before the ragged route existed.  The fused routes of the fp32 entry open no trace scope.
def _da_general(p, M3, HW, C, cm, cn):
    return [(f"gemm_kernel<prec {p},b0,a0> batch=2 M={cm} N={cn} K={HW}", 1), (f"gemm_kernel<prec {p},b1,a0> batch=2 M={C} N={HW} K={cn}", 1),
            (f"gemm_kernel<prec {p},b1,a0> batch=2 M={C} N={cn} K={cm}", 1), (f"gemm_kernel<prec {p},b1,a0> batch=2 M={M3} N={HW} K={C}", 1)]


BEFORE_DA = {
    ((2, 64, 32, 32), 32, 0, torch.float32): _da_general(0, 96, 1024, 64, 32, 32),
    ((2, 64, 32, 32), 32, 1, torch.float32): [],
    ((2, 64, 32, 32), 32, 2, torch.float32): [],
    ((2, 64, 32, 32), 32, 1, torch.float16): [("da_small_kernel<io16> io=1 B=2 HW=1024", 1)],
    ((2, 64, 32, 32), 32, 2, torch.bfloat16): [("da_small_kernel<io16> io=2 B=2 HW=1024", 1)],
    ((2, 48, 6, 6), 12, 0, torch.float32): _da_general(0, 36, 36, 48, 12, 12),
    ((2, 48, 6, 6), 12, 1, torch.float32): _da_general(1, 36, 36, 48, 12, 12),
    ((2, 48, 6, 6), 12, 2, torch.float32): _da_general(2, 36, 36, 48, 12, 12),
    ((2, 48, 6, 6), 12, 1, torch.float16): [("da_round16_kernel io=1 n=3456", 1), ("da_widen_kernel io=1 n=3456", 1)] + _da_general(1, 36, 36, 48, 12, 12),
    ((2, 48, 6, 6), 12, 2, torch.bfloat16): [("da_round16_kernel io=2 n=3456", 1), ("da_widen_kernel io=2 n=3456", 1)] + _da_general(2, 36, 36, 48, 12, 12),
}
BEFORE_CAM = {p: [("gemm_kernel<prec 0,b0,a0> batch=2 M=64 N=64 K=1024", 1), (f"gemm_kernel<prec {p},b1,a0> batch=2 M=64 N=1024 K=64", 1)]
              for p in (0, 1, 2)}


def test_aligned_shapes_keep_their_kernels():
    for (shape, c, prec, dtype), want in BEFORE_DA.items():
        case = (shape, c, c)
        m = R.da_module(case, precision=prec).cuda()
        x = R.da_input(case).to(dtype).cuda()
        y, tags = _trace(lambda: m(x))
        assert tags == sorted(want), (shape, c, prec, dtype, tags)
        assert not any(t.startswith(RAGGED_TAGS) for t, _ in tags)
        with torch.no_grad():
            assert torch.equal(m(x), y)
    for prec, want in BEFORE_CAM.items():
        m = _cam(prec).cuda()
        g = torch.Generator(device="cpu").manual_seed(4321)
        x = (R.CAM_SCALE * torch.randn(2, 64, 32, 32, generator=g) / 32).cuda()
        y, tags = _trace(lambda: m(x))
        assert tags == sorted(want), (prec, tags)
        with torch.no_grad():
            assert torch.equal(m(x), y)
    _status()


def test_ragged_shapes_take_the_new_kernels():
    """The other half: a ragged shape runs the staging kernel once, the masked softmax once, and none of the fused routes' kernels --
    (3, 128, 13, 13) with c 128 has the two-pass route's channel counts and (2, 64, 7, 7) with c 32 the one-kernel route's."""
    for case in (R.DA[0], R.DA[1]):
        for dtype, prec in ((torch.float32, 1), (torch.float16, None)):
            m = R.da_module(case, precision=prec).cuda()
            x = R.da_input(case).to(dtype).cuda()
            _, tags = _trace(lambda: m(x))
            names = [t for t, _ in tags]
            assert all(n == 1 for _, n in tags), tags
            for k in RAGGED_TAGS[:3]:
                assert sum(t.startswith(k) for t in names) == 1, (case, k, tags)
            assert sum(t.startswith("da_round16_ragged_kernel") for t in names) == (dtype == torch.float16), tags
            assert sum(t.startswith("gemm_kernel<prec 1,") for t in names) == 4, tags
            assert not any(t.startswith(("da_small", "da_pass", "da_prep", "da_widen", "nchw_to_tokens16")) for t in names), tags
    _, tags = _trace(lambda: _cam(2).cuda()(R.cam_input(R.CAM[0]).cuda()))
    names = [t for t, _ in tags]
    assert sum(t.startswith("ragged_stage_kernel") for t in names) == 1 and sum(t.startswith("ragged_softmax_rows_kernel") for t in names) == 1
    assert "gemm_kernel<prec 0,b0,a0> batch=2 M=64 N=64 K=52" in names and "gemm_kernel<prec 2,b1,a0> batch=2 M=64 N=49 K=64" in names, tags
    _status()


# ---- range guard ----------------------------------------------------------------------------------------------------------------------
def test_range_guard_on_the_ragged_route():
    """x at 1e5: x itself and A = WA x + bA leave the fp16 range (the staging kernel reports code 8, the engine code 6).  One warning, and
    the forward returns what the strict route returns.  An ordinary x raises nothing: the zero pads never report."""
    case = R.DA[3]
    m1, m0 = R.da_module(case, precision=1).cuda(), R.da_module(case, precision=0).cuda()
    x = R.da_input(case).cuda()
    with warnings.catch_warnings(record=True) as rec, torch.no_grad():
        warnings.simplefilter("always")
        y = m1(x)
        torch.cuda.synchronize()
    assert not [w for w in rec if "overflowed" in str(w.message)], [str(w.message) for w in rec]
    assert_parity(y.cpu(), R.da_ref(case), R.TOL[1], "ordinary x")
    _status()
    big = x * 1e5
    with warnings.catch_warnings(record=True) as rec, torch.no_grad():
        warnings.simplefilter("always")
        y = m1(big)
        torch.cuda.synchronize()
    fired = [w for w in rec if issubclass(w.category, RuntimeWarning) and "overflowed" in str(w.message)]
    assert len(fired) == 1, [str(w.message) for w in rec]
    with torch.no_grad():
        strict = m0(big)
    assert torch.isfinite(y).all() and torch.equal(y, strict)
    _status()


# ---- graph capture --------------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One ragged DoubleAttention and one ragged CAM forward captured on a single stream and replayed twice equal the eager result."""
    case, shape = R.DA[3], R.CAM[1]
    da, cam = R.da_module(case, precision=1).cuda(), _cam(1).cuda()
    xd, xc = R.da_input(case).cuda(), R.cam_input(shape).cuda()
    with torch.no_grad():
        want = (da(xd).clone(), cam(xc).clone())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        da(xd), cam(xc)                                                # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = (da(xd), cam(xc))
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]), f"replay {rep} differs from the eager result"
        out[0].zero_(), out[1].zero_()
    _status()
