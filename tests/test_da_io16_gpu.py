"""GPU tests (-m gpu): DoubleAttention on fp16 and bf16 activations (mi355_double_attn16_fwd: the 16-bit-I/O instantiations of
csrc/double_attn_small.hip and csrc/double_attn_fused.hip, and the general route of csrc/double_attn.hip).

Reference: oracle.chan_attn.double_attention_forward in fp64 on x16.double() and the fp32 parameters.  The bars are the ones the suite
already uses for this module at these operand formats (TOL of tests/test_ops_gpu.py): conftest.assert_parity at 1e-3 for fp16 and
1.2e-2 for bf16, no element excluded.  tests/test_da_io16_cpu.py shows that an fp64 evaluation with the kernels' 16-bit rounding points
(weights, A, E, V, G, M', the output) stays 2-3x inside them.

From the operand tile onwards the 16-bit-I/O kernels keep the tile size, tile order and wave ownership of the fp32-I/O kernels, and a
16-bit x enters the MFMAs unrounded, so m(x16) is DoubleAttention(precision = io)(x16.float()) rounded once: the two differ by at most
the rounding of nearly equal fp32 values, norm-wise well under half a unit u = 2^-11 (fp16) / 2^-8 (bf16)."""
import copy
import warnings

import pytest
import torch

import oracle.chan_attn as OC
from conftest import assert_parity, no_range_fallback, rel_fro
from io16_common import DTYPES, IO, U, _input, _status

pytestmark = pytest.mark.gpu

TOL = {torch.float16: 1e-3, torch.bfloat16: 1.2e-2}

# (shape, c_m, c_n)
SMALL = [((2, 64, 32, 32), 32, 32),
         ((3, 64, 4, 8), 32, 32),           # one group: seven idle waves
         ((1, 64, 8, 12), 32, 32)]
TWO_PASS = [((2, 256, 8, 8), 128, 128),
            ((1, 128, 2, 2), 128, 128),
            ((2, 256, 14, 14), 128, 128),   # rows 8-byte aligned only
            ((2, 256, 6, 10), 128, 128),    # ragged last tile
            ((5, 128, 28, 28), 128, 128),
            ((3, 256, 56, 56), 128, 128),   # several ranges per image
            ((300, 128, 6, 6), 128, 128)]   # one range per image: pass 1 combines
GENERAL = [((2, 64, 10, 10), 32, 32), ((2, 48, 6, 6), 12, 12), ((2, 128, 8, 8), 64, 32)]
PASS_TAGS = ("da_prep_kernel<io16>", "da_pass1_kernel<io16>", "da_combine_kernel<io16>", "da_pass2_kernel<io16>")
NEW_TAGS = ("io16", "da_widen_kernel", "da_round16_kernel")


def _sid(case):
    return "x".join(map(str, case[0])) + f"_c{case[1]}_{case[2]}"


def _module(C, cm, cn, precision=None, seed=1234):
    from mi355attn.modules import DoubleAttention
    torch.manual_seed(seed)
    return DoubleAttention(C, cm, cn, precision=precision).eval()     # default Conv2d init


def _params(m):
    return [t.detach().cpu().float() for t in (m.convA.weight, m.convA.bias, m.convB.weight, m.convB.bias, m.convV.weight, m.convV.bias,
                                               m.proj.weight, m.proj.bias)]


def _ref(x16, m):
    return OC.double_attention_forward(x16.double().cpu(), *_params(m), dtype=torch.float64)


def _trace(fn):
    import mi355attn
    out = []
    with torch.no_grad():
        rows = mi355attn.kernel_trace(lambda: out.append(fn()))
    return out[0], {tag: count for tag, count, *_ in rows}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", SMALL + TWO_PASS + GENERAL, ids=_sid)
def test_parity_against_fp64(case, dtype):
    shape, cm, cn = case
    m = _module(shape[1], cm, cn)
    x16 = _input(shape, dtype)
    ref = _ref(x16, m)
    with torch.no_grad():
        y = m.cuda()(x16.cuda())                                       # raises TypeError without the feature
    assert y.dtype == dtype and tuple(y.shape) == shape
    y = y.float().cpu()
    print(f"[da16] {_sid(case)} {dtype}: rel_fro {rel_fro(y, ref):.2e} max-abs ratio {float((y.double() - ref).abs().max() / ref.abs().max()):.2e}"
          f" (bar {TOL[dtype]:g})")
    assert_parity(y, ref, TOL[dtype], f"DoubleAttention {_sid(case)} {dtype}")
    _status()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_routes(dtype):
    """What kernel_trace shows: one entry per traced launch.  Every launch of the 16-bit entry's own kernels opens a trace scope
    (da_small / da_prep / da_pass1 / da_combine / da_pass2 with the <io16> mark, da_widen, da_round16, the 16-bit transpose), and so do
    cast16 and the GEMMs of the general route; the fp32 entry's fused launches open none, as before this path existed.  So "exactly
    one kernel" and "only prep / pass 1 / (combine) / pass 2" count the traced launches of the 16-bit entry, and the fp32 half checks
    that an fp32 x never reaches a kernel of the new entry -- not that the fp32 trace is complete."""
    x32_seen = []
    for cases, kind in ((SMALL, "small"), (TWO_PASS, "two-pass"), (GENERAL, "general")):
        for case in cases:
            shape, cm, cn = case
            m = _module(shape[1], cm, cn).cuda()
            x16 = _input(shape, dtype).cuda()
            y, tags = _trace(lambda: m(x16))
            assert y.dtype == dtype
            if kind == "small":
                assert sum(tags.values()) == 1 and next(iter(tags)).startswith("da_small_kernel<io16>"), (case, tags)
            elif kind == "two-pass":
                assert all(t.startswith(PASS_TAGS) and n == 1 for t, n in tags.items()), (case, tags)
                for k in (PASS_TAGS[0], PASS_TAGS[1], PASS_TAGS[3]):
                    assert any(t.startswith(k) for t in tags), (case, k, tags)
                assert not any("cast16" in t or "widen" in t or "round16" in t for t in tags), (case, tags)
            else:
                assert any(t.startswith("da_round16_kernel") for t in tags), (case, tags)
                first = "da_widen_kernel" if shape[1] % 64 else "nchw_to_tokens16_kernel<io16>"
                assert any(t.startswith(first) for t in tags), (case, first, tags)
                assert not any(t.startswith(("da_small_kernel", "da_pass")) for t in tags), (case, tags)
            # every launch of the 16-bit entry is told apart from the fp32 entry's, which shows none of the new tags
            y32, tags32 = _trace(lambda: m(x16.float()))
            assert y32.dtype == torch.float32 and not any(k in t for t in tags32 for k in NEW_TAGS), (case, tags32)
            if kind != "general":
                assert all("io16" in t for t in tags), (case, tags)
            x32_seen.append(case)
    assert len(x32_seen) == len(SMALL + TWO_PASS + GENERAL)
    _status()


SAME = SMALL + TWO_PASS + GENERAL


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", SAME, ids=_sid)
def test_same_arithmetic_as_the_fp32_kernels(case, dtype):
    shape, cm, cn = case
    m = _module(shape[1], cm, cn).cuda()
    m32 = _module(shape[1], cm, cn, precision=IO[dtype]).cuda()        # the same seed: the same weights
    x16 = _input(shape, dtype).cuda()
    with torch.no_grad():
        y16 = m(x16)
        r = m32(x16.float()).to(dtype)
    differ = int((y16.float() != r.float()).sum())
    rf = rel_fro(y16.float(), r.float())
    print(f"[da16] {_sid(case)} {dtype}: {differ} of {y16.numel()} elements differ from the rounded fp32-I/O result, rel_fro {rf:.2e}")
    assert rf <= U[dtype], (case, dtype, rf, differ)
    _status()


@pytest.mark.parametrize("case", [((2, 64, 8, 8), 32, 32), ((2, 128, 8, 8), 128, 128)], ids=_sid)
def test_range_fallback(case):
    import mi355attn
    from mi355attn import functional as F
    shape, cm, cn = case
    m = _module(shape[1], cm, cn)
    with torch.no_grad():
        m.convA.weight.mul_(1e5)
        m.proj.weight.mul_(1e-5)
    for dtype in DTYPES:
        x16 = _input(shape, dtype)
        ref = _ref(x16, m)
        md = copy.deepcopy(m).cuda()
        with warnings.catch_warnings(record=True) as rec, torch.no_grad():
            warnings.simplefilter("always")
            y = md(x16.cuda())
            torch.cuda.synchronize()
        fired = [w for w in rec if issubclass(w.category, RuntimeWarning) and "overflowed" in str(w.message)]
        assert len(fired) == (1 if dtype == torch.float16 else 0), [str(w.message) for w in rec]
        assert y.dtype == dtype and torch.isfinite(y).all()
        assert_parity(y.float().cpu(), ref, TOL[dtype], f"range fallback {_sid(case)} {dtype}")
        _status()
    # the round-3 contract: no wait, no re-run -- the report surfaces on the next status read, as for fp32
    md = copy.deepcopy(m).cuda()
    x16 = _input(shape, torch.float16).cuda()
    with no_range_fallback(), torch.no_grad():
        md(x16)
        with pytest.raises(mi355attn.Mi355RangeError):
            F.range_status(wait=True)
    _status()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_parameters_off_16_byte_alignment_take_the_general_route(dtype):
    """Parameters that are views into a flat buffer at a 4-byte offset: the one-kernel path wants 16-byte aligned weights, so the call
    takes the general route with the workspace mi355_double_attn16_ws_bytes names -- served, as mi355_double_attn_fwd serves it."""
    case = SMALL[0]
    shape, cm, cn = case
    m = _module(shape[1], cm, cn)
    x16 = _input(shape, dtype)
    ref = _ref(x16, m)
    m = m.cuda()
    keep = []
    for p in m.parameters():
        flat = torch.empty(p.numel() + 1, device="cuda")
        view = flat[1:].view_as(p)
        view.copy_(p.data)
        p.data = view
        keep.append(flat)
        assert p.data_ptr() % 16 == 4
    y, tags = _trace(lambda: m(x16.cuda()))
    assert y.dtype == dtype and any(t.startswith("da_round16_kernel") for t in tags) and not any(t.startswith("da_small") for t in tags), tags
    assert_parity(y.float().cpu(), ref, TOL[dtype], f"unaligned parameters {dtype}")
    with torch.no_grad():
        y32 = m(x16.cuda().float())                                    # the fp32 entry serves the same module
    assert_parity(y32.cpu(), ref, TOL[dtype], f"unaligned parameters, fp32 x, {dtype}")
    _status()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_nan_stays_in_its_image(dtype):
    shape, cm, cn = TWO_PASS[0]
    m = _module(shape[1], cm, cn).cuda()
    x = _input(shape, dtype).cuda()
    with torch.no_grad():
        clean = m(x).clone()
        x[1, 3, 2, 5] = float("nan")
        y = m(x)
    torch.cuda.synchronize()
    assert torch.equal(y[0], clean[0]) and bool(torch.isnan(y[1]).any())
    _status()                                                          # a NaN is not a saturation: nothing reported, no re-run


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_plumbing(dtype):
    shape, cm, cn = SMALL[0]
    B, C, H, W = shape
    m16 = _module(C, cm, cn).cuda().to(dtype)                          # module.half() / .bfloat16()
    m32 = _module(C, cm, cn).cuda()
    with torch.no_grad():
        for p16, p32 in zip(m16.parameters(), m32.parameters()):
            p32.copy_(p16.float())                                     # fp32 parameters of the same values
    x = _input(shape, dtype).cuda()
    with torch.no_grad():
        y = m32(x)
        assert y.dtype == dtype and torch.equal(m16(x), y)
        m16.convA.weight.mul_(2.0)                                     # an in-place update is followed
        m32.convA.weight.copy_(m16.convA.weight.float())
        y2 = m32(x)
        assert torch.equal(m16(x), y2) and not torch.equal(y2, y)
        # non-contiguous inputs equal their .contiguous() result
        assert torch.equal(m32(x.to(memory_format=torch.channels_last)), y2)
        wide = _input((B, C, H, W + 8), dtype, seed=7).cuda()
        sl = wide[..., 3:3 + W]
        assert not sl.is_contiguous() and torch.equal(m32(sl), m32(sl.contiguous()))
    # behind an autocast convolution
    torch.manual_seed(5)
    from mi355attn.modules import DoubleAttention
    net = torch.nn.Sequential(torch.nn.Conv2d(3, C, 3, padding=1), DoubleAttention(C, cm, cn)).eval().cuda()
    img = torch.randn(2, 3, 32, 32, device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype):
        out = net(img)
    assert out.dtype == dtype and tuple(out.shape) == (2, C, 32, 32) and torch.isfinite(out).all()
    _status()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_back_to_back_launches_and_graph_replay(dtype):
    """Two launches back to back on one stream and a captured-and-replayed graph of the one-kernel path (a straight chain, no parallel
    branches) give the bits of an eager launch."""
    shape, cm, cn = SMALL[0]
    m = _module(shape[1], cm, cn).cuda()
    static_x = _input(shape, dtype, seed=41).cuda()
    with torch.no_grad():
        want = m(static_x).clone()
        a = m(static_x)
        b = m(static_x)
    torch.cuda.synchronize()
    assert torch.equal(a, want) and torch.equal(b, want)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        m(static_x)                                                    # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = m(static_x)
    for rep in range(2):
        x = _input(shape, dtype, seed=100 + rep).cuda()
        static_x.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        got = out.clone()
        with torch.no_grad():
            eager = m(x)
        assert torch.equal(got, eager), f"replay {rep}: replay and eager launch differ"
    _status()
