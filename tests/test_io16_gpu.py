"""GPU tests (-m gpu): SELayer / ECALayer / CBAM / ChannelAttention / SpatialAttention on fp16 and bf16 activations (csrc/chan_io16.hip).

Reference: the oracle functions in fp64 on x16.double() and the fp32 parameters.  The kernels compute in fp32 and round once, so for
every element
    |got - ref64| <= u * |ref64| + t32 (+ 2^-25 for fp16 results below the normal range),
u = 2^-11 (fp16) / 2^-8 (bf16): half an ulp, relative.  t32 is what the fp32 GPU tests of the same modules allow for the same shapes,
max|y - r| <= 1e-5 * max|r| (tests/test_chan_attn_gpu.py:38-43 for the small shapes, :279 for the C2 shape; conftest.assert_parity).
No element is excluded."""
import pytest
import torch

import oracle.chan_attn as OC
from io16_common import DTYPES, _check_chan as _check, _input, _status as _common_status, _ulps

pytestmark = pytest.mark.gpu

NEW_TAGS = ("se16_", "eca16_", "cbam16_", "pool16_", "scale16_", "chan_gates16_")


def _mods(C, red=16, ks=7):
    from mi355attn.modules import CBAM, ECALayer, SELayer
    torch.manual_seed(1234)
    return SELayer(C, red).eval(), ECALayer(C).eval(), CBAM(C, red, ks).eval()


def _blocks(C, red=16, ks=7):
    """(name, module, fp64 reference of a host tensor) for the five blocks, modules on the device with fp32 parameters."""
    se, eca, cbam = _mods(C, red, ks)
    sd = {k: v.detach().clone() for k, v in cbam.state_dict().items()}
    w1, w2, wc = sd["ca.fc.0.weight"], sd["ca.fc.2.weight"], sd["sa.conv.weight"]
    sw1, sw2, ew = se.fc[0].weight.detach().clone(), se.fc[2].weight.detach().clone(), eca.conv.weight.detach().clone()
    f64 = torch.float64
    cbam = cbam.cuda()
    return [("se", se.cuda(), lambda x: OC.se_forward(x.double(), sw1, sw2, dtype=f64)),
            ("eca", eca.cuda(), lambda x: OC.eca_forward(x.double(), ew, dtype=f64)),
            ("cbam", cbam, lambda x: OC.cbam_forward(x.double(), w1, w2, wc, dtype=f64)),
            ("ca", cbam.ca, lambda x: OC.cbam_channel_forward(x.double(), w1, w2, dtype=f64)),
            ("sa", cbam.sa, lambda x: OC.cbam_spatial_forward(x.double(), wc, dtype=f64))]


def _status():
    _common_status(range_word=False)                                   # these tests have always read the sync word alone


def _red_ks(shape):
    B, C, H, W = shape
    return (16 if C >= 32 else 4), (7 if min(H, W) >= 3 else 3)


SMALL = (2, 64, 32, 32)
# general form: rows that are not a multiple of 16 bytes, C not a multiple of 8, 1 x 1 maps
GENERAL = [(3, 72, 7, 7), (2, 48, 13, 17), (1, 8, 1, 1), (2, 100, 5, 9)]
# 16 register slots per lane with the last one partly filled: the fp32 CBAM reads x once here, the 16-bit CBAM refuses the single-read
# kernel and takes its general form (SE and ECA read once)
CBAM_NV16_PARTIAL = (2, 400, 8, 8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [SMALL] + GENERAL + [CBAM_NV16_PARTIAL])
def test_blocks_vs_fp64_oracle(shape, dtype):
    red, ks = _red_ks(shape)
    x = _input(shape, dtype)
    xd = x.cuda()
    for name, m, ref in _blocks(shape[1], red, ks):
        with torch.no_grad():
            y = m(xd)
        _check(y, ref(x), dtype, f"{name}{shape} {dtype}")
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_general_form_when_single_read_is_switched_off(dtype):
    import mi355attn
    shape = (2, 512, 28, 28)
    x = _input(shape, dtype)
    xd = x.cuda()
    blocks = _blocks(512)
    with torch.no_grad():
        single = {name: m(xd) for name, m, _ in blocks}
    with mi355attn.options(se_single=0, eca_single=0, cbam_single=0):
        for name, m, ref in blocks:
            with torch.no_grad():
                rows = mi355attn.kernel_trace(lambda: m(xd))
                y = m(xd)
            tags = [r[0] for r in rows]
            assert not any("_single_kernel" in t or "halo_kernel" in t for t in tags), tags
            assert any(t.startswith("scale16_kernel") for t in tags), tags
            _check(y, ref(x), dtype, f"{name}{shape} general {dtype}")
            # a shape both forms accept: they differ by at most one ulp of the I/O type
            d = _ulps(y, single[name])
            print(f"[io16] {name} single vs general: {d} ulp")
            assert d <= 1, f"{name}: single-read and general form differ by {d} ulps"
    _status()


@pytest.fixture(scope="module")
def c2_batches():
    """(256, 256, 56, 56) from the seed-4321 CPU stream in slabs of 32, as the fp32 full-size test fills it; images 0, 127, 255 kept."""
    g = torch.Generator(device="cpu").manual_seed(4321)
    pick = [0, 127, 255]
    x = torch.empty(256, 256, 56, 56, device="cuda")
    host = {}
    for b0 in range(0, 256, 32):
        blk = torch.randn(32, 256, 56, 56, generator=g)
        x[b0:b0 + 32] = blk.cuda()
        for b in pick:
            if b0 <= b < b0 + 32:
                host[b] = blk[b - b0].clone()
    out = {"pick": pick, "host": torch.stack([host[b] for b in pick])}
    for dt in DTYPES:
        out[dt] = x.to(dt)
    del x
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_c2_bench_shape(c2_batches, dtype):
    import mi355attn
    pick = c2_batches["pick"]
    x = c2_batches[dtype]
    xs = c2_batches["host"].to(dtype)                                  # what the device holds for the sampled images
    for name, m, ref in _blocks(256):
        with torch.no_grad():
            rows = []
            tr = mi355attn.kernel_trace(lambda: rows.append(m(x)))
            y = rows[0]
            y2 = m(x)
        tags = [r[0] for r in tr]
        if name in ("se", "eca", "cbam"):
            assert any("_single_kernel" in t or "halo_kernel" in t for t in tags), (name, tags)   # the C2 shape runs the single-read form
        assert torch.equal(y, y2), f"{name}: run-to-run results differ"
        _check(y[pick], ref(xs), dtype, f"{name}[C2 sample] {dtype}")
        del y, y2, rows
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [SMALL, (3, 72, 7, 7)])
def test_16bit_path_vs_fp32_path_rounded(shape, dtype):
    """m(x16) against m(x16.float()) rounded to the I/O type: at most one ulp of that type, everywhere."""
    red, ks = _red_ks(shape)
    xd = _input(shape, dtype).cuda()
    for name, m, _ in _blocks(shape[1], red, ks):
        with torch.no_grad():
            y16 = m(xd)
            y32 = m(xd.float())
        assert y32.dtype == torch.float32
        d = _ulps(y16, y32.to(dtype))
        print(f"[io16] {name}{shape} {dtype}: {d} ulp from the fp32 path")
        assert d <= 1, f"{name}{shape}: {d} ulps"
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_16bit_parameters_and_in_place_update(dtype):
    xd = _input(SMALL, dtype).cuda()
    for name, m, _ in _blocks(64):
        with torch.no_grad():
            m16 = {torch.float16: m.half, torch.bfloat16: m.bfloat16}[dtype]()     # in place: the parameters are 16-bit now
            assert all(p.dtype == dtype for p in m16.parameters())
            y16 = m16(xd)
            vals = {k: v.detach().clone() for k, v in m16.state_dict().items()}
            m32 = m16.float()                                          # the same values in fp32 parameters
            assert all(torch.equal(v.float(), m32.state_dict()[k]) for k, v in vals.items())
            y32 = m32(xd)
            assert y16.dtype == dtype and torch.equal(y16, y32), f"{name}: 16-bit parameters change the result"
            m16 = {torch.float16: m.half, torch.bfloat16: m.bfloat16}[dtype]()
            again = m16(xd)
            assert torch.equal(again, y16)
            p = next(m16.parameters())
            p.mul_(-1.5)                                               # in-place update: the cached fp32 copy must not survive it
            after = m16(xd)
            assert not torch.equal(after, y16), f"{name}: stale fp32 copy of an updated 16-bit weight"
            want = m16.float()(xd)
            assert torch.equal(after, want), name
    _status()


def test_fp32_input_still_runs_the_fp32_kernels():
    import mi355attn
    from conftest import assert_parity
    import oracle as O
    x = _input(SMALL, torch.float32)
    xd = x.cuda()
    se, eca, cbam = _mods(64)
    refs = {"se": O.se_forward(x, se.fc[0].weight, se.fc[2].weight), "eca": O.eca_forward(x, eca.conv.weight),
            "cbam": O.cbam_forward(x, cbam.ca.fc[0].weight, cbam.ca.fc[2].weight, cbam.sa.conv.weight)}
    for name, m in (("se", se.cuda()), ("eca", eca.cuda()), ("cbam", cbam.cuda())):
        outs = []
        with torch.no_grad():
            rows = mi355attn.kernel_trace(lambda: outs.append(m(xd)))
            rows16 = mi355attn.kernel_trace(lambda: m(xd.half()))
        assert not any(r[0].startswith(NEW_TAGS) for r in rows), rows
        assert any(r[0].startswith(NEW_TAGS) for r in rows16), rows16
        assert outs[0].dtype == torch.float32
        assert_parity(outs[0].cpu(), refs[name], 1e-5, name + " fp32")
    _status()


def test_large_values_inf_and_nan():
    shape = SMALL
    x = torch.full(shape, 60000.0, dtype=torch.float16)
    for name, m, ref in _blocks(64):
        with torch.no_grad():
            y = m(x.cuda())
        assert torch.isfinite(y).all(), f"{name}: 60000 everywhere must stay finite (fp32 pooling sum)"
        _check(y, ref(x), torch.float16, f"{name} x=60000")
    for dtype in DTYPES:
        x = _input(shape, dtype)
        x[0, 3, 4, 5] = float("inf")
        x[1, 7, 0, 1] = float("nan")
        for name, m, ref in _blocks(64):
            with torch.no_grad():
                y = m(x.cuda())
            _check(y, ref(x), dtype, f"{name} inf/nan {dtype}")
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_channels_last_and_strided_inputs(dtype):
    base = _input((2, 64, 32, 40), dtype).cuda()
    cl = _input(SMALL, dtype).cuda().contiguous(memory_format=torch.channels_last)
    sl = base[:, :, :, 4:36]
    assert not cl.is_contiguous() and not sl.is_contiguous()
    for name, m, _ in _blocks(64):
        with torch.no_grad():
            for v in (cl, sl):
                a, b = m(v), m(v.contiguous())
                assert a.dtype == dtype and torch.equal(a, b), f"{name}: non-contiguous input"
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_back_to_back_launches_and_graph_replay(dtype):
    """Two launches back to back on one stream and a captured-and-replayed graph of the SE module (a straight chain) give the bits of an
    eager launch: the granule epoch protocol."""
    se = _blocks(64)[0][1]
    static_x = _input((6, 64, 28, 28), dtype, seed=41).cuda()
    with torch.no_grad():
        want = se(static_x).clone()
        a = se(static_x)
        b = se(static_x)
    torch.cuda.synchronize()
    assert torch.equal(a, want) and torch.equal(b, want)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        se(static_x)                                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = se(static_x)
    for rep in range(3):
        x = _input((6, 64, 28, 28), dtype, seed=100 + rep).cuda()
        static_x.copy_(x)
        g.replay()
        if rep == 1:
            g.replay()                                                 # two replays back to back: the epoch advances inside the graph
        torch.cuda.synchronize()
        got = out.clone()
        with torch.no_grad():
            eager = se(x)                                              # an eager call in between
        assert torch.equal(got, eager), f"replay {rep}: replay and eager launch differ"
    _status()
