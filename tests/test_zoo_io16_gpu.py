"""GPU tests (-m gpu): the CNN SE variants (SELayerBias, SELayerBias4, SqueezeExcite, SELayerHidden) and simam_module / SRM /
GaussianGCT / LCT / GCT on fp16 and bf16 activations (csrc/chan_io16.hip mi355_se16_ex_fwd, csrc/chan_stat_io16.hip).

Reference: the oracle functions in fp64 on x16.double() and the fp32 parameters.  The kernels compute in fp32 and round once, so for
every element, none excluded,
    |got - ref64| <= u * |ref64| + 1e-5 * max|ref64| (+ 2^-25 for fp16 results below the normal range),
u = 2^-11 (fp16) / 2^-8 (bf16): half an ulp, relative; 1e-5 is what the fp32 GPU tests of these modules allow
(tests/test_chan_attn_gpu.py, assert_parity(..., 1e-5, ...)).  io16_common._check_chan is that bound; it prints max err / bound first.

Parameters are seeded with O(1) values: the defaults make GCT (gamma = beta = 0) and SRM's BatchNorm the identity."""
import pytest
import torch

import oracle.chan_attn as OC
from io16_common import DTYPES, U, _check_chan as _check, _input, _run, _status, _ulps

pytestmark = pytest.mark.gpu

F64 = torch.float64
SINGLE = [(2, 64, 32, 32),        # two full chunks per lane
          (2, 16, 56, 56),        # 392 chunks over 64 lanes: the 7th slot is ragged (parking of idle lanes in SimAM / SRM)
          (2, 64, 8, 8),          # 8 live lanes
          (3, 8, 64, 64)]         # 8 chunks per lane, the row limit
GENERAL = [(3, 72, 7, 7), (2, 48, 13, 17), (2, 100, 5, 9), (1, 8, 1, 2), (1, 8, 1, 1)]
SMALL = SINGLE[0]


def _zoo(C, hw):
    """(name, module on the device, fp64 reference of a host tensor) for the statistics gates at C channels; parameters non-trivial.
    LCT with 16 channels per group (a group spans two workgroups) and with 4 (two groups inside one), where C allows."""
    from mi355attn.modules import GCT, LCT, SRM, GaussianGCT, simam_module
    g = torch.Generator().manual_seed(77)
    rn = lambda *s: torch.randn(*s, generator=g)
    out = []
    if hw > 1:
        out.append(("simam", simam_module(), lambda x: OC.simam_forward(x.double(), 1e-4, dtype=F64)))
        srm = SRM(C).eval()
        with torch.no_grad():
            srm.cfc.weight.copy_(rn(C, 1, 2))
            srm.bn.weight.copy_(0.5 + torch.rand(C, generator=g))
            srm.bn.bias.copy_(0.5 * rn(C))
            srm.bn.running_mean.copy_(0.3 * rn(C))
            srm.bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
        sd = {k: v.detach().clone() for k, v in srm.state_dict().items()}
        out.append(("srm", srm, lambda x: OC.srm_forward(x.double(), sd["cfc.weight"], sd["bn.weight"], sd["bn.bias"], sd["bn.running_mean"],
                                                          sd["bn.running_var"], srm.bn.eps, dtype=F64)))
    out.append(("gct_gauss", GaussianGCT(C), lambda x: OC.gct_gauss_forward(x.double(), 2, 1e-5, dtype=F64)))
    for cpg in (16, 4):
        if C % cpg == 0:
            lct = LCT(C, C // cpg)
            with torch.no_grad():
                lct.w.copy_(rn(C))
                lct.b.copy_(rn(C))
            w, b = lct.w.detach().clone(), lct.b.detach().clone()
            out.append((f"lct/{cpg}", lct, lambda x, w=w, b=b, gr=C // cpg: OC.lct_forward(x.double(), w, b, gr, 1e-5, dtype=F64)))
    for mode, relu in (("l2", False), ("l1", False), ("l1", True)):
        gct = GCT(C, mode=mode, after_relu=relu)
        with torch.no_grad():
            gct.alpha.copy_(0.5 + torch.rand(1, C, 1, 1, generator=g))
            gct.gamma.copy_(rn(1, C, 1, 1))
            gct.beta.copy_(0.5 * rn(1, C, 1, 1))
        al, ga, be = (p.detach().clone() for p in (gct.alpha, gct.gamma, gct.beta))
        out.append((f"gct_{mode}{'_relu' if relu else ''}", gct,
                    lambda x, al=al, ga=ga, be=be, mode=mode, relu=relu: OC.gct_forward(x.double(), al, ga, be, 1e-5, mode, relu, dtype=F64)))
    return [(n, m.cuda(), r) for n, m, r in out]


def _se(C):
    """(name, module on the device, fp64 reference) for the four SE variants; biases O(1)."""
    from mi355attn.modules import SELayerBias, SELayerBias4, SELayerHidden, SqueezeExcite
    torch.manual_seed(99)
    g = torch.Generator().manual_seed(98)
    out = []
    for name, m in (("se_bias", SELayerBias(C, 8)), ("se_bias4", SELayerBias4(C))):
        with torch.no_grad():
            m.fc[0].bias.copy_(torch.randn(m.fc[0].bias.shape, generator=g))
            m.fc[2].bias.copy_(torch.randn(m.fc[2].bias.shape, generator=g))
        p = [t.detach().clone() for t in (m.fc[0].weight, m.fc[0].bias, m.fc[2].weight, m.fc[2].bias)]
        out.append((name, m, lambda x, p=p: OC.se_ex_forward(x.double(), *p, gate="sigmoid", dtype=F64)))
    sq = SqueezeExcite(C)
    with torch.no_grad():
        sq.conv_reduce.bias.copy_(torch.randn(sq.conv_reduce.bias.shape, generator=g))
        sq.conv_expand.bias.copy_(3.0 * torch.randn(C, generator=g))          # pre-gate values on both clamps of the hard sigmoid
    p = [t.detach().clone() for t in (sq.conv_reduce.weight, sq.conv_reduce.bias, sq.conv_expand.weight, sq.conv_expand.bias)]
    out.append(("squeeze_excite", sq, lambda x, p=p: OC.se_ex_forward(x.double(), *p, gate="hard_sigmoid", dtype=F64)))
    hid = SELayerHidden(C, 24)
    w = [hid.fc[0].weight.detach().clone(), hid.fc[2].weight.detach().clone()]
    out.append(("se_hidden", hid, lambda x, w=w: OC.se_forward(x.double(), *w, dtype=F64)))
    return [(n, m.eval().cuda(), r) for n, m, r in out], p


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SINGLE + GENERAL)
def test_statistics_gates_vs_fp64_oracle(shape, dtype):
    x = _input(shape, dtype)
    xd = x.cuda()
    blocks = _zoo(shape[1], shape[2] * shape[3])
    assert len(blocks) >= (4 if shape[2] * shape[3] == 1 else 7)
    for name, m, ref in blocks:
        y, tags = _run(m, xd)
        if shape in SINGLE:
            assert any(t.startswith("stat16_single_kernel") for t in tags), (name, tags)
        else:
            assert any(t.startswith("stat_apply16_kernel") for t in tags) and not any("_single_kernel" in t for t in tags), (name, tags)
        _check(y, ref(x), dtype, f"{name}{shape} {dtype}")
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 64, 32, 32), (3, 72, 7, 7), (2, 40, 14, 14)])
def test_se_variants_vs_fp64_oracle(shape, dtype):
    from mi355attn import functional as F
    x = 3.0 * _input(shape, torch.float32)
    x = x.to(dtype)
    xd = x.cuda()
    blocks, sq = _se(shape[1])
    # the hard sigmoid's pre-gate values (the oracle's intermediate, restated) lie on both clamps and in between
    w1, b1, w2, b2 = (t.double() for t in sq)
    z = torch.relu(x.double().mean(dim=(2, 3)) @ w1.reshape(w1.shape[0], -1).t() + b1) @ w2.reshape(w2.shape[0], -1).t() + b2
    want = x.double() * (torch.clamp(z + 3.0, 0.0, 6.0) / 6.0)[:, :, None, None]
    assert torch.equal(want, OC.se_ex_forward(x.double(), *sq, gate="hard_sigmoid", dtype=F64))
    assert bool((z <= -3).any()) and bool((z >= 3).any()) and bool(((z > -2.5) & (z < 2.5)).any()), (float(z.min()), float(z.max()))
    for name, m, ref in blocks:
        y, tags = _run(m, xd)
        assert any(t.startswith(("se16_single_kernel", "scale16_kernel")) for t in tags), (name, tags)
        if shape == (2, 64, 32, 32):
            assert any(t.startswith("se16_single_kernel") for t in tags), (name, tags)
        _check(y, ref(x), dtype, f"{name}{shape} {dtype}")
    # SELayer keeps its bits: mi355_se16_fwd against mi355_se16_ex_fwd with null biases and gate 0
    hid = blocks[3][1]
    with torch.no_grad():
        a = F.se_forward(xd, hid.fc[0].weight, hid.fc[2].weight)
        b = F.se_ex_forward(xd, hid.fc[0].weight, None, hid.fc[2].weight, None)
    assert torch.equal(a, b), "mi355_se16_ex_fwd without biases differs from mi355_se16_fwd"
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_general_form_agrees_with_single_read(dtype):
    import mi355attn
    x = _input(SMALL, dtype)
    xd = x.cuda()
    blocks = _zoo(64, 1024) + _se(64)[0]
    with torch.no_grad():
        single = {name: m(xd) for name, m, _ in blocks}
    with mi355attn.options(zoo_single=0, se_single=0):
        for name, m, ref in blocks:
            y, tags = _run(m, xd)
            assert tags and not any("_single_kernel" in t for t in tags), (name, tags)
            _check(y, ref(x), dtype, f"{name}{SMALL} general {dtype}")
            d = _ulps(y, single[name])
            print(f"[zoo16] {name} single vs general: {d} ulp")
            assert d <= 1, f"{name}: single-read and general form differ by {d} ulps"
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [SMALL, (2, 16, 56, 56), (3, 72, 7, 7)])
def test_16bit_path_vs_fp32_path_rounded(shape, dtype):
    """m(x16) against m(x16.float()) rounded to the I/O type: at most one representable value apart, everywhere."""
    xd = _input(shape, dtype).cuda()
    for name, m, _ in _zoo(shape[1], shape[2] * shape[3]) + _se(shape[1])[0]:
        with torch.no_grad():
            y16 = m(xd)
            y32 = m(xd.float())
        assert y16.dtype == dtype and y32.dtype == torch.float32
        d = _ulps(y16, y32.to(dtype))
        print(f"[zoo16] {name}{shape} {dtype}: {d} ulp from the fp32 path")
        assert d <= 1, f"{name}{shape}: {d} ulps"
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_16bit_parameters_and_in_place_update(dtype):
    xd = _input(SMALL, dtype).cuda()
    for name, m, _ in _zoo(64, 1024) + _se(64)[0]:
        if not list(m.parameters()):
            continue                                                   # simam_module, GaussianGCT: nothing to convert
        with torch.no_grad():
            m16 = {torch.float16: m.half, torch.bfloat16: m.bfloat16}[dtype]()     # in place: parameters and BatchNorm statistics are 16-bit now
            assert all(p.dtype == dtype for p in m16.parameters())
            y16 = m16(xd)
            vals = {k: v.detach().clone() for k, v in m16.state_dict().items()}
            m32 = m16.float()                                          # the same (rounded) values in fp32 parameters
            assert all(torch.equal(v.float(), m32.state_dict()[k].float()) for k, v in vals.items())
            y32 = m32(xd)
            assert y16.dtype == dtype and torch.equal(y16, y32), f"{name}: 16-bit parameters change the result"
            m16 = {torch.float16: m.half, torch.bfloat16: m.bfloat16}[dtype]()
            assert torch.equal(m16(xd), y16)
            p = next(m16.parameters())
            p.mul_(-1.5)                                               # in-place update: the cached fp32 copy must not survive it
            after = m16(xd)
            assert not torch.equal(after, y16), f"{name}: stale fp32 copy of an updated 16-bit parameter"
            assert torch.equal(after, m16.float()(xd)), name
    _status()


def test_gct_fp16_overflow_follows_the_rounded_reference():
    """GCT's gate reaches 2: y = x * gate may leave the fp16 range.  y is +-inf exactly where the fp64 reference rounded to fp16 is, finite
    elsewhere; nothing is reported (outputs are not MFMA operands); the same input in bf16 stays finite."""
    from mi355attn.modules import GCT
    g = torch.Generator().manual_seed(5)
    C = 64
    gct = GCT(C)
    with torch.no_grad():
        gct.alpha.copy_(0.5 + torch.rand(1, C, 1, 1, generator=g))
        gct.gamma.copy_(0.2 * torch.randn(1, C, 1, 1, generator=g).abs())
        gct.beta.fill_(0.7)
    al, ga, be = (p.detach().clone() for p in (gct.alpha, gct.gamma, gct.beta))
    gct = gct.cuda()
    x = _input(SMALL, torch.float16)
    big = [(0, 3, 4, 5, 60000.0), (0, 3, 31, 31, -60000.0), (1, 40, 0, 0, 60000.0), (1, 63, 17, 2, -60000.0), (0, 17, 9, 9, 60000.0)]
    for b, c, i, j, v in big:
        x[b, c, i, j] = v
    ref = OC.gct_forward(x.double(), al, ga, be, 1e-5, "l2", False, dtype=F64)
    for b, c, i, j, v in big:
        gate = float(ref[b, c, i, j]) / v
        assert gate > 1.1, (b, c, gate)                                # the fp64 reference confirms the gate of these channels
    ref16 = ref.to(torch.float16)
    assert int(torch.isinf(ref16).sum()) == len(big)
    with torch.no_grad():
        y = gct(x.cuda()).cpu()
    assert y.dtype == torch.float16
    assert torch.equal(torch.isinf(y), torch.isinf(ref16)) and torch.equal(y[torch.isinf(ref16)], ref16[torch.isinf(ref16)]), "inf pattern"
    assert not torch.isnan(y).any()
    fin = ~torch.isinf(ref16)
    err = (y.double() - ref)[fin].abs()
    bound = U[torch.float16] * ref[fin].abs() + 1e-5 * float(ref[fin].abs().max()) + (ref[fin].abs() < 2.0 ** -14).double() * 2.0 ** -25
    print(f"[zoo16] gct overflow: max err / bound on the finite elements = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    _status()                                                          # sync and range words stay clean
    with torch.no_grad():
        yb = gct(x.bfloat16().cuda())
    assert torch.isfinite(yb).all(), "bf16 has the fp32 range"
    _check(yb, OC.gct_forward(x.bfloat16().double(), al, ga, be, 1e-5, "l2", False, dtype=F64), torch.bfloat16, "gct bf16, x = +-60000")
    _status()


def test_workspaces_per_io_type_and_graph_replay():
    """fp32, fp16, bf16 and fp32 again on one shape: the fp32 results are bit-identical (no shared ticket state).  Then one fp16 GCT and
    one fp16 LCT forward captured on a single stream and replayed twice: the ticket and epoch live in the workspace, a replay is a launch."""
    blocks = {n: (m, r) for n, m, r in _zoo(64, 1024)}
    gct, gref = blocks["gct_l2"]
    lct, _ = blocks["lct/16"]
    x32 = _input(SMALL, torch.float32)
    xd = x32.cuda()
    with torch.no_grad():
        first = gct(xd)
        h = gct(xd.half())
        bf = gct(xd.bfloat16())
        last = gct(xd)
    assert first.dtype == torch.float32 and torch.equal(first, last)
    _check(h, gref(x32.half()), torch.float16, "gct between fp32 calls, fp16")
    _check(bf, gref(x32.bfloat16()), torch.bfloat16, "gct between fp32 calls, bf16")
    _status()
    static_x = _input(SMALL, torch.float16, seed=41).cuda()
    with torch.no_grad():
        want = (gct(static_x).clone(), lct(static_x).clone())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        gct(static_x), lct(static_x)                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = (gct(static_x), lct(static_x))
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]), f"replay {rep} differs from the eager result"
        out[0].zero_(), out[1].zero_()
    _status()


def test_fp32_input_keeps_its_kernels_and_other_modules_still_refuse():
    from conftest import assert_parity
    from mi355attn.modules import GCModule
    x = _input(SMALL, torch.float32)
    xd = x.cuda()
    for name, m, ref in _zoo(64, 1024) + _se(64)[0]:
        y, tags = _run(m, xd)
        assert y.dtype == torch.float32 and not any("16_" in t for t in tags), (name, tags)
        _, tags16 = _run(m, xd.half())
        assert any("16_" in t for t in tags16), (name, tags16)
        assert_parity(y.cpu(), ref(x).float(), 1e-5, name + " fp32")
    with pytest.raises(TypeError) as e:
        GCModule(64).eval().cuda()(xd.half())
    for accepted in ("SELayerBias", "SELayerBias4", "SELayerHidden", "SqueezeExcite", "simam_module", "SRM", "GaussianGCT", "LCT", "GCT"):
        assert accepted in str(e.value), (accepted, str(e.value))
    _status()
