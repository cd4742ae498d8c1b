"""GPU tests (-m gpu): MixerLayer, mlps.mlp_mixer.PatchEmbedding and MLP_Mixer on fp16 / bf16 activations.  Shapes, seeds and the fp64
references (the oracle's Mixer restatement with the interface roundings applied) are tests/mixer_io16_cases.py; a reference is computed
once and shared.  Bars: conftest.assert_parity at arena_cases.TOL[io] against fp64, 1 ulp of the I/O type against the fp32-I/O module
(which runs the same arithmetic on x16.float(): the 16-bit path may differ from it only in where the one rounding of y falls)."""
import copy
import warnings

import pytest
import torch

import mixer_io16_cases as MC
from arena_cases import TOL
from conftest import assert_parity, max_abs_ratio, rel_fro
from io16_common import _run, _status, _ulps

pytestmark = pytest.mark.gpu
IDS = ["fp16", "bf16"]
TNAME = {torch.float16: "f16", torch.bfloat16: "bf16"}


def _x_sized_cast(tags, n):
    """Tags of mi355_cast16_fwd launches over n elements (weights are cast once, activations must never be)."""
    return [t for t in tags if t.startswith("cast16_kernel") and t.endswith(f"n={n}")]


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=IDS)
@pytest.mark.parametrize("cid", list(MC.LAYERS))
def test_layer_on_16bit_activations(cid, dtype):
    """Checks 1, 2, 3 and 5 of the layer: the type of y, 1 ulp against the fp32-I/O module at precision = io, parity against the fp64
    oracle on x16 with y rounded once, and the kernels that ran."""
    from mi355attn.modules import MixerLayer
    c, io = MC.LAYERS[cid], MC.IO[dtype]
    m = MC.layer_module(cid).cuda()
    x16 = MC.layer_input(cid).to(dtype).cuda()
    y, tags = _run(m, x16)
    assert y.dtype == dtype and y.shape == x16.shape                                               # 1
    m32 = MixerLayer(c["C"], c["N"], mlp_ratio=c["ratio"] or [0.5, 4], precision=io).eval().cuda()
    m32.load_state_dict(m.state_dict())
    with torch.no_grad():
        y32 = m32(x16.float())
    assert y32.dtype == torch.float32
    ulps = _ulps(y, y32.to(dtype))
    ref = MC.layer_emulated(cid, dtype)
    rf, ma = rel_fro(y.cpu(), ref), max_abs_ratio(y.cpu(), ref)
    print(f"[mixer_io16] {cid} {dtype}: {ulps} ulp from the fp32-I/O module; vs fp64: rel_fro {rf:.3e} max_abs_ratio {ma:.3e} (bar {TOL[io]:g})")
    assert ulps <= 1, f"{cid}: {ulps} ulp from the fp32-I/O module rounded to {dtype}"              # 2
    assert_parity(y.cpu(), ref, TOL[io], f"{cid} {dtype} vs the fp64 oracle on x16, y rounded once")  # 3
    token16 = [t for t in tags if t.startswith(f"mixer_token16_kernel<{TNAME[dtype]}>")]           # 5
    widen = [t for t in tags if t.startswith("widen16_kernel")]
    assert not _x_sized_cast(tags, x16.numel()), tags
    assert not any(t.startswith("round16_kernel") for t in tags), tags                              # the last GEMM's epilogue rounds y
    if c["fused"]:
        assert len(token16) == 1 and not widen, tags
        assert any(t.startswith(f"row_stats_x16_kernel<{TNAME[dtype]}>") for t in tags), tags
        assert not any(t.startswith("mixer_token_kernel") or t.startswith("row_stats_kernel") for t in tags), tags
    else:
        assert len(widen) == 1 and widen[0].endswith(f"n={x16.numel()}") and not token16, tags
    _status()


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=IDS)
@pytest.mark.parametrize("cid", ["c512_b2", "c128_n49_b2"])
def test_16bit_parameters_give_the_bits_of_their_widened_values(cid, dtype):
    """Check 4: fp32 parameters (autocast) and module.half() / .bfloat16() parameters of the same values give the same bits, on the fused
    and on the widening route; an in-place update of a 16-bit parameter is seen by the next forward."""
    m16 = MC.layer_module(cid).to(dtype).cuda()
    m32 = copy.deepcopy(m16).float()                                       # the widened values, as fp32 parameters
    x16 = MC.layer_input(cid).to(dtype).cuda()
    with torch.no_grad():
        a, b = m32(x16), m16(x16)
        assert a.dtype == b.dtype == dtype and torch.equal(a, b), f"{_ulps(a, b)} ulp between fp32 and 16-bit parameters"
        for m in (m16, m32):
            m.channel_mlp.fc2.bias.mul_(2.0)
            m.token_mlp.fc1.weight.mul_(0.5)                               # powers of two: exact in fp32 and in the 16-bit type alike
            m.norm1.weight.mul_(2.0)
        a2, b2 = m32(x16), m16(x16)
    assert torch.equal(a2, b2) and not torch.equal(a2, a), "the in-place update of a parameter was not seen"
    _status()


def test_fp32_forward_keeps_bits_and_tags_around_16bit_calls():
    """Check 6."""
    m = MC.layer_module("c512_b2").cuda()
    x = MC.layer_input("c512_b2").cuda()
    _run(m, x)                                                             # the weights' 16-bit copies are made here, once
    before, tags0 = _run(m, x)
    for dtype in MC.DTYPES:
        _run(m, x.to(dtype))
    after, tags1 = _run(m, x)
    assert before.dtype == torch.float32 and torch.equal(before, after) and sorted(tags0) == sorted(tags1)
    assert any(t.startswith("mixer_token_kernel") for t in tags0) and any(t.startswith("row_stats_kernel") for t in tags0), tags0
    assert not any("mixer_token16" in t or "row_stats_x16" in t or "widen16" in t or "round16" in t for t in tags0), tags0
    _status()


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=IDS)
def test_each_image_is_independent_of_its_batch(dtype):
    """Check 7: every image of the B = 3 case equals its B = 1 run, bit for bit."""
    m = MC.layer_module("c256_b3").cuda()
    x16 = MC.layer_input("c256_b3").to(dtype).cuda()
    with torch.no_grad():
        y = m(x16)
        for i in range(x16.shape[0]):
            assert torch.equal(y[i:i + 1], m(x16[i:i + 1].contiguous())), f"image {i} depends on the batch around it"
    _status()


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=IDS)
@pytest.mark.parametrize("cid", ["c512_b8", "c512_b2", "c256_b3"])
def test_early_and_stats_variants_of_the_16bit_kernel_are_bit_identical(cid, dtype):
    """Options "mixer_early" and "mixer_stats" select the same variants of the 16-bit-x kernel as of the fp32-x one: same bits, their tags
    behind the type (the statistics inside the kernel are built for C = 512: both workgroup-id mappings, and C = 256 keeps the pre-pass)."""
    import mi355attn
    m = MC.layer_module(cid).cuda()
    x16 = MC.layer_input(cid).to(dtype).cuda()
    y0, _ = _run(m, x16)
    with mi355attn.options(mixer_early=1, mixer_stats=1):
        y1, tags = _run(m, x16)
    tok = [t for t in tags if t.startswith("mixer_token16_kernel")]
    want = f"mixer_token16_kernel<{TNAME[dtype]}><early>" + ("<stats>" if MC.LAYERS[cid]["C"] == 512 else "")
    assert len(tok) == 1 and tok[0].startswith(want + " "), tags
    assert any(t.startswith("row_stats_x16_kernel") for t in tags) == (MC.LAYERS[cid]["C"] != 512), tags
    assert torch.equal(y0, y1)
    _status()


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=IDS)
@pytest.mark.parametrize("M,N,K", [(392, 256, 1024), (1568, 512, 2048), (2048, 64, 128)])
def test_fc2_epilogue_adds_the_residual_before_it_rounds(M, N, K, dtype):
    """Check 8: linear16(resid = x1, out16) = round(the fp32 product + x1) within 1 ulp -- an epilogue that dropped the residual, or
    rounded before adding it, is off by far more (x1 is as large as the product).  The three shapes are the layer's fc2 at C = 256 and
    512 (plain tile kernel: every persistent kernel refuses a 16-bit output with a residual) and a short-K shape (the
    weight-stationary kernel)."""
    from mi355attn import functional as F
    io = MC.IO[dtype]
    g = torch.Generator().manual_seed(M + N + K)
    h16 = torch.randn(M, K, generator=g).to(dtype).cuda()
    w16 = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).cuda()
    bias = (0.1 * torch.randn(N, generator=g)).cuda()
    x1 = (1.5 * torch.randn(M, N, generator=g)).cuda()
    y = F.linear16(h16, w16, bias, resid=x1, out16=True, precision=io)
    plain = F.linear16(h16, w16, bias, out16=False, precision=io)
    assert y.dtype == dtype and plain.dtype == torch.float32
    want = (plain + x1).to(dtype)
    ulps, dropped = _ulps(y, want), _ulps(y, plain.to(dtype))
    print(f"[mixer_io16] fc2 {M}x{N}x{K} {dtype}: {ulps} ulp from round(product + x1); {dropped} ulp from the product alone")
    assert ulps <= 1 and dropped > 16
    _status()


def test_saturating_layernorm_warns_once_and_returns_the_strict_result():
    """Check 9.  LayerNorm removes the scale of x, so no x can saturate LN(x) w + b by its size alone: the layer's norm1.bias is raised to
    7e4 on one channel instead (beyond 65504 for every token), which saturates the fp16 LN operand inside the token kernel (range code
    4).  fp16: exactly one warning, and the strict result rounded once.  bf16: silence."""
    from mi355attn.modules import MixerLayer
    m = MC.layer_module("c256_b1")
    m.norm1.bias[5] = 7.0e4
    m = m.cuda()
    strict = MixerLayer(256, 196, precision=0).eval().cuda()
    strict.load_state_dict(m.state_dict())
    x = MC.layer_input("c256_b1").cuda()
    with torch.no_grad():
        want32 = strict(x.half().float())
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            y = m(x.half())
        assert len(seen) == 1 and "re-running this forward in strict mode" in str(seen[0].message), [str(w.message) for w in seen]
        assert y.dtype == torch.float16 and torch.equal(y, want32.half())
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            yb = m(x.bfloat16())
        assert not seen and yb.dtype == torch.bfloat16 and torch.isfinite(yb).all(), [str(w.message) for w in seen]
    _status()


def test_graph_capture_and_two_replays_equal_eager():
    """Check 10, one fp16 layer."""
    m = MC.layer_module("c512_b2").cuda()
    static_x = MC.layer_input("c512_b2").half().cuda()
    with torch.no_grad():
        want = m(static_x).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        m(static_x)                                                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = m(static_x)
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), f"replay {rep} differs from the eager result"
        out.zero_()
    _status()


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=IDS)
def test_model_is_the_composition_of_its_parts(dtype):
    """Check 11: MLP_Mixer(dim 256, depth 2) on (2, 3, 224, 224) equals embed -> each layer -> token mean -> head on 16-bit tensors bit for
    bit, and meets the fp64 oracle with the interface roundings applied at TOL[io]; the distance to the unrounded oracle is printed."""
    from mi355attn import functional as F
    io = MC.IO[dtype]
    m = MC.model_module().cuda()
    img = MC.model_input().to(dtype).cuda()
    import mi355attn
    outs = []
    with torch.no_grad():
        rows = mi355attn.kernel_trace(lambda: outs.append(m(img)))          # (tag, launches, ...) per distinct tag
    y, tags, count = outs[0], [r[0] for r in rows], {r[0]: r[1] for r in rows}
    assert y.dtype == dtype and tuple(y.shape) == (2, MC.MODEL["num_classes"])
    with torch.no_grad():
        x = m.patch_embedding(img)
        assert x.dtype == dtype and tuple(x.shape) == (2, 196, 256)
        for blk in m.blocks:
            x = blk(x)
            assert x.dtype == dtype
        pooled = F.token_mean16(x)
        manual = F.linear(pooled, m.head.weight, m.head.bias, precision=io).to(dtype)
    assert pooled.dtype == torch.float32 and torch.equal(y, manual), f"{_ulps(y, manual)} ulp from the manual composition"
    assert_parity(pooled.cpu(), x.double().mean(1).cpu(), 1e-6, "token_mean16 vs fp64")
    plain, emu = MC.model_refs(dtype)
    print(f"[mixer_io16] model {dtype}: vs the emulated 16-bit composition rel_fro {rel_fro(y.cpu(), emu):.3e} max_abs_ratio "
          f"{max_abs_ratio(y.cpu(), emu):.3e} (bar {TOL[io]:g}); vs the unrounded oracle rel_fro {rel_fro(y.cpu(), plain):.3e} "
          f"max_abs_ratio {max_abs_ratio(y.cpu(), plain):.3e} (not gated)")
    assert_parity(y.cpu(), emu, TOL[io], f"MLP_Mixer {dtype} vs the fp64 oracle with the interface roundings")
    assert any(t.startswith("im2col_gather16_kernel") for t in tags) and any(t.startswith(f"token_mean16_kernel<{TNAME[dtype]}>") for t in tags), tags
    assert sum(n for t, n in count.items() if t.startswith(f"mixer_token16_kernel<{TNAME[dtype]}>")) == MC.MODEL["depth"], count
    assert not any(t.startswith(("widen16_kernel", "round16_kernel", "im2col16_kernel")) for t in tags), tags
    assert not _x_sized_cast(tags, img.numel()) and not _x_sized_cast(tags, 2 * 196 * 256), tags
    _status()
