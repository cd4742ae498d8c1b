"""GPU tests (-m gpu): CSWinBlock, LePEAttention, Merge_Block and CSWinTransformer on fp16 / bf16 activations, and the two entries under
the narrow stages (mi355_cswin_stripe_attn_x16_fwd, mi355_proj_mlp_fused_x16_fwd).  Shapes, seeds and the fp64 references (the oracle's
CSWin restatement with the interface roundings applied) are tests/cswin_io16_cases.py; a reference is computed once and shared.  Bars:
conftest.assert_parity at arena_cases.TOL[io] against fp64; 1 ulp of the I/O type against the fp32-I/O module on the routes whose
arithmetic between load and store is the same code (0 is expected and the count is printed); bit equality of each entry against its
fp32-x sibling on the widened x."""
import copy
import ctypes
import warnings

import pytest
import torch

import cswin_io16_cases as CC
from arena_cases import TOL
from conftest import assert_parity, max_abs_ratio, rel_fro
from io16_common import _run, _status, _ulps

pytestmark = pytest.mark.gpu
IDS = ["fp16", "bf16"]
STRIPE = [cid for cid, c in CC.BLOCKS.items() if c["route"] in ("A", "A2") and "opts" not in c]
FUSED = [cid for cid, c in CC.BLOCKS.items() if c["route"] in ("A", "B") and "opts" not in c]


def _traced(m, x, opts=None):
    """(output, {tag: launches}) of one forward."""
    import mi355attn
    outs = []
    with torch.no_grad(), mi355attn.options(**(opts or {})):
        rows = mi355attn.kernel_trace(lambda: outs.append(m(x)))
    tally = {}
    for tag, count, *_ in rows:
        tally[tag] = tally.get(tag, 0) + count
    return outs[0], tally


def _count(tally, prefix, suffix=""):
    return sum(n for t, n in tally.items() if t.startswith(prefix) and t.endswith(suffix))


# ---- check 1: the block --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", CC.DTYPES, ids=IDS)
@pytest.mark.parametrize("cid", list(CC.BLOCKS))
def test_block_on_16bit_activations(cid, dtype):
    """The type of y (TypeError before the 16-bit path existed), parity against the fp64 oracle on x16 with y rounded once, the distance
    to the fp32-I/O module at precision = io, and the kernels that ran (counted on the second forward: the first one prepares the
    weights' 16-bit copies)."""
    import mi355attn
    c, io = CC.BLOCKS[cid], CC.IO[dtype]
    route, opts = c["route"], c.get("opts", {})
    m = CC.block_module(cid).cuda()
    x16 = CC.block_input(cid).to(dtype).cuda()
    with torch.no_grad(), mi355attn.options(**opts):
        m(x16)
    y, tally = _traced(m, x16, opts)
    assert y.dtype == dtype and y.shape == x16.shape
    twin = CC.block_module(cid, precision=io).cuda()
    with torch.no_grad(), mi355attn.options(**opts):
        y32 = twin(x16.float())
    assert y32.dtype == torch.float32
    ulps = _ulps(y, y32.to(dtype))
    ref = CC.block_emulated(cid, dtype)
    rf, ma = rel_fro(y.cpu(), ref), max_abs_ratio(y.cpu(), ref)
    print(f"[cswin_io16] {cid} {dtype} route {route}: {ulps} ulp from the fp32-I/O module at precision {io}; vs fp64: rel_fro {rf:.3e} "
          f"max_abs_ratio {ma:.3e} (bar {TOL[io]:g}); tally {sorted(tally.items())}")
    assert_parity(y.cpu(), ref, TOL[io], f"{cid} {dtype} vs the fp64 oracle on x16, y rounded once")
    B, L, C = x16.shape
    n = x16.numel()
    tname = "f16" if io == 1 else "bf16"
    if route in ("A", "A2"):
        assert ulps <= 1, f"{cid}: {ulps} ulp from the fp32-I/O module rounded to {dtype}"
        reso, split = c["args"][1], c["kw"]["split_size"]
        assert tally.get(f"cswin_stripe_kernel<C={C},x16> B={B} reso={reso} split={split}") == 1, tally
        assert _count(tally, "cswin_stripe_kernel") == 1, tally
    if route in ("A", "B"):
        assert tally.get(f"mlp_fused_kernel<C={C},proj,x16> M={B * L}") == 1 and _count(tally, "mlp_fused_kernel") == 1, tally
    if route == "A":
        assert sum(tally.values()) == 2, f"two launches per block: {tally}"
    if route in ("A2", "B2"):
        H = m.mlp.fc1.out_features
        assert tally.get(f"gemm16_res_kernel<{tname},r16,o32> M={B * L} N={C} K={C}") == 1, tally
        assert tally.get(f"gemm16_res_kernel<{tname},r32,o16> M={B * L} N={C} K={H}") == 1, tally
    if route in ("B", "B2"):
        assert twin is not None and y32.shape == y.shape          # parity with the twin only: it may fold LayerNorm into its weights
        assert_parity(y.float().cpu(), y32.double().cpu(), TOL[io], f"{cid} {dtype} vs the fp32-I/O module")
        assert tally.get(f"layernorm_x16_kernel<{tname}> rows={B * L} cols={C}") == 1 and not _count(tally, "cswin_stripe_kernel"), tally
    if route != "C":
        assert not _count(tally, "widen16_kernel") and not _count(tally, "round16_kernel") and not _count(tally, "cast16_kernel", f"n={n}"), tally
    else:
        assert _count(tally, "widen16_kernel") == 1 == _count(tally, "widen16_kernel", f"n={n}"), tally
        assert _count(tally, "round16_kernel") == 1 == _count(tally, "round16_kernel", f"n={n}"), tally
        assert not any("x16" in t for t in tally), tally
        with torch.no_grad():
            same = CC.block_module(cid, precision=c.get("precision", io)).cuda()(x16.float()).to(dtype)
        assert torch.equal(y, same), f"route C is widen, the fp32 body, round: {_ulps(y, same)} ulp"
    _status()


# ---- check 2: the entries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", CC.DTYPES, ids=IDS)
@pytest.mark.parametrize("cid", STRIPE)
def test_stripe_x16_entry_has_the_bits_of_the_fp32_entry_on_the_widened_x(cid, dtype):
    from mi355attn import functional as F
    io = CC.IO[dtype]
    m = CC.block_module(cid).cuda()
    x16 = CC.block_input(cid).to(dtype).cuda()
    a0, a1 = m.attns
    args = (m.norm1, m.qkv, a0.get_v, a1.get_v, m.patches_resolution, m.num_heads, m.split_size, a0.scale)
    with torch.no_grad():
        got = F.cswin_stripe_attention16(x16, *args)
        want = F.cswin_stripe_attention(x16.float(), *args, io)
    assert got.dtype == want.dtype == dtype and got.shape == x16.shape
    assert torch.equal(got, want), f"{cid} {dtype}: {int((got != want).sum())} of {got.numel()} elements differ, {_ulps(got, want)} ulp"
    _status()


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=IDS)
@pytest.mark.parametrize("cid,tt4", [(cid, 0) for cid in FUSED] + [(cid, 1) for cid in FUSED if CC.BLOCKS[cid]["args"][0] == 64])
def test_proj_mlp_x16_entry_rounds_the_fp32_entrys_y_once(cid, tt4, dtype):
    """y16 is the fp32 entry's y (computed from x16 widened) rounded once -- bit for bit -- and more than 16 ulp away from that y without
    the residual x: an epilogue that dropped x, or rounded before adding it, cannot pass."""
    import mi355attn
    from mi355attn import functional as F
    io = CC.IO[dtype]
    m = CC.block_module(cid).cuda()
    x16 = CC.block_input(cid).to(dtype).cuda()
    g = torch.Generator().manual_seed(CC.SEED[cid] + 2)
    ctx16 = torch.randn(*x16.shape, generator=g).to(dtype).cuda()
    with torch.no_grad(), mi355attn.options(mlp_tt4=tt4):
        got, tags = _run(lambda t: F.proj_mlp_fused16(t, ctx16, m.proj, m.norm2, m.mlp.fc1, m.mlp.fc2), x16)
        y32 = F.mlp_fused(x16.float(), m.norm2, m.mlp.fc1, m.mlp.fc2, precision=io, ctx16=ctx16, proj=m.proj)
    want = y32.to(dtype)
    assert got.dtype == dtype and got.shape == x16.shape and any("proj,x16>" in t for t in tags), tags
    assert torch.equal(got, want), f"{cid} {dtype}: {int((got != want).sum())} of {got.numel()} elements differ, {_ulps(got, want)} ulp"
    dropped = _ulps(got, (y32 - x16.float()).to(dtype))
    print(f"[cswin_io16] proj_mlp_fused16 {cid} {dtype} tt4={tt4}: {dropped} ulp from the value without the residual")
    assert dropped > 16
    _status()


# ---- check 3: refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", CC.DTYPES, ids=IDS)
def test_refusals_leave_the_output_as_it_was(dtype):
    from mi355attn import _ffi
    io, lib, P = CC.IO[dtype], _ffi.lib(), ctypes.c_void_p
    B, reso, C = 2, 8, 128
    M = B * reso * reso
    z16 = torch.zeros(M * C + 64, dtype=dtype, device="cuda")
    w16 = torch.zeros(4 * C * C + 64, dtype=dtype, device="cuda")
    f32 = torch.zeros(4 * C + 64, device="cuda")
    out = torch.full((M * C + 64,), 3.0, dtype=dtype, device="cuda")
    st = _ffi.stream_ptr(out.device)
    z, w, f, o = z16.data_ptr(), w16.data_ptr(), f32.data_ptr(), out.data_ptr()

    def stripe(x=z, wq=w, ctx=o, c=64, hb=1, r=reso, split=2, prec=io):
        return lib.mi355_cswin_stripe_attn_x16_fwd(P(x), P(wq), P(f), P(f), P(f), P(f), P(f), P(ctx), B, r, c, hb, split, 32 ** -0.5, 1e-5, prec, st)

    def mlp(x=z, ctx=z, y=o, wp=w, c=64, hidden=256, prec=io):
        return lib.mi355_proj_mlp_fused_x16_fwd(P(x), P(ctx), P(wp), P(f), P(w), P(f), P(w), P(f), P(None), P(y), M, c, hidden, 1, 1e-5, prec, st)
    assert stripe(x=None) == -1 and stripe(wq=None) == -1 and stripe(ctx=None) == -1 and stripe(prec=0) == -1 and stripe(prec=3) == -1
    assert stripe(x=z + 8) == -2 and stripe(ctx=o + 8) == -2 and stripe(c=96) == -2
    assert stripe(r=16, split=8) == -2 and b"tokens = 128" in lib.mi355_last_error()               # more than 64 tokens per stripe
    assert mlp(x=None) == -1 and mlp(ctx=None) == -1 and mlp(y=None) == -1 and mlp(wp=None) == -1 and mlp(prec=0) == -1 and mlp(prec=3) == -1
    assert mlp(x=z + 8) == -2 and mlp(ctx=z + 8) == -2 and mlp(y=o + 8) == -2
    assert mlp(c=96, hidden=384) == -2 and mlp(c=64, hidden=128) == -2 and mlp(c=128, hidden=256) == -2          # C = 96, hidden != 4 C
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()), "a refused call wrote its output"
    _status()


# ---- check 4: fp32 neighbours --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["c64_r6_s2", "c128_r6_s3", "c256_r7_s7"])
def test_fp32_forward_keeps_bits_and_tags_around_16bit_calls(cid):
    m = CC.block_module(cid).cuda()
    x = CC.block_input(cid).cuda()
    _run(m, x)                                                             # the weights' 16-bit copies are made here, once
    before, tags0 = _run(m, x)
    for dtype in CC.DTYPES:
        _run(m, x.to(dtype))
    after, tags1 = _run(m, x)
    assert before.dtype == torch.float32 and torch.equal(before, after) and sorted(tags0) == sorted(tags1)
    assert not any(k in t for t in tags0 for k in ("x16", "widen16", "round16", "gemm16_res")), tags0
    _status()


# ---- check 5: range ------------------------------------------------------------------------------------------------------------------
def test_saturating_y_warns_once_and_returns_the_strict_result():
    """y leaves fp16 while no operand does: one element of x at 64992 (an fp16 value) and proj.bias at 1024 for that channel put x1, and
    with it y, at about 66016 for one (token, channel); LayerNorm sees an ordinary row.  The fused kernel reports its store (code 3):
    exactly one warning, then the strict re-run -- widen, the precision-0 body, round -- whose bits are those of the precision-0 module
    on x16.float() rounded once, inf where the fp32-I/O module's y rounds to inf.  bf16 holds the value: silence.  This saturates a
    number format; nothing faults."""
    cid = "c64_r6_s2"
    m = CC.block_module(cid)
    m.proj.bias[7] = 1024.0
    m = m.cuda()
    strict = CC.block_module(cid, precision=0)
    strict.load_state_dict(m.state_dict())
    strict = strict.cuda()
    x = CC.block_input(cid)
    x[0, 5, 7] = 64992.0
    x = x.cuda()
    with torch.no_grad():
        want = strict(x.half().float()).half()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            y = m(x.half())
        assert len(seen) == 1 and "re-running this forward in strict mode" in str(seen[0].message), [str(w.message) for w in seen]
        assert "mi355_proj_mlp_fused_x16_fwd" in str(seen[0].message), str(seen[0].message)          # range code 3: the 16-bit store
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            wide = m(x.half().float()).half()                              # the fp32-I/O module: nothing to report, y = 66016 is an fp32 value
        assert not seen, [str(w.message) for w in seen]
        inf = torch.isinf(wide)
        assert y.dtype == torch.float16 and torch.equal(y, want), f"{_ulps(y, want)} ulp from the strict result"
        assert bool(inf[0, 5, 7]) and int(inf.sum()) == 1 and torch.equal(torch.isinf(y), inf) and torch.equal(y[inf], wide[inf])
        print(f"[cswin_io16] range: {_ulps(y[~inf], wide[~inf])} ulp between the strict re-run and the fp32-I/O module at precision 1 (finite part)")
        assert_parity(y[~inf].float().cpu(), wide[~inf].double().cpu(), TOL[1], "strict re-run vs the fp32-I/O module, finite part")
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            yb = m(x.bfloat16())
        assert not seen and yb.dtype == torch.bfloat16 and torch.isfinite(yb).all(), [str(w.message) for w in seen]
    _status()


# ---- check 6: LePEAttention, Merge_Block, the model, 16-bit parameters ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", CC.DTYPES, ids=IDS)
@pytest.mark.parametrize("idx,reso,split", [(0, 8, 2), (1, 8, 2), (-1, 7, 7)])
def test_lepe_attention_returns_the_type_of_qkv(idx, reso, split, dtype):
    from mi355attn.modules import LePEAttention
    from oracle.cswin import lepe_attention_forward
    from route_cases import prep_nontrivial
    io, C, heads, B = CC.IO[dtype], 64, 2, 2
    torch.manual_seed(9300 + idx)
    m = LePEAttention(C, reso, idx, split, num_heads=heads).eval().requires_grad_(False)
    prep_nontrivial(m)
    g = torch.Generator().manual_seed(9301)
    qkv = torch.randn(3, B, reso * reso, C, generator=g).to(dtype)
    ref = lepe_attention_forward(qkv.double(), m.get_v.weight, m.get_v.bias, reso, idx, split, heads, torch.float64).to(dtype)
    m = m.cuda()
    y, tags = _run(m, qkv.cuda())
    assert y.dtype == dtype and tuple(y.shape) == (B, reso * reso, C)
    assert not any(t.startswith(("widen16", "round16")) for t in tags), tags
    assert_parity(y.cpu(), ref, TOL[io], f"LePEAttention idx {idx} {dtype} vs fp64")
    m0 = copy.deepcopy(m)
    m0.precision = 0
    with torch.no_grad():
        y0, tags0 = _run(m0, qkv.cuda())
        want0 = m0(qkv.cuda().float()).to(dtype)
    assert y0.dtype == dtype and torch.equal(y0, want0), "precision 0 widens, runs the strict core and rounds"
    assert sum(t.startswith("widen16") for t in tags0) == 1 and sum(t.startswith("round16") for t in tags0) == 1, tags0
    _status()


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=IDS)
def test_merge_block_widens_and_rounds_once(dtype):
    import torch.nn.functional as TF

    from mi355attn.modules import Merge_Block
    from route_cases import prep_nontrivial
    io = CC.IO[dtype]
    torch.manual_seed(9400)
    m = Merge_Block(64, 128).eval().requires_grad_(False)
    prep_nontrivial(m)
    g = torch.Generator().manual_seed(9401)
    x16 = torch.randn(2, 64, 64, generator=g).to(dtype)
    grid = TF.conv2d(x16.double().transpose(1, 2).reshape(2, 64, 8, 8), m.conv.weight.double(), m.conv.bias.double(), stride=2, padding=1)
    ref = TF.layer_norm(grid.flatten(2).transpose(1, 2), (128,), m.norm.weight.double(), m.norm.bias.double(), m.norm.eps).to(dtype)
    m = m.cuda()
    y, tags = _run(m, x16.cuda())
    twin = copy.deepcopy(m)
    twin.precision = io
    with torch.no_grad():
        want = twin(x16.cuda().float()).to(dtype)
    assert y.dtype == dtype and tuple(y.shape) == (2, 16, 128) and torch.equal(y, want)
    assert sum(t.startswith("widen16") for t in tags) == 1 and sum(t.startswith("round16") for t in tags) == 1, tags
    assert_parity(y.cpu(), ref, TOL[io], f"Merge_Block {dtype} vs fp64")
    _status()


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=IDS)
def test_model_is_the_composition_of_its_parts(dtype):
    """m(img16) equals stem -> each block / merge -> LayerNorm -> token mean -> head -> .to(dtype) on 16-bit tensors bit for bit, and
    meets the fp64 emulation of that composition at TOL[io]; the distance to the unrounded oracle is printed."""
    from mi355attn import functional as F
    io = CC.IO[dtype]
    m = CC.model_module().cuda()
    img = CC.model_input().to(dtype).cuda()
    with torch.no_grad():
        m(img)
    y, tally = _traced(m, img)
    assert y.dtype == dtype and tuple(y.shape) == (CC.MODEL_SHAPE[0], CC.MODEL["num_classes"])
    with torch.no_grad():
        stem, ln = m.stage1_conv_embed[0], m.stage1_conv_embed[2]
        x, _ = F.conv2d_tokens(img.float(), stem.weight, stem.bias, 7, 4, 2, in_layout=0, precision=io)
        x = F.layernorm(x, ln.weight, ln.bias, ln.eps).to(dtype)
        for blk in m.stage1:
            x = blk(x)
        for pre, blocks in ((m.merge1, m.stage2), (m.merge2, m.stage3), (m.merge3, m.stage4)):
            x = pre(x)
            assert x.dtype == dtype
            for blk in blocks:
                x = blk(x)
                assert x.dtype == dtype
        pooled = F.token_mean16(F.layernorm16_x16(x, m.norm.weight, m.norm.bias, m.norm.eps))
        manual = F.linear(pooled, m.head.weight, m.head.bias, precision=io).to(dtype)
    assert pooled.dtype == torch.float32 and torch.equal(y, manual), f"{_ulps(y, manual)} ulp from the manual composition"
    plain, emu = CC.model_refs(dtype)
    print(f"[cswin_io16] model {dtype}: vs the emulated 16-bit composition rel_fro {rel_fro(y.cpu(), emu):.3e} max_abs_ratio "
          f"{max_abs_ratio(y.cpu(), emu):.3e} (bar {TOL[io]:g}); vs the unrounded oracle rel_fro {rel_fro(y.cpu(), plain):.3e} "
          f"max_abs_ratio {max_abs_ratio(y.cpu(), plain):.3e} (not gated); tally {sorted(tally.items())}")
    assert_parity(y.cpu(), emu, TOL[io], f"CSWinTransformer {dtype} vs the fp64 emulation of the 16-bit composition")
    assert _count(tally, "cswin_stripe_kernel<C=64,x16>") == 1 and _count(tally, "cswin_stripe_kernel<C=128,x16>") == 1, tally
    assert _count(tally, "mlp_fused_kernel<C=64,proj,x16>") == 1 and _count(tally, "mlp_fused_kernel<C=128,proj,x16>") == 1, tally
    assert _count(tally, "widen16_kernel") == 4 and _count(tally, "round16_kernel") == 4, "the stem and three merges widen and round"
    _status()


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=IDS)
@pytest.mark.parametrize("cid", ["c64_r6_s2", "c128_r6_s3", "c64_r8_s2_mlp2", "c256_r7_s7", "c32_r8_s8", "model"])
def test_16bit_parameters_give_the_bits_of_their_widened_values(cid, dtype):
    """fp32 parameters (autocast) and module.half() / .bfloat16() parameters of the same values give the same bits on every route; an
    in-place update of a 16-bit parameter is seen by the next forward."""
    if cid == "model":
        m16, x16 = CC.model_module().to(dtype).cuda(), CC.model_input().to(dtype).cuda()
        touch = lambda m: (m.stage1[0].proj.bias, m.stage2[0].norm1.weight, m.merge1.conv.weight)        # noqa: E731
    else:
        m16, x16 = CC.block_module(cid).to(dtype).cuda(), CC.block_input(cid).to(dtype).cuda()
        touch = lambda m: (m.mlp.fc2.bias, m.proj.weight, m.norm1.weight)                                 # noqa: E731
    m32 = copy.deepcopy(m16).float()                                       # the widened values, as fp32 parameters
    with torch.no_grad():
        a, b = m32(x16), m16(x16)
        assert a.dtype == b.dtype == dtype and torch.equal(a, b), f"{_ulps(a, b)} ulp between fp32 and 16-bit parameters"
        for m in (m16, m32):
            bias, weight, gain = touch(m)
            bias.mul_(2.0)
            weight.mul_(0.5)                                               # powers of two: exact in fp32 and in the 16-bit type alike
            gain.mul_(2.0)
        a2, b2 = m32(x16), m16(x16)
    assert torch.equal(a2, b2) and not torch.equal(a2, a), "the in-place update of a parameter was not seen"
    _status()
