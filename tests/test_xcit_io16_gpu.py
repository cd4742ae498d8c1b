"""GPU tests (-m gpu): XCA, LPI, Mlp, XCABlock, ClassAttention(Block), ConvPatchEmbed and XCiT on fp16 / bf16 activations, and the three
entries under the block (mi355_linear16_res_scale_fwd, mi355_linear16_stats_r16_fwd, mi355_mlp_fused_o16_fwd).  Shapes, seeds and the fp64
references (the oracle's XCiT restatement with the interface roundings applied) are tests/xcit_io16_cases.py; a reference is computed
once and shared.  Bars: conftest.assert_parity at arena_cases.TOL[io] against fp64; 1 ulp of the I/O type against the fp32-I/O module
on the routes whose arithmetic between load and store is the same code (0 is expected and the count is printed); bit equality of each
entry against its fp32 sibling."""
import copy
import ctypes
import warnings

import pytest
import torch

import xcit_io16_arena_rows  # noqa: F401  (registers the arena rows of the three entries)
import xcit_io16_cases as XC
from arena_cases import TOL
from conftest import assert_parity, max_abs_ratio, rel_fro
from io16_common import _run, _status, _ulps

pytestmark = pytest.mark.gpu
IDS = ["fp16", "bf16"]
TNAME = {torch.float16: "f16", torch.bfloat16: "bf16"}
NEW_FORMS = ("resid16", ",scale>", ",o16>")


def _traced(fn, opts=None):
    """(output, {tag: launches}) of one call."""
    import mi355attn
    outs = []
    with torch.no_grad(), mi355attn.options(**(opts or {})):
        rows = mi355attn.kernel_trace(lambda: outs.append(fn()))
    tally = {}
    for tag, count, *_ in rows:
        tally[tag] = tally.get(tag, 0) + count
    return outs[0], tally


def _count(tally, prefix, suffix=""):
    return sum(n for t, n in tally.items() if t.startswith(prefix) and t.endswith(suffix))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- check 1: the block --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", XC.DTYPES, ids=IDS)
@pytest.mark.parametrize("cid", list(XC.BLOCKS))
def test_block_on_16bit_activations(cid, dtype):
    """The type of y (TypeError before the 16-bit path existed), parity against the fp64 oracle on x16 with y rounded once, the distance
    to the fp32-I/O module at precision = io, and the kernels that ran (counted on the second forward: the first one prepares the
    weights' 16-bit copies)."""
    import mi355attn
    c, io = XC.BLOCKS[cid], XC.IO[dtype]
    route, opts = XC.route(cid, dtype), c.get("opts", {})
    H, W = c["hw"]
    m = XC.block_module(cid).cuda()
    x16 = XC.block_input(cid).to(dtype).cuda()
    with torch.no_grad(), mi355attn.options(**opts):
        m(x16, H, W)
    y, tally = _traced(lambda: m(x16, H, W), opts)
    assert y.dtype == dtype and y.shape == x16.shape
    twin = XC.block_module(cid, precision=c.get("precision", io)).cuda()
    with torch.no_grad(), mi355attn.options(**opts):
        y32 = twin(x16.float(), H, W)
    assert y32.dtype == torch.float32
    ulps = _ulps(y, y32.to(dtype))
    ref = XC.block_emulated(cid, dtype)
    rf, ma = rel_fro(y.cpu(), ref), max_abs_ratio(y.cpu(), ref)
    print(f"[xcit_io16] {cid} {dtype} route {route}: {ulps} ulp from the fp32-I/O module at precision {c.get('precision', io)}; vs fp64: "
          f"rel_fro {rf:.3e} max_abs_ratio {ma:.3e} (bar {TOL[io]:g}); tally {sorted(tally.items())}")
    assert_parity(y.cpu(), ref, TOL[io], f"{cid} {dtype} vs the fp64 oracle on x16, y rounded once")
    B, N, C = x16.shape
    M, n, t, hidden = B * N, x16.numel(), TNAME[dtype], m.mlp.fc1.out_features
    if route == "W":
        assert _count(tally, "widen16_kernel") == 1 == _count(tally, "widen16_kernel", f"n={n}"), tally
        assert _count(tally, "round16_kernel") == 1 == _count(tally, "round16_kernel", f"n={n}"), tally
        assert not any(k in tag for tag in tally for k in NEW_FORMS + ("x16",)), tally
        assert torch.equal(y, y32.to(dtype)), f"route W is widen, the fp32 body, round: {ulps} ulp"
        _status()
        return
    assert not _count(tally, "widen16_kernel") and not _count(tally, "round16_kernel") and not _count(tally, "cast16_kernel", f"n={n}"), tally
    assert tally.get(f"layernorm_x16_kernel<{t}> rows={M} cols={C}") == 1, tally
    assert _count(tally, "xca_") == 1, tally                   # one core launch, on the 16-bit qkv
    assert _count(tally, "gemm16_res_kernel") + _count(tally, "gemm16_wreg_kernel") + _count(tally, "mlp_fused_kernel") == 2, tally
    if N > 256:
        assert _count(tally, "lpi_tile_kernel") >= 1, tally
    if route == "G-stats":
        assert tally.get(f"gemm16_wreg_kernel<{t},resid16+stats> M={M} N={C} K={C}") == 1 and _count(tally, "gemm16_wreg_kernel") == 1, tally
        assert tally.get(f"gemm16_res_kernel<{t},r32,o16> M={M} N={C} K={hidden}") == 1 and _count(tally, "gemm16_res_kernel") == 1, tally
    elif route == "G":
        scale = ",scale" if cid == "c256_eta" else ""          # fp16 at eta = 1e-5: the fold is refused, gamma runs in both epilogues
        assert tally.get(f"gemm16_res_kernel<{t},r16,o32{scale}> M={M} N={C} K={C}") == 1, tally
        assert tally.get(f"gemm16_res_kernel<{t},r32,o16{scale}> M={M} N={C} K={hidden}") == 1 and _count(tally, "gemm16_res_kernel") == 2, tally
    else:
        assert tally.get(f"mlp_fused_kernel<C={C},o16> M={M}") == 1 and _count(tally, "mlp_fused_kernel") == 1, tally
        assert tally.get(f"gemm16_res_kernel<{t},r16,o32> M={M} N={C} K={C}") == 1 and _count(tally, "gemm16_res_kernel") == 1, tally
    if route in ("G", "G-stats"):                             # no LayerNorm fold in the fp32 twin at these widths: the same arithmetic
        assert ulps <= 1, f"{cid}: {ulps} ulp from the fp32-I/O module rounded to {dtype}"
    else:                                                     # the twin folds LayerNorm 1 into the qkv weights (ln_linear16): parity only
        assert_parity(y.float().cpu(), y32.double().cpu(), TOL[io], f"{cid} {dtype} vs the fp32-I/O module")
    _status()


# ---- check 2: the entries against their fp32 siblings, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", XC.DTYPES, ids=IDS)
@pytest.mark.parametrize("N,K", [(192, 192), (256, 1024)])
@pytest.mark.parametrize("pair", ["r16_o32", "r32_o16"])
def test_res_scale_entry_has_the_bits_of_linear16(pair, N, K, dtype):
    from mi355attn import functional as F
    io, M = XC.IO[dtype], 105
    g = _gen(9801 + N)
    x = torch.randn(M, K, generator=g).to(dtype).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).cuda()
    b = (0.1 * torch.randn(N, generator=g)).cuda()
    gam = (0.5 + torch.rand(N, generator=g)).cuda()
    r = (1.5 * torch.randn(M, N, generator=g))
    r = (r.to(dtype) if pair == "r16_o32" else r).cuda()
    out = torch.float32 if pair == "r16_o32" else dtype
    with torch.no_grad():
        for gamma in (gam, None):
            got, tally = _traced(lambda: F.linear16_res_scale(x, w, b, gamma, r, out_dtype=out, precision=io))
            want = F.linear16(x, w, b, gamma=gamma, resid=r.float(), precision=io).to(out)
            tag = f"gemm16_res_kernel<{TNAME[dtype]},{pair.replace('_', ',')}{',scale' if gamma is not None else ''}> M={M} N={N} K={K}"
            assert tally == {tag: 1}, tally
            assert got.dtype == out and torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} elements differ"
            if gamma is None:
                assert torch.equal(got, F.linear16_res(x, w, b, r, out_dtype=out, precision=io)), "a null gamma is linear16_res"
                plain = got
        scaled = F.linear16_res_scale(x, w, b, gam, r, out_dtype=out, precision=io)
        far = _ulps(scaled.to(dtype), plain.to(dtype))
        print(f"[xcit_io16] linear16_res_scale {pair} {N}x{K} {dtype}: {far} ulp between the scaled and the unscaled result")
        assert far > 16, "a dropped scale cannot pass"
    _status()


@pytest.mark.parametrize("dtype", XC.DTYPES, ids=IDS)
@pytest.mark.parametrize("M,N", [(105, 256), (105, 384), (392, 256), (392, 384)])
def test_stats_r16_entry_has_the_bits_of_the_fp32_residual_entry(M, N, dtype):
    from mi355attn import functional as F
    io = XC.IO[dtype]
    g = _gen(9811 + M + N)
    x = torch.randn(M, N, generator=g).to(dtype).cuda()
    w = (torch.randn(N, N, generator=g) / N ** 0.5).to(dtype).cuda()
    b = (0.1 * torch.randn(N, generator=g)).cuda()
    r16 = (1.5 * torch.randn(M, N, generator=g) + 0.3).to(dtype).cuda()
    with torch.no_grad():
        (y, st), tally = _traced(lambda: F.linear16_stats_r16(x, w, b, r16, 1e-6, precision=io))
        y32, st32 = F.linear16_stats(x, w, b, r16.float(), 1e-6, precision=io)
    assert tally == {f"gemm16_wreg_kernel<{TNAME[dtype]},resid16+stats> M={M} N={N} K={N}": 1}, tally
    assert y.dtype == torch.float32 and torch.equal(y, y32) and torch.equal(st, st32), (int((y != y32).sum()), int((st != st32).sum()))
    assert not torch.equal(y, y32 - r16.float()), "the residual was added"
    _status()


@pytest.mark.parametrize("dtype", XC.DTYPES, ids=IDS)
@pytest.mark.parametrize("C,tt4", [(64, 0), (64, 1), (128, 0)])
def test_mlp_o16_entry_rounds_the_fp32_entrys_y_once(C, tt4, dtype):
    """y16 is the fp32 entry's y rounded once -- bit for bit -- and more than 16 ulp away from that y without the residual x: an epilogue
    that dropped x, or rounded before adding it, cannot pass."""
    import mi355attn
    from mi355attn import functional as F
    io, M = XC.IO[dtype], 105
    m = XC.block_module("c64_h2" if C == 64 else "c128_h4").cuda()
    x = (torch.randn(M, C, generator=_gen(9821 + C)) * 1.3 + 0.2).cuda()
    with torch.no_grad(), mi355attn.options(mlp_tt4=tt4):
        F.mlp_fused_o16(x, m.norm2, m.mlp.fc1, m.mlp.fc2, precision=io)      # the folded 16-bit weights are made here, once
        for gamma in (m.gamma2, None):
            got, tags = _run(lambda t: F.mlp_fused_o16(t, m.norm2, m.mlp.fc1, m.mlp.fc2, gamma=gamma, precision=io), x)
            y32 = F.mlp_fused(x, m.norm2, m.mlp.fc1, m.mlp.fc2, gamma=gamma, precision=io)
            want = y32.to(dtype)
            assert got.dtype == dtype and got.shape == x.shape and tags == [f"mlp_fused_kernel<C={C},o16> M={M}"], tags
            assert torch.equal(got, want), f"C={C} {dtype}: {int((got != want).sum())} of {got.numel()} elements differ, {_ulps(got, want)} ulp"
            dropped = _ulps(got, (y32 - x).to(dtype))
            print(f"[xcit_io16] mlp_fused_o16 C={C} {dtype} tt4={tt4} gamma={gamma is not None}: {dropped} ulp from the value without the residual")
            assert dropped > 16
    _status()


@pytest.mark.parametrize("dtype", XC.DTYPES, ids=IDS)
@pytest.mark.parametrize("pattern", ["pad", "block"])
@pytest.mark.parametrize("entry", ["res_scale", "stats_r16"])
def test_gemm_entries_on_strided_rows(entry, pattern, dtype):
    """The stride patterns of tests/gemm_ld_cases.py for the two new GEMM entries: rows padded by the smallest stride the header allows
    (+ 8 elements), and the operand as column block 1 of a matrix three times as wide.  Every buffer is poisoned around its live columns;
    the strided call returns the bits of the dense call and writes nothing else."""
    from mi355attn import _ffi
    io, lib, P = XC.IO[dtype], _ffi.lib(), ctypes.c_void_p
    M, N, K = (70, 72, 128) if entry == "res_scale" else (100, 256, 256)
    g = _gen(9861)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).cuda()
    b = (0.1 * torch.randn(N, generator=g)).cuda()
    gam = (0.5 + torch.rand(N, generator=g)).cuda()
    r = (1.5 * torch.randn(M, N, generator=g)).to(dtype)
    ydt = dtype if entry == "res_scale" else torch.float32
    stream = _ffi.stream_ptr(torch.device("cuda", 0))

    def call(ldx, ldy, cx, cy):
        """The entry on x, resid and y held as the columns [c, c + width) of poisoned matrices of row strides ldx, ldy."""
        X = torch.full((M, ldx), 777.0, dtype=dtype, device="cuda")
        R = torch.full((M, ldy), -555.0, dtype=dtype, device="cuda")
        Y = torch.full((M, ldy), 3.0, dtype=ydt, device="cuda")
        X[:, cx:cx + K], R[:, cy:cy + N] = x.cuda(), r.cuda()
        st = torch.full((M, 2), 3.0, device="cuda")
        px, pr, py = (P(t.data_ptr() + c * t.element_size()) for t, c in ((X, cx), (R, cy), (Y, cy)))
        if entry == "res_scale":
            rc = lib.mi355_linear16_res_scale_fwd(px, P(w.data_ptr()), P(b.data_ptr()), P(gam.data_ptr()), pr, io, py, io, M, N, K, ldx, ldy, 1, io, stream)
        else:
            rc = lib.mi355_linear16_stats_r16_fwd(px, P(w.data_ptr()), P(b.data_ptr()), pr, py, M, N, K, ldx, ldy, io, P(st.data_ptr()), 1e-6, stream)
        assert rc == 0, lib.mi355_last_error()
        torch.cuda.synchronize()
        live = Y[:, cy:cy + N].clone()
        Y[:, cy:cy + N] = 3.0
        assert bool((Y == 3.0).all()), "the call wrote outside the live columns of Y"
        return live, st
    dense, st0 = call(K, N, 0, 0)
    got, st1 = call(*((K + 8, N + 8, 0, 0) if pattern == "pad" else (3 * K, 3 * N, K, N)))
    assert torch.equal(got, dense), f"{int((got != dense).sum())} of {got.numel()} elements differ from the dense call"
    if entry == "stats_r16":
        assert torch.equal(st0, st1) and not bool((st1 == 3.0).all())
    want = x.double() @ w.cpu().double().t() + b.cpu().double()
    if entry == "res_scale":
        want = 0.5 * want * (1.0 + torch.erf(want / 2.0 ** 0.5)) * gam.cpu().double()
    assert_parity(got.float().cpu(), want + r.double(), TOL[io], f"{entry} {pattern} {dtype} vs fp64")
    _status()


# ---- check 3: refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", XC.DTYPES, ids=IDS)
def test_refusals_leave_the_output_as_it_was(dtype):
    from mi355attn import _ffi
    io, lib, P = XC.IO[dtype], _ffi.lib(), ctypes.c_void_p
    M = 105
    z16 = torch.zeros(M * 1024 + 64, dtype=dtype, device="cuda")
    f32 = torch.zeros(M * 384 + 64, device="cuda")
    out = torch.full((M * 384 + 64,), 3.0, device="cuda")
    out16 = torch.full((M * 384 + 64,), 3.0, dtype=dtype, device="cuda")
    st = _ffi.stream_ptr(out.device)
    z, f, o, o16 = z16.data_ptr(), f32.data_ptr(), out.data_ptr(), out16.data_ptr()

    def scale(x=z, w=z, g=f, r=z, rio=io, y=o, oio=0, N=192, K=192, prec=io):
        return lib.mi355_linear16_res_scale_fwd(P(x), P(w), P(f), P(g), P(r), rio, P(y), oio, M, N, K, K, N, 0, prec, st)

    def stats(x=z, w=z, r=z, y=o, N=256, K=256, rows=M, prec=io, s=f):
        return lib.mi355_linear16_stats_r16_fwd(P(x), P(w), P(f), P(r), P(y), rows, N, K, K, N, prec, P(s), 1e-6, st)

    def mlp(x=f, w1=z, w2=z, y=o16, C=64, hidden=256, prec=io):
        return lib.mi355_mlp_fused_o16_fwd(P(x), P(w1), P(f), P(w2), P(f), P(f), P(y), M, C, hidden, 1, 1e-5, prec, st)
    assert scale(x=None) == -1 and scale(w=None) == -1 and scale(r=None) == -1 and scale(y=None) == -1 and scale(prec=0, rio=0) == -1 and scale(prec=3) == -1
    assert scale(x=z + 8) == -2 and scale(y=o + 8) == -2 and scale(g=f + 8) == -2 and scale(r=z + 8) == -2 and scale(rio=0, oio=0) == -2
    assert scale(y=o16, oio=io, x=z + 8) == -2 and scale(K=96) == -2
    assert stats(x=None) == -1 and stats(r=None) == -1 and stats(y=None) == -1 and stats(s=None) == -1 and stats(prec=0) == -1 and stats(prec=3) == -1
    assert stats(N=192, K=192) == -2 and b"N = K = 256 / 384" in lib.mi355_last_error()
    assert stats(r=z + 8) == -2 and stats(y=o + 8) == -2 and stats(x=z + 8) == -2 and stats(rows=31) == -2 and stats(s=f + 4) == -2
    assert mlp(x=None) == -1 and mlp(w1=None) == -1 and mlp(y=None) == -1 and mlp(prec=0) == -1 and mlp(prec=3) == -1
    assert mlp(x=f + 8) == -2 and mlp(y=o16 + 8) == -2 and mlp(w2=z + 8) == -2
    assert mlp(C=96, hidden=384) == -2 and b"C = 96" in lib.mi355_last_error() and mlp(C=256, hidden=1024) == -2 and mlp(C=64, hidden=128) == -2
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((out16 == 3.0).all()), "a refused call wrote its output"
    _status()


# ---- check 4: fp32 neighbours --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["c64_h2", "c256_h8", "c384_h8"])
def test_fp32_forward_keeps_bits_and_tags_around_16bit_calls(cid):
    H, W = XC.BLOCKS[cid]["hw"]
    m = XC.block_module(cid).cuda()
    x = XC.block_input(cid).cuda()
    fwd = lambda t: m(t, H, W)                                             # noqa: E731
    _run(fwd, x)                                                           # the weights' 16-bit copies are made here, once
    before, tags0 = _run(fwd, x)
    for dtype in XC.DTYPES:
        _run(fwd, x.to(dtype))
    after, tags1 = _run(fwd, x)
    assert before.dtype == torch.float32 and torch.equal(before, after) and sorted(tags0) == sorted(tags1)
    assert not any(k in t for t in tags0 for k in ("x16", "o16", "resid16", "widen16", "round16", "gemm16_res")), tags0
    _status()


# ---- check 5: range ------------------------------------------------------------------------------------------------------------------
def test_saturating_y_warns_once_and_returns_the_strict_result():
    """Only y leaves fp16: one element of x at 64992 (an fp16 value) and mlp.fc2.bias at 1024 for that channel put y at about 66016 for
    one (token, channel); every LayerNorm sees an ordinary row and x1, x2 are fp32.  The fused kernel reports its store (code 3):
    exactly one warning, then the strict re-run -- widen, the precision-0 body, round -- whose bits are those of the precision-0 module
    on x16.float() rounded once, inf where that has inf.  bf16 holds the value: silence.  This saturates a number format; nothing
    faults."""
    cid = "c64_h2"
    H, W = XC.BLOCKS[cid]["hw"]
    m = XC.block_module(cid)
    m.mlp.fc2.bias[7] = 1024.0 / float(m.gamma2[7])
    m = m.cuda()
    strict = XC.block_module(cid, precision=0)
    strict.load_state_dict(m.state_dict())
    strict = strict.cuda()
    x = XC.block_input(cid)
    x[0, 5, 7] = 64992.0
    x = x.cuda()
    with torch.no_grad():
        want = strict(x.half().float(), H, W).half()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            y = m(x.half(), H, W)
        assert len(seen) == 1 and "re-running this forward in strict mode" in str(seen[0].message), [str(w.message) for w in seen]
        assert "mi355_mlp_fused_o16_fwd" in str(seen[0].message), str(seen[0].message)             # range code 3: the 16-bit store
        inf = torch.isinf(want)
        assert y.dtype == torch.float16 and torch.equal(y, want), f"{_ulps(y, want)} ulp from the strict result"
        assert bool(inf[0, 5, 7]) and int(inf.sum()) == 1, "only the planted element leaves fp16"
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            yb = m(x.bfloat16(), H, W)
        assert not seen and yb.dtype == torch.bfloat16 and torch.isfinite(yb).all(), [str(w.message) for w in seen]
    _status()


# ---- check 6: the standalone modules -------------------------------------------------------------------------------------------------
def _standalone(kind):
    from mi355attn.modules import LPI, XCA, ClassAttentionBlock
    from mi355attn.modules.xcit import Mlp
    from route_cases import prep_nontrivial
    torch.manual_seed(9830)
    m = {"xca": lambda: XCA(128, 4, qkv_bias=True), "mlp": lambda: Mlp(128, 512), "lpi": lambda: LPI(128),
         "cab": lambda: ClassAttentionBlock(128, 4, qkv_bias=True, eta=1.0, tokens_norm=False),
         "cab_tn": lambda: ClassAttentionBlock(128, 4, qkv_bias=True, eta=1.0, tokens_norm=True)}[kind]().eval()
    prep_nontrivial(m)
    return m.requires_grad_(False)


@pytest.mark.parametrize("dtype", XC.DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["xca", "mlp", "lpi", "cab", "cab_tn"])
def test_standalone_modules_return_the_type_of_x(kind, dtype):
    import oracle.transformer as OT
    import oracle.xcit as OX
    io, B, H, W, C = XC.IO[dtype], 3, 5, 7, 128
    m = _standalone(kind)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    N = H * W + (1 if kind.startswith("cab") else 0)
    x16 = (torch.randn(B, N, C, generator=_gen(9831)) * 1.3 + 0.2).to(dtype)
    xd = x16.double()
    if kind == "xca":
        ref, args = OX.xca_forward(xd, sd, 4, torch.float64), ()
    elif kind == "mlp":
        h = OT.gelu(OT.linear(xd, sd["fc1.weight"].double(), sd["fc1.bias"].double()))
        ref, args = OT.linear(h, sd["fc2.weight"].double(), sd["fc2.bias"].double()), ()
    elif kind == "lpi":
        ref, args = OX.lpi_forward(xd, sd, H, W, torch.float64), (H, W)
    else:
        ref, args = OX.class_attention_block_forward(xd, sd, 4, torch.float64, tokens_norm=kind == "cab_tn"), (H, W)
    m = m.cuda()
    fwd = lambda t: m(t, *args)                                            # noqa: E731
    _run(fwd, x16.cuda())
    y, tags = _run(fwd, x16.cuda())
    assert y.dtype == dtype and tuple(y.shape) == tuple(ref.shape)
    assert_parity(y.cpu(), ref.to(dtype), TOL[io], f"{kind} {dtype} vs fp64, y rounded once")
    widens, rounds = sum(t.startswith("widen16") for t in tags), sum(t.startswith("round16") for t in tags)
    if kind in ("xca", "mlp"):
        assert widens == 0 == rounds, tags                                 # the GEMMs read x16 and store 16 bit themselves
    else:
        assert widens == 1 == rounds, tags
        twin = copy.deepcopy(m)
        for mod in twin.modules():
            if hasattr(mod, "precision"):
                mod.precision = io
        with torch.no_grad():
            want = twin(x16.cuda().float(), *args).to(dtype)
        assert torch.equal(y, want), f"{kind}: widen, the fp32 body at precision {io}, round: {_ulps(y, want)} ulp"
    _status()


@pytest.mark.parametrize("dtype", XC.DTYPES, ids=IDS)
def test_conv_patch_embed_returns_16bit_tokens(dtype):
    import oracle.xcit as OX
    from mi355attn.modules import ConvPatchEmbed
    from route_cases import prep_nontrivial
    io = XC.IO[dtype]
    torch.manual_seed(9840)
    m = ConvPatchEmbed(img_size=64, patch_size=16, embed_dim=64).eval().requires_grad_(False)
    prep_nontrivial(m)
    img = torch.randn(2, 3, 64, 64, generator=_gen(9841)).to(dtype)
    ref, hw = OX.conv_patch_embed_forward(img.double(), {k: v.detach().clone() for k, v in m.state_dict().items()}, torch.float64)
    m = m.cuda()
    (y, got_hw), tags = _run(m, img.cuda())
    assert y.dtype == dtype and tuple(y.shape) == (2, 16, 64) and tuple(got_hw) == tuple(hw) == (4, 4)
    assert sum(t.startswith("widen16") for t in tags) == 1 == sum(t.startswith("round16") for t in tags), tags
    assert_parity(y.cpu(), ref.to(dtype), TOL[io], f"ConvPatchEmbed {dtype} vs fp64, tokens rounded once")
    _status()


# ---- check 7: the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", XC.DTYPES, ids=IDS)
def test_model_is_the_composition_of_its_16bit_parts_then_the_fp32_tail(dtype):
    io = XC.IO[dtype]
    m = XC.model_module().cuda()
    img = XC.model_input().to(dtype).cuda()
    with torch.no_grad():
        m(img)
    y, tally = _traced(lambda: m(img))
    assert y.dtype == dtype and tuple(y.shape) == (XC.MODEL_SHAPE[0], XC.MODEL["num_classes"])
    plain, emu = XC.model_refs(dtype)
    print(f"[xcit_io16] model {dtype}: vs the emulated 16-bit composition rel_fro {rel_fro(y.cpu(), emu):.3e} max_abs_ratio "
          f"{max_abs_ratio(y.cpu(), emu):.3e} (bar {TOL[io]:g}); vs the unrounded oracle rel_fro {rel_fro(y.cpu(), plain):.3e} "
          f"max_abs_ratio {max_abs_ratio(y.cpu(), plain):.3e} (not gated); tally {sorted(tally.items())}")
    assert_parity(y.cpu(), emu, TOL[io], f"XCiT {dtype} vs the fp64 emulation of the 16-bit composition")
    n_img, n_tok = img.numel(), XC.MODEL_SHAPE[0] * 16 * XC.MODEL["embed_dim"]
    assert _count(tally, "widen16_kernel") == 2 and _count(tally, "widen16_kernel", f"n={n_img}") == 1 == _count(tally, "widen16_kernel", f"n={n_tok}"), tally
    assert _count(tally, "round16_kernel") == 1 == _count(tally, "round16_kernel", f"n={n_tok}"), "the embedding rounds its tokens; nothing else does"
    assert _count(tally, "mlp_fused_kernel<C=64,o16>") == XC.MODEL["depth"] == _count(tally, f"layernorm_x16_kernel<{TNAME[dtype]}>"), tally
    with torch.no_grad():                                                  # the composition, by hand
        pos = m.pos_embeder.tokens(4, 4)
        x, (Hp, Wp) = m.patch_embed(img, pos=pos)
        assert x.dtype == dtype
        for blk in m.blocks:
            x = blk(x, Hp, Wp)
            assert x.dtype == dtype
        twin = XC.model_module(precision=io).cuda()
        t = torch.cat([twin.cls_token.expand(x.shape[0], -1, -1), x.float()], dim=1)
        for blk in twin.cls_attn_blocks:
            t = blk(t, Hp, Wp)
        from mi355attn import functional as F
        cls = F.layernorm(t[:, 0].contiguous(), twin.norm.weight, twin.norm.bias, twin.norm.eps)
        manual = F.linear(cls, twin.head.weight, twin.head.bias, precision=io).to(dtype)
    assert torch.equal(y, manual), f"{_ulps(y, manual)} ulp from the manual composition"
    _status()


def test_nano_model_returns_finite_fp16_logits():
    from mi355attn.modules import xcit_nano_12_p16
    torch.manual_seed(9850)
    m = xcit_nano_12_p16(num_classes=10).eval().requires_grad_(False).cuda()
    img = torch.randn(1, 3, 64, 64, generator=_gen(9851)).half().cuda()
    with torch.no_grad():
        y = m(img)
    assert y.dtype == torch.float16 and tuple(y.shape) == (1, 10) and bool(torch.isfinite(y).all())
    _status()


# ---- check 8: 16-bit parameters ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", XC.DTYPES, ids=IDS)
@pytest.mark.parametrize("cid", ["c128_h4", "c256_h8"])
def test_16bit_parameters_give_the_bits_of_their_widened_values(cid, dtype):
    """module.half() / .bfloat16() parameters and fp32 parameters of the same (widened) values give the same bits; an in-place update of
    a 16-bit parameter is seen by the next forward."""
    H, W = XC.BLOCKS[cid]["hw"]
    m16 = copy.deepcopy(XC.block_module(cid)).to(dtype).cuda()
    x16 = XC.block_input(cid).to(dtype).cuda()
    m32 = copy.deepcopy(m16).float()                                       # the widened values, as fp32 parameters
    with torch.no_grad():
        a, b = m32(x16, H, W), m16(x16, H, W)
        assert a.dtype == b.dtype == dtype and torch.equal(a, b), f"{_ulps(a, b)} ulp between fp32 and 16-bit parameters"
        for m in (m16, m32):
            m.mlp.fc2.bias.mul_(2.0)
            m.attn.proj.weight.mul_(2.0)                                   # powers of two, upwards: exact in fp32 and in the 16-bit type alike
            m.norm1.weight.mul_(2.0)
        a2, b2 = m32(x16, H, W), m16(x16, H, W)
    assert torch.equal(a2, b2) and not torch.equal(a2, a), "the in-place update of a parameter was not seen"
    _status()


# ---- check 9: graph capture ----------------------------------------------------------------------------------------------------------
def test_block_replays_from_a_captured_graph():
    """One fp16 forward on route G-stats captured on a single stream after an eager warm-up (the weights' 16-bit copies and the
    LayerScale fold decision are made there), replayed twice: the eager bits."""
    cid = "c256_h8"
    H, W = XC.BLOCKS[cid]["hw"]
    m = XC.block_module(cid).cuda()
    x16 = XC.block_input(cid).half().cuda()
    with torch.no_grad():
        eager = m(x16, H, W).clone()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m(x16, H, W)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(x16, H, W)
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager), f"{_ulps(out, eager)} ulp between the replay and the eager forward"
    _status()
