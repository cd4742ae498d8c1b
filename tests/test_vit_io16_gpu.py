"""GPU tests (-m gpu): TransformerEncoder, vision_transformers.ViT.PatchEmbedding and VisionTransformer on fp16 / bf16 activations, and
the two entries under them (mi355_layernorm16_x16_fwd, mi355_linear16_res_fwd).  Shapes, seeds and the fp64 references (the oracle's
ViT restatement with the interface roundings applied) are tests/vit_io16_cases.py; a reference is computed once and shared.  Bars:
conftest.assert_parity at arena_cases.TOL[io] against fp64, 1 ulp of the I/O type against the fp32-I/O module (which runs the same
arithmetic on x16.float(): the 16-bit path may differ from it only in where the one rounding of y falls), bit equality against the
engine's fp32-residual route for the GEMM entry and against mi355_layernorm16_fwd for the LayerNorm entry."""
import copy
import functools
import warnings

import pytest
import torch

import vit_io16_cases as VC
from arena_cases import TOL, gelu64
from conftest import assert_parity, max_abs_ratio, rel_fro
from io16_common import _run, _status, _ulps

pytestmark = pytest.mark.gpu
IDS = ["fp16", "bf16"]
TNAME = {torch.float16: "f16", torch.bfloat16: "bf16"}
NEW_KERNELS = ("layernorm_x16_kernel", "gemm16_res_kernel")


def _x_sized_cast(tags, n):
    """Tags of mi355_cast16_fwd launches over n elements (weights are cast once, activations must never be)."""
    return [t for t in tags if t.startswith("cast16_kernel") and t.endswith(f"n={n}")]


@pytest.mark.parametrize("dtype", VC.DTYPES, ids=IDS)
@pytest.mark.parametrize("cid", list(VC.BLOCKS))
def test_block_on_16bit_activations(cid, dtype):
    """Check 1: the type of y (TypeError before the 16-bit path existed), 1 ulp against the fp32-I/O module, parity against the fp64
    oracle on x16 with y rounded once, and the kernels that ran.  The fp32-I/O twin runs at precision = io, the arithmetic of the 16-bit
    path whatever the module's setting; the strict case, where the 16-bit path widens, runs precision 0 and rounds, is held to bit
    equality with its precision-0 twin instead (its distance to the precision-io twin is printed: 16-bit against strict arithmetic)."""
    c, io = VC.BLOCKS[cid], VC.IO[dtype]
    m = VC.block_module(cid).cuda()
    x16 = VC.block_input(cid).to(dtype).cuda()
    y, tags = _run(m, x16)
    assert y.dtype == dtype and y.shape == x16.shape
    twin = VC.block_module(cid, precision=io).cuda()
    with torch.no_grad():
        y32 = twin(x16.float())
    assert y32.dtype == torch.float32
    ulps = _ulps(y, y32.to(dtype))
    ref = VC.block_emulated(cid, dtype)
    rf, ma = rel_fro(y.cpu(), ref), max_abs_ratio(y.cpu(), ref)
    print(f"[vit_io16] {cid} {dtype}: {ulps} ulp from the fp32-I/O module at precision {io}; vs fp64: rel_fro {rf:.3e} max_abs_ratio {ma:.3e} "
          f"(bar {TOL[io]:g}); tags {sorted(tags)}")
    if c.get("precision") == 0:
        with torch.no_grad():
            assert torch.equal(y, VC.block_module(cid).cuda()(x16.float()).to(dtype)), "the strict route is widen, precision 0, round"
    else:
        assert ulps <= 1, f"{cid}: {ulps} ulp from the fp32-I/O module rounded to {dtype}"
    assert_parity(y.cpu(), ref, TOL[io], f"{cid} {dtype} vs the fp64 oracle on x16, y rounded once")
    widen = [t for t in tags if t.startswith("widen16_kernel")]
    rnd = [t for t in tags if t.startswith("round16_kernel")]
    res = [t for t in tags if t.startswith("gemm16_res_kernel")]
    if c["fast"]:
        M, C = x16.shape[0] * x16.shape[1], c["C"]
        assert [t for t in tags if t.startswith("layernorm_x16_kernel")] == [f"layernorm_x16_kernel<{TNAME[dtype]}> rows={M} cols={C}"], tags
        assert sorted(res) == sorted([f"gemm16_res_kernel<{TNAME[dtype]},r16,o32> M={M} N={C} K={C}",
                                      f"gemm16_res_kernel<{TNAME[dtype]},r32,o16> M={M} N={C} K={4 * C} gelu"]), tags
        assert not widen and not rnd and not _x_sized_cast(tags, x16.numel()), tags
    else:
        assert len(widen) == 1 and widen[0].endswith(f"n={x16.numel()}") and len(rnd) == 1 and rnd[0].endswith(f"n={x16.numel()}"), tags
        assert not res and not any(t.startswith("layernorm_x16_kernel") for t in tags), tags
    _status()


# ---- check 2: the GEMM entry ---------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(394, 256, 256), (394, 256, 1024), (77, 72, 192), (33024 + 77, 512, 256)]


def _parity_dev(y, r, tol, what):
    """conftest.assert_parity with its two measures taken on the device (the largest shape holds 17 M outputs per combination)."""
    assert tuple(y.shape) == tuple(r.shape) and bool(torch.isfinite(y).all()), f"{what}: shape or non-finite output"
    y = y.double()
    rf, ma = float((y - r).norm() / r.norm().clamp_min(1e-300)), float((y - r).abs().max() / r.abs().max().clamp_min(1e-300))
    assert rf <= tol and ma <= tol, f"{what}: rel_fro={rf:.3e} max_abs_ratio={ma:.3e} (tol {tol:g})"
    return rf, ma


def _ulps_dev(a, b):
    """io16_common._ulps on the device."""
    def order(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return int((order(a) - order(b)).abs().max())


@functools.lru_cache(maxsize=None)
def _gemm_case(M, N, K, dtype):
    """Operands on the device and the fp64 product X W^T (without bias), computed once per (shape, type) on the device in fp64."""
    g = torch.Generator().manual_seed(M + N + K)
    x16 = torch.randn(M, K, generator=g).to(dtype).cuda()
    w16 = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).cuda()
    bias = (0.1 * torch.randn(N, generator=g)).cuda()
    r = (1.5 * torch.randn(M, N, generator=g)).cuda()
    return x16, w16, bias, r, x16.double() @ w16.double().t()


@pytest.mark.parametrize("dtype", VC.DTYPES, ids=IDS)
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_linear16_res_adds_in_fp32_and_rounds_once(M, N, K, dtype):
    """The three (residual, result) type pairs x act none / GELU x bias / no bias under gemm_splitk = 0: the fp32 result holds the bits of
    linear16(resid = r.float(), out16 = False), the 16-bit result those bits rounded once; both meet the fp64 product at TOL[io]; and
    the result is more than 16 ulp away from the product without the residual (an epilogue that dropped it, or rounded before adding
    it, is off by far more than 1 ulp: the residual is as large as the product)."""
    import mi355attn
    from mi355attn import functional as F
    io = VC.IO[dtype]
    x16, w16, bias, r32, prod = _gemm_case(M, N, K, dtype)
    with mi355attn.options(gemm_splitk=0):
        for act in (F.ACT_NONE, F.ACT_GELU):
            for b in (bias, None):
                z = prod if b is None else prod + b.double()
                z = gelu64(z) if act == F.ACT_GELU else z
                plain = F.linear16(x16, w16, b, act=act, out16=False, precision=io)
                for r16, o16 in ((True, False), (False, True), (True, True)):
                    r = r32.to(dtype) if r16 else r32
                    want32 = F.linear16(x16, w16, b, act=act, resid=r.float(), out16=False, precision=io)
                    got = F.linear16_res(x16, w16, b, r, act=act, out_dtype=dtype if o16 else torch.float32, precision=io)
                    what = f"{M}x{N}x{K} {dtype} r{16 if r16 else 32} o{16 if o16 else 32} act {act} bias {b is not None}"
                    assert got.dtype == (dtype if o16 else torch.float32) and tuple(got.shape) == (M, N), what
                    want = want32.to(dtype) if o16 else want32
                    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {got.numel()} elements differ from the engine's bits"
                    rf, ma = _parity_dev(got, z + r.double(), TOL[io], what + " vs fp64")
                    dropped = _ulps_dev(got.to(dtype), plain.to(dtype))
                    print(f"[vit_io16] linear16_res {what}: rel_fro {rf:.3e} max_abs_ratio {ma:.3e}; {dropped} ulp from the product alone")
                    assert dropped > 16, what
    _status()


# ---- check 3: the LayerNorm entry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", VC.DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,cols", [(5, 64), (394, 768), (33, 384), (300, 384), (1000, 768), (802, 64), (33, 128), (9, 52)])
def test_layernorm16_x16_has_the_bits_of_layernorm16_on_the_widened_rows(rows, cols, dtype):
    from mi355attn import functional as F
    g = torch.Generator().manual_seed(rows + cols)
    x16 = (torch.randn(rows, cols, generator=g) * 2 + 0.5).to(dtype).cuda()
    w, b = (0.5 + torch.rand(cols, generator=g)).cuda(), (0.2 * torch.randn(cols, generator=g)).cuda()
    got = F.layernorm16_x16(x16, w, b, 1e-5)
    want = F.layernorm16(x16.float(), w, b, 1e-5, VC.IO[dtype])
    assert got.dtype == dtype and torch.equal(got, want), f"{_ulps(got, want)} ulp from layernorm16 on the widened rows"
    ref = torch.nn.functional.layer_norm(x16.double(), (cols,), w.double(), b.double(), 1e-5)
    assert_parity(got.cpu(), ref.cpu(), TOL[VC.IO[dtype]], f"layernorm16_x16 {rows}x{cols} {dtype} vs fp64")
    _status()


# ---- checks 4 .. 8 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", VC.DTYPES, ids=IDS)
@pytest.mark.parametrize("cid", ["c256_h4_n50_b3", "c192_h4_n50"])
def test_16bit_parameters_give_the_bits_of_their_widened_values(cid, dtype):
    """Check 4: fp32 parameters (autocast) and module.half() / .bfloat16() parameters of the same values give the same bits, on the fast
    and on the widening route; an in-place update of a 16-bit parameter is seen by the next forward."""
    m16 = VC.block_module(cid).to(dtype).cuda()
    m32 = copy.deepcopy(m16).float()                                       # the widened values, as fp32 parameters
    x16 = VC.block_input(cid).to(dtype).cuda()
    with torch.no_grad():
        a, b = m32(x16), m16(x16)
        assert a.dtype == b.dtype == dtype and torch.equal(a, b), f"{_ulps(a, b)} ulp between fp32 and 16-bit parameters"
        for m in (m16, m32):
            m.mlp.fc2.bias.mul_(2.0)
            m.attn.proj.weight.mul_(0.5)                                   # powers of two: exact in fp32 and in the 16-bit type alike
            m.layernorm1.weight.mul_(2.0)
        a2, b2 = m32(x16), m16(x16)
    assert torch.equal(a2, b2) and not torch.equal(a2, a), "the in-place update of a parameter was not seen"
    _status()


def test_fp32_forward_keeps_bits_and_tags_around_16bit_calls():
    """Check 5."""
    m = VC.block_module("c256_h4_n50_b3").cuda()
    x = VC.block_input("c256_h4_n50_b3").cuda()
    _run(m, x)                                                             # the weights' 16-bit copies are made here, once
    before, tags0 = _run(m, x)
    for dtype in VC.DTYPES:
        _run(m, x.to(dtype))
    after, tags1 = _run(m, x)
    assert before.dtype == torch.float32 and torch.equal(before, after) and sorted(tags0) == sorted(tags1)
    assert not any(k in t for t in tags0 for k in NEW_KERNELS + ("widen16", "round16")), tags0
    _status()


@pytest.mark.parametrize("dtype", VC.DTYPES, ids=IDS)
def test_each_image_is_independent_of_its_batch(dtype):
    """Check 6: every image of the B = 3 case equals its B = 1 run, bit for bit."""
    m = VC.block_module("c256_h4_n50_b3").cuda()
    x16 = VC.block_input("c256_h4_n50_b3").to(dtype).cuda()
    with torch.no_grad():
        y = m(x16)
        for i in range(x16.shape[0]):
            assert torch.equal(y[i:i + 1], m(x16[i:i + 1].contiguous())), f"image {i} depends on the batch around it"
    _status()


def test_saturating_layernorm_warns_once_and_returns_the_strict_result():
    """Check 7: layernorm1.bias[5] = 7e4 saturates the fp16 LN operand for every token (range code 2).  fp16: exactly one warning, and
    the strict result rounded once.  bf16: silence."""
    m = VC.block_module("c256_h4_n50_b3")
    m.layernorm1.bias[5] = 7.0e4
    m = m.cuda()
    strict = VC.block_module("c256_h4_n50_b3", precision=0)
    strict.load_state_dict(m.state_dict())
    strict = strict.cuda()
    x = VC.block_input("c256_h4_n50_b3").cuda()
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
    """Check 8, one fp16 block."""
    m = VC.block_module("c384_h6_n197").cuda()
    static_x = VC.block_input("c384_h6_n197").half().cuda()
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


# ---- check 9: the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", VC.DTYPES, ids=IDS)
@pytest.mark.parametrize("mid", list(VC.MODELS))
def test_model_is_the_composition_of_its_parts(mid, dtype):
    """m(img16) equals embed -> each block -> pooled row -> head -> .to(dtype) on 16-bit tensors bit for bit, and meets the fp64 oracle
    with the interface roundings applied at TOL[io]; the distance to the unrounded oracle is printed."""
    import mi355attn
    from mi355attn import functional as F
    io = VC.IO[dtype]
    m = VC.model_module(mid).cuda()
    img = VC.model_input(mid).to(dtype).cuda()
    B, _, H, W = img.shape
    ps, E = VC.MODEL["patch_size"], VC.MODEL["embedding_dim"]
    n_tok = (H // ps) * (W // ps) + 1
    outs = []
    with torch.no_grad():
        rows = mi355attn.kernel_trace(lambda: outs.append(m(img)))          # (tag, launches, ...) per distinct tag
    y, tags, count = outs[0], [r[0] for r in rows], {r[0]: r[1] for r in rows}
    assert y.dtype == dtype and tuple(y.shape) == (B, VC.MODEL["num_classes"])
    with torch.no_grad():
        pos = F.vit_pos_table(m.position_embedding, ps, H, W)
        tok32 = F.patch_embed(img.float(), m.patch_embedding.proj.weight, m.patch_embedding.proj.bias, m.cls_token.reshape(-1), pos, ps, io)
        x = tok32.to(dtype)
        assert tuple(x.shape) == (B, n_tok, E)
        for blk in m.blocks:
            x = blk(x)
            assert x.dtype == dtype
        pooled = x[:, 0].float() if VC.MODELS[mid]["global_pool"] == "token" else F.token_mean16(x, skip_first=1)
        manual = F.linear(pooled, m.head.weight, m.head.bias, precision=io).to(dtype)
        if VC.MODELS[mid]["global_pool"] == "avg":
            assert_parity(pooled.cpu(), x[:, 1:].double().mean(1).cpu(), 1e-6, "token_mean16(skip_first=1) vs fp64")
    assert pooled.dtype == torch.float32 and torch.equal(y, manual), f"{_ulps(y, manual)} ulp from the manual composition"
    plain, emu = VC.model_refs(mid, dtype)
    print(f"[vit_io16] model {mid} {dtype}: vs the emulated 16-bit composition rel_fro {rel_fro(y.cpu(), emu):.3e} max_abs_ratio "
          f"{max_abs_ratio(y.cpu(), emu):.3e} (bar {TOL[io]:g}); vs the unrounded oracle rel_fro {rel_fro(y.cpu(), plain):.3e} "
          f"max_abs_ratio {max_abs_ratio(y.cpu(), plain):.3e} (not gated)")
    assert_parity(y.cpu(), emu, TOL[io], f"VisionTransformer {mid} {dtype} vs the fp64 oracle with the interface roundings")
    assert sum(n for t, n in count.items() if t.startswith(f"gemm16_res_kernel<{TNAME[dtype]}")) == 2 * VC.MODEL["depths"], count
    assert sum(n for t, n in count.items() if t.startswith("widen16_kernel")) == 1 and sum(n for t, n in count.items() if t.startswith("round16_kernel")) == 1, count
    assert not _x_sized_cast(tags, B * n_tok * E), tags                    # no cast launch over the token stream
    _status()


def test_patch_embedding_takes_a_16bit_image():
    """vision_transformers.ViT.PatchEmbedding does what mlps.mlp_mixer.PatchEmbedding does: the same tokens, in the type of the image."""
    from mi355attn.modules import PatchEmbedding
    from mi355attn.modules.mixer import PatchEmbedding as MixerEmbedding
    torch.manual_seed(8601)
    a = PatchEmbedding(64, 16, 3, 128).eval().requires_grad_(False).cuda()
    b = MixerEmbedding(64, 16, 3, 128).eval().requires_grad_(False).cuda()
    b.load_state_dict(a.state_dict())
    img = VC.model_input("token_64").cuda()
    for dtype in VC.DTYPES:
        with torch.no_grad():
            ya, yb = a(img.to(dtype)), b(img.to(dtype))
        assert ya.dtype == dtype and tuple(ya.shape) == (2, 16, 128) and torch.equal(ya, yb)
    _status()


# ---- check 10: refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", VC.DTYPES, ids=IDS)
def test_refusals_leave_the_output_as_it_was(dtype):
    import ctypes

    from mi355attn import _ffi
    io, lib, P = VC.IO[dtype], _ffi.lib(), ctypes.c_void_p
    M, N, K = 70, 72, 192
    x16, w16 = torch.zeros(M, K + 8, dtype=dtype, device="cuda"), torch.zeros(N + 8, K, dtype=dtype, device="cuda")
    r, bias = torch.zeros(M, N, dtype=dtype, device="cuda"), torch.zeros(N, device="cuda")
    y = torch.full((M, N), 3.0, dtype=dtype, device="cuda")
    st = _ffi.stream_ptr(y.device)

    def call(x=x16.data_ptr(), w=w16.data_ptr(), b=bias.data_ptr(), res=r.data_ptr(), rio=io, out=y.data_ptr(), oio=io, n=N, k=K, prec=io):
        return lib.mi355_linear16_res_fwd(P(x), P(w), P(b), P(res), rio, P(out), oio, M, n, k, k, n, 0, prec, st)
    assert call(prec=0) == -1 and call(prec=3) == -1 and call(rio=3 - io) == -1 and call(oio=3 - io) == -1        # bad type codes
    assert call(x=None) == -1 and call(w=None) == -1 and call(res=None) == -1 and call(out=None) == -1           # NULL pointers
    assert call(k=K + 8) == -2 and call(n=N + 4) == -2                                                           # K % 64, N % 8
    assert call(x=x16.data_ptr() + 8) == -2 and call(res=r.data_ptr() + 8) == -2 and call(out=y.data_ptr() + 8) == -2 and call(b=bias.data_ptr() + 4) == -2
    assert call(rio=0, oio=0) == -2                                                                               # the all-fp32 pair
    xl, yl = torch.zeros(5, 64, dtype=dtype, device="cuda"), torch.full((5, 64), 3.0, dtype=dtype, device="cuda")
    wl = torch.ones(64, device="cuda")

    def ln(x=xl.data_ptr(), out=yl.data_ptr(), code=io, cols=64):
        return lib.mi355_layernorm16_x16_fwd(P(x), P(wl.data_ptr()), P(wl.data_ptr()), P(out), 5, cols, 1e-5, code, st)
    assert ln(code=0) == -1 and ln(code=3) == -1 and ln(x=None) == -1 and ln(out=None) == -1 and ln(cols=0) == -1
    assert ln(x=xl.data_ptr() + 1) == -2 and ln(out=yl.data_ptr() + 1) == -2
    torch.cuda.synchronize()
    assert bool((y == 3.0).all()) and bool((yl == 3.0).all()), "a refused call wrote its output"
    _status()
