"""The software-pipelined one-wave-per-SIMD weight-stationary GEMM (gemm16_wst.hip, gemm16_wst1_kernel: option `gemm_wst` = 3 / 4 and the
default route, `gemm_wst` = 5 / 6) against the tile kernels, bit for bit.

Row counts under `gemm_wst` = 4 (a workgroup walks every nstream-th 32-row tile of its slab, nstream = 256 CUs / slabs = 28 / 42 / 21 for
N = 2304 / 1536 / 3072): one tile in the whole launch, most streams empty (32, 64), streams of one and two tiles (32 * 28, 32 * 29, 32 * 57), the
pipeline's fill and drain and the first wrap of the three-tile ring (32 * 85: four tiles in the first stream at N = 2304 / 3072), and a model
shape (7424).  The operands are shared by all cases of a (precision, N) pair; the tile kernels' result is computed once per case."""
import pytest
import torch

from kernel_cases import _tags

pytestmark = pytest.mark.gpu

K = 768
MS = (32, 64, 32 * 28, 32 * 29, 32 * 57, 32 * 85, 7424)
WST = "gemm16_wst_kernel"
_OPERANDS = {}


def _operands(prec, N):
    from mi355attn import functional as F
    if (prec, N) not in _OPERANDS:
        g = torch.Generator(device="cuda").manual_seed(1000 * prec + N)
        x16 = F.cast16(torch.randn(max(MS), K, device="cuda", generator=g), prec)
        w16 = F.cast16((torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).contiguous(), prec)
        b = torch.randn(N, device="cuda", generator=g)
        _OPERANDS[(prec, N)] = (x16, w16, b)
    return _OPERANDS[(prec, N)]


def _tile(x16, w16, b, act, prec):
    """The tile kernels: `gemm_wst` = 0 (which also turns the default route off)."""
    import mi355attn
    from mi355attn import functional as F
    out = {}
    with mi355attn.options(gemm_wst=0):
        tags = _tags(lambda: out.__setitem__("y", F.linear16(x16, w16, b, act=act, out16=True, precision=prec)))
    assert not any(WST in t for t in tags), tags
    return out["y"]


def _wst(x16, w16, b, act, prec, **opts):
    import mi355attn
    from mi355attn import functional as F
    out = {}
    with mi355attn.options(**(opts or {"gemm_wst": 4})):
        tags = _tags(lambda: out.__setitem__("y", F.linear16(x16, w16, b, act=act, out16=True, precision=prec)))
    return out["y"], tags


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("N", [1536, 2304, 3072])
@pytest.mark.parametrize("M", MS)
def test_bit_identity_with_the_tile_kernels(M, N, prec):
    from mi355attn import functional as F
    xfull, w16, b = _operands(prec, N)
    x16 = xfull[:M]
    for act in (F.ACT_NONE, F.ACT_GELU):
        for bias in (b, None):
            ref = _tile(x16, w16, bias, act, prec)
            y, tags = _wst(x16, w16, bias, act, prec)
            assert any(WST in t for t in tags), tags
            assert torch.equal(y, ref), (M, N, prec, act, bias is not None)


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("N,act", [(2304, 0), (3072, 1)])
def test_consistency_run_to_run_on_half_the_rows_and_on_strided_rows(N, act, prec):
    import mi355attn
    from mi355attn import functional as F
    M = 32 * 85
    xfull, w16, b = _operands(prec, N)
    x16 = xfull[:M]
    a = F.ACT_GELU if act else F.ACT_NONE
    y, tags = _wst(x16, w16, b, a, prec)
    assert any(WST in t for t in tags), tags
    again, _ = _wst(x16, w16, b, a, prec)
    assert torch.equal(again, y), "run to run"
    half = M // 2 // 32 * 32
    first, tags = _wst(x16[:half], w16, b, a, prec)
    assert any(WST in t for t in tags), tags
    assert torch.equal(first, y[:half]), "a row's bits do not depend on its neighbours"
    wide = torch.zeros(M, K + 64, device="cuda", dtype=x16.dtype)      # the C entry takes the row stride; F.linear16 passes K
    wide[:, :K] = x16
    strided = torch.empty_like(y)
    def run():
        from mi355attn.functional import check, dptr, lib, stream_ptr
        check(lib().mi355_linear16_ws_fwd(dptr(wide), dptr(w16), dptr(b), None, None, dptr(strided), M, N, K, K + 64, N, a, 1, prec, None, 0,
                                          stream_ptr(wide.device)), "mi355_linear16_ws_fwd")
    with mi355attn.options(gemm_wst=4):
        tags = _tags(run)
    assert any(WST in t for t in tags), tags
    assert torch.equal(strided, y), "row stride above K"


FLOOR = 32768                                                          # row floor of the default route (linear16_dispatch)


@pytest.mark.parametrize("M,N,opt", [(32 * 57 + 8, 2304, 4), (32 * 57, 2304 + 128, 4), (FLOOR + 8, 2304, 6), (FLOOR, 2304 + 128, 6)])
def test_refused_shapes_fall_through_to_the_tile_kernels(M, N, opt):
    """M % 32 != 0 or N % 256 != 0: forced (`gemm_wst` = 4) and on the route of every product (`gemm_wst` = 6, at row counts above its floor, where
    the route does reach the kernel's own check) the call lands on a tile kernel."""
    from mi355attn import functional as F
    g = torch.Generator(device="cuda").manual_seed(M + N)
    x16 = F.cast16(torch.randn(M, K, device="cuda", generator=g), 1)
    w16 = F.cast16((torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).contiguous(), 1)
    b = torch.randn(N, device="cuda", generator=g)
    y, tags = _wst(x16, w16, b, F.ACT_NONE, 1, gemm_wst=opt)
    assert tags and not any(WST in t for t in tags), (opt, tags)
    assert torch.equal(y, _tile(x16, w16, b, F.ACT_NONE, 1))


def _default(x16, w16, b, act, prec):
    """The call with no option override at all."""
    import mi355attn
    from mi355attn import functional as F
    assert mi355attn.get_option("gemm_wst") == 5, "the default route is the default"
    out = {}
    tags = _tags(lambda: out.__setitem__("y", F.linear16(x16, w16, b, act=act, out16=True, precision=prec)))
    return out["y"], tags


@pytest.mark.parametrize("prec", [1, 2])
def test_default_route_starts_at_its_row_floor(prec):
    """Default options, fc1 of ViT-Base (N = 3072, GELU): below the floor the product stays on the tile kernels (gemm16_pa where the rows fill its 128-row tiles), at the floor it takes the
    weight-stationary kernel; a product without activation stays on gemm16_w4 at the floor.  The same bits either way."""
    from mi355attn import functional as F
    g = torch.Generator(device="cuda").manual_seed(77 + prec)
    x16 = F.cast16(torch.randn(FLOOR, K, device="cuda", generator=g), prec)
    w16 = F.cast16((torch.randn(3072, K, device="cuda", generator=g) / K ** 0.5).contiguous(), prec)
    b = torch.randn(3072, device="cuda", generator=g)
    below, tags = _default(x16[:FLOOR - 32], w16, b, F.ACT_GELU, prec)  # one row tile short of the floor: some tile kernel
    assert tags and not any(WST in t for t in tags), tags
    _, tags = _default(x16[:FLOOR - 128], w16, b, F.ACT_GELU, prec)      # whole 128-row tiles: the kernel that had fc1 before
    assert any("gemm16_pa_kernel" in t for t in tags) and not any(WST in t for t in tags), tags
    at, tags = _default(x16, w16, b, F.ACT_GELU, prec)
    assert any(WST in t for t in tags), tags
    assert torch.equal(at[:FLOOR - 32], below) and torch.equal(at, _tile(x16, w16, b, F.ACT_GELU, prec))
    _, tags = _default(x16, w16[:2304], b[:2304], F.ACT_NONE, prec)
    assert any("gemm16_w4_kernel" in t for t in tags) and not any(WST in t for t in tags), tags


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("N,act,opts", [(2304, 0, {"gemm_wst": 6}), (3072, 1, None)])
def test_default_route_at_the_model_shape(N, act, opts, prec):
    """M = 50 432 (ViT-Base at 256 images).  fc1 (GELU) takes the weight-stationary kernel with no option set; the qkv product takes it under
    `gemm_wst` = 6 -- by default it stays on gemm16_w4, which tests/test_round5_gpu.py pins for qkv-shaped products of 16 384 and 76 800
    rows (profiles/gemm_wst_pipe.md)."""
    from mi355attn import functional as F
    M = 50432
    g = torch.Generator(device="cuda").manual_seed(N + prec)
    x16 = F.cast16(torch.randn(M, K, device="cuda", generator=g), prec)
    w16 = F.cast16((torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).contiguous(), prec)
    b = torch.randn(N, device="cuda", generator=g)
    a = F.ACT_GELU if act else F.ACT_NONE
    y, tags = _wst(x16, w16, b, a, prec, **opts) if opts else _default(x16, w16, b, a, prec)
    assert any(WST in t for t in tags), tags
    assert torch.equal(y, _tile(x16, w16, b, a, prec))


def test_range_guard_reports_like_the_tile_kernels():
    """One row of inputs at the top of the fp16 range (6e4; 7e4 is not an fp16 number): its products reach several 1e4 .. 1e5, outputs beyond
    65 504 round to inf in fp16 and both kernels raise the range report."""
    import mi355attn
    from mi355attn import functional as F
    M, N = 32 * 57, 2304
    xfull, w16, b = _operands(1, N)
    x16 = xfull[:M].clone()
    x16[32 * 28 + 5] = 6e4                                             # against weights of scale K ** -0.5: the row's outputs are ~ 6e4 N(0, 1)
    x16[32 * 28 + 5, ::2] *= -1
    mi355attn.range_status(wait=True)
    fired = {}
    for name, opts in (("tile", {"gemm_wst": 0}), ("wst", {"gemm_wst": 4})):
        with mi355attn.options(**opts):
            y = F.linear16(x16, w16, b, out16=True, precision=1)
        assert torch.isinf(y[32 * 28 + 5]).any(), "the test's input does not leave the fp16 range"
        try:
            mi355attn.range_status(wait=True)
            fired[name] = False
        except mi355attn.Mi355RangeError:
            fired[name] = True
    assert fired == {"tile": True, "wst": True}, fired
    with mi355attn.options(gemm_wst=4):                                # an ordinary input raises nothing
        F.linear16(xfull[:M], w16, b, out16=True, precision=1)
    mi355attn.range_status(wait=True)
