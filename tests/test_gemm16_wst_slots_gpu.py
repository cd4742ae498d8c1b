"""gemm16_wst1_kernel with its epilogue as inline-assembly pieces dealt out to the MFMA slots (gemm16_wst.hip, WstPlan) against the tile
kernels (`gemm_wst` = 0), bit for bit.

N = 3072 has twelve 256-column slabs, so a workgroup walks every 21st or 22nd 32-row tile of its slab (256 CUs): M = 32 and 64 leave most
streams empty, 32 * 21 and 32 * 22 give streams of one and of two tiles, 32 * 64 four tiles in the first streams -- the peeled first tile,
the tile loop with and without DMA pieces, the first wrap of the three-tile ring and the drain.  N = 256 is one slab of 256 streams;
M = 32 * 257 gives the first of them two tiles.  The operands are made once per (precision, N) and the tile kernels' result once per case."""
import pytest
import torch

from kernel_cases import _tags

pytestmark = pytest.mark.gpu

K = 768
WST = "gemm16_wst_kernel"
SHAPES = [(3072, 32), (3072, 64), (3072, 32 * 21), (3072, 32 * 22), (3072, 32 * 64), (256, 32 * 257)]
_OPERANDS = {}


def _operands(prec, N):
    from mi355attn import functional as F
    if (prec, N) not in _OPERANDS:
        g = torch.Generator(device="cuda").manual_seed(4000 * prec + N)
        rows = max(m for n, m in SHAPES if n == N)
        x16 = F.cast16(torch.randn(rows, K, device="cuda", generator=g), prec)
        w16 = F.cast16((torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).contiguous(), prec)
        b = torch.randn(N, device="cuda", generator=g)
        _OPERANDS[(prec, N)] = (x16, w16, b)
    return _OPERANDS[(prec, N)]


def _run(x16, w16, b, act, prec, opt):
    import mi355attn
    from mi355attn import functional as F
    out = {}
    with mi355attn.options(gemm_wst=opt):
        tags = _tags(lambda: out.__setitem__("y", F.linear16(x16, w16, b, act=act, out16=True, precision=prec)))
    assert any(WST in t for t in tags) == (opt != 0), (opt, tags)
    return out["y"]


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("N,M", SHAPES)
def test_bit_identity_with_the_tile_kernels(N, M, prec):
    from mi355attn import functional as F
    xfull, w16, b = _operands(prec, N)
    x16 = xfull[:M]
    for act in (F.ACT_NONE, F.ACT_GELU):
        for bias in (b, None):
            assert torch.equal(_run(x16, w16, bias, act, prec, 4), _run(x16, w16, bias, act, prec, 0)), (M, N, prec, act, bias is not None)


@pytest.mark.parametrize("prec", [1, 2])
def test_every_column_gets_its_own_weight_row_and_bias(prec):
    """Weight row n is (n % 7 + 1) at k = n % 768 and zero elsewhere, bias n is n % 61 - 30, x holds integers in [-3, 3]: output (r, n) is
    x[r, n % 768] * (n % 7 + 1) + n % 61 - 30, an integer below 64 that fp16 and bf16 hold exactly.  A column that took another column's
    weight fragment, bias or place in the store shows as a wrong integer in that column, not as noise."""
    from mi355attn import functional as F
    M, N = 32 * 22, 3072
    dt = torch.float16 if prec == 1 else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(9 + prec)
    x = torch.randint(-3, 4, (M, K), device="cuda", generator=g)
    n = torch.arange(N, device="cuda")
    w = torch.zeros(N, K, device="cuda")
    w[n, n % K] = (n % 7 + 1).float()
    b = (n % 61 - 30).float()
    want = (x[:, n % K] * (n % 7 + 1) + (n % 61 - 30)).to(dt)
    y = _run(x.to(dt), w.to(dt), b, F.ACT_NONE, prec, 4)
    wrong = (y != want).any(dim=0).nonzero().flatten().tolist()
    assert not wrong, ("columns with a wrong value", wrong[:16])
    assert torch.equal(y, _run(x.to(dt), w.to(dt), b, F.ACT_NONE, prec, 0))


def test_captured_and_replayed_launch_equals_the_eager_one():
    import mi355attn
    from mi355attn import functional as F
    M, N = 32 * 64, 3072
    xfull, w16, b = _operands(1, N)
    x16 = xfull[:M].clone()
    eager = _run(x16, w16, b, F.ACT_GELU, 1, 4)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with mi355attn.options(gemm_wst=4), torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            y_cap = F.linear16(x16, w16, b, act=F.ACT_GELU, out16=True, precision=1)
    torch.cuda.current_stream().wait_stream(s)
    for rep in range(2):
        y_cap.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y_cap, eager), f"replay {rep}"
