"""Op-level checks of the kernels and fixes added in round 3:

  * two-accumulator persistent GEMM (gemm16_pa.hip, gemm_variant 16): bit identity with the round-1 tile kernel (variant 7) for every
    epilogue it takes, on shapes that exercise one tile per workgroup (serial drain only), several tiles (epilogue pieces riding in the
    next tile's main loop), a partial last round, bias / no bias, residual / none, GELU / none, fp16 and bf16; the fp64 product;
    the default dispatch picks it for fp32 + residual outputs; it refuses what it does not take;
  * persistent GEMM's split last round (gemm16_p8.hip): correct under hipGraph capture + replay with changing inputs (ADVICE round 2:
    a captured launch replays its per-launch tag), and a many-launch stress run with varying inputs against the unsplit result;
  * mi355_mhsa_fwd (the ViT attention block as one C call) against the composition it replaces and the oracle; bad arguments;
  * PositionalEncodingFourier.forward as a (B, dim, H, W) map; dropout rates do not change an eval forward;
  * the ReLU epilogue of the fp32 engine;
  * LayerNorm fused into the LPI stencil kernel is bit-identical to layernorm -> lpi;
  * the one-kernel DoubleAttention path (double_attn_small.hip) in both operand types.
"""
import pytest
import torch

from conftest import assert_parity
from kernel_cases import PA_SHAPES, _bn_randomise, _ref_linear

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prec,dt", [(1, torch.float16), (2, torch.bfloat16)])
@pytest.mark.parametrize("M,N,K", PA_SHAPES)
def test_two_accumulator_gemm_bit_identical_to_tile_kernel(M, N, K, prec, dt):
    import mi355attn
    from mi355attn import functional as F
    torch.manual_seed(M + N + K)
    x16 = torch.randn(M, K, device="cuda").to(dt)
    w16 = (torch.randn(N, K, device="cuda") / K ** 0.5).to(dt)
    b = torch.randn(N, device="cuda")
    resid = torch.randn(M, N, device="cuda")
    combos = [dict(bias=b, out16=True), dict(bias=b, act=F.ACT_GELU, out16=True), dict(bias=None, out16=True),
              dict(bias=b, resid=resid), dict(bias=b, resid=resid, act=F.ACT_GELU), dict(bias=None, resid=resid), dict(bias=b), dict(bias=None)]
    if K < 640:
        combos = [kw for kw in combos if kw.get("out16")]     # the fp32 epilogue needs ten K-tiles of the next tile's main loop
    for kw in combos:
        with mi355attn.options(gemm_variant=7):
            y7 = F.linear16(x16, w16, precision=prec, **kw)
        with mi355attn.options(gemm_variant=16):
            y16 = F.linear16(x16, w16, precision=prec, **kw)
            y16b = F.linear16(x16, w16, precision=prec, **kw)
        assert torch.equal(y16, y16b), f"run-to-run difference with {sorted(kw)}"
        assert torch.equal(y7, y16), f"two-accumulator kernel differs from variant 7 with {sorted(kw)}"
    if M * N <= 3_000_000 and K >= 640:
        ref = _ref_linear(x16.cpu(), w16.cpu(), b.cpu(), True, resid.cpu())
        with mi355attn.options(gemm_variant=16):
            assert_parity(F.linear16(x16, w16, b, act=F.ACT_GELU, resid=resid, precision=prec).cpu(), ref.float(), 2e-5, "fp64 product")


def test_two_accumulator_gemm_is_the_default_for_fp32_residual_outputs_and_batch_independent():
    """Default dispatch at the ViT-Base proj / fc2 shapes: same bits as the forced variant 16 (i.e. that kernel ran), and a row's bits
    do not depend on the batch it sits in (no split-K anywhere on this path)."""
    import mi355attn
    from mi355attn import functional as F
    torch.manual_seed(3)
    for N, K in ((768, 768), (768, 3072)):
        M = 256 * 197
        x16 = torch.randn(M, K, device="cuda").half()
        w16 = (torch.randn(N, K, device="cuda") / K ** 0.5).half()
        b = torch.randn(N, device="cuda")
        resid = torch.randn(M, N, device="cuda")
        y0 = F.linear16(x16, w16, b, resid=resid, precision=1)
        with mi355attn.options(gemm_variant=16):
            y16 = F.linear16(x16, w16, b, resid=resid, precision=1)
        assert torch.equal(y0, y16)
        Ms = 128 * 197                                        # half the batch: different tile -> workgroup assignment
        ys = F.linear16(x16[:Ms].contiguous(), w16, b, resid=resid[:Ms].contiguous(), precision=1)
        assert torch.equal(ys, y0[:Ms]), "rows depend on the batch they are computed in"


def test_two_accumulator_gemm_refuses_what_it_does_not_take():
    import mi355attn
    from mi355attn import functional as F
    x16 = torch.randn(130, 768, device="cuda").half()          # M % 128 != 0
    w16 = torch.randn(256, 768, device="cuda").half()
    with mi355attn.options(gemm_variant=16):
        with pytest.raises(RuntimeError, match="two-accumulator"):
            F.linear16(x16, w16, precision=1)
        with pytest.raises(RuntimeError, match="two-accumulator"):      # K too short for the nine epilogue K-tiles
            F.linear16(torch.randn(128, 512, device="cuda").half(), torch.randn(256, 512, device="cuda").half(), precision=1)
    y = F.linear16(x16, w16, precision=1)                      # default dispatch falls through to the other kernels
    assert_parity(y.cpu(), (x16.double() @ w16.double().t()).float().cpu(), 2e-5, "fallback")


def test_split_k_gemm_under_graph_capture_and_replay():
    """A captured launch replays with the same kernel arguments.  The split last round keys its flags on a per-launch tag, so the
    launcher must not split under capture: replay twice with CHANGED inputs and compare with eager results."""
    import mi355attn
    from mi355attn import functional as F
    M, N, K = 50432, 768, 3072
    torch.manual_seed(11)
    x16 = torch.randn(M, K, device="cuda").half()
    w16 = (torch.randn(N, K, device="cuda") / K ** 0.5).half()
    b = torch.randn(N, device="cuda")
    resid = torch.randn(M, N, device="cuda")
    with mi355attn.options(gemm_pa=0, gemm_splitk=1):          # the persistent 256 x 256 kernel with its split last round is the default then
        y_eager = F.linear16(x16, w16, b, resid=resid, precision=1)          # also warms the workspace cache outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                y_cap = F.linear16(x16, w16, b, resid=resid, precision=1)
        torch.cuda.current_stream().wait_stream(s)
        for rep in range(3):
            x16.copy_(torch.randn(M, K, device="cuda").half())
            resid.copy_(torch.randn(M, N, device="cuda"))
            g.replay()
            torch.cuda.synchronize()
            with mi355attn.options(gemm_splitk=0):
                y_ref = F.linear16(x16, w16, b, resid=resid, precision=1)
            assert_parity(y_cap.cpu(), y_ref.cpu(), 2e-6, f"replay {rep}")
        # eager launches after the replays still work (the workspace history was not corrupted by the capture)
        y2 = F.linear16(x16, w16, b, resid=resid, precision=1)
        with mi355attn.options(gemm_splitk=0):
            y3 = F.linear16(x16, w16, b, resid=resid, precision=1)
        assert_parity(y2.cpu(), y3.cpu(), 2e-6, "eager after replay")
        assert mi355attn.lib().mi355_sync_status() == 0
    del y_eager


def test_split_k_gemm_stress_varying_inputs():
    """Forty back-to-back split launches on fresh inputs (the flag area is never zeroed: only the per-launch tag separates them), each
    compared with the unsplit kernel; every element, not a sample."""
    import mi355attn
    from mi355attn import functional as F
    M, N, K = 50432, 768, 3072
    torch.manual_seed(5)
    w16 = (torch.randn(N, K, device="cuda") / K ** 0.5).half()
    b = torch.randn(N, device="cuda")
    with mi355attn.options(gemm_pa=0):
        worst = 0.0
        for it in range(40):
            x16 = torch.randn(M, K, device="cuda").half() * (1.0 + 0.1 * it)
            with mi355attn.options(gemm_splitk=1):
                ys = F.linear16(x16, w16, b, precision=1)
            with mi355attn.options(gemm_splitk=0):
                yu = F.linear16(x16, w16, b, precision=1)
            d = float((ys - yu).abs().max() / yu.abs().max())
            worst = max(worst, d)
            assert d < 2e-6, f"launch {it}: split result off by {d:.3e} (stale or half-written partial slab?)"
        assert mi355attn.lib().mi355_sync_status() == 0


# ---- boundary completion: the ViT attention block as one C call -------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C,heads,x16", [(3, 197, 768, 12, True), (2, 197, 768, 12, False), (2, 50, 768, 4, True), (1, 300, 384, 6, False),
                                             (2, 64, 128, 4, True)])
def test_mhsa_block_entry_matches_composition_and_oracle(B, N, C, heads, x16):
    """mi355_mhsa_fwd (one C call) against the three-call composition it replaces (bit-identical: the same kernels) and against the
    oracle's ViT Attention forward (1e-3)."""
    import oracle as O
    from mi355attn import functional as F
    from mi355attn.modules import Attention
    torch.manual_seed(1234)
    m = Attention(C, heads, qkv_bias=True).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(4321)
    x = torch.randn(B, N, C)
    resid = torch.randn(B, N, C)
    ref = O.vit_attention_forward(x, sd, heads) + resid
    m = m.cuda()
    xd, rd = x.cuda(), resid.cuda()
    p = F._prec(None)
    xin = F.cast16(xd, p) if x16 else xd
    with torch.no_grad():
        y = m(xin, resid=rd)
        y2 = m(xin, resid=rd)
        x16t = xin if x16 else F.cast16(xd, p)
        qkv16 = F.linear16(x16t, F.weight16(m.qkv.weight, p), m.qkv.bias, out16=True, precision=p)
        ctx16 = m._core(qkv16, True)
        yc = F.linear16(ctx16, F.weight16(m.proj.weight, p), m.proj.bias, resid=rd, precision=p)
    assert torch.equal(y, y2)
    assert torch.equal(y, yc), "block entry differs from the composition of its own kernels"
    assert_parity(y.cpu(), ref, 1e-3, "mhsa block vs oracle")


def test_mhsa_block_entry_rejects_bad_arguments():
    from mi355attn import functional as F
    x = torch.randn(2, 10, 96, device="cuda")                   # C % 64 != 0
    w = torch.randn(288, 96, device="cuda").half()
    wp = torch.randn(96, 96, device="cuda").half()
    with pytest.raises(RuntimeError, match="mi355_mhsa_fwd"):
        F.mhsa16(x, w, None, wp, None, 3, 0.1, precision=1)


def test_fourier_position_encoding_forward():
    """PositionalEncodingFourier.forward(B, H, W) (xcit.py:56-77) as a (B, dim, H, W) map against torch's conv on the engine's own
    feature table (the table itself is pinned against the reference in tests/test_helper_modules.py)."""
    from mi355attn.modules.xcit import PositionalEncodingFourier
    torch.manual_seed(3)
    m = PositionalEncodingFourier(hidden_dim=32, dim=96).eval()
    B, H, W = 3, 14, 9
    feat = m.features(H, W)
    with torch.no_grad():
        ref = m.token_projection(feat.reshape(1, H, W, 64).permute(0, 3, 1, 2)).expand(B, -1, -1, -1)
        y = m.cuda()(B, H, W)
    assert tuple(y.shape) == (B, 96, H, W)
    assert_parity(y.cpu(), ref, 5e-5, "PositionalEncodingFourier.forward")


def test_dropout_rates_do_not_change_an_eval_forward():
    from mi355attn.modules import mhsa
    torch.manual_seed(5)
    a = mhsa.Attention(64, num_heads=2, qkv_bias=True).eval().cuda()
    b = mhsa.Attention(64, num_heads=2, qkv_bias=True, attn_drop=0.3, proj_drop=0.1).eval().cuda()
    b.load_state_dict(a.state_dict())
    x = torch.randn(2, 50, 64, device="cuda")
    with torch.no_grad():
        assert torch.equal(a(x), b(x))
    b.train()
    with pytest.raises(RuntimeError, match="eval"):
        b(x)


def test_relu_epilogue_of_the_fp32_engine():
    from mi355attn import functional as F
    torch.manual_seed(2)
    x = torch.randn(300, 132, device="cuda")
    w = torch.randn(72, 132, device="cuda") / 11
    b = torch.randn(72, device="cuda")
    y = F.linear(x, w, b, act=F.ACT_RELU, precision=F.PREC_STRICT)
    ref = torch.relu(x.double().cpu() @ w.double().cpu().t() + b.double().cpu())
    assert_parity(y.cpu(), ref.float(), 5e-5, "linear + relu")
    xn = x.clone()
    xn[3, 5] = float("nan")
    yn = F.linear(xn, w, b, act=F.ACT_RELU, precision=F.PREC_STRICT)
    assert torch.isnan(yn[3]).all() and not torch.isnan(yn[4]).any(), "relu must keep a NaN like torch.relu"


@pytest.mark.parametrize("B,H,W,C", [(2, 14, 14, 384), (1, 7, 7, 40), (3, 4, 9, 100), (2, 16, 16, 128), (1, 1, 1, 32), (2, 5, 3, 30)])
def test_ln_lpi_fused_is_bit_identical_to_layernorm_then_lpi(B, H, W, C):
    """mi355_ln_lpi_fwd (row statistics + normalisation on the way into the stencil kernel) against mi355_layernorm_fwd followed by
    mi355_lpi_fwd: the same expression per element, so the same bits; and against the oracle."""
    import oracle as O
    from mi355attn import functional as F
    from mi355attn.modules import LPI
    torch.manual_seed(C + H)
    m = LPI(C).eval()
    _bn_randomise(m)
    ln = torch.nn.LayerNorm(C)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.normal_(0, 0.2)
    x = torch.randn(B, H * W, C) * 2 + 0.5
    gamma = torch.rand(C) + 0.5
    m, ln = m.cuda(), ln.cuda()
    xd, gd = x.cuda(), gamma.cuda()
    with torch.no_grad():
        fused = m(xd, H, W, gamma=gd, resid=xd, ln=ln)
        unfused = m(F.layernorm(xd, ln.weight, ln.bias, ln.eps), H, W, gamma=gd, resid=xd)
        fused2 = m(xd, H, W, gamma=gd, resid=xd, ln=ln)
    assert torch.equal(fused, fused2)
    assert torch.equal(fused, unfused), "fused LayerNorm differs from layernorm -> lpi"
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    u = torch.nn.functional.layer_norm(x, (C,), ln.weight.cpu(), ln.bias.cpu(), ln.eps)
    ref = x + gamma * O.lpi_forward(u, sd, H, W)
    assert_parity(fused.cpu(), ref, 2e-5, "ln + lpi vs oracle")


@pytest.mark.parametrize("prec,tol", [(1, 1e-3), (2, 8e-3)])
def test_double_attention_one_kernel_path_properties(prec, tol):
    """double_attn_small.hip (c_m = c_n = 32, C = 64, H*W <= 1024): parity at the README shape in both operand types, run-to-run bit
    identity, and batch independence (an image is one workgroup: its bits cannot depend on its neighbours)."""
    import oracle as O
    from mi355attn.modules import DoubleAttention
    torch.manual_seed(1234)
    m = DoubleAttention(64, 32, 32, precision=prec).eval()
    sd = m.state_dict()
    torch.manual_seed(4321)
    x = torch.randn(6, 64, 32, 32)
    ref = O.double_attention_forward(x, sd["convA.weight"], sd["convA.bias"], sd["convB.weight"], sd["convB.bias"],
                                     sd["convV.weight"], sd["convV.bias"], sd["proj.weight"], sd["proj.bias"], torch.float64)
    m = m.cuda()
    with torch.no_grad():
        y = m(x.cuda())
        y2 = m(x.cuda())
        y1 = m(x[3:4].cuda())
    assert torch.equal(y, y2)
    assert torch.equal(y[3:4], y1), "an image's result depends on the batch around it"
    assert_parity(y.cpu(), ref.float(), tol, f"DoubleAttention(64,32,32) p{prec}")
