"""Round-5 GPU tests (VERDICT round 4 "Next round" + the advisor's findings):

  * LayerScale with the published deep-XCiT initialisation (eta = 1e-5): the branch y - x of XCABlock against fp64 (the host no longer folds
    a gamma whose products would land in the fp16 subnormals);
  * the small-output GEMM, the four-token-tile MLP variant, the attention core on seven waves and gemm16_w4.hip, each bit-identical to the
    path it replaces.

The Mixer tests are in tests/test_mixer_gpu.py, the kernel tally, the MFMA yardstick and the bench.py runs in tests/test_bench_gpu.py, the
fused Mixer kernel's range report in tests/test_range_guard_gpu.py.
"""
import pytest
import torch

import oracle as O
from conftest import assert_parity, rel_fro
from kernel_cases import W4_CASES, _drain_range

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("eta", [1e-5, 1e-3, 1.0])
def test_xcablock_small_layerscale_branch_accuracy(eta):
    """with gamma folded into fp16 weights the proj / fc2 branch lost 9e-2 relative accuracy at eta = 1e-5 and
    no test saw it (the branch is 1e-5 of the residual).  The branch y - x is compared with an fp64 evaluation of the reference math."""
    from mi355attn import functional as F
    from mi355attn.modules import XCABlock
    torch.manual_seed(1234)
    m = XCABlock(384, 8, qkv_bias=True, eta=eta).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(4321)
    x = torch.randn(4, 196, 384)
    ref = O.xca_block_forward(x, sd, 8, 14, 14, dtype=torch.float64)
    m = m.cuda()
    with torch.no_grad():
        y = m(x.cuda(), 14, 14).cpu()
    branch, want = (y.double() - x.double()), (ref.double() - x.double())
    # fp32 cancellation noise of y - x: |x| * 2^-24 against a branch of size ~eta
    floor = float(x.abs().max()) * 2.0 ** -23 / max(float(want.abs().mean()), 1e-30)
    err = rel_fro(branch, want)
    assert err <= 2e-3 + 4 * floor, f"eta={eta}: branch error {err:.3e} (cancellation floor {floor:.1e})"
    folded = F.weight16_scaled(m.attn.proj.weight, m.attn.proj.bias, m.gamma1, 1) is not None
    assert folded == (eta >= 0.1), "fold decision"


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("M,N,K,stride", [(256, 1000, 768, 197 * 768), (5, 10, 64, 64), (40, 33, 100, 104), (130, 257, 36, 36), (300, 700, 256, 256)])
def test_small_output_gemm_is_bit_identical_to_the_engine(M, N, K, stride, prec):
    """gemm_small.hip (one-wave 16 x 32 tiles for outputs under an eighth of a round of 128 x 128 tiles: the ViT head, VERDICT round 4
    "What's missing" 6) accumulates a row's K steps in the engine's order: same bits as gemm_kernel with the option off, also through a
    strided X (token 0 of every image in place), a ragged edge in M and N, and a K that is not a multiple of 32."""
    import mi355attn
    from mi355attn import functional as F
    torch.manual_seed(M * 7 + N)
    base = torch.randn(M, stride, device="cuda")
    x = base[:, :K]                                                   # row stride `stride`, consumed in place
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).contiguous()
    b = torch.randn(N, device="cuda")
    outs, tags = {}, {}
    for v in (1, 0):
        with mi355attn.options(gemm_small=v):
            def run():
                outs[v] = (F.linear(x, w, b, precision=prec), F.linear(x, w, None, precision=prec))
            tags[v] = [t for t, *_ in mi355attn.kernel_trace(run)]
    assert all("gemm_small_kernel" in t for t in tags[1]) and len(tags[1]) >= 1, tags[1]
    assert not any("gemm_small_kernel" in t for t in tags[0]), tags[0]
    assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1])
    ref = x.double().cpu() @ w.double().cpu().t() + b.double().cpu()
    assert_parity(outs[1][0].cpu(), ref.float(), 5e-5 if prec == 0 else (1e-3 if prec == 1 else 8e-3), "small GEMM")


def test_vit_head_runs_on_the_small_tile_kernel():
    import mi355attn
    from mi355attn.modules import VisionTransformer
    torch.manual_seed(1)
    m = VisionTransformer(image_size=32, patch_size=16, depths=1, num_heads=4, embedding_dim=256, num_classes=1000).eval().cuda()
    x = torch.randn(64, 3, 32, 32, device="cuda")
    with torch.no_grad():
        tags = [t for t, *_ in mi355attn.kernel_trace(lambda: m(x))]
    assert any("gemm_small_kernel" in t and "N=1000" in t for t in tags), tags


@pytest.mark.parametrize("prec", [1, 2])
def test_fused_mlp_four_tile_variant_is_bit_identical(prec):
    """Option "mlp_tt4" (8 waves x 4 token tiles at 256 registers; VERDICT rounds 2-4: 'the 256-VGPR MLP kernel with four token tiles per
    wave') changes which wave owns which tokens, not the arithmetic: same bits as the 16 x 2 default, with and without the projection in
    front, on a token count that leaves ragged chunks."""
    import mi355attn
    from mi355attn.modules import CSWinBlock
    torch.manual_seed(21)
    m = CSWinBlock(64, 56, 2, split_size=1, qkv_bias=True, precision=prec).eval().cuda()
    x = torch.randn(3, 3136, 64, device="cuda")
    with torch.no_grad():
        with mi355attn.options(mlp_tt4=0):
            y0 = m(x)
        with mi355attn.options(mlp_tt4=1):
            y1 = m(x)
    assert torch.isfinite(y0).all() and torch.equal(y0, y1)


@pytest.mark.parametrize("prec", [1, 2])
def test_attention_core_on_seven_waves_is_bit_identical(prec):
    """Option "attn_nw" = 7: the 13 query tiles of a 197-token head on seven waves (six carry two tiles, one carries one) instead of eight
    (five carry two, three carry one).  A query tile's arithmetic does not depend on the wave that owns it: same bits."""
    import mi355attn
    from mi355attn.modules import Attention
    torch.manual_seed(3)
    m = Attention(768, 12, precision=prec).eval().cuda()
    x = torch.randn(5, 197, 768, device="cuda")
    with torch.no_grad():
        with mi355attn.options(attn_nw=8):
            y8 = m(x)
        with mi355attn.options(attn_nw=7):
            y7 = m(x)
    assert torch.isfinite(y8).all() and torch.equal(y8, y7)


# ---- gemm16_w4.hip: the one-wave-per-SIMD persistent kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("case", W4_CASES)
def test_one_wave_per_simd_gemm_is_bit_identical_to_the_eight_wave_kernel(case, prec):
    """gemm16_w4.hip (round 5; 16-bit outputs): hand-placed MFMA / ds_read / LDS-DMA stream, accumulators in AGPRs, bias through an LDS-DMA
    piece, two-slab pipelined epilogue -- same K order per output as gemm16_p8.hip / gemm16_pa.hip, so the bits must agree (variant 17
    against 15 / 16 / the default dispatch), run to run as well.  fp32 outputs are refused (they belong to gemm16_pa)."""
    import mi355attn
    from mi355attn import functional as F
    M, N, K, gelu, bias = case
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    dt = torch.float16 if prec == 1 else torch.bfloat16
    x16 = torch.randn(M, K, generator=g).to(dev).to(dt)
    w16 = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev).to(dt)
    b = torch.randn(N, generator=g).to(dev) if bias else None
    act = F.ACT_GELU if gelu else F.ACT_NONE
    outs = {}
    for v in (17, 0, 15, 16, 17):
        with mi355attn.options(gemm_variant=v):
            try:
                y = F.linear16(x16, w16, b, act=act, out16=True, precision=prec)
            except mi355attn.Mi355Error:
                assert v in (15, 16), "variant %d refused %r" % (v, case)        # the forced partners may not take every shape
                continue
            torch.cuda.synchronize()
            outs.setdefault(v, []).append(y.clone())
    _drain_range()
    assert len(outs[17]) == 2 and torch.equal(outs[17][0], outs[17][1])
    with mi355attn.options(gemm_variant=17):
        with pytest.raises(mi355attn.Mi355Error):
            F.linear16(x16, w16, b, act=act, out16=False, precision=prec)
    for v, ys in outs.items():
        assert torch.equal(ys[0], outs[17][0]), "variant %d differs from gemm16_w4 on %r" % (v, case)
    ref = x16.float() @ w16.float().t() + (b if b is not None else 0.0)
    if gelu:
        ref = torch.nn.functional.gelu(ref)
    assert rel_fro(outs[17][0].float(), ref) < (3e-3 if prec == 1 else 8e-3)


def test_qkv_shaped_products_take_the_one_wave_per_simd_kernel():
    """Dispatch: 16-bit outputs, whole 256 x 256 tiles, 576 <= K < 1536 -> gemm16_w4 (option "gemm_w4"); the same call with the option off runs
    gemm16_p8; the results agree bit for bit."""
    import mi355attn
    from mi355attn import functional as F
    dev = torch.device("cuda", 0)
    x16 = torch.randn(256 * 300, 768, device=dev).half()
    w16 = (torch.randn(2304, 768, device=dev) / 27.7).half()
    b = torch.randn(2304, device=dev)
    res = {}
    for v in (1, 0):
        with mi355attn.options(gemm_w4=v):
            box = {}
            def run():
                box["y"] = F.linear16(x16, w16, b, out16=True, precision=1)
            tags = [t for t, *_ in mi355attn.kernel_trace(run)]
            torch.cuda.synchronize()
            res[v] = (box["y"].clone(), tags)
    assert any("gemm16_w4_kernel" in t for t in res[1][1]), res[1][1]
    assert any("gemm16_p8_kernel" in t for t in res[0][1]) and not any("gemm16_w4_kernel" in t for t in res[0][1]), res[0][1]
    assert torch.equal(res[0][0], res[1][0])


def test_one_wave_per_simd_gemm_under_graph_capture_and_on_a_side_stream():
    """gemm16_w4 has no inter-workgroup exchange, no workspace and no host-side state per launch: a captured launch replays on changed
    inputs bit for bit like an eager one, and a launch on a non-default stream gives the same bits."""
    import mi355attn
    from mi355attn import functional as F
    M, N, K = 256 * 64, 2304, 768
    torch.manual_seed(5)
    x16 = torch.randn(M, K, device="cuda").half()
    w16 = (torch.randn(N, K, device="cuda") / K ** 0.5).half()
    b = torch.randn(N, device="cuda")
    tags = [t for t, *_ in mi355attn.kernel_trace(lambda: F.linear16(x16, w16, b, out16=True, precision=1))]
    assert any("gemm16_w4_kernel" in t for t in tags), tags                  # 576 tiles >= one round: the dispatch takes the kernel
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            y_cap = F.linear16(x16, w16, b, out16=True, precision=1)
    torch.cuda.current_stream().wait_stream(s)
    for rep in range(3):
        x16.copy_(torch.randn(M, K, device="cuda").half())
        g.replay()
        torch.cuda.synchronize()
        y_ref = F.linear16(x16, w16, b, out16=True, precision=1)
        torch.cuda.synchronize()
        assert torch.equal(y_cap, y_ref), "replay %d" % rep
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y_side = F.linear16(x16, w16, b, out16=True, precision=1)
    side.synchronize()
    assert torch.equal(y_side, y_ref)
    _drain_range()
