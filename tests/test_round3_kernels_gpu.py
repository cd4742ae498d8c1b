"""Op-level checks of the kernels and fixes added in round 3:

  * two-accumulator persistent GEMM (gemm16_pa.hip, gemm_variant 16): bit identity with the round-1 tile kernel (variant 7) for every
    epilogue it takes, on shapes that exercise one tile per workgroup (serial drain only), several tiles (epilogue pieces riding in the
    next tile's main loop), a partial last round, bias / no bias, residual / none, GELU / none, fp16 and bf16; the fp64 product;
    the default dispatch picks it for fp32 + residual outputs; it refuses what it does not take;
  * persistent GEMM's split last round (gemm16_p8.hip): correct under hipGraph capture + replay with changing inputs (ADVICE round 2:
    a captured launch replays its per-launch tag), and a many-launch stress run with varying inputs against the unsplit result.
"""
import pytest
import torch

from conftest import assert_parity

pytestmark = pytest.mark.gpu


def _ref_linear(x16, w16, b, act, resid):
    y = x16.double() @ w16.double().t()
    if b is not None:
        y = y + b.double()
    if act:
        y = torch.nn.functional.gelu(y)
    if resid is not None:
        y = y + resid.double()
    return y


PA_SHAPES = [  # (M, N, K): M % 128 == 0, N % 256 == 0, K >= 640
    (128, 256, 640),                 # one tile, one workgroup: serial drain only
    (128 * 5, 512, 768),             # 10 tiles on 256 CUs: one tile each
    (128 * 300, 256, 640),           # 300 tiles: one full round + a partial one; tiles_n = 1
    (128 * 394, 768, 768),           # ViT-Base proj: 4.6 rounds
    (128 * 200, 768, 3072),          # long reduction (ViT-Base fc2 geometry)
    (128 * 37, 1024, 1152),
    # round 4, swapped orientation (256 x 128 tiles): M % 256 == 0, N % 128 == 0 but not % 256
    (256, 128, 640),                 # one tile
    (256 * 3, 384, 768),             # 9 tiles, three column tiles per row panel
    (256 * 196, 384, 1536),          # XCiT-S fc2 at B = 256: 588 tiles = 2.3 rounds
    (256 * 70, 640, 1024),           # five column tiles
    # round 4, short reductions (16-bit epilogue packed two / three pieces per barrier interval; fp32 outputs refuse K < 640)
    (128 * 40, 512, 256),            # K = 256: four K-tiles, three pieces per interval
    (128 * 300, 768, 320),           # five K-tiles, two pieces per interval
    (256 * 20, 384, 384),            # swapped orientation + six K-tiles
    (128 * 64, 1024, 512),           # eight K-tiles
]


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


# ---- boundary completion: the ViT attention block as one C call, helper classes on their own -------------------------------------
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


def _bn_randomise(mod):
    with torch.no_grad():
        for c in mod.modules():
            if isinstance(c, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                c.running_mean.normal_(0, 0.3)
                c.running_var.uniform_(0.5, 1.5)
                c.weight.uniform_(0.5, 1.5)
                c.bias.normal_(0, 0.2)


@pytest.mark.parametrize("B,C,H,W,ks", [(2, 64, 32, 32, 7), (3, 20, 9, 13, 3), (1, 7, 5, 6, 5)])
def test_triplet_helper_classes_stand_alone(B, C, H, W, ks):
    """ZPool / BasicConv2d / AttentionGate forwards (triplet_attention.py:19-49) against the same math in torch on the CPU."""
    from mi355attn.modules.axis import AttentionGate, BasicConv2d, ZPool
    torch.manual_seed(7)
    x = torch.randn(B, C, H, W)
    z = ZPool()(x.cuda())
    zr = torch.cat([x.mean(dim=1, keepdim=True), x.max(dim=1, keepdim=True)[0]], dim=1)
    assert_parity(z.cpu(), zr, 1e-6, "ZPool")
    g = AttentionGate(ks).eval()
    _bn_randomise(g)
    c = g.conv
    with torch.no_grad():
        gr = x * torch.sigmoid(torch.relu(c.bn(c.conv(zr))))
        gy = g.cuda()(x.cuda())
    assert_parity(gy.cpu(), gr, 2e-6, "AttentionGate")
    bc = BasicConv2d(C, 12, ks).eval()
    _bn_randomise(bc)
    with torch.no_grad():
        br = torch.relu(bc.bn(bc.conv(x)))
        by = bc.cuda()(x.cuda())
    assert by.shape == br.shape
    assert_parity(by.cpu(), br, 5e-5, "BasicConv2d")


@pytest.mark.parametrize("B,C,H,W", [(2, 64, 32, 32), (3, 32, 9, 14)])
def test_bam_gates_stand_alone(B, C, H, W):
    """ChannelGate / SpatialGate forwards (bam.py:16-61) against the same math in torch on the CPU, and consistency with BAM.forward."""
    from mi355attn.modules.axis import BAM
    torch.manual_seed(9)
    m = BAM(C).eval()
    _bn_randomise(m)
    x = torch.randn(B, C, H, W)
    ch, sp = m.channel_attn, m.spatial_attn
    with torch.no_grad():
        cr = ch.bn(ch.mlp(x.mean(dim=(2, 3)))).view(B, C, 1, 1).expand_as(x)
        sr = sp.bn(sp.conv3(sp.conv2(sp.conv1(x)))).expand_as(x)
        yr = x + x * torch.sigmoid(cr + sr)
        m = m.cuda()
        cy = m.channel_attn(x.cuda())
        sy = m.spatial_attn(x.cuda())
        yy = m(x.cuda())
    assert cy.shape == x.shape and sy.shape == x.shape
    assert_parity(cy.cpu(), cr, 1e-5, "ChannelGate")
    assert_parity(sy.cpu(), sr, 1e-4, "SpatialGate")
    assert_parity(yy.cpu(), yr, 1e-5, "BAM")


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


# ---- fp16 range guard ------------------------------------------------------------------------------------------------------------
def _drain_range():
    import mi355attn
    try:
        mi355attn.range_status(wait=True)
    except mi355attn.Mi355RangeError:
        pass


def test_range_guard_cast16():
    import mi355attn
    from mi355attn import functional as F
    _drain_range()
    x = torch.randn(1000, 64, device="cuda")
    F.cast16(x, 1)
    mi355attn.range_status(wait=True)                               # ordinary data: nothing to report
    x[17, 3] = 7.0e4                                                # finite in fp32, inf in fp16
    y = F.cast16(x, 1)
    assert torch.isinf(y[17, 3])
    with pytest.raises(mi355attn.Mi355RangeError, match="cast16"):
        mi355attn.range_status(wait=True)
    mi355attn.range_status(wait=True)                               # reported once
    x[17, 3] = 65519.0                                              # largest magnitude that still rounds to 65504
    assert float(F.cast16(x, 1)[17, 3]) == 65504.0
    mi355attn.range_status(wait=True)
    x[17, 3] = float("inf")                                         # an inf that was already there is the input's, not the engine's
    x[18, 3] = float("nan")
    F.cast16(x, 1)
    mi355attn.range_status(wait=True)
    x[17, 3] = 7.0e4
    F.cast16(x, 2)                                                  # bf16 has the fp32 range
    mi355attn.range_status(wait=True)
    F.cast16(x, 1)                                                  # the NEXT 16-bit launch refuses to compute on inf
    torch.cuda.synchronize()
    with pytest.raises(mi355attn.Mi355RangeError):
        F.cast16(x, 1)
    _drain_range()


def test_range_guard_layernorm16_and_gemm_epilogues():
    import mi355attn
    from mi355attn import functional as F
    _drain_range()
    torch.manual_seed(0)
    x = torch.randn(300, 768, device="cuda")
    w, b = torch.ones(768, device="cuda"), torch.zeros(768, device="cuda")
    F.layernorm16(x, w, b, precision=1)
    mi355attn.range_status(wait=True)
    F.layernorm16(x, w * 5.0e4, b, precision=1)                     # LayerNorm gain x 50000: |normalised| up to ~4 -> 2e5
    with pytest.raises(mi355attn.Mi355RangeError, match="layernorm16"):
        mi355attn.range_status(wait=True)
    # 16-bit-output GEMM epilogues: every kernel of the dispatch (tile kernel 7, persistent 15, two-accumulator 16, short-K weight-stationary)
    for (M, N, K, variant) in ((512, 256, 768, 7), (50432, 512, 768, 15), (128 * 300, 256, 768, 16), (4096, 256, 64, 0)):
        x16 = (torch.randn(M, K, device="cuda") * 40).half()
        w16 = (torch.randn(N, K, device="cuda") * 0.5).half()
        with mi355attn.options(gemm_variant=variant):
            y32 = F.linear16(x16, w16, out16=False, precision=1)    # fp32 output: nothing to saturate
            mi355attn.range_status(wait=True)
            assert float(y32.abs().max()) < 65000                   # ... and this scale stays inside fp16 anyway
            F.linear16(x16, w16, out16=True, precision=1)
            mi355attn.range_status(wait=True)
            y16 = F.linear16(x16 * 200, w16, out16=True, precision=1)       # sums ~ 40 * 200 * 0.5 * sqrt(K) >> 65504
            torch.cuda.synchronize()
            assert torch.isinf(y16).any()
            with pytest.raises(mi355attn.Mi355RangeError, match="GEMM"):
                mi355attn.range_status(wait=True)
            F.linear16((x16 * 200).to(torch.bfloat16), w16.to(torch.bfloat16), out16=True, precision=2)    # bf16: no guard needed
            mi355attn.range_status(wait=True)
    _drain_range()


@pytest.mark.parametrize("scale", [1.0e4, 1.0e5])
def test_guarded_forward_reruns_in_strict_mode(scale):
    """Activations of 1e4-1e5: the fp32 reference is finite; the engine must be finite and within tolerance, or must
    report -- guarded_forward then re-runs the module in strict mode, whose result sits on the reference at the strict tolerance.
    Module: ViT's Mlp (fc1 -> GELU -> fc2 -> GELU, ViT.py:58-65), a well-conditioned map at any input scale (softmax attention on raw
    1e4-scaled tokens is not: its logits reach 1e8 and the fp32 reference itself is one rounding away from another arg-max), and the
    pre-LN encoder block, whose LayerNorm removes the scale before any fp16 operand is formed."""
    import warnings
    import mi355attn
    import oracle as O
    from mi355attn.modules import TransformerEncoder
    from mi355attn.modules.vit import Mlp
    _drain_range()
    torch.manual_seed(1234)
    m = Mlp(768, 3072).eval()
    with torch.no_grad():
        for lin in (m.fc1, m.fc2):
            torch.nn.init.trunc_normal_(lin.weight, std=.02)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(4321)
    x = torch.randn(2, 197, 768) * scale
    ref = O.vit_mlp_forward(x, sd)
    assert torch.isfinite(ref).all()
    m = m.cuda()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            y = mi355attn.guarded_forward(m, x.cuda())
    assert torch.isfinite(y).all()
    reran = any("strict mode" in str(w.message) for w in rec)
    assert_parity(y.cpu(), ref, 5e-5 if reran else 1e-3, f"Mlp at scale {scale:g} ({'strict re-run' if reran else 'fp16'})")
    if scale >= 1.0e5:
        assert reran, "activations of 1e5 cannot be represented in fp16: the guard must have fired"
    # the pre-LN block at the same scale: no fp16 tensor ever sees the raw activations
    torch.manual_seed(1234)
    blk = TransformerEncoder(768, 12).eval()
    sdb = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    refb = O.vit_encoder_forward(x, sdb, 12)
    with torch.no_grad():
        yb = blk.cuda()(x.cuda())
    mi355attn.range_status(wait=True)
    assert_parity(yb.cpu(), refb, 1e-3, f"TransformerEncoder at scale {scale:g}")
    _drain_range()


def test_massive_activation_channel_and_large_layernorm_gain():
    """One 3e4 'massive activation' channel in the residual stream and a LayerNorm gain x 50: finite and
    within 1e-3 of the fp32 oracle, or reported and re-run."""
    import warnings
    import mi355attn
    import oracle as O
    from mi355attn.modules import TransformerEncoder
    _drain_range()
    torch.manual_seed(1234)
    blk = TransformerEncoder(768, 12).eval()
    with torch.no_grad():
        blk.layernorm1.weight.mul_(50.0)
        blk.layernorm2.weight.mul_(50.0)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    torch.manual_seed(4321)
    x = torch.randn(2, 197, 768)
    x[:, :, 7] = 3.0e4 + 10 * torch.randn(2, 197)
    ref = O.vit_encoder_forward(x, sd, 12)
    assert torch.isfinite(ref).all()
    blk = blk.cuda()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            y = mi355attn.guarded_forward(blk, x.cuda())
    assert torch.isfinite(y).all()
    reran = any("strict mode" in str(w.message) for w in rec)
    assert_parity(y.cpu(), ref, 1e-3, "massive activation block (%s)" % ("strict re-run" if reran else "fp16"))
    _drain_range()


def test_non_default_init_weights_vit_and_cswin():
    """Parity with every parameter moved away from its default initialisation (the f2 cases already do this; here the MFMA rows).
    The step is sized like a trained checkpoint -- weights at about twice their initial spread, biases and LayerNorm affine parts
    non-trivial -- not the 0.3-sigma jolt of cases.perturb_all: at that size the attention logits reach a spread of ~70 and softmax
    amplifies ANY 16-bit operand rounding to several 1e-3 (measured 3.9e-3), which says nothing about the kernels."""
    import oracle as O
    from mi355attn.modules import CSWinBlock, TransformerEncoder

    def perturb_all(module, step=0.03):
        g = torch.Generator().manual_seed(778)
        with torch.no_grad():
            for p in module.parameters():
                p.add_(step * torch.randn(p.shape, generator=g))

    torch.manual_seed(1234)
    enc = TransformerEncoder(768, 12, qkv_bias=True).eval()
    perturb_all(enc)
    enc.eval()
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    torch.manual_seed(4321)
    x = torch.randn(3, 197, 768)
    ref = O.vit_encoder_forward(x, sd, 12)
    with torch.no_grad():
        y = enc.cuda()(x.cuda())
    assert_parity(y.cpu(), ref, 1e-3, "perturbed TransformerEncoder")
    for args, kw, shp, o in (((64, 56, 2), dict(split_size=1, qkv_bias=True), (3136, 64), (56, 2, 1)),
                             ((256, 14, 8), dict(split_size=7, qkv_bias=True), (196, 256), (14, 8, 7))):
        torch.manual_seed(1234)
        m = CSWinBlock(*args, **kw).eval()
        perturb_all(m)
        m.eval()
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        torch.manual_seed(4321)
        x = torch.randn(2, *shp)
        ref = O.cswin_block_forward(x, sd, *o)
        with torch.no_grad():
            y = m.cuda()(x.cuda())
        assert_parity(y.cpu(), ref, 1e-3, f"perturbed CSWinBlock{args}")


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
