"""The fp16 range contract: a finite fp32 value that becomes an fp16 inf is reported, never silently computed on.

  * the range word: cast16, layernorm16 and the 16-bit epilogue of every GEMM kernel of the dispatch report a saturating value (once),
    an inf / NaN that was already in the input is the input's own, bf16 needs no guard, a saturation next to an input inf is still seen;
  * the fused block kernels (mixer_fused.hip, mlp_fused.hip, mlp_wide.hip, cswin_fused.hip) report a saturating 16-bit intermediate;
  * guarded_forward re-runs a module in strict mode after a report or a non-finite output for a finite input, sub-modules built with
    an explicit 16-bit precision included, and restores the precisions;
  * option "range_fallback" = 1 (the default): `module(x)` of a drop-in whose fp16 operands saturate returns the strict-mode result
    with one warning, like the fp32 reference, without caller edits; mi355_range_wait synchronises on one event behind the last fp16
    producer; "range_fallback" = 0 keeps the report-on-the-next-call contract (Mi355RangeError);
  * activations of 1e4-1e5, a massive-activation channel, a large LayerNorm gain and weights away from their initialisation stay
    within tolerance of the fp32 oracle, or are reported and re-run.

tests/test_range_sweep_gpu.py sweeps the same contract over every drop-in module.
"""
import warnings

import pytest
import torch

import oracle as O
from conftest import assert_parity
from kernel_cases import _drain_range, _sd, _seeded, _tags

pytestmark = pytest.mark.gpu


# ---- the range word -----------------------------------------------------------------------------------------------------------------
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


def test_range_guard_sees_a_saturation_next_to_an_input_inf():
    """rg_absmax skips a group of four that holds an inf (the input's own, not reported) instead of poisoning the lane's running maximum:
    a later finite value >= 65520 in the same lane is still reported."""
    import mi355attn
    from mi355attn import functional as F
    try:
        mi355attn.range_status(wait=True)
    except mi355attn.Mi355RangeError:
        pass
    x = torch.zeros(1 << 16, device="cuda")
    x[0] = float("inf")                                        # the first group of four of lane 0 ...
    F.cast16(x, 1)
    mi355attn.range_status(wait=True)                          # ... is the input's own inf: no report
    n = x.numel()
    x[n - 4096:] = 7.0e4                                       # finite values that saturate, later in the same grid-stride walks
    F.cast16(x, 1)
    with pytest.raises(mi355attn.Mi355RangeError):
        mi355attn.range_status(wait=True)


def test_fused_mixer_kernel_reports_a_saturating_intermediate():
    """LN(x) * w + b above 65504 inside mixer_token_kernel must raise Mi355RangeError at the next check."""
    import mi355attn
    from mi355attn.modules import MixerLayer
    _drain_range()
    torch.manual_seed(5)
    m = MixerLayer(256, 196, precision=1).eval().cuda()
    x = torch.randn(2, 196, 256, device="cuda")
    from conftest import no_range_fallback
    with torch.no_grad(), no_range_fallback():                     # the reporting contract itself (round 6: module(x) would absorb the report)
        tags = [t for t, *_ in mi355attn.kernel_trace(lambda: m(x))]
        assert any("mixer_token_kernel" in t for t in tags), tags
        mi355attn.range_status(wait=True)                          # ordinary data: nothing to report
        m.norm1.weight.mul_(1.0e5)                                  # LN output ~1e5: finite in fp32, inf in fp16
        raised = False
        try:
            m(x)                                                   # a later 16-bit launch of the same forward may already see the report
        except mi355attn.Mi355RangeError:
            raised = True
    if not raised:
        with pytest.raises(mi355attn.Mi355RangeError, match="fused block kernel"):
            mi355attn.range_status(wait=True)
    _drain_range()
    m2 = MixerLayer(256, 196, precision=2).eval().cuda()           # bf16 operands have the fp32 range: nothing to report
    m2.load_state_dict(m.state_dict())
    with torch.no_grad():
        m2(x)
    mi355attn.range_status(wait=True)


def test_wide_fused_mlp_reports_a_saturating_hidden_activation():
    """fc1 scaled so that gelu(H) passes 65504: the static proof fails on the host, the kernel tracks and reports (code 4), and module(x)
    of a CSWin stage-3 block falls back to strict mode like the reference (cswin.py:194-196 computes in fp32)."""
    import warnings
    import oracle as O
    import mi355attn
    from mi355attn.modules import CSWinBlock
    torch.manual_seed(1234)
    m = CSWinBlock(256, 14, 8, split_size=7, qkv_bias=True).eval()
    with torch.no_grad():
        m.mlp.fc1.weight.mul_(1e5)
        m.mlp.fc2.weight.mul_(1e-4)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(4321)
    x = torch.randn(4, 196, 256)
    ref = O.cswin_block_forward(x, sd, 14, 8, 7)
    md = m.cuda()
    mi355attn.range_status(wait=True)
    with mi355attn.options(mlp_wide=1), warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            tags = _tags(lambda: md(x.cuda()))
            y = md(x.cuda())
        torch.cuda.synchronize()
    assert any("mlp_wide_kernel" in t for t in tags), tags
    assert len([i for i in w if "strict mode" in str(i.message)]) == 2, [str(i.message) for i in w]      # two forwards, each falls back
    assert_parity(y.cpu(), ref, 2e-4, "CSWin s3 with a saturating hidden activation [strict re-run]")


# ---- guarded_forward ----------------------------------------------------------------------------------------------------------------
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


def test_guarded_forward_catches_a_saturated_fused_intermediate():
    """CSWinBlock stage 1 runs LayerNorm + fc1 + GELU + fc2 in ONE kernel whose 16-bit hidden activations never leave the registers
    (no range word to report into).  With fc1 scaled so that the hidden units pass 65504 the block's output is inf / NaN for a finite
    input: guarded_forward must re-run in strict mode -- including the sub-modules built with an explicit precision=1."""
    import mi355attn
    from mi355attn.modules import CSWinBlock
    torch.manual_seed(1234)
    blk = CSWinBlock(64, 56, 2, split_size=1, qkv_bias=True, precision=1).eval()
    with torch.no_grad():
        blk.mlp.fc1.weight.mul_(3.0e4)                         # hidden pre-activations ~ 3e4 * O(1): beyond the fp16 range
        blk.mlp.fc2.weight.mul_(1.0e-4)                        # keeps the fp32 reference finite and moderate
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    torch.manual_seed(4321)
    x = torch.randn(2, 3136, 64)
    ref = O.cswin_block_forward(x, sd, 56, 2, 1)
    assert torch.isfinite(ref).all()
    blk = blk.cuda()
    from conftest import no_range_fallback
    with torch.no_grad(), no_range_fallback():                 # the raw fp16 result (round 6: module(x) itself would fall back to strict)
        y_fast = blk(x.cuda())
    torch.cuda.synchronize()
    try:
        mi355attn.range_status(wait=True)
    except mi355attn.Mi355RangeError:
        pass
    assert not torch.isfinite(y_fast).all(), "the construction no longer saturates the fused kernel: strengthen it"
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad(), no_range_fallback():             # guarded_forward is the explicit form of the fallback: tested on its own
            y = mi355attn.guarded_forward(blk, x.cuda())
    assert any("strict mode" in str(w.message) for w in rec)
    assert torch.isfinite(y).all()
    assert_parity(y.cpu(), ref, 2e-4, "CSWinBlock s1 after the strict re-run")
    assert blk.precision == 1 and blk.mlp.precision == 1, "explicit precisions must be restored after the re-run"


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


# ---- range fallback -----------------------------------------------------------------------------------------------------------------
def _cases():
    from mi355attn.modules import Attention, CSWinBlock, TransformerEncoder

    def attn():                      # stand-alone Attention: the fp32 input itself is cast to fp16 (mi355_cast16_fwd reports, code 1)
        m = _seeded(lambda: Attention(768, 12))
        return m, (4, 197, 768), 1e5, lambda x, sd: O.vit_attention_forward(x, sd, 12), ()

    def enc_input():                 # x * 1e3 through a pre-LN block: LayerNorm absorbs the scale, nothing saturates, no warning
        m = _seeded(lambda: TransformerEncoder(768, 12))
        return m, (4, 197, 768), 1e3, lambda x, sd: O.vit_encoder_forward(x, sd, 12), ()

    def enc_weights():               # fc1 weights x 1e5: the 16-bit hidden activation saturates in the GEMM epilogue (code 3)
        m = _seeded(lambda: TransformerEncoder(768, 12))
        with torch.no_grad():
            m.mlp.fc1.weight.mul_(1e5)
        return m, (4, 197, 768), 1.0, lambda x, sd: O.vit_encoder_forward(x, sd, 12), ()

    def cswin_mlp():                 # CSWin stage 1: gelu(H) inside the fused proj + MLP kernel (code 4, round 6)
        m = _seeded(lambda: CSWinBlock(64, 56, 2, split_size=1, qkv_bias=True))
        with torch.no_grad():
            m.mlp.fc1.weight.mul_(1e5)
        return m, (2, 3136, 64), 1.0, lambda x, sd: O.cswin_block_forward(x, sd, 56, 2, 1), ()

    def cswin_v():                   # CSWin stage 1: the v third of the qkv projection x 1e5 -> v / ctx inside the stripe kernel (code 4)
        m = _seeded(lambda: CSWinBlock(64, 56, 2, split_size=1, qkv_bias=True))
        with torch.no_grad():
            m.qkv.weight[128:].mul_(1e5)
        return m, (2, 3136, 64), 1.0, lambda x, sd: O.cswin_block_forward(x, sd, 56, 2, 1), ()

    def cswin_input():               # x * 1e3 into the LN-fronted block: no saturation, fast result inside 1e-3
        m = _seeded(lambda: CSWinBlock(64, 56, 2, split_size=1, qkv_bias=True))
        return m, (2, 3136, 64), 1e3, lambda x, sd: O.cswin_block_forward(x, sd, 56, 2, 1), ()

    return {"attn_x1e5": (attn, True), "encoder_x1e3": (enc_input, False), "encoder_fc1_1e5": (enc_weights, True),
            "cswin_s1_fc1_1e5": (cswin_mlp, True), "cswin_s1_v_1e5": (cswin_v, True), "cswin_s1_x1e3": (cswin_input, False)}


def _oracle_has(name):
    return hasattr(O, name)


@pytest.mark.parametrize("case", ["attn_x1e5", "encoder_x1e3", "encoder_fc1_1e5", "cswin_s1_fc1_1e5", "cswin_s1_v_1e5", "cswin_s1_x1e3"])
def test_module_call_falls_back_to_strict_like_the_reference(case):
    """ViT.py:79-89,116-119 / cswin.py:176-197 return finite numbers at any scale.  Zero-edit drop-in, default options."""
    import mi355attn
    build, fires = _cases()[case]
    if case.startswith("encoder") and not _oracle_has("vit_encoder_forward"):
        pytest.skip("oracle has no encoder restatement")
    m, shape, xscale, ref_fn, fwd_args = build()
    sd = _sd(m)
    torch.manual_seed(4321)
    x = torch.randn(*shape) * xscale
    ref = ref_fn(x, sd)
    assert torch.isfinite(ref).all()
    md, xd = m.cuda(), x.cuda()
    assert mi355attn.get_option("range_fallback") == 1, "the default"
    mi355attn.range_status(wait=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            y = md(xd, *fwd_args)
        torch.cuda.synchronize()
    hits = [i for i in w if "re-running this forward in strict mode" in str(i.message)]
    if fires:
        assert len(hits) == 1, [str(i.message) for i in w]
        assert_parity(y.cpu(), ref, 2e-4, case + " [strict re-run]")
    else:
        assert not hits, [str(i.message) for i in hits]
        assert_parity(y.cpu(), ref, 1e-3, case + " [fast path, nothing saturated]")
    mi355attn.range_status(wait=True)                       # nothing left pending for the next caller
    # a second call behaves the same (the arm / wait state is per forward)
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        with torch.no_grad():
            y2 = md(xd, *fwd_args)
    assert torch.equal(y, y2)


def test_range_fallback_off_keeps_the_round3_contract():
    """"range_fallback" = 0: no wait, the forward returns whatever fp16 produced and the NEXT 16-bit launch raises Mi355RangeError."""
    import mi355attn
    from mi355attn.modules import Attention
    m = _seeded(lambda: Attention(768, 12)).cuda()
    torch.manual_seed(4321)
    x = (torch.randn(4, 197, 768) * 1e5).cuda()
    mi355attn.range_status(wait=True)
    try:
        with mi355attn.options(range_fallback=0):
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                with torch.no_grad():
                    y = m(x)
                torch.cuda.synchronize()
            assert not [i for i in w if "strict mode" in str(i.message)]
            assert not torch.isfinite(y).all()
            with pytest.raises(mi355attn.Mi355RangeError):
                with torch.no_grad():
                    m(x)
    finally:
        try:
            mi355attn.range_status(wait=True)
        except mi355attn.Mi355RangeError:
            pass


def test_range_wait_does_not_wait_for_launches_behind_the_last_producer():
    """mi355_range_wait synchronises on ONE event behind the last fp16 producer.  With the prediction "the first producer is the last"
    (mi355_range_arm(1 + 1)) the event is recorded in front of the first launch behind the cast16: with ~4 ms of non-reporting copies queued
    behind it the wait returns while they are still running.  Without a prediction (arm(1)) the event goes to the tail: the same wait
    drains the stream -- correct, just without the slack."""
    import mi355attn
    from mi355attn import functional as F
    L = mi355attn.lib()
    dev = torch.device("cuda", 0)
    x = torch.randn(1 << 20, device=dev)
    big = torch.empty(1 << 28, dtype=torch.float32, device=dev)        # 1 GiB: the copy behind the producer takes ~0.5 ms
    dst = torch.empty_like(big)
    torch.cuda.synchronize()
    busy = {}
    for arm in (2, 1):
        assert L.mi355_range_arm(arm) == 0
        try:
            F.cast16(x, 1)                                             # the one producer
            for _ in range(8):
                F.stream_copy(big, dst)                                # ~4 ms of non-reporting work behind it
            done = torch.cuda.Event()
            done.record()
            assert L.mi355_range_wait() == 0
            busy[arm] = not done.query()
            assert L.mi355_range_launches() == 1
        finally:
            L.mi355_range_arm(0)
        torch.cuda.synchronize()
    assert busy[2], "with the prediction, mi355_range_wait must not drain the stream"
    assert not busy[1], "without a prediction the event is recorded at the tail"
