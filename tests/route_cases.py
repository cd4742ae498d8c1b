"""Dispatch-route table of the transformer drop-ins (tests/test_routes_cpu.py, tests/test_routes_gpu.py,
tests/golden/make_live_reference.py).

CSWinBlock, MixerLayer, XCABlock, Attention and TransformerEncoder do not run one kernel sequence each: their forward picks a
composition from shape / precision predicates (mi355attn/modules/{cswin,mixer,xcit,vit}.py).  One row per (module class, route):

  id        unique row name
  mod, cls  import path and class, the same in the drop-in package and the reference (cases.py convention)
  args, kwargs, shape, fwd_args
            constructor arguments, input shape of the seed protocol (oracle/params.py), extra forward arguments
  oracle    (x, state_dict, dtype) -> output: the fp64 restatement of oracle/*.py
  route     what the row runs at precision 1 / 2, in words
  tags      substrings each of which must appear in some mi355attn.kernel_trace tag at precision 1 and 2
  absent    substrings no tag may contain at precision 1 and 2 (absent_fp16: at precision 1 only)
  claims    predicate name -> value at precision 1 and 2 (predicate_values below computes them the way forward() does)
  cached    parameters whose derived copy the route caches (_ln_folded16, weight16_scaled, weight16_padk, mlp_fused_w1, lnfold):
            the GPU test rescales them in place and re-runs
  fold16    XCABlock rows: whether weight16_scaled folds gamma1 into the fp16 projection (eta = 1e-5 twins: no)
  options   library options set for the row (restored afterwards)
  error     the forward raises Mi355Error matching this text at every precision (no kernel is built for the route)

Every row gets non-trivial parameters from prep_nontrivial: LayerNorm affine parts, every bias, BatchNorm statistics and the
XCiT LayerScales, drawn per channel.  GEMM weights keep their init scale (test_range_guard_gpu.py,
test_non_default_init_weights_vit_and_cswin: larger weights measure softmax amplification, not the kernels).
"""
import torch

import oracle as O

_CSWIN, _XCIT, _VIT, _MIXER = "vision_transformers.cswin", "vision_transformers.xcit", "vision_transformers.ViT", "mlps.mlp_mixer"


def _cswin(reso, heads, split, last=False):
    return lambda x, sd, dt: O.cswin_block_forward(x, sd, reso, heads, split, last, dt)


def _xcab(heads, H, W):
    return lambda x, sd, dt: O.xca_block_forward(x, sd, heads, H, W, dt)


def _mixer(x, sd, dt):
    return O.mixer_layer_forward(x, sd, dt)


def _vit_attn(heads):
    return lambda x, sd, dt: O.vit_attention_forward(x, sd, heads, dt)


def _vit_enc(heads):
    return lambda x, sd, dt: O.vit_encoder_forward(x, sd, heads, dt)


LEPE16 = "win_attn_kernel<d=32,lepe,io16>"
LN_GEMM = "gemm16_ws_kernel<ln,"                   # mi355_ln_linear16_fwd: LayerNorm applied in the GEMM's A staging
LN16 = "layernorm_kernel<out16>"
FP32_GEMM = "_kernel<prec "                         # gemm_kernel / gemm_small_kernel: fp32 operands (staged to 16 bit at precision 1 / 2)


def _xca_pair(rid, dim, heads, shape, H, W, tags, absent, claims, cached, fold_tags=(), fold_absent=(), **kw):
    """An XCABlock row at eta = 1 (per-channel LayerScales ~ U(0.5, 1.5): the fp16 fold of gamma into W is taken) and its
    eta = 1e-5 twin (gamma * W would be subnormal in fp16: the scale stays in the fp32 epilogue).  At eta = 1e-5 every branch moves
    the output by ~1e-5 of its size, below any bar: the twin pins the route and the fold decision, the eta = 1 row the arithmetic,
    so the twin has no in-place update step."""
    base = dict(mod=_XCIT, cls="XCABlock", args=(dim, heads), shape=shape, fwd_args=(H, W), oracle=_xcab(heads, H, W), claims=claims)
    kw1 = dict(kw, qkv_bias=kw.get("qkv_bias", True))
    return [dict(base, id=rid, kwargs=dict(kw1, eta=1.0), tags=tags + tuple(fold_tags), absent=absent, fold16=True,
                 cached=cached + ("gamma1", "gamma2"), route=f"XCABlock C={dim}: LayerScale folded into W (fp16)"),
            dict(base, id=rid + "_eta", kwargs=dict(kw1, eta=1e-5), tags=tags, absent=absent, absent_fp16=tuple(fold_absent), fold16=False,
                 cached=(), route=f"XCABlock C={dim}: LayerScale in the fp32 epilogue (eta 1e-5)")]


ROWS = [
    # ---- CSWinBlock (cswin.py forward) -----------------------------------------------------------------------------------------
    # stripe kernel edge: reso * split == 64 takes it, 128 does not
    dict(id="cswin_c64_stripe_rs64", mod=_CSWIN, cls="CSWinBlock", args=(64, 16, 2), kwargs=dict(split_size=4, qkv_bias=True),
         shape=(1, 256, 64), oracle=_cswin(16, 2, 4), route="stripe kernel (LN+qkv+both branches) + proj_mlp_fused",
         tags=("cswin_stripe_kernel<C=64>", "mlp_fused_kernel<C=64,proj>"), absent=("win_attn_kernel", LN_GEMM, LN16),
         claims=dict(fast_gemm_ok=True, cswin_head32=True, cswin_stripe_ok=True, ln_linear16_ok=True, proj_mlp_fused_ok=True,
                     mlp_fused_ok=True), cached=("norm1.weight", "norm2.weight")),
    dict(id="cswin_c64_pair_rs128", mod=_CSWIN, cls="CSWinBlock", args=(64, 16, 2), kwargs=dict(split_size=8, qkv_bias=True),
         shape=(3, 256, 64), oracle=_cswin(16, 2, 8), route="ln_linear16 + LePE pair kernel + proj_mlp_fused",
         tags=(LN_GEMM, LEPE16, "mlp_fused_kernel<C=64,proj>"), absent=("cswin_stripe", LN16),
         claims=dict(fast_gemm_ok=True, cswin_head32=True, cswin_stripe_ok=False, ln_linear16_ok=True, proj_mlp_fused_ok=True,
                     mlp_fused_ok=True), cached=("norm1.weight", "norm2.weight")),
    # split_size 7 at C = 64 (no stripe kernel), qkv without bias
    dict(id="cswin_c64_split7_nobias", mod=_CSWIN, cls="CSWinBlock", args=(64, 14, 2), kwargs=dict(split_size=7),
         shape=(1, 196, 64), oracle=_cswin(14, 2, 7), route="ln_linear16 (zero qkv bias) + LePE pair kernel + proj_mlp_fused",
         tags=(LN_GEMM, LEPE16, "mlp_fused_kernel<C=64,proj>"), absent=("cswin_stripe", LN16),
         claims=dict(fast_gemm_ok=True, cswin_head32=True, cswin_stripe_ok=False, ln_linear16_ok=True, proj_mlp_fused_ok=True),
         cached=("norm1.weight",)),
    dict(id="cswin_c128_stripe", mod=_CSWIN, cls="CSWinBlock", args=(128, 8, 4), kwargs=dict(split_size=2, qkv_bias=True),
         shape=(3, 64, 128), oracle=_cswin(8, 4, 2), route="stripe kernel at C = 128 + proj_mlp_fused",
         tags=("cswin_stripe_kernel<C=128>", "mlp_fused_kernel<C=128,proj>"), absent=("win_attn_kernel", LN16),
         claims=dict(fast_gemm_ok=True, cswin_stripe_ok=True, ln_linear16_ok=True, proj_mlp_fused_ok=True, mlp_fused_ok=True),
         cached=("norm1.weight", "norm2.weight")),
    # mlp_ratio != 4: neither fused MLP kernel; proj GEMM, standalone LayerNorm, two GEMMs
    dict(id="cswin_c64_mlp2", mod=_CSWIN, cls="CSWinBlock", args=(64, 8, 2), kwargs=dict(split_size=2, mlp_ratio=2., qkv_bias=True),
         shape=(3, 64, 64), oracle=_cswin(8, 2, 2), route="stripe kernel + proj GEMM + layernorm16 + plain MLP",
         tags=("cswin_stripe_kernel<C=64>", LN16), absent=("mlp_fused", "win_attn_kernel"),
         claims=dict(fast_gemm_ok=True, cswin_stripe_ok=True, proj_mlp_fused_ok=False, mlp_fused_ok=False), cached=("norm1.weight",)),
    # C = 256: standalone layernorm16 before qkv, pair kernel, proj GEMM that also writes norm2(x) (linear16_ln16)
    dict(id="cswin_c256_reso14", mod=_CSWIN, cls="CSWinBlock", args=(256, 14, 8), kwargs=dict(split_size=7, qkv_bias=True),
         shape=(1, 196, 256), oracle=_cswin(14, 8, 7), route="layernorm16 + qkv GEMM + LePE pair + linear16_ln16 + MLP",
         tags=(LN16, LEPE16, "resid+ln16"), absent=("mlp_fused", "mlp_wide", LN_GEMM, "cswin_stripe"),
         claims=dict(fast_gemm_ok=True, cswin_stripe_ok=False, ln_linear16_ok=False, proj_mlp_fused_ok=False, mlp_fused_ok=False),
         cached=()),
    dict(id="cswin_c256_mlp_wide", mod=_CSWIN, cls="CSWinBlock", args=(256, 14, 8), kwargs=dict(split_size=7, qkv_bias=True),
         shape=(3, 196, 256), oracle=_cswin(14, 8, 7), options=dict(mlp_wide=1), route="as above, MLP on the fused kernel (option mlp_wide)",
         tags=(LN16, LEPE16, "mlp_wide_kernel<C=256>"), absent=("resid+ln16", LN_GEMM),
         claims=dict(fast_gemm_ok=True, ln_linear16_ok=False, proj_mlp_fused_ok=False, mlp_fused_ok=True), cached=("norm2.weight",)),
    # reso == split: the one-branch last stage at C = 256 (the twin of cswin_c256_reso14)
    dict(id="cswin_c256_reso_eq_split", mod=_CSWIN, cls="CSWinBlock", args=(256, 7, 8), kwargs=dict(split_size=7, qkv_bias=True),
         shape=(3, 49, 256), oracle=_cswin(7, 8, 7), route="one full-window branch (reso == split) + linear16_ln16",
         tags=(LN16, LEPE16, "resid+ln16"), absent=("cswin_stripe", LN_GEMM, "mlp_fused"),
         claims=dict(fast_gemm_ok=True, cswin_head32=True, cswin_branch2=False, cswin_stripe_ok=False, ln_linear16_ok=False),
         cached=()),
    dict(id="cswin_c512_last", mod=_CSWIN, cls="CSWinBlock", args=(512, 7, 16), kwargs=dict(split_size=7, qkv_bias=True, last_stage=True),
         shape=(1, 49, 512), oracle=_cswin(7, 16, 7, True), route="last stage at C = 512: layernorm16, one branch, proj, layernorm16, MLP",
         tags=(LN16, LEPE16), absent=("resid+ln16", "mlp_fused", LN_GEMM),
         claims=dict(fast_gemm_ok=True, cswin_head32=True, cswin_branch2=False, ln_linear16_ok=False, mlp_fused_ok=False),
         cached=()),
    # head width != 32 (CSWin-B / -L: 96 channels, 4 heads -> 24 per head): no LePE kernel is built for it -- a clean error
    dict(id="cswin_b_head24", mod=_CSWIN, cls="CSWinBlock", args=(96, 8, 4), kwargs=dict(split_size=2, qkv_bias=True),
         shape=(1, 64, 96), oracle=_cswin(8, 4, 2), route="fp32 route; the LePE core refuses head width 24",
         tags=(), absent=(), error="head dim 24",
         claims=dict(fast_gemm_ok=False, cswin_head32=False, cswin_stripe_ok=False, ln_linear16_ok=False), cached=()),
    # ---- MixerLayer (mixer.py forward) -----------------------------------------------------------------------------------------
    dict(id="mixer_fused_c256", mod=_MIXER, cls="MixerLayer", args=(256, 196), shape=(1, 196, 256), oracle=_mixer,
         route="fused token kernel + layernorm16 + channel MLP", tags=("mixer_token_kernel", LN16),
         absent=("layernorm16_t", FP32_GEMM), claims=dict(mixer_token_ok=True, mixer_channel_major=True, fast_gemm_ok=True),
         cached=("token_mlp.fc1.weight",)),
    # C = 1024 (T = 512) is the widest fused geometry; C = 1280 leaves both 16-bit token routes
    dict(id="mixer_fused_c1024", mod=_MIXER, cls="MixerLayer", args=(1024, 196), shape=(3, 196, 1024), oracle=_mixer,
         route="fused token kernel at its widest (C 1024, T 512)", tags=("mixer_token_kernel",),
         absent=("layernorm16_t", FP32_GEMM), claims=dict(mixer_token_ok=True, fast_gemm_ok=True), cached=()),
    dict(id="mixer_c1280_fp32_token", mod=_MIXER, cls="MixerLayer", args=(1280, 196), shape=(1, 196, 1280), oracle=_mixer,
         route="fp32 token_mix (C > 1024) + 16-bit channel MLP", tags=(FP32_GEMM, LN16),
         absent=("mixer_token", "layernorm16_t"), claims=dict(mixer_token_ok=False, mixer_channel_major=False, fast_gemm_ok=True),
         cached=()),
    # N = 49 (7 x 7 patches): the strict run raised Mi355Error before token_mix zero-padded the reduction axis to a multiple of 4
    dict(id="mixer_n49_channel_major", mod=_MIXER, cls="MixerLayer", args=(128, 49), shape=(3, 49, 128), oracle=_mixer,
         route="layernorm16_t + linear16 (padded K) + linear16_tr", tags=("layernorm16_t_kernel", "gemm16_kernel<transposed out>"),
         absent=("mixer_token", FP32_GEMM), claims=dict(mixer_token_ok=False, mixer_channel_major=True, fast_gemm_ok=True),
         cached=("token_mlp.fc1.weight",)),
    # the same error at every precision here (N = 49), before the padding
    dict(id="mixer_t48_fp32", mod=_MIXER, cls="MixerLayer", args=(96, 49), shape=(1, 49, 96), oracle=_mixer,
         route="T % 64 != 0 and K % 64 != 0: fp32 token_mix and fp32 channel MLP", tags=(FP32_GEMM,),
         absent=("mixer_token", "layernorm16_t", "gemm16", "out16"),
         claims=dict(mixer_token_ok=False, mixer_channel_major=False, fast_gemm_ok=False), cached=()),
    # ---- XCABlock (xcit.py forward) -------------------------------------------------------------------------------------------
    *_xca_pair("xcab_c64", 64, 2, (3, 63, 64), 7, 9, tags=(LN_GEMM, "mlp_fused_kernel<C=64>", "<ln>"), absent=(LN16,),
               claims=dict(fast_gemm_ok=True, ln_linear16_ok=True, mlp_fused_ok=True), cached=("norm1.weight", "norm2.weight")),
    *_xca_pair("xcab_c128", 128, 4, (1, 196, 128), 14, 14, tags=(LN_GEMM, "mlp_fused_kernel<C=128>", "lpi_patch_kernel<ln>"),
               absent=(LN16,), claims=dict(fast_gemm_ok=True, ln_linear16_ok=True, mlp_fused_ok=True),
               cached=("norm1.weight", "norm2.weight")),
    *_xca_pair("xcab_c256", 256, 8, (3, 49, 256), 7, 7, tags=(LN16,), absent=(LN_GEMM, "mlp_fused"),
               claims=dict(fast_gemm_ok=True, ln_linear16_ok=False, mlp_fused_ok=False), cached=(),
               fold_tags=("resid+stats",), fold_absent=("resid+stats",)),
    *_xca_pair("xcab_c64_mlp2", 64, 2, (1, 35, 64), 5, 7, mlp_ratio=2., qkv_bias=False, tags=(LN_GEMM, LN16), absent=("mlp_fused",),
               claims=dict(fast_gemm_ok=True, ln_linear16_ok=True, mlp_fused_ok=False), cached=("norm1.weight",)),
    dict(id="xcab_c96_fp32", mod=_XCIT, cls="XCABlock", args=(96, 2), kwargs=dict(qkv_bias=True, eta=1.0), shape=(3, 20, 96),
         fwd_args=(4, 5), oracle=_xcab(2, 4, 5), route="K % 64 != 0: the fp32 route at every precision (d = 48)",
         tags=("xca_kernel<d=48>", "layernorm_kernel<out32>"), absent=("gemm16", "out16", LN_GEMM, "mlp_fused"),
         claims=dict(fast_gemm_ok=False, ln_linear16_ok=False), cached=()),
    # ---- ViT Attention / TransformerEncoder (vit.py) ----------------------------------------------------------------------------
    # N = 224 keeps K / V resident (attn.hip), N = 225 streams them (sdpa_general.hip), both inside mhsa16
    dict(id="vit_attn_n224", mod=_VIT, cls="Attention", args=(256, 4), kwargs=dict(qkv_bias=True), shape=(1, 224, 256),
         oracle=_vit_attn(4), route="mhsa16, K/V-resident core", tags=("win_attn_kernel<d=64,io16>",), absent=("sdpa_stream",),
         claims=dict(fast_gemm_ok=True, sdpa_widths=True, vit_resident_core=True), cached=()),
    dict(id="vit_attn_n225", mod=_VIT, cls="Attention", args=(256, 4), kwargs=dict(qkv_bias=True), shape=(3, 225, 256),
         oracle=_vit_attn(4), route="mhsa16, streaming core", tags=("sdpa_stream_kernel<d=64",), absent=("win_attn_kernel",),
         claims=dict(fast_gemm_ok=True, sdpa_widths=True, vit_resident_core=False), cached=()),
    dict(id="vit_attn_d48_padded", mod=_VIT, cls="Attention", args=(192, 4), kwargs=dict(qkv_bias=True), shape=(3, 50, 192),
         oracle=_vit_attn(4), route="odd head width 48: zero-padded projections + streaming core at d = 64",
         tags=("sdpa_stream_kernel<d=64",), absent=("win_attn_kernel",), claims=dict(fast_gemm_ok=True, sdpa_widths=False), cached=()),
    dict(id="vit_attn_k96_fp32", mod=_VIT, cls="Attention", args=(96, 3), kwargs=dict(qkv_bias=True), shape=(1, 197, 96),
         oracle=_vit_attn(3), route="K % 64 != 0: fp32-input GEMMs + fp32-I/O resident core",
         tags=(FP32_GEMM, "win_attn_kernel<d=32>"), absent=("io16", "gemm16", "sdpa_stream"),
         claims=dict(fast_gemm_ok=False, sdpa_widths=True, vit_resident_core=True), cached=()),
    dict(id="vit_enc_c256", mod=_VIT, cls="TransformerEncoder", args=(256, 4), kwargs=dict(qkv_bias=True), shape=(3, 65, 256),
         oracle=_vit_enc(4), route="layernorm16 + mhsa16 + layernorm16 + MLP (both GELUs)", tags=(LN16, "win_attn_kernel<d=64,io16>"),
         absent=("ln_center16",), claims=dict(fast_gemm_ok=True, sdpa_widths=True, ln_fold_ok=False), cached=()),
    dict(id="vit_enc_lnfold", mod=_VIT, cls="TransformerEncoder", args=(768, 12), kwargs=dict(qkv_bias=True), shape=(1, 128, 768),
         oracle=_vit_enc(12), options=dict(ln_fold=1), route="LayerNorms folded into the GEMMs (option ln_fold)",
         tags=("ln_center16_kernel",), absent=("layernorm_kernel",), claims=dict(fast_gemm_ok=True, sdpa_widths=True, ln_fold_ok=True),
         cached=("layernorm1.weight", "layernorm2.weight")),
]

BY_ID = {r["id"]: r for r in ROWS}


# ---- non-trivial parameters --------------------------------------------------------------------------------------------------
def prep_nontrivial(module, seed=97):
    """LayerNorm gamma ~ U(0.5, 1.5) and beta ~ N(0, 0.2) per channel; every Linear / Conv2d bias ~ N(0, 0.1) (LePE get_v and the LPI
    convs included); BatchNorm affine terms and running statistics perturbed; XCiT gamma1 / gamma2 / gamma3 each rescaled by its own
    U(0.5, 1.5) draw (so eta sets their magnitude); XCA temperatures ~ U(0.5, 1.5).  Weights keep their init.  Walks the modules in
    name order, so the drop-in and the reference module get the same values."""
    g = torch.Generator().manual_seed(seed)
    nn = torch.nn
    with torch.no_grad():
        for _, m in sorted(module.named_modules(), key=lambda t: t[0]):
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, (nn.Linear, nn.Conv2d)):
                if m.bias is not None:
                    m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.2 * torch.randn(m.num_features, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.num_features, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
            for name in ("gamma1", "gamma2", "gamma3"):
                t = m._parameters.get(name)
                if t is not None:
                    t.mul_(0.5 + torch.rand(t.shape, generator=g))
            t = m._parameters.get("temperature")
            if t is not None:
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
    return module


def build_row(row, cls):
    """(module, x) of a row under the seed protocol, with non-trivial parameters."""
    from oracle.params import seeded_module_inputs
    m, x = seeded_module_inputs(lambda: cls(*row.get("args", ()), **row.get("kwargs", {})), row["shape"])
    prep_nontrivial(m)
    return m, x


# ---- the predicates forward() evaluates, computed the same way from a built module --------------------------------------------
def predicate_values(row, m, p):
    """{name: value} of every predicate the row's class consults, at precision p.  A predicate that reads a library option raises
    whatever the option read raises (the CPU test defers those to the GPU test)."""
    from mi355attn import functional as F
    cls = row["cls"]
    B, N, C = row["shape"]

    def fast(*lins):
        return all(F.fast_gemm_ok(l.in_features, l.out_features) for l in lins)

    v = {}
    if cls == "CSWinBlock":
        hidden = m.mlp.fc1.out_features
        v["fast_gemm_ok"] = fast(m.qkv, m.proj, m.mlp.fc1, m.mlp.fc2)
        v["cswin_head32"] = m.attns[0].dim // m.attns[0].num_heads == 32
        v["cswin_branch2"] = m.branch_num == 2
        v["cswin_stripe_ok"] = F.cswin_stripe_ok(C, m.patches_resolution, m.split_size, m.num_heads, p)
        v["ln_linear16_ok"] = F.ln_linear16_ok(C, 3 * C, p)
        v["proj_mlp_fused_ok"] = F.proj_mlp_fused_ok(C, hidden, p)
        v["mlp_fused_ok"] = lambda: F.mlp_fused_ok(C, hidden, p)
    elif cls == "MixerLayer":
        T, Nt = m.token_mlp.fc1.weight.shape
        v["fast_gemm_ok"] = fast(m.channel_mlp.fc1, m.channel_mlp.fc2)
        v["mixer_channel_major"] = T % 64 == 0 and C % 4 == 0 and C <= 1024
        v["mixer_token_ok"] = lambda: F.mixer_token_ok(Nt, T, C, p)
    elif cls == "XCABlock":
        v["fast_gemm_ok"] = fast(m.attn.qkv, m.attn.proj, m.mlp.fc1, m.mlp.fc2)
        v["ln_linear16_ok"] = F.ln_linear16_ok(C, 3 * C, p)
        v["mlp_fused_ok"] = lambda: F.mlp_fused_ok(C, m.mlp.fc1.out_features, p)
    elif cls in ("Attention", "TransformerEncoder"):
        at = m if cls == "Attention" else m.attn
        d = at.qkv.in_features // at.num_heads
        v["fast_gemm_ok"] = fast(at.qkv, at.proj) if cls == "Attention" else fast(at.qkv, at.proj, m.mlp.fc1, m.mlp.fc2)
        v["sdpa_widths"] = d in F.SDPA_WIDTHS
        v["vit_resident_core"] = d in (32, 64) and N <= 224
        if cls == "TransformerEncoder":
            v["ln_fold_ok"] = lambda: (F.ln_fold_ok(B * N, C, C, C, p) and F.ln_fold_ok(B * N, C, C, m.mlp.fc1.out_features, p))
    else:
        raise KeyError(cls)
    return v
