"""Whole-model table of the drop-ins (tests/test_models_cpu.py, tests/test_models_gpu.py, tests/golden/make_live_reference.py).

tests/route_cases.py pins every block route; this table pins the glue above the blocks: the stem and Merge_Block LayerNorms, the
final `norm`, ViT's cls-last layout and its three pooling branches, the bicubic position table, XCiT's ConvPatchEmbed (four or three
convs), the Fourier position rows, the cls-token concatenation and the class-attention stage with its doubled patch-token path, and
the Identity heads.  One row per (model class, configuration):

  id, mod, cls, args, kwargs, shape, fwd_args   as in route_cases.py (cls may be a factory function)
  oracle    (x, state_dict, dtype) -> output: the fp64 restatement of oracle/*.py
  route     what the row exercises, in words
  tags      substrings each of which must appear in some mi355attn.kernel_trace tag at precision 1 and 2
  absent    substrings no tag may contain at precision 1 and 2
  cached    parameters / buffers whose derived copy the model caches (16-bit weights, the bicubic position table, BatchNorm-folded
            conv rows, the Fourier rows, ClassAttentionBlock's doubled norm2 / gamma1): rescaled in place after a first forward
  options   library options set for the row (restored afterwards)
  error     the exception type the REFERENCE raises for this configuration; the drop-in must raise the same (at construction)
  covers    the (class, public option) pairs the row witnesses (tests/test_models_cpu.py holds the list that must be covered)

Parameters: the seed protocol (oracle.params.seeded_module_inputs), then route_cases.prep_nontrivial (LayerNorm affine terms, biases,
BatchNorm statistics, LayerScales, XCA temperatures), then prep_model with a generator of its own: cls_token / position_embedding
~ N(0, 0.02) where the constructor left them zero (XCiT's cls_token, xcit.py:332).  prep_nontrivial's draws stay untouched:
tests/golden/live/routes.npz depends on them.
"""
import torch
import torch.nn as nn

import oracle as O

_CSWIN, _XCIT, _VIT, _MIXER = "vision_transformers.cswin", "vision_transformers.xcit", "vision_transformers.ViT", "mlps.mlp_mixer"

LN16 = "layernorm_kernel<out16>"
LN_GEMM = "gemm16_ws_kernel<ln,"
LEPE16 = "win_attn_kernel<d=32,lepe,io16>"
VIT_RESIDENT = "win_attn_kernel<d=64,io16>"

MODEL_SEED = 211            # prep_model's generator
SECOND_SEEDS = (1235, 98, 212)   # weights, prep_nontrivial, prep_model of the second state dict (load_state_dict after a forward)


def _vit(heads, depth, pool="token"):
    return lambda x, sd, dt: O.vit_forward(x, sd, heads, depth, dt, pool)


def _cswin(depth, heads, split=(1, 2, 7, 7), dim=64):
    return lambda x, sd, dt: O.cswin_forward(x, sd, dim, depth, split, heads, dt)


def _mixer(depth):
    return lambda x, sd, dt: O.mixer_forward(x, sd, depth, dt)


def _xcit(heads, depth, cls_layers=2, tokens_norm=False, use_pos=True):
    return lambda x, sd, dt: O.xcit_forward(x, sd, heads, depth, cls_layers, dt, tokens_norm, use_pos)


def _cab(heads, tokens_norm=False, qk_scale=None):
    return lambda x, sd, dt: O.class_attention_block_forward(x, sd, heads, dt, tokens_norm, qk_scale)


_VIT_KW = dict(depths=2, num_heads=12, qkv_bias=True, num_classes=10)
_XCIT_KW = dict(patch_size=16, embed_dim=128, depth=2, num_heads=4, mlp_ratio=4, qkv_bias=True, norm_layer=nn.LayerNorm, eta=1.0,
                num_classes=10)
_CSWIN_KW = dict(patch_size=4, embed_dim=64, depth=[1, 1, 1, 1], split_size=[1, 2, 7, 7], num_heads=[2, 4, 8, 16], num_classes=10)
_XCIT_BN = ("patch_embed.proj.0.1.running_var", "patch_embed.proj.2.1.weight", "patch_embed.proj.6.1.running_mean")
_XCIT_POS = ("pos_embeder.token_projection.weight", "pos_embeder.token_projection.bias")
_XCIT_TAGS = (LN_GEMM, "xca_tr_kernel<d=32>", "lpi_patch_kernel<ln>", "mlp_fused_kernel<C=128>")

ROWS = [
    # ---- VisionTransformer (ViT.py:121-192) ---------------------------------------------------------------------------------------
    dict(id="vit_pool_token", mod=_VIT, cls="VisionTransformer", kwargs=dict(_VIT_KW), shape=(2, 3, 224, 224), oracle=_vit(12, 2),
         route="d = 64 K/V-resident core, logits from token 0 (the first PATCH token: cls is appended last)",
         tags=(LN16, VIT_RESIDENT), absent=("ln_center16", "sdpa_stream"), cached=("blocks.0.attn.qkv.weight", "head.weight"),
         covers=(("VisionTransformer", "global_pool=token"), ("VisionTransformer", "qkv_bias"))),
    dict(id="vit_pool_avg", mod=_VIT, cls="VisionTransformer", kwargs=dict(_VIT_KW, global_pool="avg"), shape=(2, 3, 224, 224),
         oracle=_vit(12, 2, "avg"), route="mean over tokens 1.. (skips patch 0, keeps cls), head", tags=(LN16, VIT_RESIDENT),
         absent=("ln_center16",), cached=("blocks.1.layernorm2.weight",), covers=(("VisionTransformer", "global_pool=avg"),)),
    dict(id="vit_pool_none", mod=_VIT, cls="VisionTransformer", kwargs=dict(_VIT_KW, global_pool="none"), shape=(2, 3, 224, 224),
         oracle=_vit(12, 2, "none"), route="no pooling: the head on every token (B, N+1, classes)", tags=(LN16, VIT_RESIDENT),
         absent=("ln_center16",), cached=(), covers=(("VisionTransformer", "global_pool=other"),)),
    dict(id="vit_rect_224x256", mod=_VIT, cls="VisionTransformer", kwargs=dict(_VIT_KW, depths=1), shape=(2, 3, 224, 256),
         oracle=_vit(12, 1), route="off the native grid: bicubic position table (cached per parameter version), 225 tokens",
         tags=(LN16, "sdpa_stream_kernel<d=64"), absent=("ln_center16",), cached=("position_embedding", "blocks.0.attn.proj.weight"),
         covers=(("VisionTransformer", "image size != image_size"),)),
    dict(id="vit_heads8_d96", mod=_VIT, cls="VisionTransformer", kwargs=dict(_VIT_KW, num_heads=8), shape=(2, 3, 224, 224),
         oracle=_vit(8, 2), route="head width 96: fp32 LayerNorms, zero-padded projections, streaming core at d = 128",
         tags=("layernorm_kernel<out32>", "sdpa_stream_kernel<d=128"),
         absent=("win_attn_kernel",), cached=("blocks.0.attn.qkv.weight",), covers=(("VisionTransformer", "num_heads=8"),)),
    dict(id="vit_heads4_d192", mod=_VIT, cls="VisionTransformer", kwargs=dict(_VIT_KW, num_heads=4), shape=(2, 3, 224, 224),
         oracle=_vit(4, 2), route="default num_heads=4 (d = 192): streaming core", tags=(LN16, "sdpa_stream_kernel<d=192"),
         absent=("win_attn_kernel",), cached=(), covers=(("VisionTransformer", "num_heads=4"),)),
    # rows = 128 images * 17 tokens = 2176 = 17 * 128: the fold's producer envelope (functional.ln_fold_ok)
    dict(id="vit_ln_fold", mod=_VIT, cls="VisionTransformer",
         kwargs=dict(_VIT_KW, image_size=32, patch_size=8, embedding_dim=768), shape=(128, 3, 32, 32), oracle=_vit(12, 2),
         options=dict(ln_fold=1), route="LayerNorms folded into the GEMMs, state carried block to block (option ln_fold)",
         tags=("ln_center16_kernel",), absent=("layernorm_kernel",),
         cached=("blocks.0.layernorm1.weight", "blocks.1.layernorm2.bias"), covers=(("VisionTransformer", "ln_fold"),)),
    # ---- CSWinTransformer (cswin.py:235-346) --------------------------------------------------------------------------------------
    dict(id="cswin_d1111", mod=_CSWIN, cls="CSWinTransformer", kwargs=dict(_CSWIN_KW), shape=(2, 3, 224, 224),
         oracle=_cswin((1, 1, 1, 1), (2, 4, 8, 16)), route="stem LN, one block per stage, Merge_Block LNs, final LN, token mean, head",
         tags=("cswin_stripe_kernel<C=64>", LEPE16, LN16), absent=(),
         cached=("stage1.0.norm1.weight", "stage2.0.norm2.weight", "merge1.conv.weight"),
         covers=(("CSWinTransformer", "num_classes>0"),)),
    dict(id="cswin_d1111_features", mod=_CSWIN, cls="CSWinTransformer", kwargs=dict(_CSWIN_KW, num_classes=0), shape=(2, 3, 224, 224),
         oracle=_cswin((1, 1, 1, 1), (2, 4, 8, 16)), route="num_classes=0: Identity head, the pooled features", tags=(LEPE16, LN16),
         absent=(), cached=(), covers=(("CSWinTransformer", "num_classes=0"),)),
    dict(id="cswin_tiny_224", mod=_CSWIN, cls="CSWin_64_12211_tiny_224", kwargs=dict(num_classes=10), shape=(2, 3, 224, 224),
         oracle=_cswin((1, 2, 21, 1), (2, 4, 8, 16)), route="the tiny factory: 25 blocks", tags=("cswin_stripe_kernel<C=64>", LEPE16),
         absent=(), cached=(), covers=(("CSWin_64_12211_tiny_224", "factory"),)),
    # ---- MLP_Mixer (mlp_mixer.py:65-79) -------------------------------------------------------------------------------------------
    dict(id="mixer_d512_p16", mod=_MIXER, cls="MLP_Mixer", kwargs=dict(dim=512, depth=2, num_classes=10), shape=(2, 3, 224, 224),
         oracle=_mixer(2), route="N = 196: fused token kernel", tags=("mixer_token_kernel", LN16), absent=(),
         cached=("blocks.0.token_mlp.fc1.weight", "blocks.1.channel_mlp.fc2.weight"), covers=(("MLP_Mixer", "patch_size=16"),)),
    dict(id="mixer_d512_p32", mod=_MIXER, cls="MLP_Mixer", kwargs=dict(dim=512, depth=2, patch_size=32, num_classes=10),
         shape=(2, 3, 224, 224), oracle=_mixer(2), route="N = 49: channel-major token mix with the zero-padded reduction axis",
         tags=("layernorm16_t_kernel", "gemm16_kernel<transposed out>"), absent=("mixer_token",),
         cached=("blocks.0.token_mlp.fc1.weight",), covers=(("MLP_Mixer", "patch_size=32"),)),
    dict(id="mixer_d256_p16", mod=_MIXER, cls="MLP_Mixer", kwargs=dict(dim=256, depth=2, num_classes=10), shape=(2, 3, 224, 224),
         oracle=_mixer(2), route="dim 256, N = 196", tags=("mixer_token_kernel",), absent=(), cached=(),
         covers=(("MLP_Mixer", "dim=256"),)),
    # ---- XCiT (xcit.py:296-414) ---------------------------------------------------------------------------------------------------
    dict(id="xcit_p16", mod=_XCIT, cls="XCiT", kwargs=dict(_XCIT_KW), shape=(2, 3, 224, 224), oracle=_xcit(4, 2),
         route="four-conv ConvPatchEmbed + Fourier rows, 2 XCABlocks, cls concat, 2 class-attention blocks, norm, head",
         tags=_XCIT_TAGS, absent=(), cached=_XCIT_BN + _XCIT_POS + ("blocks.0.gamma1", "cls_attn_blocks.0.gamma1"),
         covers=(("XCiT", "patch_size=16"), ("XCiT", "eta=1.0"), ("XCiT", "tokens_norm=False"), ("XCiT", "cls_attn_layers=2"))),
    dict(id="xcit_p8", mod=_XCIT, cls="XCiT", kwargs=dict(_XCIT_KW, patch_size=8), shape=(2, 3, 112, 112), oracle=_xcit(4, 2),
         route="three-conv ConvPatchEmbed (patch 8)", tags=_XCIT_TAGS, absent=(),
         cached=("patch_embed.proj.4.1.running_var", "patch_embed.proj.4.1.bias"), covers=(("XCiT", "patch_size=8"),)),
    dict(id="xcit_s12_tokens_norm", mod=_XCIT, cls="XCiT", kwargs=dict(_XCIT_KW, embed_dim=384, num_heads=8, depth=1, tokens_norm=True),
         shape=(2, 3, 224, 224), oracle=_xcit(8, 1, tokens_norm=True), route="S12 width (384, 8 heads): norm2 over every token",
         tags=("xca_tr_kernel<d=48>", "resid+stats", LN16), absent=(),
         cached=("cls_attn_blocks.0.norm2.weight", "cls_attn_blocks.1.norm2.bias", "cls_attn_blocks.1.gamma1"),
         covers=(("XCiT", "tokens_norm=True"),)),
    dict(id="xcit_eta_1e-5", mod=_XCIT, cls="XCiT", kwargs=dict(_XCIT_KW, eta=1e-5), shape=(2, 3, 224, 224), oracle=_xcit(4, 2),
         route="LayerScale 1e-5: the fp16 fold is declined, gamma in the fp32 epilogue", tags=(LN_GEMM, "xca_tr_kernel<d=32>"),
         absent=(), cached=(), covers=(("XCiT", "eta=1e-5"),)),
    dict(id="xcit_cls_layers1", mod=_XCIT, cls="XCiT", kwargs=dict(_XCIT_KW, cls_attn_layers=1), shape=(3, 3, 224, 224),
         oracle=_xcit(4, 2, cls_layers=1), route="one class-attention block, ragged batch", tags=_XCIT_TAGS, absent=(), cached=(),
         covers=(("XCiT", "cls_attn_layers=1"),)),
    dict(id="xcit_nopos_nobias", mod=_XCIT, cls="XCiT", kwargs=dict(_XCIT_KW, use_pos=False, qkv_bias=False), shape=(2, 3, 224, 224),
         oracle=_xcit(4, 2, use_pos=False), route="no position rows, qkv without bias", tags=(LN_GEMM, "xca_tr_kernel<d=32>"),
         absent=(), cached=_XCIT_BN, covers=(("XCiT", "use_pos=False"), ("XCiT", "qkv_bias=False"))),
    dict(id="xcit_features", mod=_XCIT, cls="XCiT", kwargs=dict(_XCIT_KW, num_classes=0), shape=(2, 3, 224, 224), oracle=_xcit(4, 2),
         route="num_classes=0: Identity head, the normed cls features", tags=_XCIT_TAGS, absent=(), cached=(),
         covers=(("XCiT", "num_classes=0"),)),
    dict(id="xcit_nano_12_p16", mod=_XCIT, cls="xcit_nano_12_p16", kwargs=dict(num_classes=10), shape=(2, 3, 224, 224),
         oracle=_xcit(4, 12), route="the nano factory: 12 XCABlocks", tags=_XCIT_TAGS, absent=(), cached=(),
         covers=(("xcit_nano_12_p16", "factory"),)),
    # eta=None multiplies None by a tensor in XCABlock (xcit.py:286)
    dict(id="xcit_eta_none", mod=_XCIT, cls="XCiT", kwargs=dict(_XCIT_KW, eta=None), shape=(2, 3, 224, 224), oracle=None,
         route="refused by the reference", tags=(), absent=(), cached=(), error=TypeError, covers=(("XCiT", "eta=None"),)),
    # ---- ClassAttentionBlock alone: its output carries the patch tokens that XCiT's final cls row hides ------------------------------
    dict(id="cab_eta1", mod=_XCIT, cls="ClassAttentionBlock", args=(128, 4), kwargs=dict(qkv_bias=True, eta=1.0), shape=(2, 197, 128),
         fwd_args=(14, 14), oracle=_cab(4), route="patch tokens 2x + 2 gamma1 LN1(x) (gamma1 doubled, cached)", tags=(), absent=(),
         cached=("gamma1", "norm1.bias"), covers=(("ClassAttentionBlock", "eta=1.0"), ("ClassAttentionBlock", "tokens_norm=False"))),
    dict(id="cab_eta1_tokens_norm", mod=_XCIT, cls="ClassAttentionBlock", args=(128, 4),
         kwargs=dict(qkv_bias=True, eta=1.0, tokens_norm=True), shape=(2, 197, 128), fwd_args=(14, 14), oracle=_cab(4, True),
         route="patch tokens 2 LN2(x + gamma1 LN1(x)) (norm2 affine doubled, cached)", tags=(), absent=(),
         cached=("norm2.weight", "norm2.bias"), covers=(("ClassAttentionBlock", "tokens_norm=True"),)),
    dict(id="cab_eta_none", mod=_XCIT, cls="ClassAttentionBlock", args=(128, 4), kwargs=dict(qkv_bias=True), shape=(2, 197, 128),
         fwd_args=(14, 14), oracle=_cab(4), route="no LayerScale (gamma = 1.0): patch tokens 2x + 2 LN1(x)", tags=(), absent=(),
         cached=(), covers=(("ClassAttentionBlock", "eta=None"),)),
    dict(id="cab_eta_none_tokens_norm", mod=_XCIT, cls="ClassAttentionBlock", args=(128, 4), kwargs=dict(qkv_bias=True, tokens_norm=True),
         shape=(3, 197, 128), fwd_args=(14, 14), oracle=_cab(4, True), route="no LayerScale, norm2 over every token", tags=(),
         absent=(), cached=("norm2.bias",), covers=()),
    dict(id="cab_nobias", mod=_XCIT, cls="ClassAttentionBlock", args=(128, 4), kwargs=dict(eta=1.0), shape=(2, 197, 128),
         fwd_args=(14, 14), oracle=_cab(4), route="qkv without bias", tags=(), absent=(), cached=(),
         covers=(("ClassAttentionBlock", "qkv_bias=False"),)),
    dict(id="cab_qk_scale", mod=_XCIT, cls="ClassAttentionBlock", args=(128, 4), kwargs=dict(qkv_bias=True, eta=1.0, qk_scale=0.5),
         shape=(2, 197, 128), fwd_args=(14, 14), oracle=_cab(4, qk_scale=0.5), route="explicit qk_scale 0.5 (default 32**-0.5)",
         tags=(), absent=(), cached=(), covers=(("ClassAttentionBlock", "qk_scale"),)),
]

BY_ID = {r["id"]: r for r in ROWS}

def prep_model(module, seed=MODEL_SEED):
    """cls_token / position_embedding ~ N(0, 0.02) where the constructor left them all zero, in parameter-name order."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in sorted(module.named_parameters(), key=lambda kv: kv[0]):
            if name.rsplit(".", 1)[-1] in ("cls_token", "position_embedding") and not t.any():
                t.copy_(0.02 * torch.randn(t.shape, generator=g))
    return module


def _ctor(row, cls):
    return lambda: cls(*row.get("args", ()), **row.get("kwargs", {}))


def build_row(row, cls):
    """(module, x) of a row: seed protocol, prep_nontrivial, prep_model."""
    from oracle.params import seeded_module_inputs
    from route_cases import prep_nontrivial
    m, x = seeded_module_inputs(_ctor(row, cls), row["shape"])
    prep_nontrivial(m)
    prep_model(m)
    return m, x


def second_state(row, cls):
    """A differently seeded non-trivial state dict of the row's model (CPU): what a trained checkpoint loads after a warm-up."""
    from route_cases import prep_nontrivial
    wseed, pseed, mseed = SECOND_SEEDS
    torch.manual_seed(wseed)
    m = _ctor(row, cls)().eval()
    prep_nontrivial(m, seed=pseed)
    prep_model(m, seed=mseed)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def rescale_cached(m, names, seed=5):
    """Multiply each named parameter / buffer in place by a per-element factor ~ U(0.6, 1.4) (positive: running_var stays valid)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name in names:
            try:
                t = m.get_parameter(name)
            except AttributeError:
                t = m.get_buffer(name)
            t.mul_((0.6 + 0.8 * torch.rand(t.shape, generator=g)).to(t.device))
