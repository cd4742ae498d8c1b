"""Branch table of the multi-head attention copies in mi355attn/modules/mhsa.py (tests/test_mhsa_cases_cpu.py, tests/test_mhsa_gpu.py,
tests/golden/make_live_reference.py --mhsa-only).

The kernels under these classes have their own fp64 tests; what this table pins is the host-side composition: which weights are
padded and how, which slices reach which kernel, which derived tensors are cached, in which order H and W are read.  One row per
(class, branch), conventions of tests/route_cases.py:

  id        unique row name
  mod, cls  import path and class, the same in the drop-in package and the reference
  args, kwargs, shape, fwd_args
            constructor arguments, input shape of the seed protocol (oracle/params.py), extra forward arguments ("relpos:" / "dconvs:"
            strings go through cases.make_arg)
  oracle    (x, state_dict, dtype) -> output (a tuple for Broad_Attention): the fp64 restatement of oracle/transformer.py
  branch    what the row pins, in words
  tags      substrings each of which must appear in some mi355attn.kernel_trace tag
  absent    substrings no tag may contain
  gemms     the (N, K) of every GEMM launch of one forward, sorted: an unpadded row runs the parameters' own shapes and nothing else
            (KNNAttention adds one logits GEMM per head, N = keys, K = kernel head width)
  cached    parameters and buffers from which the branch caches a derived tensor (functional.head_padded "headpad",
            QKVSplitAttention._fused "qk_v_fused", the BatchNorm folds "dwbn_nchw" / "dwpatch", ConvAttention._AsLinear): the GPU test
            rescales them in place, then loads a second state, and re-runs after each
  perturb   ((what, oracle or None, state_dict edit or None), ...): one or two slips the row must notice -- each moves the fp64 output
            by more than SENSITIVITY rel-Frobenius (tests/test_mhsa_cases_cpu.py)
  knn       (heads, topk) of KNNAttention rows: tokens whose selection is ambiguous in fp64 are left out of the comparison
  error     error rows: name of the exception the drop-in raises at every precision; `ref_raises`: what the reference does (None: it
            runs), checked against the live record; `x_dtype` / `train`: input type and training mode of the row

Parameters: oracle.params.seeded_module_inputs, then route_cases.prep_nontrivial (every bias, the LayerNorm affine terms and the
BatchNorm state per channel; GEMM weights at init scale, for the reason route_cases.py gives).

KNN selection margin.  torch.topk is discontinuous: a token is compared only where the choice is unambiguous in fp64.  A token is
ambiguous if, for any head, its k-th and (k+1)-th largest unscaled logits differ by less than KNN_MARGIN * max|logit| of the case
(1e-4: twice the strict bar 5e-5 that mi355_qk_logits_fwd is held to).  At most KNN_MAX_AMBIGUOUS of a row's tokens may be left out;
the CPU test asserts it from the oracle alone.  Shares left out with this builder (default seeds, prep_nontrivial seed 97):
kvt_k7 1.3 %, kvt_k_eq_n 0 % (topk == N: there is no (k+1)-th logit), kvt_n300 7.3 %.  The golden case kvt_attn ((2,197,256), k = 100)
would leave out 14.7 %, which is why that shape is not a row.
"""
import torch

import oracle as O
from cases import make_arg

_VT = "vision_transformers."
SENSITIVITY = 10 * 1e-3
KNN_MARGIN = 1e-4
KNN_MAX_AMBIGUOUS = 0.10
WIDTHS = (32, 64, 128, 192, 256)


# ---- oracle closures -------------------------------------------------------------------------------------------------------------
def _mhsa(heads, H=None, W=None, sr=1, layout="qkv", relpos=None):
    def f(x, sd, dt):
        rp = make_arg(relpos) if relpos is not None else None
        return O.mhsa_forward(x, sd, heads, H, W, sr, relative_pos=rp, layout=layout, dtype=dt)
    return f


def _glob(heads, scale=None):
    return lambda x, sd, dt: O.global_attention_forward(x, sd, heads, dt, scale=scale)


def _broad(heads, dim_head):
    return lambda x, sd, dt: O.broad_attention_forward(x, sd, heads, dim_head, dt)


def _eff(query_dim, heads):
    return lambda x, sd, dt: O.qk_v_attention_forward(x, sd, query_dim, heads, dt)


def _knn(heads, topk):
    return lambda x, sd, dt: O.knn_attention_forward(x, sd, heads, topk, dt)


def _cvt(heads, swap_hw=False):
    def f(x, sd, dt):
        if not swap_hw:
            return O.conv_attention_forward(x, sd, heads, dt)
        B, C, H, W = x.shape                     # the same memory read as a (W, H) map, the result read back as (H, W)
        return O.conv_attention_forward(x.reshape(B, C, W, H), sd, heads, dt).reshape(B, C, H, W)
    return f


def _p2t(H, W, dconvs, heads, ratios, scale=None, sizes=None):
    return lambda x, sd, dt: O.pooling_attention_forward(x, sd, H, W, make_arg(dconvs), heads, ratios, dt, scale=scale, sizes=sizes)


# ---- state_dict edits of the perturbations ---------------------------------------------------------------------------------------
def _zero(*keys):
    def f(sd):
        for k in keys:
            sd[k] = torch.zeros_like(sd[k])
    return f


def _bn_reset(prefix):
    def f(sd):
        sd[prefix + ".running_mean"] = torch.zeros_like(sd[prefix + ".running_mean"])
        sd[prefix + ".running_var"] = torch.ones_like(sd[prefix + ".running_var"])
    return f


def _swap_qk(sd):
    w = sd["to_qkv.weight"]
    n = w.shape[0] // 3
    sd["to_qkv.weight"] = torch.cat([w[n:2 * n], w[:n], w[2 * n:]])


def _half_up(v):
    return int(v + 0.5)


# ---- trace tags ------------------------------------------------------------------------------------------------------------------
def _sd(d):
    return "sdpa_stream_kernel<d=%d," % d


def _only(d):
    return tuple(_sd(w) for w in WIDTHS if w != d)


def _g(*nk):
    return tuple(sorted(nk))


def _gt(*nk):
    return tuple("N=%d K=%d" % t for t in nk)


_SR_BN = ("sr.0.weight", "sr.0.bias", "sr.1.weight", "sr.1.bias", "sr.1.running_mean", "sr.1.running_var")
_CVT_CACHED = tuple("conv_proj_qkv." + s for s in ("0.weight", "0.bias", "1.weight", "1.bias", "1.running_mean", "1.running_var", "2.weight",
                                                    "2.bias")) + ("proj.weight", "proj.bias")
_QKV3 = ("q.weight", "q.bias", "k.weight", "k.bias", "v.weight", "v.bias")

ROWS = [
    # ---- Attention (setr / moat): fused qkv ---------------------------------------------------------------------------------------
    dict(id="attn_d64_ragged", mod=_VT + "setr", cls="Attention", args=(128, 2), kwargs=dict(qkv_bias=True), shape=(2, 70, 128),
         oracle=_mhsa(2), branch="width 64 on the parameters themselves, partial key tile (70 keys)",
         tags=(_sd(64),) + _gt((384, 128), (128, 128)), absent=_only(64), gemms=_g((384, 128), (128, 128)), cached=(),
         perturb=(("4 heads of 32", _mhsa(4), None), ("qkv.bias dropped", None, _zero("qkv.bias")))),
    dict(id="attn_d32_nobias", mod=_VT + "moat", cls="Attention", args=(128, 4), shape=(3, 33, 128),
         oracle=_mhsa(4), branch="width 32, qkv without bias",
         tags=(_sd(32),) + _gt((384, 128), (128, 128)), absent=_only(32), gemms=_g((384, 128), (128, 128)), cached=(),
         perturb=(("2 heads of 64", _mhsa(2), None), ("proj.bias dropped", None, _zero("proj.bias")))),
    dict(id="attn_d128", mod=_VT + "setr", cls="Attention", args=(256, 2), kwargs=dict(qkv_bias=True), shape=(1, 40, 256),
         oracle=_mhsa(2), branch="width 128 unpadded", tags=(_sd(128),) + _gt((768, 256), (256, 256)), absent=_only(128),
         gemms=_g((768, 256), (256, 256)), cached=(),
         perturb=(("4 heads of 64", _mhsa(4), None), ("qkv.bias dropped", None, _zero("qkv.bias")))),
    dict(id="attn_d192_one_head", mod=_VT + "moat", cls="Attention", args=(192, 1), shape=(2, 20, 192),
         oracle=_mhsa(1), branch="width 192 unpadded, one head", tags=(_sd(192),) + _gt((576, 192), (192, 192)), absent=_only(192),
         gemms=_g((576, 192), (192, 192)), cached=(),
         perturb=(("3 heads of 64", _mhsa(3), None), ("proj.bias dropped", None, _zero("proj.bias")))),
    dict(id="attn_d256", mod=_VT + "setr", cls="Attention", args=(256, 1), kwargs=dict(qkv_bias=True), shape=(1, 24, 256),
         oracle=_mhsa(1), branch="width 256 unpadded, one head", tags=(_sd(256),) + _gt((768, 256), (256, 256)), absent=_only(256),
         gemms=_g((768, 256), (256, 256)), cached=(),
         perturb=(("2 heads of 128", _mhsa(2), None), ("qkv.bias dropped", None, _zero("qkv.bias")))),
    dict(id="attn_d48_padded", mod=_VT + "moat", cls="Attention", args=(96, 2), shape=(2, 50, 96),
         oracle=_mhsa(2), branch="width 48 zero padded to 64: qkv rows and proj columns (head_padded)",
         tags=(_sd(64),) + _gt((384, 96), (96, 128)), absent=_only(64) + _gt((288, 96), (96, 96)), gemms=_g((384, 96), (96, 128)),
         cached=("qkv.weight", "proj.weight"),
         perturb=(("3 heads of 32", _mhsa(3), None), ("proj.bias dropped", None, _zero("proj.bias")))),
    # ---- SRAttention (pvt): separate q / k / v, depth-wise reduction + BatchNorm --------------------------------------------------
    dict(id="pvt_sr1", mod=_VT + "pvt", cls="Attention", args=(512, 8, 1), kwargs=dict(qkv_bias=True), shape=(2, 49, 512), fwd_args=(7, 7),
         oracle=_mhsa(8, 7, 7, 1, "q,k,v"), branch="sr_ratio 1 (PVT's last stage): no sr submodule, K / V from x",
         tags=(_sd(64),) + _gt((512, 512)), absent=_only(64), gemms=_g(*[(512, 512)] * 4), cached=(),
         perturb=(("4 heads of 128", _mhsa(4, 7, 7, 1, "q,k,v"), None), ("v.bias dropped", None, _zero("v.bias")))),
    dict(id="pvt_sr4", mod=_VT + "pvt", cls="Attention", args=(128, 2, 4), kwargs=dict(qkv_bias=True), shape=(2, 64, 128), fwd_args=(8, 8),
         oracle=_mhsa(2, 8, 8, 4, "q,k,v"), branch="sr_ratio 4: 4 key tokens", tags=(_sd(64),) + _gt((128, 128)), absent=_only(64),
         gemms=_g(*[(128, 128)] * 4), cached=_SR_BN,
         perturb=(("sr BatchNorm statistics reset", None, _bn_reset("sr.1")), ("sr conv bias dropped", None, _zero("sr.0.bias")))),
    dict(id="pvt_sr2_rect", mod=_VT + "pvt", cls="Attention", args=(64, 1, 2), shape=(3, 60, 64), fwd_args=(6, 10),
         oracle=_mhsa(1, 6, 10, 2, "q,k,v"), branch="H != W (6 x 10), no qkv bias", tags=(_sd(64),) + _gt((64, 64)), absent=_only(64),
         gemms=_g(*[(64, 64)] * 4), cached=_SR_BN,
         perturb=(("H and W swapped", _mhsa(1, 10, 6, 2, "q,k,v"), None), ("sr BatchNorm statistics reset", None, _bn_reset("sr.1")))),
    dict(id="pvt_d48_padded", mod=_VT + "pvt", cls="Attention", args=(96, 2, 2), kwargs=dict(qkv_bias=True), shape=(2, 48, 96),
         fwd_args=(6, 8), oracle=_mhsa(2, 6, 8, 2, "q,k,v"), branch="width 48 padded to 64: q / k / v rows, proj columns; H != W",
         tags=(_sd(64),) + _gt((128, 96), (96, 128)), absent=_only(64) + _gt((96, 96)), gemms=_g(*[(128, 96)] * 3, (96, 128)),
         cached=_QKV3 + ("proj.weight",) + _SR_BN,
         perturb=(("H and W swapped", _mhsa(2, 8, 6, 2, "q,k,v"), None), ("v.bias dropped", None, _zero("v.bias")))),
    # ---- SRAttentionRelPos (cmt) ------------------------------------------------------------------------------------------------
    dict(id="cmt_sr1_relpos", mod=_VT + "cmt", cls="Attention", args=(128,), kwargs=dict(num_heads=2, qkv_bias=True, sr_ratio=1),
         shape=(2, 35, 128), fwd_args=(5, 7, "relpos:2,35,35"), oracle=_mhsa(2, 5, 7, 1, "q,k,v", "relpos:2,35,35"),
         branch="relative_pos with Nkv == N (sr_ratio 1)", tags=(_sd(64),) + _gt((128, 128)), absent=_only(64),
         gemms=_g(*[(128, 128)] * 4), cached=(),
         perturb=(("relative_pos dropped", _mhsa(2, 5, 7, 1, "q,k,v"), None), ("v.bias dropped", None, _zero("v.bias")))),
    dict(id="cmt_sr2_relpos_rect", mod=_VT + "cmt", cls="Attention", args=(64,), kwargs=dict(num_heads=1, qkv_bias=True, sr_ratio=2),
         shape=(2, 48, 64), fwd_args=(6, 8, "relpos:1,48,12"), oracle=_mhsa(1, 6, 8, 2, "q,k,v", "relpos:1,48,12"),
         branch="H != W with relative_pos (48 x 12)", tags=(_sd(64),) + _gt((64, 64)), absent=_only(64), gemms=_g(*[(64, 64)] * 4),
         cached=_SR_BN,
         perturb=(("relative_pos dropped", _mhsa(1, 6, 8, 2, "q,k,v"), None),
                  ("H and W swapped", _mhsa(1, 8, 6, 2, "q,k,v", "relpos:1,48,12"), None))),
    # ---- SRConvAttention (segformer): q + fused kv, dense reduction conv ---------------------------------------------------------
    dict(id="seg_sr1", mod=_VT + "segformer", cls="Attention", args=(64,), kwargs=dict(num_heads=1, sr_ratio=1), shape=(2, 35, 64),
         fwd_args=(5, 7), oracle=_mhsa(1, 5, 7, 1, "q,kv"), branch="sr_ratio 1: no sr submodule, no qkv bias",
         tags=(_sd(64),) + _gt((64, 64), (128, 64)), absent=_only(64), gemms=_g((64, 64), (128, 64), (64, 64)), cached=(),
         perturb=(("2 heads of 32", _mhsa(2, 5, 7, 1, "q,kv"), None), ("proj.bias dropped", None, _zero("proj.bias")))),
    dict(id="seg_sr4_rect", mod=_VT + "segformer", cls="Attention", args=(128,), kwargs=dict(num_heads=2, qkv_bias=True, sr_ratio=4),
         shape=(2, 96, 128), fwd_args=(8, 12), oracle=_mhsa(2, 8, 12, 4, "q,kv"), branch="dense 4 x 4 conv on 8 x 12: 6 key tokens",
         tags=(_sd(64),) + _gt((128, 128), (256, 128), (128, 2048)), absent=_only(64),
         gemms=_g((128, 128), (128, 2048), (256, 128), (128, 128)), cached=(),
         perturb=(("H and W swapped", _mhsa(2, 12, 8, 4, "q,kv"), None), ("sr.bias dropped", None, _zero("sr.bias")))),
    dict(id="seg_d48_padded", mod=_VT + "segformer", cls="Attention", args=(96,), kwargs=dict(num_heads=2, sr_ratio=2), shape=(2, 48, 96),
         fwd_args=(6, 8), oracle=_mhsa(2, 6, 8, 2, "q,kv"), branch="width 48 padded to 64: q and kv rows, proj columns; H != W",
         tags=(_sd(64),) + _gt((128, 96), (256, 96), (96, 128)), absent=_only(64) + _gt((192, 96), (96, 96)),
         gemms=_g((128, 96), (96, 384), (256, 96), (96, 128)), cached=("q.weight", "kv.weight", "proj.weight"),
         perturb=(("H and W swapped", _mhsa(2, 8, 6, 2, "q,kv"), None), ("3 heads of 32", _mhsa(3, 6, 8, 2, "q,kv"), None))),
    dict(id="seg_sr2_floor", mod=_VT + "segformer", cls="Attention", args=(64,), kwargs=dict(num_heads=1, qkv_bias=True, sr_ratio=2),
         shape=(2, 35, 64), fwd_args=(5, 7), oracle=_mhsa(1, 5, 7, 2, "q,kv"),
         branch="H and W no multiples of sr_ratio: the dense conv floors as the reference does (2 x 3 key tokens)",
         tags=(_sd(64),) + _gt((64, 64), (128, 64), (64, 256)), absent=_only(64), gemms=_g((64, 64), (64, 256), (128, 64), (64, 64)), cached=(),
         perturb=(("H and W swapped", _mhsa(1, 7, 5, 2, "q,kv"), None), ("sr.bias dropped", None, _zero("sr.bias")))),
    # ---- GlobalAttention (dilateformer) ---------------------------------------------------------------------------------------
    dict(id="dilate_rect_qkscale", mod=_VT + "dilateformer", cls="GlobalAttention", args=(72,), kwargs=dict(num_heads=3, qkv_bias=True, qk_scale=0.3),
         shape=(2, 5, 9, 72), oracle=_glob(3, 0.3), branch="qk_scale given (`qk_scale or ...`), width 24 padded to 32, 5 x 9 grid",
         tags=(_sd(32),) + _gt((288, 72), (72, 96)), absent=_only(32), gemms=_g((288, 72), (72, 96)),
         cached=("qkv.weight", "qkv.bias", "proj.weight"),
         perturb=(("qk_scale ignored", _glob(3), None), ("qkv.bias dropped", None, _zero("qkv.bias")))),
    dict(id="dilate_d96_pad128", mod=_VT + "dilateformer", cls="GlobalAttention", args=(192,), kwargs=dict(num_heads=2), shape=(1, 6, 7, 192),
         oracle=_glob(2), branch="width 96 padded to 128", tags=(_sd(128),) + _gt((768, 192), (192, 256)), absent=_only(128),
         gemms=_g((768, 192), (192, 256)), cached=("qkv.weight", "proj.weight"),
         perturb=(("one head of 192", _glob(1), None), ("proj.bias dropped", None, _zero("proj.bias")))),
    # ---- Broad_Attention (bvit): returns (out, q, k, v) -------------------------------------------------------------------------
    dict(id="bvit_identity_padded", mod=_VT + "bvit", cls="Broad_Attention", args=(48,), kwargs=dict(heads=1, dim_head=48), shape=(2, 37, 48),
         oracle=_broad(1, 48), branch="heads == 1 and dim_head == dim: to_out is Identity; padded head, the module's own un-padding slice",
         tags=(_sd(64),) + _gt((192, 48)), absent=_only(64), gemms=_g((192, 48)), cached=("to_qkv.weight",),
         perturb=(("q and k blocks of to_qkv swapped", None, _swap_qk),)),
    dict(id="bvit_identity_d64", mod=_VT + "bvit", cls="Broad_Attention", args=(64,), kwargs=dict(heads=1, dim_head=64), shape=(2, 20, 64),
         oracle=_broad(1, 64), branch="to_out is Identity, no padding", tags=(_sd(64),) + _gt((192, 64)), absent=_only(64),
         gemms=_g((192, 64)), cached=(), perturb=(("q and k blocks of to_qkv swapped", None, _swap_qk),)),
    dict(id="bvit_inner_ne_dim", mod=_VT + "bvit", cls="Broad_Attention", args=(80,), kwargs=dict(heads=2, dim_head=64), shape=(2, 29, 80),
         oracle=_broad(2, 64), branch="inner width 128 != dim 80", tags=(_sd(64),) + _gt((384, 80), (80, 128)), absent=_only(64),
         gemms=_g((384, 80), (80, 128)), cached=(),
         perturb=(("one head of 128", _broad(1, 128), None), ("to_out bias dropped", None, _zero("to_out.0.bias")))),
    # ---- QKVSplitAttention (efficientformer) ----------------------------------------------------------------------------------
    dict(id="eff_dq_gt_dv", mod=_VT + "efficientformer", cls="Attention", args=(64, 256, 2), kwargs=dict(qkv_bias=True), shape=(2, 49, 64),
         oracle=_eff(256, 2), branch="dq = 128 > dv = 32: the padded width comes from the query side; v rows and proj columns padded",
         tags=(_sd(128),) + _gt((768, 64), (64, 256)), absent=_only(128), gemms=_g((768, 64), (64, 256)),
         cached=("qk.weight", "qk.bias", "v.weight", "v.bias", "proj.weight"),
         perturb=(("one head (dq 256, dv 64)", _eff(256, 1), None), ("v.bias dropped", None, _zero("v.bias")))),
    dict(id="eff_equal_nobias", mod=_VT + "efficientformer", cls="Attention", args=(128, 128, 4), shape=(2, 30, 128),
         oracle=_eff(128, 4), branch="dq == dv == 32: no padding, no bias (the fused q|k|v weight is still cached)",
         tags=(_sd(32),) + _gt((384, 128), (128, 128)), absent=_only(32), gemms=_g((384, 128), (128, 128)),
         cached=("qk.weight", "v.weight"),
         perturb=(("2 heads of 64", _eff(128, 2), None), ("proj.bias dropped", None, _zero("proj.bias")))),
    # ---- KNNAttention (kvt) ---------------------------------------------------------------------------------------------------
    dict(id="kvt_k7", mod=_VT + "kvt", cls="KNNAttention", args=(96, 4), kwargs=dict(qkv_bias=True, topk=7), shape=(3, 50, 96),
         oracle=_knn(4, 7), knn=(4, 7), branch="width 24 padded to 32, 7 of 50 keys kept",
         tags=(_sd(32),) + _gt((384, 96), (96, 128)), absent=_only(32), gemms=_g((384, 96), *[(50, 32)] * 4, (96, 128)),
         cached=("qkv.weight", "qkv.bias", "proj.weight"),
         perturb=(("topk 8", _knn(4, 8), None), ("topk 6", _knn(4, 6), None))),
    dict(id="kvt_k_eq_n", mod=_VT + "kvt", cls="KNNAttention", args=(64, 2), kwargs=dict(qkv_bias=True, topk=33), shape=(2, 33, 64),
         oracle=_knn(2, 33), knn=(2, 33), branch="topk == N: the mask keeps every key", tags=(_sd(32),) + _gt((192, 64), (64, 64)),
         absent=_only(32), gemms=_g((192, 64), *[(33, 32)] * 2, (64, 64)), cached=(),
         perturb=(("topk 32", _knn(2, 32), None),)),
    dict(id="kvt_n300", mod=_VT + "kvt", cls="KNNAttention", args=(128, 2), kwargs=dict(qkv_bias=True, topk=40), shape=(1, 300, 128),
         oracle=_knn(2, 40), knn=(2, 40), branch="rows of 257...1024 keys: the second top-k instantiation",
         tags=(_sd(64),) + _gt((384, 128), (128, 128)), absent=_only(64), gemms=_g((384, 128), *[(300, 64)] * 2, (128, 128)), cached=(),
         perturb=(("topk 41", _knn(2, 41), None), ("topk 39", _knn(2, 39), None))),
    # ---- ConvAttention (cvt): NCHW in and out ----------------------------------------------------------------------------------
    dict(id="cvt_ks3_rect", mod=_VT + "cvt", cls="Attention", args=(64,), kwargs=dict(num_heads=2, ks=3), shape=(2, 64, 5, 9),
         oracle=_cvt(2), branch="H != W (5 x 9), 3 x 3 depth-wise conv", tags=(_sd(32),) + _gt((192, 64), (64, 64)), absent=_only(32),
         gemms=_g((192, 64), (64, 64)), cached=_CVT_CACHED,
         perturb=(("H and W swapped", _cvt(2, True), None), ("BatchNorm statistics reset", None, _bn_reset("conv_proj_qkv.1")))),
    dict(id="cvt_ks7_small_map", mod=_VT + "cvt", cls="Attention", args=(48,), kwargs=dict(num_heads=2, ks=7), shape=(1, 48, 6, 4),
         oracle=_cvt(2), branch="7 x 7 window wider than the 6 x 4 map; width 24 padded to 32",
         tags=(_sd(32),) + _gt((192, 48), (48, 64)), absent=_only(32), gemms=_g((192, 48), (48, 64)), cached=_CVT_CACHED,
         perturb=(("H and W swapped", _cvt(2, True), None), ("BatchNorm statistics reset", None, _bn_reset("conv_proj_qkv.1")))),
    # ---- PoolingAttention (p2t) -------------------------------------------------------------------------------------------------
    dict(id="p2t_round_half_even", mod=_VT + "p2t", cls="PoolingAttention", args=(64,),
         kwargs=dict(num_heads=1, qkv_bias=True, pool_ratios=[2, 3, 4, 5]), shape=(2, 140, 64), fwd_args=(10, 14, "dconvs:64,4"),
         oracle=_p2t(10, 14, "dconvs:64,4", 1, [2, 3, 4, 5]),
         branch="round(10 / 4) = 2 and round(14 / 4) = 4: ties round half to even (p2t.py:78); half-up gives 3 and 4",
         tags=(_sd(64),) + _gt((64, 64), (128, 64)), absent=_only(64), gemms=_g((64, 64), (128, 64), (64, 64)), cached=(),
         perturb=(("pooled sizes rounded half up", _p2t(10, 14, "dconvs:64,4", 1, [2, 3, 4, 5],
                                                        sizes=[(_half_up(10 / r), _half_up(14 / r)) for r in (2, 3, 4, 5)]), None),
                  ("norm.bias dropped", None, _zero("norm.bias")))),
    dict(id="p2t_d40_qkscale", mod=_VT + "p2t", cls="PoolingAttention", args=(80,), kwargs=dict(num_heads=2, qk_scale=0.2), shape=(1, 49, 80),
         fwd_args=(7, 7, "dconvs:80,4"), oracle=_p2t(7, 7, "dconvs:80,4", 2, [1, 2, 3, 6], scale=0.2),
         branch="qk_scale given; 7 / 2 -> 4, 7 / 6 -> 1; width 40 padded to 64",
         tags=(_sd(64),) + _gt((128, 80), (256, 80), (80, 128)), absent=_only(64), gemms=_g((128, 80), (256, 80), (80, 128)),
         cached=("q.0.weight", "kv.0.weight", "proj.weight"),
         perturb=(("qk_scale ignored", _p2t(7, 7, "dconvs:80,4", 2, [1, 2, 3, 6]), None), ("norm.bias dropped", None, _zero("norm.bias")))),
]


# ---- error rows: the same outcome at every precision ---------------------------------------------------------------------------------
def _err(rid, mod, cls, args, kwargs, shape, fwd_args, error, ref_raises, branch, **extra):
    return dict(id=rid, mod=_VT + mod, cls=cls, args=args, kwargs=kwargs, shape=shape, fwd_args=fwd_args, oracle=None, branch=branch,
                tags=(), absent=(), cached=(), error=error, ref_raises=ref_raises, **extra)


# one small valid configuration per class: (mod, cls, args(dim, heads) -> (args, kwargs), shape(dim), fwd_args(dim, heads), dropout kw)
_TEMPLATES = (
    ("setr", "setr", "Attention", lambda C, h: ((C, h), {}), lambda C: (1, 12, C), lambda C, h: (), "attn_drop"),
    ("pvt", "pvt", "Attention", lambda C, h: ((C, h, 2), {}), lambda C: (1, 16, C), lambda C, h: (4, 4), "proj_drop"),
    ("cmt", "cmt", "Attention", lambda C, h: ((C, h, 2), {}), lambda C: (1, 16, C), lambda C, h: (4, 4, "relpos:%d,16,4" % h), "attn_drop"),
    ("seg", "segformer", "Attention", lambda C, h: ((C,), dict(num_heads=h, sr_ratio=2)), lambda C: (1, 16, C), lambda C, h: (4, 4), "proj_drop"),
    ("dilate", "dilateformer", "GlobalAttention", lambda C, h: ((C,), dict(num_heads=h)), lambda C: (1, 3, 4, C), lambda C, h: (), "attn_drop"),
    ("bvit", "bvit", "Broad_Attention", lambda C, h: ((C,), dict(heads=h, dim_head=2 * C // h if h > 1 else C)), lambda C: (1, 12, C),
     lambda C, h: (), "dropout"),
    ("eff", "efficientformer", "Attention", lambda C, h: ((C, C, h), {}), lambda C: (1, 12, C), lambda C, h: (), "proj_drop"),
    ("kvt", "kvt", "KNNAttention", lambda C, h: ((C, h), dict(topk=5)), lambda C: (1, 12, C), lambda C, h: (), "attn_drop"),
    ("cvt", "cvt", "Attention", lambda C, h: ((C,), dict(num_heads=h)), lambda C: (1, C, 3, 4), lambda C, h: (), "attn_drop"),
    ("p2t", "p2t", "PoolingAttention", lambda C, h: ((C,), dict(num_heads=h)), lambda C: (1, 36, C), lambda C, h: (6, 6, "dconvs:%d,4" % C),
     "proj_drop"),
)

ERROR_ROWS = [
    _err("err_kvt_topk_gt_n", "kvt", "KNNAttention", (64, 2), dict(qkv_bias=True, topk=34), (2, 33, 64), (), "RuntimeError", "RuntimeError",
         "topk > N: torch.topk raises in the reference as well"),
    _err("err_pvt_hw_ne_n", "pvt", "Attention", (64, 1, 2), {}, (2, 48, 64), (6, 7), "ValueError", "RuntimeError", "H * W != N"),
    _err("err_seg_hw_ne_n", "segformer", "Attention", (64,), dict(num_heads=1, sr_ratio=2), (2, 48, 64), (6, 7), "ValueError", "RuntimeError",
         "H * W != N"),
    _err("err_p2t_hw_ne_n", "p2t", "PoolingAttention", (64,), dict(num_heads=1), (1, 49, 64), (7, 6, "dconvs:64,4"), "ValueError",
         "RuntimeError", "H * W != N"),
    _err("err_pvt_h_mod_sr", "pvt", "Attention", (64, 1, 2), {}, (2, 35, 64), (5, 7), "Mi355Error", None,
         "H % sr_ratio != 0: outside the reduction kernel's stated envelope (the reference floors)", match="divisible by sr"),
    _err("err_cmt_w_mod_sr", "cmt", "Attention", (64, 1, 4), dict(qkv_bias=True), (2, 24, 64), (4, 6, "relpos:1,24,1"), "Mi355Error", None,
         "W % sr_ratio != 0 (4 x 6 grid, sr_ratio 4: the reference floors to 1 x 1)", match="divisible by sr"),
]
for _n, _m, _c, _ak, _shape, _fa, _drop in _TEMPLATES:
    _a, _k = _ak(320, 1)
    ERROR_ROWS.append(_err("err_%s_wide" % _n, _m, _c, _a, _k, _shape(320), _fa(320, 1), "ValueError", None,
                           "head width 320 > 256: ValueError from attn_head_width", match="head width 320"))
    _a, _k = _ak(64, 2)
    ERROR_ROWS.append(_err("err_%s_fp16" % _n, _m, _c, _a, _k, _shape(64), _fa(64, 2), "TypeError", "RuntimeError",
                           "fp16 input: these classes take fp32 activations", x_dtype="float16"))
    ERROR_ROWS.append(_err("err_%s_train_dropout" % _n, _m, _c, _a, dict(_k, **{_drop: 0.25}), _shape(64), _fa(64, 2), "RuntimeError", None,
                           ".train() with a non-zero dropout rate: the stochastic forward does not exist here", train=True))
ERROR_ROWS.append(_err("err_cvt_train", "cvt", "Attention", (64,), dict(num_heads=2), (1, 64, 3, 4), (), "RuntimeError", None,
                       "ConvAttention in training mode: BatchNorm would use batch statistics", train=True, match="running statistics"))

ALL_ROWS = ROWS + ERROR_ROWS
for _r in ALL_ROWS:
    for _k, _v in (("args", ()), ("kwargs", {}), ("fwd_args", ())):
        _r.setdefault(_k, _v)
BY_ID = {r["id"]: r for r in ALL_ROWS}


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def build_row(row, cls, weight_seed=None, prep_seed=97):
    """(module, x) of a row under the seed protocol with route_cases.prep_nontrivial parameters.  weight_seed / prep_seed: a second
    state for the same configuration (the GPU test loads it into the module it has already run)."""
    from oracle.params import seeded_module_inputs
    from route_cases import prep_nontrivial
    m, x = seeded_module_inputs(lambda: cls(*row.get("args", ()), **row.get("kwargs", {})), row["shape"])
    if weight_seed is not None:
        with torch.random.fork_rng():
            torch.manual_seed(weight_seed)
            m = cls(*row.get("args", ()), **row.get("kwargs", {})).eval()
    prep_nontrivial(m, prep_seed)
    if row.get("x_dtype"):
        x = x.to(getattr(torch, row["x_dtype"]))
    if row.get("train"):
        m.train()
    return m, x


def fwd_args(row, device=None):
    out = []
    for a in row.get("fwd_args", ()):
        a = make_arg(a)
        if device is not None and isinstance(a, (torch.Tensor, torch.nn.Module)):
            a = a.to(device)
        out.append(a)
    return out


def knn_unambiguous(x, sd, heads, topk):
    """(B, N) bool: tokens whose top-k key set is unambiguous in fp64 (module docstring)."""
    x = x.double()
    B, N, C = x.shape
    d = C // heads
    qkv = x @ sd["qkv.weight"].double().t()
    if "qkv.bias" in sd:
        qkv = qkv + sd["qkv.bias"].double()
    qkv = qkv.reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    logits = qkv[0] @ qkv[1].transpose(-1, -2)                      # (B, heads, N, N), unscaled
    if topk >= N:
        return torch.ones(B, N, dtype=torch.bool)
    top = torch.topk(logits, topk + 1, dim=-1)[0]
    gap = top[..., topk - 1] - top[..., topk]                       # (B, heads, N)
    return (gap >= KNN_MARGIN * float(logits.abs().max())).all(dim=1)
