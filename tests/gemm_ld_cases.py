"""Rows of the row-stride tests of the GEMM entries (tests/test_gemm_ld_gpu.py, tests/test_gemm_ld_cpu.py): one row per entry, kernel
and epilogue of include/mi355attn.h that takes a leading-dimension argument (ldx / ldy / ldu / lda).

A row is a dict:
  id        unique name
  entry     the mi355_* symbol called, through _ffi.lib() with device pointers (`invoke` below is the one place that knows the prototypes)
  kind      which prototype / operation the row is (the keys of RULES)
  shape     (M, N, K): the smallest at which the row's kernel still tiles raggedly and that its launcher accepts on a 256-CU part (the
            row floors of gemm16_wslab / gemm16_wst / the tail split depend on the CU count; the arithmetic is next to each row)
  out16     1: Y in the 16-bit type of the precision, 0: fp32
  inputs    "b" bias, "g" gamma, "r" residual
  act       MI355_ACT_*
  opts      the options that force the kernel (mi355attn.options)
  tags      substrings that must appear among the kernel_trace tags of the call on a 256-CU part ("{p}" = f16 / bf16, "{prec}" = 0 / 1 / 2)
  dense_tags  the same for the dense call where the stride changes the kernel on purpose (row A), else the strided and the dense call must
            show the same tags
  bits      False: the bits may depend on the launch (split-K only): compared at the tolerance instead of bit for bit
  precs     (1, 2) for the 16-bit engine, (0, 1, 2) for the fp32 engine
  ld        per-row strides of the "pad" pattern where the table asks for a particular one ({"ldy": N + 1})
  patterns  the stride patterns the row runs (default: both)
  tol_prec  {output: precision whose bar it is held to} where that is not the row's precision
  ws        True: the call gets the workspace of mi355_linear16_workspace_bytes, which must not be 0 on a 256-CU part
  ref_on_device  True for the two largest rows: the float64 reference product is torch.matmul in float64 on the device

Stride patterns (strides(row, pattern)):
  dense   ld = width: the call the rest of the suite makes; the strided calls must return its bits
  pad     the smallest stride above the width that the entry's stated alignment allows: + 8 elements for 16-bit buffers, + 4 for fp32
          buffers (+ 8 for the fp32 Y of mi355_ln_linear16_fwd and mi355_linear16_res_fwd, whose header asks for ldy % 8 == 0 in both types)
  block   the operand is column block 1 of a matrix three times as wide: ldx = 3 K, ldy = 3 N, ldu = 3 N (the q of a fused qkv buffer)
"""
import math

import torch

ACT_NONE, ACT_GELU = 0, 1
TOL = {0: 5e-5, 1: 1e-3, 2: 1.2e-2}        # tests/arena_cases.TOL: the bar this family is already held to
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
PATTERNS = ("pad", "block")
LN_EPS = 1e-6

# header entries with an ldx / ldy / ldu / lda parameter that are no GEMM and have no row here, each with the reason
ELSEWHERE = {
    "mi355_axpby_fwd": "element-wise glue, not a GEMM; called with ldx / ldu / ldy != cols (and 0) by the XCiT class-attention rows of "
                       "tests/arena_cases.py (xcit_cls_block, xcit_cls_block_tn)",
}

ROWS = []


def dt16(p):
    return torch.float16 if p == 1 else torch.bfloat16


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def row(rid, entry, kind, shape, out16=0, inputs="", act=ACT_NONE, opts=None, tags=(), bits=True, precs=(1, 2), **extra):
    assert rid not in {r["id"] for r in ROWS}, rid
    opts = dict(opts or {})
    if kind in ("linear16", "x32"):
        opts.setdefault("gemm_splitk", 0 if bits else 1)
    r = dict(id=rid, entry=entry, kind=kind, shape=tuple(shape), out16=out16, inputs=inputs, act=act, opts=opts, tags=tuple(tags), bits=bits,
             precs=tuple(precs), dense_tags=None, ld={}, ws=False)
    r.update(extra)
    ROWS.append(r)
    return r


# ---- mi355_linear16_ws_fwd (and mi355_linear16_fwd for one row per kernel) -------------------------------------------------------------
WS, NOWS = "mi355_linear16_ws_fwd", "mi355_linear16_fwd"

# plain tile kernels, forced: 130 rows = one full and one 2-row tile, 132 columns = N % 8 == 4 with a partial column tile, three K-steps
for v in (1, 2, 3, 7, 9):                  # 128 x 128, 256 x 128, 256 x 256, 128 x 256, 256 x 64 tiles
    o = {"gemm_variant": v}
    row(f"tile_v{v}_out32_bgr_gelu", WS, "linear16", (130, 132, 192), 0, "bgr", ACT_GELU, o, [f"gemm16_kernel<variant {v},out32> M=130 N=132 K=192 gelu"])
    row(f"tile_v{v}_out16_b", WS, "linear16", (130, 132, 192), 1, "b", ACT_NONE, o, [f"gemm16_kernel<variant {v},out16> M=130 N=132 K=192"])
    row(f"tile_v{v}_out16_br", WS, "linear16", (130, 132, 192), 1, "br", ACT_NONE, o, [f"gemm16_kernel<variant {v},out16> M=130 N=132 K=192"])
row("tile_v7_out16_br_nows", NOWS, "linear16", (130, 132, 192), 1, "br", ACT_NONE, {"gemm_variant": 7}, ["gemm16_kernel<variant 7,out16> M=130 N=132 K=192"])

# weight-stationary short-K kernel: default dispatch from M >= 2048; 2050 rows = 16 full tiles and one of 2 rows; partial column tiles
row("ws_k64_out16_gelu", WS, "linear16", (2050, 72, 64), 1, "b", ACT_GELU, {}, ["gemm16_ws_kernel<out16> M=2050 N=72 K=64"])
row("ws_k128_out32_br", WS, "linear16", (2050, 136, 128), 0, "br", ACT_NONE, {}, ["gemm16_ws_kernel<out32> M=2050 N=136 K=128"])
row("ws_k64_out16_gelu_nows", NOWS, "linear16", (2050, 72, 64), 1, "b", ACT_GELU, {}, ["gemm16_ws_kernel<out16> M=2050 N=72 K=64"])
# Row A: the same product with a 16-bit Y at ldy = 76 = 4 (mod 8).  The kernel above stores 16-byte units to Y + m * ldy + n, so the
# dispatch hands such a Y to the plain tile kernel (8-byte stores) -- include/mi355attn.h, mi355_linear16_fwd -- and the result is the
# dense call's, bit for bit.  ("block" is 3 N = 216 = 0 (mod 8): the weight-stationary kernel again.)
row("ws_k64_out16_ldy4mod8", WS, "linear16", (2050, 72, 64), 1, "b", ACT_GELU, {}, ["gemm16_kernel<variant 1,out16> M=2050 N=72 K=64 gelu"],
    ld={"ldy": 76}, dense_tags=("gemm16_ws_kernel<out16> M=2050 N=72 K=64",), patterns=("pad",))

# two-accumulator persistent kernel, forced: whole 128 x 256 tiles only (M % 128, N % 256; fp32 outputs from ten K-tiles), or 256 x 128 tiles
# with the operand roles swapped (N % 128, M % 256); three row tiles x two column tiles is its smallest several-tiles-per-axis shape
row("pa_out32_br", WS, "linear16", (384, 512, 640), 0, "br", ACT_NONE, {"gemm_variant": 16}, ["gemm16_pa_kernel<{p},out32> M=384 N=512 K=640"])
row("pa_out16_gelu", WS, "linear16", (384, 512, 256), 1, "b", ACT_GELU, {"gemm_variant": 16}, ["gemm16_pa_kernel<{p},out16,3 pieces> M=384 N=512 K=256 gelu"])
row("pa_out16_swapped", WS, "linear16", (512, 384, 384), 1, "b", ACT_NONE, {"gemm_variant": 16}, ["gemm16_pa_kernel<{p},out16,256x128,2 pieces> M=512 N=384 K=384"])
row("pa_out32_br_nows", NOWS, "linear16", (384, 512, 640), 0, "br", ACT_NONE, {"gemm_variant": 16}, ["gemm16_pa_kernel<{p},out32> M=384 N=512 K=640"])

# persistent 256 x 256 kernel, forced: 300 rows = one full and one partial row tile
row("p8_out32_br", WS, "linear16", (300, 512, 256), 0, "br", ACT_NONE, {"gemm_variant": 15}, ["gemm16_p8_kernel<{p},out32> M=300 N=512 K=256"])
row("p8_out16_b", WS, "linear16", (300, 512, 256), 1, "b", ACT_NONE, {"gemm_variant": 15}, ["gemm16_p8_kernel<{p},out16> M=300 N=512 K=256"])
row("p8_out16_b_nows", NOWS, "linear16", (300, 512, 256), 1, "b", ACT_NONE, {"gemm_variant": 15}, ["gemm16_p8_kernel<{p},out16> M=300 N=512 K=256"])
# split-K of the left-over tiles (48 K-tiles: six chunks) through the workspace of mi355_linear16_workspace_bytes: bits may differ
row("p8_splitk_out32_br", WS, "linear16", (300, 768, 3072), 0, "br", ACT_NONE, {"gemm_variant": 15}, ["gemm16_p8_kernel<{p},out32> M=300 N=768 K=3072"],
    bits=False, ws=True)

# one wave per SIMD, 256 x 256 tiles, forced: M % 256, N % 256, 16-bit out; two tiles per axis
row("w4_out16", WS, "linear16", (512, 512, 768), 1, "b", ACT_NONE, {"gemm_variant": 17}, ["gemm16_w4_kernel<{p},out16> M=512 N=512 K=768"])
row("w4_out16_gelu", WS, "linear16", (512, 512, 768), 1, "b", ACT_GELU, {"gemm_variant": 17}, ["gemm16_w4_kernel<{p},out16> M=512 N=512 K=768 gelu"])
row("w4_out16_nows", NOWS, "linear16", (512, 512, 768), 1, "b", ACT_NONE, {"gemm_variant": 17}, ["gemm16_w4_kernel<{p},out16> M=512 N=512 K=768"])

# slab-stationary kernel, gemm_wslab = 2.  Its launcher wants four 32-row tiles per stream; on 256 CUs: K = 256 (four waves, 512 slots, N = 512
# = 2 slabs: 256 streams) 1024 tiles; K = 384 (four waves, N = 1152 = 6 slabs: 85 streams) 340 tiles; K = 512 (eight waves, 256 slots, 2 slabs:
# 128 streams) 512 tiles.  M = 32 * (tiles - 1) + 4: the last tile holds four rows, M is no multiple of 32.
WSLAB = {256: (32740, 512), 384: (10852, 1152), 512: (16356, 512)}
for K, (M, N) in WSLAB.items():
    nw = 8 if K == 512 else 4
    row(f"wslab_k{K}", WS, "linear16", (M, N, K), 1, "b", ACT_GELU if K == 384 else ACT_NONE, {"gemm_wslab": 2},
        [f"gemm16_wslab_kernel<{{p}},K{K},{nw}w> M={M} N={N}"])
row("wslab_k384_nows", NOWS, "linear16", (10852, 1152, 384), 1, "b", ACT_NONE, {"gemm_wslab": 2}, ["gemm16_wslab_kernel<{p},K384,4w> M=10852 N=1152"])

# weights in registers, default dispatch for square short products with an fp32 output: 100 rows = three full 32-row tiles and one of four rows
row("wreg_256", WS, "linear16", (100, 256, 256), 0, "br", ACT_NONE, {}, ["gemm16_wreg_kernel<{p},resid> M=100 N=256 K=256"])
row("wreg_384", WS, "linear16", (100, 384, 384), 0, "br", ACT_NONE, {}, ["gemm16_wreg_kernel<{p},resid> M=100 N=384 K=384"])
row("wreg_256_nows", NOWS, "linear16", (100, 256, 256), 0, "br", ACT_NONE, {}, ["gemm16_wreg_kernel<{p},resid> M=100 N=256 K=256"])

# weight-stationary K = 768 kernel.  Eight waves (gemm_wst = 2): N = 2304 = 12 slabs of 192, at least 8 tiles per workgroup of a slab:
# M >= 32 * 8 * (256 / 12) = 5376; 5378 leaves a two-row tile.  One wave per SIMD (gemm_wst = 4): M % 32 == 0, N = 9 slabs of 256, 28 or
# 29 streams per slab: 60 tiles give every stream two tiles and some a third.
row("wst_8wave", WS, "linear16", (5378, 2304, 768), 1, "b", ACT_GELU, {"gemm_wst": 2}, ["gemm16_wst_kernel<{p},out16> M=5378 N=2304 K=768 gelu"], ref_on_device=True)
row("wst_1wave", WS, "linear16", (1920, 2304, 768), 1, "b", ACT_NONE, {"gemm_wst": 4}, ["gemm16_wst_kernel<{p},out16> M=1920 N=2304 K=768"])
row("wst_1wave_gelu_nows", NOWS, "linear16", (1920, 2304, 768), 1, "b", ACT_GELU, {"gemm_wst": 4}, ["gemm16_wst_kernel<{p},out16> M=1920 N=2304 K=768 gelu"])

# the default tail split, the one place that offsets A, C and the residual by rows1 * ld: 130 x 2 tiles of 128 x 256 on 256 CUs = one round and
# four tiles; gemm_pa_tail = 99 lets them go to the 32 x 64 ring kernel: 16384 rows on the two-accumulator kernel, 256 on the tail
row("tail_split", WS, "linear16", (16640, 512, 1024), 0, "br", ACT_NONE, {"gemm_pa_tail": 99},
    ["gemm16_pa_kernel<{p},out32> M=16384 N=512 K=1024", "gemm16_kernel<tail 32x64> M=256 N=512 K=1024"], ref_on_device=True)

# ---- the other entries ---------------------------------------------------------------------------------------------------------------
for K, (M, N) in WSLAB.items():
    nw = 4 if K == 256 else 8
    row(f"x32_k{K}", "mi355_linear16_x32_fwd", "x32", (M, N, K), 1, "b", ACT_GELU if K == 512 else ACT_NONE, {},
        [f"gemm16_wslab_kernel<{{p}},K{K},{nw}w,x32> M={M} N={N}"])
row("stats_256", "mi355_linear16_stats_fwd", "stats", (100, 256, 256), 0, "br", tags=["gemm16_wreg_kernel<{p},resid+stats> M=100 N=256 K=256"])
row("stats_384", "mi355_linear16_stats_fwd", "stats", (100, 384, 384), 0, "r", tags=["gemm16_wreg_kernel<{p},resid+stats> M=100 N=384 K=384"])
row("ln16_256", "mi355_linear16_ln16_fwd", "ln16", (100, 256, 256), 0, "br", tags=["gemm16_wreg_kernel<{p},resid+ln16> M=100 N=256 K=256"])
for rio, oio in ((1, 1), (1, 0), (0, 1)):
    row(f"res_r{16 if rio else 32}_o{16 if oio else 32}", "mi355_linear16_res_fwd", "res", (70, 72, 128), oio, "br", ACT_GELU,
        tags=[f"gemm16_res_kernel<{{p}},r{16 if rio else 32},o{16 if oio else 32}> M=70 N=72 K=128 gelu"], resid16=rio)
for M, N, K in ((300, 72, 64), (1000, 136, 128)):
    for o16 in (0, 1):
        row(f"lnlin_k{K}_out{16 if o16 else 32}", "mi355_ln_linear16_fwd", "lnlin", (M, N, K), o16, "b", ACT_GELU if o16 else ACT_NONE,
            tags=[f"gemm16_ws_kernel<ln,{'out16' if o16 else 'out32'}> M={M} N={N} K={K}"])
row("tr_3x68", "mi355_linear16_tr_fwd", "tr", (3 * 68, 52, 128), 0, "br", tags=["gemm16_kernel<transposed out> M=204 N=52 K=128"], rows_per_image=68)
row("emit", "mi355_linear16_emit_fwd", "emit", (256, 256, 640), 0, "br", ACT_GELU, tags=["gemm16_pa_kernel<{p},out32,emit> M=256 N=256 K=640 gelu"])
row("lnfold", "mi355_linear16_lnfold_fwd", "lnfold", (300, 512, 256), 1, "b", ACT_GELU, tags=["gemm16_p8_kernel<{p},out16,fold> M=300 N=512 K=256 gelu"])
# the fp32-operand engine
L32 = "mi355_linear_fwd"
row("gemm32_vec", L32, "linear32", (130, 132, 192), 0, "bgr", ACT_GELU, tags=["gemm_kernel<prec {prec},b0,a0> batch=1 M=130 N=132 K=192"], precs=(0, 1, 2))
row("gemm32_scalar_store", L32, "linear32", (130, 132, 192), 0, "bgr", ACT_GELU, tags=["gemm_kernel<prec {prec},b0,a0> batch=1 M=130 N=132 K=192"],
    precs=(0, 1, 2), ld={"ldy": 133}, patterns=("pad",))
row("gemm32_small", L32, "linear32", (5, 10, 64), 0, "b", ACT_NONE, tags=["gemm_small_kernel<prec {prec}> M=5 N=10 K=64"], precs=(0, 1, 2),
    ld={"ldx": 68, "ldy": 13}, patterns=("pad",))
row("gemm32_alias", "mi355_gemm_bias_act_fwd", "linear32", (130, 132, 192), 0, "bgr", ACT_GELU,
    tags=["gemm_kernel<prec {prec},b0,a0> batch=1 M=130 N=132 K=192"], precs=(0, 1, 2))

# precision 3's qkv projection: fp32 rows in, five 16-bit planes out; no precision argument (run once, as "p1").  The v plane is fp16 operands
# and an fp16 result: the fp16 bar.  q and k are products of bf16 hi + lo pairs stored as hi + lo pairs (~16 mantissa bits each: the header's
# "strict operand format"): the bar of precision 0.  shape = (M, C, K)
row("qkv_split16", "mi355_qkv_split16_fwd", "qkv5", (130, 64, 192), 1, "b", tags=["qkv_split16_kernel M=130 C=64 K=192"], precs=(1,),
    tol_prec={"q": 0, "k": 0})

BY_ID = {r["id"]: r for r in ROWS}
CASES = [(r["id"], p, pat) for r in ROWS for p in r["precs"] for pat in r.get("patterns", PATTERNS)]


def case_id(c):
    return f"{c[0]}-p{c[1]}-{c[2]}"


# ---- buffers of a row ------------------------------------------------------------------------------------------------------------------
def buffers(r, p):
    """[(name, rows, width, dtype, stride key or None, "in" / "out")]: every device buffer of the row's call.  A stride key names the entry's
    leading-dimension argument that spaces the buffer's rows; None = dense."""
    M, N, K = r["shape"]
    t16, f32 = dt16(p), torch.float32
    k = r["kind"]
    yt = t16 if r["out16"] else f32
    vec = [("bias", 1, N, f32, None, "in")] if "b" in r["inputs"] else []
    if "g" in r["inputs"]:
        vec.append(("gamma", 1, N, f32, None, "in"))
    if k in ("linear16", "x32", "stats", "ln16", "res", "lnlin", "linear32", "lnfold"):
        xt = f32 if k in ("x32", "lnlin", "linear32") else t16
        wt = f32 if k == "linear32" else t16
        b = [("x", M, K, xt, "ldx", "in"), ("w", N, K, wt, None, "in")] + vec
        if "r" in r["inputs"]:
            b.append(("resid", M, N, t16 if r.get("resid16") else f32, "ldy", "in"))
        b.append(("y", M, N, yt, "ldy", "out"))
        if k == "stats":
            b.append(("stats", M, 2, f32, None, "out"))
        if k == "ln16":
            b += [("lnw", 1, N, f32, None, "in"), ("lnb", 1, N, f32, None, "in"), ("u16", M, N, t16, "ldu", "out")]
        if k == "lnfold":
            b += [("rowtau", M, 2, f32, None, "in"), ("colsum", 1, N, f32, None, "in")]
        return b
    if k == "tr":
        rpi = r["rows_per_image"]
        return [("x", M, K, t16, "ldx", "in"), ("w", N, K, t16, None, "in")] + vec + [("resid", M // rpi * N, rpi, f32, None, "in"),
                                                                                     ("y", M // rpi * N, rpi, f32, None, "out")]
    if k == "qkv5":                                                      # N is C here; the five planes come back as one int16 matrix
        return [("x", M, K, f32, "ldx", "in"), ("w_hi", 2 * N, K, torch.bfloat16, None, "in"), ("w_lo", 2 * N, K, torch.bfloat16, None, "in"),
                ("w_v", N, K, torch.float16, None, "in"), ("bias", 1, 3 * N, f32, None, "in"), ("y", M, 5 * N, torch.int16, None, "out")]
    assert k == "emit", k
    return [("x", M, K, t16, "ldx", "in"), ("w", N, K, t16, None, "in")] + vec + [
        ("resid", M, N, f32, None, "in"), ("cvec", 1, M, f32, None, "in"), ("y", M, N, f32, None, "out"), ("a16", M, N, t16, None, "out"),
        ("gstats", N // 32 * M, 2, f32, None, "out")]


def ld_keys(r):
    return sorted({b[4] for b in buffers(r, 1) if b[4]})


# the alignment (in elements) that include/mi355attn.h states for each stride argument, by kind of row; no key = no rule
RULES = {"linear16": {"ldx": 8, "ldy": 4}, "x32": {"ldx": 4, "ldy": 8}, "stats": {"ldx": 8, "ldy": 4}, "ln16": {"ldx": 8, "ldy": 4, "ldu": 4},
         "res": {"ldx": 8, "ldy": 8}, "lnlin": {"ldx": 4, "ldy": 8}, "tr": {"ldx": 8}, "emit": {"ldx": 8}, "lnfold": {"ldx": 8, "ldy": 8},
         "linear32": {"ldx": 4}, "qkv5": {}}
PRIMARY = {"ldx": "x", "ldy": "y", "ldu": "u16"}                        # the buffer whose type decides the padding of a stride (resid shares ldy)


def strides(r, p, pattern):
    """{stride key: elements} of the row's call under a pattern."""
    out = {}
    for name, rows, width, dtype, key, role in buffers(r, p):
        if key is None or PRIMARY[key] != name:
            continue
        if pattern == "dense":
            ld = width
        elif pattern == "block":
            ld = 3 * width
        else:
            ld = r["ld"].get(key, width + max(RULES[r["kind"]].get(key, 1), 4 if dtype == torch.float32 else 8))
        out[key] = ld
    return out


# ---- inputs and the float64 reference ----------------------------------------------------------------------------------------------------
def make(r, p, seed=1234):
    """CPU inputs of the row by buffer name."""
    g = torch.Generator().manual_seed(seed)
    M, N, K = r["shape"]
    d = {}
    for name, rows, width, dtype, key, role in buffers(r, p):
        if role != "in" or name in ("w_lo", "w_v"):
            continue
        if name == "w_hi":                                              # (3C, K) weight split as functional.qkv_split_weights does
            w = torch.randn(3 * N, K, generator=g) / math.sqrt(K)
            d["w_hi"] = w[:2 * N].to(torch.bfloat16)
            d["w_lo"] = (w[:2 * N] - d["w_hi"].float()).to(torch.bfloat16)
            d["w_v"] = w[2 * N:].to(torch.float16)
            continue
        if name == "w":
            t = torch.randn(rows, width, generator=g) / math.sqrt(K)
        elif name in ("gamma", "lnw"):
            t = torch.rand(rows, width, generator=g) + 0.5
        elif name in ("bias", "lnb", "colsum", "cvec"):
            t = torch.randn(rows, width, generator=g) * 0.1
        elif name == "rowtau":
            t = torch.stack([torch.rand(rows, generator=g) + 0.5, torch.randn(rows, generator=g) * 0.1], dim=1)
        else:
            t = torch.randn(rows, width, generator=g)
            if name == "x" and r["kind"] == "lnlin":
                t = t * 1.5 + 0.3
        d[name] = t.to(dtype)
    return d


def reference(r, p, d, device="cpu"):
    """{output name: float64 tensor} from the operands the kernel multiplies, widened to float64 (an fp32 activation that the entry casts
    inside the kernel is rounded to the 16-bit type first, as the header says; the fp32 engine's reference keeps the fp32 operands)."""
    k = r["kind"]
    f = lambda t: t.to(device).double()                                 # noqa: E731
    if k == "qkv5":
        C = r["shape"][1]
        w = torch.cat([f(d["w_hi"]) + f(d["w_lo"]), f(d["w_v"])])
        qkv = f(d["x"]) @ w.t() + f(d["bias"])
        return {"q": qkv[:, :C].cpu(), "k": qkv[:, C:2 * C].cpu(), "v": qkv[:, 2 * C:].cpu()}
    x = d["x"]
    if k == "x32":
        x = x.to(dt16(p))
    x = f(x)
    if k == "lnlin":
        mu = x.mean(-1, keepdim=True)
        x = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + LN_EPS)
    y = x @ f(d["w"]).t()
    del x
    if k == "lnfold":
        y = f(d["rowtau"])[:, :1] * y + f(d["rowtau"])[:, 1:] * f(d["colsum"])
    if "bias" in d:
        y = y + f(d["bias"])
    if r["act"] == ACT_GELU:
        y = gelu64(y)
    if "gamma" in d:
        y = y * f(d["gamma"])
    if k == "tr":
        rpi = r["rows_per_image"]
        M, N, K = r["shape"]
        y = y.reshape(M // rpi, rpi, N).transpose(1, 2).reshape(M // rpi * N, rpi)
    if "resid" in d:
        y = y + f(d["resid"])
    out = {"y": y}
    if k in ("stats", "ln16"):
        mu = y.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((y - mu) ** 2).mean(-1, keepdim=True) + LN_EPS)
        if k == "stats":
            out["stats"] = torch.cat([mu, rstd], dim=1)
        else:
            out["u16"] = (y - mu) * rstd * f(d["lnw"]) + f(d["lnb"])
    if k == "emit":
        M, N, K = r["shape"]
        out["a16"] = y - f(d["cvec"]).reshape(M, 1)
        grp = y.reshape(M, N // 32, 32)
        gm = grp.mean(-1)
        m2 = ((grp - gm.unsqueeze(-1)) ** 2).sum(-1)
        out["gstats"] = torch.stack([gm.t(), m2.t()], dim=-1).reshape(N // 32 * M, 2)      # stats[(n / 32) * M + m] = {mean, M2}
    return {n: t.cpu() for n, t in out.items()}


def values(r, raw):
    """{name: tensor} of what is compared with the reference, from the raw output buffers {name: tensor} (the live columns)."""
    if r["kind"] != "qkv5":
        return dict(raw)
    C = r["shape"][1]
    pl = [raw["y"][:, i * C:(i + 1) * C].contiguous() for i in range(5)]
    b = [t.view(torch.bfloat16).double() for t in pl[:4]]
    return {"q": b[0] + b[1], "k": b[2] + b[3], "v": pl[4].view(torch.float16).double()}


# ---- the call ---------------------------------------------------------------------------------------------------------------------------
def invoke(lib, r, p, P, ld, stream, ws=None, ws_bytes=0):
    """Call the row's entry.  P: buffer name -> pointer (ctypes.c_void_p, int or None); ld: stride key -> elements."""
    M, N, K = r["shape"]
    e, act, o16 = r["entry"], r["act"], r["out16"]
    g = P.get
    ldx, ldy = ld.get("ldx", K), ld.get("ldy", N)
    if e == "mi355_linear16_ws_fwd":
        return lib.mi355_linear16_ws_fwd(g("x"), g("w"), g("bias"), g("gamma"), g("resid"), g("y"), M, N, K, ldx, ldy, act, o16, p, ws, ws_bytes, stream)
    if e == "mi355_linear16_fwd":
        return lib.mi355_linear16_fwd(g("x"), g("w"), g("bias"), g("gamma"), g("resid"), g("y"), M, N, K, ldx, ldy, act, o16, p, stream)
    if e == "mi355_linear16_x32_fwd":
        return lib.mi355_linear16_x32_fwd(g("x"), g("w"), g("bias"), g("y"), M, N, K, ldx, ldy, act, p, stream)
    if e == "mi355_linear16_stats_fwd":
        return lib.mi355_linear16_stats_fwd(g("x"), g("w"), g("bias"), g("resid"), g("y"), M, N, K, ldx, ldy, p, g("stats"), LN_EPS, stream)
    if e == "mi355_linear16_ln16_fwd":
        return lib.mi355_linear16_ln16_fwd(g("x"), g("w"), g("bias"), g("resid"), g("y"), g("lnw"), g("lnb"), LN_EPS, g("u16"), M, N, K, ldx, ldy,
                                           ld.get("ldu", N), p, stream)
    if e == "mi355_linear16_res_fwd":
        return lib.mi355_linear16_res_fwd(g("x"), g("w"), g("bias"), g("resid"), p if r["resid16"] else 0, g("y"), p if o16 else 0, M, N, K, ldx,
                                          ldy, act, p, stream)
    if e == "mi355_ln_linear16_fwd":
        return lib.mi355_ln_linear16_fwd(g("x"), g("w"), g("bias"), g("y"), M, N, K, ldx, ldy, LN_EPS, act, o16, p, stream)
    if e == "mi355_linear16_tr_fwd":
        return lib.mi355_linear16_tr_fwd(g("x"), g("w"), g("bias"), g("resid"), g("y"), M, N, K, ldx, r["rows_per_image"], p, stream)
    if e == "mi355_linear16_emit_fwd":
        return lib.mi355_linear16_emit_fwd(g("x"), g("w"), g("bias"), g("resid"), g("y"), M, N, K, ldx, act, p, g("cvec"), g("a16"), g("gstats"), stream)
    if e == "mi355_linear16_lnfold_fwd":
        return lib.mi355_linear16_lnfold_fwd(g("x"), g("w"), g("bias"), g("rowtau"), g("colsum"), g("y"), M, N, K, ldx, ldy, act, p, stream)
    if e == "mi355_qkv_split16_fwd":
        return lib.mi355_qkv_split16_fwd(g("x"), g("w_hi"), g("w_lo"), g("w_v"), g("bias"), g("y"), M, N, K, ldx, stream)
    assert e in ("mi355_linear_fwd", "mi355_gemm_bias_act_fwd"), e
    return getattr(lib, e)(g("x"), g("w"), g("bias"), g("gamma"), g("resid"), g("y"), M, N, K, ldx, ldy, act, p, stream)


def misaligned(r):
    """[(stride key, ld, alignment)]: for every stride argument of the row's entry with an alignment rule in the header, an ld above the
    width that breaks the rule."""
    M, N, K = r["shape"]
    width = {"ldx": K, "ldy": N, "ldu": N}
    out = []
    for key, a in sorted(RULES[r["kind"]].items()):
        ld = width[key] + a // 2
        ld += 1 if ld % a == 0 else 0
        out.append((key, ld, a))
    return out
