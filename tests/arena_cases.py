"""Rows of the ABI memory-contract test (tests/test_abi_memory_gpu.py): one or more per entry point of include/mi355attn.h.

A row is a dict:
  id        unique name
  entries   the mi355_* symbols the row must reach (checked against what tests/arena.RecordingLib saw)
  opts      library options set for the row with mi355attn.options(...)
  prec      precision of the row: argument of the functional wrappers, default precision of a module row
  make      seed -> dict of CPU inputs: tensors, nn.Modules (their parameters and buffers are placed one by one), plain values
  run       (F, inputs on the device) -> tensor or tuple of tensors
  ref       CPU inputs -> fp64 reference(s) of the outputs that are compared (None = that output is compared bit for bit only)
  tol       parity bar of the plain run against ref: a bar an existing test file already uses for the same kernel family
  tags      substrings that must appear in mi355attn.kernel_trace tags of the arena run (256-CU parts only: the CU count enters
            the GEMM dispatch; from tests/test_gemm16_dispatch_gpu.py and tests/route_cases.py)
  bits      False: the row's result may depend on the launch (split-K): guards and inputs are checked, values compared at `tol`
  refuses_at_16B / alignment_route
            documented exceptions (none today): the entry refuses 16-byte-aligned tensors cleanly / picks another kernel for them

Every entry with an `int precision` parameter has rows at every precision it takes: 0, 1 and 2, or 1 and 2 where its operands are
16-bit buffers (tests/test_abi_memory_cpu.py reads both facts out of the header).  Every entry has a row that is ragged in each
dimension its kernel tiles, next to a model shape.

Shapes come from the tables the suite already trusts (LINEAR_SHAPES, GENERAL, CONVS, WINDOWS, the gemm16 dispatch table, route_cases.ROWS,
tests/golden/cases.py) plus shapes that are ragged in every tiled dimension.  Module-level rows run a drop-in module whose
parameters, buffers and input live in the arena; every output and workspace its functional calls allocate lands there too.
"""
import importlib
import math

import torch

import oracle as O

TOL = {0: 5e-5, 1: 1e-3, 2: 1.2e-2}        # tests/test_ops_gpu.py, tests/test_routes_gpu.py
VEC, CHAIN = 1e-5, 3e-5                     # tests/test_gpu_parity.py: fp32 vector math / longer dependent chains

EXEMPT = {
    "mi355_allgather_f32": "needs several ranks (tests/test_dist_cpu.py, MULTICHIP runs)",
    "mi355_mfma_yardstick": "measurement tool of bench.py: writes a 24-byte report, no tensor arithmetic",
    "mi355_stream_read": "measurement tool of bench.py: read-only sweep into a 4-byte sink",
    # aliases of the legacy names block: the cited line of csrc/api.hip is the one forwarding call that is the whole body
    # (tests/test_abi_memory_cpu.py checks the body and the line number)
    "mi355_sdpa_core_fwd": "alias: csrc/api.hip:498 forwards to mi355_sdpa_fwd in one call",
    "mi355_gemm_bias_act_fwd": "alias: csrc/api.hip:503 forwards to mi355_linear_fwd in one call",
    "mi355_mixer_token_mlp_fwd": "alias: csrc/api.hip:509 forwards to mi355_mixer_token_fwd in one call",
}

# options that do not select a kernel (tests/test_abi_memory_cpu.py: every OTHER key of csrc/options.h must appear in some row)
OPTIONS_NOT_COVERED = {
    "chunk_images": "chunking of the two-pass SE path by cache size: same kernels, another loop split",
    "nt": "non-temporal load / store hints of the final pass",
    "reverse": "walk order of the final pass",
    "spin_limit": "poll budget; 0 forces the time-out path, which a memory test must not provoke",
    "range_fallback": "host policy of the modules",
    "vit_tail": "host policy of VisionTransformer",
    "ws_persistent": "a caller promise about workspace reuse; the arena hands out fresh regions and forgets them on reset",
    "gemm_pa_block": "tile walk order of one kernel",
    "gemm_pa_tail": "covered where cheap (gemm_pa_tail_off row); the default tail split needs a 200 MB operand",
}

ACT_NONE, ACT_GELU = 0, 1


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dt16(p):
    return torch.float16 if p == 1 else torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape, s=1.0):
    return torch.randn(*shape, generator=g) * s


def ln64(x, w, b, eps):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.double() + b.double()


def sdpa64(q, k, v, scale, bias=None):
    """q (B,h,Nq,d) k, v (B,h,Nk,d) fp64."""
    s = q @ k.transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias
    return torch.softmax(s, dim=-1) @ v


ROWS = []


def row(**kw):
    kw.setdefault("opts", {})
    kw.setdefault("prec", 1)
    kw.setdefault("tags", ())
    kw.setdefault("bits", True)
    kw.setdefault("refuses_at_16B", False)
    kw.setdefault("alignment_route", False)
    assert kw["id"] not in {r["id"] for r in ROWS}, kw["id"]
    ROWS.append(kw)


# ---- module-level rows: tests/golden/cases.py and tests/route_cases.py ------------------------------------------------------
def _module_row(rid, c, build, oracle, entries, tol, prec=1, opts=None, tags=()):
    def make(seed):
        m, x = build()
        return dict(m=m.eval(), x=x)

    def run(F, d):
        from cases import flat_out, make_arg
        args = [make_arg(a) for a in c.get("fwd_args", ())]
        args = [a.to(d["x"].device) if isinstance(a, (torch.Tensor, torch.nn.Module)) else a for a in args]
        with torch.no_grad():
            return flat_out(d["m"](d["x"], *args))

    def ref(d):
        from cases import flat_out
        return flat_out(oracle(d["x"].float(), d["m"].state_dict(), torch.float64))

    row(id=rid, entries=entries, opts=dict(opts or {}), prec=prec, make=make, run=run, ref=ref, tol=tol, tags=tuple(tags), module=True)


def _case_rows():
    from cases import BY_ID, build_case

    def add(cid, entries, tol=None, prec=1, opts=None, suffix=""):
        c = BY_ID[cid]

        def build():
            cls = getattr(importlib.import_module(c["mod"]), c["cls"])
            return build_case(c, cls)
        _module_row(f"case_{cid}{suffix}", c, build, c["oracle"], entries, TOL[prec] if tol is None else tol, prec, opts)

    # channel gates: single-read and multi-pass kernels behind one entry; a model shape at B = 4 and a small one
    for cid, sym in (("se64", "mi355_se_fwd"), ("se256", "mi355_se_fwd"), ("se_effnet", "mi355_se_ex_fwd")):
        add(cid, (sym,), VEC)
        add(cid, (sym,), VEC, opts=dict(se_single=0), suffix="_multi")
    add("se256", ("mi355_se_fwd",), VEC, opts=dict(se_occ=2), suffix="_occ2")
    add("se_ghost", ("mi355_se_ex_fwd",), VEC)
    add("se_ghost", ("mi355_se_ex_fwd",), VEC, opts=dict(se_single=0), suffix="_multi")
    for cid in ("cbam64", "cbam256"):
        add(cid, ("mi355_cbam_fwd",), VEC)
        add(cid, ("mi355_cbam_fwd",), VEC, opts=dict(cbam_single=0), suffix="_multi")
    for cid in ("eca64", "eca256"):
        add(cid, ("mi355_eca_fwd",), VEC)
        add(cid, ("mi355_eca_fwd",), VEC, opts=dict(eca_single=0), suffix="_multi")
    for cid, sym in (("simam64", "mi355_simam_fwd"), ("srm64", "mi355_srm_fwd"), ("gctg64", "mi355_gct_gauss_fwd"), ("lct64", "mi355_lct_fwd"),
                     ("gct64", "mi355_gct_fwd"), ("gct64_l1", "mi355_gct_fwd"), ("simam256", "mi355_simam_fwd"), ("srm256", "mi355_srm_fwd"),
                     ("gctg256", "mi355_gct_gauss_fwd"), ("lct256", "mi355_lct_fwd"), ("gct256", "mi355_gct_fwd")):
        add(cid, (sym,), VEC)
        if cid.endswith("64"):
            add(cid, (sym,), VEC, opts=dict(zoo_single=0), suffix="_multi")
    add("da64", ("mi355_double_attn_fwd",))
    add("da64", ("mi355_double_attn_fwd",), opts=dict(da_fused=0), suffix="_pipeline")
    add("da64", ("mi355_double_attn_fwd",), opts=dict(da_ranges=4), suffix="_ranges4")
    add("da64", ("mi355_double_attn_fwd",), prec=0, suffix="_strict")
    add("da64", ("mi355_double_attn_fwd",), prec=2, suffix="_bf16")
    # gates from axis reductions
    for cid, sym in (("gc64", "mi355_gc_fwd"), ("gc_ragged", "mi355_gc_fwd"), ("coord64", "mi355_coordatt_fwd"),
                     ("coord_ragged", "mi355_coordatt_fwd"), ("coord_bigplane", "mi355_coordatt_fwd"), ("triplet64", "mi355_triplet_fwd"),
                     ("triplet_k5", "mi355_triplet_fwd"), ("triplet_tall", "mi355_triplet_fwd"), ("triplet_bigplane_k9", "mi355_triplet_fwd"),
                     ("bam64", "mi355_bam_fwd"), ("bam_ragged", "mi355_bam_fwd"), ("bam512", "mi355_bam_fwd"), ("sk64", "mi355_sk_fwd"),
                     ("sk_ragged", "mi355_sk_fwd"), ("sk_wide_groups", "mi355_sk_fwd")):
        add(cid, (sym,), CHAIN)
    for cid in ("cam64", "cam256"):
        add(cid, ("mi355_cam_fwd",))
    add("cam64", ("mi355_cam_fwd",), prec=0, suffix="_strict")
    for cid in ("pam64", "pam64_ragged"):
        add(cid, ("mi355_conv2d_tokens_fwd", "mi355_sdpa_general_fwd", "mi355_tokens_to_nchw_axpy_fwd"))
    # attention copies of the other ViT files: the glue entries
    add("setr_attn", ("mi355_sdpa_general_fwd",))
    add("pvt_attn_s3", ("mi355_dwconv_patch_tokens_fwd", "mi355_sdpa_general_fwd"))
    add("cmt_attn", ("mi355_dwconv_patch_tokens_fwd", "mi355_sdpa_general_fwd"))
    add("kvt_attn_small", ("mi355_qk_logits_fwd", "mi355_topk_mask_fwd", "mi355_sdpa_general_fwd"))
    add("kvt_attn", ("mi355_qk_logits_fwd", "mi355_topk_mask_fwd", "mi355_sdpa_general_fwd"))
    add("cvt_attn_d24", ("mi355_dwconv_nchw_tokens_fwd", "mi355_sdpa_general_fwd"))
    add("cvt_attn", ("mi355_dwconv_nchw_tokens_fwd", "mi355_sdpa_general_fwd"))
    add("p2t_attn_d40", ("mi355_adaptive_pool_tokens_fwd", "mi355_dwconv3x3_tokens_residual_fwd", "mi355_sdpa_general_fwd"))
    add("bvit_attn_d48", ("mi355_sdpa_general_fwd",))
    add("vit_attn_d128", ("mi355_mhsa_fwd",))
    add("xcit_cls_block", ("mi355_class_attn_fwd", "mi355_axpby_fwd"))
    add("xcit_cls_block_tn", ("mi355_class_attn_fwd", "mi355_axpby_fwd"))
    add("vit_rect", ("mi355_bicubic_rows_fwd", "mi355_axpby_fwd", "mi355_patch_embed_ws_fwd"))
    add("mixer", ("mi355_mixer_token_fwd",))
    add("mixer", ("mi355_mixer_token_fwd",), opts=dict(mixer_stats=1, mixer_early=1), suffix="_stats_early")
    add("mixer", ("mi355_layernorm16_t_fwd", "mi355_linear16_tr_fwd"), opts=dict(mixer_fused=0), suffix="_unfused")
    add("xca_block", ("mi355_xca16_fwd", "mi355_linear16_stats_fwd", "mi355_ln_lpi_stats_fwd"))
    add("xca_block", ("mi355_xca16_fwd", "mi355_mlp_fused_fwd"), opts=dict(mlp_wide=1), suffix="_mlp_wide")
    add("cswin_s1", ("mi355_cswin_stripe_attn_fwd", "mi355_proj_mlp_fused_fwd"))
    add("cswin_s1", ("mi355_cswin_stripe_attn_fwd", "mi355_proj_mlp_fused_fwd"), opts=dict(mlp_tt4=1), suffix="_tt4")
    add("cswin_s1", ("mi355_cswin_stripe_attn_fwd", "mi355_proj_mlp_fused_fwd"), prec=2, suffix="_bf16")
    add("cswin_s2", ("mi355_cswin_stripe_attn_fwd", "mi355_proj_mlp_fused_fwd"))
    add("cswin_s4", ("mi355_layernorm16_fwd", "mi355_cswin_lepe_attn16_fwd"))
    add("cswin_s4", ("mi355_cswin_lepe_attn_fwd", "mi355_layernorm_fwd", "mi355_linear_fwd"), prec=0, suffix="_strict")
    add("vit_enc", ("mi355_layernorm16_fwd", "mi355_mhsa_fwd", "mi355_linear16_ws_fwd"), opts=dict(gemm_splitk=0))
    add("vit_enc", ("mi355_layernorm16_fwd", "mi355_mhsa_fwd"), opts=dict(gemm_splitk=0, attn_nw=7), suffix="_nw7")
    add("vit_enc", ("mi355_layernorm16_fwd", "mi355_mhsa_fwd"), opts=dict(gemm_splitk=0), prec=2, suffix="_bf16")


def _route_rows():
    import route_cases as R
    entries = {
        "cswin_c64_stripe_rs64": ("mi355_cswin_stripe_attn_fwd", "mi355_proj_mlp_fused_fwd"),
        "cswin_c64_pair_rs128": ("mi355_ln_linear16_fwd", "mi355_cswin_lepe_attn16_pair_fwd", "mi355_proj_mlp_fused_fwd"),
        "cswin_c64_split7_nobias": ("mi355_ln_linear16_fwd", "mi355_cswin_lepe_attn16_pair_fwd"),
        "cswin_c128_stripe": ("mi355_cswin_stripe_attn_fwd", "mi355_proj_mlp_fused_fwd"),
        "cswin_c64_mlp2": ("mi355_cswin_stripe_attn_fwd", "mi355_layernorm16_fwd", "mi355_linear16_ws_fwd"),
        "cswin_c256_reso14": ("mi355_layernorm16_fwd", "mi355_cswin_lepe_attn16_pair_fwd", "mi355_linear16_ln16_fwd"),
        "cswin_c256_mlp_wide": ("mi355_cswin_lepe_attn16_pair_fwd", "mi355_mlp_fused_fwd"),
        "cswin_c256_reso_eq_split": ("mi355_cswin_lepe_attn16_fwd", "mi355_linear16_ln16_fwd"),
        "cswin_c512_last": ("mi355_layernorm16_fwd", "mi355_cswin_lepe_attn16_fwd"),
        "mixer_fused_c256": ("mi355_mixer_token_fwd", "mi355_layernorm16_fwd"),
        "mixer_fused_c1024": ("mi355_mixer_token_fwd",),
        "mixer_c1280_fp32_token": ("mi355_token_mix_fwd", "mi355_layernorm_fwd"),
        "mixer_n49_channel_major": ("mi355_layernorm16_t_fwd", "mi355_linear16_tr_fwd"),
        "mixer_t48_fp32": ("mi355_token_mix_fwd", "mi355_linear_fwd"),
        "xcab_c64": ("mi355_ln_linear16_fwd", "mi355_xca16_fwd", "mi355_mlp_fused_fwd", "mi355_ln_lpi_fwd"),
        "xcab_c128": ("mi355_ln_linear16_fwd", "mi355_xca16_fwd", "mi355_mlp_fused_fwd", "mi355_ln_lpi_fwd"),
        "xcab_c256": ("mi355_layernorm16_fwd", "mi355_xca16_fwd", "mi355_linear16_stats_fwd", "mi355_ln_lpi_stats_fwd"),
        "xcab_c64_mlp2": ("mi355_ln_linear16_fwd", "mi355_xca16_fwd", "mi355_layernorm16_fwd"),
        "xcab_c96_fp32": ("mi355_xca_fwd", "mi355_layernorm_fwd", "mi355_linear_fwd", "mi355_ln_lpi_fwd"),
        "vit_attn_n224": ("mi355_mhsa_fwd",),
        "vit_attn_n225": ("mi355_mhsa_fwd",),
        "vit_attn_d48_padded": ("mi355_sdpa_general_fwd",),
        "vit_attn_k96_fp32": ("mi355_linear_fwd", "mi355_sdpa_fwd"),
        "vit_enc_c256": ("mi355_layernorm16_fwd", "mi355_mhsa_fwd"),
        "vit_enc_lnfold": ("mi355_ln_center16_fwd", "mi355_linear16_emit_fwd", "mi355_ln_finalize_fwd", "mi355_linear16_lnfold_fwd"),
    }
    for r in R.ROWS:
        if r.get("error") or r["id"].endswith("_eta"):
            continue

        def build(r=r):
            cls = getattr(importlib.import_module(r["mod"]), r["cls"])
            return R.build_row(r, cls)
        opts = dict(r.get("options", {}), gemm_splitk=0)
        for p in (1, 2):
            _module_row(f"route_{r['id']}_p{p}", r, build, r["oracle"], entries[r["id"]], TOL[p], p, opts, tags=r["tags"])


# ---- the 16-bit GEMM engine: one row per kernel an option or a shape selects -------------------------------------------------
def _gemm_inputs(seed, M, N, K, inputs, p):
    g = _gen(seed)
    d = dict(x16=_rn(g, M, K).to(dt16(p)), w16=(_rn(g, N, K) / K ** 0.5).to(dt16(p)))
    d["bias"] = _rn(g, N, s=0.1) if "b" in inputs else None
    d["gamma"] = torch.rand(N, generator=g) + 0.5 if "g" in inputs else None
    d["resid"] = _rn(g, M, N) if "r" in inputs else None
    return d


def _gemm_ref(d, act):
    y = d["x16"].double() @ d["w16"].double().t()
    if d["bias"] is not None:
        y = y + d["bias"].double()
    if act == ACT_GELU:
        y = gelu64(y)
    if d["gamma"] is not None:
        y = y * d["gamma"].double()
    if d["resid"] is not None:
        y = y + d["resid"].double()
    return y


def _linear16_row(rid, M, N, K, out16, act, inputs, opts, p, tags=(), bits=True):
    opts = dict(opts)
    opts.setdefault("gemm_splitk", 0 if bits else 1)
    row(id=rid, entries=("mi355_linear16_ws_fwd",), opts=opts, prec=p, tags=tuple(tags), bits=bits, tol=TOL[p],
        make=lambda seed: _gemm_inputs(seed, M, N, K, inputs, p),
        run=lambda F, d: F.linear16(d["x16"], d["w16"], d["bias"], act=act, gamma=d["gamma"], resid=d["resid"], out16=bool(out16), precision=p),
        ref=lambda d: _gemm_ref(d, act))


def _gemm_rows():
    from test_gemm16_dispatch_gpu import ROWS as DISPATCH
    for rid, entry, (M, N, K), out16, act, inputs, opts, want in DISPATCH:
        if isinstance(want, tuple) or entry.endswith("_c") or entry == "patch_embed":
            continue
        if M * (2 * K + 10 * N) > (300 << 20):                  # operands + residual + output + reference slack: keep inside the arena
            continue
        if rid.startswith("variant_") and rid not in ("variant_7", "variant_15", "variant_16", "variant_17"):
            continue
        for p in (1, 2):
            tags = tuple(t.replace("{p}", "f16" if p == 1 else "bf16") for t in want)
            if entry == "linear16":
                _linear16_row(f"gemm_{rid}_p{p}", M, N, K, out16, act, inputs, opts, p, tags)
            elif entry == "cast_linear16":
                def make(seed, M=M, N=N, K=K, p=p):
                    d = _gemm_inputs(seed, M, N, K, "b", p)
                    d["x"] = _rn(_gen(seed + 1), M, K)
                    d["x16"] = d["x"].to(dt16(p))
                    return d
                ents = ("mi355_linear16_x32_fwd",) if "x32" in rid else ("mi355_cast16_fwd", "mi355_linear16_ws_fwd")
                row(id=f"gemm_{rid}_p{p}", entries=ents, opts=dict(opts, gemm_splitk=0), prec=p, tags=tags, tol=TOL[p], make=make,
                    run=lambda F, d, act=act, p=p: F.cast_linear16(d["x"], d["w16"], d["bias"], act=act, precision=p),
                    ref=lambda d, act=act: _gemm_ref(d, act))
            elif entry == "ln_linear16":
                def make(seed, M=M, N=N, K=K):
                    torch.manual_seed(seed)
                    ln, lin = torch.nn.LayerNorm(K), torch.nn.Linear(K, N)
                    with torch.no_grad():
                        ln.weight.copy_(0.5 + torch.rand(K))
                        ln.bias.copy_(0.2 * torch.randn(K))
                    return dict(x=torch.randn(M, K), ln=ln, lin=lin)

                def ref(d, act=act):
                    y = ln64(d["x"], d["ln"].weight, d["ln"].bias, d["ln"].eps) @ d["lin"].weight.double().t() + d["lin"].bias.double()
                    return gelu64(y) if act == ACT_GELU else y
                row(id=f"gemm_{rid}_p{p}", entries=("mi355_ln_linear16_fwd",), opts=dict(opts), prec=p, tags=tags, tol=TOL[p], make=make,
                    run=lambda F, d, act=act, out16=out16, p=p: F.ln_linear16(d["x"], d["ln"], d["lin"], act=act, out16=bool(out16), precision=p),
                    ref=ref)
            elif entry in ("linear16_stats", "linear16_ln16"):
                def make(seed, M=M, N=N, K=K, inputs=inputs, p=p):
                    d = _gemm_inputs(seed, M, N, K, inputs, p)
                    torch.manual_seed(seed)
                    d["ln"] = torch.nn.LayerNorm(N)
                    with torch.no_grad():
                        d["ln"].weight.copy_(0.5 + torch.rand(N))
                        d["ln"].bias.copy_(0.2 * torch.randn(N))
                    return d
                if entry == "linear16_stats":
                    def ref(d):
                        y = _gemm_ref(d, ACT_NONE)
                        mu = y.mean(-1)
                        return y, torch.stack([mu, 1.0 / torch.sqrt(y.var(-1, unbiased=False) + 1e-6)], dim=-1)
                    row(id=f"gemm_{rid}_p{p}", entries=("mi355_linear16_stats_fwd",), opts=dict(opts), prec=p, tags=tags, tol=TOL[p], make=make,
                        run=lambda F, d, p=p: F.linear16_stats(d["x16"], d["w16"], d["bias"], d["resid"], 1e-6, precision=p), ref=ref)
                else:
                    def ref(d):
                        y = _gemm_ref(d, ACT_NONE)
                        return y, ln64(y, d["ln"].weight, d["ln"].bias, d["ln"].eps)
                    row(id=f"gemm_{rid}_p{p}", entries=("mi355_linear16_ln16_fwd",), opts=dict(opts), prec=p, tags=tags, tol=TOL[p], make=make,
                        run=lambda F, d, p=p: F.linear16_ln16(d["x16"], d["w16"], d["bias"], d["resid"], d["ln"], precision=p), ref=ref)
    # the entry without a workspace argument has no wrapper: called through lib() directly
    def direct(F, d, out16, act, p):
        from mi355attn import _ffi
        M, K = d["x16"].shape
        N = d["w16"].shape[0]
        y = F.torch.empty(M, N, dtype=dt16(p) if out16 else torch.float32, device=d["x16"].device)
        _ffi.check(F.lib().mi355_linear16_fwd(_ffi.dptr(d["x16"]), _ffi.dptr(d["w16"]), _ffi.dptr(d["bias"]), _ffi.dptr(d["gamma"]),
                                              _ffi.dptr(d["resid"]), _ffi.dptr(y), M, N, K, K, N, act, out16, p, _ffi.stream_ptr(y.device)),
                   "mi355_linear16_fwd")
        return y
    for p in (1, 2):
        for i, (M, N, K, out16, act, inputs) in enumerate([(130, 132, 192, 0, ACT_GELU, "bgr"), (257, 516, 320, 1, ACT_NONE, "b"),
                                                           (197 * 16, 768, 3072, 1, ACT_GELU, "b"), (128 * 20, 768, 768, 0, ACT_NONE, "br")]):
            row(id=f"linear16_nows{i}_p{p}", entries=("mi355_linear16_fwd",), opts=dict(gemm_splitk=0), prec=p, tol=TOL[p],
                make=lambda seed, a=(M, N, K, inputs, p): _gemm_inputs(seed, *a), ref=lambda d, act=act: _gemm_ref(d, act),
                run=lambda F, d, out16=out16, act=act, p=p: direct(F, d, out16, act, p))
    # ragged in every tiled dimension: partial last row tile, partial column tile (N % 8 != 0 as well), several K steps
    for p in (1, 2):
        for i, (M, N, K) in enumerate([(130, 132, 192), (257, 516, 320), (1, 4, 64), (300, 2304, 768), (197 * 3, 772, 1024)]):
            _linear16_row(f"gemm_ragged{i}_out32_p{p}", M, N, K, 0, ACT_GELU, "bgr", {}, p)
            _linear16_row(f"gemm_ragged{i}_out16_p{p}", M, N, K, 1, ACT_NONE, "b", {}, p)
            _linear16_row(f"gemm_ragged{i}_v7_p{p}", M, N, K, 0, ACT_NONE, "br", {"gemm_variant": 7}, p)
        _linear16_row(f"gemm_pa_tail_off_p{p}", 128 * 70, 512, 1024, 0, ACT_NONE, "br", {"gemm_pa_tail": 0}, p)
        _linear16_row(f"gemm_pa_unblocked_p{p}", 128 * 20, 2048, 640, 0, ACT_NONE, "br", {"gemm_pa_block": 0}, p)
        _linear16_row(f"gemm_small_round_p{p}", 128 * 20, 2048, 640, 0, ACT_NONE, "br", {"gemm_pa": 0}, p)
        # split-K of the last partial round (K >= 1536): the one row whose bits may depend on the launch
        _linear16_row(f"gemm_splitk_p{p}", 197 * 16, 768, 3072, 1, ACT_GELU, "b", {"gemm_pa16": 0, "gemm_w4": 0}, p, bits=False)
        _linear16_row(f"gemm_splitk_fp32_p{p}", 197 * 16, 768, 3072, 0, ACT_NONE, "br", {"gemm_pa": 0}, p, bits=False)


# ---- the fp32-input engine, LayerNorm, casts -----------------------------------------------------------------------------------
def _dense_rows():
    from test_ops_gpu import LINEAR_SHAPES

    def lin_make(M, N, K, full):
        def make(seed):
            g = _gen(seed)
            d = dict(x=_rn(g, M, K), w=_rn(g, N, K) / math.sqrt(K), b=_rn(g, N))
            d["gamma"] = torch.rand(N, generator=g) + 0.5 if full else None
            d["resid"] = _rn(g, M, N) if full else None
            return d
        return make

    def lin_ref(act):
        def ref(d):
            y = d["x"].double() @ d["w"].double().t() + d["b"].double()
            y = gelu64(y) if act else y
            if d["gamma"] is not None:
                y = y * d["gamma"].double() + d["resid"].double()
            return y
        return ref
    for M, N, K in LINEAR_SHAPES:
        for p in (0, 1, 2):
            full = (M + N) % 2 == 0
            row(id=f"linear_{M}x{N}x{K}_p{p}", entries=("mi355_linear_fwd",), prec=p, tol=TOL[p], make=lin_make(M, N, K, full),
                run=lambda F, d, p=p, full=full: F.linear(d["x"], d["w"], d["b"], act=ACT_GELU if full else ACT_NONE, gamma=d["gamma"],
                                                            resid=d["resid"], precision=p), ref=lin_ref(full))
    for p in (0, 1):
        row(id=f"linear_head_engine_p{p}", entries=("mi355_linear_fwd",), opts=dict(gemm_small=0), prec=p, tol=TOL[p],
            make=lin_make(64, 1000, 768, False), run=lambda F, d, p=p: F.linear(d["x"], d["w"], d["b"], precision=p), ref=lin_ref(False))
        row(id=f"linear_head_small_p{p}", entries=("mi355_linear_fwd",), opts=dict(gemm_small=1), prec=p, tol=TOL[p],
            make=lin_make(256, 1000, 768, False), run=lambda F, d, p=p: F.linear(d["x"], d["w"], d["b"], precision=p), ref=lin_ref(False))
    for rows_, cols in ((197 * 3, 768), (37, 100), (1, 4), (130, 2048)):
        def make(seed, rows_=rows_, cols=cols):
            g = _gen(seed)
            return dict(x=_rn(g, rows_, cols) + 0.3, w=torch.rand(cols, generator=g) + 0.5, b=_rn(g, cols, s=0.2))
        row(id=f"layernorm_{rows_}x{cols}", entries=("mi355_layernorm_fwd",), tol=TOL[0], make=make,
            run=lambda F, d: F.layernorm(d["x"], d["w"], d["b"], 1e-6), ref=lambda d: ln64(d["x"], d["w"], d["b"], 1e-6))
        if cols % 4 == 0:
            for p in (1, 2):
                row(id=f"layernorm16_{rows_}x{cols}_p{p}", entries=("mi355_layernorm16_fwd",), prec=p, tol=TOL[p], make=make,
                    run=lambda F, d, p=p: F.layernorm16(d["x"], d["w"], d["b"], 1e-6, precision=p), ref=lambda d: ln64(d["x"], d["w"], d["b"], 1e-6))
    for p in (1, 2):
        for n in ((1001, 7), (4,), (3, 197, 768)):
            row(id=f"cast16_{'x'.join(map(str, n))}_p{p}", entries=("mi355_cast16_fwd",), prec=p, tol=TOL[p],
                make=lambda seed, n=n: dict(x=_rn(_gen(seed), *n)), run=lambda F, d, p=p: F.cast16(d["x"], p), ref=lambda d: d["x"].double())
    for n in ((1 << 20) + 16, 16):
        row(id=f"stream_copy_{n}", entries=("mi355_stream_copy",), tol=0.0, make=lambda seed, n=n: dict(x=_rn(_gen(seed), n // 4)),
            run=lambda F, d: F.stream_copy(d["x"], F.torch.empty_like(d["x"])), ref=lambda d: d["x"].double())
    for B, N, C, skip in ((3, 197, 768, 1), (2, 49, 100, 0), (5, 1, 4, 0)):
        row(id=f"token_mean_{B}x{N}x{C}", entries=("mi355_token_mean_fwd",), tol=TOL[0], make=lambda seed, s=(B, N, C): dict(x=_rn(_gen(seed), *s)),
            run=lambda F, d, skip=skip: F.token_mean(d["x"], skip), ref=lambda d, skip=skip: d["x"].double()[:, skip:].mean(1))
    for B, N, T, C in ((3, 196, 256, 100), (2, 49, 48, 96), (1, 64, 33, 4)):
        for p in (0, 1, 2):
            def make(seed, s=(B, N, T, C)):
                g = _gen(seed)
                B_, N_, T_, C_ = s
                return dict(w=_rn(g, T_, N_) / math.sqrt(N_), x=_rn(g, B_, N_, C_), b=_rn(g, T_), r=_rn(g, B_, T_, C_))
            row(id=f"token_mix_{B}x{N}x{T}x{C}_p{p}", entries=("mi355_token_mix_fwd",), prec=p, tol=TOL[p], make=make,
                run=lambda F, d, p=p: F.token_mix(d["w"], d["x"], d["b"], act=ACT_GELU, resid=d["r"], precision=p),
                ref=lambda d: d["r"].double() + gelu64(d["w"].double() @ d["x"].double() + d["b"].double()[None, :, None]))


# ---- attention cores ---------------------------------------------------------------------------------------------------------------
def _heads(t, h):
    B, N, C = t.shape
    return t.reshape(B, N, h, C // h).transpose(1, 2)


def _qkv_ref(qkv, h, scale):
    B, N, C3 = qkv.shape
    q, k, v = qkv.double().reshape(B, N, 3, C3 // 3).unbind(2)
    return sdpa64(_heads(q, h), _heads(k, h), _heads(v, h), scale).transpose(1, 2).reshape(B, N, C3 // 3)


def _attention_rows():
    from test_ops_gpu import GENERAL
    SD = [(2, 197, 3, 64), (3, 50, 4, 32), (1, 224, 2, 64), (5, 1, 1, 32), (2, 208, 12, 64)]        # (B, N, heads, d): 13 query tiles at 197 / 208
    for B, N, h, d in SD:
        mk = lambda seed, s=(B, N, 3 * h * d): dict(qkv=_rn(_gen(seed), *s))
        for p in (0, 1, 2):
            row(id=f"sdpa_{B}x{N}x{h}x{d}_p{p}", entries=("mi355_sdpa_fwd",), prec=p, tol=TOL[p], make=mk,
                run=lambda F, dd, h=h, d=d, p=p: F.sdpa(dd["qkv"], h, d ** -0.5, precision=p), ref=lambda dd, h=h, d=d: _qkv_ref(dd["qkv"], h, d ** -0.5))
        for p in (1, 2):
            mk16 = lambda seed, s=(B, N, 3 * h * d), p=p: dict(qkv=_rn(_gen(seed), *s).to(dt16(p)))
            for nw in (8, 7):
                if nw == 7 and not 193 <= N <= 208:
                    continue
                row(id=f"sdpa16_{B}x{N}x{h}x{d}_nw{nw}_p{p}", entries=("mi355_sdpa16_fwd",), opts=dict(attn_nw=nw), prec=p, tol=TOL[p], make=mk16,
                    run=lambda F, dd, h=h, d=d, p=p: F.sdpa16(dd["qkv"], h, d ** -0.5, precision=p),
                    ref=lambda dd, h=h, d=d: _qkv_ref(dd["qkv"], h, d ** -0.5))
            for qr in sorted({1, min(N, 17)}):
                row(id=f"sdpa16_rows{qr}_{B}x{N}x{h}x{d}_p{p}", entries=("mi355_sdpa16_rows_fwd",), prec=p, tol=TOL[p], make=mk16,
                    run=lambda F, dd, h=h, d=d, p=p, qr=qr: F.sdpa16_rows(dd["qkv"], h, d ** -0.5, qr, precision=p),
                    ref=lambda dd, h=h, d=d, qr=qr: _qkv_ref(dd["qkv"], h, d ** -0.5)[:, :qr])
    for B, Nq, Nkv, h, d, has_bias in GENERAL:
        def make(seed, s=(B, Nq, Nkv, h, d, has_bias)):
            B_, Nq_, Nkv_, h_, d_, hb = s
            g = _gen(seed)
            return dict(q=_rn(g, B_, Nq_, h_ * d_), kv=_rn(g, B_, Nkv_, 2 * h_ * d_), bias=_rn(g, h_, Nq_, Nkv_) if hb else None)

        def ref(dd, h=h, d=d):
            C = h * d
            q, k, v = dd["q"].double(), dd["kv"].double()[..., :C], dd["kv"].double()[..., C:]
            b = None if dd["bias"] is None else dd["bias"].double()[None]
            return sdpa64(_heads(q, h), _heads(k, h), _heads(v, h), d ** -0.5, b).transpose(1, 2).reshape(q.shape)
        for p in (0, 1, 2):
            row(id=f"sdpa_general_{B}x{Nq}x{Nkv}x{h}x{d}_p{p}", entries=("mi355_sdpa_general_fwd",), prec=p, tol=TOL[p], make=make, ref=ref,
                run=lambda F, dd, h=h, d=d, p=p: F.sdpa_general(dd["q"], dd["kv"][..., :h * d], dd["kv"][..., h * d:], h, d ** -0.5, dd["bias"], precision=p))
        for p in (1, 2):
            def make16(seed, make=make, p=p):
                dd = make(seed)
                return dict(dd, q=dd["q"].to(dt16(p)), kv=dd["kv"].to(dt16(p)))
            row(id=f"sdpa_general16_{B}x{Nq}x{Nkv}x{h}x{d}_p{p}", entries=("mi355_sdpa_general_fwd",), prec=p, tol=TOL[p], make=make16, ref=ref,
                run=lambda F, dd, h=h, d=d, p=p: F.sdpa_general(dd["q"], dd["kv"][..., :h * d], dd["kv"][..., h * d:], h, d ** -0.5, dd["bias"], precision=p))
    # precision 3 of the host mirror: the split qkv projection and its attention core
    for M_, C, K, h in (((3, 197), 128, 192, 2), ((2, 50), 64, 64, 2), ((1, 224), 768, 768, 12)):
        def make(seed, s=(M_, C, K)):
            (B_, N_), C_, K_ = s
            g = _gen(seed)
            w = _rn(g, 3 * C_, K_) / math.sqrt(K_)
            hi = w[:2 * C_].to(torch.bfloat16)
            lo = (w[:2 * C_] - hi.float()).to(torch.bfloat16)
            return dict(x=_rn(g, B_, N_, K_), w=w, hi=hi, lo=lo, v16=w[2 * C_:].to(torch.float16), b=_rn(g, 3 * C_, s=0.1))

        def run(F, dd, h=h, C=C):
            qkv5 = F.qkv_split16(dd["x"], dd["hi"], dd["lo"], dd["v16"], dd["b"])
            return F.sdpa16_split(qkv5, h, (C // h) ** -0.5), qkv5

        def ref(dd, h=h, C=C):
            w = torch.cat([dd["hi"].double() + dd["lo"].double(), dd["v16"].double()])
            qkv = dd["x"].double() @ w.t() + dd["b"].double()
            return _qkv_ref(qkv, h, (C // h) ** -0.5), None
        row(id=f"logit_mode_{C}x{K}", entries=("mi355_qkv_split16_fwd", "mi355_sdpa16_split_fwd"), prec=1, tol=TOL[1], make=make, run=run, ref=ref)
    # the last encoder block of a token-pooled ViT: only the pooled token's rows (mi355_vit_tail_fwd, its workspace embeds linear16's)
    for B, N, C, h in ((3, 65, 256, 4), (4, 197, 768, 12), (5, 17, 128, 4), (1, 224, 64, 2)):
        def make(seed, s=(B, N, C, h)):
            from mi355attn.modules import TransformerEncoder
            from route_cases import prep_nontrivial
            B_, N_, C_, h_ = s
            torch.manual_seed(seed)
            return dict(m=prep_nontrivial(TransformerEncoder(C_, h_, qkv_bias=True).eval()), x=torch.randn(B_, N_, C_))

        def run(F, dd, p):
            m = dd["m"]
            at, mlp = m.attn, m.mlp
            return F.vit_tail16(dd["x"], m.layernorm1, F.weight16(at.qkv.weight, p), at.qkv.bias, F.weight16(at.proj.weight, p), at.proj.bias,
                                m.layernorm2, F.weight16(mlp.fc1.weight, p), mlp.fc1.bias, F.weight16(mlp.fc2.weight, p), mlp.fc2.bias,
                                at.num_heads, at.scale, precision=p)
        for p in (1, 2):
            row(id=f"vit_tail_{B}x{N}x{C}_p{p}", entries=("mi355_vit_tail_fwd",), opts=dict(gemm_splitk=0), prec=p, tol=TOL[p], make=make, module=True,
                run=lambda F, dd, p=p, run=run: run(F, dd, p), ref=lambda dd, h=h: O.vit_encoder_forward(dd["x"], dd["m"].state_dict(), h, torch.float64)[:, 0])
    # XCA: fp32 core (any head width), 16-bit core with and without the transposed-LDS kernel
    for B, N, h, d in ((2, 196, 8, 48), (3, 63, 2, 32), (1, 225, 4, 64)):
        def make(seed, s=(B, N, h, d)):
            B_, N_, h_, d_ = s
            g = _gen(seed)
            return dict(qkv=_rn(g, B_, N_, 3 * h_ * d_), t=torch.rand(h_, generator=g) + 0.5)

        def ref(dd, h=h, d=d):
            B_, N_, _ = dd["qkv"].shape
            q, k, v = dd["qkv"].double().reshape(B_, N_, 3, h, d).permute(2, 0, 3, 4, 1)
            q, k = torch.nn.functional.normalize(q, dim=-1), torch.nn.functional.normalize(k, dim=-1)
            a = torch.softmax(q @ k.transpose(-1, -2) * dd["t"].double()[None, :, None, None], dim=-1)
            return (a @ v).permute(0, 3, 1, 2).reshape(B_, N_, h * d)
        for p in (0, 1, 2):
            row(id=f"xca_{B}x{N}x{h}x{d}_p{p}", entries=("mi355_xca_fwd",), prec=p, tol=TOL[p], make=make, ref=ref,
                run=lambda F, dd, h=h, p=p: F.xca_core(dd["qkv"], dd["t"], h, precision=p))
        for p in (1, 2):
            for tr in (1, 0):
                row(id=f"xca16_{B}x{N}x{h}x{d}_tr{tr}_p{p}", entries=("mi355_xca16_fwd",), opts=dict(xca_tr=tr), prec=p, tol=TOL[p], ref=ref,
                    make=lambda seed, make=make, p=p: (lambda dd: dict(dd, qkv=dd["qkv"].to(dt16(p))))(make(seed)),
                    run=lambda F, dd, h=h, p=p: F.xca_core(dd["qkv"], dd["t"], h, precision=p, out16=True))
            row(id=f"xca16_from32_{B}x{N}x{h}x{d}_p{p}", entries=("mi355_xca16_fwd",), prec=p, tol=TOL[p], make=make, ref=ref,
                run=lambda F, dd, h=h, p=p: F.xca_core(dd["qkv"], dd["t"], h, precision=p, out16=True))


# ---- convolutions on tokens, LPI, patch embedding ------------------------------------------------------------------------------------
def _conv_rows():
    from test_ops_gpu import CONVS
    for i, (B, Cin, H, W, Cout, k, stride, pad) in enumerate(CONVS):
        def make(seed, s=(B, Cin, H, W, Cout, k)):
            B_, Cin_, H_, W_, Cout_, k_ = s
            g = _gen(seed)
            return dict(x=_rn(g, B_, Cin_, H_, W_), w=_rn(g, Cout_, Cin_, k_, k_) / math.sqrt(Cin_ * k_ * k_), b=_rn(g, Cout_, s=0.1))

        def ref(dd, stride=stride, pad=pad):
            y = torch.nn.functional.conv2d(dd["x"].double(), dd["w"].double(), dd["b"].double(), stride=stride, padding=pad)
            return y.flatten(2).transpose(1, 2)
        for p in (0, 1, 2):
            for direct in (1, 0):
                if direct == 0 and not (Cin <= 4 and Cout <= 64):
                    continue
                row(id=f"conv{i}_nchw_direct{direct}_p{p}", entries=("mi355_conv2d_tokens_fwd",), opts=dict(stem_direct=direct), prec=p, tol=TOL[p],
                    make=make, ref=ref,
                    run=lambda F, dd, k=k, stride=stride, pad=pad, p=p: F.conv2d_tokens(dd["x"], dd["w"], dd["b"], k, stride, pad, 0, precision=p)[0])
            if Cin % 4:                                     # token-major input: the header asks for Cin % 4 == 0
                continue
            row(id=f"conv{i}_tokens_p{p}", entries=("mi355_conv2d_tokens_fwd",), prec=p, tol=TOL[p], make=make, ref=ref,
                run=lambda F, dd, k=k, stride=stride, pad=pad, p=p, hw=(H, W): F.conv2d_tokens(
                    dd["x"].flatten(2).transpose(1, 2).contiguous(), dd["w"], dd["b"], k, stride, pad, 1, hw=hw, precision=p, act=ACT_NONE)[0])
    # LPI: the 14 x 14 patch kernel and the general kernel, with and without the LayerNorm in front
    for B, H, W, C in ((2, 14, 14, 128), (3, 7, 9, 64), (1, 5, 3, 4), (2, 14, 14, 384)):
        def make(seed, s=(B, H, W, C)):
            B_, H_, W_, C_ = s
            g = _gen(seed)
            torch.manual_seed(seed)
            ln = torch.nn.LayerNorm(C_, eps=1e-6)
            with torch.no_grad():
                ln.weight.copy_(0.5 + torch.rand(C_))
                ln.bias.copy_(0.2 * torch.randn(C_))
            return dict(x=_rn(g, B_, H_ * W_, C_), w1=_rn(g, C_, 3, 3, s=0.3), b1=_rn(g, C_, s=0.1), bw=torch.rand(C_, generator=g) + 0.5,
                        bb=_rn(g, C_, s=0.1), bm=_rn(g, C_, s=0.2), bv=torch.rand(C_, generator=g) + 0.5, w2=_rn(g, C_, 3, 3, s=0.3),
                        b2=_rn(g, C_, s=0.1), gamma=torch.rand(C_, generator=g) + 0.5, ln=ln)

        def ref(dd, use_ln, H=H, W=W):
            x = dd["x"].double()
            z = ln64(x, dd["ln"].weight, dd["ln"].bias, dd["ln"].eps) if use_ln else x
            p_ = {"conv1.weight": dd["w1"].unsqueeze(1), "conv1.bias": dd["b1"], "bn.weight": dd["bw"], "bn.bias": dd["bb"], "bn.running_mean": dd["bm"],
                  "bn.running_var": dd["bv"], "conv2.weight": dd["w2"].unsqueeze(1), "conv2.bias": dd["b2"]}
            return x + dd["gamma"].double() * O.lpi_forward(z, p_, H, W, torch.float64)

        def run(F, dd, use_ln, H=H, W=W):
            return F.lpi(dd["x"], dd["w1"], dd["b1"], dd["bw"], dd["bb"], dd["bm"], dd["bv"], 1e-5, dd["w2"], dd["b2"], H, W, gamma=dd["gamma"],
                         resid=dd["x"], ln=dd["ln"] if use_ln else None)
        for patch in (1, 0):
            if patch == 0 and (H, W) != (14, 14):
                continue
            row(id=f"lpi_{B}x{H}x{W}x{C}_patch{patch}", entries=("mi355_lpi_fwd",), opts=dict(lpi_patch=patch), tol=TOL[0], make=make,
                run=lambda F, dd, run=run: run(F, dd, False), ref=lambda dd, ref=ref: ref(dd, False))
            row(id=f"ln_lpi_{B}x{H}x{W}x{C}_patch{patch}", entries=("mi355_ln_lpi_fwd",), opts=dict(lpi_patch=patch), tol=TOL[0], make=make,
                run=lambda F, dd, run=run: run(F, dd, True), ref=lambda dd, ref=ref: ref(dd, True))
    # patch embedding: fp32 engine, the 16-bit engine with its im2col workspace, plain patches (Mixer)
    for B, HW, ps, E, vit in ((2, 224, 16, 768, True), (3, 32, 8, 100, True), (2, 224, 16, 512, False), (128, 224, 16, 768, True)):
        def make(seed, s=(B, HW, ps, E, vit)):
            B_, HW_, ps_, E_, vit_ = s
            g = _gen(seed)
            P = (HW_ // ps_) ** 2
            return dict(img=_rn(g, B_, 3, HW_, HW_), wp=_rn(g, E_, 3, ps_, ps_, s=0.02), bp=_rn(g, E_, s=0.1),
                        cls=_rn(g, 1, 1, E_) if vit_ else None, pos=_rn(g, 1, P + 1, E_) if vit_ else None)

        def ref(dd, ps=ps):
            t = torch.nn.functional.conv2d(dd["img"].double(), dd["wp"].double(), dd["bp"].double(), stride=ps).flatten(2).transpose(1, 2)
            if dd["cls"] is None:
                return t
            t = torch.cat([t, dd["cls"].double().expand(t.shape[0], -1, -1)], dim=1)
            return t + dd["pos"].double()
        for p in (0, 1, 2):
            if B == 128 and p == 0:
                continue
            ws = vit and p != 0 and E % 64 == 0               # mi355_patch_embed_workspace_bytes != 0: the im2col + 16-bit GEMM path
            row(id=f"patch_embed_{B}x{HW}x{ps}x{E}_p{p}", entries=("mi355_patch_embed_ws_fwd" if ws else "mi355_patch_embed_fwd",), prec=p,
                tol=TOL[p], make=make, ref=ref, run=lambda F, dd, ps=ps, p=p: F.patch_embed(dd["img"], dd["wp"], dd["bp"], dd["cls"], dd["pos"], ps, precision=p))


# ---- 16-bit channel gates (chan_io16.hip) and the helper classes of the axis modules --------------------------------------------
def _io16_rows():
    from test_io16_gpu import GENERAL as IO_GENERAL
    from test_io16_gpu import SMALL
    for shape in [SMALL, (4, 256, 56, 56)] + list(IO_GENERAL):
        B, C, H, W = shape
        red = 16 if C >= 32 else 4
        ks = 7 if min(H, W) >= 3 else 3
        k = 3
        for dt, p in ((torch.float16, 1), (torch.bfloat16, 2)):
            def make(seed, shape=shape, dt=dt, C=C, red=red, ks=ks, k=k):
                g = _gen(seed)
                return dict(x=_rn(g, *shape).to(dt), w1=_rn(g, C // red, C) / math.sqrt(C), w2=_rn(g, C, C // red) / math.sqrt(C // red),
                            wc=_rn(g, 1, 2, ks, ks, s=0.2), we=_rn(g, k, s=0.5))
            sid = "x".join(map(str, shape))
            for single in (1, 0):
                row(id=f"se16_{sid}_s{single}_p{p}", entries=("mi355_se16_fwd",), opts=dict(se_single=single), prec=p, tol=TOL[p], make=make,
                    run=lambda F, d: F.se_forward(d["x"], d["w1"], d["w2"]), ref=lambda d: O.se_forward(d["x"].double(), d["w1"], d["w2"], torch.float64))
                row(id=f"eca16_{sid}_s{single}_p{p}", entries=("mi355_eca16_fwd",), opts=dict(eca_single=single), prec=p, tol=TOL[p], make=make,
                    run=lambda F, d: F.eca_forward(d["x"], d["we"]), ref=lambda d: O.eca_forward(d["x"].double(), d["we"].reshape(1, 1, -1), torch.float64))
                row(id=f"cbam16_{sid}_s{single}_p{p}", entries=("mi355_cbam16_fwd",), opts=dict(cbam_single=single), prec=p, tol=TOL[p], make=make,
                    run=lambda F, d: F.cbam_forward(d["x"], d["w1"], d["w2"], d["wc"]),
                    ref=lambda d: O.cbam_forward(d["x"].double(), d["w1"], d["w2"], d["wc"], torch.float64))
            row(id=f"se16_{sid}_occ2_p{p}", entries=("mi355_se16_fwd",), opts=dict(io16_occ=2), prec=p, tol=TOL[p], make=make,
                run=lambda F, d: F.se_forward(d["x"], d["w1"], d["w2"]), ref=lambda d: O.se_forward(d["x"].double(), d["w1"], d["w2"], torch.float64))
            for stage, fn in ((1, lambda d: O.cbam_channel_forward(d["x"].double(), d["w1"], d["w2"], torch.float64)),
                              (2, lambda d: O.cbam_spatial_forward(d["x"].double(), d["wc"], torch.float64))):
                row(id=f"cbam16_{sid}_stage{stage}_p{p}", entries=("mi355_cbam16_fwd",), prec=p, tol=TOL[p], make=make, ref=fn,
                    run=lambda F, d, stage=stage: F.cbam_forward(d["x"], d["w1"], d["w2"], d["wc"], stage=stage))
    # fp32 CBAM stages 1 and 2 (their own workspaces), ragged shapes of the fp32 gates
    for shape in ((2, 48, 7, 9), (2, 100, 10, 10), (2, 64, 32, 32)):
        B, C, H, W = shape
        def make(seed, shape=shape, C=C):
            g = _gen(seed)
            return dict(x=_rn(g, *shape), w1=_rn(g, C // 4, C) / math.sqrt(C), w2=_rn(g, C, C // 4) / math.sqrt(C // 4), wc=_rn(g, 1, 2, 7, 7, s=0.2),
                        we=_rn(g, 5, s=0.5), aff=torch.tensor([0.8, 0.1]))
        sid = "x".join(map(str, shape))
        row(id=f"cbam_{sid}_stage1", entries=("mi355_cbam_fwd",), tol=VEC, make=make, run=lambda F, d: F.cbam_forward(d["x"], d["w1"], d["w2"], stage=1),
            ref=lambda d: O.cbam_channel_forward(d["x"].double(), d["w1"], d["w2"], torch.float64))
        row(id=f"cbam_{sid}_stage2", entries=("mi355_cbam_fwd",), tol=VEC, make=make, run=lambda F, d: F.cbam_forward(d["x"], wconv=d["wc"], stage=2),
            ref=lambda d: O.cbam_spatial_forward(d["x"].double(), d["wc"], torch.float64))
        for single in (1, 0):
            row(id=f"cbam_{sid}_s{single}", entries=("mi355_cbam_fwd",), opts=dict(cbam_single=single), tol=VEC, make=make,
                run=lambda F, d: F.cbam_forward(d["x"], d["w1"], d["w2"], d["wc"]), ref=lambda d: O.cbam_forward(d["x"].double(), d["w1"], d["w2"], d["wc"], torch.float64))
            row(id=f"se_{sid}_s{single}", entries=("mi355_se_fwd",), opts=dict(se_single=single), tol=VEC, make=make,
                run=lambda F, d: F.se_forward(d["x"], d["w1"], d["w2"]), ref=lambda d: O.se_forward(d["x"].double(), d["w1"], d["w2"], torch.float64))
            row(id=f"eca_{sid}_s{single}", entries=("mi355_eca_fwd",), opts=dict(eca_single=single), tol=VEC, make=make,
                run=lambda F, d: F.eca_forward(d["x"], d["we"]), ref=lambda d: O.eca_forward(d["x"].double(), d["we"].reshape(1, 1, -1), torch.float64))
        row(id=f"zpool_{sid}", entries=("mi355_zpool_fwd",), tol=VEC, make=make, run=lambda F, d: F.zpool(d["x"]),
            ref=lambda d: torch.stack([d["x"].double().mean(1), d["x"].double().max(1).values], dim=1))

        def gate_ref(d):
            x = d["x"].double()
            z = torch.stack([x.mean(1), x.max(1).values], dim=1)
            s = torch.nn.functional.conv2d(z, d["wc"].double(), padding=3) * 0.8 + 0.1
            return x * torch.sigmoid(torch.relu(s))
        row(id=f"attention_gate_{sid}", entries=("mi355_attention_gate_fwd",), tol=CHAIN, make=make, ref=gate_ref,
            run=lambda F, d: F.attention_gate(d["x"], d["wc"], d["aff"], 7))


def _helper_rows():
    """ChannelGate / SpatialGate of BAM on their own (mi355_bam_gates_fwd) through the helper modules of the drop-in package."""
    def make(seed):
        from mi355attn.modules import BAM
        torch.manual_seed(seed)
        m = BAM(80).eval()
        with torch.no_grad():
            for p_ in m.parameters():
                p_.add_(0.2 * torch.randn_like(p_))
            for mod in m.modules():
                if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                    mod.running_mean.normal_(0, 0.2)
                    mod.running_var.uniform_(0.5, 1.5)
        return dict(m=m, x=torch.randn(3, 80, 9, 11))

    def run(F, d):
        with torch.no_grad():
            return d["m"].channel_attn(d["x"]).contiguous(), d["m"].spatial_attn(d["x"]).contiguous()

    def ref(d):
        with torch.no_grad():
            return None, None, O.bam_forward(d["x"], d["m"].state_dict(), 4, torch.float64)

    def run_all(F, d):
        with torch.no_grad():
            return run(F, d) + (d["m"](d["x"]),)
    row(id="bam_gates_ragged", entries=("mi355_bam_gates_fwd", "mi355_bam_fwd"), tol=CHAIN, make=make, run=run_all, ref=ref, module=True)


# ---- entries that the module rows reach at one shape or one precision only: called through their functional wrappers ------------------
def _params_of(test_fn):
    """The case list of a parametrised test of the suite (imported, not copied)."""
    mark = next(m for m in test_fn.pytestmark if m.name == "parametrize")
    return list(mark.args[1])


def _glue_rows():
    import test_ops_gpu as T
    # the fp32-I/O LePE core over every stripe geometry the suite trusts: both idx branches, split < reso, the whole-plane window.
    # The branch attends over the channel slice [c0, c0 + dim) of a (B,L,3,2*dim) buffer and must leave the other half of `out` alone.
    for reso, idx, split, dim, heads in T.WINDOWS:
        def make(seed, s=(reso, idx, dim)):
            reso_, idx_, dim_ = s
            g = _gen(seed)
            ctot = dim_ if idx_ < 0 else 2 * dim_
            return dict(qkv=_rn(g, 2, reso_ * reso_, 3 * ctot), w=_rn(g, dim_, 1, 3, 3, s=0.3), b=_rn(g, dim_, s=0.1))

        def run(F, dd, p, s=(reso, idx, split, dim, heads)):
            reso_, idx_, split_, dim_, heads_ = s
            hsp, wsp = (reso_, reso_) if idx_ < 0 else ((reso_, split_) if idx_ == 0 else (split_, reso_))
            B, L, c3 = dd["qkv"].shape
            out = F.torch.zeros(B, L, c3 // 3, dtype=torch.float32, device=dd["qkv"].device)
            return F.cswin_lepe_attention(dd["qkv"], dd["w"], dd["b"], out, reso_, max(idx_, 0) * dim_, dim_, heads_, hsp, wsp,
                                          (dim_ // heads_) ** -0.5, precision=p)

        def ref(dd, s=(reso, idx, split, dim, heads)):
            reso_, idx_, split_, dim_, heads_ = s
            B, L, c3 = dd["qkv"].shape
            c0 = max(idx_, 0) * dim_
            qkv = dd["qkv"].reshape(B, L, 3, c3 // 3)[..., c0:c0 + dim_].permute(2, 0, 1, 3)
            out = torch.zeros(B, L, c3 // 3, dtype=torch.float64)
            out[..., c0:c0 + dim_] = O.lepe_attention_forward(qkv, dd["w"], dd["b"], reso_, idx_, split_, heads_, torch.float64)
            return out
        for p in (0, 1, 2):
            row(id=f"lepe_r{reso}_i{idx}_s{split}_c{dim}_h{heads}_p{p}", entries=("mi355_cswin_lepe_attn_fwd",), prec=p, tol=TOL[p], make=make,
                ref=ref, run=lambda F, dd, p=p, run=run: run(F, dd, p))
    # CAM: C and H*W multiples of 4 (the header's envelope), neither a multiple of a GEMM tile; one model-sized plane
    for B, C, H, W in ((2, 36, 6, 6), (3, 100, 10, 14), (1, 132, 9, 12), (2, 512, 16, 16)):
        for p in (0, 1, 2):
            row(id=f"cam_{B}x{C}x{H}x{W}_p{p}", entries=("mi355_cam_fwd",), prec=p, tol=TOL[p],
                make=lambda seed, s=(B, C, H, W): dict(x=_rn(_gen(seed), *s, s=0.5), beta=torch.tensor([0.7])),
                run=lambda F, dd, p=p: F.cam_forward(dd["x"], dd["beta"], precision=p),
                ref=lambda dd: O.cam_forward(dd["x"], {"beta": dd["beta"]}, torch.float64))
    # unscaled logits on views into fused projections (row strides 3C and 2C)
    for B, h, Nq, Nkv, d in _params_of(T.test_qk_logits) + [(2, 2, 130, 257, 20), (1, 12, 197, 197, 64)]:
        def make(seed, s=(B, h, Nq, Nkv, d)):
            B_, h_, Nq_, Nkv_, d_ = s
            g = _gen(seed)
            return dict(qkv=_rn(g, B_, Nq_, 3 * h_ * d_), kk=_rn(g, B_, Nkv_, 2 * h_ * d_))

        def ref(dd, h=h, d=d):
            C = h * d
            q = dd["qkv"][..., :C].double().reshape(dd["qkv"].shape[0], -1, h, d).permute(0, 2, 1, 3)
            k = dd["kk"][..., C:].double().reshape(dd["kk"].shape[0], -1, h, d).permute(0, 2, 1, 3)
            return q @ k.transpose(-1, -2)
        for p in (0, 1, 2):
            row(id=f"qk_logits_{B}x{h}x{Nq}x{Nkv}x{d}_p{p}", entries=("mi355_qk_logits_fwd",), prec=p, tol=TOL[p], make=make, ref=ref,
                run=lambda F, dd, h=h, d=d, p=p: F.qk_logits(dd["qkv"][..., :h * d], dd["kk"][..., h * d:], h, precision=p))
    # P2T's pooled pyramid: odd grids, C that is no multiple of 4, several levels written into one token sequence
    pyramids = [(B, H, W, C, [(oh, ow), (max(oh // 2, 1), max(ow // 2, 1)), (1, 1)]) for B, H, W, C, oh, ow in
                _params_of(T.test_adaptive_pool_and_dwconv_residual_on_tokens)]
    for B, H, W, C, sizes in pyramids + [(2, 7, 9, 6, [(3, 4), (2, 5), (7, 9)]), (3, 13, 11, 101, [(5, 3), (4, 4)])]:
        def make(seed, s=(B, H, W, C), n=len(sizes)):
            B_, H_, W_, C_ = s
            torch.manual_seed(seed)
            convs = torch.nn.ModuleList([torch.nn.Conv2d(C_, C_, 3, 1, 1, groups=C_) for _ in range(n)]).eval()
            return dict(x=torch.randn(B_, H_ * W_, C_), convs=convs)

        def ref(dd, s=(B, H, W, C), sizes=sizes):
            B_, H_, W_, C_ = s
            grid = dd["x"].double().permute(0, 2, 1).reshape(B_, C_, H_, W_)
            levels = []
            for size, conv in zip(sizes, dd["convs"]):
                pool = torch.nn.functional.adaptive_avg_pool2d(grid, size)
                pool = pool + torch.nn.functional.conv2d(pool, conv.weight.double(), conv.bias.double(), padding=1, groups=C_)
                levels.append(pool.reshape(B_, C_, -1))
            return torch.cat(levels, dim=2).permute(0, 2, 1)
        row(id=f"pyramid_{B}x{H}x{W}x{C}_{'_'.join(f'{a}x{b}' for a, b in sizes)}", tol=VEC, make=make, ref=ref,
            entries=("mi355_adaptive_pool_tokens_fwd", "mi355_dwconv3x3_tokens_residual_fwd"),
            run=lambda F, dd, H=H, W=W, sizes=sizes: F.pooled_pyramid_tokens(dd["x"], H, W, sizes, list(dd["convs"])))
    # bicubic resize of the position table: rectangular targets, down- and up-scaling, a width that is no multiple of 4
    for n0, E, patch, H, W in ((5, 100, 4, 28, 12), (3, 6, 2, 10, 14), (7, 33, 8, 24, 104), (14, 192, 16, 352, 224)):
        row(id=f"bicubic_{n0}x{n0}x{E}_to_{H // patch}x{W // patch}", entries=("mi355_bicubic_rows_fwd", "mi355_axpby_fwd"), tol=VEC,
            make=lambda seed, s=(n0, E): dict(pe=_rn(_gen(seed), 1, 1 + s[0] * s[0], s[1])),
            run=lambda F, dd, a=(patch, H, W): F.vit_pos_table(dd["pe"], *a),
            ref=lambda dd, a=(patch, H, W): O.vit_position_rows(dd["pe"], *a, torch.float64)[0])


_built = False


def build():
    global _built
    if not _built:
        _built = True
        _case_rows()
        _route_rows()
        _gemm_rows()
        _dense_rows()
        _attention_rows()
        _conv_rows()
        _io16_rows()
        _helper_rows()
        _glue_rows()
    return ROWS


build()
BY_ID = {r["id"]: r for r in ROWS}
