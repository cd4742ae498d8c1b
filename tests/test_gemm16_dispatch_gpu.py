"""Which kernels the 16-bit GEMM dispatch (gemm16.hip linear16_dispatch) runs: one row per branch of its policy.

Each row drives a public entry (F.linear16, F.cast_linear16, F.ln_linear16, F.linear16_stats, F.linear16_ln16, F.patch_embed, or the C
entry itself for a refusal) at one shape, with the options of the row set, and compares the kernel tally of the call (mi355attn.kernel_trace,
as a multiset: the tally aggregates tags) with the launches recorded for it.  The tags carry M / N / K, so a row also pins the row counts
of a split launch.  "{p}" in a tag stands for the precision's operand format (f16 / bf16).  A refusal row gives the full error text.

The CU count enters the choice (tile counts against one round of workgroups), so the module runs only on the 256-CU MI355X the table
was recorded on.
"""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_GELU = 0, 1

# (id, entry, (M, N, K), out16, act, inputs, options, expected)
#   inputs: "b" bias, "g" gamma, "r" residual; entry "patch_embed" reads M as the batch of 224 x 224 images (ViT-B/16: M = 197 B rows)
#   expected: {tag: launches}, or ("raises", error text) for a refusal
ROWS = [
    # ---- defaults: the model shapes the dispatch comments name ----------------------------------------------------------------------------
    ("vit_qkv", "linear16", (7424, 2304, 768), 1, ACT_NONE, "b", {}, {"gemm16_w4_kernel<{p},out16> M=7424 N=2304 K=768": 1}),
    ("vit_fc1", "linear16", (5632, 3072, 768), 1, ACT_GELU, "b", {}, {"gemm16_pa_kernel<{p},out16> M=5632 N=3072 K=768 gelu": 1}),
    ("vit_proj", "linear16", (5504, 768, 768), 0, ACT_NONE, "br", {}, {"gemm16_pa_kernel<{p},out32> M=5504 N=768 K=768": 1}),
    ("vit_fc2", "linear16", (5504, 768, 3072), 0, ACT_NONE, "br", {}, {"gemm16_pa_kernel<{p},out32> M=5504 N=768 K=3072": 1}),
    ("mixer_fc2_tail", "linear16", (50176, 512, 2048), 0, ACT_NONE, "br", {},
     {"gemm16_pa_kernel<{p},out32> M=49152 N=512 K=2048": 1, "gemm16_kernel<tail 32x64> M=1024 N=512 K=2048": 1}),
    ("xcit_proj", "linear16", (50176, 384, 384), 0, ACT_NONE, "br", {}, {"gemm16_wreg_kernel<{p},resid> M=50176 N=384 K=384": 1}),
    ("xcit_qkv_ragged", "linear16", (12000, 1152, 384), 1, ACT_NONE, "b", {}, {"gemm16_wslab_kernel<{p},K384,4w> M=12000 N=1152": 1}),
    ("xcit_qkv_whole", "linear16", (11008, 1152, 384), 1, ACT_NONE, "b", {},
     {"gemm16_pa_kernel<{p},out16,256x128,2 pieces> M=11008 N=1152 K=384": 1}),
    ("cswin_k64_bn256", "linear16", (4096, 256, 64), 1, ACT_GELU, "b", {}, {"gemm16_ws_kernel<out16> M=4096 N=256 K=64": 1}),
    ("cswin_k64_bn128", "linear16", (4096, 192, 64), 1, ACT_NONE, "b", {}, {"gemm16_ws_kernel<out16> M=4096 N=192 K=64": 1}),
    ("cswin_k64_bn64", "linear16", (4096, 64, 64), 0, ACT_NONE, "br", {}, {"gemm16_ws_kernel<out32> M=4096 N=64 K=64": 1}),
    ("cswin_k128_bn256", "linear16", (4096, 384, 128), 1, ACT_NONE, "b", {}, {"gemm16_ws_kernel<out16> M=4096 N=384 K=128": 1}),
    ("cswin_k128_bn128", "linear16", (4096, 128, 128), 0, ACT_NONE, "br", {}, {"gemm16_ws_kernel<out32> M=4096 N=128 K=128": 1}),
    ("cswin_k128_bn64", "linear16", (2048, 64, 128), 1, ACT_NONE, "b", {}, {"gemm16_ws_kernel<out16> M=2048 N=64 K=128": 1}),
    ("short_k_few_rows", "linear16", (1024, 256, 64), 1, ACT_NONE, "b", {}, {"gemm16_kernel<variant 1,out16> M=1024 N=256 K=64": 1}),
    ("tile_k192", "linear16", (8192, 1024, 192), 0, ACT_NONE, "b", {}, {"gemm16_kernel<variant 7,out32> M=8192 N=1024 K=192": 1}),
    ("tile_halved", "linear16", (4096, 1024, 256), 0, ACT_NONE, "b", {}, {"gemm16_kernel<variant 1,out32> M=4096 N=1024 K=256": 1}),
    ("tile_narrow", "linear16", (4096, 64, 256), 0, ACT_NONE, "b", {}, {"gemm16_kernel<variant 9,out32> M=4096 N=64 K=256": 1}),
    ("p8_fp32", "linear16", (16384, 1024, 256), 0, ACT_NONE, "b", {}, {"gemm16_p8_kernel<{p},out32> M=16384 N=1024 K=256": 1}),
    # inputs that a kernel's own checks refuse, where the dispatch tests only its policy before trying it
    ("out16_gamma", "linear16", (12000, 1152, 384), 1, ACT_NONE, "bg", {}, {"gemm16_kernel<variant 7,out16> M=12000 N=1152 K=384": 1}),
    ("out16_resid", "linear16", (4000, 256, 256), 1, ACT_NONE, "br", {}, {"gemm16_kernel<variant 1,out16> M=4000 N=256 K=256": 1}),
    ("out16_resid_full_round", "linear16", (16384, 1024, 256), 1, ACT_NONE, "br", {},
     {"gemm16_kernel<variant 7,out16> M=16384 N=1024 K=256": 1}),
    ("out16_k192", "linear16", (8192, 1024, 192), 1, ACT_NONE, "b", {}, {"gemm16_kernel<variant 7,out16> M=8192 N=1024 K=192": 1}),
    ("n_not_8", "linear16", (16384, 1020, 256), 0, ACT_NONE, "b", {}, {"gemm16_kernel<variant 7,out32> M=16384 N=1020 K=256": 1}),
    # ---- options ------------------------------------------------------------------------------------------------------------------------
    ("w4_off", "linear16", (7424, 2304, 768), 1, ACT_NONE, "b", {"gemm_w4": 0}, {"gemm16_p8_kernel<{p},out16> M=7424 N=2304 K=768": 1}),
    ("pa16_0", "linear16", (5632, 3072, 768), 1, ACT_GELU, "b", {"gemm_pa16": 0},
     {"gemm16_w4_kernel<{p},out16> M=5632 N=3072 K=768 gelu": 1}),
    ("pa16_2", "linear16", (7424, 2304, 768), 1, ACT_NONE, "b", {"gemm_pa16": 2}, {"gemm16_pa_kernel<{p},out16> M=7424 N=2304 K=768": 1}),
    ("pa_off_fp32", "linear16", (5504, 768, 768), 0, ACT_NONE, "br", {"gemm_pa": 0},
     {"gemm16_kernel<variant 1,out32> M=5504 N=768 K=768": 1}),
    ("pa_off_out16", "linear16", (11008, 1152, 384), 1, ACT_NONE, "b", {"gemm_pa": 0},
     {"gemm16_kernel<variant 7,out16> M=11008 N=1152 K=384": 1}),
    ("pa_tail_off", "linear16", (50176, 512, 2048), 0, ACT_NONE, "br", {"gemm_pa_tail": 0},
     {"gemm16_pa_kernel<{p},out32> M=50176 N=512 K=2048": 1}),
    ("wreg_off", "linear16", (50176, 384, 384), 0, ACT_NONE, "br", {"gemm_wreg": 0}, {"gemm16_p8_kernel<{p},out32> M=50176 N=384 K=384": 1}),
    ("wslab_off", "linear16", (12000, 1152, 384), 1, ACT_NONE, "b", {"gemm_wslab": 0},
     {"gemm16_kernel<variant 7,out16> M=12000 N=1152 K=384": 1}),
    ("wslab_2", "linear16", (11008, 1152, 384), 1, ACT_NONE, "b", {"gemm_wslab": 2}, {"gemm16_wslab_kernel<{p},K384,4w> M=11008 N=1152": 1}),
    ("wslab_2_fp32", "linear16", (50176, 384, 384), 0, ACT_NONE, "br", {"gemm_wslab": 2},
     {"gemm16_wreg_kernel<{p},resid> M=50176 N=384 K=384": 1}),
    ("wslab_2_k768", "linear16", (7424, 2304, 768), 1, ACT_NONE, "b", {"gemm_wslab": 2}, {"gemm16_w4_kernel<{p},out16> M=7424 N=2304 K=768": 1}),
    ("wst_1_qkv", "linear16", (7424, 2304, 768), 1, ACT_NONE, "b", {"gemm_wst": 1}, {"gemm16_wst_kernel<{p},out16> M=7424 N=2304 K=768": 1}),
    ("wst_1_fc1", "linear16", (5632, 3072, 768), 1, ACT_GELU, "b", {"gemm_wst": 1},
     {"gemm16_pa_kernel<{p},out16> M=5632 N=3072 K=768 gelu": 1}),
    ("wst_2_fc1", "linear16", (5632, 3072, 768), 1, ACT_GELU, "b", {"gemm_wst": 2},
     {"gemm16_wst_kernel<{p},out16> M=5632 N=3072 K=768 gelu": 1}),
    ("wst_3_qkv", "linear16", (7424, 2304, 768), 1, ACT_NONE, "b", {"gemm_wst": 3}, {"gemm16_wst_kernel<{p},out16> M=7424 N=2304 K=768": 1}),
    ("wst_3_fc1", "linear16", (5632, 3072, 768), 1, ACT_GELU, "b", {"gemm_wst": 3},
     {"gemm16_pa_kernel<{p},out16> M=5632 N=3072 K=768 gelu": 1}),
    ("wst_4_fc1", "linear16", (5632, 3072, 768), 1, ACT_GELU, "b", {"gemm_wst": 4},
     {"gemm16_wst_kernel<{p},out16> M=5632 N=3072 K=768 gelu": 1}),
    ("wst_2_k384", "linear16", (12000, 1152, 384), 1, ACT_NONE, "b", {"gemm_wst": 2}, {"gemm16_wslab_kernel<{p},K384,4w> M=12000 N=1152": 1}),
    ("wst_2_fp32", "linear16", (5504, 768, 768), 0, ACT_NONE, "br", {"gemm_wst": 2}, {"gemm16_pa_kernel<{p},out32> M=5504 N=768 K=768": 1}),
] + [
    ("variant_%d" % v, "linear16", (512, 512, 256), 0, ACT_NONE, "b", {"gemm_variant": v},
     {"gemm16_kernel<variant %d,out32> M=512 N=512 K=256" % (0 if v == 8 else v): 1}) for v in range(1, 15)
] + [
    ("variant_15", "linear16", (7424, 2304, 768), 1, ACT_NONE, "b", {"gemm_variant": 15},
     {"gemm16_p8_kernel<{p},out16> M=7424 N=2304 K=768": 1}),
    ("variant_16", "linear16", (7424, 2304, 768), 1, ACT_NONE, "b", {"gemm_variant": 16},
     {"gemm16_pa_kernel<{p},out16> M=7424 N=2304 K=768": 1}),
    ("variant_17", "linear16", (7424, 2304, 768), 1, ACT_NONE, "b", {"gemm_variant": 17},
     {"gemm16_w4_kernel<{p},out16> M=7424 N=2304 K=768": 1}),
    ("variant_15_refused", "linear16", (4096, 1024, 256), 1, ACT_NONE, "br", {"gemm_variant": 15},
     ("raises", "mi355_linear16_ws_fwd failed (code -2): mi355_linear16_fwd: persistent kernel does not take this shape")),
    ("variant_16_refused", "linear16", (4096, 1024, 256), 0, ACT_NONE, "bg", {"gemm_variant": 16},
     ("raises", "mi355_linear16_ws_fwd failed (code -2): mi355_linear16_fwd: the two-accumulator kernel does not take this shape")),
    ("variant_17_refused", "linear16", (4096, 1024, 256), 0, ACT_NONE, "b", {"gemm_variant": 17},
     ("raises", "mi355_linear16_ws_fwd failed (code -2): mi355_linear16_fwd: the one-wave-per-SIMD kernel does not take this shape")),
    # ---- entries beside the dispatch ------------------------------------------------------------------------------------------------------
    ("cast_linear16_x32", "cast_linear16", (12000, 1152, 384), 1, ACT_NONE, "b", {},
     {"gemm16_wslab_kernel<{p},K384,8w,x32> M=12000 N=1152": 1}),
    ("cast_linear16_cast", "cast_linear16", (7424, 2304, 768), 1, ACT_NONE, "b", {},
     {"cast16_kernel n=5701632": 1, "gemm16_w4_kernel<{p},out16> M=7424 N=2304 K=768": 1}),
    ("ln_linear16_k64", "ln_linear16", (4096, 256, 64), 1, ACT_GELU, "b", {}, {"gemm16_ws_kernel<ln,out16> M=4096 N=256 K=64": 1}),
    ("ln_linear16_k128", "ln_linear16", (1000, 384, 128), 0, ACT_NONE, "b", {}, {"gemm16_ws_kernel<ln,out32> M=1000 N=384 K=128": 1}),
    ("stats_256", "linear16_stats", (4096, 256, 256), 0, ACT_NONE, "br", {}, {"gemm16_wreg_kernel<{p},resid+stats> M=4096 N=256 K=256": 1}),
    ("stats_384", "linear16_stats", (4096, 384, 384), 0, ACT_NONE, "r", {}, {"gemm16_wreg_kernel<{p},resid+stats> M=4096 N=384 K=384": 1}),
    ("stats_refused_shape", "linear16_stats_c", (4096, 512, 512), 0, ACT_NONE, "br", {},
     ("raises", "mi355_linear16_stats_fwd failed (code -2): mi355_linear16_stats_fwd: built for N = K = 256 / 384, M >= 32 (got M=4096 "
                "N=512 K=512): use mi355_linear16_fwd and a statistics pass")),
    ("stats_refused_option", "linear16_stats_c", (4096, 256, 256), 0, ACT_NONE, "br", {"gemm_wreg": 0},
     ("raises", "mi355_linear16_stats_fwd failed (code -2): mi355_linear16_stats_fwd: 16-byte aligned buffers and option gemm_wreg = 1 "
                "required")),
    ("ln16_256", "linear16_ln16", (4096, 256, 256), 0, ACT_NONE, "br", {}, {"gemm16_wreg_kernel<{p},resid+ln16> M=4096 N=256 K=256": 1}),
    ("ln16_refused_shape", "linear16_ln16_c", (4096, 384, 384), 0, ACT_NONE, "br", {},
     ("raises", "mi355_linear16_ln16_fwd failed (code -2): mi355_linear16_ln16_fwd: built for N = K = 256 / 384, M >= 32 (got M=4096 "
                "N=384 K=384): use mi355_linear16_fwd + mi355_layernorm16_fwd")),
    ("ln16_refused_option", "linear16_ln16_c", (4096, 256, 256), 0, ACT_NONE, "br", {"gemm_wreg": 0},
     ("raises", "mi355_linear16_ln16_fwd failed (code -2): mi355_linear16_ln16_fwd: 16-byte aligned buffers and option gemm_wreg = 1 "
                "required")),
    ("patch_embed_tiles", "patch_embed", (2, 768, 768), 0, ACT_NONE, "", {},
     {"cast16_kernel n=589824": 1, "patch_table_kernel rows=197 E=768": 1, "im2col16_kernel B=2 224x224 ps=16": 1,
      "gemm16_kernel<variant 1,out32> M=394 N=768 K=768": 1}),
    ("patch_embed_p8", "patch_embed", (128, 768, 768), 0, ACT_NONE, "", {},
     {"cast16_kernel n=589824": 1, "patch_table_kernel rows=197 E=768": 1, "im2col16_kernel B=128 224x224 ps=16": 1,
      "gemm16_p8_kernel<{p},out32> M=25216 N=768 K=768": 1}),
]


@pytest.fixture(scope="module", autouse=True)
def _recorded_cu_count():
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table was recorded on a 256-CU MI355X; the CU count enters the kernel choice")


def _call(entry, M, N, K, out16, act, inputs, prec):
    """The call of a row as a closure (inputs made here, outside the traced region)."""
    from mi355attn import _ffi
    from mi355attn import functional as F
    torch.manual_seed(M + N + K)
    dev = torch.device("cuda", 0)
    dt = F.dtype16(prec)
    bias = torch.randn(N, device=dev) * 0.1 if "b" in inputs else None
    gamma = torch.rand(N, device=dev) + 0.5 if "g" in inputs else None
    resid = torch.randn(M, N, device=dev) if "r" in inputs else None
    w16 = (torch.randn(N, K, device=dev) / K ** 0.5).to(dt)
    if entry == "patch_embed":
        img = torch.randn(M, 3, 224, 224, device=dev)
        wp = torch.randn(N, 3, 16, 16, device=dev) * 0.02
        bp, cls, pos = torch.randn(N, device=dev) * 0.1, torch.randn(1, 1, N, device=dev), torch.randn(1, 197, N, device=dev)
        return lambda: F.patch_embed(img, wp, bp, cls, pos, 16, precision=prec)
    if entry in ("cast_linear16", "ln_linear16"):
        x = torch.randn(M, K, device=dev)
        if entry == "cast_linear16":
            return lambda: F.cast_linear16(x, w16, bias, act=act, precision=prec)
        ln, lin = torch.nn.LayerNorm(K).to(dev), torch.nn.Linear(K, N).to(dev)
        return lambda: F.ln_linear16(x, ln, lin, act=act, out16=bool(out16), precision=prec)
    x16 = torch.randn(M, K, device=dev).to(dt)
    if entry == "linear16":
        return lambda: F.linear16(x16, w16, bias, act=act, gamma=gamma, resid=resid, out16=bool(out16), precision=prec)
    ln = torch.nn.LayerNorm(N).to(dev)
    if entry == "linear16_stats":
        return lambda: F.linear16_stats(x16, w16, bias, resid, 1e-6, precision=prec)
    if entry == "linear16_ln16":
        return lambda: F.linear16_ln16(x16, w16, bias, resid, ln, precision=prec)
    # the C entries themselves: the functional layer does not call them for a shape they refuse
    y = torch.empty(M, N, device=dev)
    st = _ffi.stream_ptr(dev)
    if entry == "linear16_stats_c":
        stats = torch.empty(M, 2, device=dev)
        return lambda: _ffi.check(_ffi.lib().mi355_linear16_stats_fwd(
            _ffi.dptr(x16), _ffi.dptr(w16), _ffi.dptr(bias), _ffi.dptr(resid), _ffi.dptr(y), M, N, K, K, N, prec, _ffi.dptr(stats), 1e-6, st),
            "mi355_linear16_stats_fwd")
    assert entry == "linear16_ln16_c", entry
    u16 = torch.empty(M, N, device=dev, dtype=dt)
    return lambda: _ffi.check(_ffi.lib().mi355_linear16_ln16_fwd(
        _ffi.dptr(x16), _ffi.dptr(w16), _ffi.dptr(bias), _ffi.dptr(resid), _ffi.dptr(y), _ffi.dptr(ln.weight), _ffi.dptr(ln.bias), 1e-5,
        _ffi.dptr(u16), M, N, K, K, N, N, prec, st), "mi355_linear16_ln16_fwd")


def run_row(row, prec):
    """The kernel tally of one call of the row ({tag: launches}), or ("raises", error text)."""
    import mi355attn
    _, entry, (M, N, K), out16, act, inputs, opts, _ = row
    fn = _call(entry, M, N, K, out16, act, inputs, prec)
    with mi355attn.options(**opts), torch.no_grad():
        try:
            fn()                                    # first call: one-time weight preparation stays out of the tally
            torch.cuda.synchronize()
        except mi355attn.Mi355Error as e:
            return ("raises", str(e))
        out = {}

        def call():
            out["y"] = fn()
        tally = collections.Counter()
        for tag, count, *_ in mi355attn.kernel_trace(call):
            tally[tag] += count
    assert out["y"] is not None, "the entry declined the row"
    return dict(tally)


def expected_of(row, prec):
    want = row[-1]
    if isinstance(want, tuple):
        return want
    p = "f16" if prec == 1 else "bf16"
    return {tag.replace("{p}", p): n for tag, n in want.items()}


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_dispatch_runs_the_recorded_kernels(row, prec):
    assert run_row(row, prec) == expected_of(row, prec)
