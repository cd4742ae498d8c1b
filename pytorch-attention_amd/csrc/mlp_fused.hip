// mlp_fused.hip -- y = x + gamma * (W2 gelu(W1 LN(x) + b1) + b2) in ONE kernel for narrow token streams (C = 64, hidden = 256:
// CSWin stage 1, cswin.py:194-196 with Mlp :29-44), gfx950.
//
// At C = 64 the two Linears of the MLP are HBM-bound as separate kernels: the (M x 4C) hidden tensor is written and read back
// (822 MB at the C4 shape, against 410 MB for x and y together) and the first one spends its time in the GELU epilogue.  Here the
// hidden activations never leave registers:
//
//   workgroup = 16 waves sharing one LDS copy of W1 (hidden x C) and W2 (C x hidden) in the MFMA operand format
//   wave      = 32 tokens per step (two 16-token tiles); LayerNorm in registers (a token's C channels live in 4 lanes)
//   per 32 hidden units:  H^T = W1 . Xn^T   (MFMA; a lane then holds 4 consecutive hidden units of one token)
//                         + b1, GELU, re-packed IN-LANE as the A operand of the second product (same trick as P in attn.hip)
//                         Y  += gelu(H) . W2^T   (MFMA)
//   end:                  (+ b2) * gamma -> per-wave LDS slab -> + x (re-read, Infinity-Cache resident) -> 256-byte row stores
// LayerNorm's affine part is folded into W1 / b1 by the caller (W1' = W1 diag(ln_w), b1' = b1 + W1 ln_b): the kernel only
// normalises.  Weights are 16-bit (fp16 / bf16 per `precision`), accumulation fp32.
#include "common.h"
#include "mma.h"

namespace {

struct MlpArgs {
    const void* x; void* y;                    // (M, C) fp32; the IO16 instantiations: 16-bit in the operand type; the o16 kernels: y alone
    const void* w1; const void* w2;            // 16-bit: (HD, C) and (C, HD), row-major
    const float* b1; const float* b2; const float* gamma;
    long M;
    float eps;
    int do_ln;
    // PROJ kernels: x1 = x + ctx Wp^T + bp is formed first (the proj Linear + residual of the block half in front of the MLP,
    // cswin.py:191-193), the MLP then runs on x1:  y = x1 + gamma * (W2 gelu(W1 LN(x1) + b1) + b2)
    const void* ctx; const void* wp; const float* bp;      // ctx (M, C) 16-bit, wp (C, C) 16-bit, bp (C) fp32
    // fp16 range word (common.h rg_report_f, code 4; null for bf16 / under capture without a word): gelu(H) is the one 16-bit intermediate
    // whose magnitude the weights do not bound a priori -- LN(x) is at most sqrt(C - 1) -- and it never reaches HBM, so nobody else sees it
    unsigned* ovf;
    // IO16 and o16 kernels in fp16: the range word again for the y store (code 3, as gemm16_res_kernel reports its 16-bit stores) -- set whether
    // or not the hidden activation is proven, since y = x1 + ... is bounded by nothing
    unsigned* ovf_y;
};

// the kernels: once in the forms of mi355_mlp_fused_fwd / mi355_proj_mlp_fused_fwd / mi355_proj_mlp_fused_x16_fwd, once with an fp32 x and a
// 16-bit y (mlp_fused_body.h)
#define MLP_O16 0
#include "mlp_fused_body.h"
#undef MLP_O16
#define MLP_O16 1
#include "mlp_fused_body.h"
#undef MLP_O16

template <int C, int HD>
constexpr size_t mlp_smem(bool proj = false) {
    return (size_t)(HD * (C + 8) + C * (HD + 4)) * 2 + (size_t)HD * 4 + (size_t)16 * 16 * (C + 4) * 4 + (proj ? (size_t)C * (C + 8) * 2 : 0);
}

}  // namespace

extern "C" int mi355_mlp_fused_fwd(const float* x, const void* w1_16, const float* b1, const void* w2_16, const float* b2, const float* gamma,
                                   float* y, long M, int C, int hidden, int layernorm, float eps, int precision, mi355_stream_t stream) {
    MI355_CHECK_ARG(x && w1_16 && b1 && w2_16 && y && M > 0);
    MI355_CHECK_ARG(precision == MI355_PREC_FP16 || precision == MI355_PREC_BF16);
    MI355_CHECK_ARG(layernorm >= 0 && layernorm <= 3);                          // flag word: bit 0 LayerNorm, bit 1 range proven
    if (!aligned16(x) || !aligned16(y) || !aligned16(w1_16) || !aligned16(w2_16))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_mlp_fused_fwd: 16-byte aligned buffers required");
    if (mi355::mlp_wide_applicable(C, hidden) && mi355::opt(mi355::O_MLP_WIDE)) {        // C = 256 / 384: the weight-split kernel (mlp_wide.hip), W2 row-major
        if ((b2 && !aligned16(b2)) || (gamma && !aligned16(gamma)) || !aligned16(b1))
            return mi355::fail(MI355_EUNSUPPORTED, "mi355_mlp_fused_fwd: 16-byte aligned bias / LayerScale vectors required at C = %d", C);
        if (int rc = mi355::mlp_wide(x, w1_16, b1, w2_16, b2, gamma, y, M, C, layernorm, eps, precision, static_cast<hipStream_t>(stream))) return rc;
        MI355_LAUNCH_CHECK();
        return MI355_OK;
    }
    if (!((C == 64 && hidden == 256) || (C == 128 && hidden == 512)))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_mlp_fused_fwd: built for C = 64 / 128 / 256 / 384 with hidden = 4 C (got C = %d, hidden = %d)", C, hidden);
    MlpArgs a{};
    a.x = x; a.y = y; a.w1 = w1_16; a.w2 = w2_16; a.b1 = b1; a.b2 = b2; a.gamma = gamma; a.M = M; a.eps = eps; a.do_ln = (layernorm & 1) ? 1 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // layernorm bit 1: the caller has PROVEN |gelu(H)| < 65504 from the folded weights (|LN(x)| <= sqrt(C - 1)): nothing to report, and the
    // launch is not a producer the host would have to wait for (mi355_range_wait)
    a.ovf = (precision == MI355_PREC_FP16 && !(layernorm & 2)) ? mi355::range_word(st) : nullptr;
    const int ncu = mi355::resident_slots(1);
    MI355_TRACE(st, "mlp_fused_kernel<C=%d> M=%ld", C, M);
    if (C == 128) {
        constexpr size_t sm = (size_t)2 * (32 * (128 + 8) + 128 * 36) * 2 + (size_t)8 * 16 * 68 * 4 + (size_t)512 * 4;
        static_assert(sm <= 160 * 1024, "LDS budget");
        const long niter = ((M + 15) / 16 + 15) / 16;
        const int grid2 = (int)(niter < ncu ? niter : ncu);
        if (precision == MI355_PREC_FP16) {
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_stream_kernel<1, 128, 512>), (int)sm)) return rc;
            mlp_fused_stream_kernel<1, 128, 512><<<grid2, 512, sm, st>>>(a);
        } else {
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_stream_kernel<2, 128, 512>), (int)sm)) return rc;
            mlp_fused_stream_kernel<2, 128, 512><<<grid2, 512, sm, st>>>(a);
        }
        MI355_LAUNCH_CHECK();
        return MI355_OK;
    }
    constexpr size_t smem = mlp_smem<64, 256>();
    static_assert(smem <= 160 * 1024, "LDS budget");
    const bool tt4 = mi355::opt(mi355::O_MLP_TT4) != 0;
    const long nchunk = (M + (tt4 ? 63 : 31)) / (tt4 ? 64 : 32);
    long grid = (nchunk + (tt4 ? 7 : 15)) / (tt4 ? 8 : 16);
    if (grid > ncu) grid = ncu;
#define MLP64(P_, PR_, IO_)                                                                                                                   \
    do {                                                                                                                                  \
        if (tt4) {                                                                                                                        \
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_kernel<P_, 64, 256, PR_, 8, 4, IO_>), (int)smem)) return rc;   \
            mlp_fused_kernel<P_, 64, 256, PR_, 8, 4, IO_><<<(int)grid, 512, smem, st>>>(a);                                                    \
        } else {                                                                                                                          \
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_kernel<P_, 64, 256, PR_, 16, 2, IO_>), (int)smem)) return rc; \
            mlp_fused_kernel<P_, 64, 256, PR_, 16, 2, IO_><<<(int)grid, 1024, smem, st>>>(a);                                                         \
        }                                                                                                                                 \
    } while (0)
    if (precision == MI355_PREC_FP16) MLP64(1, false, false);
    else MLP64(2, false, false);
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}

extern "C" int mi355_proj_mlp_fused_fwd(const float* x, const void* ctx16, const void* wp16, const float* bp, const void* w1_16, const float* b1,
                                        const void* w2_16, const float* b2, const float* gamma, float* y, long M, int C, int hidden,
                                        int layernorm, float eps, int precision, mi355_stream_t stream) {
    MI355_CHECK_ARG(x && ctx16 && wp16 && bp && w1_16 && b1 && w2_16 && y && M > 0);
    MI355_CHECK_ARG(precision == MI355_PREC_FP16 || precision == MI355_PREC_BF16);
    MI355_CHECK_ARG(layernorm >= 0 && layernorm <= 3);                          // flag word: bit 0 LayerNorm, bit 1 range proven
    if (!((C == 64 && hidden == 256) || (C == 128 && hidden == 512)))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_proj_mlp_fused_fwd: built for C = 64, hidden = 256 and C = 128, hidden = 512 (got C = %d, hidden = %d)", C, hidden);
    if (!aligned16(x) || !aligned16(y) || !aligned16(w1_16) || !aligned16(w2_16) || !aligned16(ctx16) || !aligned16(wp16) || !aligned16(bp))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_proj_mlp_fused_fwd: 16-byte aligned buffers required");
    MlpArgs a{};
    a.x = x; a.y = y; a.w1 = w1_16; a.w2 = w2_16; a.b1 = b1; a.b2 = b2; a.gamma = gamma; a.M = M; a.eps = eps; a.do_ln = (layernorm & 1) ? 1 : 0;
    a.ctx = ctx16; a.wp = wp16; a.bp = bp;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // layernorm bit 1: the caller has PROVEN |gelu(H)| < 65504 from the folded weights (|LN(x)| <= sqrt(C - 1)): nothing to report, and the
    // launch is not a producer the host would have to wait for (mi355_range_wait)
    a.ovf = (precision == MI355_PREC_FP16 && !(layernorm & 2)) ? mi355::range_word(st) : nullptr;
    const int ncu = mi355::resident_slots(1);
    MI355_TRACE(st, "mlp_fused_kernel<C=%d,proj> M=%ld", C, M);
    if (C == 128) {
        constexpr size_t sm = (size_t)2 * (32 * (128 + 8) + 128 * 36) * 2 + (size_t)8 * 16 * 68 * 4 + (size_t)128 * (128 + 8) * 2 + (size_t)512 * 4;
        static_assert(sm <= 160 * 1024, "LDS budget");
        const long niter = ((M + 15) / 16 + 15) / 16;
        const int grid2 = (int)(niter < ncu ? niter : ncu);
        if (precision == MI355_PREC_FP16) {
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_stream_kernel<1, 128, 512, true>), (int)sm)) return rc;
            mlp_fused_stream_kernel<1, 128, 512, true><<<grid2, 512, sm, st>>>(a);
        } else {
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_stream_kernel<2, 128, 512, true>), (int)sm)) return rc;
            mlp_fused_stream_kernel<2, 128, 512, true><<<grid2, 512, sm, st>>>(a);
        }
        MI355_LAUNCH_CHECK();
        return MI355_OK;
    }
    constexpr size_t smem = mlp_smem<64, 256>(true);
    static_assert(smem <= 160 * 1024, "LDS budget");
    const bool tt4 = mi355::opt(mi355::O_MLP_TT4) != 0;
    const long nchunk = (M + (tt4 ? 63 : 31)) / (tt4 ? 64 : 32);
    long grid = (nchunk + (tt4 ? 7 : 15)) / (tt4 ? 8 : 16);
    if (grid > ncu) grid = ncu;
    if (precision == MI355_PREC_FP16) MLP64(1, true, false);
    else MLP64(2, true, false);
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}

// mi355_proj_mlp_fused_fwd with x16 and y16 (M, C) in the operand type of `precision` (the IO16 instantiations): same grids, same LDS
extern "C" int mi355_proj_mlp_fused_x16_fwd(const void* x16, const void* ctx16, const void* wp16, const float* bp, const void* w1_16, const float* b1,
                                            const void* w2_16, const float* b2, const float* gamma, void* y16, long M, int C, int hidden,
                                            int layernorm, float eps, int precision, mi355_stream_t stream) {
    MI355_CHECK_ARG(x16 && ctx16 && wp16 && bp && w1_16 && b1 && w2_16 && y16 && M > 0);
    MI355_CHECK_ARG(precision == MI355_PREC_FP16 || precision == MI355_PREC_BF16);
    MI355_CHECK_ARG(layernorm >= 0 && layernorm <= 3);                          // flag word: bit 0 LayerNorm, bit 1 range proven
    if (!((C == 64 && hidden == 256) || (C == 128 && hidden == 512)))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_proj_mlp_fused_x16_fwd: built for C = 64, hidden = 256 and C = 128, hidden = 512 (got C = %d, hidden = %d)", C, hidden);
    if (!aligned16(x16) || !aligned16(y16) || !aligned16(w1_16) || !aligned16(w2_16) || !aligned16(ctx16) || !aligned16(wp16) || !aligned16(bp))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_proj_mlp_fused_x16_fwd: 16-byte aligned buffers required");
    MlpArgs a{};
    a.x = x16; a.y = y16; a.w1 = w1_16; a.w2 = w2_16; a.b1 = b1; a.b2 = b2; a.gamma = gamma; a.M = M; a.eps = eps; a.do_ln = (layernorm & 1) ? 1 : 0;
    a.ctx = ctx16; a.wp = wp16; a.bp = bp;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the fp16 y store can always saturate (code 3), so an fp16 launch is a producer whether or not the hidden activation is proven (bit 1:
    // code 4 is then not reported)
    a.ovf_y = precision == MI355_PREC_FP16 ? mi355::range_word(st) : nullptr;
    a.ovf = (layernorm & 2) ? nullptr : a.ovf_y;
    const int ncu = mi355::resident_slots(1);
    MI355_TRACE(st, "mlp_fused_kernel<C=%d,proj,x16> M=%ld", C, M);
    if (C == 128) {
        constexpr size_t sm = (size_t)2 * (32 * (128 + 8) + 128 * 36) * 2 + (size_t)8 * 16 * 68 * 4 + (size_t)128 * (128 + 8) * 2 + (size_t)512 * 4;
        static_assert(sm <= 160 * 1024, "LDS budget");
        const long niter = ((M + 15) / 16 + 15) / 16;
        const int grid2 = (int)(niter < ncu ? niter : ncu);
        if (precision == MI355_PREC_FP16) {
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_stream_kernel<1, 128, 512, true, true>), (int)sm)) return rc;
            mlp_fused_stream_kernel<1, 128, 512, true, true><<<grid2, 512, sm, st>>>(a);
        } else {
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_stream_kernel<2, 128, 512, true, true>), (int)sm)) return rc;
            mlp_fused_stream_kernel<2, 128, 512, true, true><<<grid2, 512, sm, st>>>(a);
        }
        MI355_LAUNCH_CHECK();
        return MI355_OK;
    }
    constexpr size_t smem = mlp_smem<64, 256>(true);
    static_assert(smem <= 160 * 1024, "LDS budget");
    const bool tt4 = mi355::opt(mi355::O_MLP_TT4) != 0;
    const long nchunk = (M + (tt4 ? 63 : 31)) / (tt4 ? 64 : 32);
    long grid = (nchunk + (tt4 ? 7 : 15)) / (tt4 ? 8 : 16);
    if (grid > ncu) grid = ncu;
    if (precision == MI355_PREC_FP16) MLP64(1, true, true);
    else MLP64(2, true, true);
#undef MLP64
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}

// mi355_mlp_fused_fwd with y16 (M, C) in the operand type of `precision` (I/O form 2): x stays fp32 -- the residual stream behind the LPI
// third of an XCABlock on fp16 / bf16 activations -- and the epilogue rounds x + gamma * mlp once.  Same grids, same LDS; C = 64 / 128 only
// (the weight-split kernel of C = 256 / 384 has no 16-bit store).
extern "C" int mi355_mlp_fused_o16_fwd(const float* x, const void* w1_16, const float* b1, const void* w2_16, const float* b2, const float* gamma,
                                       void* y16, long M, int C, int hidden, int layernorm, float eps, int precision, mi355_stream_t stream) {
    MI355_CHECK_ARG(x && w1_16 && b1 && w2_16 && y16 && M > 0);
    MI355_CHECK_ARG(precision == MI355_PREC_FP16 || precision == MI355_PREC_BF16);
    MI355_CHECK_ARG(layernorm >= 0 && layernorm <= 3);                          // flag word: bit 0 LayerNorm, bit 1 range proven
    if (!((C == 64 && hidden == 256) || (C == 128 && hidden == 512)))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_mlp_fused_o16_fwd: built for C = 64, hidden = 256 and C = 128, hidden = 512 (got C = %d, hidden = %d)", C, hidden);
    if (!aligned16(x) || !aligned16(y16) || !aligned16(w1_16) || !aligned16(w2_16))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_mlp_fused_o16_fwd: 16-byte aligned buffers required");
    MlpArgs a{};
    a.x = x; a.y = y16; a.w1 = w1_16; a.w2 = w2_16; a.b1 = b1; a.b2 = b2; a.gamma = gamma; a.M = M; a.eps = eps; a.do_ln = (layernorm & 1) ? 1 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the fp16 y store can always saturate (code 3): an fp16 launch is a producer whether or not the hidden activation is proven (bit 1)
    a.ovf_y = precision == MI355_PREC_FP16 ? mi355::range_word(st) : nullptr;
    a.ovf = (layernorm & 2) ? nullptr : a.ovf_y;
    const int ncu = mi355::resident_slots(1);
    MI355_TRACE(st, "mlp_fused_kernel<C=%d,o16> M=%ld", C, M);
    if (C == 128) {
        constexpr size_t sm = (size_t)2 * (32 * (128 + 8) + 128 * 36) * 2 + (size_t)8 * 16 * 68 * 4 + (size_t)512 * 4;
        static_assert(sm <= 160 * 1024, "LDS budget");
        const long niter = ((M + 15) / 16 + 15) / 16;
        const int grid2 = (int)(niter < ncu ? niter : ncu);
        if (precision == MI355_PREC_FP16) {
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_stream_o16_kernel<1, 128, 512>), (int)sm)) return rc;
            mlp_fused_stream_o16_kernel<1, 128, 512><<<grid2, 512, sm, st>>>(a);
        } else {
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_stream_o16_kernel<2, 128, 512>), (int)sm)) return rc;
            mlp_fused_stream_o16_kernel<2, 128, 512><<<grid2, 512, sm, st>>>(a);
        }
        MI355_LAUNCH_CHECK();
        return MI355_OK;
    }
    constexpr size_t smem = mlp_smem<64, 256>();
    static_assert(smem <= 160 * 1024, "LDS budget");
    const bool tt4 = mi355::opt(mi355::O_MLP_TT4) != 0;
    const long nchunk = (M + (tt4 ? 63 : 31)) / (tt4 ? 64 : 32);
    long grid = (nchunk + (tt4 ? 7 : 15)) / (tt4 ? 8 : 16);
    if (grid > ncu) grid = ncu;
#define MLP64_O16(P_)                                                                                                                     \
    do {                                                                                                                                  \
        if (tt4) {                                                                                                                        \
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_o16_kernel<P_, 64, 256, 8, 4>), (int)smem)) return rc;  \
            mlp_fused_o16_kernel<P_, 64, 256, 8, 4><<<(int)grid, 512, smem, st>>>(a);                                                       \
        } else {                                                                                                                          \
            if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mlp_fused_o16_kernel<P_, 64, 256, 16, 2>), (int)smem)) return rc; \
            mlp_fused_o16_kernel<P_, 64, 256, 16, 2><<<(int)grid, 1024, smem, st>>>(a);                                                     \
        }                                                                                                                                 \
    } while (0)
    if (precision == MI355_PREC_FP16) MLP64_O16(1);
    else MLP64_O16(2);
#undef MLP64_O16
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}
