// mixer_fused.hip -- the token-mixing half of a MixerLayer in ONE kernel (+ a row-statistics pass), gfx950:
//
//   y = x + ( gelu( LN(x)^T W1^T + b1 ) W2^T + b2 )^T          mlp_mixer.py:47 with Mlp.forward :27-33 and norm1
//
// for N = 196 tokens (14 x 14 patches), T % 32 == 0 hidden token units (the Mixer's default: T = C / 2 = 256), C % 256 == 0 channels.  As three launches
// (transposing LayerNorm -> fc1 + GELU -> transposed-output fc2 + residual: layernorm.hip, gemm16_pa.hip, gemm16.hip) the half moves
// 560 MB and takes 175 us at B = 256, C = 512 for 26 GFLOP: the 16-bit LN(x)^T (59 MB) and the hidden tensor (67 MB) are written and
// read back, and every launch is bound by that traffic.  Here both stay on the chip:
//
//   workgroup = (image, 256 channels), 8 waves; wave = 32 channels (two 16-channel MFMA tiles), ALL tokens
//   phase 1   the wave reads its 32-channel slab of the image (one 128-byte line per token, 8 lanes per line), applies LayerNorm with
//             the row statistics of the pre-pass, and parks the 16-bit result CHANNEL-major in a wave-private LDS region (two tokens
//             per 32-bit word); from there it takes the B operand of the first product -- lane (l15, g): 8 consecutive tokens of
//             channel l15 -- into registers for the whole kernel (14 x 16 bytes)
//   phase 2   hidden units in blocks of 32, W1 / W2 slices double-buffered through LDS (the scheme of mlp_fused_stream_kernel):
//             H^T = W1 . U     (MFMA; a lane then holds 4 consecutive hidden units of one channel) + b1, GELU, re-packed in-lane as
//             the A operand of  O += gelu(H) . W2^T   (rows = channels, columns = tokens)
//   phase 3   a lane holds 4 consecutive CHANNELS of one token per accumulator: + b2[token] + x (re-read: the lines were fetched
//             microseconds ago) and 16-byte stores straight from the accumulators -- the reference's two transposes never exist.
// The stage buffers alias the wave-private regions of phase 1 (one barrier in between).  16-bit operands (fp16 / bf16 per `precision`),
// fp32 accumulation; the GELU result is rounded to 16 bits as the operand of the second product (gelu16_fast4).
//
// 16-bit x (mi355_mixer_token_x16_fwd: a .half() / .bfloat16() model or autocast): mixer_token16_kernel and row_stats_x16_kernel are the same
// bodies reading x in the operand format itself -- 64 bytes per token and wave in phase 1 (8 lanes x 8 bytes: still whole lines per group
// of lanes, the lane map unchanged) and in the residual re-read of phase 3 -- and widening it in registers, which is exact: the fp32
// result is bit for bit what the fp32-x kernels compute from x.float(), and it is written as fp32 (the layer's residual stream).  The
// options "mixer_early" and "mixer_stats" apply to the 16-bit-x form exactly as to the fp32 one (same template arguments, same tags
// behind the type: mixer_token16_kernel<f16><early><stats>).
#include "common.h"
#include "mma.h"

namespace {

constexpr int MX_N = 196, MX_NK = 224, MX_KS = MX_NK / 32, MX_TMAX = 512, MX_NT = 13, MX_NP = MX_NT * 16;      // T: any multiple of 32 up to TMAX
constexpr int MX_PU = MX_NK + 8;                 // pitch of the parked operand rows and of the W1 slice rows (elements)
constexpr int MX_P2 = 32 + 4;                    // pitch of the W2 slice rows
constexpr int MX_W1S = 32 * MX_PU, MX_W2S = MX_NP * MX_P2, MX_STAGE = MX_W1S + MX_W2S;
constexpr int MX_REGION = 32 * MX_PU;            // elements per wave-private region
constexpr size_t MX_LDS = (size_t)8 * MX_REGION * 2 + (size_t)(MX_TMAX + MX_NP + 2 * MX_NP) * 4;
static_assert((size_t)2 * MX_STAGE * 2 <= (size_t)8 * MX_REGION * 2, "the two weight stages alias the parked operand");
static_assert(MX_LDS <= 160 * 1024, "LDS budget");

struct MixArgs {
    const void* x;              // (B, 196, C): fp32 (mixer_token_kernel) or the operand format itself (mixer_token16_kernel)
    float* y; const float* stats;
    const float* ln_w; const float* ln_b;
    const void* w1p;            // (T, 224) 16-bit, columns >= 196 zero
    const void* w2s;            // (T / 32, 208, 32) 16-bit slice-major, rows >= 196 zero
    const float* b1; const float* b2;
    int C, halves, T;           // halves = C / 256 workgroups per image; T hidden token units
    int pair_xcd;               // halves == 2 and B % 8 == 0: the two workgroups of an image get block ids 8 apart (same XCD)
    float eps;                  // LayerNorm eps (STATS kernels)
    unsigned* ovf;              // fp16 range word (common.h rg_report): the 16-bit LN(x) and gelu(H) operands are tracked like the
                                // stand-alone producers they replace (layernorm16_t, the 16-bit GEMM epilogue); null = unguarded
};

// Four consecutive values of a 16-bit x as fp32: one 8-byte load, widened in registers (exact).
template <class XT>
__device__ __forceinline__ f4 ldx4(const XT* p) {
    typedef XT x4 __attribute__((ext_vector_type(4)));
    const x4 v = *reinterpret_cast<const x4*>(p);
    return f4{(float)v.x, (float)v.y, (float)v.z, (float)v.w};
}

// the kernels: once for an fp32 x, once for a 16-bit x (mixer_token_body.h)
#define MX_X16 0
#include "mixer_token_body.h"
#undef MX_X16
#define MX_X16 1
#include "mixer_token_body.h"
#undef MX_X16

}  // namespace

extern "C" {

size_t mi355_mixer_token_workspace_bytes(int B, int N, int C) {
    (void)C;
    if (B <= 0 || N <= 0) return 16;
    return (size_t)B * N * 2 * sizeof(float) + 16;
}

int mi355_mixer_token_fwd(const float* x, const float* ln_w, const float* ln_b, float ln_eps, const void* w1p16, const float* b1,
                          const void* w2s16, const float* b2, float* y, int B, int N, int C, int T, int precision, void* ws, size_t ws_bytes,
                          mi355_stream_t stream) {
    MI355_CHECK_ARG(x && ln_w && ln_b && w1p16 && b1 && w2s16 && b2 && y && ws && B > 0);
    MI355_CHECK_ARG(precision == MI355_PREC_FP16 || precision == MI355_PREC_BF16);
    if (N != MX_N || T <= 0 || (T % 32) != 0 || T > MX_TMAX || C <= 0 || (C % 256) != 0 || C > 1024)
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_mixer_token_fwd: built for N = 196 tokens, T %% 32 == 0 (<= 512), C %% 256 == 0 (<= 1024) (N=%d T=%d C=%d)", N, T, C);
    if (!aligned16(x) || !aligned16(y) || !aligned16(ws) || !aligned16(w1p16) || !aligned16(w2s16) || !aligned16(ln_w) || !aligned16(ln_b))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_mixer_token_fwd: 16-byte aligned buffers required");
    MI355_CHECK_ARG(ws_bytes >= mi355_mixer_token_workspace_bytes(B, N, C));
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* stats = static_cast<float*>(ws);
    const long rows = (long)B * N;
    const bool instats = mi355::opt(mi355::O_MIXER_STATS) != 0 && C == 512;    // statistics inside the token kernel (phase 0; built for C = 512) or by the pre-pass
    if (!instats) {
        const int sgrid = (int)(cdiv(rows, 4) < 8192 ? cdiv(rows, 4) : 8192);
        MI355_TRACE(st, "row_stats_kernel rows=%ld cols=%d", rows, C);
        if (C <= 256) row_stats_kernel<1><<<sgrid, 256, 0, st>>>(x, stats, rows, C, ln_eps);
        else if (C <= 512) row_stats_kernel<2><<<sgrid, 256, 0, st>>>(x, stats, rows, C, ln_eps);
        else row_stats_kernel<4><<<sgrid, 256, 0, st>>>(x, stats, rows, C, ln_eps);
        MI355_LAUNCH_CHECK();
    }
    MixArgs a{};
    a.x = x; a.y = y; a.stats = stats; a.ln_w = ln_w; a.ln_b = ln_b; a.w1p = w1p16; a.w2s = w2s16; a.b1 = b1; a.b2 = b2;
    a.C = C; a.halves = C / 256; a.T = T; a.eps = ln_eps;
    a.pair_xcd = (a.halves == 2 && (B % 8) == 0) ? 1 : 0;
    const long grid = (long)B * a.halves;
    if (grid >= (1L << 31)) return mi355::fail(MI355_EUNSUPPORTED, "mi355_mixer_token_fwd: batch too large");
    a.ovf = precision == MI355_PREC_FP16 ? mi355::range_word(st) : nullptr;
    const bool early = mi355::opt(mi355::O_MIXER_EARLY) != 0;
    MI355_TRACE(st, "mixer_token_kernel%s%s B=%d C=%d", early ? "<early>" : "", instats ? "<stats>" : "", B, C);
#define MIXER_LAUNCH(P_, E_, S_)                                                                                                      \
    do {                                                                                                                             \
        if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mixer_token_kernel<P_, E_, S_>), (int)MX_LDS)) return rc;  \
        mixer_token_kernel<P_, E_, S_><<<(int)grid, 512, MX_LDS, st>>>(a);                                                           \
    } while (0)
#define MIXER_BY(P_)                                                                            \
    do {                                                                                        \
        if (early) { if (instats) MIXER_LAUNCH(P_, true, 2); else MIXER_LAUNCH(P_, true, 0); }   \
        else       { if (instats) MIXER_LAUNCH(P_, false, 2); else MIXER_LAUNCH(P_, false, 0); } \
    } while (0)
    if (precision == MI355_PREC_FP16) MIXER_BY(1);
    else MIXER_BY(2);
#undef MIXER_BY
#undef MIXER_LAUNCH
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}

// The same half for an x in the operand format itself (io = 1: fp16, 2: bf16): x16 (B,196,C) 16-bit -> y (B,196,C) fp32, the residual
// stream of the layer.  Same envelope, workspace, weight layouts, options and range guard as mi355_mixer_token_fwd at precision = io;
// the values are the ones that entry computes from x16 widened to fp32.
size_t mi355_mixer_token_x16_workspace_bytes(int B, int N, int C) { return mi355_mixer_token_workspace_bytes(B, N, C); }

int mi355_mixer_token_x16_fwd(const void* x16, const float* ln_w, const float* ln_b, float ln_eps, const void* w1p16, const float* b1,
                            const void* w2s16, const float* b2, float* y, int B, int N, int C, int T, int io, void* ws, size_t ws_bytes,
                            mi355_stream_t stream) {
    MI355_CHECK_ARG(x16 && ln_w && ln_b && w1p16 && b1 && w2s16 && b2 && y && ws && B > 0);
    MI355_CHECK_ARG(io == MI355_PREC_FP16 || io == MI355_PREC_BF16);
    if (N != MX_N || T <= 0 || (T % 32) != 0 || T > MX_TMAX || C <= 0 || (C % 256) != 0 || C > 1024)
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_mixer_token_x16_fwd: built for N = 196 tokens, T %% 32 == 0 (<= 512), C %% 256 == 0 (<= 1024) (N=%d T=%d C=%d)", N, T, C);
    if (!aligned16(x16) || !aligned16(y) || !aligned16(ws) || !aligned16(w1p16) || !aligned16(w2s16) || !aligned16(ln_w) || !aligned16(ln_b))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_mixer_token_x16_fwd: 16-byte aligned buffers required");
    MI355_CHECK_ARG(ws_bytes >= mi355_mixer_token_x16_workspace_bytes(B, N, C));
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* stats = static_cast<float*>(ws);
    const long rows = (long)B * N;
    const char* tname = io == MI355_PREC_FP16 ? "f16" : "bf16";
    const bool instats = mi355::opt(mi355::O_MIXER_STATS) != 0 && C == 512;
    if (!instats) {
        const int sgrid = (int)(cdiv(rows, 4) < 8192 ? cdiv(rows, 4) : 8192);
        MI355_TRACE(st, "row_stats_x16_kernel<%s> rows=%ld cols=%d", tname, rows, C);
#define STATS16(T_)                                                                                                        \
    do {                                                                                                                   \
        const T_* xs = static_cast<const T_*>(x16);                                                                        \
        if (C <= 256) row_stats_x16_kernel<T_, 1><<<sgrid, 256, 0, st>>>(xs, stats, rows, C, ln_eps);                        \
        else if (C <= 512) row_stats_x16_kernel<T_, 2><<<sgrid, 256, 0, st>>>(xs, stats, rows, C, ln_eps);                   \
        else row_stats_x16_kernel<T_, 4><<<sgrid, 256, 0, st>>>(xs, stats, rows, C, ln_eps);                                 \
    } while (0)
        if (io == MI355_PREC_FP16) STATS16(_Float16); else STATS16(__bf16);
#undef STATS16
        MI355_LAUNCH_CHECK();
    }
    MixArgs a{};
    a.x = x16; a.y = y; a.stats = stats; a.ln_w = ln_w; a.ln_b = ln_b; a.w1p = w1p16; a.w2s = w2s16; a.b1 = b1; a.b2 = b2;
    a.C = C; a.halves = C / 256; a.T = T; a.eps = ln_eps;
    a.pair_xcd = (a.halves == 2 && (B % 8) == 0) ? 1 : 0;
    const long grid = (long)B * a.halves;
    if (grid >= (1L << 31)) return mi355::fail(MI355_EUNSUPPORTED, "mi355_mixer_token_x16_fwd: batch too large");
    a.ovf = io == MI355_PREC_FP16 ? mi355::range_word(st) : nullptr;
    const bool early = mi355::opt(mi355::O_MIXER_EARLY) != 0;
    MI355_TRACE(st, "mixer_token16_kernel<%s>%s%s B=%d C=%d", tname, early ? "<early>" : "", instats ? "<stats>" : "", B, C);
#define MIXER16_LAUNCH(P_, E_, S_)                                                                                                      \
    do {                                                                                                                               \
        if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(mixer_token16_kernel<P_, E_, S_>), (int)MX_LDS)) return rc;  \
        mixer_token16_kernel<P_, E_, S_><<<(int)grid, 512, MX_LDS, st>>>(a);                                                           \
    } while (0)
#define MIXER16_BY(P_)                                                                              \
    do {                                                                                            \
        if (early) { if (instats) MIXER16_LAUNCH(P_, true, 2); else MIXER16_LAUNCH(P_, true, 0); }   \
        else       { if (instats) MIXER16_LAUNCH(P_, false, 2); else MIXER16_LAUNCH(P_, false, 0); } \
    } while (0)
    if (io == MI355_PREC_FP16) MIXER16_BY(1);
    else MIXER16_BY(2);
#undef MIXER16_BY
#undef MIXER16_LAUNCH
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}

}  // extern "C"
