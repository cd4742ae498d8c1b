// gemm16_res.hip -- the 16-bit GEMM with a residual whose residual and / or result is 16-bit (mi355_linear16_res_fwd):
//
//   Y (M x N) = round_out( widen(resid) + act( X16 (M x K) . W16^T (N x K) + bias ) )      X16, W16: IEEE half (precision 1) or bfloat16 (2)
//   ... with a LayerScale (mi355_linear16_res_scale_fwd):  round_out( widen(resid) + gamma * act( .. ) )
//
// Every persistent kernel of the engine refuses a 16-bit output WITH a residual (their 16-bit epilogues round in the layout-change slab,
// before a residual could be added), and none reads a 16-bit residual.  A ViT encoder block on fp16 / bf16 activations has both: proj
// adds the block's 16-bit input to an fp32 stream (r16, o32), fc2 adds that fp32 stream and stores the block's 16-bit output (r32, o16).
// Here the residual is loaded IN ACCUMULATOR LAYOUT -- lane (l15, g) of a transposed 16 x 16 MFMA tile holds row m and four consecutive
// columns, i.e. one 8-byte (16-bit) or 16-byte (fp32) pack of the residual row -- widened in registers (exact), added in fp32 behind bias
// and activation, and the sum is rounded ONCE on its way out.  No slab, no second pass, no inter-workgroup exchange (capture-safe, and
// a row's bits never depend on the batch around it).
//
// Main loop: the engine's 128 x BN x 64 tile (BN = 256: 8 waves of 64 x 64; BN = 128: 4 waves, where 256-wide tiles would not fill the
// chip), LDS-DMA staging with the source-side XOR swizzle, one LDS buffer and two barriers per K-step, several workgroups per CU -- the
// other workgroups' main loops cover this one's residual loads and stores.  K-tiles are added in ascending order into one accumulator
// per output, MFMA 16x16x32, epilogue order bias / act / residual: a row's fp32 value is the bits mi355_linear16_ws_fwd computes.
#include <type_traits>
#include "gemm16.h"

namespace {
using namespace g16;

struct ResArgs {
    const void* A; const void* B; const float* bias; const void* resid; void* C;
    int M, N, K, lda, ldc, act;
    unsigned* ovf;      // fp16 range guard word (common.h rg_report) for an fp16 store, else null
    const float* gamma; // gemm16_res_scale_kernel only: the LayerScale (N), not null there
};

// the kernel: once without and once with the LayerScale (gemm16_res_body.h)
#define RES_SCALE 0
#include "gemm16_res_body.h"
#undef RES_SCALE
#define RES_SCALE 1
#include "gemm16_res_body.h"
#undef RES_SCALE

template <typename T, bool R16, bool O16>
void launch_res(const ResArgs& g, bool narrow, hipStream_t st) {
    if (g.gamma) {
        if (narrow) gemm16_res_scale_kernel<T, R16, O16, 128, 2><<<cdiv(g.M, 128) * cdiv(g.N, 128), 256, 0, st>>>(g);
        else        gemm16_res_scale_kernel<T, R16, O16, 256, 4><<<cdiv(g.M, 128) * cdiv(g.N, 256), 512, 0, st>>>(g);
        return;
    }
    if (narrow) gemm16_res_kernel<T, R16, O16, 128, 2><<<cdiv(g.M, 128) * cdiv(g.N, 128), 256, 0, st>>>(g);
    else        gemm16_res_kernel<T, R16, O16, 256, 4><<<cdiv(g.M, 128) * cdiv(g.N, 256), 512, 0, st>>>(g);
}

template <typename T>
void launch_res_io(const ResArgs& g, bool r16, bool o16, bool narrow, hipStream_t st) {
    if (r16 && o16)  launch_res<T, true, true>(g, narrow, st);
    else if (r16)    launch_res<T, true, false>(g, narrow, st);
    else             launch_res<T, false, true>(g, narrow, st);
}

}  // namespace

// The one launcher of mi355_linear16_res_fwd (gamma null) and mi355_linear16_res_scale_fwd; `who` names the entry in the error texts.
static int linear16_res_launch(const char* who, const void* X16, const void* W16, const float* bias, const float* gamma, const void* resid,
                               int resid_io, void* Y, int out_io, int M, int N, int K, int ldx, int ldy, int act, int precision,
                               mi355_stream_t stream) {
#define RES_CHECK_ARG(cond)                                                                 \
    do {                                                                                    \
        if (!(cond)) return mi355::fail(MI355_EINVAL, "%s: invalid argument: %s", who, #cond); \
    } while (0)
    RES_CHECK_ARG(X16 && W16 && resid && Y && M > 0 && N > 0 && K > 0 && ldx >= K && ldy >= N);
    RES_CHECK_ARG(act == MI355_ACT_NONE || act == MI355_ACT_GELU);
    RES_CHECK_ARG(precision == MI355_PREC_FP16 || precision == MI355_PREC_BF16);
    RES_CHECK_ARG((resid_io == 0 || resid_io == precision) && (out_io == 0 || out_io == precision));
    if (resid_io == 0 && out_io == 0)
        return mi355::fail(MI355_EUNSUPPORTED, "%s: an fp32 residual with an fp32 result is mi355_linear16_ws_fwd's", who);
    if ((K % BK) || (N & 7) || (ldx & 7) || (ldy & 7) || !aligned16(X16) || !aligned16(W16) || !aligned16(Y) || !aligned16(resid) ||
        (bias && !aligned16(bias)) || (gamma && !aligned16(gamma)) || (long)cdiv(M, 128) * cdiv(N, 128) >= (1L << 31))
        return mi355::fail(MI355_EUNSUPPORTED, "%s: needs K %% 64 == 0, N %% 8 == 0, 16-byte aligned rows (K=%d N=%d ldx=%d ldy=%d)", who,
                           K, N, ldx, ldy);
#undef RES_CHECK_ARG
    hipStream_t st = static_cast<hipStream_t>(stream);
    ResArgs g{};
    g.A = X16; g.B = W16; g.bias = bias; g.gamma = gamma; g.resid = resid; g.C = Y;
    g.M = M; g.N = N; g.K = K; g.lda = ldx; g.ldc = ldy; g.act = act;
    if (out_io == MI355_PREC_FP16) g.ovf = mi355::range_word(st);              // fp16 range guard, like every 16-bit GEMM epilogue
    // 128 x 256 tiles where they give every CU one, else 128 x 128 (the engine's rule for its plain tile kernel)
    const bool narrow = N <= 128 || (long)cdiv(M, 128) * cdiv(N, 256) < mi355::resident_slots(1);
    MI355_TRACE(st, "gemm16_res_kernel<%s,%s,%s%s> M=%d N=%d K=%d%s", precision == MI355_PREC_FP16 ? "f16" : "bf16", resid_io ? "r16" : "r32",
                out_io ? "o16" : "o32", gamma ? ",scale" : "", M, N, K, act == MI355_ACT_GELU ? " gelu" : "");
    if (precision == MI355_PREC_FP16) launch_res_io<_Float16>(g, resid_io != 0, out_io != 0, narrow, st);
    else                              launch_res_io<__bf16>(g, resid_io != 0, out_io != 0, narrow, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mi355::fail(MI355_EHIP, "%s: kernel launch -> %s", who, hipGetErrorString(e));
    mi355::range_mark_entry_done();
    return MI355_OK;
}

extern "C" int mi355_linear16_res_fwd(const void* X16, const void* W16, const float* bias, const void* resid, int resid_io, void* Y, int out_io,
                                      int M, int N, int K, int ldx, int ldy, int act, int precision, mi355_stream_t stream) {
    return linear16_res_launch("mi355_linear16_res_fwd", X16, W16, bias, nullptr, resid, resid_io, Y, out_io, M, N, K, ldx, ldy, act, precision, stream);
}

// mi355_linear16_res_fwd with a LayerScale: Y = round_out( widen(resid) + gamma * act( X16 . W16^T + bias ) ); a null gamma is that entry
extern "C" int mi355_linear16_res_scale_fwd(const void* X16, const void* W16, const float* bias, const float* gamma, const void* resid, int resid_io,
                                            void* Y, int out_io, int M, int N, int K, int ldx, int ldy, int act, int precision,
                                            mi355_stream_t stream) {
    return linear16_res_launch("mi355_linear16_res_scale_fwd", X16, W16, bias, gamma, resid, resid_io, Y, out_io, M, N, K, ldx, ldy, act, precision,
                               stream);
}
