// gemm16_res.hip -- the 16-bit GEMM with a residual whose residual and / or result is 16-bit (mi355_linear16_res_fwd):
//
//   Y (M x N) = round_out( widen(resid) + act( X16 (M x K) . W16^T (N x K) + bias ) )      X16, W16: IEEE half (precision 1) or bfloat16 (2)
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
};

// (launch bounds: <= 128 registers for either tile -- four waves per SIMD, i.e. two 512-thread or four 256-thread workgroups per CU)
template <typename T, bool R16, bool O16, int BN, int WN>
__global__ __launch_bounds__(2 * WN * 64, WN == 2 ? 4 : 2) void gemm16_res_kernel(const ResArgs g) {
    using v8 = typename Vec8<T>::t;
    using v4 = typename Vec8<T>::t4;
    constexpr int BM = 128, WM = 2, NW = WM * WN;
    constexpr int TM = BM / WM, TN = BN / WN, MF = TM / 16, NF = TN / 16;
    constexpr int IA = BM / 8 / NW, IB = BN / 8 / NW;           // LDS-DMA instructions per wave per K-tile (8 rows of 128 B each)
    static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0 && TM == 64 && TN == 64, "tile/wave geometry");
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[(BM + BN) * BK * 2];
    T* lds = reinterpret_cast<T*>(lds_raw);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = wave / WN, wc = wave % WN;
    const int tiles_n = (g.N + BN - 1) / BN;
    const int wg = xcd_contiguous_block();                     // neighbouring tiles (one row of W tiles, then the next) share an L2
    const int m0 = (wg / tiles_n) * BM, n0 = (wg % tiles_n) * BN;
    const T* __restrict__ A = static_cast<const T*>(g.A);
    const T* __restrict__ B = static_cast<const T*>(g.B);

    // LDS-DMA sources: lane -> (row = lane >> 3, physical 16-byte chunk = lane & 7) holds logical chunk (lane & 7) ^ (row & 7)
    const int lrow = lane >> 3, pch = lane & 7;
    const int csw = (pch ^ lrow) * 8;
    const T* a_src[IA];
    const T* b_src[IB];
#pragma unroll
    for (int i = 0; i < IA; ++i) {
        int ma = m0 + (wave * IA + i) * 8 + lrow; if (ma >= g.M) ma = g.M - 1;   // clamp: tail rows are computed and discarded
        a_src[i] = A + (long)ma * g.lda + csw;
    }
#pragma unroll
    for (int i = 0; i < IB; ++i) {
        int nb = n0 + (wave * IB + i) * 8 + lrow; if (nb >= g.N) nb = g.N - 1;
        b_src[i] = B + (long)nb * g.K + csw;
    }
    T* sAw = lds + (wave * IA * 8) * BK;
    T* sBw = lds + BM * BK + (wave * IB * 8) * BK;

    f4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4, fsw = lane & 7;
    const T* sA = lds + (wr * TM + frow) * BK;
    const T* sB = lds + BM * BK + (wc * TN + frow) * BK;
    const int nk = g.K / BK;
    for (int kt = 0; kt < nk; ++kt) {
        const int k0 = kt * BK;
#pragma unroll
        for (int i = 0; i < IA; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[i] + k0),
                                             (__attribute__((address_space(3))) void*)(sAw + i * 8 * BK), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < IB; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_src[i] + k0),
                                             (__attribute__((address_space(3))) void*)(sBw + i * 8 * BK), 16, 0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int off = (((ks * 4 + fq) ^ fsw) * 8);
            v8 fa[MF], fb[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) fb[j] = *reinterpret_cast<const v8*>(sB + j * 16 * BK + off);
#pragma unroll
            for (int i = 0; i < MF; ++i) fa[i] = *reinterpret_cast<const v8*>(sA + i * 16 * BK + off);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j) acc[i][j] = mma16<T>(fb[j], fa[i], acc[i][j]);      // D^T = W . X^T: see the epilogue
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
    }

    // ---- epilogue straight from the accumulators: the MFMAs compute the TRANSPOSED 16 x 16 tiles, so lane (l15, g) holds output row
    //      m = i*16 + l15 and four CONSECUTIVE columns n = j*16 + g*4 + [0, 4) -- the pack of the residual row it needs and of the
    //      output row it writes.  All residual packs of a row tile are requested before the first is used.
    const int l15 = lane & 15, g4 = (lane >> 4) * 4;
    const float* Rf = static_cast<const float*>(g.resid);
    const T* Rh = static_cast<const T*>(g.resid);
    float* Cf = static_cast<float*>(g.C);
    T* Ch = static_cast<T*>(g.C);
    float rgmax = 0.f;
    f4 bias4[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int n = n0 + wc * TN + j * 16 + g4;
        bias4[j] = (g.bias && n < g.N) ? *reinterpret_cast<const f4*>(g.bias + n) : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        const int m = m0 + wr * TM + i * 16 + l15;
        if (m >= g.M) continue;
        const long ro = (long)m * g.ldc;
        f4 r[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const int n = n0 + wc * TN + j * 16 + g4;
            if (n >= g.N) { r[j] = f4{0.f, 0.f, 0.f, 0.f}; continue; }           // N % 8 == 0: a pack of four is in or out
            if constexpr (R16) {
                const v4 h = *reinterpret_cast<const v4*>(Rh + ro + n);
                r[j] = f4{(float)h.x, (float)h.y, (float)h.z, (float)h.w};
            } else {
                r[j] = *reinterpret_cast<const f4*>(Rf + ro + n);
            }
        }
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const int n = n0 + wc * TN + j * 16 + g4;
            if (n >= g.N) continue;
            f4 v = acc[i][j] + bias4[j];
            if (g.act == MI355_ACT_GELU) v = gelu_fast4(v);     // the fp32 form also in front of a 16-bit store: the sum is what is rounded
            v = v + r[j];
            if constexpr (O16) {
                if constexpr (std::is_same<T, _Float16>::value) rgmax = rg_absmax4(rgmax, v);
                *reinterpret_cast<v4*>(Ch + ro + n) = v4{(T)v.x, (T)v.y, (T)v.z, (T)v.w};
            } else {
                *reinterpret_cast<f4*>(Cf + ro + n) = v;
            }
        }
    }
    if constexpr (O16 && std::is_same<T, _Float16>::value) rg_report(rgmax, g.ovf, 3u);
}

template <typename T, bool R16, bool O16>
void launch_res(const ResArgs& g, bool narrow, hipStream_t st) {
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

extern "C" int mi355_linear16_res_fwd(const void* X16, const void* W16, const float* bias, const void* resid, int resid_io, void* Y, int out_io,
                                      int M, int N, int K, int ldx, int ldy, int act, int precision, mi355_stream_t stream) {
    MI355_CHECK_ARG(X16 && W16 && resid && Y && M > 0 && N > 0 && K > 0 && ldx >= K && ldy >= N);
    MI355_CHECK_ARG(act == MI355_ACT_NONE || act == MI355_ACT_GELU);
    MI355_CHECK_ARG(precision == MI355_PREC_FP16 || precision == MI355_PREC_BF16);
    MI355_CHECK_ARG((resid_io == 0 || resid_io == precision) && (out_io == 0 || out_io == precision));
    if (resid_io == 0 && out_io == 0)
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_linear16_res_fwd: an fp32 residual with an fp32 result is mi355_linear16_ws_fwd's");
    if ((K % BK) || (N & 7) || (ldx & 7) || (ldy & 7) || !aligned16(X16) || !aligned16(W16) || !aligned16(Y) || !aligned16(resid) ||
        (bias && !aligned16(bias)) || (long)cdiv(M, 128) * cdiv(N, 128) >= (1L << 31))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_linear16_res_fwd: needs K %% 64 == 0, N %% 8 == 0, 16-byte aligned rows (K=%d N=%d ldx=%d ldy=%d)",
                           K, N, ldx, ldy);
    hipStream_t st = static_cast<hipStream_t>(stream);
    ResArgs g{};
    g.A = X16; g.B = W16; g.bias = bias; g.resid = resid; g.C = Y;
    g.M = M; g.N = N; g.K = K; g.lda = ldx; g.ldc = ldy; g.act = act;
    if (out_io == MI355_PREC_FP16) g.ovf = mi355::range_word(st);              // fp16 range guard, like every 16-bit GEMM epilogue
    // 128 x 256 tiles where they give every CU one, else 128 x 128 (the engine's rule for its plain tile kernel)
    const bool narrow = N <= 128 || (long)cdiv(M, 128) * cdiv(N, 256) < mi355::resident_slots(1);
    MI355_TRACE(st, "gemm16_res_kernel<%s,%s,%s> M=%d N=%d K=%d%s", precision == MI355_PREC_FP16 ? "f16" : "bf16", resid_io ? "r16" : "r32",
                out_io ? "o16" : "o32", M, N, K, act == MI355_ACT_GELU ? " gelu" : "");
    if (precision == MI355_PREC_FP16) launch_res_io<_Float16>(g, resid_io != 0, out_io != 0, narrow, st);
    else                              launch_res_io<__bf16>(g, resid_io != 0, out_io != 0, narrow, st);
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}
