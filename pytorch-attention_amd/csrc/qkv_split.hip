// qkv_split.hip -- the qkv projection of ViT Attention (ViT.py:79) for precision 3 ("logit-compensated"), gfx950.
//
//   one launch:   [q | k | v] (M x 3C) = x (M x K, fp32) . W^T (3C x K) + bias
//
// The logit path and the value path of the attention block want different operand formats (profiles/logit_mode.md: the error that grows
// with the weight scale is made where x and W are rounded for the q / k columns, before q and k exist; the value path is scale-free):
//   column tiles below 2C (q, k):  x rows split into bf16 hi + lo in the staging registers, W pre-split on the host (hi, lo planes),
//                                  hi.hi + hi.lo + lo.hi through mma_step<0> (fp32-class product), result stored as a bf16 hi / lo PAIR;
//   column tiles from 2C up (v):   x rows rounded to fp16 in the staging registers, W as fp16, one fp16 MFMA per step, result stored as fp16
//                                  -- the bits of precision 1's cast16 + linear16 up to the summation order.
// Output layout (documented in include/mi355attn.h): five C-wide 16-bit planes per token row,
//   row m = [ q_hi (C) | q_lo (C) | k_hi (C) | k_lo (C) | v (C) ],   row stride 5C elements;   q = q_hi + q_lo, k = k_hi + k_lo.
// Tiling is gemm.hip's (128 x 128 x 32 per 256-thread workgroup, 2 x 2 waves of 64 x 64, two LDS buffers, one barrier per K-step, the
// next step's global loads in flight under the MFMAs, epilogue through a per-wave LDS slab); 2C is a multiple of 128 whenever C % 64 == 0,
// so a tile is entirely logit path or entirely value path and the choice is workgroup-uniform.
// fp16 range guard: the v tiles report what precision 1 reports -- the staged x values with code 1 (mi355_cast16_fwd's), the fp16 results
// with code 3 (a 16-bit GEMM epilogue's); bf16 is never flagged.
#include "common.h"
#include "mma.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int PITCH = BK + 8;                 // LDS row pitch in 16-bit elements (80 B, keeps 16-B alignment)
constexpr int EPITCH = 68;                    // epilogue slab pitch in floats
constexpr int PLANE = BM * PITCH;             // one operand plane of one buffer (A and B tiles have the same shape)

struct QkvSplitArgs {
    const float* x;                           // (M, K) fp32, row stride ldx
    const unsigned short* w_hi;               // (2C, K) bf16: hi part of the q and k rows of qkv.weight
    const unsigned short* w_lo;               // (2C, K) bf16: lo part
    const unsigned short* w_v;                // (C, K) fp16: the v rows
    const float* bias;                        // (3C) fp32 or null
    unsigned short* out;                      // (M, 5C)
    int M, C, K, ldx;
    unsigned* ovf;                            // fp16 range word or null
};

// V = false: logit-path tile (split-bf16 operands, NS = 2 planes); V = true: value-path tile (fp16 operands, one plane)
template <bool V>
__device__ __forceinline__ void qkv_tile(const QkvSplitArgs& g, unsigned char* lds_raw, int m0, int n0) {
    constexpr int PREC = V ? 1 : 0;
    using M_ = Mma<PREC>;
    using v8 = typename M_::v8;
    using v4 = typename M_::v4;
    constexpr int NS = M_::NSPLIT;
    constexpr int BUF = 2 * NS * PLANE;                      // elements per buffer: [A planes | B planes]
    unsigned short* lds = reinterpret_cast<unsigned short*>(lds_raw);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int N = 3 * g.C;

    // ---- staging coordinates: A as in gemm.hip (float4 of row lr + 32 i), B as 16-byte chunks of the 16-bit weight rows -------------
    const int lr = t >> 3, lk = (t & 7) * 4;
    const float* a_ptr[4];
    bool a_ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + lr + 32 * i;
        a_ok[i] = m < g.M;
        a_ptr[i] = g.x + (long)(a_ok[i] ? m : 0) * g.ldx + lk;
    }
    const int br = t >> 2, bk8 = (t & 3) * 8;                // weight row (of 64, + 64 j) and k offset of this thread's chunks
    const unsigned short* b_ptr[NS][2];
    bool b_ok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + br + 64 * j;
        b_ok[j] = n < N;
        const long row = b_ok[j] ? (V ? n - 2 * g.C : n) : 0;
        if constexpr (V) b_ptr[0][j] = g.w_v + row * g.K + bk8;
        else { b_ptr[0][j] = g.w_hi + row * g.K + bk8; b_ptr[NS - 1][j] = g.w_lo + row * g.K + bk8; }
    }

    f4 ra[4];
    v8 rb[NS][2];
    float rgin = 0.f, rgout = 0.f;
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = a_ok[i] ? *reinterpret_cast<const f4*>(a_ptr[i] + k0) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                v8 z;
#pragma unroll
                for (int e = 0; e < 8; ++e) z[e] = (typename M_::e)0.f;
                rb[s][j] = b_ok[j] ? *reinterpret_cast<const v8*>(b_ptr[s][j] + k0) : z;
            }
    };
    auto store_tile = [&](int buf) {
        unsigned short* sA = lds + buf * BUF;
        unsigned short* sB = sA + NS * PLANE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int off = (lr + 32 * i) * PITCH + lk;
            if constexpr (V) rgin = rg_absmax4(rgin, ra[i]);
            const v4 h = M_::cvt(ra[i]);
            *reinterpret_cast<v4*>(sA + off) = h;
            if constexpr (NS == 2) *reinterpret_cast<v4*>(sA + PLANE + off) = M_::cvt_lo(ra[i], h);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int j = 0; j < 2; ++j) *reinterpret_cast<v8*>(sB + s * PLANE + (br + 64 * j) * PITCH + bk8) = rb[s][j];
    };

    f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int nk = g.K / BK;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    const int frow = lane & 15, fk = (lane >> 4) * 8;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tile((kt + 1) * BK);           // next tile in flight under the MFMAs
        const unsigned short* sA = lds + buf * BUF + (wr * 64 + frow) * PITCH + fk;
        const unsigned short* sB = lds + buf * BUF + NS * PLANE + (wc * 64 + frow) * PITCH + fk;
        v8 fa[4][NS], fb[4][NS];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                fa[i][s] = *reinterpret_cast<const v8*>(sA + s * PLANE + i * 16 * PITCH);
                fb[i][s] = *reinterpret_cast<const v8*>(sB + s * PLANE + i * 16 * PITCH);
            }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mma_step<PREC>(fa[i], fb[j], acc[i][j]);
        if (kt + 1 < nk) store_tile(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: 2 passes of 32 rows per wave through a private LDS slab; + bias, then the hi / lo split (q, k) or fp16 (v) ------------
    float* slab = reinterpret_cast<float*>(lds_raw) + wave * 32 * EPITCH;
    const long ldo = 5L * g.C;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    slab[(ii * 16 + (lane >> 4) * 4 + r) * EPITCH + j * 16 + (lane & 15)] = acc[p * 2 + ii][j][r];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int rl = it * 4 + (lane >> 4), cl = (lane & 15) * 4;
            const int m = m0 + wr * 64 + p * 32 + rl, n = n0 + wc * 64 + cl;
            if (m >= g.M || n >= N) continue;                // N % 4 == 0: a quad is whole or absent
            f4 v = *reinterpret_cast<const f4*>(slab + rl * EPITCH + cl);
            if (g.bias) v = v + *reinterpret_cast<const f4*>(g.bias + n);
            unsigned short* orow = g.out + (long)m * ldo;
            if constexpr (V) {
                rgout = rg_absmax4(rgout, v);
                *reinterpret_cast<v4*>(orow + n + 2 * g.C) = M_::cvt(v);             // plane 4
            } else {
                const int hc = n < g.C ? n : n + g.C;                                  // q: planes 0 / 1, k: planes 2 / 3
                const v4 h = M_::cvt(v);
                *reinterpret_cast<v4*>(orow + hc) = h;
                *reinterpret_cast<v4*>(orow + hc + g.C) = M_::cvt_lo(v, h);
            }
        }
        __syncthreads();
    }
    if constexpr (V) {
        rg_report(rgin, g.ovf, 1u);
        rg_report(rgout, g.ovf, 3u);
    }
}

__global__ __launch_bounds__(256, 2) void qkv_split16_kernel(const QkvSplitArgs g) {
    constexpr int LDS_BYTES = 2 * 2 * 2 * PLANE * 2;        // two buffers x (A, B) x (hi, lo) planes; the epilogue slabs (34 KB) alias it
    static_assert(LDS_BYTES >= 4 * 32 * EPITCH * 4, "epilogue slabs must fit the staging area");
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    const int tiles_n = (3 * g.C + BN - 1) / BN;
    const int wg = xcd_contiguous_block();                   // n fastest: the x panel of a tile row meets in one L2
    const int m0 = (wg / tiles_n) * BM, n0 = (wg % tiles_n) * BN;
    if (n0 >= 2 * g.C) qkv_tile<true>(g, lds_raw, m0, n0);   // workgroup-uniform: 2C % 128 == 0
    else qkv_tile<false>(g, lds_raw, m0, n0);
}

}  // namespace

extern "C" int mi355_qkv_split16_fwd(const float* x, const void* w_hi, const void* w_lo, const void* w_v16, const float* bias,
                                     void* qkv5, int M, int C, int K, int ldx, mi355_stream_t stream) {
    MI355_CHECK_ARG(x && w_hi && w_lo && w_v16 && qkv5 && M > 0 && C > 0 && K > 0 && ldx >= K);
    if (C % 64 || K % 64) return mi355::fail(MI355_EUNSUPPORTED, "mi355_qkv_split16_fwd: C = %d, K = %d (built: C %% 64 == 0, K %% 64 == 0)", C, K);
    MI355_CHECK_ARG((ldx & 3) == 0 && aligned16(x) && aligned16(w_hi) && aligned16(w_lo) && aligned16(w_v16) && aligned16(qkv5) &&
                    (!bias || aligned16(bias)));
    const long tiles = (long)cdiv(M, BM) * cdiv(3L * C, BN);
    MI355_CHECK_ARG(tiles < (1L << 31));
    hipStream_t st = static_cast<hipStream_t>(stream);
    QkvSplitArgs g{x, static_cast<const unsigned short*>(w_hi), static_cast<const unsigned short*>(w_lo),
                   static_cast<const unsigned short*>(w_v16), bias, static_cast<unsigned short*>(qkv5), M, C, K, ldx, nullptr};
    g.ovf = mi355::range_word(st);                           // the v tiles convert to fp16: a producer
    {
        MI355_TRACE(st, "qkv_split16_kernel M=%d C=%d K=%d", M, C, K);
        qkv_split16_kernel<<<(int)tiles, 256, 0, st>>>(g);
    }
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}
