// xcit.hip -- XCiT cross-covariance attention core (XCA) and the LPI depth-wise stencil block for gfx950.
//
// XCA (xcit.py:249-262): per (image, head) the attention matrix is only d x d (48 x 48 for XCiT-S); one workgroup streams
// the head's tokens through LDS in chunks of 64 (any token count) and the arithmetic is done in
// EXACT fp32 on the matrix cores (v_mfma_f32_16x16x4_f32: bitwise an fmaf chain, cdna_hip_programming.md section 3) --
// no operand rounding, hence the `precision` argument does not change the result:
//     G = Q^T K (d x d, contraction over tokens)   ->  G_ij / (max(|q_i|,eps) max(|k_j|,eps)) * temperature_h
//     A = softmax_rows(G)                          ->  O = A V^T (d x N)  ->  out[b, n, h*d + i] = O[i][n]
// HBM traffic = read the head's q,k,v once + write out once.
//
// LPI (xcit.py:149-157): tokens -> (C,H,W) image -> dw3x3 -> GELU -> BatchNorm(eval) -> dw3x3 -> tokens, fused in one
// kernel per (image, 32-channel group): the token tile and the intermediate sit in LDS, a lane owns 4 channels (16-byte LDS
// and HBM accesses, 128-byte row pieces per token); LayerScale + residual fused.  Token grids above 16 x 16 (patch 8 at 224 px, patch 16
// at 384 px) run the same block per (image, tile of the grid, 32-channel group) with a 2-cell halo: lpi_tile_kernel.
#include <type_traits>
#include "common.h"
#include "mma.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// XCA core, streaming over tokens in chunks of 64: LDS holds one q/k (then v) chunk + the d x d matrix, so 4 workgroups fit a
// CU (latency hiding comes from the neighbours) and the token count is unbounded.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int XCA_TC = 64;      // tokens per chunk

// OT: output element type (float, or the 16-bit operand type of the proj GEMM that follows: saves the cast pass over ctx);
// IT: element type of qkv (float, or the 16-bit output of the qkv GEMM: halves the 3C-wide tensor the core streams twice).
// Round 4 (the kernel sat at 82 us for three rounds; its busiest wave issued 336 exact-fp32 MFMAs of 32 cycles per (image, head)):
//   * phase 1 is split along the TOKENS: wave w owns tokens 16 w .. 16 w + 15 of a chunk and accumulates all DT x DT tiles of
//     G = Q^T K for them -- balanced (the tile-per-wave form left 9 tiles on 4 waves as 3 / 2 / 2 / 2), every q / k value is read
//     from LDS once per row tile instead of once per tile pair, the squared column norms ride on the very values that feed the
//     MFMAs, and 16-token slices beyond N are skipped (N = 196: 13 slices instead of 16).  The four partial sums are added in a
//     fixed order (waves 0 + 3, then 1, then 2), so results stay bit-identical run to run;
//   * phase 3 with 16-bit I/O (PV16): O = A V^T on the 16-bit matrix pipe -- A in [0, 1] rounded to the operand type (relative
//     2^-11, the rounding v already carries), the V fragments come straight from global memory in operand layout (a lane's 8
//     consecutive channels of one token = 16 bytes), no LDS staging and no barriers.  G, the norms and the softmax stay exact fp32;
//     with fp32 I/O (strict mode) phase 3 stays on the exact-fp32 MFMA as well.
template <int D, typename OT = float, typename IT = float>
__global__ __launch_bounds__(256, D <= 48 ? 4 : 2) void xca_kernel(const IT* __restrict__ qkv, const float* __restrict__ temperature,
                                                 OT* __restrict__ out, int N, int heads) {
    constexpr bool PV16 = !std::is_same<IT, float>::value && std::is_same<OT, IT>::value;
    constexpr int P = D + 1;                 // LDS pitch (floats): odd -> conflict-free column walks
    constexpr int DT = D / 16, D4 = D / 4;
    constexpr int NLD = (XCA_TC * D4 + 255) / 256;          // float4 loads per thread per array per chunk
    constexpr int GD = D * D;                               // a dense partial G
    __shared__ __attribute__((aligned(16))) float s_ab[2 * XCA_TC * P];   // q | k chunk (fp32 path: later the v chunk); after phase 1: two dense partial Gs
    __shared__ __attribute__((aligned(16))) float s_g[D * P];             // G partial of waves 0 + 3, then A = softmax(G) (PV16: as a 16-bit image, pitch AP)
    __shared__ float s_nw[4][2 * D];         // per-wave squared column norms of q and k
    __shared__ float s_n[2 * D];             // the norms
    static_assert(2 * GD <= 2 * XCA_TC * P, "two dense partials must fit the chunk buffers");
    float* s_a = s_ab;
    float* s_b = s_ab + XCA_TC * P;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, g = lane >> 4;
    const int lid = xcd_contiguous_block();                 // the heads of an image read adjacent column blocks of the same rows
    const int h = lid % heads, b = lid / heads;
    const int C = heads * D;
    const long row3 = 3L * C;
    const IT* base = qkv + (long)b * N * row3 + h * D;
    typedef IT i4 __attribute__((ext_vector_type(4)));
    auto ld4 = [&](const IT* p) { const i4 v = *reinterpret_cast<const i4*>(p); return f4{(float)v.x, (float)v.y, (float)v.z, (float)v.w}; };
    const int nchunks = (N + XCA_TC - 1) / XCA_TC;

    auto stage = [&](int chunk, int which_a, int which_b, bool two) {     // which_*: 0 = q, 1 = k, 2 = v
        f4 ra[NLD], rb[NLD];
#pragma unroll
        for (int it = 0; it < NLD; ++it) {
            const int idx = t + it * 256, nl = idx / D4, d4 = idx % D4, n = chunk * XCA_TC + nl;
            ra[it] = f4{0.f, 0.f, 0.f, 0.f};
            rb[it] = f4{0.f, 0.f, 0.f, 0.f};
            if (idx < XCA_TC * D4 && n < N) {
                ra[it] = ld4(base + (long)n * row3 + which_a * C + d4 * 4);
                if (two) rb[it] = ld4(base + (long)n * row3 + which_b * C + d4 * 4);
            }
        }
#pragma unroll
        for (int it = 0; it < NLD; ++it) {
            const int idx = t + it * 256, nl = idx / D4, d4 = idx % D4;
            if (idx < XCA_TC * D4) {
                float* pa = s_a + nl * P + d4 * 4;
                pa[0] = ra[it].x; pa[1] = ra[it].y; pa[2] = ra[it].z; pa[3] = ra[it].w;
                if (two) {
                    float* pb = s_b + nl * P + d4 * 4;
                    pb[0] = rb[it].x; pb[1] = rb[it].y; pb[2] = rb[it].z; pb[3] = rb[it].w;
                }
            }
        }
    };

    // ---- phase 1: G = Q^T K and the squared column norms; wave w owns tokens 16 w .. 16 w + 15 of every chunk -------------------
    f4 gacc[DT][DT];
    float nq[DT], nk[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) {
        nq[i] = nk[i] = 0.f;
#pragma unroll
        for (int j = 0; j < DT; ++j) gacc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    }
    for (int ch = 0; ch < nchunks; ++ch) {
        stage(ch, 0, 1, true);
        __syncthreads();
        if (ch * XCA_TC + wave * 16 < N) {                  // wave-uniform: slices beyond N hold only zero rows
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int row = wave * 16 + ks * 4 + g;
                float av[DT], bv[DT];
#pragma unroll
                for (int i = 0; i < DT; ++i) {
                    av[i] = s_a[row * P + i * 16 + l15];
                    bv[i] = s_b[row * P + i * 16 + l15];
                    nq[i] += av[i] * av[i];
                    nk[i] += bv[i] * bv[i];
                }
#pragma unroll
                for (int i = 0; i < DT; ++i)
#pragma unroll
                    for (int j = 0; j < DT; ++j) gacc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], gacc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // column norms: a lane saw the tokens of its quarter g; quarters, then waves, are added in a fixed order
#pragma unroll
    for (int i = 0; i < DT; ++i) {
        nq[i] += __shfl_xor(nq[i], 16, WAVE);
        nq[i] += __shfl_xor(nq[i], 32, WAVE);
        nk[i] += __shfl_xor(nk[i], 16, WAVE);
        nk[i] += __shfl_xor(nk[i], 32, WAVE);
        if (g == 0) {
            s_nw[wave][i * 16 + l15] = nq[i];
            s_nw[wave][D + i * 16 + l15] = nk[i];
        }
    }
    // partial Gs: wave 0 -> s_g, waves 1 / 2 -> the two dense buffers over the (now free) chunk area, wave 3 is added to s_g afterwards
    {
        float* dst = wave == 1 ? s_ab : s_ab + GD;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int j = 0; j < DT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int gi = i * 16 + g * 4 + r, gj = j * 16 + l15;
                    if (wave == 0) s_g[gi * P + gj] = gacc[i][j][r];
                    else if (wave != 3) dst[gi * D + gj] = gacc[i][j][r];
                }
    }
    __syncthreads();
    if (wave == 3) {
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int j = 0; j < DT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) s_g[(i * 16 + g * 4 + r) * P + j * 16 + l15] += gacc[i][j][r];
    }
    if (t < 2 * D) s_n[t] = fmaxf(sqrtf(((s_nw[0][t] + s_nw[1][t]) + s_nw[2][t]) + s_nw[3][t]), 1e-12f);     // F.normalize: x / max(||x||, 1e-12)
    __syncthreads();
    // ---- phase 2: A = softmax_rows(G / (|q_i| |k_j|) * temperature): 16 lanes per row; rows stay in registers until every thread has
    //      read the partial sums, then A replaces G (PV16: as the 16-bit operand image) ------------------------------------------
    constexpr int KSA = (D + 31) / 32;       // 16x16x32 steps over j
    constexpr int AP = KSA * 32 + 8;         // pitch (elements) of the 16-bit A image: KSA * 32 k columns (D .. zero) + 8 of padding
    constexpr int RPT = (D + 15) / 16;       // rows per thread
    {
        const float temp = temperature[h];
        const int tj = t & 15;
        float pv[RPT][DT];
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
            const int i = (t >> 4) + 16 * rr;
            float m = -INFINITY;
#pragma unroll
            for (int c = 0; c < DT; ++c) {
                const int j = tj + 16 * c;
                const float gij = i < D ? (s_g[i * P + j] + s_ab[i * D + j]) + s_ab[GD + i * D + j] : 0.f;
                pv[rr][c] = i < D ? gij / (s_n[i] * s_n[D + j]) * temp : 0.f;
                m = fmaxf(m, pv[rr][c]);
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < DT; ++c) { pv[rr][c] = expf(pv[rr][c] - m); sum += pv[rr][c]; }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, WAVE);
#pragma unroll
            for (int c = 0; c < DT; ++c) pv[rr][c] = pv[rr][c] / sum;
        }
        __syncthreads();
        if constexpr (PV16) {
            IT* a16 = reinterpret_cast<IT*>(s_g);
            static_assert(D * AP * 2 <= D * P * 4, "the 16-bit A image must fit the G buffer");
#pragma unroll
            for (int rr = 0; rr < RPT; ++rr) {
                const int i = (t >> 4) + 16 * rr;
                if (i < D) {
#pragma unroll
                    for (int c = 0; c < 2 * KSA; ++c) a16[i * AP + tj + 16 * c] = c < DT ? (IT)pv[rr][c < DT ? c : 0] : (IT)0.f;
                }
            }
        } else {
#pragma unroll
            for (int rr = 0; rr < RPT; ++rr) {
                const int i = (t >> 4) + 16 * rr;
                if (i < D) {
#pragma unroll
                    for (int c = 0; c < DT; ++c) s_g[i * P + tj + 16 * c] = pv[rr][c];
                }
            }
        }
    }
    __syncthreads();
    // ---- phase 3: O[i][n] = sum_j A[i][j] v[n][j]; lane holds 4 consecutive i of one token -> 8 / 16-byte stores -----------------
    if constexpr (PV16) {
        typedef IT v8 __attribute__((ext_vector_type(8)));
        typedef OT o4 __attribute__((ext_vector_type(4)));
        constexpr int KS = KSA;
        const IT* a16 = reinterpret_cast<const IT*>(s_g);
        v8 af[DT][KS];
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) af[i][kk] = *reinterpret_cast<const v8*>(a16 + (i * 16 + l15) * AP + kk * 32 + g * 8);
        const int ntiles = (N + 15) >> 4;
        for (int nt = wave; nt < ntiles; nt += 4) {
            const int n = nt * 16 + l15;
            v8 bf[KS];
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                bf[kk] = v8{};
                if (n < N && kk * 32 + g * 8 < D) bf[kk] = *reinterpret_cast<const v8*>(base + (long)n * row3 + 2 * C + kk * 32 + g * 8);
            }
#pragma unroll
            for (int i = 0; i < DT; ++i) {
                f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {
                    if constexpr (std::is_same<IT, _Float16>::value) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][kk], bf[kk], acc, 0, 0, 0);
                    else acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][kk], bf[kk], acc, 0, 0, 0);
                }
                if (n < N) *reinterpret_cast<o4*>(out + ((long)b * N + n) * C + h * D + i * 16 + g * 4) = o4{(OT)acc.x, (OT)acc.y, (OT)acc.z, (OT)acc.w};
            }
        }
    } else {
        for (int ch = 0; ch < nchunks; ++ch) {
            stage(ch, 2, 2, false);
            __syncthreads();
            for (int tl = wave; tl < DT * (XCA_TC / 16); tl += 4) {
                const int it = tl % DT, nt = tl / DT;
                if (ch * XCA_TC + nt * 16 >= N) continue;   // wave-uniform: token tiles beyond N
                f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < D / 4; ++ks) {
                    const float av = s_g[(it * 16 + l15) * P + ks * 4 + g];
                    const float bv = s_a[(nt * 16 + l15) * P + ks * 4 + g];
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
                }
                const int n = ch * XCA_TC + nt * 16 + l15;
                if (n < N) {
                    typedef OT o4 __attribute__((ext_vector_type(4)));
                    *reinterpret_cast<o4*>(out + ((long)b * N + n) * C + h * D + it * 16 + g * 4) = o4{(OT)acc.x, (OT)acc.y, (OT)acc.z, (OT)acc.w};
                }
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// XCA core for 16-bit q / k / v and N <= 224 tokens (XCiT at 224 px: 14 x 14 = 196), round 6.  The streaming kernel above spends its
// phase 1 on 468 exact-fp32 MFMAs of 32 cycles per (image, head) over fp32 copies of q / k that it parks in LDS chunk by chunk (four
// stage-barrier-compute-barrier rounds): 58 us for 153 MB.  When q and k ARRIVE in the 16-bit operand format (the output of the qkv
// GEMM), their products are exact in fp32 anyway (11-bit x 11-bit significands), so G = Q^T K runs on the 16-bit matrix pipe with fp32
// accumulation -- 63 MFMAs of 16 cycles -- and loses nothing that the inputs still carry:
//   * ONE stage: the head's q and k go to LDS transposed ([channel][token], zero beyond N) through a 4-token x 8-channel register
//     transpose (eight 8-byte writes per four 16-byte loads), one barrier;
//   * G tiles are dealt to the waves whole (full token range each: no partial sums, no reduction order to fix), the squared column
//     norms are summed from the same LDS image in token order;
//   * G, then the 16-bit image of A = softmax(G), overwrite the q / k area; phase 2 (norms, temperature, row softmax in fp32) and phase 3
//     (O = A V^T with V fragments straight from global memory -- requested at kernel start, beside q and k) are those of xca_kernel.
// 44.5 KB of LDS per workgroup at d = 48: three workgroups per CU.
// ---------------------------------------------------------------------------------------------------------------------------
template <int D, typename T>
__global__ __launch_bounds__(256, D <= 48 ? 3 : 2) void xca_tr_kernel(const T* __restrict__ qkv, const float* __restrict__ temperature, T* __restrict__ out,
                                                        int N, int heads) {
    typedef T v8 __attribute__((ext_vector_type(8)));
    typedef T v4 __attribute__((ext_vector_type(4)));
    constexpr int NMAX = 224, TP = NMAX + 8;          // token pitch of the transposed images (elements)
    constexpr int DT = D / 16, D8 = D / 8, P = D + 1;
    constexpr int KSA = (D + 31) / 32, AP = KSA * 32 + 8, RPT = (D + 15) / 16;
    constexpr int UNITS = (NMAX / 4) * D8;            // (4 tokens x 8 channels) units per array
    __shared__ __attribute__((aligned(16))) unsigned short s_t[2 * D * TP];    // q^T | k^T; later G (fp32, pitch P), then the 16-bit image of A
    __shared__ float s_n[2 * D];
    static_assert(D * P * 4 <= 2 * D * TP * 2 && D * AP * 2 <= D * P * 4, "G and the A image fit the q / k area");
    T* s_q = reinterpret_cast<T*>(s_t);
    T* s_k = s_q + D * TP;
    float* s_g = reinterpret_cast<float*>(s_t);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, g = lane >> 4;
    const int lid = xcd_contiguous_block();
    const int h = lid % heads, b = lid / heads;
    const int C = heads * D;
    const long row3 = 3L * C;
    const T* base = qkv + (long)b * N * row3 + h * D;
    // ---- everything the workgroup needs from HBM is requested up front: q and k (to be transposed into LDS), and this wave's V fragments
    //      of phase 3 (token tiles wave, wave + 4, ...: at most four of the fourteen), which wait in registers until A exists ------------------
    constexpr int UPT = (2 * UNITS + 255) / 256;       // (4 tokens x 8 channels) units per thread
    v8 r[UPT][4];
#pragma unroll
    for (int it = 0; it < UPT; ++it) {
        const int u = t + it * 256;
        const int arr = u >= UNITS, uu = u - arr * UNITS, tg = uu / D8, cg = uu % D8;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = tg * 4 + j;
            r[it][j] = v8{};
            if (u < 2 * UNITS && n < N) r[it][j] = *reinterpret_cast<const v8*>(base + (long)n * row3 + arr * C + cg * 8);
        }
    }
    constexpr int VT = (NMAX / 16 + 3) / 4;            // token tiles of phase 3 per wave
    v8 vfr[VT][KSA];
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        const int n = (wave + 4 * i) * 16 + l15;
#pragma unroll
        for (int kk = 0; kk < KSA; ++kk) {
            vfr[i][kk] = v8{};
            if (n < N && kk * 32 + g * 8 < D) vfr[i][kk] = *reinterpret_cast<const v8*>(base + (long)n * row3 + 2 * C + kk * 32 + g * 8);
        }
    }
#pragma unroll
    for (int it = 0; it < UPT; ++it) {
        const int u = t + it * 256;
        if (u < 2 * UNITS) {
            const int arr = u >= UNITS, uu = u - arr * UNITS, tg = uu / D8, cg = uu % D8;
            T* dst = (arr ? s_k : s_q) + (cg * 8) * TP + tg * 4;
#pragma unroll
            for (int q = 0; q < 8; ++q) *reinterpret_cast<v4*>(dst + q * TP) = v4{r[it][0][q], r[it][1][q], r[it][2][q], r[it][3][q]};
        }
    }
    __syncthreads();
    // ---- squared column norms (token order) and G = Q^T K on the 16-bit pipe ------------------------------------------------------------
    const int nks = (N + 31) >> 5;
    float nrm = 0.f;
    if (t < 2 * D) {
        const T* col = s_q + t * TP;                   // rows 0 .. D-1 are q^T, D .. 2D-1 are k^T (s_k = s_q + D * TP)
        for (int c = 0; c < nks * 4; ++c) {
            const v8 v = *reinterpret_cast<const v8*>(col + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) nrm = __builtin_fmaf((float)v[e], (float)v[e], nrm);
        }
    }
    constexpr int NTILE = DT * DT, TPW = (NTILE + 3) / 4;
    f4 gacc[TPW];
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
        gacc[k] = f4{0.f, 0.f, 0.f, 0.f};
        const int tile = wave + 4 * k;
        if (tile < NTILE) {
            const int i = tile / DT, j = tile % DT;
            for (int ks = 0; ks < nks; ++ks) {
                const v8 af = *reinterpret_cast<const v8*>(s_q + (i * 16 + l15) * TP + ks * 32 + g * 8);
                const v8 bf = *reinterpret_cast<const v8*>(s_k + (j * 16 + l15) * TP + ks * 32 + g * 8);
                if constexpr (std::is_same<T, _Float16>::value) gacc[k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, gacc[k], 0, 0, 0);
                else gacc[k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, gacc[k], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                   // everybody is done reading q^T / k^T
    if (t < 2 * D) s_n[t] = fmaxf(sqrtf(nrm), 1e-12f);                 // F.normalize: x / max(||x||, 1e-12)
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
        const int tile = wave + 4 * k;
        if (tile < NTILE) {
            const int i = tile / DT, j = tile % DT;
#pragma unroll
            for (int r = 0; r < 4; ++r) s_g[(i * 16 + g * 4 + r) * P + j * 16 + l15] = gacc[k][r];
        }
    }
    __syncthreads();
    // ---- phase 2: A = softmax_rows(G / (|q_i| |k_j|) * temperature), 16 lanes per row (xca_kernel) ----------------------------------------
    {
        const float temp = temperature[h];
        const int tj = t & 15;
        float pv[RPT][DT];
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
            const int i = (t >> 4) + 16 * rr;
            float m = -INFINITY;
#pragma unroll
            for (int c = 0; c < DT; ++c) {
                const int j = tj + 16 * c;
                pv[rr][c] = i < D ? s_g[i * P + j] / (s_n[i] * s_n[D + j]) * temp : 0.f;
                m = fmaxf(m, pv[rr][c]);
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < DT; ++c) { pv[rr][c] = expf(pv[rr][c] - m); sum += pv[rr][c]; }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, WAVE);
#pragma unroll
            for (int c = 0; c < DT; ++c) pv[rr][c] = pv[rr][c] / sum;
        }
        __syncthreads();
        T* a16 = reinterpret_cast<T*>(s_t);
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
            const int i = (t >> 4) + 16 * rr;
            if (i < D) {
#pragma unroll
                for (int c = 0; c < 2 * KSA; ++c) a16[i * AP + tj + 16 * c] = c < DT ? (T)pv[rr][c < DT ? c : 0] : (T)0.f;
            }
        }
    }
    __syncthreads();
    // ---- phase 3: O[i][n] = sum_j A[i][j] v[n][j] on the 16-bit pipe, V fragments straight from global memory (xca_kernel, PV16) -----------
    {
        const T* a16 = reinterpret_cast<const T*>(s_t);
        v8 af[DT][KSA];
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int kk = 0; kk < KSA; ++kk) af[i][kk] = *reinterpret_cast<const v8*>(a16 + (i * 16 + l15) * AP + kk * 32 + g * 8);
#pragma unroll
        for (int vi = 0; vi < VT; ++vi) {
            const int n = (wave + 4 * vi) * 16 + l15;
#pragma unroll
            for (int i = 0; i < DT; ++i) {
                f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KSA; ++kk) {
                    if constexpr (std::is_same<T, _Float16>::value) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][kk], vfr[vi][kk], acc, 0, 0, 0);
                    else acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][kk], vfr[vi][kk], acc, 0, 0, 0);
                }
                if (n < N) *reinterpret_cast<v4*>(out + ((long)b * N + n) * C + h * D + i * 16 + g * 4) = v4{(T)acc.x, (T)acc.y, (T)acc.z, (T)acc.w};
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// XCA core at a RUN-TIME head width, 1 <= d <= 256: every width the templates above are not built for (they keep 32 / 48 / 64).
// Zero-padding d onto a built width is wrong here -- the softmax runs over the d channels of a head, a padded column has logit 0 and
// would take exp(0 - max) of every row -- so this kernel masks.
//   * Rows of the d x d matrix are independent: workgroup = (image, head, block of RB rows of G).  It streams the tokens through LDS in
//     chunks of TC: its RB channels of q and all d channels of k; forms its RB x d slab of G, its q norms and ALL k norms (recomputed per
//     row block: TC reads per column and chunk); masked row softmax; then streams v and writes its RB channels of every token.
//   * d is padded to dp = the next multiple of 16 in LDS only: channels >= d and tokens >= N are staged as zeros, softmax columns >= d
//     never enter the maximum or the sum and end up as A = 0, rows >= d are never stored; nothing outside [h d, h d + d) of a token's
//     row is written.
//   * One arithmetic for the three type modes (fp32 -> fp32, fp32 -> 16 bit, 16 bit -> same): widened at the load (exact), ONE rounding
//     at the store, everything between in fp32 -- G and A V^T on the exact-fp32 MFMA, as in xca_kernel, so `precision` changes nothing.
//   * (16 x 16) tiles of the slab are dealt to the waves whole (full token range each, wave w owns tiles w, w + waves, ...: at most 8),
//     the column norms are summed in token order by one thread per column: no partial sums, no atomics, nothing between workgroups --
//     run-to-run bit-identical and safe under graph capture.  RB, TC and the workgroup size are functions of d alone
//     (xca_any_geom), so an image's bits do not depend on its batch.
//   * 16-byte global accesses where d allows them (d % 4 == 0 for fp32, d % 8 == 0 for 16-bit elements: every head then starts on a
//     16-byte boundary of the 16-byte aligned tensors), element-wise otherwise.
//   * LDS is dynamic and sized by d (odd pitches): 10 KB at d = 16, 50 KB at 64, 59 KB at 128, 70 KB at 256 (two workgroups per CU).
// The fp32-in / 16-bit-out mode does not report its fp16 conversion to the range guard: the known gap of xca_kernel's same mode.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int XCA_ANY_MAX = 256;      // widest head
constexpr int XCA_ANY_UNITS = 8;      // (16 x 16) tiles of G per wave: (RB / 16) * (dp / 16) <= 4 * this

struct XcaAnyGeom { int RB, TC, threads, nrb; size_t lds; };
static XcaAnyGeom xca_any_geom(int d) {
    XcaAnyGeom g;
    const int dp = (d + 15) & ~15;
    g.RB = dp <= 64 ? dp : 32;                 // whole heads up to 64 (k is streamed once), 32-row blocks above
    g.TC = dp <= 128 ? 64 : 32;
    const int units = (g.RB / 16) * (dp / 16);
    g.threads = 64 * (units < 4 ? units : 4);
    g.nrb = (dp + g.RB - 1) / g.RB;
    g.lds = ((size_t)g.RB * (dp + 1) + (size_t)g.TC * (dp + 1) + (size_t)g.TC * (g.RB + 1) + dp + g.RB) * sizeof(float);
    return g;
}

// `width` channels from channel c0 on (a multiple of 16) of the tokens n0 .. n0 + tc - 1 -> dst[token][channel] (pitch floats), zeros for
// channels >= d and tokens >= N.  VW elements per load; (token, channel group) advances by the workgroup size without a division.
template <int VW, typename IT>
__device__ __forceinline__ void xca_any_stage(const IT* __restrict__ src, long row3, float* __restrict__ dst, int pitch, int c0, int width,
                                              int d, int n0, int tc, int N, int t, int nthr) {
    const int wv = width / VW, total = tc * wv;
    const int qs = nthr / wv, rs = nthr - qs * wv;
    int nl = t / wv, cv = t - nl * wv;
#pragma unroll 4
    for (int idx = t; idx < total; idx += nthr) {
        const int c = c0 + cv * VW, n = n0 + nl;
        float v[VW];
#pragma unroll
        for (int e = 0; e < VW; ++e) v[e] = 0.f;
        if (n < N && c < d) {
            const IT* p = src + (long)n * row3 + c;
            if constexpr (VW == 1) v[0] = (float)p[0];
            else {
                typedef IT iv __attribute__((ext_vector_type(VW)));
                const iv r = *reinterpret_cast<const iv*>(p);
#pragma unroll
                for (int e = 0; e < VW; ++e) v[e] = (float)r[e];
            }
        }
        float* q = dst + nl * pitch + cv * VW;
#pragma unroll
        for (int e = 0; e < VW; ++e) q[e] = v[e];
        nl += qs;
        cv += rs;
        if (cv >= wv) { cv -= wv; ++nl; }
    }
}

template <typename OT, typename IT>
__global__ __launch_bounds__(256) void xca_any_kernel(const IT* __restrict__ qkv, const float* __restrict__ temperature, OT* __restrict__ out,
                                                      int N, int heads, int d, int RB, int TC, int vec_in, int vec_out) {
    extern __shared__ __attribute__((aligned(16))) float xa_smem[];
    constexpr int VWI = 16 / (int)sizeof(IT);
    const int dp = (d + 15) & ~15, DT = dp >> 4, PG = dp + 1, PQ = RB + 1;
    const int nrb = (dp + RB - 1) / RB;
    float* s_g = xa_smem;               // [RB][PG]: the slab of G, then of A = softmax(G)
    float* s_k = s_g + RB * PG;         // [TC][PG]: k chunk, later the v chunk
    float* s_q = s_k + TC * PG;         // [TC][PQ]: the block's channels of the q chunk
    float* s_n = s_q + TC * PQ;         // [dp] k norms | [RB] q norms
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), l15 = lane & 15, g = lane >> 4;
    const int nthr = blockDim.x, nw = nthr >> 6;
    const int lid = xcd_contiguous_block();                 // the row blocks of a head, then the heads of an image, read the same rows
    const int rb = lid % nrb, hb = lid / nrb, h = hb % heads, b = hb / heads;
    const int r0 = rb * RB, rt = min(RB, dp - r0) >> 4;     // first row, row tiles of this block
    const int nunits = rt * DT;
    const int C = heads * d;
    const long row3 = 3L * C;
    const IT* base = qkv + (long)b * N * row3 + h * d;
    const int nchunks = (N + TC - 1) / TC;
    auto stage = [&](const IT* src, float* dst, int pitch, int c0, int width, int n0) {
        if (vec_in) xca_any_stage<VWI>(src, row3, dst, pitch, c0, width, d, n0, TC, N, t, nthr);
        else        xca_any_stage<1>(src, row3, dst, pitch, c0, width, d, n0, TC, N, t, nthr);
    };

    // ---- phase 1: the slab of G = Q^T K and the squared column norms ---------------------------------------------------------------
    f4 gacc[XCA_ANY_UNITS];
    int offa[XCA_ANY_UNITS], offb[XCA_ANY_UNITS];
#pragma unroll
    for (int s = 0; s < XCA_ANY_UNITS; ++s) {
        const int u = wave + nw * s, ui = u / DT, uj = u - ui * DT;
        gacc[s] = f4{0.f, 0.f, 0.f, 0.f};
        offa[s] = ui * 16 + l15;
        offb[s] = uj * 16 + l15;
    }
    float nrm0 = 0.f, nrm1 = 0.f;       // columns t and t + nthr of (k | q): dp + RB <= 2 nthr
    const int ncol = dp + RB;
    const float* col0 = t < dp ? s_k + t : s_q + (t - dp);
    const int cp0 = t < dp ? PG : PQ;
    const int t1 = t + nthr;
    const float* col1 = t1 < dp ? s_k + t1 : s_q + (t1 - dp);
    const int cp1 = t1 < dp ? PG : PQ;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int n0 = ch * TC, nv = min(TC, N - n0);
        stage(base, s_q, PQ, r0, RB, n0);
        stage(base + C, s_k, PG, 0, dp, n0);
        __syncthreads();
        if (t < ncol) {
#pragma unroll 8
            for (int n = 0; n < nv; ++n) { const float x = col0[n * cp0]; nrm0 = __builtin_fmaf(x, x, nrm0); }
        }
        if (t1 < ncol) {
#pragma unroll 8
            for (int n = 0; n < nv; ++n) { const float x = col1[n * cp1]; nrm1 = __builtin_fmaf(x, x, nrm1); }
        }
        const int ksteps = (nv + 3) >> 2;                   // token quads beyond N hold only zero rows
        for (int ks = 0; ks < ksteps; ++ks) {
            const int row = ks * 4 + g;
#pragma unroll
            for (int s = 0; s < XCA_ANY_UNITS; ++s) {
                if (wave + nw * s < nunits) {               // wave-uniform
                    const float av = s_q[row * PQ + offa[s]];
                    const float bv = s_k[row * PG + offb[s]];
                    gacc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, gacc[s], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    if (t < ncol) s_n[t] = fmaxf(sqrtf(nrm0), 1e-12f);      // F.normalize: x / max(||x||, 1e-12)
    if (t1 < ncol) s_n[t1] = fmaxf(sqrtf(nrm1), 1e-12f);
#pragma unroll
    for (int s = 0; s < XCA_ANY_UNITS; ++s) {
        if (wave + nw * s < nunits) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s_g[(offa[s] - l15 + g * 4 + r) * PG + offb[s]] = gacc[s][r];
        }
    }
    __syncthreads();
    // ---- phase 2: A = softmax_rows(G / (|q_i| |k_j|) * temperature) over the columns j < d, 16 lanes per row, in place ---------------
    {
        const float temp = temperature[h];
        const int tj = t & 15;
        for (int il = t >> 4; il < rt * 16; il += nthr >> 4) {
            float* grow = s_g + il * PG;
            const bool live = r0 + il < d;                  // the same for the 16 lanes of a row
            const float nqi = s_n[dp + il];
            float m = -INFINITY;
            for (int j = tj; j < dp; j += 16) {
                if (live && j < d) {
                    const float v = grow[j] / (nqi * s_n[j]) * temp;
                    grow[j] = v;
                    m = fmaxf(m, v);
                }
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
            float sum = 0.f;
            for (int j = tj; j < dp; j += 16) {
                if (live && j < d) {
                    const float e = expf(grow[j] - m);
                    grow[j] = e;
                    sum += e;
                }
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, WAVE);
            for (int j = tj; j < dp; j += 16) grow[j] = (live && j < d) ? grow[j] / sum : 0.f;
        }
    }
    __syncthreads();
    // ---- phase 3: O[i][n] = sum_j A[i][j] v[n][j]; a lane holds 4 consecutive i of one token ------------------------------------------
    const int ntl = TC >> 4, kq = (d + 3) >> 2;             // A is zero from column d on
    for (int ch = 0; ch < nchunks; ++ch) {
        const int n0 = ch * TC;
        stage(base + 2 * C, s_k, PG, 0, dp, n0);
        __syncthreads();
        for (int tl = wave; tl < rt * ntl; tl += nw) {
            const int nt = tl / rt, it = tl - nt * rt;
            if (n0 + nt * 16 >= N) continue;                // wave-uniform: token tiles beyond N
            const float* ap = s_g + (it * 16 + l15) * PG + g;
            const float* bp = s_k + (nt * 16 + l15) * PG + g;
            f4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int ks = 0; ks < kq; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[ks * 4], bp[ks * 4], acc, 0, 0, 0);
            const int n = n0 + nt * 16 + l15, i0 = r0 + it * 16 + g * 4;
            if (n < N && i0 < d) {
                OT* o = out + ((long)b * N + n) * C + h * d + i0;
                if (vec_out) {                              // d % 4 == 0: the four rows are in range together
                    typedef OT o4 __attribute__((ext_vector_type(4)));
                    *reinterpret_cast<o4*>(o) = o4{(OT)acc.x, (OT)acc.y, (OT)acc.z, (OT)acc.w};
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (i0 + r < d) o[r] = (OT)acc[r];
                }
            }
        }
        __syncthreads();
    }
}

template <typename OT, typename IT>
static int xca_any_launch(const char* who, const IT* qkv, const float* temperature, OT* out, int B, int N, int heads, int d, hipStream_t st) {
    const XcaAnyGeom gm = xca_any_geom(d);
    const long grid = (long)B * heads * gm.nrb;
    if (grid > 0x7fffffffL) return mi355::fail(MI355_EUNSUPPORTED, "%s: B * heads * row blocks = %ld workgroups", who, grid);
    if (gm.lds > 65536)
        if (int rc = mi355::func_dynamic_lds(reinterpret_cast<const void*>(xca_any_kernel<OT, IT>), (int)gm.lds)) return rc;
    const int vec_in = d % (16 / (int)sizeof(IT)) == 0, vec_out = d % (16 / (int)sizeof(OT)) == 0;
    xca_any_kernel<OT, IT><<<(int)grid, gm.threads, gm.lds, st>>>(qkv, temperature, out, N, heads, d, gm.RB, gm.TC, vec_in, vec_out);
    return MI355_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// LPI: workgroup = (image, 32 channels); 256 threads = 32 token lanes x 8 channel quads (16-byte LDS / HBM accesses).
// Round 3: ONE LDS tile with a zero halo.  The first conv's results of a thread's (at most 8) tokens wait in registers until every
// thread has read its 3x3 neighbourhoods, then overwrite the tile's interior in place -- 32 KB instead of 50 KB per workgroup at 14x14
// (four to five workgroups per CU instead of three), and the stencils are nine unconditional 16-byte LDS reads + 36 FMAs per token
// (the round-1 form tested every tap against the grid border and divided by W per token and conv).
// Optional LayerNorm on the way in (XCABlock: x + gamma3 * LPI(norm3(x)), xcit.py:292): `stats` holds (mean, rstd) per token from
// ln_stats_kernel, the rows are normalised as they are parked in LDS -- the normalised tensor never exists in HBM and the residual is
// the very row the workgroup has just read.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int LPI_CG = 32;
constexpr int LPI_TMAX = 8;      // tokens per thread (N <= 256)

__global__ __launch_bounds__(256, 4) void lpi_kernel(const float* __restrict__ x, const float* __restrict__ w1,
                                                    const float* __restrict__ b1, const float* __restrict__ bn_w,
                                                    const float* __restrict__ bn_b, const float* __restrict__ bn_m,
                                                    const float* __restrict__ bn_v, float bn_eps, const float* __restrict__ w2,
                                                    const float* __restrict__ b2, const float* __restrict__ gamma,
                                                    const float* __restrict__ resid, float* __restrict__ y, int H, int W, int C,
                                                    int groups, const float* __restrict__ stats, const float* __restrict__ ln_w,
                                                    const float* __restrict__ ln_b) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int N = H * W, PW = W + 2;
    float* s_x = smem;                 // [(H+2)][(W+2)][32]: input tile with a zero halo (the stencils carry no bounds logic), then the intermediate
    const int t = threadIdx.x, cq = t & 7, tl = t >> 3;              // channel quad, token lane
    const int b = blockIdx.x / groups, c = (blockIdx.x % groups) * LPI_CG + cq * 4;
    const bool vec = ((C & 3) == 0) && (c + 3 < C);                  // whole quad in range and 16-byte aligned rows
    const float* xb = x + (long)b * N * C;
    auto ldc = [&](const float* p, int cc, float dflt) { return cc < C ? p[cc] : dflt; };
    auto ld4 = [&](const float* p, float dflt) { return f4{ldc(p, c, dflt), ldc(p, c + 1, dflt), ldc(p, c + 2, dflt), ldc(p, c + 3, dflt)}; };
    const f4 lw = stats ? ld4(ln_w, 0.f) : f4{1.f, 1.f, 1.f, 1.f}, lb = stats ? ld4(ln_b, 0.f) : f4{0.f, 0.f, 0.f, 0.f};
    // this thread's tokens n = tl + 32 j and their cells in the padded tile
    int cell[LPI_TMAX];
    f4 v0[LPI_TMAX];
#pragma unroll
    for (int j = 0; j < LPI_TMAX; ++j) {
        const int n = tl + 32 * j;
        const int yy = n / W, xx = n - yy * W;
        cell[j] = ((yy + 1) * PW + xx + 1) * LPI_CG + cq * 4;
        v0[j] = f4{0.f, 0.f, 0.f, 0.f};
        if (n < N) {
            if (vec) v0[j] = *reinterpret_cast<const f4*>(xb + (long)n * C + c);
            else v0[j] = f4{ldc(xb + (long)n * C, c, 0.f), ldc(xb + (long)n * C, c + 1, 0.f), ldc(xb + (long)n * C, c + 2, 0.f),
                            ldc(xb + (long)n * C, c + 3, 0.f)};
            if (stats) {                                              // the expression of layernorm_kernel: same bits as the unfused LayerNorm
                const float mean = stats[((long)b * N + n) * 2], rstd = stats[((long)b * N + n) * 2 + 1];
                v0[j] = (v0[j] - mean) * rstd * lw + lb;
            }
        }
    }
    for (int q = t; q < (H + 2) * PW * (LPI_CG / 4); q += 256) reinterpret_cast<f4*>(s_x)[q] = f4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LPI_TMAX; ++j)
        if (tl + 32 * j < N) *reinterpret_cast<f4*>(s_x + cell[j]) = v0[j];
    auto tap = [&](const float* p, int ch, int i) { return ch < C ? p[(long)ch * 9 + i] : 0.f; };     // dw weight (C,3,3)
    auto taps = [&](const float* p, f4* k) {
#pragma unroll
        for (int i = 0; i < 9; ++i) k[i] = f4{tap(p, c, i), tap(p, c + 1, i), tap(p, c + 2, i), tap(p, c + 3, i)};
    };
    auto conv = [&](const f4* k, f4 bias, int at) {                  // 3x3 around tile cell `at`: nine 16-byte LDS reads, no bounds logic
        f4 acc = bias;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
                acc = acc + k[(dy + 1) * 3 + dx + 1] * *reinterpret_cast<const f4*>(s_x + at + (dy * PW + dx) * LPI_CG);
        return acc;
    };
    f4 k[9];
    taps(w1, k);
    const f4 bias1 = ld4(b1, 0.f);
    const f4 mean = ld4(bn_m, 0.f), var = ld4(bn_v, 1.f), bw = ld4(bn_w, 0.f), bb = ld4(bn_b, 0.f);
    const f4 rstd = f4{1.0f / sqrtf(var.x + bn_eps), 1.0f / sqrtf(var.y + bn_eps), 1.0f / sqrtf(var.z + bn_eps),
                       1.0f / sqrtf(var.w + bn_eps)};
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LPI_TMAX; ++j) {
        if (tl + 32 * j < N) {
            const f4 u = conv(k, bias1, cell[j]);
            const f4 v = gelu_fast4(u);   // |erf error| <= 1.5e-7, ~3x fewer instructions than erff
            v0[j] = (v - mean) * rstd * bw + bb;
        }
    }
    taps(w2, k);                          // the first conv's taps are dead: same registers
    const f4 bias2 = ld4(b2, 0.f);
    __syncthreads();                      // every neighbourhood of the input tile has been read
#pragma unroll
    for (int j = 0; j < LPI_TMAX; ++j)
        if (tl + 32 * j < N) *reinterpret_cast<f4*>(s_x + cell[j]) = v0[j];
    __syncthreads();
    const f4 gm = gamma ? ld4(gamma, 1.f) : f4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int j = 0; j < LPI_TMAX; ++j) {
        const int n = tl + 32 * j;
        if (n >= N) continue;
        f4 v = conv(k, bias2, cell[j]);
        const long o = ((long)b * N + n) * C + c;
        if (gamma) v = v * gm;
        if (vec) {
            if (resid) v = v + *reinterpret_cast<const f4*>(resid + o);
            *reinterpret_cast<f4*>(y + o) = v;
        } else {
            const float vv[4] = {v.x, v.y, v.z, v.w};
            for (int q = 0; q < 4; ++q)
                if (c + q < C) y[o + q] = vv[q] + (resid ? resid[o + q] : 0.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Round 4: the same block for even token grids of at most 64 2 x 2 patches (XCiT at 224 px: 14 x 14), bound by LDS reads in the form
// above (nine 16-byte reads per token, stencil and channel quad; taps in 36 + 36 vector registers, 9 spilled at the 128-register budget).
//   * LDS holds the zero-haloed tile CHANNEL-QUAD-major in four planes (row parity x column parity of the padded grid), so that the 64
//     lanes of a wave, lane = one 2 x 2 patch, read any element of their 4 x 4 neighbourhoods as consecutive 16-byte chunks: 16 reads
//     for four outputs instead of 36, no bank conflict by construction (plane pitch odd, quad pitch = 2 mod 16 chunks for the
//     coalesced load / store phases, whose lanes are 8 quads x 8 tokens);
//   * a wave works on ONE channel quad at a time, so the 36 taps, bias, BatchNorm and LayerScale factors are wave-uniform: scalar
//     loads through a constant-address-space view of the weights (a plain global load after a barrier is not scalarised by hipcc),
//     pinned to their phase by an opaque zero in the index (hoisted to the kernel's top they cost > 100 live SGPRs, spilled into
//     VGPR lanes, which then spill to scratch);
//   * fused multiply-adds in the stencils (the form above rounds product and sum separately: -ffp-contract=off);
//   * load and store phases unchanged: 8 lanes = one 128-byte line of x / y.
// tools/lpi_probe.hip (B = 256, 14 x 14 x 384, inputs rotated through 616 MB): 73.6 -> 44.6 us, 33 us of it LDS + VALU.
// ---------------------------------------------------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) float* lpi_cptr;
constexpr int lpi_quad_pitch(int pls) { int c = 4 * pls; while (c % 16 != 2) ++c; return c; }

template <int H, int W, bool LN>
__global__ __launch_bounds__(256, 4) void lpi_patch_kernel(const float* __restrict__ x, const float* w1, const float* b1, const float* bn_w,
                                                           const float* bn_b, const float* bn_m, const float* bn_v, float bn_eps,
                                                           const float* w2, const float* b2, const float* gamma, const float* resid,
                                                           float* __restrict__ y, int C, int groups, const float* __restrict__ stats,
                                                           const float* __restrict__ ln_w, const float* __restrict__ ln_b) {
    constexpr int N = H * W, PR = H / 2 + 1, PP = W / 2 + 1, PLS = (PR * PP) | 1, CQS = lpi_quad_pitch(PLS), NJ = (N + 31) / 32;
    static_assert(H % 2 == 0 && W % 2 == 0 && (H / 2) * PP <= 64 && (PP & (PP - 1)) == 0, "one 2 x 2 patch per lane, PP lanes per patch row");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    f4* s = reinterpret_cast<f4*>(smem);
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int cq = t & 7, tl = t >> 3;
    const int b = blockIdx.x / groups, c0 = (blockIdx.x % groups) * LPI_CG;
    auto adr_of = [&](int n) {                                       // token n of channel quad cq in the planes
        const int yy = n / W, xx = n - yy * W, R = yy + 1, Cc = xx + 1;
        return cq * CQS + ((R & 1) * 2 + (Cc & 1)) * PLS + (R >> 1) * PP + (Cc >> 1);
    };
    auto mine = [&](int j) { return 32 * j + 31 < N || tl + 32 * j < N; };      // full iterations are decided at compile time
    // ---- phase 1: coalesced loads, LayerNorm applied on the way into LDS (the expression of layernorm_kernel: same bits) ----
    {
        const float* xb = x + ((long)b * N) * C + c0 + cq * 4;
        f4 v0[NJ];
        float2 st[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int n = tl + 32 * j;
            v0[j] = f4{0.f, 0.f, 0.f, 0.f};
            st[j] = float2{0.f, 1.f};
            if (mine(j)) {
                v0[j] = *reinterpret_cast<const f4*>(xb + (long)n * C);
                if constexpr (LN) st[j] = *reinterpret_cast<const float2*>(stats + ((long)b * N + n) * 2);
            }
        }
        // zero halo of every quad while the loads fly: 2 (W + 2) + 2 H cells x 8 quads; every interior cell is written below
        constexpr int HC = 2 * (W + 2) + 2 * H;
#pragma unroll
        for (int i = 0; i < (8 * HC + 255) / 256; ++i) {
            const int q = t + 256 * i;
            if (q < 8 * HC) {
                const int zq = q / HC, h = q - zq * HC;
                int R, Cc;
                if (h < W + 2) { R = 0; Cc = h; }
                else if (h < 2 * (W + 2)) { R = H + 1; Cc = h - (W + 2); }
                else { const int k = h - 2 * (W + 2); R = 1 + (k >> 1); Cc = (k & 1) ? W + 1 : 0; }
                s[zq * CQS + ((R & 1) * 2 + (Cc & 1)) * PLS + (R >> 1) * PP + (Cc >> 1)] = f4{0.f, 0.f, 0.f, 0.f};
            }
        }
        f4 lw = f4{1.f, 1.f, 1.f, 1.f}, lb = f4{0.f, 0.f, 0.f, 0.f};
        if constexpr (LN) { lw = *reinterpret_cast<const f4*>(ln_w + c0 + cq * 4); lb = *reinterpret_cast<const f4*>(ln_b + c0 + cq * 4); }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (mine(j)) {
                if constexpr (LN) s[adr_of(tl + 32 * j)] = (v0[j] - st[j].x) * st[j].y * lw + lb;
                else              s[adr_of(tl + 32 * j)] = v0[j];
            }
    }
    const int py = lane / PP, px = lane & (PP - 1);
    const bool active = px < W / 2 && py < H / 2;
    auto quad4 = [&](lpi_cptr p, int cb) { return f4{p[cb], p[cb + 1], p[cb + 2], p[cb + 3]}; };
    auto stencil = [&](const float* wt_, const float* bs_, int q, f4* out) {
        lpi_cptr wt = (lpi_cptr)wt_, bs = (lpi_cptr)bs_;
        int pin = 0;
        asm volatile("" : "+s"(pin));                                 // the scalar loads below stay in this phase
        const int cb = c0 + q * 4 + pin;
        const f4* base = s + q * CQS + py * PP + px;
        const f4 bias = quad4(bs, cb);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = bias;
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                // one row of the 4 x 4 neighbourhood at a time: 16 operand registers
            f4 in[4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) in[cc] = base[((r & 1) * 2 + (cc & 1)) * PLS + (r >> 1) * PP + (cc >> 1)];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int dy = r - a;                                 // taps in the order dy, dx of the form above
                if (dy < 0 || dy > 2) continue;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int i9 = dy * 3 + dx;
                    const f4 k = f4{wt[(cb + 0) * 9 + i9], wt[(cb + 1) * 9 + i9], wt[(cb + 2) * 9 + i9], wt[(cb + 3) * 9 + i9]};
#pragma unroll
                    for (int bb = 0; bb < 2; ++bb) {
                        f4& o = out[a * 2 + bb];
                        const f4 v = in[bb + dx];
                        o = f4{__builtin_fmaf(k.x, v.x, o.x), __builtin_fmaf(k.y, v.y, o.y), __builtin_fmaf(k.z, v.z, o.z), __builtin_fmaf(k.w, v.w, o.w)};
                    }
                }
            }
        }
    };
    auto put = [&](int q, const f4* out) {                            // the patch's four tokens back into the planes
        f4* base = s + q * CQS + py * PP + px;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) base[(((a + 1) & 1) * 2 + ((bb + 1) & 1)) * PLS + ((a + 1) >> 1) * PP + ((bb + 1) >> 1)] = out[a * 2 + bb];
    };
    f4 res[2][4];
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = wave * 2 + i;
            stencil(w1, b1, q, res[i]);
            int pin = 0;
            asm volatile("" : "+s"(pin));
            const int cb = c0 + q * 4 + pin;
            const f4 mean = quad4((lpi_cptr)bn_m, cb), var = quad4((lpi_cptr)bn_v, cb), bw = quad4((lpi_cptr)bn_w, cb), bb = quad4((lpi_cptr)bn_b, cb);
            const f4 rstd = f4{1.0f / sqrtf(var.x + bn_eps), 1.0f / sqrtf(var.y + bn_eps), 1.0f / sqrtf(var.z + bn_eps), 1.0f / sqrtf(var.w + bn_eps)};
#pragma unroll
            for (int e = 0; e < 4; ++e) res[i][e] = (gelu_fast4(res[i][e]) - mean) * rstd * bw + bb;
        }
    }
    __syncthreads();                      // every neighbourhood of the input tile has been read
    if (active) { put(wave * 2, res[0]); put(wave * 2 + 1, res[1]); }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = wave * 2 + i;
            stencil(w2, b2, q, res[i]);
            if (gamma) {
                int pin = 0;
                asm volatile("" : "+s"(pin));
                const f4 gm = quad4((lpi_cptr)gamma, c0 + q * 4 + pin);
#pragma unroll
                for (int e = 0; e < 4; ++e) res[i][e] = res[i][e] * gm;
            }
        }
    }
    __syncthreads();
    if (active) { put(wave * 2, res[0]); put(wave * 2 + 1, res[1]); }
    __syncthreads();
    // ---- phase 4: residual + coalesced store ----
    float* yp = y + ((long)b * N) * C + c0 + cq * 4;
    f4 rr[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        rr[j] = f4{0.f, 0.f, 0.f, 0.f};
        if (resid && mine(j)) rr[j] = *reinterpret_cast<const f4*>(resid + ((long)b * N + tl + 32 * j) * C + c0 + cq * 4);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (mine(j)) *reinterpret_cast<f4*>(yp + (long)(tl + 32 * j) * C) = s[adr_of(tl + 32 * j)] + rr[j];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Token grids above 16 x 16 (XCiT patch 8 at 224 px: 28 x 28; patch 16 at 384 px: 24 x 24; any H, W, C): lpi_kernel's block on a TILE of
// the grid.  Workgroup = (image, tile, 32 channels); the tile is `rows` x `cols` output tokens and sits in LDS with a 2-cell halo of
// INPUT, because two stacked 3 x 3 stencils reach that far.  Same structure as lpi_kernel: 32 token lanes x 8 channel quads, 16-byte
// LDS / HBM accesses, the first conv's results wait in registers and overwrite the tile in place, no bounds logic in the stencils, the
// same per-element expressions in the same order (separately rounded products and sums, gelu_fast4, BatchNorm as (v - mean) * rstd *
// bw + bb, LayerNorm as (v - mean) * rstd * lw + lb from `stats`, which therefore holds a row for every halo token as well).
//   * input cells outside the grid are zero (conv1's padding); every cell of the tile is written exactly once on the way in, so there
//     is no separate zero fill;
//   * the intermediate is needed on the 1-cell ring around the tile's outputs: ring cells INSIDE the grid are recomputed (conv1 + GELU
//     + BatchNorm, what the neighbouring tile computes for its own outputs: same inputs, same expressions, same bits); ring cells
//     OUTSIDE the grid are ZERO -- they are conv2's padding, not conv1 of padded input (that would be bn(gelu(b1)) != 0);
//   * the outermost ring keeps its input values after the in-place overwrite; conv2 never reads it.
// Tile shape: lpi_tile_shape below, from (H, W) alone -- at most 384 cells of 128 bytes (48 KB: three workgroups per CU, which is what
// __launch_bounds__(256, 3) states), hence at most 320 ring-1 cells = LPI_TILE_TM per thread.  Cell coordinates advance by 32 cells per
// step without a division (quotient and remainder of 32 by the pitch are workgroup constants).  y must not alias x: neighbouring
// tiles read each other's rows.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int LPI_TILE_CELLS = 384;   // (rows + 4) * (cols + 4) <= this
constexpr int LPI_TILE_TM = 10;       // (rows + 2) * (cols + 2) <= 32 * this whenever the line above holds (a + b >= 2 sqrt(ab))

template <bool LN>
__global__ __launch_bounds__(256, 3) void lpi_tile_kernel(const float* __restrict__ x, const float* __restrict__ w1,
                                                         const float* __restrict__ b1, const float* __restrict__ bn_w,
                                                         const float* __restrict__ bn_b, const float* __restrict__ bn_m,
                                                         const float* __restrict__ bn_v, float bn_eps, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, const float* __restrict__ gamma,
                                                         const float* __restrict__ resid, float* __restrict__ y, int H, int W, int C,
                                                         int groups, int R, int TW, int nby, int nbx, const float* __restrict__ stats,
                                                         const float* __restrict__ ln_w, const float* __restrict__ ln_b) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_x = smem;                 // [(rows+4)][(cols+4)][32]: input tile with its 2-cell halo, then the intermediate on the inner ring
    const int t = threadIdx.x, cq = t & 7, tl = t >> 3;              // channel quad, token lane
    int bid = blockIdx.x;                                            // (image, tile row, tile column, channel group), group fastest
    const int c = (bid % groups) * LPI_CG + cq * 4;
    bid /= groups;
    const int bx = bid % nbx;
    bid /= nbx;
    const int by = bid % nby, b = bid / nby;
    const int r0 = by * R, c0 = bx * TW;                             // first output row / column of the tile
    const int rows = min(R, H - r0), cols = min(TW, W - c0), PW = cols + 4;
    const long N = (long)H * W;
    const bool vec = ((C & 3) == 0) && (c + 3 < C);                  // whole quad in range and 16-byte aligned rows
    const float* xb = x + (long)b * N * C;
    auto ldc = [&](const float* p, int cc, float dflt) { return cc < C ? p[cc] : dflt; };
    auto ld4 = [&](const float* p, float dflt) { return f4{ldc(p, c, dflt), ldc(p, c + 1, dflt), ldc(p, c + 2, dflt), ldc(p, c + 3, dflt)}; };
    auto inside = [&](int gy, int gx) { return (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W; };
    // ---- the tile with its halo: cell p = tl + 32 i, four loads in flight per thread ----
    {
        const f4 lw = LN ? ld4(ln_w, 0.f) : f4{1.f, 1.f, 1.f, 1.f}, lb = LN ? ld4(ln_b, 0.f) : f4{0.f, 0.f, 0.f, 0.f};
        const int ncell = (rows + 4) * PW, q32 = 32 / PW, r32 = 32 - q32 * PW;
        int ty = tl / PW, tx = tl - ty * PW;
        for (int p0 = tl; p0 < ncell; p0 += 128) {
            f4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int gy = r0 - 2 + ty, gx = c0 - 2 + tx;
                v[u] = f4{0.f, 0.f, 0.f, 0.f};
                if (p0 + 32 * u < ncell && inside(gy, gx)) {
                    const long n = (long)gy * W + gx;
                    const float* xr = xb + n * C;
                    if (vec) v[u] = *reinterpret_cast<const f4*>(xr + c);
                    else v[u] = f4{ldc(xr, c, 0.f), ldc(xr, c + 1, 0.f), ldc(xr, c + 2, 0.f), ldc(xr, c + 3, 0.f)};
                    if (LN) {                                         // the expression of layernorm_kernel: same bits as the unfused LayerNorm
                        const float mean = stats[((long)b * N + n) * 2], rstd = stats[((long)b * N + n) * 2 + 1];
                        v[u] = (v[u] - mean) * rstd * lw + lb;
                    }
                }
                tx += r32;
                ty += q32;
                if (tx >= PW) { tx -= PW; ++ty; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (p0 + 32 * u < ncell) *reinterpret_cast<f4*>(s_x + (p0 + 32 * u) * LPI_CG + cq * 4) = v[u];
        }
    }
    auto tap = [&](const float* p, int ch, int i) { return ch < C ? p[(long)ch * 9 + i] : 0.f; };     // dw weight (C,3,3)
    auto taps = [&](const float* p, f4* k) {
#pragma unroll
        for (int i = 0; i < 9; ++i) k[i] = f4{tap(p, c, i), tap(p, c + 1, i), tap(p, c + 2, i), tap(p, c + 3, i)};
    };
    auto conv = [&](const f4* k, f4 bias, int at) {                  // 3x3 around tile cell `at`: nine 16-byte LDS reads, no bounds logic
        f4 acc = bias;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
                acc = acc + k[(dy + 1) * 3 + dx + 1] * *reinterpret_cast<const f4*>(s_x + at + (dy * PW + dx) * LPI_CG);
        return acc;
    };
    f4 k[9];
    taps(w1, k);
    const f4 bias1 = ld4(b1, 0.f);
    const f4 mean = ld4(bn_m, 0.f), var = ld4(bn_v, 1.f), bw = ld4(bn_w, 0.f), bb = ld4(bn_b, 0.f);
    const f4 rstd = f4{1.0f / sqrtf(var.x + bn_eps), 1.0f / sqrtf(var.y + bn_eps), 1.0f / sqrtf(var.z + bn_eps),
                       1.0f / sqrtf(var.w + bn_eps)};
    // ---- the intermediate on the tile's outputs and the ring around them: cell m = tl + 32 j of a (rows+2) x (cols+2) window ----
    const int IW = cols + 2, nmid = (rows + 2) * IW;
    int cell[LPI_TILE_TM];
    f4 v0[LPI_TILE_TM];
    __syncthreads();
    {
        const int q32 = 32 / IW, r32 = 32 - q32 * IW;
        int iy = tl / IW, ix = tl - iy * IW;
#pragma unroll
        for (int j = 0; j < LPI_TILE_TM; ++j) {
            cell[j] = ((iy + 1) * PW + ix + 1) * LPI_CG + cq * 4;
            v0[j] = f4{0.f, 0.f, 0.f, 0.f};                           // outside the grid: conv2's zero padding
            if (tl + 32 * j < nmid && inside(r0 - 1 + iy, c0 - 1 + ix)) {
                const f4 u = conv(k, bias1, cell[j]);
                const f4 v = gelu_fast4(u);   // |erf error| <= 1.5e-7, ~3x fewer instructions than erff
                v0[j] = (v - mean) * rstd * bw + bb;
            }
            ix += r32;
            iy += q32;
            if (ix >= IW) { ix -= IW; ++iy; }
        }
    }
    taps(w2, k);                          // the first conv's taps are dead: same registers
    const f4 bias2 = ld4(b2, 0.f);
    __syncthreads();                      // every neighbourhood of the input tile has been read
#pragma unroll
    for (int j = 0; j < LPI_TILE_TM; ++j)
        if (tl + 32 * j < nmid) *reinterpret_cast<f4*>(s_x + cell[j]) = v0[j];
    __syncthreads();
    // ---- outputs: token o = tl + 32 j of the rows x cols interior ----
    const f4 gm = gamma ? ld4(gamma, 1.f) : f4{1.f, 1.f, 1.f, 1.f};
    const int nout = rows * cols, q32 = 32 / cols, r32 = 32 - q32 * cols;
    int oy = tl / cols, ox = tl - oy * cols;
#pragma unroll
    for (int j = 0; j < LPI_TILE_TM; ++j) {
        if (tl + 32 * j < nout) {
            f4 v = conv(k, bias2, ((oy + 2) * PW + ox + 2) * LPI_CG + cq * 4);
            const long o = ((long)b * N + (long)(r0 + oy) * W + c0 + ox) * C + c;
            if (gamma) v = v * gm;
            if (vec) {
                if (resid) v = v + *reinterpret_cast<const f4*>(resid + o);
                *reinterpret_cast<f4*>(y + o) = v;
            } else {
                const float vv[4] = {v.x, v.y, v.z, v.w};
                for (int q = 0; q < 4; ++q)
                    if (c + q < C) y[o + q] = vv[q] + (resid ? resid[o + q] : 0.f);
            }
        }
        ox += r32;
        oy += q32;
        if (ox >= cols) { ox -= cols; ++oy; }
    }
}

// (mean, rstd) of every token row: the statistics of layernorm_kernel (two-pass, biased variance, eps inside the sqrt), one wave per
// row; what the LayerNorm-fused LPI above normalises with.  Reads x once, writes 8 bytes per row.
__global__ __launch_bounds__(256) void ln_stats_kernel(const float* __restrict__ x, float* __restrict__ stats, long rows, int cols, float eps) {
    const int lane = threadIdx.x & 63;
    const long wave0 = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    const float inv = 1.0f / (float)cols;
    const bool vec = (cols & 3) == 0;
    for (long row = wave0; row < rows; row += nwaves) {
        const float* xr = x + row * cols;
        float s = 0.f, q = 0.f;
        if (vec && cols <= 512) {                                       // the row fits two float4 per lane: read once (same sums, same order)
            const int n4 = cols >> 2;
            const bool h0 = lane < n4, h1 = lane + 64 < n4;
            const f4 z = f4{0.f, 0.f, 0.f, 0.f};
            const f4 v0 = h0 ? reinterpret_cast<const f4*>(xr)[lane] : z, v1 = h1 ? reinterpret_cast<const f4*>(xr)[lane + 64] : z;
            if (h0) s += (v0.x + v0.y) + (v0.z + v0.w);
            if (h1) s += (v1.x + v1.y) + (v1.z + v1.w);
            const float mean = wave_sum(s) * inv;
            if (h0) { const f4 d = v0 - mean; q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w); }
            if (h1) { const f4 d = v1 - mean; q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w); }
            const float r = 1.0f / sqrtf(wave_sum(q) * inv + eps);
            if (lane == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = r; }
        } else if (vec) {
            const int n4 = cols >> 2;
            for (int i = lane; i < n4; i += 64) { const f4 v = reinterpret_cast<const f4*>(xr)[i]; s += (v.x + v.y) + (v.z + v.w); }
            const float mean = wave_sum(s) * inv;
            for (int i = lane; i < n4; i += 64) {
                const f4 d = reinterpret_cast<const f4*>(xr)[i] - mean;
                q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
            }
            const float r = 1.0f / sqrtf(wave_sum(q) * inv + eps);     // every lane takes part in the reduction
            if (lane == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = r; }
        } else {
            for (int i = lane; i < cols; i += 64) s += xr[i];          // the expressions of layernorm_generic_kernel (true divisions)
            const float mean = wave_sum(s) / (float)cols;
            for (int i = lane; i < cols; i += 64) { const float d = xr[i] - mean; q += d * d; }
            const float r = 1.0f / sqrtf(wave_sum(q) / (float)cols + eps);
            if (lane == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = r; }
        }
    }
}

}  // namespace

extern "C" {

int mi355_xca_fwd(const float* qkv, const float* temperature, float* out, int B, int N, int heads, int d, int precision,
                  mi355_stream_t stream) {
    MI355_CHECK_ARG(qkv && temperature && out && B > 0 && N > 0 && heads > 0);
    MI355_CHECK_ARG(precision >= 0 && precision <= 2);      // accepted for API symmetry; the core is exact fp32 in every mode
    MI355_CHECK_ARG(aligned16(qkv) && aligned16(out));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = B * heads;
    if (d < 1 || d > XCA_ANY_MAX) return mi355::fail(MI355_EUNSUPPORTED, "mi355_xca_fwd: head dim %d (supported: 1 .. %d)", d, XCA_ANY_MAX);
    if (d != 32 && d != 48 && d != 64) {                    // every width without a template: the run-time-width kernel
        MI355_TRACE(st, "xca_any_kernel<d=%d> B=%d N=%d heads=%d", d, B, N, heads);
        if (int rc = xca_any_launch<float, float>("mi355_xca_fwd", qkv, temperature, out, B, N, heads, d, st)) return rc;
        MI355_LAUNCH_CHECK();
        return MI355_OK;
    }
    MI355_TRACE(st, "xca_kernel<d=%d> B=%d N=%d heads=%d", d, B, N, heads);
    switch (d) {
        case 32: xca_kernel<32><<<grid, 256, 0, st>>>(qkv, temperature, out, N, heads); break;
        case 48: xca_kernel<48><<<grid, 256, 0, st>>>(qkv, temperature, out, N, heads); break;
        default: xca_kernel<64><<<grid, 256, 0, st>>>(qkv, temperature, out, N, heads); break;
    }
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}
// The same core with the context written in the 16-bit operand format of `precision` (1 = fp16, 2 = bf16): what the proj GEMM of the
// 16-bit dataflow reads (xcit.py:248-249), without a separate cast pass; qkv_is16 != 0: qkv itself is in that format (the 16-bit
// output of the qkv GEMM).
int mi355_xca16_fwd(const void* qkv, int qkv_is16, const float* temperature, void* out16, int B, int N, int heads, int d, int precision,
                    mi355_stream_t stream) {
    MI355_CHECK_ARG(qkv && temperature && out16 && B > 0 && N > 0 && heads > 0);
    MI355_CHECK_ARG(precision == MI355_PREC_FP16 || precision == MI355_PREC_BF16);
    MI355_CHECK_ARG(aligned16(qkv) && aligned16(out16));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = B * heads;
    if (d < 1 || d > XCA_ANY_MAX) return mi355::fail(MI355_EUNSUPPORTED, "mi355_xca16_fwd: head dim %d (supported: 1 .. %d)", d, XCA_ANY_MAX);
    if (d != 32 && d != 48 && d != 64) {                    // every width without a template: the run-time-width kernel, same three type modes
        MI355_TRACE(st, "xca_any_kernel<d=%d%s,out16> B=%d N=%d heads=%d", d, qkv_is16 ? ",in16" : "", B, N, heads);
        int rc;
        if (qkv_is16) {
            if (precision == MI355_PREC_FP16) rc = xca_any_launch<_Float16, _Float16>("mi355_xca16_fwd", static_cast<const _Float16*>(qkv), temperature, static_cast<_Float16*>(out16), B, N, heads, d, st);
            else                              rc = xca_any_launch<__bf16, __bf16>("mi355_xca16_fwd", static_cast<const __bf16*>(qkv), temperature, static_cast<__bf16*>(out16), B, N, heads, d, st);
        } else if (precision == MI355_PREC_FP16) rc = xca_any_launch<_Float16, float>("mi355_xca16_fwd", static_cast<const float*>(qkv), temperature, static_cast<_Float16*>(out16), B, N, heads, d, st);
        else                              rc = xca_any_launch<__bf16, float>("mi355_xca16_fwd", static_cast<const float*>(qkv), temperature, static_cast<__bf16*>(out16), B, N, heads, d, st);
        if (rc) return rc;
        MI355_LAUNCH_CHECK();
        return MI355_OK;
    }
    if (qkv_is16 && N <= 224 && mi355::opt(mi355::O_XCA_TR) && (d == 32 || d == 48 || d == 64)) {
        // 16-bit q / k / v, at most 224 tokens: covariance on the 16-bit matrix pipe from ONE transposed LDS image (xca_tr_kernel)
        MI355_TRACE(st, "xca_tr_kernel<d=%d> B=%d N=%d heads=%d", d, B, N, heads);
#define XTR(D_)                                                                                                                          \
        do {                                                                                                                             \
            if (precision == MI355_PREC_FP16) xca_tr_kernel<D_, _Float16><<<grid, 256, 0, st>>>(static_cast<const _Float16*>(qkv), temperature, static_cast<_Float16*>(out16), N, heads); \
            else                              xca_tr_kernel<D_, __bf16><<<grid, 256, 0, st>>>(static_cast<const __bf16*>(qkv), temperature, static_cast<__bf16*>(out16), N, heads);         \
        } while (0)
        if (d == 32) XTR(32); else if (d == 48) XTR(48); else XTR(64);
#undef XTR
        MI355_LAUNCH_CHECK();
        return MI355_OK;
    }
    MI355_TRACE(st, "xca_kernel<d=%d,out16%s> B=%d N=%d heads=%d", d, qkv_is16 ? ",in16" : "", B, N, heads);
#define XCA16(D_)                                                                                                              \
    do {                                                                                                                       \
        if (qkv_is16) {                                                                                                        \
            if (precision == MI355_PREC_FP16) xca_kernel<D_, _Float16, _Float16><<<grid, 256, 0, st>>>(static_cast<const _Float16*>(qkv), temperature, static_cast<_Float16*>(out16), N, heads); \
            else                              xca_kernel<D_, __bf16, __bf16><<<grid, 256, 0, st>>>(static_cast<const __bf16*>(qkv), temperature, static_cast<__bf16*>(out16), N, heads);         \
        } else if (precision == MI355_PREC_FP16) xca_kernel<D_, _Float16><<<grid, 256, 0, st>>>(static_cast<const float*>(qkv), temperature, static_cast<_Float16*>(out16), N, heads); \
        else                              xca_kernel<D_, __bf16><<<grid, 256, 0, st>>>(static_cast<const float*>(qkv), temperature, static_cast<__bf16*>(out16), N, heads);     \
    } while (0)
    switch (d) {
        case 32: XCA16(32); break;
        case 48: XCA16(48); break;
        default: XCA16(64); break;
    }
#undef XCA16
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}


size_t mi355_lpi_workspace_bytes(int B, int H, int W, int) {      // (mean, rstd) per token of the LayerNorm-fused form
    if (B <= 0 || H <= 0 || W <= 0) return 16;
    return (size_t)B * H * W * 2 * sizeof(float) + 16;
}

// Tile of lpi_tile_kernel for an H x W token grid: R rows x TW columns of outputs, (R + 4) * (TW + 4) <= LPI_TILE_CELLS.  A function of
// (H, W) only -- not of B, C or the CU count -- so an image's result does not depend on the batch it arrives in.
//   * W <= 44 (a band of at least 4 rows fits): row bands of the full width, the tallest that fit, evened out over the grid
//     (28 x 28: 4 bands of 7 rows, 44 KB; 24 x 24: 3 bands of 8 rows, 42 KB).  The kernel then loads (R + 4) / R and runs conv1 on
//     about (R + 2) / R of what an untiled pass would.
//   * wider grids: column tiles as well -- the number of tile columns that loads the fewest cells per output, rows as above.
static void lpi_tile_shape(int H, int W, int* R, int* TW) {
    auto band = [&](int tw) {                                        // evened-out band height for tile width tw (0: not even one row fits)
        const int rmax = LPI_TILE_CELLS / (tw + 4) - 4;
        if (rmax < 1) return 0;
        return (int)cdiv(H, cdiv(H, rmax < H ? rmax : H));
    };
    *TW = W;
    *R = band(W);
    if (W <= 44) return;
    double best = 1e30;
    for (int nbx = 1; nbx <= W; ++nbx) {
        const int tw = (int)cdiv(W, nbx), r = band(tw);
        if (r > 0) {
            const double cost = (double)(r + 4) * (tw + 4) / ((double)r * tw);
            if (cost < best) { best = cost; *R = r; *TW = tw; }
        }
        if (tw <= 8) break;                                          // narrower tiles only load more halo
    }
}

static int lpi_launch(const float* x, const float* w1, const float* b1, const float* bn_w, const float* bn_b, const float* bn_mean,
                      const float* bn_var, float bn_eps, const float* w2, const float* b2, const float* gamma, const float* resid,
                      float* y, int B, int H, int W, int C, const float* stats, const float* ln_w, const float* ln_b, hipStream_t st) {
    if ((long)H * W > 32 * LPI_TMAX) {
        // above 16 x 16 tokens: tiles of the grid with a 2-cell halo (see lpi_tile_kernel)
        int R, TW;
        lpi_tile_shape(H, W, &R, &TW);
        const int groups = cdiv(C, LPI_CG), nby = cdiv(H, R), nbx = cdiv(W, TW);
        const long grid = (long)B * groups * nby * nbx;
        if (grid > 0x7fffffffL) return mi355::fail(MI355_EINVAL, "mi355_lpi_fwd: B=%d %dx%d C=%d needs %ld workgroups", B, H, W, C, grid);
        const size_t smem = (size_t)(R + 4) * (TW + 4) * LPI_CG * sizeof(float);
        MI355_TRACE(st, "lpi_tile_kernel%s B=%d %dx%d C=%d tile=%dx%d", stats ? "<ln>" : "", B, H, W, C, R, TW);
        if (stats) lpi_tile_kernel<true><<<(unsigned)grid, 256, smem, st>>>(x, w1, b1, bn_w, bn_b, bn_mean, bn_var, bn_eps, w2, b2, gamma, resid, y, H, W, C, groups, R, TW, nby, nbx, stats, ln_w, ln_b);
        else       lpi_tile_kernel<false><<<(unsigned)grid, 256, smem, st>>>(x, w1, b1, bn_w, bn_b, bn_mean, bn_var, bn_eps, w2, b2, gamma, resid, y, H, W, C, groups, R, TW, nby, nbx, nullptr, nullptr, nullptr);
        MI355_LAUNCH_CHECK();
        return MI355_OK;
    }
    if (H == 14 && W == 14 && (C % LPI_CG) == 0 && mi355::opt(mi355::O_LPI_PATCH) && aligned16(x) && aligned16(y) && (!resid || aligned16(resid)) &&
        (!stats || (aligned16(ln_w) && aligned16(ln_b)))) {
        // 2 x 2 patches per lane, channel-quad-major planes (see lpi_patch_kernel)
        constexpr int PLS = (8 * 8) | 1, CQS = lpi_quad_pitch(PLS);
        const size_t smem = (size_t)8 * CQS * 16;
        const int groups = C / LPI_CG;
        MI355_TRACE(st, "lpi_patch_kernel%s B=%d %dx%d C=%d", stats ? "<ln>" : "", B, H, W, C);
        if (stats) lpi_patch_kernel<14, 14, true><<<B * groups, 256, smem, st>>>(x, w1, b1, bn_w, bn_b, bn_mean, bn_var, bn_eps, w2, b2, gamma, resid, y, C, groups, stats, ln_w, ln_b);
        else       lpi_patch_kernel<14, 14, false><<<B * groups, 256, smem, st>>>(x, w1, b1, bn_w, bn_b, bn_mean, bn_var, bn_eps, w2, b2, gamma, resid, y, C, groups, nullptr, nullptr, nullptr);
        MI355_LAUNCH_CHECK();
        return MI355_OK;
    }
    const size_t smem = (size_t)(H + 2) * (W + 2) * LPI_CG * sizeof(float);
    const int groups = cdiv(C, LPI_CG);
    MI355_TRACE(st, "lpi_kernel%s B=%d %dx%d C=%d", stats ? "<ln>" : "", B, H, W, C);
    lpi_kernel<<<B * groups, 256, smem, st>>>(x, w1, b1, bn_w, bn_b, bn_mean, bn_var, bn_eps, w2, b2, gamma, resid, y, H, W, C, groups,
                                              stats, ln_w, ln_b);
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}

int mi355_lpi_fwd(const float* x, const float* w1, const float* b1, const float* bn_w, const float* bn_b, const float* bn_mean,
                  const float* bn_var, float bn_eps, const float* w2, const float* b2, const float* gamma, const float* resid,
                  float* y, int B, int H, int W, int C, void* ws, size_t ws_bytes, mi355_stream_t stream) {
    MI355_CHECK_ARG(x && w1 && b1 && bn_w && bn_b && bn_mean && bn_var && w2 && b2 && y);
    MI355_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0);
    (void)ws; (void)ws_bytes;
    return lpi_launch(x, w1, b1, bn_w, bn_b, bn_mean, bn_var, bn_eps, w2, b2, gamma, resid, y, B, H, W, C, nullptr, nullptr, nullptr,
                      static_cast<hipStream_t>(stream));
}

int mi355_ln_lpi_fwd(const float* x, const float* ln_w, const float* ln_b, float ln_eps, const float* w1, const float* b1,
                     const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var, float bn_eps, const float* w2,
                     const float* b2, const float* gamma, const float* resid, float* y, int B, int H, int W, int C, void* ws,
                     size_t ws_bytes, mi355_stream_t stream) {
    MI355_CHECK_ARG(x && ln_w && ln_b && w1 && b1 && bn_w && bn_b && bn_mean && bn_var && w2 && b2 && y && ws);
    MI355_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0);
    MI355_CHECK_ARG(ws_bytes >= mi355_lpi_workspace_bytes(B, H, W, C) && aligned16(ws) && aligned16(x));
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* stats = static_cast<float*>(ws);
    const long rows = (long)B * H * W;
    const int grid = (int)(cdiv(rows, 4) < 8192 ? cdiv(rows, 4) : 8192);
    {
        MI355_TRACE(st, "ln_stats_kernel rows=%ld cols=%d", rows, C);
        ln_stats_kernel<<<grid, 256, 0, st>>>(x, stats, rows, C, ln_eps);
    }
    return lpi_launch(x, w1, b1, bn_w, bn_b, bn_mean, bn_var, bn_eps, w2, b2, gamma, resid, y, B, H, W, C, stats, ln_w, ln_b, st);
}

// The same with the LayerNorm statistics GIVEN: stats (B*H*W, 2) = (mean, 1 / sqrt(var + eps)) per token, as written by
// mi355_linear16_stats_fwd beside the tensor x (XCABlock: the proj GEMM in front of this block writes them for free).
int mi355_ln_lpi_stats_fwd(const float* x, const float* stats, const float* ln_w, const float* ln_b, const float* w1, const float* b1,
                           const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var, float bn_eps, const float* w2,
                           const float* b2, const float* gamma, const float* resid, float* y, int B, int H, int W, int C,
                           mi355_stream_t stream) {
    MI355_CHECK_ARG(x && stats && ln_w && ln_b && w1 && b1 && bn_w && bn_b && bn_mean && bn_var && w2 && b2 && y);
    MI355_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && aligned16(x));
    return lpi_launch(x, w1, b1, bn_w, bn_b, bn_mean, bn_var, bn_eps, w2, b2, gamma, resid, y, B, H, W, C, stats, ln_w, ln_b,
                      static_cast<hipStream_t>(stream));
}

}  // extern "C"
