// dual_attn_io16.hip -- DANet's CAM and the two x-touching steps of PAM on fp16 / bf16 activations (gfx950, wave64).
// io = 1: IEEE half, 2: bfloat16 (the library's precision codes); x and y are NCHW in that type, everything in between is fp32.
//
// Every product of two 16-bit values fits an fp32 significand, so x enters every product UNROUNDED and is never converted to a
// narrower type:
//   bf16 x  is its own split-bf16 `hi` plane (lo = 0);
//   fp16 x  is exactly bf16 hi + bf16 lo (hi = rne_bf16(x), lo = x - hi: 11 significand bits = 8 + at most 4), and bf16 has the fp32
//           exponent range, so fp16 subnormals are ordinary bf16 numbers.
//
//   cam_gram16_kernel     G[b] = X X^T (fp32) from x as it lies: ONE native v_mfma_f32_16x16x32_f16 / _bf16 per step where the fp32 path
//                         needs the three of the split-bf16 mode.  Upper tiles only, mirrored at the store.  The fp16 form is the NATIVE
//                         product: a probe on an MI355X (A or B = 2^-20, an fp16 subnormal, against 1 and against itself, 32 terms) gave
//                         the exact sums, i.e. the fp16 MFMA does not flush subnormal A / B operands, and
//                         tests/test_dual_io16_gpu.py::test_cam_subnormal_channel holds it to that (a flushed Gram is 206 x its bound).
//                         The hi / lo-plane form of the fp16 Gram was therefore not built (profiles/dual_io16.md).
//   (softmax)             ragged_softmax_rows of ragged_maps.hip over the C valid columns of the Cp-wide rows, scaled by beta, zeros behind.
//   cam_apply16_kernel    y = rne(attn . X + x): attn (fp32, beta folded in by the softmax) split into bf16 hi / lo in the staging, X the
//                         K = channel operand read TRANSPOSED from the [channel][pixel] LDS tile (ds_read_b64_tr_b16): bf16 x in two
//                         MFMAs (lo.x, hi.x), fp16 x on its planes in three (lo.xh, hi.xl, hi.xh).  The residual is read from x at the
//                         store (the tile holds the K rows, not the output rows), added in fp32, one rounding to nearest even.
//   conv1x1_tokens16_kernel   tokens[b, p, o] = sum_c x[b, c, p] w[o, c] + bias[o] (fp32 rows): the same tile with x as the A operand,
//                         the fp32 weights split hi / lo.  Always this strict-class form.
//   tokens_to_nchw_axpy16_kernel   the 32 x 32 transposing tile of sk_dual.hip with 16-bit x loads and y stores.
//
// Any B, C, H, W >= 1 without a staged copy of x: rows of x are 16-byte aligned only when H*W % 8 == 0, so the x loads come in three widths
// (vec = 8: 16-byte pieces, 4: 8-byte pieces for H*W % 8 == 4, 1: guarded 2-byte loads, DANet's 65 x 65 among them); pad rows / columns of
// every tile are ZERO-FILLED in the staging, never handled by divergent reads, and y is stored element by element.
//
// Transposed read (EXEC is all ones: every workgroup is 256 threads and no lane leaves before the last MFMA; every address is 8-byte
// aligned and inside the tile).  K order inside a 32-step is PERMUTED so that one read instruction of a 32-lane half covers 8 consecutive
// tile rows: lane l (g = l >> 4) holds k = 4g + [0,4) in elements 0..3 and k = 16 + 4g + [0,4) in elements 4..7; the fp32-side operand
// is read in the same order (two 8-byte reads).
// LDS banks (bank = (addr / 4) % 64 for these reads, per 32-lane half):
//   x tile      [32 k][80] 16-bit, 160-byte rows = 40 dwords: a half reads 8 rows x 32 bytes, 40 r mod 64 = 0, 40, 16, 56, 32, 8, 48, 24
//               for r = 0..7 -> eight disjoint 8-dword windows: conflict-free.
//   attn / w    [64][40] bf16, 80-byte rows = 20 dwords: a half reads 16 rows x (2 lanes x 2 dwords); 20 r mod 64 takes 16 distinct
//               multiples of 4 for r = 0..15 -> conflict-free.
//   Gram tiles  [64][72] 16-bit, 144-byte rows = 36 dwords, 16-byte row reads: the 16 rows of a 16-lane group start at 36 r mod 64 =
//               16 distinct multiples of 4 and cover the 64 banks once.
// (The staging writes were not analysed.)
//
// Range contract (tests/test_range_audit_cpu.py): this file converts fp32 to 16 bit but calls no rg_report and takes no range_word(): the
// MFMA operands it converts are bf16 planes (fp32 range, common.h "fp16 range guard"), and the fp16 conversions are OUTPUTS at their one
// store.  |attn . x| <= |beta| max|x|, so |y| <= (1 + |beta|) max|x|: an fp16 y beyond 65504 is inf exactly where the fp32 result
// rounded to fp16 is, and nothing is reported (the contract of mi355_bam16_fwd).
#include "common.h"
#include "io16.h"
#include "mma.h"

namespace {

typedef short s4 __attribute__((ext_vector_type(4)));
typedef short s8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s4 lds_s4;

constexpr int XP = 80;      // x tile: 64 pixels + 16 pad, elements
constexpr int WP = 40;      // attn / weight tile: 32 k + 8 pad, elements
constexpr int GP = 72;      // Gram tiles: 64 pixels + 8 pad, elements

// 8 consecutive 16-bit elements of a row (null: a pad row) from pixel p0 (a multiple of 8), zeros at and beyond HW
template <int VEC>
__device__ __forceinline__ u32x4 load8(const u16* __restrict__ row, long p0, long HW) {
    u32x4 r = {0u, 0u, 0u, 0u};
    if (!row) return r;
    if constexpr (VEC == 8) {
        if (p0 < HW) r = *reinterpret_cast<const u32x4*>(row + p0);
    } else if constexpr (VEC == 4) {
        if (p0 < HW) { const u32x2 a = *reinterpret_cast<const u32x2*>(row + p0); r.x = a.x; r.y = a.y; }
        if (p0 + 4 < HW) { const u32x2 a = *reinterpret_cast<const u32x2*>(row + p0 + 4); r.z = a.x; r.w = a.y; }
    } else {
        u32 h[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (p0 + e < HW) ? (u32)row[p0 + e] : 0u;
        r = u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
    }
    return r;
}

// one fp16 value -> its bf16 planes; an inf / NaN keeps lo = 0 (inf - inf would turn an inf into a NaN)
__device__ __forceinline__ void split_h1(u32 h, u32& hi, u32& lo) {
    const float v = (float)__builtin_bit_cast(_Float16, (u16)h);
    const __bf16 a = (__bf16)v;
    const __bf16 d = (__bf16)(v - (float)a);
    hi = __builtin_bit_cast(u16, a);
    lo = ((h & 0x7c00u) == 0x7c00u) ? 0u : (u32)__builtin_bit_cast(u16, d);
}
__device__ __forceinline__ void split_h8(u32x4 raw, u32x4& hi, u32x4& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        u32 h0, l0, h1, l1;
        split_h1(raw[i] & 0xffffu, h0, l0);
        split_h1(raw[i] >> 16, h1, l1);
        hi[i] = h0 | (h1 << 16);
        lo[i] = l0 | (l1 << 16);
    }
}
// a 16-byte piece of x into the tile's plane(s) at `off` elements: bf16 as it lies, fp16 as hi / lo
template <int IO>
__device__ __forceinline__ void put_x(u16* plane0, int plane_stride, int off, u32x4 raw) {
    if constexpr (IO == 1) {
        u32x4 hi, lo;
        split_h8(raw, hi, lo);
        *reinterpret_cast<u32x4*>(plane0 + off) = hi;
        *reinterpret_cast<u32x4*>(plane0 + plane_stride + off) = lo;
    } else {
        *reinterpret_cast<u32x4*>(plane0 + off) = raw;
    }
}
// four fp32 values of the other operand into its hi / lo planes (the strict idiom of mma.h)
__device__ __forceinline__ void put_w(u16* hi_row, u16* lo_row, int off, f4 v) {
    const b4 h = Mma<0>::cvt(v), l = Mma<0>::cvt_lo(v, h);
    *reinterpret_cast<u32x2*>(hi_row + off) = __builtin_bit_cast(u32x2, h);
    *reinterpret_cast<u32x2*>(lo_row + off) = __builtin_bit_cast(u32x2, l);
}
// fragment of the fp32-side operand (row = its M or N index): k = 4g + [0,4) | 16 + 4g + [0,4)
__device__ __forceinline__ b8 wfrag(const u16* row, int g) {
    const u32x2 a = *reinterpret_cast<const u32x2*>(row + 4 * g);
    const u32x2 b = *reinterpret_cast<const u32x2*>(row + 16 + 4 * g);
    return __builtin_bit_cast(b8, u32x4{a.x, a.y, b.x, b.y});
}
// fragment of x for the 16 pixels from n0 (a multiple of 16) of a [32 k][XP] plane, in the same k order: lane 4q + p of a 16-lane group
// addresses row q, columns 4p .. 4p + 3 of its group's 4 x 16 block and receives column (lane & 15), rows 0..3
__device__ __forceinline__ b8 xfrag(const u16* plane, int n0, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const u16* a = plane + (4 * g + q) * XP + n0 + 4 * p;
    const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)a);
    const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(a + 16 * XP));
    return __builtin_bit_cast(b8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// acc += x . w in the strict class: x exact on NP planes, w = wh + wl.  X_IS_A: x is the A operand (conv), else the B operand (apply)
template <int NP, bool X_IS_A>
__device__ __forceinline__ f4 strict_mma(const b8* xf, b8 wh, b8 wl, f4 acc) {
    if constexpr (X_IS_A) {
        acc = Mma<2>::mma(xf[0], wl, acc);
        if constexpr (NP == 2) acc = Mma<2>::mma(xf[1], wh, acc);
        return Mma<2>::mma(xf[0], wh, acc);
    } else {
        acc = Mma<2>::mma(wl, xf[0], acc);
        if constexpr (NP == 2) acc = Mma<2>::mma(wh, xf[1], acc);
        return Mma<2>::mma(wh, xf[0], acc);
    }
}

// ---- G[b] = X X^T: 64 x 64 tiles (tj >= ti), 4 waves of 32 x 32, K = 64 pixels per stage ----------------------------------------------
template <int IO, int VEC>
__global__ __launch_bounds__(256) void cam_gram16_kernel(const u16* __restrict__ x, float* __restrict__ G, int C, int Cp, long HW) {
    using M = Mma<IO>;
    __shared__ __attribute__((aligned(16))) u16 As[64][GP];
    __shared__ __attribute__((aligned(16))) u16 Bs[64][GP];
    const int ti = blockIdx.y, tj = blockIdx.x, b = blockIdx.z;
    if (tj < ti) return;                                           // the whole workgroup: the mirror tile stores this one
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1, g = lane >> 4, li = lane & 15;
    const u16* xb = x + (long)b * C * HW;
    f4 acc[2][2] = {};
    for (long p0 = 0; p0 < HW; p0 += 64) {
#pragma unroll
        for (int q = t; q < 512; q += 256) {
            const int row = q >> 3, c8 = (q & 7) * 8;
            const int ia = ti * 64 + row, ib = tj * 64 + row;
            *reinterpret_cast<u32x4*>(&As[row][c8]) = load8<VEC>(ia < C ? xb + (long)ia * HW : nullptr, p0 + c8, HW);
            *reinterpret_cast<u32x4*>(&Bs[row][c8]) = load8<VEC>(ib < C ? xb + (long)ib * HW : nullptr, p0 + c8, HW);
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            typename M::v8 a[2], bf[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                a[m] = *reinterpret_cast<const typename M::v8*>(&As[wm * 32 + m * 16 + li][ks * 32 + 8 * g]);
                bf[m] = *reinterpret_cast<const typename M::v8*>(&Bs[wn * 32 + m * 16 + li][ks * 32 + 8 * g]);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = M::mma(a[m], bf[n], acc[m][n]);
        }
        __syncthreads();
    }
    float* Gb = G + (long)b * Cp * Cp;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = ti * 64 + wm * 32 + m * 16 + g * 4 + r, gj = tj * 64 + wn * 32 + n * 16 + li;
                if (gi < Cp && gj < Cp) {
                    Gb[(long)gi * Cp + gj] = acc[m][n][r];
                    if (ti != tj) Gb[(long)gj * Cp + gi] = acc[m][n][r];
                }
            }
}

// ---- y[b, i, p] = rne(sum_j attn[b, i, j] x[b, j, p] + x[b, i, p]): 64 channels x 64 pixels per workgroup, K = 32 channels per stage ---
template <int IO, int VEC>
__global__ __launch_bounds__(256) void cam_apply16_kernel(const u16* __restrict__ x, const float* __restrict__ attn, u16* __restrict__ y,
                                                         int C, int Cp, long HW) {
    constexpr int NP = IO == 1 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) u16 Ws[2][64][WP];
    __shared__ __attribute__((aligned(16))) u16 Xs[NP][32][XP];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1, g = lane >> 4, li = lane & 15;
    const int b = blockIdx.z, i0 = blockIdx.y * 64;
    const long p0 = (long)blockIdx.x * 64;
    const u16* xb = x + (long)b * C * HW;
    const float* ab = attn + (long)b * Cp * Cp;
    f4 acc[2][2] = {};
    for (int j0 = 0; j0 < Cp; j0 += 32) {
#pragma unroll
        for (int q = t; q < 512; q += 256) {
            const int row = q >> 3, c4 = (q & 7) * 4;
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (i0 + row < C) v = *reinterpret_cast<const f4*>(ab + (long)(i0 + row) * Cp + j0 + c4);
            put_w(&Ws[0][row][0], &Ws[1][row][0], c4, v);
        }
        {
            const int row = t >> 3, c8 = (t & 7) * 8, j = j0 + row;
            put_x<IO>(&Xs[0][0][0], 32 * XP, row * XP + c8, load8<VEC>(j < C ? xb + (long)j * HW : nullptr, p0 + c8, HW));
        }
        __syncthreads();
        b8 xf[2][NP];
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) xf[n][pl] = xfrag(&Xs[pl][0][0], wn * 32 + n * 16, lane);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int row = wm * 32 + m * 16 + li;
            const b8 ah = wfrag(&Ws[0][row][0], g), al = wfrag(&Ws[1][row][0], g);
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[m][n] = strict_mma<NP, false>(xf[n], ah, al, acc[m][n]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wm * 32 + m * 16 + g * 4 + r;
                const long p = p0 + wn * 32 + n * 16 + li;
                if (i < C && p < HW) {
                    const long o = ((long)b * C + i) * HW + p;
                    y[o] = to16<IO>(acc[m][n][r] + from16<IO>(x[o]));
                }
            }
}

// ---- tokens[b, p, o] = sum_c x[b, c, p] w[o, c] + bias[o]: 64 pixels of ONE image x 64 outputs per workgroup, K = 32 channels per stage -
template <int IO, int VEC>
__global__ __launch_bounds__(256) void conv1x1_tokens16_kernel(const u16* __restrict__ x, const float* __restrict__ wt,
                                                              const float* __restrict__ bias, float* __restrict__ y, int Cin, long HW,
                                                              int Cout, int ldw) {
    constexpr int NP = IO == 1 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) u16 Ws[2][64][WP];
    __shared__ __attribute__((aligned(16))) u16 Xs[NP][32][XP];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1, g = lane >> 4, li = lane & 15;
    const int b = blockIdx.z, o0 = blockIdx.y * 64;
    const long p0 = (long)blockIdx.x * 64;
    const u16* xb = x + (long)b * Cin * HW;
    f4 acc[2][2] = {};
    for (int j0 = 0; j0 < Cin; j0 += 32) {
#pragma unroll
        for (int q = t; q < 512; q += 256) {
            const int row = q >> 3, c4 = (q & 7) * 4;
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (o0 + row < Cout && j0 + c4 + 4 <= ldw) v = *reinterpret_cast<const f4*>(wt + (long)(o0 + row) * ldw + j0 + c4);
            put_w(&Ws[0][row][0], &Ws[1][row][0], c4, v);
        }
        {
            const int row = t >> 3, c8 = (t & 7) * 8, j = j0 + row;
            put_x<IO>(&Xs[0][0][0], 32 * XP, row * XP + c8, load8<VEC>(j < Cin ? xb + (long)j * HW : nullptr, p0 + c8, HW));
        }
        __syncthreads();
        b8 xf[2][NP];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) xf[m][pl] = xfrag(&Xs[pl][0][0], wm * 32 + m * 16, lane);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int row = wn * 32 + n * 16 + li;
            const b8 wh = wfrag(&Ws[0][row][0], g), wl = wfrag(&Ws[1][row][0], g);
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[m][n] = strict_mma<NP, true>(xf[m], wh, wl, acc[m][n]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int o = o0 + wn * 32 + n * 16 + li;
            const float bo = (bias && o < Cout) ? bias[o] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long p = p0 + wm * 32 + m * 16 + g * 4 + r;
                if (o < Cout && p < HW) y[((long)b * HW + p) * Cout + o] = acc[m][n][r] + bo;
            }
        }
}

// ---- PAM epilogue on 16-bit x / y: y[b, c, p] = rne(alpha[0] * tok[b, p, c] + x[b, c, p]); 32 x 32 tiles through LDS --------------------
template <int IO>
__global__ __launch_bounds__(256) void tokens_to_nchw_axpy16_kernel(const float* __restrict__ tok, const u16* __restrict__ x,
                                                                   const float* __restrict__ alpha, u16* __restrict__ y, long HW, int C,
                                                                   long ldt) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
    const long p0 = (long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const float* tb = tok + (long)b * HW * ldt;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long p = p0 + ty + r * 8;
        const int c = c0 + tx;
        tile[ty + r * 8][tx] = (p < HW && c < C) ? tb[p * ldt + c] : 0.f;
    }
    __syncthreads();
    const float a = alpha ? alpha[0] : 1.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = c0 + ty + r * 8;
        const long p = p0 + tx;
        if (c < C && p < HW) {
            const long o = ((long)b * C + c) * HW + p;
            y[o] = to16<IO>(a * tile[tx][ty + r * 8] + (x ? from16<IO>(x[o]) : 0.f));
        }
    }
}

// widest x load the shape and the pointer allow: 16-byte pieces, 8-byte pieces, single elements
int x_vec(const void* x, long HW) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(x);
    return ((HW & 7) == 0 && (a & 15) == 0) ? 8 : ((HW & 3) == 0 && (a & 7) == 0) ? 4 : 1;
}
size_t round32(size_t n) { return (n + 31) & ~(size_t)31; }

#define IO_VEC_LAUNCH(KERNEL, GRID, ...)                                                     \
    do {                                                                                     \
        if (io == MI355_PREC_FP16) {                                                         \
            if (vec == 8) KERNEL<1, 8><<<GRID, 256, 0, st>>>(__VA_ARGS__);                   \
            else if (vec == 4) KERNEL<1, 4><<<GRID, 256, 0, st>>>(__VA_ARGS__);              \
            else KERNEL<1, 1><<<GRID, 256, 0, st>>>(__VA_ARGS__);                            \
        } else {                                                                             \
            if (vec == 8) KERNEL<2, 8><<<GRID, 256, 0, st>>>(__VA_ARGS__);                   \
            else if (vec == 4) KERNEL<2, 4><<<GRID, 256, 0, st>>>(__VA_ARGS__);              \
            else KERNEL<2, 1><<<GRID, 256, 0, st>>>(__VA_ARGS__);                            \
        }                                                                                    \
    } while (0)

}  // namespace

extern "C" {

size_t mi355_cam16_ws_bytes(int B, int C, int H, int W, int io) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (io != MI355_PREC_FP16 && io != MI355_PREC_BF16)) return 0;
    const size_t Cp = round32((size_t)C);
    return 4 * (size_t)B * Cp * Cp + 256;                         // the Gram matrices at pitch Cp; x is never copied
}

int mi355_cam_x16_fwd(const void* x, const float* beta, void* y, int B, int C, int H, int W, int io, void* workspace, size_t workspace_bytes,
                      mi355_stream_t stream) {
    MI355_CHECK_ARG(io == MI355_PREC_FP16 || io == MI355_PREC_BF16);
    MI355_CHECK_ARG(x && beta && y && workspace && B > 0 && C > 0 && H > 0 && W > 0);
    MI355_CHECK_ARG(workspace_bytes >= mi355_cam16_ws_bytes(B, C, H, W, io) && aligned16(workspace));
    const long HW = (long)H * W;
    const int Cp = (int)round32((size_t)C), tiles = cdiv(C, 64);
    if (B > 65535 || tiles > 65535)
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_cam_x16_fwd: B = %d or C = %d above the grid limits (65535 images, 65535 x 64 channels)", B, C);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const u16* xs = static_cast<const u16*>(x);
    float* G = static_cast<float*>(workspace);
    const int vec = x_vec(x, HW);
    {
        MI355_TRACE(st, "cam_gram16_kernel io=%d vec=%d C=%d HW=%ld", io, vec, C, HW);
        IO_VEC_LAUNCH(cam_gram16_kernel, dim3(tiles, tiles, B), xs, G, C, Cp, HW);
    }
    mi355::ragged_softmax_rows(G, B, C, C, Cp, (long)Cp * Cp, beta, st);
    {
        MI355_TRACE(st, "cam_apply16_kernel io=%d vec=%d C=%d HW=%ld", io, vec, C, HW);
        IO_VEC_LAUNCH(cam_apply16_kernel, dim3(cdiv(HW, 64), tiles, B), xs, G, static_cast<u16*>(y), C, Cp, HW);
    }
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}

int mi355_conv1x1_tokens16_fwd(const void* x, const float* w, const float* bias, float* y, int B, int Cin, int HW, int Cout, int ldw, int io,
                               mi355_stream_t stream) {
    MI355_CHECK_ARG(io == MI355_PREC_FP16 || io == MI355_PREC_BF16);
    MI355_CHECK_ARG(x && w && y && B > 0 && Cin > 0 && HW > 0 && Cout > 0);
    MI355_CHECK_ARG(ldw >= Cin && ldw % 4 == 0 && aligned16(w));
    if (B > 65535 || cdiv(Cout, 64) > 65535)
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_conv1x1_tokens16_fwd: B = %d or Cout = %d above the grid limits", B, Cout);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int vec = x_vec(x, HW);
    MI355_TRACE(st, "conv1x1_tokens16_kernel io=%d vec=%d Cin=%d Cout=%d HW=%d", io, vec, Cin, Cout, HW);
    IO_VEC_LAUNCH(conv1x1_tokens16_kernel, dim3(cdiv(HW, 64), cdiv(Cout, 64), B), static_cast<const u16*>(x), w, bias, y, Cin, (long)HW, Cout,
                  ldw);
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}

int mi355_tokens_to_nchw_axpy_x16_fwd(const float* tokens, const void* x, const float* alpha, void* y, int B, int HW, int C, long ld_tokens,
                                      int io, mi355_stream_t stream) {
    MI355_CHECK_ARG(io == MI355_PREC_FP16 || io == MI355_PREC_BF16);
    MI355_CHECK_ARG(tokens && y && B > 0 && HW > 0 && C > 0 && B <= 65535 && ld_tokens >= C);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(cdiv(HW, 32), cdiv(C, 32), B);
    MI355_TRACE(st, "tokens_to_nchw_axpy16_kernel io=%d C=%d HW=%d", io, C, HW);
    if (io == MI355_PREC_FP16)
        tokens_to_nchw_axpy16_kernel<1><<<grid, 256, 0, st>>>(tokens, static_cast<const u16*>(x), alpha, static_cast<u16*>(y), HW, C, ld_tokens);
    else
        tokens_to_nchw_axpy16_kernel<2><<<grid, 256, 0, st>>>(tokens, static_cast<const u16*>(x), alpha, static_cast<u16*>(y), HW, C, ld_tokens);
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}

}  // extern "C"
