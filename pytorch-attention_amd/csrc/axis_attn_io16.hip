// axis_attn_io16.hip -- the sweeps over x of CoordinateAttention / TripletAttention (AttentionGate) / BAM on 16-bit activations (IEEE half
// or bfloat16 in, the same type out) for gfx950: the four kernels of axis_attn.hip that touch x or y, with x and y in the I/O type.
//     chan_reduce16_kernel      reductions over C for every pixel      (1x1 conv to K planes, or ZPool = mean & max over channels)
//     plane_pool16(_lds)_kernel row and column mean (and max) of every (image, channel) plane
//     plane_dot16_kernel        plain per-plane sums                    (BAM's channel mean)
//     apply16_kernel<MODE>      the broadcast pass: 16-bit x, fp32 gates, 16-bit y
// Everything between them (pooled axes, the coordinate MLP, the gate convolutions, BAM's dilated stack) is fp32 in the workspace and runs
// on the kernels of axis_attn.hip unchanged; the entries (mi355_coordatt16_fwd, mi355_triplet16_fwd, mi355_attention_gate16_fwd,
// mi355_bam16_fwd) live there too and share one host body per gate with the fp32 entries; that body's io-switching launchers
// (chan_reduce, plane_pool, plane_dot, apply) reach this file through the mi355::axis16_* functions declared in common.h.
//
// All arithmetic is fp32 on the exactly widened inputs, in fixed orders; the only rounding the path adds is the one store of y, to
// nearest even.  Conversions go through io16.h only.
// Range contract (tests/test_range_audit_cpu.py): this file converts fp32 to 16 bit but calls no rg_report and takes no range_word() on
// purpose -- the converted values are OUTPUTS, never MFMA operands.  Triplet's and AttentionGate's gates are sigmoids in (0, 1), so
// |y| <= |x| and a finite x gives a finite y.  CoordinateAttention multiplies by two UNBOUNDED linear maps (the reference applies no
// sigmoid), and BAM's y = x (1 + sigmoid(.)) reaches 2|x|: there an fp16 y may overflow, and it is +-inf exactly where the fp32
// module's result rounded to fp16 is -- the overflow is the result's own, as for `m(x.float()).half()`, so nothing is reported and
// nothing re-runs.
//
// Two forms per kernel: 16-byte lanes (8 values per load; 8-byte lanes, 4 values, for the 16- and 32-plane channel reductions, whose
// accumulators would not fit beside 8 pixels) when the row length allows and the pointers are 16-byte aligned, 2-byte lanes for any
// shape and any 2-byte-aligned pointer.
#include "common.h"
#include "io16.h"

namespace {

using mi355::AP_COORD;
using mi355::AP_TRIPLET;
using mi355::AP_BAM;
using mi355::AP_SPATIAL;

typedef float v8f __attribute__((ext_vector_type(8)));

// VEC consecutive pixels of one channel: the fp32 vector a thread accumulates, how it is loaded from 16-bit x and stored to an fp32 plane
template <int IO, int VEC> struct Pix16;
template <int IO> struct Pix16<IO, 8> {
    using V = v8f;
    static __device__ __forceinline__ V load(const u16* p) {
        const u32x4 r = *reinterpret_cast<const u32x4*>(p);
        return V{lo16<IO>(r.x), hi16<IO>(r.x), lo16<IO>(r.y), hi16<IO>(r.y), lo16<IO>(r.z), hi16<IO>(r.z), lo16<IO>(r.w), hi16<IO>(r.w)};
    }
    static __device__ __forceinline__ void store(float* p, V v) {
        *reinterpret_cast<v4f*>(p) = __builtin_shufflevector(v, v, 0, 1, 2, 3);
        *reinterpret_cast<v4f*>(p + 4) = __builtin_shufflevector(v, v, 4, 5, 6, 7);
    }
    static __device__ __forceinline__ V splat(float s) { return V{s, s, s, s, s, s, s, s}; }
};
template <int IO> struct Pix16<IO, 4> {
    using V = v4f;
    static __device__ __forceinline__ V load(const u16* p) { return up4<IO>(*reinterpret_cast<const u32x2*>(p)); }
    static __device__ __forceinline__ void store(float* p, V v) { *reinterpret_cast<v4f*>(p) = v; }
    static __device__ __forceinline__ V splat(float s) { return V{s, s, s, s}; }
};
template <int IO> struct Pix16<IO, 1> {
    using V = float;
    static __device__ __forceinline__ V load(const u16* p) { return from16<IO>(*p); }
    static __device__ __forceinline__ void store(float* p, V v) { *p = v; }
    static __device__ __forceinline__ V splat(float s) { return s; }
};
__device__ __forceinline__ v8f vmaxf(v8f a, v8f b) {
    return v8f{fmaxf(a[0], b[0]), fmaxf(a[1], b[1]), fmaxf(a[2], b[2]), fmaxf(a[3], b[3]),
               fmaxf(a[4], b[4]), fmaxf(a[5], b[5]), fmaxf(a[6], b[6]), fmaxf(a[7], b[7])};
}
__device__ __forceinline__ v4f vmaxf(v4f a, v4f b) { return v4f{fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)}; }
__device__ __forceinline__ float vmaxf(float a, float b) { return fmaxf(a, b); }

// ---- reductions over the channel axis: chan_reduce_kernel of axis_attn.hip on a 16-bit x, fp32 planes out ------------------------------
// MODE 0: out[b, k, p] = bias[k] + sum_c w[k*C + c] * x[b, c, p]  for k < K (K <= KMAX)
// MODE 1: out[b, 0, p] = mean_c x[b, c, p],  out[b, 1, p] = max_c x[b, c, p]
// Same channel order as the fp32 kernel, so the two paths differ by nothing but the widening: U loads in flight, ragged C re-loads the last
// channel with weight 0 (-inf for the max), KMAX == 1 walks eight channel groups starting at group b mod 8 and combines the eight partials
// in a fixed order (a result does not depend on the batch index).
template <int IO, int MODE, int KMAX, int VEC>
__global__ __launch_bounds__(256) void chan_reduce16_kernel(const u16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ out, int C, long HW, int K) {
    using P = Pix16<IO, VEC>;
    using V = typename P::V;
    const long p_raw = ((long)blockIdx.x * 256 + threadIdx.x) * VEC;
    const bool live = p_raw < HW;
    const long p = live ? p_raw : 0;                             // idle threads shadow pixel 0 (they take part in the LDS staging barrier)
    const int b = blockIdx.y;
    const u16* xp = x + (long)b * C * HW + p;
    constexpr int NA = MODE == 0 ? KMAX : 2;
    constexpr int U = (MODE == 0 && KMAX >= 16) ? 4 : 8;
    V acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = P::splat((MODE == 1 && k == 1) ? -INFINITY : 0.f);
    extern __shared__ __attribute__((aligned(16))) float wl[];   // [c][KMAX], zero rows past K
    if constexpr (MODE == 0 && KMAX >= 4) {
        for (int q = threadIdx.x; q < C * KMAX; q += 256) {
            const int c = q / KMAX, k = q - c * KMAX;
            wl[q] = k < K ? w[(long)k * C + c] : 0.f;
        }
        __syncthreads();
    }
    auto sweep = [&](int cbeg, int cend) {                       // channels [cbeg, cend) into acc, U loads in flight
        for (int c = cbeg; c < cend; c += U) {
            V v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = P::load(xp + (long)(c + u < cend ? c + u : cend - 1) * HW);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = c + u < cend;
                if constexpr (MODE == 0 && KMAX >= 4) {
                    if (in) {
                        const v4f* wr = reinterpret_cast<const v4f*>(wl + (c + u) * KMAX);
#pragma unroll
                        for (int k4 = 0; k4 < KMAX / 4; ++k4) {
                            const v4f wk = wr[k4];
                            acc[k4 * 4 + 0] += wk.x * v[u]; acc[k4 * 4 + 1] += wk.y * v[u];
                            acc[k4 * 4 + 2] += wk.z * v[u]; acc[k4 * 4 + 3] += wk.w * v[u];
                        }
                    }
                } else if constexpr (MODE == 0) {
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) {
                        const float wk = (k < K && in) ? w[(long)k * C + c + u] : 0.f;
                        acc[k] += wk * v[u];
                    }
                } else {
                    acc[0] += in ? v[u] : P::splat(0.f);
                    acc[1] = vmaxf(acc[1], in ? v[u] : P::splat(-INFINITY));
                }
            }
        }
    };
    if constexpr (KMAX == 1) {
        constexpr int G = 8;
        const int gs = ((C + G - 1) / G + U - 1) / U * U;
        V part[G][NA];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int k = 0; k < NA; ++k) part[g][k] = P::splat((MODE == 1 && k == 1) ? -INFINITY : 0.f);
        for (int step = 0; step < G; ++step) {
            const int g = (b + step) & (G - 1);
            const int cbeg = g * gs, cend = cbeg + gs < C ? cbeg + gs : C;
#pragma unroll
            for (int k = 0; k < NA; ++k) acc[k] = P::splat((MODE == 1 && k == 1) ? -INFINITY : 0.f);
            if (cbeg < cend) sweep(cbeg, cend);
#pragma unroll
            for (int q = 0; q < G; ++q)
#pragma unroll
                for (int k = 0; k < NA; ++k) part[q][k] = q == g ? acc[k] : part[q][k];
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            if (MODE == 1 && k == 1)
                acc[k] = vmaxf(vmaxf(vmaxf(part[0][k], part[1][k]), vmaxf(part[2][k], part[3][k])),
                               vmaxf(vmaxf(part[4][k], part[5][k]), vmaxf(part[6][k], part[7][k])));
            else
                acc[k] = ((part[0][k] + part[1][k]) + (part[2][k] + part[3][k])) + ((part[4][k] + part[5][k]) + (part[6][k] + part[7][k]));
        }
    } else {
        sweep(0, C);
    }
    const int nout = MODE == 0 ? K : 2;
    float* op = out + (long)b * nout * HW + p;
    if (!live) return;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        if (k < nout) {
            V r;
            if constexpr (MODE == 0) r = acc[k] + P::splat(bias ? bias[k] : 0.f);
            else                     r = k == 0 ? acc[0] / (float)C : acc[1];
            P::store(op + (long)k * HW, r);
        }
    }
}

template <int IO, int MODE, int KMAX>
void launch_chan_reduce16(const u16* x, const float* w, const float* bias, float* out, int B, int C, long HW, int K, hipStream_t st) {
    constexpr int WIDE = (MODE == 0 && KMAX >= 16) ? 4 : 8;      // pixels per thread of the wide form: no instantiation has scratch
    const bool vec = (HW & 7) == 0 && aligned16(x) && aligned16(out);
    const size_t lds = (MODE == 0 && KMAX >= 4) ? (size_t)C * KMAX * sizeof(float) : 0;
    MI355_TRACE(st, "chan_reduce16_kernel io=%d mode=%d kmax=%d vec=%d", IO, MODE, KMAX, vec ? WIDE : 1);
    if (vec) chan_reduce16_kernel<IO, MODE, KMAX, WIDE><<<dim3(cdiv(HW / WIDE, 256), B), 256, lds, st>>>(x, w, bias, out, C, HW, K);
    else     chan_reduce16_kernel<IO, MODE, KMAX, 1><<<dim3(cdiv(HW, 256), B), 256, lds, st>>>(x, w, bias, out, C, HW, K);
}

// ---- reductions over W (one value per row) and over H (one value per column) of every (image, channel) plane ---------------------------
// plane_pool_kernel of axis_attn.hip: one wave per plane, lanes along a row (NCH chunks of 64 columns), rows of loads in flight.
template <int IO, bool WITH_MAX, int NCH>
__global__ __launch_bounds__(256) void plane_pool16_kernel(const u16* __restrict__ x, float* __restrict__ h_mean, float* __restrict__ h_max,
                                                          float* __restrict__ w_mean, float* __restrict__ w_max, long planes, int H, int W) {
    const int lane = threadIdx.x & 63;
    const long plane = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const u16* xp = x + plane * (long)H * W;
    float csum[NCH], cmax[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) { csum[ch] = 0.f; cmax[ch] = -INFINITY; }
    float keep_s = 0.f, keep_m = 0.f;
    const float inv_w = 1.f / (float)W, inv_h = 1.f / (float)H;
    constexpr int RU = NCH == 1 ? 8 : 4;
    for (int i0 = 0; i0 < H; i0 += RU) {
        float v[RU][NCH];
#pragma unroll
        for (int r = 0; r < RU; ++r)
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const int j = ch * 64 + lane;
                v[r][ch] = (i0 + r < H && j < W) ? from16<IO>(xp[(long)(i0 + r) * W + j]) : 0.f;
            }
#pragma unroll
        for (int r = 0; r < RU; ++r) {
            const int i = i0 + r;
            if (i >= H) break;
            float rs = 0.f, rm = -INFINITY;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const bool in = ch * 64 + lane < W;
                csum[ch] += v[r][ch];
                rs += v[r][ch];
                if constexpr (WITH_MAX) {
                    const float vm = in ? v[r][ch] : -INFINITY;
                    cmax[ch] = fmaxf(cmax[ch], vm);
                    rm = fmaxf(rm, vm);
                }
            }
            rs = wave_sum(rs);
            if constexpr (WITH_MAX) rm = wave_max(rm);
            if (lane == (i & 63)) { keep_s = rs * inv_w; keep_m = rm; }
            if ((i & 63) == 63 || i == H - 1) {
                const int base = i & ~63;
                if (base + lane <= i) {
                    h_mean[plane * H + base + lane] = keep_s;
                    if constexpr (WITH_MAX) h_max[plane * H + base + lane] = keep_m;
                }
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int j = ch * 64 + lane;
        if (j < W) {
            w_mean[plane * W + j] = csum[ch] * inv_h;
            if constexpr (WITH_MAX) w_max[plane * W + j] = cmax[ch];
        }
    }
}

// Planes that fit LDS as fp32 (H * (W + 1) floats <= 64 KB): one workgroup per plane streams the 16-bit plane in (16-byte loads when
// W % 8 == 0), parks it widened in LDS with the odd pitch, then half of the threads reduce rows and the other half columns.
template <int IO, bool WITH_MAX, int VEC>
__global__ __launch_bounds__(256) void plane_pool16_lds_kernel(const u16* __restrict__ x, float* __restrict__ h_mean, float* __restrict__ h_max,
                                                              float* __restrict__ w_mean, float* __restrict__ w_max, int H, int W) {
    extern __shared__ float tile[];
    const long plane = blockIdx.x;
    const int t = threadIdx.x, pitch = W + 1;
    const u16* xp = x + plane * (long)H * W;
    if constexpr (VEC == 8) {
        const int w8 = W >> 3, n8 = H * w8;
        int row = t / w8, col = t - row * w8;
        const int drow = 256 / w8, dcol = 256 - drow * w8;
        for (int i = t; i < n8; i += 256) {
            const u32x4 r = *reinterpret_cast<const u32x4*>(xp + (long)i * 8);
            float* d = tile + row * pitch + col * 8;
            d[0] = lo16<IO>(r.x); d[1] = hi16<IO>(r.x); d[2] = lo16<IO>(r.y); d[3] = hi16<IO>(r.y);
            d[4] = lo16<IO>(r.z); d[5] = hi16<IO>(r.z); d[6] = lo16<IO>(r.w); d[7] = hi16<IO>(r.w);
            row += drow; col += dcol;
            if (col >= w8) { col -= w8; ++row; }
        }
    } else {
        const int n = H * W;
        int row = t / W, col = t - row * W;
        const int drow = 256 / W, dcol = 256 - drow * W;
        for (int i = t; i < n; i += 256) {
            tile[row * pitch + col] = from16<IO>(xp[i]);
            row += drow; col += dcol;
            if (col >= W) { col -= W; ++row; }
        }
    }
    __syncthreads();
    if (t < 128) {
        for (int r = t; r < H; r += 128) {
            const float* q = tile + r * pitch;
            float s = 0.f, m = -INFINITY;
            for (int j = 0; j < W; ++j) { s += q[j]; if constexpr (WITH_MAX) m = fmaxf(m, q[j]); }
            h_mean[plane * H + r] = s / (float)W;
            if constexpr (WITH_MAX) h_max[plane * H + r] = m;
        }
    } else {
        for (int j = t - 128; j < W; j += 128) {
            const float* q = tile + j;
            float s = 0.f, m = -INFINITY;
            for (int r = 0; r < H; ++r) { s += q[r * pitch]; if constexpr (WITH_MAX) m = fmaxf(m, q[r * pitch]); }
            w_mean[plane * W + j] = s / (float)H;
            if constexpr (WITH_MAX) w_max[plane * W + j] = m;
        }
    }
}

// the two forms, the limits and the refusal of launch_plane_pool (axis_attn.hip)
template <int IO, bool WITH_MAX>
int launch_plane_pool16(const u16* x, float* h_mean, float* h_max, float* w_mean, float* w_max, long planes, int H, int W, hipStream_t st) {
    const size_t lds = (size_t)H * (W + 1) * sizeof(float);
    if (lds <= 65536 && planes < (1L << 31)) {
        const bool vec = (W & 7) == 0 && aligned16(x);
        MI355_TRACE(st, "plane_pool16_lds_kernel io=%d max=%d vec=%d H=%d W=%d", IO, (int)WITH_MAX, vec ? 8 : 1, H, W);
        if (vec) plane_pool16_lds_kernel<IO, WITH_MAX, 8><<<(int)planes, 256, lds, st>>>(x, h_mean, h_max, w_mean, w_max, H, W);
        else     plane_pool16_lds_kernel<IO, WITH_MAX, 1><<<(int)planes, 256, lds, st>>>(x, h_mean, h_max, w_mean, w_max, H, W);
        return MI355_OK;
    }
    if (W > 256) return mi355::fail(MI355_EUNSUPPORTED, "axis pooling: W = %d > 256 with a plane larger than 64 KB", W);
    const int grid = cdiv(planes, 4);
    MI355_TRACE(st, "plane_pool16_kernel io=%d max=%d H=%d W=%d", IO, (int)WITH_MAX, H, W);
    if (W <= 64)       plane_pool16_kernel<IO, WITH_MAX, 1><<<grid, 256, 0, st>>>(x, h_mean, h_max, w_mean, w_max, planes, H, W);
    else if (W <= 128) plane_pool16_kernel<IO, WITH_MAX, 2><<<grid, 256, 0, st>>>(x, h_mean, h_max, w_mean, w_max, planes, H, W);
    else               plane_pool16_kernel<IO, WITH_MAX, 4><<<grid, 256, 0, st>>>(x, h_mean, h_max, w_mean, w_max, planes, H, W);
    return MI355_OK;
}

// ---- out[plane] = scale * sum_p x[plane, p] -- one wave per plane, four 16-byte loads in flight per lane, add8's order ------------------
// The 2-byte form walks the same chunks of 8 in the same order, so a sum does not depend on the alignment of x.
template <int IO, int VEC>
__global__ __launch_bounds__(256) void plane_dot16_kernel(const u16* __restrict__ x, float* __restrict__ out, long planes, long HW, float scale) {
    const int lane = threadIdx.x & 63;
    const long plane = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const u16* xp = x + plane * HW;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const long n8 = HW >> 3;
    for (long q0 = lane; q0 < n8; q0 += 256) {
        if constexpr (VEC == 8) {
            u32x4 a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long q = q0 + 64 * k < n8 ? q0 + 64 * k : q0;
                a[k] = *reinterpret_cast<const u32x4*>(xp + q * 8);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (q0 + 64 * k < n8) add8<IO>(a[k], s0, s1, s2, s3);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (q0 + 64 * k < n8) {
                    const u16* c = xp + (q0 + 64 * k) * 8;
                    s0 += from16<IO>(c[0]); s1 += from16<IO>(c[1]); s2 += from16<IO>(c[2]); s3 += from16<IO>(c[3]);
                    s0 += from16<IO>(c[4]); s1 += from16<IO>(c[5]); s2 += from16<IO>(c[6]); s3 += from16<IO>(c[7]);
                }
            }
        }
    }
    if constexpr (VEC == 1) {                                    // the H*W % 8 values behind the last whole chunk
        if (lane == 0)
            for (long q = n8 * 8; q < HW; ++q) s0 += from16<IO>(xp[q]);
    }
    const float s = wave_sum((s0 + s1) + (s2 + s3));
    if (lane == 0) out[plane] = s * scale;
}

// ---- the broadcast pass: apply_kernel of axis_attn.hip with a 16-bit x and y, one element group per thread ----------------------------
struct Apply16Args {
    const u16* x; u16* y;
    const float* a;      // COORD: a_h (B,C,H)   TRIPLET: s_ch (B,C,H)   BAM: channel gate (B,C)
    const float* b;      // COORD: a_w (B,C,W)   TRIPLET: s_cw (B,C,W)   BAM: spatial gate (B,HW)
    const float* c;      //                      TRIPLET: s_hw (B,HW)    SPATIAL: gate (B,HW)
    long total;          // B*C*HW / VEC
    int C, H, W;
};

template <int IO, int MODE, int VEC>
__global__ __launch_bounds__(256) void apply16_kernel(const Apply16Args g) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.total) return;
    const long HW = (long)g.H * g.W;
    const long per = HW / VEC;
    const long plane = idx / per;
    const long p = (idx - plane * per) * VEC;
    const int i = (int)(p / g.W), j = (int)(p - (long)i * g.W);
    const long img = plane / g.C;
    float xv[VEC], yv[VEC];
    const u16* xp = g.x + plane * HW + p;
    if constexpr (VEC == 8) {
        const u32x4 r = *reinterpret_cast<const u32x4*>(xp);
        xv[0] = lo16<IO>(r.x); xv[1] = hi16<IO>(r.x); xv[2] = lo16<IO>(r.y); xv[3] = hi16<IO>(r.y);
        xv[4] = lo16<IO>(r.z); xv[5] = hi16<IO>(r.z); xv[6] = lo16<IO>(r.w); xv[7] = hi16<IO>(r.w);
    } else {
        xv[0] = from16<IO>(xp[0]);
    }
    if constexpr (MODE == AP_COORD) {
        const float ah = g.a[plane * g.H + i];
#pragma unroll
        for (int e = 0; e < VEC; ++e) yv[e] = xv[e] * ah * g.b[plane * g.W + j + e];
    } else if constexpr (MODE == AP_TRIPLET) {
        const float s1 = g.a[plane * g.H + i];
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            yv[e] = (xv[e] * s1 + xv[e] * g.b[plane * g.W + j + e] + xv[e] * g.c[img * HW + p + e]) * (1.0f / 3.0f);
    } else if constexpr (MODE == AP_SPATIAL) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) yv[e] = xv[e] * g.c[img * HW + p + e];
    } else {
        const float cg = g.a[plane];
#pragma unroll
        for (int e = 0; e < VEC; ++e) yv[e] = xv[e] + xv[e] * sigmoidf_(cg + g.b[img * HW + p + e]);
    }
    u16* yp = g.y + plane * HW + p;
    if constexpr (VEC == 8)
        *reinterpret_cast<u32x4*>(yp) = u32x4{pack16<IO>(yv[0], yv[1]), pack16<IO>(yv[2], yv[3]), pack16<IO>(yv[4], yv[5]), pack16<IO>(yv[6], yv[7])};
    else {
        // hipcc otherwise folds the last product into the conversion (v_fma_mixlo_f16: one rounding of the exact product), and the 2-byte
        // form would differ from the 16-byte form, which rounds the fp32 product, in the last bit of rare elements
        asm volatile("" : "+v"(yv[0]));
        yp[0] = to16<IO>(yv[0]);
    }
}

template <int IO, int MODE>
void launch_apply16(Apply16Args g, int B, hipStream_t st) {
    const long n = (long)B * g.C * g.H * g.W;
    const bool vec = (g.W & 7) == 0 && aligned16(g.x) && aligned16(g.y);
    MI355_TRACE(st, "apply16_kernel io=%d mode=%d vec=%d", IO, MODE, vec ? 8 : 1);
    if (vec) { g.total = n / 8; apply16_kernel<IO, MODE, 8><<<cdiv(g.total, 256), 256, 0, st>>>(g); }
    else     { g.total = n;     apply16_kernel<IO, MODE, 1><<<cdiv(g.total, 256), 256, 0, st>>>(g); }
}

template <int IO>
void chan_reduce16_io(const u16* x, int mode, int kmax, const float* w, const float* bias, float* out, int B, int C, long HW, int K, hipStream_t st) {
    if (mode == 1)       launch_chan_reduce16<IO, 1, 1>(x, nullptr, nullptr, out, B, C, HW, 2, st);
    else if (kmax <= 4)  launch_chan_reduce16<IO, 0, 4>(x, w, bias, out, B, C, HW, K, st);
    else if (kmax <= 8)  launch_chan_reduce16<IO, 0, 8>(x, w, bias, out, B, C, HW, K, st);
    else if (kmax <= 16) launch_chan_reduce16<IO, 0, 16>(x, w, bias, out, B, C, HW, K, st);
    else                 launch_chan_reduce16<IO, 0, 32>(x, w, bias, out, B, C, HW, K, st);
}

template <int IO>
void apply16_io(int mode, const Apply16Args& g, int B, hipStream_t st) {
    if (mode == AP_COORD)        launch_apply16<IO, AP_COORD>(g, B, st);
    else if (mode == AP_TRIPLET) launch_apply16<IO, AP_TRIPLET>(g, B, st);
    else if (mode == AP_BAM)     launch_apply16<IO, AP_BAM>(g, B, st);
    else                         launch_apply16<IO, AP_SPATIAL>(g, B, st);
}

}  // namespace

// ---- what the io-switching launchers of axis_attn.hip call (io = 1: IEEE half, 2: bfloat16; validated by the entries there) ----------------
namespace mi355 {

void axis16_chan_reduce(const void* x, int io, int mode, int kmax, const float* w, const float* bias, float* out, int B, int C, long HW, int K,
                        hipStream_t st) {
    const u16* xs = static_cast<const u16*>(x);
    if (io == 1) chan_reduce16_io<1>(xs, mode, kmax, w, bias, out, B, C, HW, K, st);
    else         chan_reduce16_io<2>(xs, mode, kmax, w, bias, out, B, C, HW, K, st);
}

int axis16_plane_pool(const void* x, int io, bool with_max, float* h_mean, float* h_max, float* w_mean, float* w_max, long planes, int H, int W,
                      hipStream_t st) {
    const u16* xs = static_cast<const u16*>(x);
    if (io == 1) return with_max ? launch_plane_pool16<1, true>(xs, h_mean, h_max, w_mean, w_max, planes, H, W, st)
                                 : launch_plane_pool16<1, false>(xs, h_mean, h_max, w_mean, w_max, planes, H, W, st);
    return with_max ? launch_plane_pool16<2, true>(xs, h_mean, h_max, w_mean, w_max, planes, H, W, st)
                    : launch_plane_pool16<2, false>(xs, h_mean, h_max, w_mean, w_max, planes, H, W, st);
}

void axis16_plane_dot(const void* x, int io, float* out, long planes, long HW, float scale, hipStream_t st) {
    const u16* xs = static_cast<const u16*>(x);
    const bool vec = (HW & 7) == 0 && aligned16(x);
    MI355_TRACE(st, "plane_dot16_kernel io=%d vec=%d", io, vec ? 8 : 1);
    const int grid = cdiv(planes, 4);
    if (io == 1) {
        if (vec) plane_dot16_kernel<1, 8><<<grid, 256, 0, st>>>(xs, out, planes, HW, scale);
        else     plane_dot16_kernel<1, 1><<<grid, 256, 0, st>>>(xs, out, planes, HW, scale);
    } else {
        if (vec) plane_dot16_kernel<2, 8><<<grid, 256, 0, st>>>(xs, out, planes, HW, scale);
        else     plane_dot16_kernel<2, 1><<<grid, 256, 0, st>>>(xs, out, planes, HW, scale);
    }
}

void axis16_apply(int mode, const void* x, int io, void* y, const float* a, const float* b, const float* c, int B, int C, int H, int W,
                  hipStream_t st) {
    Apply16Args g{};
    g.x = static_cast<const u16*>(x); g.y = static_cast<u16*>(y); g.a = a; g.b = b; g.c = c; g.C = C; g.H = H; g.W = W;
    if (io == 1) apply16_io<1>(mode, g, B, st);
    else         apply16_io<2>(mode, g, B, st);
}

}  // namespace mi355
