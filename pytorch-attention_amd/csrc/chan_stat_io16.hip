// chan_stat_io16.hip -- simam_module / SRM / GaussianGCT / LCT / GCT on 16-bit activations (IEEE half or bfloat16 in, the same type out)
// for gfx950: chan_stat.hip with x and y in the I/O type.
//
// Parameters are fp32 and every piece of arithmetic (row sums, statistics, the exchange between workgroups, sigmoid / tanh / exp, the
// per-element SimAM gate, the products) is fp32; the only rounding the path adds is the one store of y, to nearest even.
// Range contract (tests/test_range_audit_cpu.py): this file converts fp32 to 16 bit but calls no rg_report and takes no range_word() on
// purpose -- the converted values are OUTPUTS, never MFMA operands.  The gates of SimAM, SRM, GaussianGCT and LCT lie in (0, 1], so
// |y| <= |x| and a finite x gives a finite y.  GCT is the exception: its gate 1 + tanh(.) lies in [0, 2], |y| can reach 2|x| and an fp16
// store may overflow.  The contract there is that y is +-inf exactly where the fp32 module's result, rounded to fp16, is: the overflow is
// the result's own, as it would be for `m(x.float()).half()`, so there is no range-word report and no strict re-run.
//
// Two forms, as in chan_stat.hip:
//   single read   stat_single_kernel's geometry (512 threads, 8 channel rows per workgroup, one per wave) with the row PACKED in
//                 registers as in se16_single_kernel (8 values per 16-byte load, unpacked to fp32 only for the sums and the products).
//                 GaussianGCT / LCT / GCT exchange one fp32 number per channel through the same tagged granules, ticket, epoch and
//                 error words.  H*W % 8 == 0, H*W <= 4096, C % 8 == 0, 16-byte aligned pointers, option "zoo_single".
//   general       any shape the fp32 entries accept: row statistics in fp32 from 16-bit loads, then gate + scale with a 16-bit store;
//                 16-byte lanes when H*W % 8 == 0 and the pointers allow, 2-byte lanes otherwise.  Correct everywhere, not tuned.
// Both accumulate in fixed orders.
#include "common.h"
#include "bufops.h"
#include "io16.h"
#include "chan_stat.h"

namespace {

typedef StatArgsT<u16> Stat16Args;

// Waves per SIMD the single-read kernel is compiled for, by mode and 16-byte chunks per lane (512 threads = 2 waves per SIMD and
// workgroup: 8 / 6 / 4 = four / three / two workgroups per CU at <= 64 / 80 / 128 VGPRs).  The launcher sizes its grid by the SAME
// function, so the workgroups it counts on are the ones the launch bounds guarantee (tests/test_zoo_io16_cpu.py pins the registers).
// The largest that compiles without scratch for every mode: beside the packed row (4 registers per chunk) a pass holds the eight fp32
// values of the chunks in flight, SimAM two transcendentals on each, SRM and l1-GCT a second form of the sums.
constexpr int stat16_nv(int nv) { return nv <= 1 ? 1 : (nv <= 2 ? 2 : (nv <= 4 ? 4 : (nv <= 7 ? 7 : 8))); }
constexpr int stat16_waves(int mode, int nv) { return mode == M_SIMAM ? (nv <= 4 ? 6 : 4) : (nv <= 2 ? 8 : (nv <= 4 ? 6 : 4)); }

// Between two passes over the packed row: without it hipcc keeps the fp32 values the first pass unpacked (8 per chunk) alive for the
// next one, which is the register-resident fp32 row this kernel exists to avoid (scratch at 7 and 8 chunks per lane).
// The scheduling barrier keeps the chunks of a pass from being interleaved (eight independent values per chunk are parallelism enough).
__device__ __forceinline__ void keep_packed(u32x4& r) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" : "+v"(r));
}

// sum of squares / of magnitudes of the 8 values of a chunk, in add8's order
template <int IO> __device__ __forceinline__ void sq8(u32x4 r, float& s0, float& s1, float& s2, float& s3) {
    float v;
    v = lo16<IO>(r.x); s0 += v * v; v = hi16<IO>(r.x); s1 += v * v; v = lo16<IO>(r.y); s2 += v * v; v = hi16<IO>(r.y); s3 += v * v;
    v = lo16<IO>(r.z); s0 += v * v; v = hi16<IO>(r.z); s1 += v * v; v = lo16<IO>(r.w); s2 += v * v; v = hi16<IO>(r.w); s3 += v * v;
}
template <int IO> __device__ __forceinline__ void abs8(u32x4 r, float& s0, float& s1, float& s2, float& s3) {
    s0 += fabsf(lo16<IO>(r.x)); s1 += fabsf(hi16<IO>(r.x)); s2 += fabsf(lo16<IO>(r.y)); s3 += fabsf(hi16<IO>(r.y));
    s0 += fabsf(lo16<IO>(r.z)); s1 += fabsf(hi16<IO>(r.z)); s2 += fabsf(lo16<IO>(r.w)); s3 += fabsf(hi16<IO>(r.w));
}
// sum of (v - mean)^2 over a chunk; a lane beyond the row (in == false) holds zeros and is parked on the mean, value by value
template <int IO> __device__ __forceinline__ void dev8(u32x4 r, bool in, float mean, float& q0, float& q1, float& q2, float& q3) {
    float d;
    d = (in ? lo16<IO>(r.x) : mean) - mean; q0 += d * d; d = (in ? hi16<IO>(r.x) : mean) - mean; q1 += d * d;
    d = (in ? lo16<IO>(r.y) : mean) - mean; q2 += d * d; d = (in ? hi16<IO>(r.y) : mean) - mean; q3 += d * d;
    d = (in ? lo16<IO>(r.z) : mean) - mean; q0 += d * d; d = (in ? hi16<IO>(r.z) : mean) - mean; q1 += d * d;
    d = (in ? lo16<IO>(r.w) : mean) - mean; q2 += d * d; d = (in ? hi16<IO>(r.w) : mean) - mean; q3 += d * d;
}
// SimAM: v * sigmoid(d^2 / den + 0.5) on the transcendental units, idn = -log2(e) / den, hb = -0.5 log2(e) (stat_single_kernel)
__device__ __forceinline__ float simam1(float v, float mean, float idn, float hb) {
    const float d = v - mean;
    return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(d * d * idn + hb));
}
template <int IO> __device__ __forceinline__ u32x4 simam8(u32x4 r, float mean, float idn, float hb) {
    return u32x4{pack16<IO>(simam1(lo16<IO>(r.x), mean, idn, hb), simam1(hi16<IO>(r.x), mean, idn, hb)),
                 pack16<IO>(simam1(lo16<IO>(r.y), mean, idn, hb), simam1(hi16<IO>(r.y), mean, idn, hb)),
                 pack16<IO>(simam1(lo16<IO>(r.z), mean, idn, hb), simam1(hi16<IO>(r.z), mean, idn, hb)),
                 pack16<IO>(simam1(lo16<IO>(r.w), mean, idn, hb), simam1(hi16<IO>(r.w), mean, idn, hb))};
}

// =====================================================================================================================================
// single read: stat_single_kernel of chan_stat.hip on packed rows (the same granules, ticket, epoch and error words)
// =====================================================================================================================================
template <int IO, int MODE, int NV>
__global__ __launch_bounds__(512, stat16_waves(MODE, NV)) void stat16_single_kernel(const Stat16Args a, const int nts) {
    extern __shared__ __attribute__((aligned(16))) float s_p[];       // exchange modes: the image's C published values
    __shared__ float s_red[32];
    __shared__ u32 s_tk[2];
    __shared__ u32 s_ok[2][8];
    __shared__ u32 s_ep;
    const int t0 = threadIdx.x;
    constexpr bool XCH = MODE >= M_GCTG;
    // launch state lives in the workspace (chan_stat.hip): tag = epoch + 1, total + gridDim.x draws per launch, the last one resets
    const u32 last_draw = (u32)a.total + gridDim.x - 1u;
    auto draw = [&](u32 ep) -> u32 {
        const u32 v = __hip_atomic_fetch_add(a.ticket, 1u, AGENT_RLX);
        if (v == last_draw) {
            __hip_atomic_store(a.ticket, 0u, AGENT_RLX);
            __hip_atomic_store(a.epoch, ep + 1u, AGENT_RLX);
        }
        return v;
    };
    u32 EP = 0u, TAG = 1u;
    if (XCH) {
        if (t0 == 0) {
            // acquire: the epoch cannot move until this workgroup has drawn its stop ticket, but only if the load really comes first
            const u32 ep = __hip_atomic_load(a.epoch, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            s_ep = ep;
            s_tk[0] = draw(ep);
        }
        __syncthreads();
        EP = __builtin_amdgcn_readfirstlane(s_ep);
        TAG = (EP + 1u) ? EP + 1u : 1u;                               // 0 is what a zeroed granule holds
    }
    int par = 0;
    u32 slice = blockIdx.x;
    for (;;) {
        const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
        u32 tk;
        if (XCH) {
            __syncthreads();
            tk = __builtin_amdgcn_readfirstlane(s_tk[par]);
        } else {
            tk = slice;                                               // no waiting between workgroups: a plain grid-stride walk
            slice += gridDim.x;
        }
        if (tk >= (u32)a.total) return;
        // the wave's channel as a scalar: its parameters then arrive by scalar loads instead of seven 64-bit lane addresses
        const int b = tk / a.gpi, c0 = (tk - b * a.gpi) * ECW, c = __builtin_amdgcn_readfirstlane(c0 + wave);
        // lanes beyond the row read zeros and their stores are dropped (range check of the descriptor): no predicates
        const u32 rlo = (u32)((b * a.C + c) & 0x7FFFFFFF);
        const long row = (long)rlo * a.HW;
        const rsrc_t rx = make_rsrc(a.x + row, (u32)a.HW * 2u), ry = make_rsrc(a.y + row, (u32)a.HW * 2u);
        const u32 voff = (u32)lane * 16u;
        u32x4 r[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) r[j] = __builtin_amdgcn_raw_buffer_load_b128(rx, voff, (u32)j * 1024u, 0);
        // ---- row statistics from the packed registers -----------------------------------------------------------------------
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (MODE == M_GCT2) {
#pragma unroll
            for (int j = 0; j < NV; ++j) sq8<IO>(r[j], s0, s1, s2, s3);
        } else if (MODE == M_GCT1 && !a.i0) {
#pragma unroll
            for (int j = 0; j < NV; ++j) abs8<IO>(r[j], s0, s1, s2, s3);
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) add8<IO>(r[j], s0, s1, s2, s3);
        }
        const float tot = wave_sum_sw((s0 + s1) + (s2 + s3));
        const float mean = tot / (float)a.HW;
        float cvs = 0.f;                                              // sum_hw (x - mean)^2  (SIMAM, SRM)
        if (MODE == M_SIMAM || MODE == M_SRM) {
            float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                // wave-uniform branch: only the last occupied slot(s) can be ragged, the full ones carry no selects; the registers stay
                // as loaded (the stores of the parked lanes are dropped anyway)
                keep_packed(r[j]);
                if (64 * (j + 1) <= a.nchunk) dev8<IO>(r[j], true, mean, q0, q1, q2, q3);
                else dev8<IO>(r[j], lane + 64 * j < a.nchunk, mean, q0, q1, q2, q3);
            }
            cvs = wave_sum_sw((q0 + q1) + (q2 + q3));
        }
        const float own = (MODE == M_GCT2 || MODE == M_GCT1) ? tot : mean;
        float red0 = 0.f, red1 = 0.f;
        if (XCH) {
            u64* gb = a.gran + (long)b * a.C;
            if (lane == 0) __hip_atomic_store(gb + c, ((u64)TAG << 32) | (u64)__float_as_uint(own), AGENT_RLX);
            u32 spins = 0;
            bool timeout = false;
            for (;;) {
                bool ok = true;
                for (int cc = t; cc < a.C; cc += 512) {
                    const u64 g = __hip_atomic_load(gb + cc, AGENT_RLX);
                    if ((u32)(g >> 32) == TAG) s_p[cc] = __uint_as_float((u32)g);
                    else ok = false;
                }
                const int vp = (int)(spins & 1u);                     // one-barrier AND of `ok` (chan_fused.hip se_single_kernel)
                const bool wave_ok = __builtin_amdgcn_ballot_w64(!ok) == 0ull;
                if (lane == 0) s_ok[vp][wave] = wave_ok ? 1u : 0u;
                __syncthreads();
                const u32 votes = s_ok[vp][0] & s_ok[vp][1] & s_ok[vp][2] & s_ok[vp][3] & s_ok[vp][4] & s_ok[vp][5] & s_ok[vp][6] & s_ok[vp][7];
                if (__builtin_amdgcn_readfirstlane(votes)) break;
                __builtin_amdgcn_s_sleep(2);
                if (++spins > a.spin) { timeout = true; break; }
            }
            if (t == 0) {                                             // nobody is waited for any more: next ticket
                s_tk[par ^ 1] = draw(EP);
                if (timeout) {
                    __hip_atomic_store(a.err, 1u, AGENT_RLX);
                    if (a.herr) __hip_atomic_store(a.herr, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
            if (MODE == M_LCT) group_reduce(s_p, c, a.i0, red0, red1);
            else image_reduce<MODE, 512>(a, s_p, s_red, red0, red1);
        }
        // ---- scale from registers, rounded once (the row step rides in the VGPR offset of the stores: cbam_single.hip) -----------
        u32 ob = voff;
        asm volatile("" : "+v"(ob));
        if (MODE == M_SIMAM) {
            const float idn = -1.44269504088896340736f / (4.0f * (cvs / (float)(a.HW - 1) + a.f0));
            const float hb = -0.5f * 1.44269504088896340736f;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                keep_packed(r[j]);
                const u32x4 o = simam8<IO>(r[j], mean, idn, hb);
                if (nts) __builtin_amdgcn_raw_buffer_store_b128(o, ry, ob + (u32)j * 1024u, 0, AUX_NT);
                else     __builtin_amdgcn_raw_buffer_store_b128(o, ry, ob + (u32)j * 1024u, 0, 0);
            }
        } else {
            const float g = gate_of<MODE>(a, c, mean, cvs, own, red0, red1);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                keep_packed(r[j]);
                const u32x4 o = scale8<IO>(r[j], g);
                if (nts) __builtin_amdgcn_raw_buffer_store_b128(o, ry, ob + (u32)j * 1024u, 0, AUX_NT);
                else     __builtin_amdgcn_raw_buffer_store_b128(o, ry, ob + (u32)j * 1024u, 0, 0);
            }
        }
        par ^= 1;
    }
}

// =====================================================================================================================================
// general form: row statistics -> gate + scale
// =====================================================================================================================================
// pass 1: stats[row] = {sum, sum (x-mean)^2, sum x^2, sum |x|} (the layout of row_stats_kernel), one wave per row, four rows per workgroup
template <int IO, bool VEC>
__global__ __launch_bounds__(256) void row_stats16_kernel(const u16* __restrict__ x, float* __restrict__ stats, long rows, int HW) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const u16* p = x + row * HW;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if constexpr (VEC) {
        const u32x4* p8 = reinterpret_cast<const u32x4*>(p);
        for (int i = lane; i < (HW >> 3); i += 64) {
            const u32x4 v = p8[i];
            add8<IO>(v, s0, s1, s2, s3); sq8<IO>(v, q0, q1, q2, q3); abs8<IO>(v, a0, a1, a2, a3);
        }
    } else {
        for (int i = lane; i < HW; i += 64) { const float v = from16<IO>(p[i]); s0 += v; q0 += v * v; a0 += fabsf(v); }
    }
    const float s = wave_sum((s0 + s1) + (s2 + s3)), q = wave_sum((q0 + q1) + (q2 + q3)), ab = wave_sum((a0 + a1) + (a2 + a3));
    const float mean = s / (float)HW;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
    if constexpr (VEC) {
        const u32x4* p8 = reinterpret_cast<const u32x4*>(p);
        for (int i = lane; i < (HW >> 3); i += 64) dev8<IO>(p8[i], true, mean, c0, c1, c2, c3);
    } else {
        for (int i = lane; i < HW; i += 64) { const float d = from16<IO>(p[i]) - mean; c0 += d * d; }
    }
    const float cv = wave_sum((c0 + c1) + (c2 + c3));
    if (lane == 0) { stats[row * 4] = s; stats[row * 4 + 1] = cv; stats[row * 4 + 2] = q; stats[row * 4 + 3] = ab; }
}

// pass 2: stat_apply_kernel of chan_stat.hip with 16-bit loads and stores (one 256-thread workgroup per image and 4 channels)
template <int IO, int MODE, bool VEC>
__global__ __launch_bounds__(256) void stat_apply16_kernel(const Stat16Args a, int groups, int nts) {
    extern __shared__ __attribute__((aligned(16))) float s_p[];
    __shared__ float s_red[32];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x / groups, c = (blockIdx.x % groups) * 4 + wave;
    const float* st = a.stats + (long)b * a.C * 4;
    float red0 = 0.f, red1 = 0.f;
    if (MODE >= M_GCTG) {
        for (int cc = t; cc < a.C; cc += 256) {
            const float sum = st[cc * 4], sq = st[cc * 4 + 2], ab = st[cc * 4 + 3];
            s_p[cc] = (MODE == M_GCT2) ? sq : (MODE == M_GCT1 ? (a.i0 ? sum : ab) : sum / (float)a.HW);
        }
        __syncthreads();
        if (MODE != M_LCT) image_reduce<MODE, 256>(a, s_p, s_red, red0, red1);
    }
    if (c >= a.C) return;
    if (MODE == M_LCT) group_reduce(s_p, c, a.i0, red0, red1);
    const float sum = st[c * 4], cvs = st[c * 4 + 1];
    const float mean = sum / (float)a.HW;
    const float own = (MODE >= M_GCTG) ? s_p[c] : mean;
    const long row = ((long)b * a.C + c) * a.HW;
    const float den = 4.0f * (cvs / (float)(a.HW - 1) + a.f0);                     // SimAM only
    const float g = (MODE == M_SIMAM) ? 1.0f : gate_of<MODE>(a, c, mean, cvs, own, red0, red1);
    auto one = [&](float v) -> float {
        if (MODE == M_SIMAM) { const float d = v - mean; return v * sigmoidf_(d * d / den + 0.5f); }
        return v * g;
    };
    if constexpr (VEC) {
        const u32x4* x8 = reinterpret_cast<const u32x4*>(a.x + row);
        u32x4* y8 = reinterpret_cast<u32x4*>(a.y + row);
        for (int i = lane; i < (a.HW >> 3); i += 64) {
            const u32x4 v = x8[i];
            const u32x4 o = {pack16<IO>(one(lo16<IO>(v.x)), one(hi16<IO>(v.x))), pack16<IO>(one(lo16<IO>(v.y)), one(hi16<IO>(v.y))),
                             pack16<IO>(one(lo16<IO>(v.z)), one(hi16<IO>(v.z))), pack16<IO>(one(lo16<IO>(v.w)), one(hi16<IO>(v.w)))};
            if (nts) __builtin_nontemporal_store(o, &y8[i]);
            else y8[i] = o;
        }
    } else {
        for (int i = lane; i < a.HW; i += 64) a.y[row + i] = to16<IO>(one(from16<IO>(a.x[row + i])));
    }
}

template <int IO, int MODE>
void go_single(int nv, int grid, size_t smem, hipStream_t st, const Stat16Args& a, int nts) {
    switch (stat16_nv(nv)) {
        case 1: stat16_single_kernel<IO, MODE, 1><<<grid, 512, smem, st>>>(a, nts); break;
        case 2: stat16_single_kernel<IO, MODE, 2><<<grid, 512, smem, st>>>(a, nts); break;
        case 4: stat16_single_kernel<IO, MODE, 4><<<grid, 512, smem, st>>>(a, nts); break;
        case 7: stat16_single_kernel<IO, MODE, 7><<<grid, 512, smem, st>>>(a, nts); break;
        default: stat16_single_kernel<IO, MODE, 8><<<grid, 512, smem, st>>>(a, nts);
    }
}

template <int IO, int MODE>
void go_general(bool vec, const Stat16Args& a, hipStream_t st, int nts) {
    constexpr bool XCH = MODE >= M_GCTG;
    const long rows = (long)a.B * a.C;
    {
        MI355_TRACE(st, "row_stats16_kernel io=%d HW=%d", IO, a.HW);
        if (vec) row_stats16_kernel<IO, true><<<cdiv(rows, 4), 256, 0, st>>>(a.x, a.stats, rows, a.HW);
        else     row_stats16_kernel<IO, false><<<cdiv(rows, 4), 256, 0, st>>>(a.x, a.stats, rows, a.HW);
    }
    const int groups = (a.C + 3) / 4;
    const size_t smem = XCH ? (size_t)a.C * 4 : 0;
    MI355_TRACE(st, "stat_apply16_kernel io=%d mode=%d C=%d HW=%d", IO, MODE, a.C, a.HW);
    if (vec) stat_apply16_kernel<IO, MODE, true><<<a.B * groups, 256, smem, st>>>(a, groups, nts);
    else     stat_apply16_kernel<IO, MODE, false><<<a.B * groups, 256, smem, st>>>(a, groups, nts);
}

// what every entry checks before any HIP call: io, sizes (32-bit row and grid arithmetic), then the common pointers and the workspace
#define CHECK_IO16(min_hw)                                                                                                 \
    do {                                                                                                                   \
        MI355_CHECK_ARG(io == 1 || io == 2);                                                                               \
        MI355_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && (long)H * W >= (min_hw));                                      \
        MI355_CHECK_ARG((long)B * C <= (1L << 31) - 8 && (long)H * W <= (1L << 30));                                       \
        MI355_CHECK_ARG(x && y && ws);                                                                                     \
        MI355_CHECK_ARG(ws_bytes >= mi355::zoo_workspace_bytes(B, C));                                                     \
    } while (0)

// what stat_run (chan_stat.h) needs to know about packed 16-bit rows
struct Stat16 {
    typedef Stat16Args Args;
    static constexpr const char* who = "channel-statistics gate (16-bit)";
    static constexpr int EPC = 8, MAX_NV = 8;
    static constexpr bool IO_IN_KEY = true;
    static bool vec(const Args& a) { return (a.HW % 8 == 0) && aligned16(a.x) && aligned16(a.y); }
    // workgroups per CU the grid counts on: what the launch bounds of the instantiation guarantee (every one runs at least two: <= 128
    // VGPRs, <= 48 KB of LDS), as far as the LDS allows
    template <int MODE> static int occ(int nv, size_t smem) {
        int n = stat16_waves(MODE, stat16_nv(nv)) / 2;
        while (n > 2 && (smem + 256) * n > 150 * 1024) --n;
        return n;
    }
    template <int MODE> static void single(int nv, int grid, size_t smem, hipStream_t st, const Args& a, int io, bool nts) {
        MI355_TRACE(st, "stat16_single_kernel io=%d mode=%d C=%d HW=%d nv=%d NV=%d", io, MODE, a.C, a.HW, nv, stat16_nv(nv));
        if (io == 1) go_single<1, MODE>(nv, grid, smem, st, a, nts ? 1 : 0);
        else         go_single<2, MODE>(nv, grid, smem, st, a, nts ? 1 : 0);
    }
    template <int MODE> static int general(bool vec, const Args& a, int io, hipStream_t st, bool nts) {
        if (MODE >= M_GCTG && (size_t)a.C * 4 > 48 * 1024) {
            const void* fn = io == 1 ? (vec ? (const void*)stat_apply16_kernel<1, MODE, true> : (const void*)stat_apply16_kernel<1, MODE, false>)
                                     : (vec ? (const void*)stat_apply16_kernel<2, MODE, true> : (const void*)stat_apply16_kernel<2, MODE, false>);
            if (int rc = mi355::func_dynamic_lds(fn, a.C * 4)) return rc;
        }
        if (io == 1) go_general<1, MODE>(vec, a, st, nts ? 1 : 0);
        else         go_general<2, MODE>(vec, a, st, nts ? 1 : 0);
        return MI355_OK;
    }
};

template <int MODE>
int run16(const Stat16Args& a, int io, int H, int W, void* ws, size_t ws_bytes, hipStream_t st) {
    return stat_run<MODE, Stat16>(a, io, H, W, ws, ws_bytes, st);
}

}  // namespace

extern "C" {

int mi355_simam16_fwd(const void* x, void* y, int B, int C, int H, int W, float e_lambda, int io, void* ws, size_t ws_bytes,
                      mi355_stream_t stream) {
    CHECK_IO16(2);
    Stat16Args a{};
    a.x = static_cast<const u16*>(x); a.y = static_cast<u16*>(y); a.B = B; a.C = C; a.f0 = e_lambda;
    return run16<M_SIMAM>(a, io, H, W, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int mi355_srm16_fwd(const void* x, const float* cfc, const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var,
                    float bn_eps, void* y, int B, int C, int H, int W, int io, void* ws, size_t ws_bytes, mi355_stream_t stream) {
    CHECK_IO16(2);
    MI355_CHECK_ARG(cfc && bn_weight && bn_bias && bn_mean && bn_var);
    Stat16Args a{};
    a.x = static_cast<const u16*>(x); a.y = static_cast<u16*>(y); a.B = B; a.C = C;
    a.p0 = cfc; a.p1 = bn_weight; a.p2 = bn_bias; a.p3 = bn_mean; a.p4 = bn_var; a.f0 = bn_eps;
    return run16<M_SRM>(a, io, H, W, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int mi355_gct_gauss16_fwd(const void* x, void* y, int B, int C, int H, int W, float c, float eps, int io, void* ws, size_t ws_bytes,
                          mi355_stream_t stream) {
    CHECK_IO16(1);
    Stat16Args a{};
    a.x = static_cast<const u16*>(x); a.y = static_cast<u16*>(y); a.B = B; a.C = C; a.f0 = eps; a.f1 = c;
    return run16<M_GCTG>(a, io, H, W, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int mi355_lct16_fwd(const void* x, const float* w, const float* b, void* y, int B, int C, int groups, int H, int W, float eps, int io,
                    void* ws, size_t ws_bytes, mi355_stream_t stream) {
    MI355_CHECK_ARG(io == 1 || io == 2);
    MI355_CHECK_ARG(groups > 0 && C > 0 && C % groups == 0);
    CHECK_IO16(1);
    MI355_CHECK_ARG(w && b);
    Stat16Args a{};
    a.x = static_cast<const u16*>(x); a.y = static_cast<u16*>(y); a.B = B; a.C = C; a.p0 = w; a.p1 = b; a.f0 = eps; a.i0 = C / groups;
    return run16<M_LCT>(a, io, H, W, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int mi355_gct16_fwd(const void* x, const float* alpha, const float* gamma, const float* beta, void* y, int B, int C, int H, int W,
                    float epsilon, int mode_l1, int after_relu, int io, void* ws, size_t ws_bytes, mi355_stream_t stream) {
    CHECK_IO16(1);
    MI355_CHECK_ARG(alpha && gamma && beta);
    Stat16Args a{};
    a.x = static_cast<const u16*>(x); a.y = static_cast<u16*>(y); a.B = B; a.C = C;
    a.p0 = alpha; a.p1 = gamma; a.p2 = beta; a.f0 = epsilon; a.i0 = after_relu ? 1 : 0;
    return mode_l1 ? run16<M_GCT1>(a, io, H, W, ws, ws_bytes, static_cast<hipStream_t>(stream))
                   : run16<M_GCT2>(a, io, H, W, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
