// chan_io16.hip -- SELayer / ECALayer / CBAM on 16-bit activations (IEEE half or bfloat16 in, the same type out) for gfx950.
//
// x and y are NCHW in the I/O type, parameters are fp32, every piece of arithmetic (pooling sums, excitation MLP, ECA taps, k x k
// conv, sigmoid, products) is fp32: the only rounding the path adds is the one store of y, to nearest even.  A finite product cannot
// overflow (0 <= gate <= 1 -- the hard sigmoid of the SE variants reaches both ends -- so |y| <= |x|), hence no range report.
// Range contract (tests/test_range_audit_cpu.py): this file converts fp32 to 16 bit but calls no rg_report and takes no range_word() on
// purpose -- the converted values are OUTPUTS bounded by the 16-bit inputs, never MFMA operands that a larger fp32 value could saturate.
//
// Two forms per block:
//   single read   the geometry and exchange protocols of chan_fused.hip / cbam_single.hip (8 channel rows per workgroup for SE / ECA,
//                 a band of image rows of all channels for CBAM, kept in registers between pooling and scaling; SE and CBAM exchange
//                 through the same tagged granules, ticket, epoch and error words), but the row stays PACKED in registers: 8 values per
//                 16-byte load (SE / ECA), 4 per 8-byte load (CBAM) -- half the registers of the fp32 kernels, unpacked to fp32 only for
//                 the sums and the products.
//   general       any B, C, H, W >= 1: pool pass, gate kernel(s), scale pass; 16-byte lanes when H*W % 8 == 0 and the pointers allow,
//                 2-byte lanes otherwise.  Correct everywhere, not tuned.
#include "common.h"
#include "bufops.h"
#include "io16.h"
#include "cbam_band.h"

namespace {

constexpr int ECW = 8;          // channel rows per workgroup of the single-read SE / ECA kernels (chan_fused.hip)
// 16-byte chunks per lane a row needs -> the instantiation that holds it (the NV of the kernel): one table per kernel family, read by
// the dispatch chain, the occupancy rule and (static_assert) the kernel its launch bounds are computed for
constexpr int se16_nv(int nv) { return nv <= 1 ? 1 : (nv <= 2 ? 2 : (nv <= 4 ? 4 : (nv <= 7 ? 7 : 8))); }
constexpr int eca16_nv(int nv) { return nv <= 1 ? 1 : (nv <= 2 ? 2 : (nv <= 4 ? 4 : (nv <= 7 ? 7 : 8))); }
// Waves per SIMD the single-read kernels are compiled for (512 threads = 2 waves per SIMD and workgroup: 8 / 6 / 4 = four / three / two
// workgroups per CU at <= 64 / 80 / 128 VGPRs), by 16-byte chunks per lane: the largest that compiles without scratch.  The packed row
// of a 56 x 56 image (7 chunks) is 28 registers, but the SE kernel's scalar state sits at the SGPR limit and overflows into VGPRs, so
// its long rows spill below 128.
constexpr int se16_waves(int nv) { return nv <= 2 ? 8 : (nv <= 4 ? 6 : 4); }
constexpr int eca16_waves(int nv) { return nv <= 4 ? 8 : (nv <= 7 ? 6 : 4); }

// =====================================================================================================================================
// single read: ECA (eca_halo_kernel of chan_fused.hip on packed rows; no exchange, halo rows re-summed)
// =====================================================================================================================================
template <int IO, int NV, int RES>      // RES (gate_res.h): 0 = the plain gate, 1 / 2 = y = round([relu](x * g + resid)); the kernels follow
__device__ __forceinline__ void eca16_halo_body(const u16* __restrict__ x, const float* __restrict__ taps, u16* __restrict__ y,
                                                const u16* __restrict__ resid, int C, int k, int HW, int gpi, int total, int per_xcd,
                                                int nts) {
    static_assert(eca16_nv(NV) == NV, "NV is a bucket of eca16_nv");
    __shared__ float s_mean[ECW + 8];                        // means of channels c0-pad .. c0+ECW+pad-1
    const int s = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (s >= total) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int pad = (k - 1) >> 1;
    const int b = s / gpi, c0 = (s - b * gpi) * ECW;
    const float inv = 1.0f / (float)HW;
    const u16* img = x + (long)b * C * HW;
    const u32 cw = __builtin_amdgcn_readfirstlane((u32)(c0 + wave));
    const rsrc_t rx = make_rsrc(img + (long)cw * HW, (u32)HW * 2u);   // lanes beyond the row read zeros, their stores are dropped
    const u32 voff = (u32)lane * 16u;
    u32x4 r[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) r[j] = __builtin_amdgcn_raw_buffer_load_b128(rx, voff, (u32)j * 1024u, 0);
    int hc = -1, hslot = 0;
    if (wave < 2 * pad) {
        hc = (wave < pad) ? c0 - pad + wave : c0 + ECW + (wave - pad);
        hslot = (wave < pad) ? wave : ECW + wave;
    }
    const bool halo_live = hc >= 0 && hc < C;                 // wave-uniform
    float h0 = 0.f, h1 = 0.f, h2_ = 0.f, h3 = 0.f;
    if (halo_live) {
        const u32 hcw = __builtin_amdgcn_readfirstlane((u32)hc);
        const rsrc_t rh = make_rsrc(img + (long)hcw * HW, (u32)HW * 2u);
#pragma unroll
        for (int j = 0; j < NV; ++j) add8<IO>(__builtin_amdgcn_raw_buffer_load_b128(rh, voff, (u32)j * 1024u, 0), h0, h1, h2_, h3);
    }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) add8<IO>(r[j], s0, s1, s2, s3);
    const float mean = wave_sum_sw((s0 + s1) + (s2 + s3)) * inv;
    if (lane == 0) s_mean[pad + wave] = mean;
    if (wave < 2 * pad) {
        const float hm = halo_live ? wave_sum_sw((h0 + h1) + (h2_ + h3)) * inv : 0.f;
        if (lane == 0) s_mean[hslot] = hm;
    }
    __syncthreads();
    float z = 0.f;
    for (int j = 0; j < k; ++j) z += taps[j] * s_mean[wave + j];
    const float g = sigmoidf_(z);
    const rsrc_t ry = make_rsrc(y + ((long)b * C + cw) * HW, (u32)HW * 2u);
    store_row16<IO, NV, RES>(r, g, ry, voff, nts, resid + ((long)b * C + cw) * HW, (u32)HW * 2u);      // io16.h (+ residual row, ReLU)
}
template <int IO, int NV>
__global__ __launch_bounds__(512, eca16_waves(NV)) void eca16_halo_kernel(const u16* __restrict__ x, const float* __restrict__ taps, u16* __restrict__ y,
                                                           int C, int k, int HW, int gpi, int total, int per_xcd, int nts) {
    eca16_halo_body<IO, NV, 0>(x, taps, y, nullptr, C, k, HW, gpi, total, per_xcd, nts);
}

// =====================================================================================================================================
// single read: SE (se_single_kernel of chan_fused.hip on packed rows; the same granules, ticket, epoch and error words)
// =====================================================================================================================================
struct Se16Args {
    const u16* x; u16* y; const float* w1; const float* w2; const float* b1; const float* b2;
    u64* gran; u32* ticket; u32* epoch; u32* err; u32* herr;
    u32 spin;
    int nts, gate;
    int C, Cr, HW, gpi, total;
    float inv;
};

// How many workgroups per CU the launch uses is a grid size (option "io16_occ", capped by what se16_waves allows), not a template parameter.
// EXTRA: the SE variants of the reference's CNNs (excitation biases, hard-sigmoid gate: SeExtra), as in se_single_kernel -- the plain
// SELayer instantiation carries none of their pointers and selects and keeps its code.
template <int IO, int NV, bool WLDS, bool EXTRA, int RES>      // RES (gate_res.h): 0 plain, 1 / 2 = y = round([relu](x * g + resid))
__device__ __forceinline__ void se16_single_body(const Se16Args a, const u16* __restrict__ resid) {
    static_assert(se16_nv(NV) == NV, "NV is a bucket of se16_nv");
    extern __shared__ __attribute__((aligned(16))) float smem[];      // p[C] | h[Cr] | (WLDS: W1[Cr*C] | W2[C*Cr])
    __shared__ u32 s_tk[2];
    __shared__ u32 s_ep;
    __shared__ u32 s_ok[2][8];
    float* s_p = smem;
    float* s_h = smem + a.C;
    float* s_w1 = s_h + a.Cr;
    float* s_w2 = s_w1 + a.Cr * a.C;
    const int t0 = threadIdx.x;
    const float inv = a.inv;
    const u32 last_draw = (u32)a.total + gridDim.x - 1u;              // the last draw of the launch resets the ticket and advances the epoch
    auto draw = [&](u32 ep) -> u32 {
        const u32 v = __hip_atomic_fetch_add(a.ticket, 1u, AGENT_RLX);
        if (v == last_draw) {
            __hip_atomic_store(a.ticket, 0u, AGENT_RLX);
            __hip_atomic_store(a.epoch, ep + 1u, AGENT_RLX);
        }
        return v;
    };
    if (t0 == 0) {
        // before the first draw (acquire): the epoch cannot move until this workgroup has drawn its stop ticket
        const u32 ep = __hip_atomic_load(a.epoch, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        s_ep = ep;
        s_tk[0] = draw(ep);
    }
    if (WLDS) {
        const int nw = a.Cr * a.C;
        for (int i = t0; i < nw; i += 512) { s_w1[i] = a.w1[i]; s_w2[i] = a.w2[i]; }
    }
    __syncthreads();
    const int C_ = a.C, Cr_ = a.Cr;
    const u32 EP = __builtin_amdgcn_readfirstlane(s_ep);
    const u32 GRAN_TAG = (EP + 1u) ? EP + 1u : 1u;                    // 0 is what a zeroed granule holds
    int par = 0;
    for (;;) {
        __syncthreads();
        const int t = threadIdx.x;
        const int lane = t & 63, wave = t >> 6;
        const u32 tk = __builtin_amdgcn_readfirstlane(s_tk[par]);
        if (tk >= (u32)a.total) return;
        const int b = tk / a.gpi, c0 = (tk - b * a.gpi) * ECW;
        const u32 rw = __builtin_amdgcn_readfirstlane((u32)(b * C_ + c0 + wave));
        const long row = (long)rw * a.HW;
        const rsrc_t rx = make_rsrc(a.x + row, (u32)a.HW * 2u), ry = make_rsrc(a.y + row, (u32)a.HW * 2u);
        const u32 voff = (u32)lane * 16u;                              // lanes beyond the row: zeros in, stores dropped (range check)
        u32x4 r[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) r[j] = __builtin_amdgcn_raw_buffer_load_b128(rx, voff, (u32)j * 1024u, 0);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) add8<IO>(r[j], s0, s1, s2, s3);
        const float mean = wave_sum_sw((s0 + s1) + (s2 + s3)) * inv;
        u64* gb = a.gran + (long)b * C_;
        if (lane == 0)
            __hip_atomic_store(gb + c0 + wave, ((u64)GRAN_TAG << 32) | (u64)__float_as_uint(mean), AGENT_RLX);

        // sweep the image's granules until every tag is in (bounded by spin)
        u32 spins = 0;
        bool mine_done = false;                                        // C <= 512: one granule per thread; larger C loops
        for (;;) {
            bool ok = true;
            if (C_ <= 512) {
                if (t < C_ && !mine_done) {
                    const u64 g = __hip_atomic_load(gb + (u32)t, AGENT_RLX);
                    if ((u32)(g >> 32) == GRAN_TAG) { s_p[t] = __uint_as_float((u32)g); mine_done = true; }
                    else ok = false;
                }
            } else {
                for (int cc = t; cc < C_; cc += 512) {
                    const u64 g = __hip_atomic_load(gb + cc, AGENT_RLX);
                    if ((u32)(g >> 32) == GRAN_TAG) s_p[cc] = __uint_as_float((u32)g);
                    else ok = false;
                }
            }
            // workgroup-wide AND in one barrier: a ballot per wave, eight votes through LDS, two vote rows used alternately
            const int vp = (int)(spins & 1u);
            const bool wave_ok = __builtin_amdgcn_ballot_w64(!ok) == 0ull;
            if ((t & 63) == 0) s_ok[vp][t >> 6] = wave_ok ? 1u : 0u;
            __syncthreads();
            const u32 votes = s_ok[vp][0] & s_ok[vp][1] & s_ok[vp][2] & s_ok[vp][3] & s_ok[vp][4] & s_ok[vp][5] & s_ok[vp][6] & s_ok[vp][7];
            if (__builtin_amdgcn_readfirstlane(votes)) break;
            __builtin_amdgcn_s_sleep(2);
            if (++spins > a.spin) {
                if (t == 0) {
                    __hip_atomic_store(a.err, 1u, AGENT_RLX);
                    if (a.herr) __hip_atomic_store(a.herr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                break;
            }
        }
        // next slice's ticket: only now, when this workgroup no longer waits for anybody
        if (t == 0) s_tk[par ^ 1] = draw(EP);
        // excitation: h = relu(W1 p) (16 lanes per hidden unit), g = sigmoid(W2[c,:] h) (one wave per channel)
        const float* w1 = WLDS ? s_w1 : a.w1;
        const float* w2 = WLDS ? s_w2 : a.w2;
        const int part = t & 15, jl = t >> 4;
        for (int j0 = 0; j0 < Cr_; j0 += 32) {
            const int j = j0 + jl;
            float acc = 0.f;
            if (j < Cr_) {
                const float* wrow = w1 + (long)j * C_;
                for (int cc = part; cc < C_; cc += 16) acc += wrow[cc] * s_p[cc];
            }
            acc += __shfl_xor(acc, 8, WAVE);
            acc += __shfl_xor(acc, 4, WAVE);
            acc += __shfl_xor(acc, 2, WAVE);
            acc += __shfl_xor(acc, 1, WAVE);
            if (part == 0 && j < Cr_) s_h[j] = relu_nan(EXTRA ? acc + (a.b1 ? a.b1[j] : 0.f) : acc);
        }
        __syncthreads();
        const float* w2r = w2 + (long)(c0 + wave) * Cr_;
        float z = 0.f;
        for (int j = lane; j < Cr_; j += 64) z += w2r[j] * s_h[j];
        const float g = EXTRA ? se_gate(wave_sum_sw(z) + (a.b2 ? a.b2[c0 + wave] : 0.f), a.gate) : sigmoidf_(wave_sum_sw(z));
        store_row16<IO, NV, RES>(r, g, ry, voff, a.nts, resid + row, (u32)a.HW * 2u);      // io16.h (+ residual row, ReLU)
        par ^= 1;
    }
}
template <int IO, int NV, bool WLDS, bool EXTRA>
__global__ __launch_bounds__(512, se16_waves(NV)) void se16_single_kernel(const Se16Args a) {
    se16_single_body<IO, NV, WLDS, EXTRA, 0>(a, nullptr);
}
// the residual kernels and their launch table (behind the single-read launchers): MI355_OK or the launch error
static int se16_res_launch(int io, int relu, int nv, bool wlds, int grid, size_t smem, hipStream_t st, const Se16Args& a, const u16* resid, void* state);

template <int IO, int NV, bool EXTRA>
static void se16_go(bool wlds, int grid, size_t smem, hipStream_t st, const Se16Args& a) {
    if (wlds) se16_single_kernel<IO, NV, true, EXTRA><<<grid, 512, smem, st>>>(a);
    else      se16_single_kernel<IO, NV, false, EXTRA><<<grid, 512, smem, st>>>(a);
}
template <int IO, bool EXTRA>
static void se16_go_nv(int nv, bool wlds, int grid, size_t smem, hipStream_t st, const Se16Args& a) {
    switch (se16_nv(nv)) {
        case 1: se16_go<IO, 1, EXTRA>(wlds, grid, smem, st, a); break;
        case 2: se16_go<IO, 2, EXTRA>(wlds, grid, smem, st, a); break;
        case 4: se16_go<IO, 4, EXTRA>(wlds, grid, smem, st, a); break;
        case 7: se16_go<IO, 7, EXTRA>(wlds, grid, smem, st, a); break;
        default: se16_go<IO, 8, EXTRA>(wlds, grid, smem, st, a);
    }
}

// =====================================================================================================================================
// single read: CBAM (cbam_single_kernel of cbam_single.hip; a lane holds 4 pixels of a channel's band as ONE 8-byte register pair)
// =====================================================================================================================================
// granules, DPP reductions and band geometry: cbam_band.h
struct Cbam16Args : CbamArgsT<u16> {};            // a type of its own, not an alias: the kernels' symbols keep their names

template <int IO, int SEG, int NV, bool FULL, int RES>      // RES (gate_res.h): 0 plain, 1 / 2 = y = round([relu]((x * gc) * gs + resid))
__device__ __forceinline__ void cbam16_single_body(const Cbam16Args a, const u16* __restrict__ resid) {
    constexpr int NT = 512, CL = NT / SEG;                            // channel groups (segments) per workgroup
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ u32 s_tk[2];
    __shared__ u32 s_ep;
    const int C = a.C, Cr = a.Cr, W = a.W, H = a.H, ks = a.ks, pad = (ks - 1) >> 1;
    const int HW = H * W, npx = a.R * W, TW = W + 2 * pad, TH = a.R + 2 * pad;
    const int Cp = (CL * NV > C ? CL * NV : ((C + 3) & ~3)), Crp = (Cr + 3) & ~3, L2p = (a.NB * a.cpb + 3) & ~3;
    float* s_a = smem;                                                // avg[C]
    float* s_m = s_a + Cp;                                            // max[C]
    float* s_gc = s_m + Cp;                                           // channel gates [C]
    float* s_h = s_gc + Cp;                                           // hidden: relu(W1 avg)[Crp] | relu(W1 max)[Crp]
    float* s_l2s = s_h + 2 * Crp;                                     // hop-1 landing: sums [NB*cpb]
    float* s_l2m = s_l2s + L2p;                                       //                maxima
    float* s_ps = s_l2m + L2p;                                        // per-group pixel partial sums [CL][SEG*4]
    float* s_pm = s_ps + CL * SEG * 4;                                // per-group pixel partial maxima
    float* s_t = s_pm + CL * SEG * 4;                                 // statistics tile [2][TH][TW], zero border
    float* s_gs = s_t + ((2 * TH * TW + 3) & ~3);                     // spatial gate of the band [SEG*4 >= npx]
    float* s_wc = s_gs + SEG * 4;                                     // conv taps [2*ks*ks (pad 4)]
    float* s_w1 = s_wc + ((2 * ks * ks + 3) & ~3);                    // (wlds) W1 [Cr*C] | W2 [C*Cr]
    float* s_w2 = s_w1 + Cr * C;

    const int t = threadIdx.x, q = t & (SEG - 1), cl = t / SEG;
    const bool qa = q < a.Q;
    const u32 last_draw = (u32)a.total + gridDim.x - 1u;
    auto draw = [&](u32 ep) -> u32 {
        const u32 v = __hip_atomic_fetch_add(a.ticket, 1u, AGENT_RLX);
        if (v == last_draw) {
            __hip_atomic_store(a.ticket, 0u, AGENT_RLX);
            __hip_atomic_store(a.epoch, ep + 1u, AGENT_RLX);
        }
        return v;
    };
    if (t == 0) {
        const u32 ep = __hip_atomic_load(a.epoch, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        s_ep = ep;
        s_tk[0] = draw(ep);
    }
    for (int i = t; i < 2 * ks * ks; i += NT) s_wc[i] = a.wconv[i];
    if (a.wlds)
        for (int i = t; i < Cr * C; i += NT) { s_w1[i] = a.w1[i]; s_w2[i] = a.w2[i]; }
    const float* w1 = a.wlds ? s_w1 : a.w1;
    const float* w2 = a.wlds ? s_w2 : a.w2;
    __syncthreads();
    const u32 EP = s_ep;
    const u32 TAG = (EP + 1u) ? EP + 1u : 1u;                         // 0 is what a zeroed granule holds
    int par = 0;

    for (;;) {
        __syncthreads();
        const u32 tk = s_tk[par];
        if (tk >= (u32)a.total) return;
        const int b = tk / a.NB, band = tk - b * a.NB, r0 = band * a.R;
        const long img = (long)b * C * HW + (long)r0 * W;
        u32 spins = 0;
        bool timeout = false;

        // ---- the band of every channel -> registers (packed) -----------------------------------------------------------------
        u32x2 r[NV];
        const u32 ext = ((u32)C * (u32)HW - (u32)r0 * (u32)W) * 2u;                  // bytes from the band start to the image end
        const rsrc_t rx = make_rsrc(a.x + img, ext), ry = make_rsrc(a.y + img, ext);
        const u32 off0 = qa ? ((u32)cl * (u32)HW + 4u * (u32)q) * 2u : OOB, offs = (u32)CL * (u32)HW * 2u;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (FULL) r[j] = __builtin_amdgcn_raw_buffer_load_b64(rx, off0, (u32)j * offs, 0);
            else r[j] = __builtin_amdgcn_raw_buffer_load_b64(rx, (cl + CL * j < C) ? off0 + (u32)j * offs : OOB, 0, 0);
        }
        const rsrc_t rg1 = make_rsrc(a.g1 + (long)b * a.NB * C, (u32)a.NB * (u32)C * 16u);
        const rsrc_t rg2 = make_rsrc(a.g2 + (long)b * C, (u32)C * 16u);
        const rsrc_t rg3 = make_rsrc(a.g3 + (long)b * HW, (u32)HW * 16u);
        for (int i = t; i < 2 * TH * TW; i += NT) s_t[i] = 0.f;

        // ---- hop 1, publish: (sum, max) of this band for every channel ------------------------------------------------------
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = cl + CL * j;
            const v4f v = up4<IO>(r[j]);
            float s = (v.x + v.y) + (v.z + v.w);
            float m = qa ? fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)) : -INFINITY;
            seg_reduce<SEG>(s, m, t & 63);
            if (q == 0 && c < C) gran_put(rg1, (u32)(band * C + c), s, m, TAG);
        }
        // ---- hop 1, consume: this band adds up channels ck0 .. ck0+nch-1 over all bands, publishes (avg, max) as hop 2 ------
        const int ck0 = band * a.cpb;
        const int nch = (ck0 >= C) ? 0 : ((C - ck0 < a.cpb) ? C - ck0 : a.cpb);
        const int n1 = a.NB * nch;
        for (;;) {
            bool ok = true;
            for (int i = t; i < n1; i += NT) {
                const int bb = i / nch, cc = i - bb * nch;
                float v0, v1;
                if (gran_get(rg1, (u32)(bb * C + ck0 + cc), v0, v1, TAG)) { s_l2s[bb * a.cpb + cc] = v0; s_l2m[bb * a.cpb + cc] = v1; }
                else ok = false;
            }
            if (__syncthreads_and(ok)) break;
            __builtin_amdgcn_s_sleep(2);
            if (++spins > a.spin) { timeout = true; break; }
        }
        if (t < nch) {
            float s = 0.f, m = -INFINITY;
            for (int bb = 0; bb < a.NB; ++bb) { s += s_l2s[bb * a.cpb + t]; m = fmaxf(m, s_l2m[bb * a.cpb + t]); }
            gran_put(rg2, (u32)(ck0 + t), s / (float)HW, m, TAG);
        }
        // ---- hop 2, consume: (avg, max) of every channel of the image ---------------------------------------------------------
        for (;;) {
            bool ok = true;
            for (int c = t; c < C; c += NT) {
                float v0, v1;
                if (gran_get(rg2, (u32)c, v0, v1, TAG)) { s_a[c] = v0; s_m[c] = v1; }
                else ok = false;
            }
            if (__syncthreads_and(ok)) break;
            __builtin_amdgcn_s_sleep(2);
            if (++spins > a.spin) { timeout = true; break; }
        }
        // ---- channel gates: gc = sigmoid(W2 (relu(W1 avg) + relu(W1 max))) ----------------------------------------------------
        {
            const int half = t / (NT / 2), tt = t & (NT / 2 - 1), part = tt & 15, jl = tt >> 4;
            const float* vec = half ? s_m : s_a;
            float* s_hh = s_h + half * Crp;
            for (int j0 = 0; j0 < Cr; j0 += NT / 32) {
                const int j = j0 + jl;
                float h0 = 0.f, h1 = 0.f;
                if (j < Cr) {
                    const float* wrow = w1 + (long)j * C;
                    int cc = part;
                    for (; cc + 16 < C; cc += 32) { h0 += wrow[cc] * vec[cc]; h1 += wrow[cc + 16] * vec[cc + 16]; }
                    if (cc < C) h0 += wrow[cc] * vec[cc];
                }
                float h = h0 + h1;
                h += dpp<0xB1>(h); h += dpp<0x4E>(h); h += dpp<0x124>(h); h += dpp<0x128>(h);
                if (part == 0 && j < Cr) s_hh[j] = relu_nan(h);
            }
            __syncthreads();
            for (int c = t; c < C; c += NT) {
                const float* w2r = w2 + (long)c * Cr;
                float z0 = 0.f, z1 = 0.f;
                int j = 0;
                for (; j + 1 < Cr; j += 2) {
                    z0 += w2r[j] * (s_h[j] + s_h[Crp + j]);
                    z1 += w2r[j + 1] * (s_h[j + 1] + s_h[Crp + j + 1]);
                }
                if (j < Cr) z0 += w2r[j] * (s_h[j] + s_h[Crp + j]);
                s_gc[c] = sigmoidf_(z0 + z1);
            }
            __syncthreads();
        }
        // ---- per-pixel statistics of x' = x * gc over the channels -------------------------------------------------------------
        {
            v4f ps = {0.f, 0.f, 0.f, 0.f}, pm = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c = cl + CL * j;
                if (FULL || c < C) {
                    const v4f v = up4<IO>(r[j]) * s_gc[c];
                    ps += v;
                    pm.x = fmaxf(pm.x, v.x); pm.y = fmaxf(pm.y, v.y); pm.z = fmaxf(pm.z, v.z); pm.w = fmaxf(pm.w, v.w);
                }
            }
            reinterpret_cast<v4f*>(s_ps)[cl * SEG + q] = ps;
            reinterpret_cast<v4f*>(s_pm)[cl * SEG + q] = pm;
        }
        __syncthreads();
        if (t < npx) {
            float s = 0.f, m = -INFINITY;
#pragma unroll 4
            for (int g = 0; g < CL; ++g) { s += s_ps[g * SEG * 4 + t]; m = fmaxf(m, s_pm[g * SEG * 4 + t]); }
            s = s / (float)C;
            const int ty = t / W, tx = t - ty * W;
            s_t[(0 * TH + ty + pad) * TW + tx + pad] = s;
            s_t[(1 * TH + ty + pad) * TW + tx + pad] = m;
            gran_put(rg3, (u32)(r0 * W + t), s, m, TAG);                                  // hop 3, publish
        }
        // ---- hop 3, consume: halo rows of the neighbouring bands ------------------------------------------------------------------
        {
            const int up = (r0 < pad) ? r0 : pad;
            const int dn = (H - (r0 + a.R) < pad) ? H - (r0 + a.R) : pad;
            const int n3 = (up + dn) * W;
            for (;;) {
                bool ok = true;
                for (int i = t; i < n3; i += NT) {
                    const int hr = i / W, tx = i - hr * W;
                    const int gy = (hr < up) ? r0 - up + hr : r0 + a.R + (hr - up);
                    float v0, v1;
                    if (gran_get(rg3, (u32)(gy * W + tx), v0, v1, TAG)) {
                        const int ty = gy - r0 + pad;
                        s_t[(0 * TH + ty) * TW + tx + pad] = v0;
                        s_t[(1 * TH + ty) * TW + tx + pad] = v1;
                    } else ok = false;
                }
                if (__syncthreads_and(ok)) break;
                __builtin_amdgcn_s_sleep(2);
                if (++spins > a.spin) { timeout = true; break; }
            }
        }
        // nobody is waited for any more: take the next ticket (hidden behind the conv and the stores)
        u32 next_tk = 0;
        if (t == 0) {
            next_tk = draw(EP);
            if (timeout) {
                __hip_atomic_store(a.err, 1u, AGENT_RLX);
                if (a.herr) __hip_atomic_store(a.herr, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        // ---- spatial gate of the band: sigmoid(conv_ks x ks([mean, max])) -------------------------------------------------------
        {
            const int p = t >> 2, part = t & 3;
            float acc = 0.f;
            if (p < npx) {
                const int ty = p / W, tx = p - ty * W;
                for (int rr = part; rr < 2 * ks; rr += 4) {
                    const int ch = rr / ks, dy = rr - ch * ks;
                    const float* trow = s_t + (ch * TH + ty + dy) * TW + tx;
                    const float* wrow = s_wc + rr * ks;
                    float a0 = 0.f, a1 = 0.f;
                    int dx = 0;
                    for (; dx + 1 < ks; dx += 2) { a0 += wrow[dx] * trow[dx]; a1 += wrow[dx + 1] * trow[dx + 1]; }
                    if (dx < ks) a0 += wrow[dx] * trow[dx];
                    acc += a0 + a1;
                }
            }
            acc += dpp<0xB1>(acc);
            acc += dpp<0x4E>(acc);
            if (p < npx && part == 0) s_gs[p] = sigmoidf_(acc);
        }
        __syncthreads();
        // ---- y = (x * gc) * gs from registers, rounded once ------------------------------------------------------------------------
        {
            const v4f s4 = reinterpret_cast<const v4f*>(s_gs)[q & (SEG - 1)];       // lanes beyond the band: stores are dropped (OOB)
            u32 ob = off0;
            asm volatile("" : "+v"(ob));
            cbam_store16<IO, NV, CL, FULL, RES>(r, s_gc, s4, ry, ob, offs, cl, C, a.nts, resid + img, ext);      // io16.h (+ residual band, ReLU)
        }
        if (t == 0) s_tk[par ^ 1] = next_tk;
        par ^= 1;
    }
}
template <int IO, int SEG, int NV, bool FULL>
__global__ __launch_bounds__(512, 4) void cbam16_single_kernel(const Cbam16Args a) {
    cbam16_single_body<IO, SEG, NV, FULL, 0>(a, nullptr);
}
// The residual form, a kernel of its own (the plain instantiations keep their names and arguments); 16 register pairs per lane leave no
// room for the residual in the 128 registers of two workgroups per CU: that instantiation is built for one.  (The bodies take their
// argument blocks by value: by reference hipcc allocated a scalar register more or less in the plain SE instantiations.)
constexpr int cbam16_res_waves(int nv) { return nv >= 16 ? 2 : 4; }
template <int IO, int SEG, int NV, bool FULL, bool RELU>
__global__ __launch_bounds__(512, cbam16_res_waves(NV)) void cbam16_single_res_kernel(const Cbam16Args a, const u16* __restrict__ resid) {
    cbam16_single_body<IO, SEG, NV, FULL, RELU ? 2 : 1>(a, resid);
}

// =====================================================================================================================================
// general form: pool pass -> gate kernel(s) -> scale pass
// =====================================================================================================================================
// one wave per (b, c) row, four rows per workgroup: avg[row] = sum / HW, mx[row] = max (CBAM)
template <int IO, bool WITH_MAX, bool VEC>
__global__ __launch_bounds__(256) void pool16_kernel(const u16* __restrict__ x, float* __restrict__ avg, float* __restrict__ mx, long rows,
                                                    int HW) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const u16* p = x + row * HW;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, m = -INFINITY;
    if constexpr (VEC) {
        const u32x4* p8 = reinterpret_cast<const u32x4*>(p);
        const int n8 = HW >> 3;
        for (int i = lane; i < n8; i += 64) {
            const u32x4 v = p8[i];
            add8<IO>(v, s0, s1, s2, s3);
            if constexpr (WITH_MAX) {
                m = fmaxf(m, fmaxf(fmaxf(fmaxf(lo16<IO>(v.x), hi16<IO>(v.x)), fmaxf(lo16<IO>(v.y), hi16<IO>(v.y))),
                                   fmaxf(fmaxf(lo16<IO>(v.z), hi16<IO>(v.z)), fmaxf(lo16<IO>(v.w), hi16<IO>(v.w)))));
            }
        }
    } else {
        for (int i = lane; i < HW; i += 64) {
            const float v = from16<IO>(p[i]);
            s0 += v;
            if constexpr (WITH_MAX) m = fmaxf(m, v);
        }
    }
    const float s = wave_sum((s0 + s1) + (s2 + s3));
    if constexpr (WITH_MAX) m = wave_max(m);
    if (lane == 0) {
        avg[row] = s / (float)HW;
        if constexpr (WITH_MAX) mx[row] = m;
    }
}

__device__ __forceinline__ float dot16(const float* __restrict__ wrow, const float* s_p, int C, int part) {
    float acc = 0.f;
    for (int c = part; c < C; c += 16) acc += wrow[c] * s_p[c];
    acc += __shfl_xor(acc, 8, WAVE);
    acc += __shfl_xor(acc, 4, WAVE);
    acc += __shfl_xor(acc, 2, WAVE);
    acc += __shfl_xor(acc, 1, WAVE);
    return acc;
}

// Gates of one image from its pooled vectors, IN PLACE over avg (the whole image is read into LDS before the first gate is written).
//   MODE 0 SE:   g = gate(W2 relu(W1 avg + b1) + b2), ex = the variants' biases (may be null) and gate code; the plain SELayer passes none
//   MODE 1 ECA:  g_c = sigmoid(sum_j w[j] avg[c + j - pad]) (Cr = k)
//   MODE 2 CBAM: g = sigmoid(W2 (relu(W1 avg) + relu(W1 max)))
// smem: a[C] | m[C] | h[Cr]
template <int MODE>
__global__ __launch_bounds__(256) void chan_gates16_kernel(float* __restrict__ avg, const float* __restrict__ mx, const float* __restrict__ wa,
                                                          const float* __restrict__ wb, int C, int Cr, const mi355::SeExtra ex) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_a = smem;
    float* s_m = smem + C;
    float* s_h = s_m + C;
    const int t = threadIdx.x;
    float* ab = avg + (long)blockIdx.x * C;
    for (int c = t; c < C; c += 256) {
        s_a[c] = ab[c];
        if (MODE == 2) s_m[c] = mx[(long)blockIdx.x * C + c];
    }
    __syncthreads();
    if constexpr (MODE == 1) {
        const int k = Cr, pad = (k - 1) / 2;
        for (int c = t; c < C; c += 256) {
            float z = 0.f;
            for (int j = 0; j < k; ++j) {
                const int cc = c + j - pad;
                if (cc >= 0 && cc < C) z += wa[j] * s_a[cc];
            }
            ab[c] = sigmoidf_(z);
        }
    } else {
        const int part = t & 15, jl = t >> 4;
        for (int j0 = 0; j0 < Cr; j0 += 16) {
            const int j = j0 + jl;
            float ha = 0.f, hm = 0.f;
            if (j < Cr) {
                ha = dot16(wa + (long)j * C, s_a, C, part);
                if (MODE == 2) hm = dot16(wa + (long)j * C, s_m, C, part);
            }
            if (part == 0 && j < Cr) s_h[j] = (MODE == 2) ? relu_nan(ha) + relu_nan(hm) : relu_nan((MODE == 0 && ex.b1) ? ha + ex.b1[j] : ha);
        }
        __syncthreads();
        for (int c = t; c < C; c += 256) {
            const float* w2r = wb + (long)c * Cr;
            float z = 0.f;
            for (int j = 0; j < Cr; ++j) z += w2r[j] * s_h[j];
            ab[c] = (MODE == 0) ? se_gate(ex.b2 ? z + ex.b2[c] : z, ex.gate) : sigmoidf_(z);
        }
    }
}

// per-pixel statistics over the channels of x' = x * gc (gc may be null): smap[b,0,p] = mean_c, smap[b,1,p] = max_c; a thread per pixel
template <int IO>
__global__ __launch_bounds__(256) void cbam16_stats_kernel(const u16* __restrict__ x, const float* __restrict__ gc, float* __restrict__ smap,
                                                          int C, int HW, int tiles) {
    const int b = blockIdx.x / tiles, p = (blockIdx.x % tiles) * 256 + threadIdx.x;
    if (p >= HW) return;
    const u16* xb = x + (long)b * C * HW + p;
    float s = 0.f, m = -INFINITY;
    for (int c = 0; c < C; ++c) {
        const float v = from16<IO>(xb[(long)c * HW]) * (gc ? gc[(long)b * C + c] : 1.0f);
        s += v;
        m = fmaxf(m, v);
    }
    smap[((long)b * 2 + 0) * HW + p] = s / (float)C;
    smap[((long)b * 2 + 1) * HW + p] = m;
}

// gs[b,p] = sigmoid(conv_ks x ks(smap[b]))  (2 -> 1 channels, zero pad ks / 2, no bias, cross-correlation); a thread per pixel
__global__ __launch_bounds__(256) void cbam16_sgate_kernel(const float* __restrict__ smap, const float* __restrict__ wconv, float* __restrict__ gs,
                                                          int H, int W, int ks, int tiles) {
    const int HW = H * W, pad = ks / 2;
    const int b = blockIdx.x / tiles, p = (blockIdx.x % tiles) * 256 + threadIdx.x;
    if (p >= HW) return;
    const int py = p / W, px = p - py * W;
    float acc = 0.f;
    for (int ch = 0; ch < 2; ++ch) {
        const float* sb = smap + ((long)b * 2 + ch) * HW;
        for (int dy = 0; dy < ks; ++dy) {
            const int gy = py + dy - pad;
            if (gy < 0 || gy >= H) continue;
            for (int dx = 0; dx < ks; ++dx) {
                const int gx = px + dx - pad;
                if (gx >= 0 && gx < W) acc += wconv[(ch * ks + dy) * ks + dx] * sb[gy * W + gx];
            }
        }
    }
    gs[(long)b * HW + p] = sigmoidf_(acc);
}

// y[row, i] = round((x[row, i] * gc[row]) * gs[b, i]); gc / gs may be null (= 1).  One wave per row, four rows per workgroup.
template <int IO, bool VEC, int RES>      // RES (gate_res.h): 0 plain, 1 / 2 = y = round([relu](product + resid)); the kernels are further down
__device__ __forceinline__ void scale16_body(const u16* __restrict__ x, const float* __restrict__ gc, const float* __restrict__ gs,
                                             u16* __restrict__ y, const u16* __restrict__ resid, long rows, int C, int HW, int nts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const float g = gc ? gc[row] : 1.0f;
    const float* gsb = gs ? gs + (row / C) * HW : nullptr;
    const u16* xr = x + row * HW;
    u16* yr = y + row * HW;
    if constexpr (VEC) {
        const u32x4* x8 = reinterpret_cast<const u32x4*>(xr);
        u32x4* y8 = reinterpret_cast<u32x4*>(yr);
        const int n8 = HW >> 3;
        for (int i = lane; i < n8; i += 64) {
            const u32x4 v = x8[i];
            v4f a = v4f{lo16<IO>(v.x), hi16<IO>(v.x), lo16<IO>(v.y), hi16<IO>(v.y)} * g;
            v4f c = v4f{lo16<IO>(v.z), hi16<IO>(v.z), lo16<IO>(v.w), hi16<IO>(v.w)} * g;
            if (gsb) {
                a = a * reinterpret_cast<const v4f*>(gsb)[2 * i];
                c = c * reinterpret_cast<const v4f*>(gsb)[2 * i + 1];
            }
            if constexpr (RES != 0) add_res8<IO, RES>(a, c, reinterpret_cast<const u32x4*>(resid + row * HW)[i]);
            const u32x4 o = {pack16<IO>(a.x, a.y), pack16<IO>(a.z, a.w), pack16<IO>(c.x, c.y), pack16<IO>(c.z, c.w)};
            if (nts) __builtin_nontemporal_store(o, &y8[i]);
            else y8[i] = o;
        }
    } else {
        for (int i = lane; i < HW; i += 64) {
            float v = from16<IO>(xr[i]) * g;
            if (gsb) v = v * gsb[i];
            if constexpr (RES != 0) v = res1<RES>(v, from16<IO>(resid[row * HW + i]));
            yr[i] = to16<IO>(v);
        }
    }
}

#define BY_IO(io, CALL) do { if ((io) == 1) { CALL(1); } else { CALL(2); } } while (0)

// ---- single-read launchers ------------------------------------------------------------------------------------------------------------
bool eca16_single_ok(int C, int k, int H, int W) {
    const long HW = (long)H * W;
    return mi355::opt(mi355::O_ECA_SINGLE) && (HW % 8 == 0) && (HW / 8 <= 8 * 64) && (C % ECW == 0) && (k - 1 <= 8) && (k & 1);
}

int eca16_single(const u16* x, const float* taps, u16* y, int B, int C, int k, int H, int W, int io, hipStream_t st) {
    const int HW = H * W, n8 = HW / 8, gpi = C / ECW;
    const long total_l = (long)B * gpi;
    if (total_l > (1L << 30)) return mi355::fail(MI355_EUNSUPPORTED, "eca16_single: too many slices");
    const int total = (int)total_l, per_xcd = (total + 7) / 8, grid = per_xcd * 8;
    const int nv = (n8 + 63) / 64;
    const int nts = (mi355::opt(mi355::O_NT) & 2) ? 1 : 0;
    MI355_TRACE(st, "eca16_halo_kernel io=%d C=%d HW=%d k=%d nv=%d NV=%d", io, C, HW, k, nv, eca16_nv(nv));
#define GO(IO_, NV_) eca16_halo_kernel<IO_, NV_><<<grid, 512, 0, st>>>(x, taps, y, C, k, HW, gpi, total, per_xcd, nts)
#define GO_IO(IO_)                      \
    switch (eca16_nv(nv)) {             \
        case 1: GO(IO_, 1); break;      \
        case 2: GO(IO_, 2); break;      \
        case 4: GO(IO_, 4); break;      \
        case 7: GO(IO_, 7); break;      \
        default: GO(IO_, 8);            \
    }
    BY_IO(io, GO_IO);
#undef GO_IO
#undef GO
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mi355::fail(MI355_EHIP, "eca16_single: launch -> %s", hipGetErrorString(e));
    return MI355_OK;
}

bool se16_single_ok(int C, int Cr, int H, int W) {
    const long HW = (long)H * W;
    // every slice of an image (C / 8 workgroups) has to be resident at the same time: two workgroups per CU are resident in every
    // configuration (<= 128 VGPRs, <= 60 KB of LDS)
    return mi355::opt(mi355::O_SE_SINGLE) && (HW % 8 == 0) && (HW / 8 <= 8 * 64) && (C % ECW == 0) && ((size_t)(C + Cr) * 4 <= 48 * 1024) &&
           C / ECW <= mi355::resident_slots(2);
}

// `state` = epoch | (B - 1 unused words) | ticket | err (fused_state_bytes), `gran` = B*C granules: the layout of the fp32 kernel
int se16_single(const u16* x, const float* w1, const float* w2, u16* y, int B, int C, int Cr, int H, int W, int io, void* state, void* gran,
                mi355::SeExtra ex, hipStream_t st, const u16* resid = nullptr, int relu = 0) {
    Se16Args a{};
    a.x = x; a.y = y; a.w1 = w1; a.w2 = w2; a.b1 = ex.b1; a.b2 = ex.b2; a.gate = ex.gate;
    a.gran = static_cast<u64*>(gran);
    a.ticket = static_cast<u32*>(state) + B;
    a.epoch = static_cast<u32*>(state);
    a.err = a.ticket + 1;
    if (int rc = mi355::xch_begin("se16_single", st, &a.herr, &a.spin)) return rc;
    a.C = C; a.Cr = Cr; a.HW = H * W; a.gpi = C / ECW;
    a.inv = 1.0f / (float)a.HW;
    a.nts = (mi355::opt(mi355::O_NT) & 2) ? 1 : 0;
    const long total_l = (long)B * a.gpi;
    if (total_l > (1L << 30)) return mi355::fail(MI355_EUNSUPPORTED, "se16_single: too many slices");
    a.total = (int)total_l;
    const bool wlds = (size_t)(C + Cr + 2 * (size_t)C * Cr) * sizeof(float) <= 60 * 1024;   // both weight matrices resident in LDS
    const size_t smem = ((size_t)C + Cr + (wlds ? 2 * (size_t)C * Cr : 0)) * sizeof(float);
    const int nv = (a.HW / 8 + 63) / 64;
    int occ = (int)mi355::opt(mi355::O_IO16_OCC);                 // workgroups per CU the grid is sized for: 2 .. 4, as far as registers and LDS allow
    if (occ > se16_waves(se16_nv(nv)) / 2) occ = se16_waves(se16_nv(nv)) / 2;
    while (occ > 2 && smem * occ > 150 * 1024) --occ;
    long grid = (long)mi355::resident_slots(occ);
    if (a.gpi > (long)mi355::resident_slots(2))
        return mi355::fail(MI355_EUNSUPPORTED, "se16_single: an image needs %d resident workgroups, the device holds %d", a.gpi, mi355::resident_slots(2));
    if (grid > a.total) grid = a.total;
    const unsigned long long key = ((unsigned long long)B << 32) ^ (unsigned long long)C ^ ((unsigned long long)grid << 44) ^ 0x5E16000000000000ull;
    if (int rc = mi355::xch_zero("se16_single", state, key, mi355::fused_state_bytes(B) + mi355::se_single_extra_bytes(B, C), st)) return rc;   // epoch, ticket, granules (contiguous)
    if (resid) return se16_res_launch(io, relu, nv, wlds, (int)grid, smem, st, a, resid, state);      // (the plain SELayer only: se_eca16)
    {
        const bool extra = ex.b1 || ex.b2 || ex.gate;
        MI355_TRACE(st, "se16_single_kernel io=%d C=%d HW=%d nv=%d NV=%d wlds=%d extra=%d", io, C, a.HW, nv, se16_nv(nv), (int)wlds, (int)extra);
        if (extra) {
            if (io == 1) se16_go_nv<1, true>(nv, wlds, (int)grid, smem, st, a);
            else         se16_go_nv<2, true>(nv, wlds, (int)grid, smem, st, a);
        } else {
            if (io == 1) se16_go_nv<1, false>(nv, wlds, (int)grid, smem, st, a);
            else         se16_go_nv<2, false>(nv, wlds, (int)grid, smem, st, a);
        }
    }
    return mi355::xch_launched("se16_single", state);
}

bool cbam16_single_ok(int C, int Cr, int H, int W, int ks) {
    Geo g;
    // all NB bands of an image must be resident together (two workgroups per CU); the exchange area is the fp32 kernel's
    return mi355::opt(mi355::O_CBAM_SINGLE) && geometry(512, C, Cr, H, W, ks, true, g) && g.NB <= mi355::resident_slots(2) &&
           mi355::cbam_single_extra_bytes(1, C, H, W) != 0;
}

int cbam16_single(const u16* x, const float* w1, const float* w2, const float* wconv, u16* y, int B, int C, int Cr, int H, int W, int ks, int io,
                  void* extra, hipStream_t st, const u16* resid = nullptr, int relu = 0) {
    Geo g;
    if (!geometry(512, C, Cr, H, W, ks, true, g)) return mi355::fail(MI355_EUNSUPPORTED, "cbam16_single: unsupported shape");
    Cbam16Args a{};
    a.x = x; a.y = y; a.w1 = w1; a.w2 = w2; a.wconv = wconv;
    a.g1 = static_cast<u32x4*>(extra);
    a.g2 = a.g1 + (size_t)B * g.NB * C;
    a.g3 = a.g2 + (size_t)B * C;
    a.ticket = reinterpret_cast<u32*>(a.g3 + (size_t)B * H * W);
    a.err = a.ticket + 1;
    a.epoch = a.ticket + 2;
    if (int rc = mi355::xch_begin("cbam16_single", st, &a.herr, &a.spin)) return rc;
    a.C = C; a.Cr = Cr; a.H = H; a.W = W; a.ks = ks; a.R = g.R; a.Q = g.Q; a.NB = g.NB; a.cpb = g.cpb;
    const long total_l = (long)B * g.NB;
    if (total_l > (1L << 30)) return mi355::fail(MI355_EUNSUPPORTED, "cbam16_single: too many slices");
    a.total = (int)total_l;
    a.nts = (mi355::opt(mi355::O_NT) & 2) ? 1 : 0;
    const bool full = (C == g.CL * g.NV);
    a.wlds = (g.smem_base + g.smem_w <= (size_t)(120 * 1024) / 2) ? 1 : 0;
    const size_t smem = g.smem_base + (a.wlds ? g.smem_w : 0);
    long grid = (long)mi355::resident_slots(resid ? cbam16_res_waves(g.NV) / 2 : 2);
    if (g.NB > grid) return mi355::fail(MI355_EUNSUPPORTED, "cbam16_single: an image needs %d resident workgroups, the device holds %ld", g.NB, grid);
    if (grid > a.total) grid = a.total;
    const unsigned long long key = ((unsigned long long)B << 48) ^ ((unsigned long long)C << 32) ^ ((unsigned long long)H << 16) ^ (unsigned long long)W ^ 0xCB16000000000000ull;
    if (int rc = mi355::xch_zero("cbam16_single", extra, key, mi355::cbam_single_extra_bytes(B, C, H, W), st)) return rc;
    if (resid) {
        MI355_TRACE(st, "cbam16_single_res_kernel io=%d C=%d H=%d W=%d ks=%d SEG=%d NV=%d full=%d res=1 relu=%d", io, C, H, W, ks, g.SEG, g.NV, (int)full, relu);
#define GOR(IO_, SEG_, NV_, FULL_)                                                                                     \
    do {                                                                                                               \
        if (relu) cbam16_single_res_kernel<IO_, SEG_, NV_, FULL_, true><<<(int)grid, 512, smem, st>>>(a, resid);       \
        else      cbam16_single_res_kernel<IO_, SEG_, NV_, FULL_, false><<<(int)grid, 512, smem, st>>>(a, resid);      \
    } while (0)
#define GOR_F(IO_, SEG_, NV_)                      \
    do {                                           \
        if (full) GOR(IO_, SEG_, NV_, true);       \
        else      GOR(IO_, SEG_, NV_, false);      \
    } while (0)
#define GOR_IO(IO_)                                \
    do {                                           \
        if (g.SEG == 32) {                         \
            if (g.NV == 4) GOR_F(IO_, 32, 4);      \
            else if (g.NV == 8) GOR_F(IO_, 32, 8); \
            else GOR(IO_, 32, 16, true);           \
        } else {                                   \
            if (g.NV == 4) GOR_F(IO_, 16, 4);      \
            else if (g.NV == 8) GOR_F(IO_, 16, 8); \
            else GOR(IO_, 16, 16, true);           \
        }                                          \
    } while (0)
        BY_IO(io, GOR_IO);
#undef GOR_IO
#undef GOR_F
#undef GOR
    } else {
        MI355_TRACE(st, "cbam16_single_kernel io=%d C=%d H=%d W=%d ks=%d SEG=%d NV=%d full=%d", io, C, H, W, ks, g.SEG, g.NV, (int)full);
#define GO(IO_, SEG_, NV_)                                                                         \
    do {                                                                                           \
        if (full) cbam16_single_kernel<IO_, SEG_, NV_, true><<<(int)grid, 512, smem, st>>>(a);     \
        else      cbam16_single_kernel<IO_, SEG_, NV_, false><<<(int)grid, 512, smem, st>>>(a);    \
    } while (0)
#define GO_IO(IO_)                                 \
    do {                                           \
        if (g.SEG == 32) {                         \
            if (g.NV == 4) GO(IO_, 32, 4);         \
            else if (g.NV == 8) GO(IO_, 32, 8);    \
            else cbam16_single_kernel<IO_, 32, 16, true><<<(int)grid, 512, smem, st>>>(a);  \
        } else {                                   \
            if (g.NV == 4) GO(IO_, 16, 4);         \
            else if (g.NV == 8) GO(IO_, 16, 8);    \
            else cbam16_single_kernel<IO_, 16, 16, true><<<(int)grid, 512, smem, st>>>(a);  \
        }                                          \
    } while (0)
        BY_IO(io, GO_IO);
#undef GO_IO
#undef GO
    }
    return mi355::xch_launched("cbam16_single", extra);
}

// ---- the residual forms of the single-read SE / ECA kernels: y = round([relu](x * g + resid)) (gate_res.h; store_row16 of io16.h) -------------
// Kernels of their own around the shared bodies.  Waves per SIMD as for the plain kernels (SE: se16_waves), except ECA at 7 chunks per
// lane: with the chunks of the residual in flight it spills at 80 registers and is built for two workgroups per CU.
constexpr int eca16_res_waves(int nv) { return nv <= 4 ? 8 : 4; }

template <int IO, int NV, bool RELU>
__global__ __launch_bounds__(512, eca16_res_waves(NV)) void eca16_halo_res_kernel(const u16* __restrict__ x, const float* __restrict__ taps,
                                                                   const u16* __restrict__ resid, u16* __restrict__ y, int C, int k, int HW,
                                                                   int gpi, int total, int per_xcd, int nts) {
    eca16_halo_body<IO, NV, RELU ? 2 : 1>(x, taps, y, resid, C, k, HW, gpi, total, per_xcd, nts);
}
// the residual form of the plain SELayer (no EXTRA)
template <int IO, int NV, bool WLDS, bool RELU>
__global__ __launch_bounds__(512, se16_waves(NV)) void se16_single_res_kernel(const Se16Args a, const u16* __restrict__ resid) {
    se16_single_body<IO, NV, WLDS, false, RELU ? 2 : 1>(a, resid);
}
template <int IO, int NV, bool RELU>
static void se16_res_go(bool wlds, int grid, size_t smem, hipStream_t st, const Se16Args& a, const u16* resid) {
    if (wlds) se16_single_res_kernel<IO, NV, true, RELU><<<grid, 512, smem, st>>>(a, resid);
    else      se16_single_res_kernel<IO, NV, false, RELU><<<grid, 512, smem, st>>>(a, resid);
}
template <int IO, bool RELU>
static void se16_res_go_nv(int nv, bool wlds, int grid, size_t smem, hipStream_t st, const Se16Args& a, const u16* resid) {
    switch (se16_nv(nv)) {
        case 1: se16_res_go<IO, 1, RELU>(wlds, grid, smem, st, a, resid); break;
        case 2: se16_res_go<IO, 2, RELU>(wlds, grid, smem, st, a, resid); break;
        case 4: se16_res_go<IO, 4, RELU>(wlds, grid, smem, st, a, resid); break;
        case 7: se16_res_go<IO, 7, RELU>(wlds, grid, smem, st, a, resid); break;
        default: se16_res_go<IO, 8, RELU>(wlds, grid, smem, st, a, resid);
    }
}
static int se16_res_launch(int io, int relu, int nv, bool wlds, int grid, size_t smem, hipStream_t st, const Se16Args& a, const u16* resid, void* state) {
    MI355_TRACE(st, "se16_single_res_kernel io=%d C=%d HW=%d nv=%d NV=%d wlds=%d extra=0 res=1 relu=%d", io, a.C, a.HW, nv, se16_nv(nv), (int)wlds, relu);
    if (io == 1) { if (relu) se16_res_go_nv<1, true>(nv, wlds, grid, smem, st, a, resid); else se16_res_go_nv<1, false>(nv, wlds, grid, smem, st, a, resid); }
    else         { if (relu) se16_res_go_nv<2, true>(nv, wlds, grid, smem, st, a, resid); else se16_res_go_nv<2, false>(nv, wlds, grid, smem, st, a, resid); }
    return mi355::xch_launched("se16_single", state);
}

// eca16_single with the residual: the same geometry, slices and store hint
int eca16_single_res(const u16* x, const float* taps, const u16* resid, u16* y, int B, int C, int k, int H, int W, int relu, int io, hipStream_t st) {
    const int HW = H * W, n8 = HW / 8, gpi = C / ECW;
    const long total_l = (long)B * gpi;
    if (total_l > (1L << 30)) return mi355::fail(MI355_EUNSUPPORTED, "eca16_single: too many slices");
    const int total = (int)total_l, per_xcd = (total + 7) / 8, grid = per_xcd * 8;
    const int nv = (n8 + 63) / 64;
    const int nts = (mi355::opt(mi355::O_NT) & 2) ? 1 : 0;
    MI355_TRACE(st, "eca16_halo_res_kernel io=%d C=%d HW=%d k=%d nv=%d NV=%d res=1 relu=%d", io, C, HW, k, nv, eca16_nv(nv), relu);
#define GOR(IO_, NV_)                                                                                                                   \
    do {                                                                                                                                \
        if (relu) eca16_halo_res_kernel<IO_, NV_, true><<<grid, 512, 0, st>>>(x, taps, resid, y, C, k, HW, gpi, total, per_xcd, nts);   \
        else      eca16_halo_res_kernel<IO_, NV_, false><<<grid, 512, 0, st>>>(x, taps, resid, y, C, k, HW, gpi, total, per_xcd, nts);  \
    } while (0)
#define GOR_IO(IO_)                      \
    switch (eca16_nv(nv)) {              \
        case 1: GOR(IO_, 1); break;      \
        case 2: GOR(IO_, 2); break;      \
        case 4: GOR(IO_, 4); break;      \
        case 7: GOR(IO_, 7); break;      \
        default: GOR(IO_, 8);            \
    }
    BY_IO(io, GOR_IO);
#undef GOR_IO
#undef GOR
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mi355::fail(MI355_EHIP, "eca16_single: launch -> %s", hipGetErrorString(e));
    return MI355_OK;
}

// The residual form of the single-read CBAM takes the shapes of the plain one, except where its 16-pair instantiation (one workgroup per
// CU) cannot hold an image's bands at once; those calls take the general form.
bool cbam16_single_res_ok(int C, int Cr, int H, int W, int ks) {
    Geo g;
    return cbam16_single_ok(C, Cr, H, W, ks) && geometry(512, C, Cr, H, W, ks, true, g) && g.NB <= mi355::resident_slots(cbam16_res_waves(g.NV) / 2);
}

// ---- general-form launchers ------------------------------------------------------------------------------------------------------------
template <int IO>
void pool16(bool with_max, bool vec, const u16* x, float* avg, float* mx, long rows, int HW, hipStream_t st) {
    const int grid = cdiv(rows, 4);
    MI355_TRACE(st, "pool16_kernel io=%d HW=%d", IO, HW);
    if (with_max) {
        if (vec) pool16_kernel<IO, true, true><<<grid, 256, 0, st>>>(x, avg, mx, rows, HW);
        else     pool16_kernel<IO, true, false><<<grid, 256, 0, st>>>(x, avg, mx, rows, HW);
    } else {
        if (vec) pool16_kernel<IO, false, true><<<grid, 256, 0, st>>>(x, avg, mx, rows, HW);
        else     pool16_kernel<IO, false, false><<<grid, 256, 0, st>>>(x, avg, mx, rows, HW);
    }
}
// the scale pass: the plain kernel and its residual form around scale16_body
template <int IO, bool VEC>
__global__ __launch_bounds__(256) void scale16_kernel(const u16* __restrict__ x, const float* __restrict__ gc, const float* __restrict__ gs,
                                                     u16* __restrict__ y, long rows, int C, int HW, int nts) {
    scale16_body<IO, VEC, 0>(x, gc, gs, y, nullptr, rows, C, HW, nts);
}
template <int IO, bool VEC, bool RELU>
__global__ __launch_bounds__(256) void scale16_res_kernel(const u16* __restrict__ x, const float* __restrict__ gc, const float* __restrict__ gs,
                                                         const u16* __restrict__ resid, u16* __restrict__ y, long rows, int C, int HW, int nts) {
    scale16_body<IO, VEC, RELU ? 2 : 1>(x, gc, gs, y, resid, rows, C, HW, nts);
}
template <int IO>
void scale16(bool vec, const u16* x, const float* gc, const float* gs, u16* y, long rows, int C, int HW, hipStream_t st, const u16* resid = nullptr,
             int relu = 0) {
    const int grid = cdiv(rows, 4);
    const int nts = (mi355::opt(mi355::O_NT) & 2) ? 1 : 0;
    if (resid) {
        MI355_TRACE(st, "scale16_res_kernel io=%d HW=%d res=1 relu=%d", IO, HW, relu);
        if (vec) { if (relu) scale16_res_kernel<IO, true, true><<<grid, 256, 0, st>>>(x, gc, gs, resid, y, rows, C, HW, nts);
                   else      scale16_res_kernel<IO, true, false><<<grid, 256, 0, st>>>(x, gc, gs, resid, y, rows, C, HW, nts); }
        else     { if (relu) scale16_res_kernel<IO, false, true><<<grid, 256, 0, st>>>(x, gc, gs, resid, y, rows, C, HW, nts);
                   else      scale16_res_kernel<IO, false, false><<<grid, 256, 0, st>>>(x, gc, gs, resid, y, rows, C, HW, nts); }
        return;
    }
    MI355_TRACE(st, "scale16_kernel io=%d HW=%d", IO, HW);
    if (vec) scale16_kernel<IO, true><<<grid, 256, 0, st>>>(x, gc, gs, y, rows, C, HW, nts);
    else     scale16_kernel<IO, false><<<grid, 256, 0, st>>>(x, gc, gs, y, rows, C, HW, nts);
}

bool check_io16(int io, long B, long C, long H, long W) {
    // element counts stay in 32-bit grid and row arithmetic
    return (io == 1 || io == 2) && B * C <= (1L << 31) - 8 && H * W <= (1L << 30);
}

}  // namespace

// =======================================================================================================================================
// C ABI
// =======================================================================================================================================
extern "C" {

size_t mi355_cbam16_workspace_bytes(int B, int C, int H, int W) {
    return mi355_cbam_workspace_bytes(B, C, H, W) + mi355::r16((size_t)B * H * W * sizeof(float));
}

// mode 0: SE (wa = w1, wb = w2, Cr), mode 1: ECA (wa = taps, Cr = k)
static int se_eca16(int mode, const void* xv, const float* wa, const float* wb, void* yv, int B, int C, int Cr, int H, int W, int io, void* ws,
                    hipStream_t st, mi355::SeExtra ex = mi355::SeExtra{nullptr, nullptr, 0}, const void* residv = nullptr, int relu = 0) {
    // residv (mi355_se_res_fwd / mi355_eca_res_fwd; null: the plain gate): the same route by the same predicates, the residual kernels
    const u16* x = static_cast<const u16*>(xv);
    const u16* resid = static_cast<const u16*>(residv);
    u16* y = static_cast<u16*>(yv);
    const int HW = H * W;
    const bool vec = (HW % 8 == 0) && aligned16(x) && aligned16(y) && aligned16(resid);
    const size_t smem = (size_t)(2 * (size_t)C + (mode == 0 ? Cr : 0)) * sizeof(float);
    if (smem > 64 * 1024) return mi355::fail(MI355_EUNSUPPORTED, "channel count %d too large for the gate stage", C);
    if (mode == 0 && vec && se16_single_ok(C, Cr, H, W)) {
        char* state = static_cast<char*>(ws) + mi355::pooled_bytes(B, C);
        return se16_single(x, wa, wb, y, B, C, Cr, H, W, io, state, state + mi355::fused_state_bytes(B), ex, st, resid, relu);
    }
    if (mode == 1 && vec && eca16_single_ok(C, Cr, H, W))
        return resid ? eca16_single_res(x, wa, resid, y, B, C, Cr, H, W, relu, io, st) : eca16_single(x, wa, y, B, C, Cr, H, W, io, st);
    float* pooled = static_cast<float*>(ws);
    const long rows = (long)B * C;
    if (io == 1) pool16<1>(false, vec, x, pooled, nullptr, rows, HW, st);
    else         pool16<2>(false, vec, x, pooled, nullptr, rows, HW, st);
    {
        MI355_TRACE(st, "chan_gates16_kernel mode=%d C=%d", mode, C);
        if (smem > 48 * 1024) {
            const void* fn = mode == 0 ? (const void*)chan_gates16_kernel<0> : (const void*)chan_gates16_kernel<1>;
            if (int rc = mi355::func_dynamic_lds(fn, (int)smem)) return rc;
        }
        if (mode == 0) chan_gates16_kernel<0><<<B, 256, smem, st>>>(pooled, nullptr, wa, wb, C, Cr, ex);
        else           chan_gates16_kernel<1><<<B, 256, smem, st>>>(pooled, nullptr, wa, nullptr, C, Cr, ex);
    }
    if (io == 1) scale16<1>(vec, x, pooled, nullptr, y, rows, C, HW, st, resid, relu);
    else         scale16<2>(vec, x, pooled, nullptr, y, rows, C, HW, st, resid, relu);
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}

int mi355_se16_fwd(const void* x, const float* w1, const float* w2, void* y, int B, int C, int Cr, int H, int W, int io, void* ws,
                   size_t ws_bytes, mi355_stream_t stream) {
    MI355_CHECK_ARG(io == 1 || io == 2);
    MI355_CHECK_ARG(B > 0 && C > 0 && Cr > 0 && H > 0 && W > 0);
    MI355_CHECK_ARG(x && w1 && w2 && y && ws);
    MI355_CHECK_ARG(check_io16(io, B, C, H, W));
    MI355_CHECK_ARG(ws_bytes >= mi355_se_workspace_bytes(B, C, H, W));
    return se_eca16(0, x, w1, w2, y, B, C, Cr, H, W, io, ws, static_cast<hipStream_t>(stream));
}

int mi355_se16_ex_fwd(const void* x, const float* w1, const float* b1, const float* w2, const float* b2, void* y, int B, int C, int Cr, int H,
                      int W, int gate, int io, void* ws, size_t ws_bytes, mi355_stream_t stream) {
    MI355_CHECK_ARG(io == 1 || io == 2);
    MI355_CHECK_ARG(B > 0 && C > 0 && Cr > 0 && H > 0 && W > 0 && (gate == 0 || gate == 1));
    MI355_CHECK_ARG(x && w1 && w2 && y && ws);
    MI355_CHECK_ARG(check_io16(io, B, C, H, W));
    MI355_CHECK_ARG(ws_bytes >= mi355_se_workspace_bytes(B, C, H, W));
    return se_eca16(0, x, w1, w2, y, B, C, Cr, H, W, io, ws, static_cast<hipStream_t>(stream), mi355::SeExtra{b1, b2, gate});
}

int mi355_eca16_fwd(const void* x, const float* wconv, void* y, int B, int C, int k, int H, int W, int io, void* ws, size_t ws_bytes,
                    mi355_stream_t stream) {
    MI355_CHECK_ARG(io == 1 || io == 2);
    MI355_CHECK_ARG(B > 0 && C > 0 && k > 0 && (k & 1) && H > 0 && W > 0);
    MI355_CHECK_ARG(x && wconv && y && ws);
    MI355_CHECK_ARG(check_io16(io, B, C, H, W));
    MI355_CHECK_ARG(ws_bytes >= mi355_eca_workspace_bytes(B, C, H, W));
    return se_eca16(1, x, wconv, nullptr, y, B, C, k, H, W, io, ws, static_cast<hipStream_t>(stream));
}

static int cbam16_run(const void* xv, const float* w1, const float* w2, const float* wconv, void* yv, int B, int C, int Cr, int ks, int H, int W,
                      int stage, int io, void* ws, hipStream_t st, const void* residv, int relu);

int mi355_cbam16_fwd(const void* xv, const float* w1, const float* w2, const float* wconv, void* yv, int B, int C, int Cr, int ks, int H, int W,
                     int stage, int io, void* ws, size_t ws_bytes, mi355_stream_t stream) {
    MI355_CHECK_ARG(io == 1 || io == 2);
    MI355_CHECK_ARG(stage >= 0 && stage <= 2);
    MI355_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0);
    MI355_CHECK_ARG(xv && yv && ws);
    const bool do_c = stage != 2, do_s = stage != 1;
    if (do_c) MI355_CHECK_ARG(w1 && w2 && Cr > 0);
    if (do_s) MI355_CHECK_ARG(wconv && ks > 0 && (ks & 1));
    MI355_CHECK_ARG(check_io16(io, B, C, H, W));
    MI355_CHECK_ARG(ws_bytes >= mi355_cbam16_workspace_bytes(B, C, H, W));
    return cbam16_run(xv, w1, w2, wconv, yv, B, C, Cr, ks, H, W, stage, io, ws, static_cast<hipStream_t>(stream), nullptr, 0);
}

// The launches of mi355_cbam16_fwd and of mi355_cbam_res_fwd's 16-bit half behind their argument checks.  residv (stage 0 only; null: the
// plain gate): the same route by the same predicates, the residual kernels.
static int cbam16_run(const void* xv, const float* w1, const float* w2, const float* wconv, void* yv, int B, int C, int Cr, int ks, int H, int W,
                      int stage, int io, void* ws, hipStream_t st, const void* residv, int relu) {
    const bool do_c = stage != 2, do_s = stage != 1;
    const u16* x = static_cast<const u16*>(xv);
    const u16* resid = static_cast<const u16*>(residv);
    u16* y = static_cast<u16*>(yv);
    char* wsp = static_cast<char*>(ws);
    if (stage == 0 && aligned16(x) && aligned16(y) && aligned16(resid) && (resid ? cbam16_single_res_ok(C, Cr, H, W, ks) : cbam16_single_ok(C, Cr, H, W, ks)))                  // x read once
        return cbam16_single(x, w1, w2, wconv, y, B, C, Cr, H, W, ks, io, wsp + mi355::cbam_multipass_bytes(B, C, H, W), st, resid, relu);
    const int HW = H * W;
    const bool vec = (HW % 8 == 0) && aligned16(x) && aligned16(y) && aligned16(resid);
    const size_t bc = mi355::r16((size_t)B * C * 4);
    float* avg = reinterpret_cast<float*>(wsp);                           // becomes the channel gates in place
    float* mx = reinterpret_cast<float*>(wsp + bc);
    float* smap = reinterpret_cast<float*>(wsp + 2 * bc);
    float* gs = reinterpret_cast<float*>(wsp + mi355_cbam_workspace_bytes(B, C, H, W));
    const long rows = (long)B * C;
    const int tiles = cdiv(HW, 256);
    if ((long)B * tiles > (1L << 31) - 1) return mi355::fail(MI355_EUNSUPPORTED, "mi355_cbam16_fwd: too many pixel tiles");
    if (do_c) {
        const size_t smem = (size_t)(2 * (size_t)C + Cr) * sizeof(float);
        if (smem > 64 * 1024) return mi355::fail(MI355_EUNSUPPORTED, "channel count %d too large for the gate stage", C);
        if (io == 1) pool16<1>(true, vec, x, avg, mx, rows, HW, st);
        else         pool16<2>(true, vec, x, avg, mx, rows, HW, st);
        MI355_TRACE(st, "chan_gates16_kernel mode=2 C=%d", C);
        if (smem > 48 * 1024)
            if (int rc = mi355::func_dynamic_lds((const void*)chan_gates16_kernel<2>, (int)smem)) return rc;
        chan_gates16_kernel<2><<<B, 256, smem, st>>>(avg, mx, w1, w2, C, Cr, mi355::SeExtra{nullptr, nullptr, 0});
    }
    if (do_s) {
        {
            MI355_TRACE(st, "cbam16_stats_kernel io=%d C=%d HW=%d", io, C, HW);
            if (io == 1) cbam16_stats_kernel<1><<<B * tiles, 256, 0, st>>>(x, do_c ? avg : nullptr, smap, C, HW, tiles);
            else         cbam16_stats_kernel<2><<<B * tiles, 256, 0, st>>>(x, do_c ? avg : nullptr, smap, C, HW, tiles);
        }
        {
            MI355_TRACE(st, "cbam16_sgate_kernel ks=%d HW=%d", ks, HW);
            cbam16_sgate_kernel<<<B * tiles, 256, 0, st>>>(smap, wconv, gs, H, W, ks, tiles);
        }
    }
    if (io == 1) scale16<1>(vec, x, do_c ? avg : nullptr, do_s ? gs : nullptr, y, rows, C, HW, st, resid, relu);
    else         scale16<2>(vec, x, do_c ? avg : nullptr, do_s ? gs : nullptr, y, rows, C, HW, st, resid, relu);
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}

}  // extern "C"

// the 16-bit halves of mi355_se_res_fwd / mi355_eca_res_fwd / mi355_cbam_res_fwd (chan_attn.hip checks the arguments)
namespace mi355 {
bool check_io16(int io, long B, long C, long H, long W) { return ::check_io16(io, B, C, H, W); }
int se_eca16_res(int mode, const void* x, const float* wa, const float* wb, const void* resid, void* y, int B, int C, int Cr, int H, int W, int relu,
                 int io, void* ws, hipStream_t st) {
    return se_eca16(mode, x, wa, wb, y, B, C, Cr, H, W, io, ws, st, SeExtra{nullptr, nullptr, 0}, resid, relu);
}
int cbam16_res(const void* x, const float* w1, const float* w2, const float* wconv, const void* resid, void* y, int B, int C, int Cr, int ks, int H,
               int W, int relu, int io, void* ws, hipStream_t st) {
    return cbam16_run(x, w1, w2, wconv, y, B, C, Cr, ks, H, W, 0, io, ws, st, resid, relu);
}
}  // namespace mi355
