// chan_stat.h -- what the fp32 and the 16-bit channel-statistics gates share (chan_stat.hip, chan_stat_io16.hip): the mode codes, the
// kernel argument block, the gate of a channel and the reductions over the values an image's workgroups exchange (all of it fp32), and
// the host body that picks single read or two passes and sets up the exchange (stat_run).
#pragma once
#include "common.h"

namespace {

using v4f = float __attribute__((ext_vector_type(4)));
typedef unsigned int u32;
typedef unsigned long long u64;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
#define AGENT_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

enum { M_SIMAM = 1, M_SRM = 2, M_GCTG = 3, M_LCT = 4, M_GCT2 = 5, M_GCT1 = 6 };
constexpr int ECW = 8;

// T = the element type of x and y: float (chan_stat.hip) or a 16-bit pattern (chan_stat_io16.hip); everything else is fp32 in both
template <class T>
struct StatArgsT {
    const T* x; T* y;
    const float* p0; const float* p1; const float* p2; const float* p3; const float* p4;   // per-channel parameter arrays (per mode)
    float f0, f1;                         // lambda | bn eps | eps, c | eps | epsilon
    int i0;                               // LCT: channels per group;  GCT1: after_relu
    u64* gran; u32* ticket; u32* epoch; u32* err; u32* herr; float* stats;   // exchange area (single read) / row statistics (two pass)
    int B, C, HW, nchunk, gpi, total;   // nchunk: 16-byte chunks per row (single read)
    u32 spin;
};

// gate of channel c from its own statistics and (exchange modes) the image's per-channel values s_p[0..C)
// red0/red1: image-level reductions prepared by the caller (GCTG: mean, var of the channel means; GCT: mean_c e^2 or mean_c |e|)
template <int MODE, class T>
__device__ __forceinline__ float gate_of(const StatArgsT<T>& a, int c, float mean, float cvar_sum, float own, float red0, float red1) {
    if (MODE == M_SRM) {
        const float stdv = sqrtf(cvar_sum / (float)(a.HW - 1));
        const float z = a.p0[2 * c] * mean + a.p0[2 * c + 1] * stdv;
        const float bn = (z - a.p3[c]) / sqrtf(a.p4[c] + a.f0) * a.p1[c] + a.p2[c];
        return sigmoidf_(bn);
    }
    if (MODE == M_GCTG) {
        const float yn = (own - red0) / sqrtf(red1 + a.f0);
        return expf(-(yn * yn / 2.0f * a.f1));
    }
    if (MODE == M_LCT) {
        const float yn = (own - red0) / sqrtf(red1 + a.f0);
        return sigmoidf_(a.p0[c] * yn + a.p1[c]);
    }
    if (MODE == M_GCT2) {
        const float e = sqrtf(own + a.f0) * a.p0[c];
        const float norm = a.p1[c] / sqrtf(red0 + a.f0);
        return 1.0f + tanhf(e * norm + a.p2[c]);
    }
    if (MODE == M_GCT1) {
        const float e = own * a.p0[c];
        const float norm = a.p1[c] / (red0 + a.f0);
        return 1.0f + tanhf(e * norm + a.p2[c]);
    }
    return 1.0f;
}

// image-level reductions over the C published values in s_p, by the whole workgroup (NT threads), fixed order:
//   GCTG: red0 = mean_c, red1 = mean_c(v^2) - mean_c^2;   GCT2: red0 = mean_c((v + eps) alpha^2);   GCT1: red0 = mean_c |v alpha|
template <int MODE, int NT, class T>
__device__ __forceinline__ void image_reduce(const StatArgsT<T>& a, const float* s_p, float* s_red, float& red0, float& red1) {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));                                       // formed here, not hoisted out of the caller's slice loop
    const int lane = t & 63, wave = t >> 6;
    float u = 0.f, w = 0.f;
    for (int c = t; c < a.C; c += NT) {
        const float v = s_p[c];
        if (MODE == M_GCTG) { u += v; w += v * v; }
        if (MODE == M_GCT2) { const float e = sqrtf(v + a.f0) * a.p0[c]; u += e * e; }
        if (MODE == M_GCT1) { u += fabsf(v * a.p0[c]); }
    }
    u = wave_sum_sw(u);
    w = wave_sum_sw(w);
    if (lane == 0) { s_red[wave] = u; s_red[16 + wave] = w; }
    __syncthreads();
    float su = 0.f, sw = 0.f;
    for (int i = 0; i < NT / 64; ++i) { su += s_red[i]; sw += s_red[16 + i]; }
    __syncthreads();
    red0 = su / (float)a.C;
    red1 = (MODE == M_GCTG) ? sw / (float)a.C - red0 * red0 : 0.f;
}

// LCT: mean / variance of the published means over the group of channel c (cpg channels), by one wave
__device__ __forceinline__ void group_reduce(const float* s_p, int c, int cpg, float& red0, float& red1) {
    int tl = threadIdx.x;
    asm volatile("" : "+v"(tl));
    const int lane = tl & 63, g0 = (c / cpg) * cpg;
    float u = 0.f, w = 0.f;
    for (int i = lane; i < cpg; i += 64) { const float v = s_p[g0 + i]; u += v; w += v * v; }
    u = wave_sum_sw(u);
    w = wave_sum_sw(w);
    red0 = u / (float)cpg;
    red1 = w / (float)cpg - red0 * red0;
}

// ---- host: the one launcher body of both files ----------------------------------------------------------------------------------------
// Single read when the rows fit the register layout, two passes otherwise.  TR (statics only, one struct per file) holds what depends
// on the width of x and y:
//   Args, who              StatArgsT<float> / StatArgsT<u16>; the prefix of every error text
//   EPC, MAX_NV            elements per 16-byte chunk (4 / 8); chunks per lane of the largest instantiation (16 / 8)
//   IO_IN_KEY              the I/O type is part of the exchange area's layout key
//   vec(a)                 rows are whole 16-byte chunks and both pointers are 16-byte aligned
//   occ<MODE>(nv, smem)    workgroups per CU the grid is sized for: what the instantiation's launch bounds guarantee
//   single<MODE>(..)       the bucket table: picks the instantiation for nv chunks per lane and launches it
//   general<MODE>(..)      the two passes; MI355_OK, or the error of a step in front of the launches
// io is 0 for the fp32 entries.
template <int MODE, class TR>
int stat_run(typename TR::Args a, int io, int H, int W, void* ws, size_t ws_bytes, hipStream_t st) {
    const int B = a.B, C = a.C;
    a.HW = H * W;
    constexpr bool XCH = MODE >= M_GCTG;
    const bool vec = TR::vec(a);
    const bool nts = (mi355::opt(mi355::O_NT) & 2) != 0;
    const bool single = mi355::opt(mi355::O_ZOO_SINGLE) && vec && (a.HW / TR::EPC <= TR::MAX_NV * 64) && (C % ECW == 0) &&
                        (size_t)C * 4 <= 48 * 1024 && (MODE != M_LCT || a.i0 <= C) &&
                        (!XCH || C / ECW <= mi355::resident_slots(2));     // an image's slices must all be resident to exchange granules
    if (single) {
        a.nchunk = a.HW / TR::EPC; a.gpi = C / ECW;
        const long total_l = (long)B * a.gpi;
        if (total_l > (1L << 30)) return mi355::fail(MI355_EUNSUPPORTED, "%s: too many slices", TR::who);
        a.total = (int)total_l;
        const int nv = (a.nchunk + 63) / 64;
        const size_t smem = XCH ? (size_t)C * 4 : 0;
        long grid = (long)mi355::resident_slots(TR::template occ<MODE>(nv, smem));
        if (grid > a.total) grid = a.total;
        if (XCH) {
            if (ws_bytes < mi355::zoo_workspace_bytes(B, C)) return mi355::fail(MI355_EINVAL, "%s: workspace too small", TR::who);
            char* base = static_cast<char*>(ws);
            a.ticket = reinterpret_cast<u32*>(base);
            a.err = a.ticket + 1;
            a.epoch = a.ticket + 2;
            if (int rc = mi355::xch_begin(TR::who, st, &a.herr, &a.spin)) return rc;
            a.gran = reinterpret_cast<u64*>(base + 16);
            // mode and grid size (and the I/O type) are part of the key: the ticket protocol counts total + grid draws per launch
            const unsigned long long key = ((unsigned long long)B << 32) ^ (unsigned long long)C ^ ((unsigned long long)grid << 44) ^
                                           ((unsigned long long)MODE << 56) ^ (TR::IO_IN_KEY ? (unsigned long long)io << 60 : 0ull);
            if (int rc = mi355::xch_zero(TR::who, ws, key, 16 + (size_t)B * C * 8, st)) return rc;       // ticket, epoch, granules
        }
        TR::template single<MODE>(nv, (int)grid, smem, st, a, io, nts);
    } else {
        if (ws_bytes < mi355::zoo_workspace_bytes(B, C)) return mi355::fail(MI355_EINVAL, "%s: workspace too small", TR::who);
        if ((size_t)C * 4 > 64 * 1024) return mi355::fail(MI355_EUNSUPPORTED, "%s: C = %d too large", TR::who, C);
        a.stats = reinterpret_cast<float*>(static_cast<char*>(ws) + 16 + (size_t)B * C * 8);
        if (XCH) mi355::ws_forget(ws);
        if (int rc = TR::template general<MODE>(vec, a, io, st, nts)) return rc;
    }
    return mi355::xch_launched(TR::who, XCH ? ws : nullptr);
}

}  // namespace
