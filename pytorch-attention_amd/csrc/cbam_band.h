// cbam_band.h -- what the fp32 and the 16-bit single-read CBAM kernels share (cbam_single.hip, chan_io16.hip): the band geometry and
// LDS budget the host picks, the kernel argument block, the tagged 16-byte granules and the DPP reductions inside a channel segment.
// Compiled under each including file's own flags (cbam_single.hip: -fno-honor-nans, build.py).
#pragma once
#include "common.h"
#include "bufops.h"

namespace {

typedef unsigned int u32;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

#define AGENT_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ void gran_put(rsrc_t g, u32 idx, float v0, float v1, u32 TAG) {
    const u32x4 v = {__float_as_uint(v0), TAG, __float_as_uint(v1), TAG};
    __builtin_amdgcn_raw_buffer_store_b128(v, g, idx * 16u, 0, AUX_SC1);      // one write-through 16-byte store
}
__device__ __forceinline__ bool gran_get(rsrc_t g, u32 idx, float& v0, float& v1, u32 TAG) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(g, idx * 16u, 0, AUX_SC1);
    v0 = __uint_as_float(v.x);
    v1 = __uint_as_float(v.z);
    return v.y == TAG && v.w == TAG;
}

// Cross-lane steps as DPP modifiers (one VALU op each, no LDS round trip like ds_bpermute): quad_perm for xor 1 / xor 2,
// row_ror for the rotations inside a row of 16 lanes.
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    // old = the source itself and bound_ctrl set: every lane of these permutations has a valid source, so no "old" value has to be
    // materialised and the compiler can fold the permutation into the consuming add / max as a DPP modifier
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float rdlane(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// Sum / max over the SEG (16 or 32) lanes of a segment; the result is only guaranteed in the segment's lane 0 (fixed order).
template <int SEG>
__device__ __forceinline__ void seg_reduce(float& s, float& m, int lane) {
    s += dpp<0xB1>(s);  m = fmaxf(m, dpp<0xB1>(m));                   // xor 1
    s += dpp<0x4E>(s);  m = fmaxf(m, dpp<0x4E>(m));                   // xor 2
    s += dpp<0x124>(s); m = fmaxf(m, dpp<0x124>(m));                  // row_ror 4
    s += dpp<0x128>(s); m = fmaxf(m, dpp<0x128>(m));                  // row_ror 8: every lane of the row holds the row total
    if (SEG == 32) {                                                  // rows 0+1 -> lane 0, rows 2+3 -> lane 32 (only those two lanes are used)
        const float s1 = rdlane(s, 16), s3 = rdlane(s, 48), m1 = rdlane(m, 16), m3 = rdlane(m, 48);
        s += (lane < 32) ? s1 : s3;
        m = fmaxf(m, (lane < 32) ? m1 : m3);
    }
}

// T = the element type of x and y: float (cbam_single.hip) or a 16-bit pattern (chan_io16.hip); everything else is fp32 in both
template <class T>
struct CbamArgsT {
    const T* x; T* y; const float* w1; const float* w2; const float* wconv;
    u32x4* g1; u32x4* g2; u32x4* g3; u32* ticket; u32* epoch; u32* err; u32* herr;   // herr: pinned host word every later call checks (api.hip)
    u32 spin;
    int C, Cr, H, W, ks, R, Q, NB, cpb, total, nts, wlds;
#ifdef CBAM_TIMING
    unsigned long long* dbg;       // [gridDim][16 slices][10 stamps] of wall_clock64 (tools/cbam_timing.hip, which builds the fp32 file only)
#endif
};

struct Geo {
    int NT, R, Q, NB, SEG, CL, NV, cpb;
    size_t smem_base, smem_w;
};

// Rows per band: the most pixels per band with R | H, (R*W) % 4 == 0 and R*W <= NT/4 (four conv lanes per pixel); 0 if none.
int band_rows(int H, int W, int nt) {
    int best = 0;
    for (int R = 1; R <= H; ++R) {
        if (H % R || (R * W) % 4 || R * W > nt / 4) continue;
        best = R;
    }
    return best;
}

// full16: refuse NV == 16 with a partly filled last slot (the 16-bit kernel: 16 partly filled register pairs per lane spill at 128
// VGPRs, its general form takes these shapes)
bool geometry(int nt, int C, int Cr, int H, int W, int ks, bool full16, Geo& g) {
    if (!(ks & 1) || ks > 15) return false;
    const int best = band_rows(H, W, nt);
    if (!best) return false;
    g.NT = nt;
    g.R = best;
    g.Q = best * W / 4;
    g.NB = H / best;
    g.SEG = g.Q > 16 ? 32 : 16;
    g.CL = nt / g.SEG;
    const int nv = (C + g.CL - 1) / g.CL;
    if (nv > 16) return false;
    g.NV = nv <= 4 ? 4 : (nv <= 8 ? 8 : 16);
    g.cpb = (C + g.NB - 1) / g.NB;
    const int pad = (ks - 1) / 2, TW = W + 2 * pad, TH = best + 2 * pad;
    auto r4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    const size_t Cp = (size_t)g.CL * g.NV > (size_t)C ? (size_t)g.CL * g.NV : r4(C);
    g.smem_base = (3 * Cp + 2 * r4(Cr) + 2 * r4((size_t)g.NB * g.cpb) + 2 * (size_t)g.CL * g.SEG * 4 +
                   r4(2 * (size_t)TH * TW) + (size_t)g.SEG * 4 + r4(2 * (size_t)ks * ks)) * 4;
    g.smem_w = 2 * (size_t)C * Cr * 4;
    if (full16 && g.NV == 16 && C != g.CL * g.NV) return false;
    return g.smem_base <= 40 * 1024;
}

}  // namespace
