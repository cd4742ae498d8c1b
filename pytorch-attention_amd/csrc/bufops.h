// bufops.h -- raw buffer addressing helpers shared by the register-resident streaming kernels (gfx950).
#pragma once
#include <hip/hip_runtime.h>

// Everything goes through raw buffer instructions: one wave-uniform descriptor (SGPRs) + a 32-bit per-lane byte offset + a
// wave-uniform SGPR offset.  Lanes / channels outside the band get an offset beyond num_records: their loads return 0 and their
// stores are dropped by the hardware range check, so the streaming loops carry no predicates and one VGPR of address state.
typedef unsigned int bufops_u32;
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr int AUX_SC1 = 16, AUX_NT = 2;
constexpr bufops_u32 OOB = 0x80000000u;                                    // >= any num_records used here (per-image extents < 2 GB)

__device__ __forceinline__ rsrc_t make_rsrc(const void* base, bufops_u32 bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// ---- store epilogues of the register-resident fp32 gates (chan_fused.hip, cbam_single.hip), plain and residual (gate_res.h) -----------------
// RES == 0: the plain stores, exactly the loops the kernels always had.  RES != 0: y = [relu](product + residual); the residual has the
// layout of y and is read through a second descriptor at the offsets of the stores, res_depth slots ahead of the store that consumes
// them (every index is a compile-time constant after unrolling).
#include "gate_res.h"
typedef bufops_u32 bufops_u32x4 __attribute__((ext_vector_type(4)));

// SE / ECA: row slot j sits j KB behind the lane's first (`ob`); res_row = the residual row (looked at only when RES != 0)
template <int NV, bool NTS, int RES>
__device__ __forceinline__ void store_row(const gr_f4 (&r)[NV], float g, rsrc_t ry, bufops_u32 ob, const float* res_row, bufops_u32 bytes) {
    if constexpr (RES == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const gr_f4 o = r[j] * g;
            if (NTS) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bufops_u32x4, o), ry, ob + (bufops_u32)j * 1024u, 0, AUX_NT);
            else     __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bufops_u32x4, o), ry, ob + (bufops_u32)j * 1024u, 0, 0);
        }
    } else {
        const rsrc_t rr = make_rsrc(res_row, bytes);
        constexpr int D = res_depth(NV);
        gr_f4 q[D];
#pragma unroll
        for (int j = 0; j < D; ++j) q[j] = __builtin_bit_cast(gr_f4, __builtin_amdgcn_raw_buffer_load_b128(rr, ob + (bufops_u32)j * 1024u, 0, RES_AUX));
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const gr_f4 cur = q[j % D];
            if (j + D < NV) q[j % D] = __builtin_bit_cast(gr_f4, __builtin_amdgcn_raw_buffer_load_b128(rr, ob + (bufops_u32)(j + D) * 1024u, 0, RES_AUX));
            const gr_f4 o = res4<RES>(r[j] * g, cur);
            if (NTS) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bufops_u32x4, o), ry, ob + (bufops_u32)j * 1024u, 0, AUX_NT);
            else     __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bufops_u32x4, o), ry, ob + (bufops_u32)j * 1024u, 0, 0);
        }
    }
}

// CBAM: slot j is channel cl + CL * j of the band, `offs` bytes apart; channels >= C are sent out of range (FULL: there are none);
// res_band = the residual at the band start (looked at only when RES != 0).  8 slots prefetch one slot only: the deepest that stays
// in the 128 registers of two workgroups per CU without scratch.
template <int NV, int CL, bool FULL, int RES>
__device__ __forceinline__ void cbam_store(const gr_f4 (&r)[NV], const float* s_gc, gr_f4 s4, rsrc_t ry, bufops_u32 ob, bufops_u32 offs, int cl,
                                           int C, int nts, const float* res_band, bufops_u32 ext) {
    if constexpr (RES == 0) {
        if (nts) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const gr_f4 v = (r[j] * s_gc[cl + CL * j]) * s4;
                const bufops_u32 vo = (FULL || cl + CL * j < C) ? ob + (bufops_u32)j * offs : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bufops_u32x4, v), ry, vo, 0, AUX_NT);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const gr_f4 v = (r[j] * s_gc[cl + CL * j]) * s4;
                const bufops_u32 vo = (FULL || cl + CL * j < C) ? ob + (bufops_u32)j * offs : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bufops_u32x4, v), ry, vo, 0, 0);
            }
        }
    } else {
        const rsrc_t rr = make_rsrc(res_band, ext);
        constexpr int D = NV == 8 ? 1 : res_depth(NV);
        auto off = [&](int j) -> bufops_u32 { return (FULL || cl + CL * j < C) ? ob + (bufops_u32)j * offs : OOB; };
        gr_f4 q[D];
#pragma unroll
        for (int j = 0; j < D; ++j) q[j] = __builtin_bit_cast(gr_f4, __builtin_amdgcn_raw_buffer_load_b128(rr, off(j), 0, RES_AUX));
        if (nts) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const gr_f4 cur = q[j % D];
                if (j + D < NV) q[j % D] = __builtin_bit_cast(gr_f4, __builtin_amdgcn_raw_buffer_load_b128(rr, off(j + D), 0, RES_AUX));
                const gr_f4 v = res4<RES>((r[j] * s_gc[cl + CL * j]) * s4, cur);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bufops_u32x4, v), ry, off(j), 0, AUX_NT);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const gr_f4 cur = q[j % D];
                if (j + D < NV) q[j % D] = __builtin_bit_cast(gr_f4, __builtin_amdgcn_raw_buffer_load_b128(rr, off(j + D), 0, RES_AUX));
                const gr_f4 v = res4<RES>((r[j] * s_gc[cl + CL * j]) * s4, cur);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bufops_u32x4, v), ry, off(j), 0, 0);
            }
        }
    }
}
