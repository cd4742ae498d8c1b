// io16.h -- packed 16-bit <-> fp32 helpers of the channel gates on 16-bit activations (chan_io16.hip, chan_stat_io16.hip; gfx950).
// IO = 1: IEEE half, 2: bfloat16 (the library's precision codes).  Conversions to 16 bit round to nearest even.
// Range contract (tests/test_range_audit_cpu.py): pack16 / to16 convert OUTPUTS of the gates at their one store, never MFMA operands, so
// nothing here calls rg_report; the files that include this header state what bounds their outputs.
#pragma once
#include <hip/hip_runtime.h>
#include "bufops.h"

namespace {

typedef unsigned int u32;
typedef unsigned short u16;
typedef unsigned long long u64;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32 u32x2 __attribute__((ext_vector_type(2)));
using v4f = float __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef __bf16 b2 __attribute__((ext_vector_type(2)));

template <int IO> __device__ __forceinline__ float lo16(u32 w) {
    if constexpr (IO == 1) return (float)__builtin_bit_cast(h2, w).x;
    else return __uint_as_float(w << 16);
}
template <int IO> __device__ __forceinline__ float hi16(u32 w) {
    if constexpr (IO == 1) return (float)__builtin_bit_cast(h2, w).y;
    else return __uint_as_float(w & 0xffff0000u);
}
template <int IO> __device__ __forceinline__ u32 pack16(float a, float b) {          // round to nearest even, both halves
    if constexpr (IO == 1) return __builtin_bit_cast(u32, h2{(_Float16)a, (_Float16)b});
    else return __builtin_bit_cast(u32, b2{(__bf16)a, (__bf16)b});
}
template <int IO> __device__ __forceinline__ float from16(u16 h) {
    if constexpr (IO == 1) return (float)__builtin_bit_cast(_Float16, h);
    else return __uint_as_float((u32)h << 16);
}
template <int IO> __device__ __forceinline__ u16 to16(float v) {
    if constexpr (IO == 1) return __builtin_bit_cast(u16, (_Float16)v);
    else return __builtin_bit_cast(u16, (__bf16)v);
}
template <int IO> __device__ __forceinline__ v4f up4(u32x2 r) { return v4f{lo16<IO>(r.x), hi16<IO>(r.x), lo16<IO>(r.y), hi16<IO>(r.y)}; }
template <int IO> __device__ __forceinline__ u32x2 down4(v4f v) { return u32x2{pack16<IO>(v.x, v.y), pack16<IO>(v.z, v.w)}; }
// the 8 values of one 16-byte chunk into four running sums: ONE order for own rows and halo rows (ECA), so a mean does not depend on
// which workgroup computes it
template <int IO> __device__ __forceinline__ void add8(u32x4 r, float& s0, float& s1, float& s2, float& s3) {
    s0 += lo16<IO>(r.x); s1 += hi16<IO>(r.x); s2 += lo16<IO>(r.y); s3 += hi16<IO>(r.y);
    s0 += lo16<IO>(r.z); s1 += hi16<IO>(r.z); s2 += lo16<IO>(r.w); s3 += hi16<IO>(r.w);
}
template <int IO> __device__ __forceinline__ u32x4 scale8(u32x4 r, float g) {
    return u32x4{pack16<IO>(lo16<IO>(r.x) * g, hi16<IO>(r.x) * g), pack16<IO>(lo16<IO>(r.y) * g, hi16<IO>(r.y) * g),
                 pack16<IO>(lo16<IO>(r.z) * g, hi16<IO>(r.z) * g), pack16<IO>(lo16<IO>(r.w) * g, hi16<IO>(r.w) * g)};
}

// ---- store epilogues of the register-resident 16-bit gates (chan_io16.hip), plain and residual (gate_res.h, bufops.h) -----------------------
// RES != 0: widen, fl(x * g), fl(+ widen(resid)), ReLU, ONE rounding at the store.
template <int IO, int RES> __device__ __forceinline__ u32 res2(u32 r, float g, u32 q) {
    return pack16<IO>(res1<RES>(lo16<IO>(r) * g, lo16<IO>(q)), res1<RES>(hi16<IO>(r) * g, hi16<IO>(q)));
}
template <int IO, int RES> __device__ __forceinline__ u32x4 res8(u32x4 r, float g, u32x4 q) {
    return u32x4{res2<IO, RES>(r.x, g, q.x), res2<IO, RES>(r.y, g, q.y), res2<IO, RES>(r.z, g, q.z), res2<IO, RES>(r.w, g, q.w)};
}
// the general form's scale pass: the eight products of one chunk (a: values 0 .. 3, c: 4 .. 7) + the residual chunk q, read once
template <int IO, int RES> __device__ __forceinline__ void add_res8(v4f& a, v4f& c, u32x4 q) {
    a = res4<RES>(a, v4f{lo16<IO>(q.x), hi16<IO>(q.x), lo16<IO>(q.y), hi16<IO>(q.y)});
    c = res4<RES>(c, v4f{lo16<IO>(q.z), hi16<IO>(q.z), lo16<IO>(q.w), hi16<IO>(q.w)});
}
// SE / ECA: chunk j sits j KB behind the lane's first; res_row = the residual row (looked at only when RES != 0)
template <int IO, int NV, int RES>
__device__ __forceinline__ void store_row16(const u32x4 (&r)[NV], float g, rsrc_t ry, u32 voff, int nts, const u16* res_row, u32 bytes) {
    if constexpr (RES == 0) {
        if (nts) {
#pragma unroll
            for (int j = 0; j < NV; ++j) __builtin_amdgcn_raw_buffer_store_b128(scale8<IO>(r[j], g), ry, voff, (u32)j * 1024u, AUX_NT);
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) __builtin_amdgcn_raw_buffer_store_b128(scale8<IO>(r[j], g), ry, voff, (u32)j * 1024u, 0);
        }
    } else {
        const rsrc_t rr = make_rsrc(res_row, bytes);
        // The chunk step rides in the VGPR offset here, as in the fp32 kernels: with a REGISTER soffset (steps beyond the 12-bit immediate)
        // hipcc does not pad the "wide store data, then VALU write of the same VGPRs" hazard (cbam_single.hip), and the residual form of
        // the 8-chunk SE kernel returned corrupted values.
        u32 ob = voff;
        asm volatile("" : "+v"(ob));
        constexpr int D = res_depth(NV);
        u32x4 q[D];
#pragma unroll
        for (int j = 0; j < D; ++j) q[j] = __builtin_amdgcn_raw_buffer_load_b128(rr, ob + (u32)j * 1024u, 0, RES_AUX);
        if (nts) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const u32x4 cur = q[j % D];
                if (j + D < NV) q[j % D] = __builtin_amdgcn_raw_buffer_load_b128(rr, ob + (u32)(j + D) * 1024u, 0, RES_AUX);
                __builtin_amdgcn_raw_buffer_store_b128(res8<IO, RES>(r[j], g, cur), ry, ob + (u32)j * 1024u, 0, AUX_NT);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const u32x4 cur = q[j % D];
                if (j + D < NV) q[j % D] = __builtin_amdgcn_raw_buffer_load_b128(rr, ob + (u32)(j + D) * 1024u, 0, RES_AUX);
                __builtin_amdgcn_raw_buffer_store_b128(res8<IO, RES>(r[j], g, cur), ry, ob + (u32)j * 1024u, 0, 0);
            }
        }
    }
}
// CBAM: register pair j is channel cl + CL * j of the band (cbam_store of bufops.h on packed values)
template <int IO, int NV, int CL, bool FULL, int RES>
__device__ __forceinline__ void cbam_store16(const u32x2 (&r)[NV], const float* s_gc, v4f s4, rsrc_t ry, u32 ob, u32 offs, int cl, int C, int nts,
                                             const u16* res_band, u32 ext) {
    if constexpr (RES == 0) {
        if (nts) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const v4f v = (up4<IO>(r[j]) * s_gc[cl + CL * j]) * s4;
                const u32 vo = (FULL || cl + CL * j < C) ? ob + (u32)j * offs : OOB;
                __builtin_amdgcn_raw_buffer_store_b64(down4<IO>(v), ry, vo, 0, AUX_NT);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const v4f v = (up4<IO>(r[j]) * s_gc[cl + CL * j]) * s4;
                const u32 vo = (FULL || cl + CL * j < C) ? ob + (u32)j * offs : OOB;
                __builtin_amdgcn_raw_buffer_store_b64(down4<IO>(v), ry, vo, 0, 0);
            }
        }
    } else {
        const rsrc_t rr = make_rsrc(res_band, ext);
        constexpr int D = NV == 8 ? 1 : res_depth(NV);
        auto off = [&](int j) -> u32 { return (FULL || cl + CL * j < C) ? ob + (u32)j * offs : OOB; };
        u32x2 q[D];
#pragma unroll
        for (int j = 0; j < D; ++j) q[j] = __builtin_amdgcn_raw_buffer_load_b64(rr, off(j), 0, RES_AUX);
        if (nts) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const u32x2 cur = q[j % D];
                if (j + D < NV) q[j % D] = __builtin_amdgcn_raw_buffer_load_b64(rr, off(j + D), 0, RES_AUX);
                const v4f v = res4<RES>((up4<IO>(r[j]) * s_gc[cl + CL * j]) * s4, up4<IO>(cur));
                __builtin_amdgcn_raw_buffer_store_b64(down4<IO>(v), ry, off(j), 0, AUX_NT);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const u32x2 cur = q[j % D];
                if (j + D < NV) q[j % D] = __builtin_amdgcn_raw_buffer_load_b64(rr, off(j + D), 0, RES_AUX);
                const v4f v = res4<RES>((up4<IO>(r[j]) * s_gc[cl + CL * j]) * s4, up4<IO>(cur));
                __builtin_amdgcn_raw_buffer_store_b64(down4<IO>(v), ry, off(j), 0, 0);
            }
        }
    }
}

}  // namespace
