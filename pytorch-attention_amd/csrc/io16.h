// io16.h -- packed 16-bit <-> fp32 helpers of the channel gates on 16-bit activations (chan_io16.hip, chan_stat_io16.hip; gfx950).
// IO = 1: IEEE half, 2: bfloat16 (the library's precision codes).  Conversions to 16 bit round to nearest even.
// Range contract (tests/test_range_audit_cpu.py): pack16 / to16 convert OUTPUTS of the gates at their one store, never MFMA operands, so
// nothing here calls rg_report; the files that include this header state what bounds their outputs.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace
