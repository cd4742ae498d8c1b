// gate_res.h -- the residual (+ ReLU) store epilogue of the SELayer / ECALayer / CBAM kernels (gfx950): y = [relu](x * gate + resid).
//
// RES is a template parameter of the shared kernel bodies: 0 = the plain gate (the code the plain kernels always had, nothing of this
// header is instantiated), 1 = add the residual, 2 = add the residual, then ReLU.  The arithmetic is fp32 and never contracted:
//   t = fl(x * g)  (CBAM: the product the kernel forms anyway),  s = fl(t + widen(resid)),  ReLU (NaN stays NaN),  one rounding at the store
// so an fp32 result is bit for bit torch.relu(gate(x) + resid).
// The residual has the layout of y.  The register-resident kernels read it in the store epilogue through a second buffer descriptor at
// the offsets of the stores, res_depth() slots ahead of the store that consumes them: a slot in flight costs 4 VGPRs, the slots of the
// resident row die as they are stored, and the remaining latency is covered by the other workgroups of the CU.
#pragma once
#include "common.h"

namespace {

typedef float gr_f4 __attribute__((ext_vector_type(4)));

// Cache hint of the residual loads of the register-resident kernels: the default policy, the hint their loads of x carry.  (The
// multi-pass kernels read the residual with the hint option "nt" gives their loads of x.)  The non-temporal hint has not been measured
// against it: profiles/gate_residual.md lists it as open.
constexpr int RES_AUX = 0;

// residual slots (16 bytes per lane each) in flight in front of the store that consumes them, by resident slots per lane
constexpr int res_depth(int nv) { return nv < 4 ? nv : 4; }

template <int RES>
__device__ __forceinline__ float res1(float t, float q) {
#pragma clang fp contract(off)
    const float s = __fadd_rn(t, q);
    if constexpr (RES == 2) return relu_nan(s);
    else return s;
}
template <int RES>
__device__ __forceinline__ gr_f4 res4(gr_f4 t, gr_f4 q) {
    return gr_f4{res1<RES>(t.x, q.x), res1<RES>(t.y, q.y), res1<RES>(t.z, q.z), res1<RES>(t.w, q.w)};
}

}  // namespace
