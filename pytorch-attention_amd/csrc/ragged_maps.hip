// ragged_maps.hip -- the two device steps that let the (C x HW)-matrix blocks (DoubleAttention, CAM) take maps whose H*W or channel
// counts are no multiples of 4.  The MFMA GEMM engine (gemm.hip) loads its operands in 16-byte pieces: leading dimensions and K must
// be multiples of 4 and every image plane 16-byte aligned, which a 7 x 7 or 65 x 65 map is not.  So
//   ragged_stage         copies x (B, C, HW) in fp32 / fp16 / bf16 into the engine's K-major operand (B, Cp, HWp) fp32 with
//                        Cp = round_up(C, 4), HWp = round_up(HW, 4) and ZERO pad rows and columns (scalar guarded loads, 16-byte stores);
//   ragged_softmax_rows  is the in-place row softmax over the first `cols` entries of rows of pitch `ld`, writing 0 into the pad
//                        columns (after a product with a row bias they hold the bias, not zero), optionally scaled by *scale (CAM's beta).
// With zero pads the products over the padded K are exact, and the last product stores y at its unaligned leading dimension through
// the engine's scalar store path.
#include "common.h"
#include <type_traits>

namespace {

typedef float f4_t __attribute__((ext_vector_type(4)));

// One thread per 16-byte group of the padded image.  RG (fp32 x staged for fp16 operands): the values report range code 8 like
// nchw_to_tokens16_kernel's; the pads are zero and never report.
template <typename S, bool RG>
__global__ __launch_bounds__(256) void ragged_stage_kernel(const S* __restrict__ x, float* __restrict__ xp, int C, int Cp, int HW, int HWp,
                                                           long total4, unsigned* ovf) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    float rgm = 0.f;
    if (q < total4) {
        const int per = HWp >> 2;
        const long row = q / per;                                // (image, padded channel)
        const int p0 = (int)(q - row * per) * 4;
        const long b = row / Cp;
        const int c = (int)(row - b * Cp);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            const S* src = x + (b * C + c) * (long)HW;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p0 + e < HW) v[e] = (float)src[p0 + e];
        }
        if constexpr (RG) rgm = rg_max3abs(rg_max3abs(rgm, v[0], v[1]), v[2], v[3]);
        *reinterpret_cast<f4_t*>(xp + row * HWp + p0) = f4_t{v[0], v[1], v[2], v[3]};
    }
    if constexpr (RG) rg_report_f(rgm, ovf, 8u);
}

// One wave per row: row r of image b starts at p + b * img_stride + r * ld; the softmax runs over i < cols, entries cols <= i < ld get 0.
__global__ __launch_bounds__(256) void ragged_softmax_rows_kernel(float* __restrict__ p, int rows_per_img, int cols, int ld, long img_stride,
                                                                  long total_rows, const float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= total_rows) return;
    float* row = p + (r / rows_per_img) * img_stride + (r % rows_per_img) * (long)ld;
    float m = -INFINITY;
    for (int i = lane; i < cols; i += 64) m = fmaxf(m, row[i]);
    m = wave_max(m);
    float s = 0.f;
    for (int i = lane; i < cols; i += 64) s += expf(row[i] - m);
    s = wave_sum(s);
    const float k = (scale ? scale[0] : 1.0f) / s;
    for (int i = lane; i < ld; i += 64) row[i] = i < cols ? expf(row[i] - m) * k : 0.f;
}

}  // namespace

namespace mi355 {

int ragged_stage(const void* x, int io, float* xp, int B, int C, int HW, bool report16, hipStream_t st) {
    const int Cp = (C + 3) & ~3, HWp = (HW + 3) & ~3;
    const long total4 = (long)B * Cp * (HWp >> 2);
    if (total4 > (long)0x7fffffff * 256)                         // one workgroup per 256 groups on a 1-D grid
        return fail(MI355_EUNSUPPORTED, "ragged_stage: image too large (B=%d C=%d HW=%d)", B, C, HW);
    const int grid = cdiv(total4, 256);
    MI355_TRACE(st, "ragged_stage_kernel io=%d C=%d HW=%d", io, C, HW);
    if (io == MI355_PREC_FP16)
        ragged_stage_kernel<_Float16, false><<<grid, 256, 0, st>>>(static_cast<const _Float16*>(x), xp, C, Cp, HW, HWp, total4, nullptr);
    else if (io == MI355_PREC_BF16)
        ragged_stage_kernel<__bf16, false><<<grid, 256, 0, st>>>(static_cast<const __bf16*>(x), xp, C, Cp, HW, HWp, total4, nullptr);
    else if (report16)
        ragged_stage_kernel<float, true><<<grid, 256, 0, st>>>(static_cast<const float*>(x), xp, C, Cp, HW, HWp, total4, range_word(st));
    else
        ragged_stage_kernel<float, false><<<grid, 256, 0, st>>>(static_cast<const float*>(x), xp, C, Cp, HW, HWp, total4, nullptr);
    return MI355_OK;
}

void ragged_softmax_rows(float* p, int imgs, int rows_per_img, int cols, int ld, long img_stride, const float* scale, hipStream_t st) {
    const long rows = (long)imgs * rows_per_img;
    MI355_TRACE(st, "ragged_softmax_rows_kernel rows=%ld cols=%d ld=%d", rows, cols, ld);
    ragged_softmax_rows_kernel<<<cdiv(rows, 4), 256, 0, st>>>(p, rows_per_img, cols, ld, img_stride, rows, scale);
}

}  // namespace mi355
