// gemm16_wreg.hip -- Y (M x N, fp32) = resid + X16 (M x K) . W16^T (N x K) + bias  for SQUARE, SHORT products (N = K = 256 / 384) on gfx950:
// the projection behind an attention core at token widths 256 ... 384 (XCiT XCA proj, xcit.py:263; CSWin stage 3 proj, cswin.py:192).
//
// Why a third GEMM schedule: at N = K = 384 the product is 14.8 GFLOP over 192 MB (16-bit X in, fp32 residual in, fp32 Y out) -- 6 us of
// matrix pipe against 40 us of HBM at the copy rate of these boxes.  The tile kernels of the engine stream BOTH operands through LDS
// per output tile and pay an epilogue per tile; on this shape they reach 2.8 TB/s (70 us: profiles/r05_XCABlock_kernel_seq.txt, and the
// 256 x 256 tile leaves half of its second column tile empty at N = 384).  Here the WEIGHTS ARE STATIONARY IN REGISTERS:
//
//   workgroup  = 8 waves, persistent (one per CU); wave w owns output columns [w * N/8, (w + 1) * N/8) for EVERY row: its N/8 x K slice of W
//                lives in VGPRs as MFMA A-operand fragments for the whole kernel (N = K = 384: 3 column tiles x 12 k-steps x 4 = 144 VGPRs);
//   row tile   = 32 rows of X, staged once in LDS (double-buffered: the next tile's rows are in flight during the MFMAs) and read by all
//                eight waves as B-operand fragments; Y^T tiles = W . X^T, so a lane holds 4 consecutive output columns of one row and the
//                residual load / the store are 16-byte pieces of 192-byte (N = 384) row segments;
//   per tile   : residual loads issued first, 2 x NT x K/32 MFMAs per wave, ONE workgroup barrier.
// HBM traffic = X once + residual once + Y once; W is read once per workgroup (75 MB over the chip at N = K = 384, L2-resident).
// A row's K steps are added in ascending order on the same MFMA instruction and the epilogue is (acc + bias) + resid: bit-identical to
// gemm16_p8 / gemm16_pa on these shapes (tests/test_round6_kernels_gpu.py).
#include "gemm16.h"
#include "bufops.h"
#include <type_traits>

namespace {

using namespace g16;

// the kernel: once for an fp32 residual, once for a 16-bit one (gemm16_wreg_body.h)
#define WREG_R16 0
#include "gemm16_wreg_body.h"
#undef WREG_R16
#define WREG_R16 1
#include "gemm16_wreg_body.h"
#undef WREG_R16

}  // namespace

namespace mi355 {

// MI355_EUNSUPPORTED (nothing launched) unless the shape is one of the square short products this schedule is built for.
// resid16: g.resid carries a pointer to rows in the operand type (residual + row statistics only: mi355_linear16_stats_r16_fwd).
int gemm16_wreg(const G16Args& g, int out16, int precision, hipStream_t st, bool resid16) {
    if (resid16 && (!g.resid || !g.row_stats || g.ln16_out)) return MI355_EUNSUPPORTED;
    if (out16 || g.act != MI355_ACT_NONE || g.gamma || g.resid_period || g.lnc_a || g.rowtau) return MI355_EUNSUPPORTED;
    if (g.row_stats && (!g.resid || (reinterpret_cast<uintptr_t>(g.row_stats) & 7))) return MI355_EUNSUPPORTED;
    if (g.ln16_out && g.K != 256) return MI355_EUNSUPPORTED;      // the LayerNorm-emitting epilogue is built at N = K = 256 (at 384 it would spill: 256 VGPRs + 20 B)
    if (g.ln16_out && (!g.resid || g.row_stats || !g.ln16_w || !g.ln16_b || !aligned16(g.ln16_w) || !aligned16(g.ln16_b) || !aligned16(g.ln16_out) ||
                       (g.ln16_ld & 3) || g.ln16_ld < g.N))
        return MI355_EUNSUPPORTED;
    if (!(g.N == g.K && (g.K == 256 || g.K == 384))) return MI355_EUNSUPPORTED;
    if (g.M < 32 || (g.lda & 7) || (g.ldb & 7) || (g.ldc & 3) || g.ldb < g.K) return MI355_EUNSUPPORTED;
    if ((long)32 * g.ldc * 4 >= (1L << 31) || (long)32 * g.lda * 2 >= (1L << 31)) return MI355_EUNSUPPORTED;
    if (precision != MI355_PREC_FP16 && precision != MI355_PREC_BF16) return MI355_EUNSUPPORTED;
    const long ntile = ((long)g.M + 31) / 32;
    const int ncu = resident_slots(1);
    const int grid = (int)(ntile < ncu ? ntile : ncu);
    MI355_TRACE(st, "gemm16_wreg_kernel<%s,%s> M=%d N=%d K=%d", precision == MI355_PREC_FP16 ? "f16" : "bf16", g.ln16_out ? "resid+ln16" : (g.row_stats ? (resid16 ? "resid16+stats" : "resid+stats") : (g.resid ? "resid" : "plain")), g.M, g.N, g.K);
#define GO(T_, K_, NT_)                                                                  \
    do {                                                                                 \
        if (g.ln16_out) { if constexpr (K_ == 256) gemm16_wreg_kernel<T_, K_, NT_, true, 2><<<grid, 512, 0, st>>>(g); }   \
        else if (resid16) gemm16_wreg_r16_kernel<T_, K_, NT_><<<grid, 512, 0, st>>>(g);   \
        else if (g.row_stats) gemm16_wreg_kernel<T_, K_, NT_, true, 1><<<grid, 512, 0, st>>>(g);   \
        else if (g.resid) gemm16_wreg_kernel<T_, K_, NT_, true><<<grid, 512, 0, st>>>(g);     \
        else         gemm16_wreg_kernel<T_, K_, NT_, false><<<grid, 512, 0, st>>>(g);    \
    } while (0)
    if (precision == MI355_PREC_FP16) { if (g.K == 384) GO(_Float16, 384, 3); else GO(_Float16, 256, 2); }
    else                              { if (g.K == 384) GO(__bf16, 384, 3); else GO(__bf16, 256, 2); }
#undef GO
    return MI355_OK;
}

}  // namespace mi355
