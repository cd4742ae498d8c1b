// gemm16_wst.hip -- Y16 (M x N, 16 bit) = act(X16 (M x 768) . W16^T (N x 768) + bias) with the WEIGHTS STATIONARY in registers: the qkv and fc1
// products of a ViT-Base encoder layer (ViT.py:81 and :59-61; N = 2304 / 3072, K = 768, M = 50 432 at B = 256), gfx950.  The 8-wave form is
// opt-in; the software-pipelined one-wave-per-SIMD form is the default for fc1 (GELU) from 32 768 rows up (option "gemm_wst" = 5).
//
// The tile kernels of the engine (gemm16_p8 / gemm16_w4 / gemm16_pa) stream BOTH operands through LDS for every 256 x 256 output tile:
// 1.39 GB cross the L2 -> CU path for the qkv product, half of it the same 3.5 MB of weights over and over, and the MFMA pipes sit 0.44-0.53
// busy (profiles/r06_c5_mfma_util.txt).  With K = 768 a 192-column slab of W is 295 KB -- it fits the register file of a CU:
//
//   workgroup  = 8 waves, persistent, owns ONE 192-column slab for the whole kernel and walks 32-row tiles of X (the workgroups of a slab
//                take the row tiles round-robin; the slabs of one row tile sit on one XCD, so X crosses HBM -> L2 once per XCD);
//   wave (p, h) p = wave >> 1: columns [48 p, 48 p + 48) of the slab; h = wave & 1: the K half [384 h, 384 h + 384).  Its 48 x 384 block of W
//                lives in VGPRs as MFMA A-fragments (3 column tiles x 12 k-steps x 4 = 144 registers), loaded once;
//   X tile       32 rows x 768 = 48 KB, LDS-DMA'ed as one linear block (16-byte chunks XOR-swizzled at the SOURCE: chunk c of row r sits at
//                chunk c ^ (r & 15), so the 16 rows a fragment read touches fall into 16 different bank groups), double-buffered; an X fragment
//                read from LDS feeds three MFMAs;
//   per tile     72 MFMAs per wave; the two K halves of a column block are added through LDS (wave h finishes row tile h: bias, GELU, 16 bit);
//                the 16-bit results wait in six registers and are stored one tile later, so that the one counted wait of an iteration never
//                covers a freshly issued store; two raw barriers.
// L2 -> CU bytes: X once per slab (12 x 77 MB for qkv) + W once per workgroup, against 1.39 GB for the 256 x 256 tiling.
// A row's K steps are added as (k < 384) + (k >= 384), each half in ascending order: NOT the bit pattern of the tile kernels (one chain), but
// the same for a row wherever it sits in the batch.
// MEASURED (profiles/r06_gemm_wst.md): qkv 208-219 us against 174-180 us on gemm16_w4, fc1 306-383 against 275-288 on gemm16_pa; a tie only on
// row counts the one-wave-per-SIMD kernel below does not take (M % 32 != 0: 192-200 vs 192-204 us).  Two barriers, the K-half exchange and the
// per-tile DMA address arithmetic leave the matrix pipes 0.43 busy -- below the tile kernels' 0.53.  Option "gemm_wst" = 1 / 2 (default 0).
// gemm16_wst1_kernel further down ("gemm_wst" = 3 / 4, and the default route 5 / 6) is the one-wave-per-SIMD form with W in AGPRs,
// bit-identical to the tile kernels.  Compiler-ordered it tied them at best (qkv 200-217 us, fc1 281-337).  With the epilogue of row block
// r - 1, the fragment reads, the DMA pieces and the stores placed by hand between the MFMAs of row block r (profiles/gemm_wst_pipe.md): fc1
// 245-254 us against 272-309 on gemm16_pa, qkv 162-183 against 173-187 on gemm16_w4.  With the epilogue as inline-assembly pieces dealt out
// by price (WstPlan, profiles/gemm_wst_slots.md): fc1 218-220 us against 246-252 in the same visit, qkv 148-165 against 157-172.
#include "gemm16.h"
#include "bufops.h"
#include <type_traits>

namespace {

using namespace g16;

__device__ __forceinline__ unsigned wst_lds_addr(const void* p) {
    return (unsigned)(unsigned long)(const __attribute__((address_space(3))) void*)p;
}
// One 1 KB LDS-DMA (16 bytes per lane, lane-linear at `dst`), issued behind the compiler's back like double_attn_fused.hip's: through the
// builtin hipcc would drain the prefetch with `s_waitcnt vmcnt(0)` in front of unrelated LDS accesses; the kernel counts its DMAs itself.
__device__ __forceinline__ void wst_dma16(const void* src, const void* dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(__builtin_amdgcn_readfirstlane(wst_lds_addr(dst)))
                 : "memory");
}
#define WST_BAR() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// 192-column slabs, 32-row tiles: 144 registers of W per wave leave room for two row tiles of accumulators and fragment reads three ahead.
// (Measured and removed: 256-column slabs with 16-row tiles -- 192 registers of W, twice the barriers per row: 244-262 us for the qkv product.
// profiles/r06_gemm_wst.md)
template <typename T, bool GELU>
__global__ __launch_bounds__(512, 1) void gemm16_wst_kernel(const G16Args g, int nslab) {
    using v8 = typename Vec8<T>::t;
    typedef T t4 __attribute__((ext_vector_type(4)));
    constexpr int K = 768, KSH = 12, RT = 2, ROWS = 32, CPR = K / 8, NCT = 3, SLAB = 4 * NCT * 16;
    constexpr int TILE_EL = ROWS * K;                                 // 48 KB
    constexpr int NDMA = TILE_EL * 2 / 1024 / 8;                      // 6 per wave and tile
    constexpr int NB = 2;
    __shared__ __attribute__((aligned(1024))) unsigned short s_x[NB][TILE_EL];
    __shared__ __attribute__((aligned(16))) float s_ex[8][NCT][64 * 4];
    __shared__ __attribute__((aligned(16))) float s_bias[SLAB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, gq = lane >> 4;
    const int p = wave >> 1, h = wave & 1;
    const int lid = xcd_contiguous_block();
    const int slab = lid % nslab, stream = lid / nslab;
    const int nstream = ((int)gridDim.x - slab + nslab - 1) / nslab;
    const int n0 = slab * SLAB;
    const T* __restrict__ A = static_cast<const T*>(g.A);
    const T* __restrict__ W = static_cast<const T*>(g.B);
    T* __restrict__ C = static_cast<T*>(g.C);
    v8 wfr[NCT][KSH];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int ks = 0; ks < KSH; ++ks)
            wfr[ct][ks] = *reinterpret_cast<const v8*>(W + (long)(n0 + p * (NCT * 16) + ct * 16 + l15) * g.ldb + h * 384 + ks * 32 + gq * 8);
    if (t < SLAB) s_bias[t] = g.bias ? g.bias[n0 + t] : 0.f;
    const long ntile = ((long)g.M + ROWS - 1) / ROWS;
    auto dma_tile = [&](long tile, int buf) {
        const long r0 = tile * ROWS;
#pragma unroll
        for (int m = 0; m < NDMA; ++m) {
            const unsigned q = (unsigned)((wave + 8 * m) * 64 + lane);
            const unsigned r = (q * 43691u) >> 22;                    // q / 96 for q < 4096
            const unsigned c = (q - r * 96u) ^ (r & 15u);
            long row = r0 + r;
            row = row < g.M ? row : (long)g.M - 1;
            wst_dma16(A + row * g.lda + c * 8u, &s_x[buf][(wave + 8 * m) * 512]);
        }
    };
    float rgmax = 0.f;
    long tile = stream;
    if (tile < ntile) dma_tile(tile, 0);
    int buf = 0;
    // the 16-bit results of a tile wait in six registers and are stored one tile LATER, behind the next DMA issue: everything the counted
    // wait at the top of an iteration covers (vmcnt(0): DMAs and stores alike) is then a whole tile old, nothing freshly issued is waited for
    t4 pend[NCT];
    long prow = -1;
    auto flush = [&]() {
        if (prow >= 0 && prow < g.M) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) *reinterpret_cast<t4*>(C + prow * g.ldc + n0 + p * (NCT * 16) + ct * 16 + gq * 4) = pend[ct];
        }
    };
    for (; tile < ntile; tile += nstream) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // this tile's rows and the stores of the tile before the previous one
        WST_BAR();                                                     // (1) tile complete; everybody is done with the other buffer and with s_ex
        const long next = tile + nstream;
        if (next < ntile) dma_tile(next, buf ^ 1);
        flush();
        f4 acc[RT][NCT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = f4{0.f, 0.f, 0.f, 0.f};
        const unsigned short* xb = &s_x[buf][0];
        auto xfrag = [&](int idx) {
            const int ks = idx / RT, rt = idx % RT;
            return *reinterpret_cast<const v8*>(xb + ((rt * 16 + l15) * CPR + ((h * 48 + ks * 4 + gq) ^ l15)) * 8);
        };
        v8 xq[4];
#pragma unroll
        for (int pre = 0; pre < 3; ++pre) xq[pre] = xfrag(pre);
#pragma unroll
        for (int idx = 0; idx < KSH * RT; ++idx) {
            if (idx + 3 < KSH * RT) xq[(idx + 3) & 3] = xfrag(idx + 3);
            const int ks = idx / RT, rt = idx % RT;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = mma16<T>(wfr[ct][ks], xq[idx & 3], acc[rt][ct]);
        }
        // the K halves meet: wave h finishes row tile h and hands row tile 1 - h to its partner
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) *reinterpret_cast<f4*>(&s_ex[wave][ct][lane * 4]) = h ? acc[0][ct] : acc[1][ct];
        WST_BAR();                                                     // (2)
        const long row = tile * ROWS + h * 16 + l15;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const f4 other = *reinterpret_cast<const f4*>(&s_ex[wave ^ 1][ct][lane * 4]);
            f4 v = (h ? acc[1][ct] : acc[0][ct]) + other;
            v = v + *reinterpret_cast<const f4*>(&s_bias[p * (NCT * 16) + ct * 16 + gq * 4]);
            if constexpr (GELU) v = gelu16_fast4(v);
            if constexpr (std::is_same<T, _Float16>::value) rgmax = rg_absmax4_f(rgmax, v);
            pend[ct] = t4{(T)v.x, (T)v.y, (T)v.z, (T)v.w};
        }
        prow = row;
        buf ^= 1;
    }
    flush();
    if constexpr (std::is_same<T, _Float16>::value) rg_report_f(rgmax, g.ovf, 3u);
}

// ---- ONE wave per SIMD: wave p owns 64 columns of a 256-column slab for the WHOLE reduction -- 64 x 768 of W = 384 registers, the first sixteen
// k-steps in AGPRs (256) and the last eight in VGPRs (128).  hipcc will not keep MFMA A-operands in AGPRs on its own (it shuttles them through
// v_accvgpr moves: 545 us, profiles/r06_gemm_wst.md), so the MFMAs are inline assembly whose A-operand constraint is "a": the fragments are
// written to their accumulation registers once and read there by the matrix pipe for the rest of the kernel.  No K split (a row's K steps form one
// ascending chain: the bit pattern of the tile kernels), no exchange, ONE barrier per 32-row tile, a ring of three X tiles, stores deferred by one
// row block.  With one wave per SIMD nobody else hides the wave's serial work, so the wave hides it itself: see the schedule below.
template <typename T>
__device__ __forceinline__ void wst_mfma_a(f4& c, const typename Vec8<T>::t& w, const typename Vec8<T>::t& x) {
    if constexpr (std::is_same<T, _Float16>::value) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "a"(w), "v"(x));
    else                                            asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "a"(w), "v"(x));
}
template <typename T>
__device__ __forceinline__ void wst_mfma_v(f4& c, const typename Vec8<T>::t& w, const typename Vec8<T>::t& x) {
    if constexpr (std::is_same<T, _Float16>::value) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(w), "v"(x));
    else                                            asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(w), "v"(x));
}
// one 1 KB LDS-DMA piece from a wave-uniform base + a 32-bit lane offset (no 64-bit address arithmetic per piece)
// m0 is written once per piece, not saved and restored (three scalar instructions per piece less): gemm16_wst1_kernel holds NO other
// instruction that names m0 -- LDS instructions need none on gfx9 and later, and the kernel uses nothing else that would (no LDS-DMA builtin,
// no indexed register move, no message).  m0 is a reserved register, so it cannot stand on the clobber list;
// tests/test_gemm16_wst_slots_cpu.py checks in the ISA of all four instantiations that these writes are the only lines with m0 in them.
__device__ __forceinline__ void wst_dma_so(const void* base, unsigned off, unsigned dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(off), "s"(base), "s"(dst) : "memory");
}
// the same inside the tile loop: the piece's place in the ring buffer is a compile-time distance from the wave's first piece, and the sum is
// formed in m0 itself
template <int DIST>
__device__ __forceinline__ void wst_dma_piece(const void* base, unsigned off, unsigned dst0) {
    asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(off), "s"(base), "s"(dst0), "n"(DIST) : "memory", "scc");
}

template <int I> struct WstI { static constexpr int v = I; };
template <int B, int N>
struct WstUnroll {
    template <class F>
    static __device__ __forceinline__ void run(F& f) {
        f(WstI<B>{});
        WstUnroll<B + 1, N>::run(f);
    }
};
template <int N>
struct WstUnroll<N, N> {
    template <class F>
    static __device__ __forceinline__ void run(F&) {}
};
// the first k-step of a row block multiplies into a zero C operand: no accumulator clearing
template <typename T>
__device__ __forceinline__ void wst_mfma_a0(f4& c, const typename Vec8<T>::t& w, const typename Vec8<T>::t& x) {
    if constexpr (std::is_same<T, _Float16>::value) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(c) : "a"(w), "v"(x));
    else                                            asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(c) : "a"(w), "v"(x));
}

// SOFTWARE PIPELINE INSIDE THE ONE WAVE (profiles/gemm_wst_pipe.md).  The unit is one 16-row block = 96 MFMAs (24 k-steps x 4 column tiles) =
// 1 536 matrix-pipe cycles; the two row blocks of a 32-row tile own disjoint accumulators acc[0][*] / acc[1][*], so while block r accumulates
// into one set the epilogue of block r - 1 drains the other.  The block body is 96 SLOTS, one MFMA each, and the ORDER of the statements is the
// schedule (the MFMAs and DMA pieces are `asm volatile`, a scheduling barrier closes every slot).  Behind the MFMA of slot m = 4 ks + ct ride:
//   m = 0 .. 3        the four deferred row stores of the SAME row block of the tile before (pend[rt], converted one row block ago);
//   m % 4 == 1        the ds_read_b128 of the X fragment of k-step ks + 3 (ring of four; past the end of row block 0: of row block 1; the
//                     first three of a tile are read behind the barrier);
//   m % 16 == 6       one of the tile's twelve LDS-DMA pieces (six per row block) of the tile TWO ahead; its lane offset was read from LDS
//                     fifteen slots earlier, at m % 16 == 7, right behind the piece before it;
//   m >= 4, m % 16 != 6   at most one PIECE of the epilogue of the previous row block, two to four VALU instructions of inline assembly, placed
//                     by WstPlan below.  The first reads an accumulator eight MFMAs after the MFMA that wrote it last.
//   m = 84 .. 87      row block 1 only: the four fragment pointers move on to the next ring buffer (its last fragment read is at slot 81).
// Per tile ONE counted wait and ONE barrier, in front of row block 0.  Issue order of an iteration: [4 stores][6 DMA][4 stores][6 DMA], the DMA
// pieces those of the tile two ahead.  INVARIANT of `s_waitcnt vmcnt(12)`: all pieces of the tile this iteration reads were issued BEFORE the
// twelve pieces of the next tile (in the iteration before, or in the prologue, which issues the whole first tile ahead of the second).  Loads
// return in order among themselves, so if one piece of this tile were still out, all twelve later pieces would be out too: thirteen operations,
// more than the wait leaves.  That holds whatever order stores complete in against loads -- no assumption about a common retirement order.
// With an in-order counter the wait also covers the four stores and four pieces that opened the previous iteration, one tile old; waiting
// at vmcnt(20), which needs that assumption, measured the same (profiles/gemm_wst_pipe.md).  Where no next tile was requested (the last tile of
// a stream) the wait is vmcnt(0).
// The kernel waits for no other workgroup (capture-safe); a row's K steps form one ascending chain and the epilogue expressions are those of the
// tile kernels: the output is bit-identical to theirs wherever the row sits.
// The first tile of a stream is peeled (`first` is a compile-time flag of the tile body): the deferred stores need no branch.  The stores are
// inline assembly too (wave-uniform base in SGPRs + the lane's 32-bit offset, no 64-bit address arithmetic per store).
// TOOLCHAIN: MFMAs, epilogue pieces, DMA pieces and stores are `asm volatile` and keep their order; what is left to the compiler between
// them are the LDS reads, the waits for them and scalar bookkeeping.  The MFMAs are opaque to its hazard recogniser: nothing it generates may
// read an accumulator right behind them (see the wait states that close a tile body).  tests/test_gemm16_wst_slots_cpu.py checks the compiled
// stream (what sits in every gap, no register copies of accumulators inside a body, m0), tests/test_gemm16_wst_pipe_cpu.py the registers (no
// scratch), tests/test_gemm16_wst_slots_gpu.py and tests/test_gemm16_wst_pipe_gpu.py the bits: re-run them on every toolchain change.
//
// THE PLAN of the epilogue of one row block (WstPlan): which PIECE rides behind which MFMA.  A piece is ONE `asm volatile` of two to four
// instructions.  The four outputs e = 0 .. 3 a lane holds of a column tile are four independent CHAINS with registers of their own; with
// GELU a chain is four pieces -- [bias add, min, FMA] [4 FMA] [multiply, v_exp_f32] [2 FMA]: 3, 4, 3 and 2 units of 4 issue cycles, v_exp_f32
// counting two -- without it the bias add alone.  When the four chains of a column tile are through, its TAIL follows ([2 conversions + fp16:
// the maximum of the four magnitudes] [fp16: the range test]), then the chains start on the next column tile.  Slots 0-3 (stores) and
// m % 16 == 6 (DMA piece) carry nothing; the pieces are spread evenly over the other 86 (72 of them with GELU and fp16, 24 without GELU).
// WHY CHAINS TAKE TURNS: LLVM's hazard recogniser assumes that any inline assembly forwards its destination like an SDWA / op_sel
// instruction and pads with `s_nop 0` (4 issue cycles, as much as a VALU instruction) when the next instruction that is not inline assembly
// is not between it and a statement that names one of its registers -- the MFMAs between do not count.  A piece that continues the chain of
// the piece in the slot before it costs one s_nop; one that continues a chain last touched BEFORE the k-step's ds_read_b128 (slot m % 4 == 1)
// or before the s_waitcnt in front of the k-step's first MFMA (m % 4 == 0) costs nothing.  So the plan gives a slot the least advanced chain
// that no piece has touched since the last of those two instructions.  (Plain C++ between the MFMAs, the form before, paid the same s_nop
// behind every empty asm statement that pinned a piece, and drifted: profiles/gemm_wst_slots.md.)
template <bool GELU, bool F16>
struct WstPlan {
    static constexpr int NPC = GELU ? 4 : 1;                          // pieces per chain and column tile
    static constexpr int NT = F16 ? 2 : 1;                            // tail pieces per column tile
    static constexpr int NEED = 4 * (4 * NPC + NT), AVAIL = 96 - 4 - 6;
    int code[96];                                                     // -1: nothing; ct * 32 + chain * 4 + piece; ct * 32 + 16 + tail piece
    int reload[96];                                                   // ct: read the bias of column tile ct behind this slot's piece
    bool complete;
    static constexpr bool carries(int m) { return m >= 4 && (m & 15) != 6; }
    constexpr WstPlan() : code{}, reload{}, complete(false) {
        int ct = 0, prog[4] = {0, 0, 0, 0}, tp = 0, placed = 0, seen = 0, started = 0;
        bool used[4] = {false, false, false, false};
        for (int m = 0; m < 96; ++m) {
            code[m] = -1;
            reload[m] = 0;
            if (!carries(m)) continue;
            if ((m & 3) == 0 || ((m & 3) == 1 && m < 84))             // a k-step's s_waitcnt or its fragment read stands in front of this piece
                for (int c = 0; c < 4; ++c) used[c] = false;
            const bool due = placed * AVAIL <= seen * NEED;           // even spacing
            ++seen;
            if (ct == 4 || !due) continue;
            if (prog[0] == NPC && prog[1] == NPC && prog[2] == NPC && prog[3] == NPC) {
                code[m] = ct * 32 + 16 + tp;
                for (int c = 0; c < 4; ++c) used[c] = true;
                if (++tp == NT) {
                    ++ct;
                    tp = started = 0;
                    for (int c = 0; c < 4; ++c) prog[c] = 0;
                }
            } else {
                int best = -1;
                for (int c = 0; c < 4; ++c)
                    if (prog[c] < NPC && !used[c] && (best < 0 || prog[c] < prog[best])) best = c;
                if (best < 0)
                    for (int c = 0; c < 4; ++c)
                        if (prog[c] < NPC && (best < 0 || prog[c] < prog[best])) best = c;
                code[m] = ct * 32 + best * 4 + prog[best];
                if (prog[best] == 0 && ++started == 4 && ct < 3) reload[m] = ct + 1;
                ++prog[best];
                used[best] = true;
            }
            ++placed;
        }
        complete = ct == 4;
    }
};
template <bool GELU, bool F16>
inline constexpr WstPlan<GELU, F16> wst_plan{};

template <typename T, bool GELU>
__global__ __launch_bounds__(256, 1) void gemm16_wst1_kernel(const G16Args g, int nslab) {
    using v8 = typename Vec8<T>::t;
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    constexpr bool F16 = std::is_same<T, _Float16>::value;
    constexpr int K = 768, KS = 24, KSA = 16, RT = 2, ROWS = 16 * RT, CPR = K / 8;
    constexpr int TILE_EL = ROWS * K;                                 // 48 KB
    constexpr int NDMA = TILE_EL * 2 / 1024 / 4;                      // 12 pieces per wave and tile
    constexpr int NB = 3;
    static_assert(wst_plan<GELU, F16>.complete, "every epilogue piece has a slot");
    __shared__ __attribute__((aligned(1024))) unsigned short s_x[NB][TILE_EL];
    __shared__ __attribute__((aligned(16))) float s_bias[256];
    __shared__ unsigned s_doff[NDMA][256];                            // the lanes' DMA source offsets: twelve registers the pipelined body has no room for
    const int t = threadIdx.x, lane = t & 63, l15 = lane & 15, gq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lid = xcd_contiguous_block();
    const int slab = lid % nslab, stream = lid / nslab;
    const int nstream = ((int)gridDim.x - slab + nslab - 1) / nslab;
    const int n0 = slab * 256 + wave * 64;
    const T* __restrict__ A = static_cast<const T*>(g.A);
    const T* __restrict__ W = static_cast<const T*>(g.B);
    T* __restrict__ C = static_cast<T*>(g.C);
    // ---- DMA: piece j = wave + 4 m moves LDS chunks 64 j .. 64 j + 63; LDS chunk q = (row q / 96, slot q % 96) holds the row's chunk slot ^ (row & 15).
    // The first two tiles are on their way before the weight fragments are asked for. ----
    const unsigned lds0 = wst_lds_addr(&s_x[0][0]);
    const int ntile = __builtin_amdgcn_readfirstlane(g.M / ROWS);    // launcher: M % 32 == 0
    int tile = stream;
#pragma unroll
    for (int m = 0; m < NDMA; ++m) {
        const unsigned q = (unsigned)((wave + 4 * m) * 64 + lane);
        const unsigned r = (q * 43691u) >> 22;                        // q / 96 for q < 4096
        const unsigned c = (q - r * 96u) ^ (r & 15u);
        const unsigned off = (r * (unsigned)g.lda + c * 8u) * 2u;
        s_doff[m][t] = off;                                           // read back by the lane that wrote it
        if (tile < ntile) wst_dma_so(reinterpret_cast<const char*>(A + (long)tile * ROWS * g.lda), off, lds0 + (unsigned)(wave + 4 * m) * 1024u);
    }
    if (tile + nstream < ntile) {                                     // all of the second tile BEHIND all of the first: the counted wait relies on it
#pragma unroll
        for (int m = 0; m < NDMA; ++m)
            wst_dma_so(reinterpret_cast<const char*>(A + (long)(tile + nstream) * ROWS * g.lda), s_doff[m][t],
                       lds0 + (unsigned)(TILE_EL * 2) + (unsigned)(wave + 4 * m) * 1024u);
    }
    // ---- W fragments: k-steps 0 .. 15 -> AGPRs (through the "a" constraint of their consumers), 16 .. 23 -> VGPRs -----------------------------
    v8 wa[4][KSA], wv[4][KS - KSA];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const T* wr = W + (long)(n0 + ct * 16 + l15) * g.ldb + gq * 8;
#pragma unroll
        for (int ks = 0; ks < KSA; ++ks) wa[ct][ks] = *reinterpret_cast<const v8*>(wr + ks * 32);
#pragma unroll
        for (int ks = KSA; ks < KS; ++ks) wv[ct][ks - KSA] = *reinterpret_cast<const v8*>(wr + ks * 32);
    }
    s_bias[t] = g.bias ? g.bias[slab * 256 + t] : 0.f;
    // the compiler's wait for the weight loads stands HERE, once.  Left to itself it keeps them pending into the tile loop (the bf16
    // instantiations load straight into AGPRs) and puts a `s_waitcnt vmcnt(n)`, n = 47 .. 0, in front of the first reader of every fragment
    // in EVERY tile: up to 32 scalar instructions between the MFMAs, and a vmcnt(0) among them drains the DMA pieces two tiles ahead
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
        for (int ks = 0; ks < KSA; ++ks) asm volatile("" : : "a"(wa[ct][ks]));
#pragma unroll
        for (int ks = 0; ks < KS - KSA; ++ks) asm volatile("" : : "v"(wv[ct][ks]));
    }
    // ---- fragment reads: k-step ks = 4 kh + kl of row block rt sits at chunk (16 kh + ((4 kl + gq) ^ l15)) of row rt * 16 + l15: four lane
    // offsets (kl), everything else is an immediate ----
    const unsigned short* xp[4];                                      // into ring buffer 0; they move on with the ring
#pragma unroll
    for (int kl = 0; kl < 4; ++kl) xp[kl] = &s_x[0][0] + (l15 * CPR + ((kl * 4 + gq) ^ l15)) * 8;
    auto xfrag = [&](int rt, int ks) { return *reinterpret_cast<const v8*>(xp[ks & 3] + rt * 16 * K + (ks >> 2) * 128); };
    auto bias4 = [&](int ct) { return *reinterpret_cast<const f4*>(&s_bias[wave * 64 + ct * 16 + gq * 4]); };

    const unsigned coff = ((unsigned)l15 * (unsigned)g.ldc + (unsigned)(n0 + gq * 4)) * 2u;     // the lane's byte offset in a 16-row block of C
    f4 acc[RT][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[1][ct] = f4{0.f, 0.f, 0.f, 0.f};   // the first row block drains this set before anything is in it
    v8 xq[4];
    u2 pend[RT][4];                                                   // four converted outputs of a lane: two registers
    f4 bv;
    unsigned dq = s_doff[0][t], pl = 0, ph = 0;                      // dq: the lane's source offset of the next DMA piece
    float rgmax = 0.f, tg = 0.f;
    float ex[4] = {0.f, 0.f, 0.f, 0.f}, ea[4] = {0.f, 0.f, 0.f, 0.f}, ep[4] = {0.f, 0.f, 0.f, 0.f}, et[4] = {0.f, 0.f, 0.f, 0.f};   // per chain
    // the two GELU constants that are register operands: opaque to the compiler, so that they stay where they are for the whole kernel
    float h4 = MI355_GELU16_H4, clampv = MI355_GELU_CLAMP;
    asm volatile("" : "+v"(h4), "+s"(clampv));
    static_assert(__builtin_bit_cast(unsigned, MI355_GELU16_H5) == 0xb9f82495u && __builtin_bit_cast(unsigned, MI355_GELU16_H3) == 0xbd5448beu &&
                  __builtin_bit_cast(unsigned, MI355_GELU16_H2) == 0xbeeb8427u && __builtin_bit_cast(unsigned, MI355_GELU16_H1) == 0xbf934d04u &&
                  __builtin_bit_cast(unsigned, MI355_GELU16_H0) == 0xbf80013cu, "the literals of the assembly below are gelu16_fast's coefficients");

    // Piece `code` of WstPlan for accumulator set `pv`.  The expressions are gelu16_fast's and the tile kernels' conversions, operation for
    // operation.  What the compiler no longer checks in here: v_exp_f32's result is read by the chain's NEXT piece (at least one MFMA later),
    // and an accumulator is first read eight MFMAs after the one that wrote it last.  bv holds the bias of column tile ct.
    // The range maximum is rg_absmax4_f in four instructions: the maximum of the four magnitudes g; g * 0 + g is g for a finite g and NaN
    // for inf and NaN; v_max_f32 returns the other operand for a NaN: a group that holds an inf leaves the running maximum alone.
    auto piece = [&](auto pvc, auto codec) {
        constexpr int pv = decltype(pvc)::v, code = decltype(codec)::v, ct = code >> 5, c = (code >> 2) & 3, p = code & 3;
        float &rgm = rgmax, &g4 = tg;                                  // named outside the dependent branches: the generic lambda captures them
        unsigned &lo = pl, &hi = ph;
        (void)rgm, (void)g4, (void)lo, (void)hi;
        if constexpr (!(code & 16)) {
            if constexpr (!GELU)
                asm volatile("v_add_f32_e32 %0, %1, %2" : "=v"(ex[c]) : "v"(acc[pv][ct][c]), "v"(bv[c]));
            else if constexpr (p == 0)
                asm volatile("v_add_f32_e32 %0, %3, %4\n\tv_min_f32_e64 %1, |%0|, %5\n\tv_fmamk_f32 %2, %1, 0xb9f82495, %6"
                             : "=&v"(ex[c]), "=&v"(ea[c]), "=&v"(ep[c])
                             : "v"(acc[pv][ct][c]), "v"(bv[c]), "s"(clampv), "v"(h4));
            else if constexpr (p == 1)
                asm volatile("v_fmaak_f32 %0, %0, %1, 0xbd5448be\n\tv_fmaak_f32 %0, %0, %1, 0xbeeb8427\n\t"
                             "v_fmaak_f32 %0, %0, %1, 0xbf934d04\n\tv_fmaak_f32 %0, %0, %1, 0xbf80013c"
                             : "+v"(ep[c])
                             : "v"(ea[c]));
            else if constexpr (p == 2)
                asm volatile("v_mul_f32_e32 %0, 0.5, %2\n\tv_exp_f32_e32 %1, %1" : "=&v"(et[c]), "+v"(ep[c]) : "v"(ex[c]));
            else
                asm volatile("v_fma_f32 %0, |%0|, 0.5, %1\n\tv_fma_f32 %0, -%2, %3, %0" : "+v"(ex[c]) : "v"(et[c]), "v"(ea[c]), "v"(ep[c]));
        } else if constexpr (p == 0) {
            if constexpr (F16)
                asm volatile("v_cvt_pk_f16_f32 %0, %3, %4\n\tv_cvt_pk_f16_f32 %1, %5, %6\n\tv_max3_f32 %2, |%3|, |%4|, |%5|\n\tv_max_f32_e64 %2, |%6|, %2"
                             : "=&v"(lo), "=&v"(hi), "=&v"(g4)
                             : "v"(ex[0]), "v"(ex[1]), "v"(ex[2]), "v"(ex[3]));
            else
                asm volatile("v_cvt_pk_bf16_f32 %0, %2, %3\n\tv_cvt_pk_bf16_f32 %1, %4, %5"
                             : "=&v"(lo), "=&v"(hi)
                             : "v"(ex[0]), "v"(ex[1]), "v"(ex[2]), "v"(ex[3]));
            pend[pv][ct] = u2{lo, hi};
        } else {
            asm volatile("v_fma_f32 %1, %1, 0, %1\n\tv_max_f32_e32 %0, %0, %1" : "+v"(rgm), "+v"(g4));
        }
    };

    // one row block: 96 slots.  ST: the deferred stores of this row block of the tile before exist (C rows at crow: wave-uniform, the stores add
    // one 32-bit lane offset); DMA: six pieces of the tile two ahead (source dbase, LDS byte address ddst); xstep: how far the fragment
    // pointers move on to the next ring buffer, once row block 1 has issued its last fragment read (slot 81)
    auto block = [&](auto rtc, auto dmac, auto stc, const char* crow, const char* dbase, unsigned ddst, int xstep) {
        constexpr int rt = decltype(rtc)::v;
        constexpr bool DMA = decltype(dmac)::v != 0, ST = decltype(stc)::v != 0;
        auto slot = [&](auto mc) {
            constexpr int m = decltype(mc)::v, ks = m >> 2, ct = m & 3;
            if constexpr (ks == 0)       wst_mfma_a0<T>(acc[rt][ct], wa[ct][0], xq[0]);
            else if constexpr (ks < KSA) wst_mfma_a<T>(acc[rt][ct], wa[ct][ks < KSA ? ks : 0], xq[ks & 3]);
            else                         wst_mfma_v<T>(acc[rt][ct], wv[ct][ks >= KSA ? ks - KSA : 0], xq[ks & 3]);
            if constexpr (ST && m < 4)
                asm volatile("global_store_dwordx2 %0, %1, %2 offset:%3" : : "v"(coff), "v"(pend[rt][m < 4 ? m : 0]), "s"(crow), "n"(m * 32) : "memory");
            if constexpr (m == 1) bv = bias4(0);
            if constexpr (ct == 1) {                                   // into the ring slot the k-step before has left
                constexpr int f = ks + 3;
                if constexpr (f < KS)       xq[f & 3] = xfrag(rt, f);
                else if constexpr (rt == 0) xq[f & 3] = xfrag(1, f - KS);
            }
            if constexpr (DMA && (m & 15) == 6) wst_dma_piece<(rt * 6 + (m >> 4)) * 4096>(dbase, dq, ddst);
            if constexpr (DMA && (m & 15) == 7)                        // the next piece's lane offset, fifteen slots ahead of its use: the
                dq = s_doff[(rt * 6 + (m >> 4) + 1) % NDMA][t];        // k-steps' own waits for their fragments cover it, none is added
            if constexpr (rt == 1 && m >= 84 && m < 88) xp[m >= 84 && m < 88 ? m - 84 : 0] += xstep;
            constexpr int code = wst_plan<GELU, F16>.code[m], rl = wst_plan<GELU, F16>.reload[m];
            if constexpr (code >= 0) piece(WstI<rt ^ 1>{}, WstI<(code >= 0 ? code : 0)>{});
            if constexpr (rl != 0) bv = bias4(rl);
            __builtin_amdgcn_sched_barrier(0);
        };
        WstUnroll<0, 96>::run(slot);
        // The MFMAs are opaque to the compiler: where the tile bodies meet (peeled / with / without DMA pieces, the drain) it moves the
        // accumulators of row block 1 into the registers the next body expects them in with VALU copies of its own, and it pads nothing
        // between them and the MFMA that has just written them (seen: a stale acc[1][3] in the rows 16-31 of every tile but a stream's first).
        // Twelve wait states (what an 8-pass MFMA asks for plus one) close every body, INSIDE it, in front of those copies.
        if constexpr (rt == 1) asm volatile("s_nop 11" : "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[1][2]), "+v"(acc[1][3]));
    };

    // `first` is a compile-time flag of the tile body (the first tile of a stream is peeled): no branch around the deferred stores
    int buf = 0, ahead = tile + (NB - 1) * nstream;
    const long dstride = (long)nstream * ROWS * g.lda * 2, cstride = (long)nstream * ROWS * g.ldc * 2;
    const char* dbase = reinterpret_cast<const char*>(A + (long)ahead * ROWS * g.lda);
    const char* crow = reinterpret_cast<const char*>(C + (long)(tile - nstream) * ROWS * g.ldc);   // the C rows of the tile BEFORE: stored one tile late
    auto do_tile = [&](auto firstc) {
        constexpr bool FIRST = decltype(firstc)::v != 0;
        if (tile + nstream < ntile) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");      // twelve pieces of the next tile were issued behind this one's
        else                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the last tile of the stream: nothing was
        WST_BAR();                                                     // the tile is complete in LDS; everybody is done with the previous one
#pragma unroll
        for (int f = 0; f < 3; ++f) xq[f] = xfrag(0, f);
        const unsigned ddst = lds0 + (unsigned)((buf + NB - 1) % NB) * (TILE_EL * 2) + (unsigned)wave * 1024u;   // the wave's first piece in the buffer the previous tile has just left
        const int xstep = buf == NB - 1 ? -(NB - 1) * TILE_EL : TILE_EL;
        const bool dma = ahead < ntile;
        __builtin_amdgcn_sched_barrier(0);
        if (dma) {
            block(WstI<0>{}, WstI<1>{}, WstI<!FIRST>{}, crow, dbase, ddst, xstep);
            if constexpr (FIRST) rgmax = 0.f;                          // row block 0 of the first tile drained an empty set
            block(WstI<1>{}, WstI<1>{}, WstI<!FIRST>{}, crow + 32 * (long)g.ldc, dbase, ddst, xstep);
        } else {
            block(WstI<0>{}, WstI<0>{}, WstI<!FIRST>{}, crow, dbase, ddst, xstep);
            if constexpr (FIRST) rgmax = 0.f;
            block(WstI<1>{}, WstI<0>{}, WstI<!FIRST>{}, crow + 32 * (long)g.ldc, dbase, ddst, xstep);
        }
        ahead += nstream;
        dbase += dstride;
        crow += cstride;
        buf = buf == NB - 1 ? 0 : buf + 1;
    };
    if (tile < ntile) {
        do_tile(WstI<1>{});
        for (tile += nstream; tile < ntile; tile += nstream) do_tile(WstI<0>{});
        // drain: row block 0 of the last tile waits in pend[0], row block 1 in acc[1]; crow has moved on to the last tile's rows
        char* cw = const_cast<char*>(crow);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) *reinterpret_cast<u2*>(cw + coff + ct * 32) = pend[0][ct];
        bv = bias4(0);                                                 // (the last MFMAs have retired: the wait states that close every tile)
        auto tail = [&](auto mc) {                                     // the pieces of the plan in its order, no MFMAs between them
            constexpr int m = decltype(mc)::v, code = wst_plan<GELU, F16>.code[m], rl = wst_plan<GELU, F16>.reload[m];
            if constexpr (code >= 0) piece(WstI<1>{}, WstI<(code >= 0 ? code : 0)>{});
            if constexpr (rl != 0) bv = bias4(rl);
        };
        WstUnroll<0, 96>::run(tail);
        cw += 32 * (long)g.ldc;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) *reinterpret_cast<u2*>(cw + coff + ct * 32) = pend[1][ct];
    }
    if constexpr (F16) rg_report_f(rgmax, g.ovf, 3u);
}

}  // namespace

namespace mi355 {

// MI355_EUNSUPPORTED (nothing launched) unless the product is one this schedule is built for: 16-bit output, K = 768 and
//   one_wave (the default route of linear16_dispatch, and options 3 / 4): N a multiple of 256, M of 32 -- any number of row tiles, streams of
//            0, 1, 2 ... tiles included: how many rows make the kernel worth its weight prologue is the dispatch's business;
//   otherwise (options 1 / 2): N a multiple of 192, at least eight row tiles per workgroup of a slab.
int gemm16_wst(const G16Args& g, int out16, int precision, hipStream_t st, bool one_wave) {
    one_wave = one_wave || opt(O_GEMM_WST) == 3 || opt(O_GEMM_WST) == 4;
    if (!out16 || g.K != 768 || (g.N % (one_wave ? 256 : 192)) || g.resid || g.gamma || g.resid_period || g.rowtau || g.lnc_a || g.row_stats || g.ln16_out)
        return MI355_EUNSUPPORTED;
    if (g.act != MI355_ACT_NONE && g.act != MI355_ACT_GELU) return MI355_EUNSUPPORTED;
    if ((g.lda & 7) || (g.ldb & 7) || (g.ldc & 3) || !aligned16(g.A) || !aligned16(g.B) || !aligned16(g.C) || (g.bias && !aligned16(g.bias)))
        return MI355_EUNSUPPORTED;
    if (precision != MI355_PREC_FP16 && precision != MI355_PREC_BF16) return MI355_EUNSUPPORTED;
    const int ncu = resident_slots(1);
    const int nslab = g.N / (one_wave ? 256 : 192);
    if (nslab > ncu) return MI355_EUNSUPPORTED;
    if (one_wave ? ((g.M & 31) || (long)g.lda * 32 * 2 >= (1L << 31) || (long)g.ldc * 32 * 2 >= (1L << 31)) : (long)g.M < 32L * 8 * (ncu / nslab)) return MI355_EUNSUPPORTED;
    MI355_TRACE(st, "gemm16_wst_kernel<%s,out16> M=%d N=%d K=%d%s", precision == MI355_PREC_FP16 ? "f16" : "bf16", g.M, g.N, g.K,
                g.act == MI355_ACT_GELU ? " gelu" : "");
    if (one_wave) {                                                     // one wave per SIMD, weight fragments in AGPRs (256-column slabs, M % 32 == 0)
        const int ns = nslab;
        if (g.act == MI355_ACT_GELU) {
            if (precision == MI355_PREC_FP16) gemm16_wst1_kernel<_Float16, true><<<ncu, 256, 0, st>>>(g, ns);
            else                              gemm16_wst1_kernel<__bf16, true><<<ncu, 256, 0, st>>>(g, ns);
        } else {
            if (precision == MI355_PREC_FP16) gemm16_wst1_kernel<_Float16, false><<<ncu, 256, 0, st>>>(g, ns);
            else                              gemm16_wst1_kernel<__bf16, false><<<ncu, 256, 0, st>>>(g, ns);
        }
        return MI355_OK;
    }
    if (g.act == MI355_ACT_GELU) {
        if (precision == MI355_PREC_FP16) gemm16_wst_kernel<_Float16, true><<<ncu, 512, 0, st>>>(g, nslab);
        else                              gemm16_wst_kernel<__bf16, true><<<ncu, 512, 0, st>>>(g, nslab);
    } else {
        if (precision == MI355_PREC_FP16) gemm16_wst_kernel<_Float16, false><<<ncu, 512, 0, st>>>(g, nslab);
        else                              gemm16_wst_kernel<__bf16, false><<<ncu, 512, 0, st>>>(g, nslab);
    }
    return MI355_OK;
}

}  // namespace mi355
