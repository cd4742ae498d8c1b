// attn_split.hip -- the QK^T-softmax-PV core of ViT Attention (ViT.py:82-86) for precision 3 ("logit-compensated"), gfx950.
//
// attn.hip's win_attn_kernel dataflow for one window = the whole sequence (N <= 224), no LePE, 16-bit I/O, with the two halves of the
// block in different operand formats:
//     S^T = K . Q^T      on bf16 hi / lo PAIRS through mma_step<0> (K hi and K lo both parked in LDS, Q hi / lo fragments straight from
//                        HBM): hi.hi + hi.lo + lo.hi, i.e. logits of fp32 class whatever their size (profiles/logit_mode.md)
//     softmax over keys  in registers, fp32
//     O   = P . V        P rounded to fp16 in-lane, V^T (fp16) from LDS, Mma<1>; the row sum comes off the matrix pipe (ones tile)
//     O  /= rowsum       written as fp16 rows, ready for the proj GEMM (mi355_linear16_fwd, precision 1)
// Input: the five-plane rows of mi355_qkv_split16_fwd, (B, N, 5C): [q_hi | q_lo | k_hi | k_lo | v], head h = columns [h d, (h + 1) d) of
// every plane.  A kernel of its own (not another instantiation of win_attn_kernel): that kernel's instantiations and arguments stay as
// they are.  P is in [0, 1]; the context, the one other value converted to fp16 here, reports into the range word (code 7, the attention
// cores' code) like every fp16 conversion of the library.
// LDS at d = 64, 14 key tiles: K 2 x 224 x 72 x 2 B + V^T 64 x 228 x 2 B + O slabs 8 x 16 x 72 x 2 B = 110 KB (one workgroup per CU).
#include "common.h"
#include "mma.h"
#include "bufops.h"

namespace {

struct SplitAttnArgs {
    const unsigned short* qkv5;   // (B, N, 5C)
    unsigned short* out;          // (B, N, C) fp16
    int N, C, heads;
    float scale;
    unsigned* ovf;                // fp16 range word or null
};

// KT key tiles of 16 (padded key count), NW waves share one head's K / V; TFULL: key tiles known at compile time to lie below N (their
// scores skip the validity mask), -1 = unknown.
template <int D, int KT, int NW, int TFULL>
__global__ __launch_bounds__(NW * 64, 1) void split_attn_kernel(const SplitAttnArgs a) {
    using L_ = Mma<0>;                        // logit operands: bf16 pairs
    using V_ = Mma<1>;                        // value operands: fp16
    constexpr int NTHR = NW * 64;
    constexpr int TK = KT * 16;               // padded key count
    constexpr int KP = D + 8;                 // K row pitch (elements)
    constexpr int VP = TK + 4;                // V^T row pitch (elements, multiple of 4 -> 8-byte aligned reads)
    constexpr int OP = D + 8;                 // O slab pitch
    constexpr int K_EL = TK * KP;
    constexpr int D8 = D / 8;
    __shared__ __attribute__((aligned(16))) unsigned short s_k[2 * K_EL];      // [hi | lo][key][d]
    __shared__ __attribute__((aligned(16))) unsigned short s_v[D * VP];        // [d][key]
    __shared__ __attribute__((aligned(16))) unsigned short s_o[NW * 16 * OP];

    const int lid = xcd_contiguous_block();   // heads of one image are neighbours: they share the image's rows in one L2
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int head = lid % a.heads, b = lid / a.heads;
    const int T = a.N, C = a.C;
    const int row5 = 5 * C;
    const unsigned short* base = a.qkv5 + (long)b * T * row5 + head * D;        // this head's q_hi slice of token 0
    const int l15 = lane & 15, g = lane >> 4;
    const int nqt = (T + 15) >> 4;
    constexpr int NQ = (KT + NW - 1) / NW;    // query tiles per wave

    // everything goes through one raw buffer descriptor over the image: slots past T get an out-of-range offset and come back as zeros
    const rsrc_t img_rs = make_rsrc(base, (bufops_u32)(((long)T * row5 - head * D) * 2));
    auto ld16 = [&](bool live, int token, int el_off) -> L_::v8 {
        const bufops_u32 off = live ? (bufops_u32)((token * row5 + el_off) * 2) : OOB;
        return __builtin_bit_cast(L_::v8, __builtin_amdgcn_raw_buffer_load_b128(img_rs, off, 0, 0));
    };
    // ---- all loads of the workgroup are issued up front: Q hi / lo fragments of this wave's query tiles, then K hi / lo and V ------------
    L_::v8 qf[NQ][D / 32][2];
#pragma unroll
    for (int iq = 0; iq < NQ; ++iq) {
        const int qs = (wave + iq * NW) * 16 + l15;
#pragma unroll
        for (int ks = 0; ks < D / 32; ++ks)
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) qf[iq][ks][sp] = ld16(qs < T, qs, sp * C + ks * 32 + g * 8);
    }
    constexpr int NKI = (TK * D8 + NTHR - 1) / NTHR, NVI = ((TK / 4) * D8 + NTHR - 1) / NTHR;
    L_::v8 kreg[NKI][2];
    L_::v8 vreg[NVI][4];
#pragma unroll
    for (int it = 0; it < NKI; ++it) {
        const int idx = t + it * NTHR, key = idx / D8, d8 = idx % D8;
        const bool live = idx < TK * D8 && key < T;
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) kreg[it][sp] = ld16(live, key, (2 + sp) * C + d8 * 8);
    }
#pragma unroll
    for (int it = 0; it < NVI; ++it) {
        const int idx = t + it * NTHR, kg = idx / D8, d8 = idx % D8;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int key = kg * 4 + j;
            vreg[it][j] = ld16(idx < (TK / 4) * D8 && key < T, key, 4 * C + d8 * 8);
        }
    }
    // ---- phase A: K -> LDS [key][d] (two planes), V -> LDS transposed [d][key] through a 4 (key) x 8 (d) register transpose ------------
#pragma unroll
    for (int it = 0; it < NKI; ++it) {
        const int idx = t + it * NTHR, key = idx / D8, d8 = idx % D8;
        if (idx < TK * D8) {
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) *reinterpret_cast<L_::v8*>(s_k + sp * K_EL + key * KP + d8 * 8) = kreg[it][sp];
        }
    }
#pragma unroll
    for (int it = 0; it < NVI; ++it) {
        const int idx = t + it * NTHR, kg = idx / D8, d8 = idx % D8;
        if (idx < (TK / 4) * D8) {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                *reinterpret_cast<L_::v4*>(s_v + (d8 * 8 + q) * VP + kg * 4) =
                    L_::v4{vreg[it][0][q], vreg[it][1][q], vreg[it][2][q], vreg[it][3][q]};      // 16-bit moves: the element type is irrelevant
        }
    }
    __syncthreads();

    // ---- phase B: each wave owns 16-query tiles ----------------------------------------------------------------------------------
    unsigned short* slab = s_o + wave * 16 * OP;
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float post = a.scale * 1.44269504088896340736f;     // logits in log2 units: p = 2^(s post - m post)
    float rgm = 0.f;                                           // fp16 range guard of the context values
#pragma unroll
    for (int iq = 0; iq < NQ; ++iq) {
        const int qt = wave + iq * NW;
        if (qt >= nqt) break;
        // S^T tiles: lane holds S^T[key = kt*16 + g*4 + r][q = l15]
        f4 s[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            f4 acc = zero4;
            if (kt < TFULL || kt * 16 < T) {
#pragma unroll
                for (int ks = 0; ks < D / 32; ++ks) {
                    L_::v8 kf[2];
#pragma unroll
                    for (int sp = 0; sp < 2; ++sp)
                        kf[sp] = *reinterpret_cast<const L_::v8*>(s_k + sp * K_EL + (kt * 16 + l15) * KP + ks * 32 + g * 8);
                    acc = mma_step<0>(kf, qf[iq][ks], acc);
                }
            }
            s[kt] = acc;
        }
        // softmax over keys (masked beyond T): maximum over the raw scores (post > 0), one fma in front of the v_exp
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt * 16 + g * 4 + r;
                const float v = (kt < TFULL || key < T) ? s[kt][r] : -INFINITY;
                s[kt][r] = v;
                m = fmaxf(m, v);
            }
        m = fmaxf(m, __shfl_xor(m, 16, WAVE));
        m = fmaxf(m, __shfl_xor(m, 32, WAVE));
        const float mneg = -(m * post);
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kt][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][r], post, mneg));   // fma(-inf, post, .) = -inf -> 0
        // O^T = V^T . P^T : A = V^T (row d = l15, k enumerates keys as (tile 2kb, g, r) then (tile 2kb+1, g, r)); B = P^T, the S^T
        // accumulators re-packed in-lane -> lane holds O[q = l15][d = nt*16 + g*4 + r]; a ones tile as A gives the row sum of the very
        // P values (rounded to fp16) that enter the numerator
        f4 o[D / 16];
#pragma unroll
        for (int nt = 0; nt < D / 16; ++nt) o[nt] = zero4;
        f4 osum = zero4;
        const V_::v8 ones = V_::v8{(_Float16)1.0f, (_Float16)1.0f, (_Float16)1.0f, (_Float16)1.0f, (_Float16)1.0f, (_Float16)1.0f,
                                   (_Float16)1.0f, (_Float16)1.0f};
#pragma unroll
        for (int kb = 0; kb < KT / 2; ++kb) {
            if (2 * kb < TFULL || kb * 32 < T) {
                const V_::v4 h0 = V_::cvt(s[2 * kb]), h1 = V_::cvt(s[2 * kb + 1]);
                const V_::v8 pf = V_::v8{h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
                for (int nt = 0; nt < D / 16; ++nt) {
                    const unsigned short* vr = s_v + (nt * 16 + l15) * VP + kb * 32 + g * 4;
                    const V_::v4 a0 = *reinterpret_cast<const V_::v4*>(vr);
                    const V_::v4 a1 = *reinterpret_cast<const V_::v4*>(vr + 16);
                    o[nt] = V_::mma(V_::v8{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, pf, o[nt]);
                }
                osum = V_::mma(ones, pf, osum);
            }
        }
        const float inv = __builtin_amdgcn_rcpf(osum.x);
#pragma unroll
        for (int nt = 0; nt < D / 16; ++nt) {
            const f4 val = o[nt] * inv;
            rgm = rg_absmax4(rgm, val);
            *reinterpret_cast<V_::v4*>(slab + l15 * OP + nt * 16 + g * 4) = V_::cvt(val);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // row-contiguous stores: 16 bytes per lane
        constexpr int LPR = D / 8, RPI = 64 / LPR;
#pragma unroll
        for (int it = 0; it < 16 / RPI; ++it) {
            const int r = it * RPI + lane / LPR, c8 = (lane % LPR) * 8;
            const int qslot = qt * 16 + r;
            if (qslot < T)
                *reinterpret_cast<V_::v8*>(a.out + ((long)b * T + qslot) * C + head * D + c8) = *reinterpret_cast<const V_::v8*>(slab + r * OP + c8);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    rg_report(rgm, a.ovf, 7u);
}

template <int D>
int launch_split(const SplitAttnArgs& a, int B, hipStream_t st) {
    const int grid = B * a.heads;
    MI355_TRACE(st, "split_attn_kernel<d=%d> B=%d heads=%d tokens=%d", D, B, a.heads, a.N);
    const int T = a.N;
    if (T <= 64) { if (T >= 48) split_attn_kernel<D, 4, 4, 3><<<grid, 256, 0, st>>>(a); else split_attn_kernel<D, 4, 4, -1><<<grid, 256, 0, st>>>(a); }
    else if (T <= 128) { if (T >= 96) split_attn_kernel<D, 8, 4, 6><<<grid, 256, 0, st>>>(a); else split_attn_kernel<D, 8, 4, -1><<<grid, 256, 0, st>>>(a); }
    else if (T >= 192) split_attn_kernel<D, 14, 8, 12><<<grid, 512, 0, st>>>(a);
    else split_attn_kernel<D, 14, 8, -1><<<grid, 512, 0, st>>>(a);
    return MI355_OK;
}

}  // namespace

extern "C" int mi355_sdpa16_split_fwd(const void* qkv5, void* out16, int B, int N, int heads, int d, float scale, mi355_stream_t stream) {
    MI355_CHECK_ARG(qkv5 && out16 && B > 0 && N > 0 && heads > 0);
    if (!(d == 32 || d == 64)) return mi355::fail(MI355_EUNSUPPORTED, "mi355_sdpa16_split_fwd: head dim %d (built: 32, 64)", d);
    if (N > 224) return mi355::fail(MI355_EUNSUPPORTED, "mi355_sdpa16_split_fwd: sequence length %d > 224 (single-pass softmax core)", N);
    MI355_CHECK_ARG(aligned16(qkv5) && aligned16(out16) && (long)B * heads < (1L << 31) && (long)N * 5 * heads * d * 2 < (1L << 31));
    hipStream_t st = static_cast<hipStream_t>(stream);
    SplitAttnArgs a{static_cast<const unsigned short*>(qkv5), static_cast<unsigned short*>(out16), N, heads * d, heads, scale,
                    mi355::range_word(st)};                  // the context is converted to fp16: a producer
    int rc = d == 64 ? launch_split<64>(a, B, st) : launch_split<32>(a, B, st);
    if (rc) return rc;
    MI355_LAUNCH_CHECK();
    return MI355_OK;
}
