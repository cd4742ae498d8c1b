// sk_wide.hip -- SKLayer's two grouped 3x3 branches (sk_module.py:41-46) as a grouped implicit GEMM on the matrix cores, for every
// planes / groups and Cin / groups: per group, D[output channel][pixel] = sum_k W[output channel][k] * X[k][pixel] with
// k = (tap, input channel).  Operands are split-bf16 (mma.h, Mma<0>: hi.hi + hi.lo + lo.hi, fp32 accumulation), so the results
// stay fp32-class and nothing can saturate.
//
// A workgroup (256 threads, 4 waves) owns (image, group, tile of NT * 16 output channels, band).  A band is BR rows x WCT column tiles
// of 16 pixels, at most 16 pixel tiles: a wave owns up to MT = 4 of them and keeps their accumulators of both branches in registers
// while the workgroup walks the group's input channels in chunks of CK (a multiple of 8, chosen on the host so that the tile fits).
//
// LDS tile of a chunk: (BR + 4) x (WCT * 16 + 4) pixels (zero halo of two rows and two columns: both dilations read it), pixel-major,
// the CK channels of a pixel contiguous at a pitch of CP bf16 with CP / 8 odd, one image for the hi halves and one for the lo halves.
// A lane's K fragment (one tap, 8 consecutive channels) is one 16-byte read; the 16 pixels of a lane group fall on 16 different
// 16-byte slots of the 256-byte bank row because the pitch is an odd number of slots.  Every carve offset is a multiple of 16 bytes.
//
// K order inside a chunk: (tap, channel octet), padded with zero weights to a multiple of 4 pairs; a 16x16x32 step is four pairs, one
// per lane group.  sk_wide_pack_kernel writes the weights once per call as [branch][hi | lo][group * COGP + o][chunk][K of a chunk]
// (COGP = planes / groups rounded up to 16) and the main kernel reads its A fragments from there (16 bytes per lane, L2-resident).
//
// D fragment: lane l holds pixel (l & 15) of 4 output channels (l >> 4) * 4 + [0, 4): a store instruction writes 16 consecutive
// pixels of a plane.  Pooled sums: lanes -> 16-lane butterfly -> one LDS slot per (wave, channel) -> added in wave order; one
// value per (image, channel, band), no atomics.
//
// Range guard: every conversion in this file is to bfloat16, which has the fp32 exponent range, so there is no saturation to report:
// no rg_report call and no range_word() here (common.h, "fp16 range guard": bf16 operands are not checked).  A kernel that gains an
// fp16 operand mode must add both.
#include "common.h"
#include "mma.h"

namespace {

#define SKW_ZERO8 __builtin_bit_cast(b8, f4{0.f, 0.f, 0.f, 0.f})
constexpr int SKW_MT = 4;                 // pixel tiles per wave
constexpr int SKW_LDS_BUDGET = 60 * 1024; // dynamic LDS of the main kernel (64 KB less the static reduction slots and slack)

struct SkWideArgs {
    const float* x;
    const __bf16* wp;                     // packed weights
    const float *sc1, *sh1, *sc2, *sh2;
    float *u1, *u2, *pooled;
    int Cin, planes, groups, cog, cin_g, H, W;
    int cogp, nct;                        // padded output channels per group, output-channel tiles of NT * 16 per group
    int BR, WCT, nrb, ncb;                // band geometry: rows, column tiles; bands along H and along W
    int CK, CP, chunks, KC;               // channels per chunk, LDS pixel pitch (bf16), chunks, K of a chunk (multiple of 32)
    long ocp_total;                       // groups * cogp
};

__global__ __launch_bounds__(256) void sk_wide_pack_kernel(const float* __restrict__ w1, const float* __restrict__ w2, __bf16* __restrict__ wp,
                                                          int groups, int cog, int cogp, int cin_g, int CK, int KC, int chunks, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long Ktot = (long)chunks * KC;
    const int k = (int)(idx % Ktot);
    long q = idx / Ktot;
    const long ocp_total = (long)groups * cogp;
    const long oc = q % ocp_total;
    q /= ocp_total;
    const int h = (int)(q & 1), br = (int)(q >> 1);
    const int chunk = k / KC, kk = k - chunk * KC, pair = kk >> 3, e = kk & 7, noct = CK >> 3;
    const int tap = pair / noct, oct = pair - tap * noct;
    const int c = chunk * CK + oct * 8 + e;
    const int g = (int)(oc / cogp), o = (int)(oc - (long)g * cogp);
    float v = 0.f;
    if (tap < 9 && c < cin_g && o < cog) v = (br ? w2 : w1)[(((long)g * cog + o) * cin_g + c) * 9 + tap];
    const __bf16 hi = (__bf16)v;
    wp[idx] = h ? (__bf16)(v - (float)hi) : hi;
}

template <int NT>
__global__ __launch_bounds__(256) void sk_wide_kernel(SkWideArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float red[4][NT * 16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, pix = lane & 15, lg = lane >> 4;
    const int nb = a.nrb * a.ncb;
    long bid = blockIdx.x;
    const int band = (int)(bid % nb); bid /= nb;
    const int ct = (int)(bid % a.nct); bid /= a.nct;
    const int g = (int)(bid % a.groups);
    const int b = (int)(bid / a.groups);
    const int rb = band / a.ncb, cb = band - rb * a.ncb;
    const int i0 = rb * a.BR, j0 = cb * a.WCT * 16;
    const int rows_here = min(a.BR, a.H - i0);
    const int ctiles_here = min(a.WCT, (a.W - j0 + 15) >> 4);
    const int ntiles = rows_here * ctiles_here;
    const int ROWS = a.BR + 4, COLS = a.WCT * 16 + 4, CP = a.CP, noct = a.CK >> 3;
    const int img = ROWS * COLS * CP;                            // bf16 elements of one image (hi or lo); CP % 8 == 0: 16-byte multiple
    __bf16* t_hi = reinterpret_cast<__bf16*>(smem);
    __bf16* t_lo = t_hi + img;
    const long HW = (long)a.H * a.W;
    const float* xg = a.x + ((long)b * a.Cin + (long)g * a.cin_g) * HW;
    const int ntn = min(NT, (a.cogp >> 4) - ct * NT);            // 16-channel tiles of this workgroup that exist
    const long oc_base = (long)g * a.cogp + (long)ct * NT * 16;  // first packed output channel
    const long Ktot = (long)a.chunks * a.KC;

    // the wave's pixel tiles: tile = wave * MT + m -> (row r, column tile c) of the band; LDS pixel index of its lane's pixel at tap (1,1)
    int tpix[SKW_MT];
    bool tok[SKW_MT];
#pragma unroll
    for (int m = 0; m < SKW_MT; ++m) {
        const int tile = wave * SKW_MT + m;
        tok[m] = tile < ntiles;
        const int r = tok[m] ? tile / ctiles_here : 0, c = tok[m] ? tile - r * ctiles_here : 0;
        tpix[m] = (r + 2) * COLS + c * 16 + pix + 2;
    }
    f4 acc[SKW_MT][2][NT];
#pragma unroll
    for (int m = 0; m < SKW_MT; ++m)
#pragma unroll
        for (int br = 0; br < 2; ++br)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][br][n] = f4{0.f, 0.f, 0.f, 0.f};

    // A fragments of one 32-deep step: 16 bytes per lane and (branch, channel tile, hi | lo) from the packed weights.  With one channel
    // tile they are fetched one step ahead -- the first before the tile is staged -- so that their L2 latency hides behind the staging
    // and the MFMAs.  With two tiles the second set of 32 registers costs the third wave per SIMD (212 instead of 164 VGPRs) and measured
    // slower (SKNet stage 4: 103 against 82 us), so there the step loads its own.
    constexpr bool PREFETCH = NT == 1;
    auto load_w = [&](long kl, b8 (&w)[2][NT][2]) {
        const __bf16* wk = a.wp + kl + lg * 8;
#pragma unroll
        for (int br = 0; br < 2; ++br)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (n < ntn) w[br][n][h] = *reinterpret_cast<const b8*>(wk + ((long)(br * 2 + h) * a.ocp_total + oc_base + n * 16 + pix) * Ktot);
                    else         w[br][n][h] = SKW_ZERO8;
                }
    };
    b8 wnext[2][NT][2];
    if constexpr (PREFETCH) load_w(0, wnext);

    for (int chunk = 0; chunk < a.chunks; ++chunk) {
        if (chunk) __syncthreads();                              // every wave is done with the previous chunk's tile
        // stage: one item = one pixel of the tile x one channel octet; consecutive threads take consecutive columns
        const int c0 = chunk * a.CK;
#pragma unroll 2
        for (int item = t; item < noct * ROWS * COLS; item += 256) {
            const int cc = item % COLS, rr = (item / COLS) % ROWS, oct = item / (COLS * ROWS);
            const int i = i0 - 2 + rr, j = j0 - 2 + cc;
            const bool in = i >= 0 && i < a.H && j >= 0 && j < a.W;
            b8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = c0 + oct * 8 + e;
                const float v = (in && c < a.cin_g) ? xg[(long)c * HW + (long)i * a.W + j] : 0.f;
                const __bf16 h = (__bf16)v;
                hi[e] = h;
                lo[e] = (__bf16)(v - (float)h);
            }
            const int off = (rr * COLS + cc) * CP + oct * 8;
            *reinterpret_cast<b8*>(t_hi + off) = hi;
            *reinterpret_cast<b8*>(t_lo + off) = lo;
        }
        __syncthreads();
        for (int ks = 0; ks < a.KC; ks += 32) {
            const int pair = (ks >> 3) + lg;
            const int tap = pair / noct, oct = pair - tap * noct;
            const bool kvalid = tap < 9;
            const int u = kvalid ? tap / 3 : 1, v = kvalid ? tap - u * 3 : 1;
            const int d1 = ((u - 1) * COLS + (v - 1)) * CP + (kvalid ? oct : 0) * 8;       // dilation 1, relative to the centre pixel
            const int d2 = (2 * (u - 1) * COLS + 2 * (v - 1)) * CP + (kvalid ? oct : 0) * 8;   // dilation 2
            b8 wa[2][NT][2];
            const long kl = (long)chunk * a.KC + ks;
            if constexpr (PREFETCH) {
#pragma unroll
                for (int br = 0; br < 2; ++br)
#pragma unroll
                    for (int h = 0; h < 2; ++h) wa[br][0][h] = wnext[br][0][h];
                if (kl + 32 < Ktot) load_w(kl + 32, wnext);      // the next step's weights (the next chunk's first step behind the last)
            } else {
                load_w(kl, wa);
            }
#pragma unroll
            for (int m = 0; m < SKW_MT; ++m) {
                if (!tok[m]) continue;                           // wave-uniform
#pragma unroll
                for (int br = 0; br < 2; ++br) {
                    const int off = tpix[m] * CP + (br ? d2 : d1);
                    b8 xb[2];
                    xb[0] = *reinterpret_cast<const b8*>(t_hi + off);
                    xb[1] = *reinterpret_cast<const b8*>(t_lo + off);
                    if (!kvalid) { xb[0] = SKW_ZERO8; xb[1] = xb[0]; }
#pragma unroll
                    for (int n = 0; n < NT; ++n) acc[m][br][n] = mma_step<0>(wa[br][n], xb, acc[m][br][n]);
                }
            }
        }
    }

    // epilogue: folded BatchNorm + ReLU, u1 / u2 in NCHW, the band's share of sum_hw (u1 + u2)
    float psum[NT][4];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q) psum[n][q] = 0.f;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int o = (ct * NT + n) * 16 + lg * 4 + q;       // output channel inside the group
            if (o >= a.cog) continue;
            const int ch = g * a.cog + o;
            const float s1 = a.sc1[ch], t1 = a.sh1[ch], s2 = a.sc2[ch], t2 = a.sh2[ch];
            const long plane = ((long)b * a.planes + ch) * HW;
#pragma unroll
            for (int m = 0; m < SKW_MT; ++m) {
                if (!tok[m]) continue;
                const int tile = wave * SKW_MT + m, r = tile / ctiles_here, c = tile - r * ctiles_here;
                const int i = i0 + r, j = j0 + c * 16 + pix;
                if (j < a.W) {                                   // i < H: r < rows_here
                    const float r1 = fmaxf(acc[m][0][n][q] * s1 + t1, 0.f), r2 = fmaxf(acc[m][1][n][q] * s2 + t2, 0.f);
                    a.u1[plane + (long)i * a.W + j] = r1;
                    a.u2[plane + (long)i * a.W + j] = r2;
                    psum[n][q] += r1 + r2;
                }
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float s = psum[n][q];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);   // the 16 pixel lanes of the lane group
            if (pix == 0) red[wave][n * 16 + lg * 4 + q] = s;
        }
    __syncthreads();
    if (t < NT * 16) {
        const int o = ct * NT * 16 + t;
        if (o < a.cog)
            a.pooled[((long)b * a.planes + (long)g * a.cog + o) * nb + band] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    }
}

// band geometry and channel chunk for a shape: everything the workspace query and the launch must agree on
struct SkWidePlan {
    int cog, cin_g, cogp, NT, nct, BR, WCT, nrb, ncb, nb, CK, CP, chunks, KC;
    size_t lds, pack_elems;
};

int pitch_of(int ck) { return ((ck >> 3) & 1) ? ck : ck + 8; }      // bf16 per pixel: an odd number of 16-byte slots

SkWidePlan make_plan(int Cin, int planes, int groups, int H, int W) {
    SkWidePlan p{};
    p.cog = planes / groups; p.cin_g = Cin / groups;
    p.cogp = (p.cog + 15) & ~15;
    p.NT = p.cogp == 16 ? 1 : 2;
    p.nct = cdiv(p.cogp / 16, p.NT);
    const int WT = cdiv(W, 16);
    p.ncb = cdiv(WT, 4);
    p.WCT = cdiv(WT, p.ncb);
    p.ncb = cdiv(WT, p.WCT);
    int BR = (4 * SKW_MT) / p.WCT;
    if (BR > H) BR = H;
    const int COLS = p.WCT * 16 + 4;
    int CK = (p.cin_g + 7) & ~7;
    auto bytes = [&](int ck, int br) { return (size_t)4 * (br + 4) * COLS * pitch_of(ck); };
    while (CK > 8 && bytes(CK, BR) > (size_t)SKW_LDS_BUDGET) CK = ((CK / 2) + 7) & ~7;
    while (BR > 1 && bytes(CK, BR) > (size_t)SKW_LDS_BUDGET) --BR;     // not reached: 8 channels of 8 x 68 pixels are 17 KB
    p.nrb = cdiv(H, BR);
    p.BR = cdiv(H, p.nrb);
    p.nrb = cdiv(H, p.BR);
    p.nb = p.nrb * p.ncb;
    p.CK = CK; p.CP = pitch_of(CK);
    p.chunks = cdiv(p.cin_g, CK);
    p.KC = ((9 * (CK / 8) + 3) & ~3) * 8;
    p.lds = bytes(CK, p.BR);
    p.pack_elems = (size_t)4 * groups * p.cogp * p.chunks * p.KC;
    return p;
}

size_t fl(size_t n) { return (n + 63) & ~(size_t)63; }

}  // namespace

namespace mi355 {

// floats the wide route adds behind the old workspace planes: its pooled partial sums (B, planes, bands) and the packed weights
size_t sk_wide_extra_floats(int B, int Cin, int planes, int groups, int H, int W) {
    const SkWidePlan p = make_plan(Cin, planes, groups, H, W);
    return fl((size_t)B * planes * p.nb) + fl((p.pack_elems + 1) / 2);
}

// u1 / u2 and the band-wise pooled sums of both branches; *nb_out = bands per (image, channel) of `pooled`.  `extra` is the region
// sk_wide_extra_floats() sizes (16-byte aligned); *pooled_out points into it.
int sk_wide(const float* x, const float* const* p, float* u1, float* u2, float* extra, float** pooled_out, int* nb_out, int B, int Cin,
            int planes, int groups, int H, int W, hipStream_t st) {
    const SkWidePlan pl = make_plan(Cin, planes, groups, H, W);
    const long blocks = (long)B * groups * pl.nct * pl.nb;
    if (blocks > 0x7fffffffL)
        return fail(MI355_EUNSUPPORTED, "mi355_sk_fwd: B * groups * channel tiles * bands = %ld workgroups exceed the grid (2^31 - 1)", blocks);
    const long pack_blocks = (long)((pl.pack_elems + 255) / 256);
    if (pack_blocks > 0x7fffffffL) return fail(MI355_EUNSUPPORTED, "mi355_sk_fwd: %zu packed weights exceed the grid", pl.pack_elems);
    float* pooled = extra;
    __bf16* wp = reinterpret_cast<__bf16*>(extra + fl((size_t)B * planes * pl.nb));
    {
        MI355_TRACE(st, "sk_wide_pack_kernel cog=%d cin=%d chunks=%d", pl.cog, pl.cin_g, pl.chunks);
        sk_wide_pack_kernel<<<(int)pack_blocks, 256, 0, st>>>(p[MI355_SK_CONV3_W], p[MI355_SK_CONV5_W], wp, groups, pl.cog, pl.cogp, pl.cin_g, pl.CK,
                                                              pl.KC, pl.chunks, (long)pl.pack_elems);
    }
    SkWideArgs a{};
    a.x = x; a.wp = wp;
    a.sc1 = p[MI355_SK_CONV3_SCALE]; a.sh1 = p[MI355_SK_CONV3_SHIFT]; a.sc2 = p[MI355_SK_CONV5_SCALE]; a.sh2 = p[MI355_SK_CONV5_SHIFT];
    a.u1 = u1; a.u2 = u2; a.pooled = pooled;
    a.Cin = Cin; a.planes = planes; a.groups = groups; a.cog = pl.cog; a.cin_g = pl.cin_g; a.H = H; a.W = W;
    a.cogp = pl.cogp; a.nct = pl.nct; a.BR = pl.BR; a.WCT = pl.WCT; a.nrb = pl.nrb; a.ncb = pl.ncb;
    a.CK = pl.CK; a.CP = pl.CP; a.chunks = pl.chunks; a.KC = pl.KC; a.ocp_total = (long)groups * pl.cogp;
    {
        MI355_TRACE(st, "sk_wide_kernel<nt=%d> cog=%d cin=%d bands=%d chunks=%d H=%d W=%d", pl.NT, pl.cog, pl.cin_g, pl.nb, pl.chunks, H, W);
        if (pl.NT == 1) sk_wide_kernel<1><<<(int)blocks, 256, pl.lds, st>>>(a);
        else            sk_wide_kernel<2><<<(int)blocks, 256, pl.lds, st>>>(a);
    }
    *pooled_out = pooled;
    *nb_out = pl.nb;
    return MI355_OK;
}

}  // namespace mi355
