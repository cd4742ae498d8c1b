// gemm16_res_body.h -- the kernel of gemm16_res.hip, written once and included TWICE by that file (no include guard):
//   RES_SCALE = 0   gemm16_res_kernel<T, R16, O16, BN, WN>:        Y = round_out( widen(resid) + act(X16 . W16^T + bias) )
//   RES_SCALE = 1   gemm16_res_scale_kernel<T, R16, O16, BN, WN>:  Y = round_out( widen(resid) + gamma * act(X16 . W16^T + bias) )
// The LayerScale form multiplies between the activation and the residual -- bias, act, * gamma, + widen(resid), one rounding: the epilogue
// order of gemm16_kernel -- for the XCiT blocks whose gamma * W cannot be folded into fp16 weights (eta = 1e-5: the products are fp16
// subnormals).  A textual include rather than one more template parameter: the instantiations without a scale keep their names and
// their machine code.  The kernel is described in gemm16_res.hip.

// (launch bounds: <= 128 registers for either tile -- four waves per SIMD, i.e. two 512-thread or four 256-thread workgroups per CU)
template <typename T, bool R16, bool O16, int BN, int WN>
#if RES_SCALE
// (four waves per SIMD asked for outright: at two, the 256-wide tile was given 131 registers and lost its second workgroup per CU)
__global__ __launch_bounds__(2 * WN * 64, 4) void gemm16_res_scale_kernel(const ResArgs g) {
#else
__global__ __launch_bounds__(2 * WN * 64, WN == 2 ? 4 : 2) void gemm16_res_kernel(const ResArgs g) {
#endif
    using v8 = typename Vec8<T>::t;
    using v4 = typename Vec8<T>::t4;
    constexpr int BM = 128, WM = 2, NW = WM * WN;
    constexpr int TM = BM / WM, TN = BN / WN, MF = TM / 16, NF = TN / 16;
    constexpr int IA = BM / 8 / NW, IB = BN / 8 / NW;           // LDS-DMA instructions per wave per K-tile (8 rows of 128 B each)
    static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0 && TM == 64 && TN == 64, "tile/wave geometry");
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[(BM + BN) * BK * 2];
    T* lds = reinterpret_cast<T*>(lds_raw);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = wave / WN, wc = wave % WN;
    const int tiles_n = (g.N + BN - 1) / BN;
    const int wg = xcd_contiguous_block();                     // neighbouring tiles (one row of W tiles, then the next) share an L2
    const int m0 = (wg / tiles_n) * BM, n0 = (wg % tiles_n) * BN;
    const T* __restrict__ A = static_cast<const T*>(g.A);
    const T* __restrict__ B = static_cast<const T*>(g.B);

    // LDS-DMA sources: lane -> (row = lane >> 3, physical 16-byte chunk = lane & 7) holds logical chunk (lane & 7) ^ (row & 7)
    const int lrow = lane >> 3, pch = lane & 7;
    const int csw = (pch ^ lrow) * 8;
    const T* a_src[IA];
    const T* b_src[IB];
#pragma unroll
    for (int i = 0; i < IA; ++i) {
        int ma = m0 + (wave * IA + i) * 8 + lrow; if (ma >= g.M) ma = g.M - 1;   // clamp: tail rows are computed and discarded
        a_src[i] = A + (long)ma * g.lda + csw;
    }
#pragma unroll
    for (int i = 0; i < IB; ++i) {
        int nb = n0 + (wave * IB + i) * 8 + lrow; if (nb >= g.N) nb = g.N - 1;
        b_src[i] = B + (long)nb * g.K + csw;
    }
    T* sAw = lds + (wave * IA * 8) * BK;
    T* sBw = lds + BM * BK + (wave * IB * 8) * BK;

    f4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4, fsw = lane & 7;
    const T* sA = lds + (wr * TM + frow) * BK;
    const T* sB = lds + BM * BK + (wc * TN + frow) * BK;
    const int nk = g.K / BK;
    for (int kt = 0; kt < nk; ++kt) {
        const int k0 = kt * BK;
#pragma unroll
        for (int i = 0; i < IA; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[i] + k0),
                                             (__attribute__((address_space(3))) void*)(sAw + i * 8 * BK), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < IB; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_src[i] + k0),
                                             (__attribute__((address_space(3))) void*)(sBw + i * 8 * BK), 16, 0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int off = (((ks * 4 + fq) ^ fsw) * 8);
            v8 fa[MF], fb[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) fb[j] = *reinterpret_cast<const v8*>(sB + j * 16 * BK + off);
#pragma unroll
            for (int i = 0; i < MF; ++i) fa[i] = *reinterpret_cast<const v8*>(sA + i * 16 * BK + off);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j) acc[i][j] = mma16<T>(fb[j], fa[i], acc[i][j]);      // D^T = W . X^T: see the epilogue
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
    }

    // ---- epilogue straight from the accumulators: the MFMAs compute the TRANSPOSED 16 x 16 tiles, so lane (l15, g) holds output row
    //      m = i*16 + l15 and four CONSECUTIVE columns n = j*16 + g*4 + [0, 4) -- the pack of the residual row it needs and of the
    //      output row it writes.  All residual packs of a row tile are requested before the first is used.
    const int l15 = lane & 15, g4 = (lane >> 4) * 4;
    const float* Rf = static_cast<const float*>(g.resid);
    const T* Rh = static_cast<const T*>(g.resid);
    float* Cf = static_cast<float*>(g.C);
    T* Ch = static_cast<T*>(g.C);
    float rgmax = 0.f;
    f4 bias4[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int n = n0 + wc * TN + j * 16 + g4;
        bias4[j] = (g.bias && n < g.N) ? *reinterpret_cast<const f4*>(g.bias + n) : f4{0.f, 0.f, 0.f, 0.f};
    }
#if RES_SCALE
    // gamma, once per column pack like the bias, in the bias' registers: both vectors live next to 64 accumulators, 16 residual registers
    // and the temporaries of the GELU would not fit the 128 registers of the launch bounds.  So the bias goes into the accumulators first
    // -- the sum acc + bias of the loop below, formed earlier -- and each sum is pinned by an empty asm, or the compiler sinks the
    // additions back to their uses and keeps the bias alive.
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            acc[i][j] = acc[i][j] + bias4[j];
            asm volatile("" : "+v"(acc[i][j]));
        }
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int n = n0 + wc * TN + j * 16 + g4;
        bias4[j] = n < g.N ? *reinterpret_cast<const f4*>(g.gamma + n) : f4{1.f, 1.f, 1.f, 1.f};
    }
#endif
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        const int m = m0 + wr * TM + i * 16 + l15;
        if (m >= g.M) continue;
        const long ro = (long)m * g.ldc;
        f4 r[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const int n = n0 + wc * TN + j * 16 + g4;
            if (n >= g.N) { r[j] = f4{0.f, 0.f, 0.f, 0.f}; continue; }           // N % 8 == 0: a pack of four is in or out
            if constexpr (R16) {
                const v4 h = *reinterpret_cast<const v4*>(Rh + ro + n);
                r[j] = f4{(float)h.x, (float)h.y, (float)h.z, (float)h.w};
            } else {
                r[j] = *reinterpret_cast<const f4*>(Rf + ro + n);
            }
        }
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const int n = n0 + wc * TN + j * 16 + g4;
            if (n >= g.N) continue;
#if RES_SCALE
            f4 v = acc[i][j];                                   // acc + bias (above); bias4 holds gamma
#else
            f4 v = acc[i][j] + bias4[j];
#endif
            if (g.act == MI355_ACT_GELU) v = gelu_fast4(v);     // the fp32 form also in front of a 16-bit store: the sum is what is rounded
#if RES_SCALE
            v = v * bias4[j];
#endif
            v = v + r[j];
            if constexpr (O16) {
                if constexpr (std::is_same<T, _Float16>::value) rgmax = rg_absmax4(rgmax, v);
                *reinterpret_cast<v4*>(Ch + ro + n) = v4{(T)v.x, (T)v.y, (T)v.z, (T)v.w};
            } else {
                *reinterpret_cast<f4*>(Cf + ro + n) = v;
            }
        }
    }
    if constexpr (O16 && std::is_same<T, _Float16>::value) rg_report(rgmax, g.ovf, 3u);
}
