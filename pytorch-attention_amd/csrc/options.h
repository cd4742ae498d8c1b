// options.h -- THE list of tuning options: one MI355_OPT(identifier, key, default, low, high) line per option, each followed by its
// explanation.  No include guard on purpose: the includer defines MI355_OPT and includes this file once per thing it generates --
// common.h the enum Opt { O_<identifier>, ..., O_COUNT }, api.hip the OptDesc kOpts[O_COUNT] table -- so the two cannot drift apart.
// [low, high] is the range mi355_set_option accepts.  spin_limit additionally accepts 0 (forces the time-out path in tests: every
// exchange then fails on its first unsuccessful poll; real budgets start at 1024 sweeps)
MI355_OPT(CHUNK_IMAGES, "chunk_images", 0, 0, 1L << 40)    // 0 = auto (about 200 MB of x per chunk)
MI355_OPT(NT, "nt", 3, 0, 3)                               // bit0: non-temporal loads, bit1: non-temporal stores in the final pass
MI355_OPT(REVERSE, "reverse", 0, 0, 1)
MI355_OPT(GEMM_VARIANT, "gemm_variant", 0, 0, 17)          // tile/schedule variant of the 16-bit GEMM (gemm16.hip); 0 = dispatch by shape
MI355_OPT(ECA_SINGLE, "eca_single", 1, 0, 1)               // ECA: one read + one write of x, halo channel rows re-summed per workgroup (chan_fused.hip)
MI355_OPT(SE_SINGLE, "se_single", 1, 0, 1)                 // SE: x read once, channel means exchanged as 8-byte {mean, tag} granules (chan_fused.hip)
MI355_OPT(CBAM_SINGLE, "cbam_single", 1, 0, 1)             // CBAM: x read once, row bands in registers, granule hops per band (cbam_single.hip)
MI355_OPT(WS_PERSISTENT, "ws_persistent", 0, 0, 1)         // 1 = caller keeps workspace contents between calls: granule exchanges skip their zeroing
MI355_OPT(STEM_DIRECT, "stem_direct", 1, 0, 1)             // narrow conv stems: direct fp32 kernel (stem_conv.hip) vs implicit GEMM
MI355_OPT(ZOO_SINGLE, "zoo_single", 1, 0, 1)               // SimAM / SRM / GCT / LCT: single-read register-resident path (chan_stat.hip) vs two passes
MI355_OPT(SPIN_LIMIT, "spin_limit", 1L << 22, 1024, 1L << 30)   // poll budget of the exchange kernels (sweeps) before they give up with an error code
MI355_OPT(GEMM_PA, "gemm_pa", 1, 0, 1)                     // fp32-output GEMMs: two-accumulator persistent kernel where it applies (gemm16_pa.hip)
MI355_OPT(GEMM_SPLITK, "gemm_splitk", 1, 0, 1)             // persistent GEMM: cut the tiles of the last partial round along K (gemm16_p8.hip)
MI355_OPT(DA_FUSED, "da_fused", 1, 0, 1)                   // DoubleAttention: fused kernels where they apply (double_attn_fused.hip, double_attn_small.hip)
MI355_OPT(DA_RANGES, "da_ranges", 0, 0, 32)                // ... pixel ranges per image in pass 1: 0 = from the batch size, 1..32 = fixed
MI355_OPT(SE_OCC, "se_occ", 3, 2, 3)                       // single-read SE: workgroups per CU (2: <= 128 VGPRs, 3: <= 80 VGPRs)
MI355_OPT(LN_FOLD, "ln_fold", 0, 0, 1)                     // ViT encoder chain: 1 = LayerNorm folded into the neighbouring GEMMs (ln_fold.hip); measured slower
                                                           // than the LayerNorm launches it removes, so it is opt-in
MI355_OPT(GEMM_PA16, "gemm_pa16", 1, 0, 2)                 // 16-bit outputs with K >= 576 on the two-accumulator kernel: 0 never, 1 GELU epilogues, 2 all
MI355_OPT(GEMM_PA_BLOCK, "gemm_pa_block", 1, 0, 1)         // two-accumulator kernel: blocked tile order (8 row x 4 column tiles per XCD round) for wide outputs
MI355_OPT(GEMM_PA_TAIL, "gemm_pa_tail", 10, 0, 100)        // two-accumulator kernel, K >= 1024: a last round at most this many percent full goes to the small-tile ring kernel (0 = off)
MI355_OPT(LPI_PATCH, "lpi_patch", 1, 0, 1)                 // LPI at 14 x 14 tokens, C % 32 == 0: 2 x 2 patches per lane on channel-quad-major LDS planes (xcit.hip)
MI355_OPT(MIXER_FUSED, "mixer_fused", 1, 0, 1)             // MixerLayer token mixing (host mirror): one kernel where the geometry allows (mixer_fused.hip)
MI355_OPT(MIXER_EARLY, "mixer_early", 0, 0, 1)             // mixer_token_kernel: all residual loads of the epilogue before its first store (A/B switch)
MI355_OPT(GEMM_SMALL, "gemm_small", 1, 0, 1)               // mi355_linear_fwd: outputs under an eighth of a round of 128 x 128 tiles on one-wave 16 x 32 tiles (gemm_small.hip)
MI355_OPT(MLP_TT4, "mlp_tt4", 0, 0, 1)                     // fused MLP at C = 64 (CSWin stage 1): 8 waves x 4 token tiles at 256 VGPRs instead of 16 x 2 at 128 (A/B switch)
MI355_OPT(MIXER_STATS, "mixer_stats", 0, 0, 1)             // mixer_token_kernel at C = 512: LayerNorm row statistics inside the kernel (1) or by the row_stats_kernel pre-pass (0, default: measured equal)
MI355_OPT(ATTN_NW, "attn_nw", 8, 7, 8)                     // ViT attention core at 193 .. 208 tokens (13 query tiles): waves per workgroup, 8 (13 / 16 balance) or 7 (13 / 14)
MI355_OPT(GEMM_W4, "gemm_w4", 1, 0, 1)                     // 16-bit outputs, 576 <= K < 1536, whole 256 x 256 tiles: the one-wave-per-SIMD persistent kernel (gemm16_w4.hip) instead of gemm16_p8
MI355_OPT(RANGE_FALLBACK, "range_fallback", 1, 0, 1)       // host policy of the drop-in modules (read by the binding): 1 = a forward whose fp16 operands saturated is re-run in strict mode, 0 = raise on the next call
MI355_OPT(GEMM_WREG, "gemm_wreg", 1, 0, 1)                 // fp32 (+ residual) outputs with N = K = 256 / 384: weight-stationary-in-registers streaming kernel (gemm16_wreg.hip)
MI355_OPT(XCA_TR, "xca_tr", 1, 0, 1)                       // XCA core with 16-bit q / k / v and N <= 224: covariance on the 16-bit matrix pipe from one transposed LDS image (xcit.hip xca_tr_kernel)
MI355_OPT(MLP_WIDE, "mlp_wide", 0, 0, 1)                   // 1 = mi355_mlp_fused_fwd takes C = 256 / 384 (hidden 4C) on the weight-split kernel (mlp_wide.hip); measured SLOWER than LayerNorm + two GEMMs
                                                           // (profiles/r06_mlp_wide.md), hence opt-in; 0 (default) = those shapes are MI355_EUNSUPPORTED
MI355_OPT(GEMM_WST, "gemm_wst", 5, 0, 6)                   // 16-bit outputs with K = 768 (ViT qkv / fc1): weights stationary in registers (gemm16_wst.hip).  0 = never.  Forced, whatever the row
                                                           // count: 1 = products without activation, 2 = GELU epilogues too, on the 8-wave K-split kernel (N % 192 == 0; measured slower,
                                                           // profiles/r06_gemm_wst.md); 3 / 4 = the same on the software-pipelined one-wave-per-SIMD kernel with W in AGPRs (N % 256 == 0,
                                                           // M % 32 == 0).  Default route to that kernel from the dispatch's row floor up: 5 (default) = GELU epilogues (ViT fc1), where it
                                                           // measured faster; 6 = every such product (qkv, the k / v product of the pooled-token tail too: a tie, profiles/gemm_wst_pipe.md).
                                                           // ONE value, so the modes exclude each other: forcing a kernel (1 .. 4) also turns the default route (5 / 6) off for the
                                                           // products the forced kernel does not take
MI355_OPT(GEMM_WSLAB, "gemm_wslab", 1, 0, 2)               // 16-bit outputs with K = 256 / 384 / 512 (XCiT / CSWin stage 3-4 / Mixer qkv and fc1): a column slab of W stationary in
                                                           // registers (gemm16_wslab.hip); 1 = GELU epilogues and M % 256 != 0 (where it measured faster), 2 = every product it takes
MI355_OPT(IO16_OCC, "io16_occ", 4, 2, 4)                   // single-read SE on 16-bit activations (chan_io16.hip): workgroups per CU the grid is sized for, capped by the kernel's register budget
MI355_OPT(VIT_TAIL, "vit_tail", 1, 0, 1)                   // host policy (read by the binding): 1 = a ViT that pools token 0 runs its LAST encoder block through mi355_vit_tail_fwd
                                                           // (only the rows that token needs: vit_tail.hip); 0 = the full block
MI355_OPT(SK_WIDE, "sk_wide", 0, 0, 1)                     // SKLayer branches: 1 = every shape on the matrix-core grouped implicit GEMM (sk_wide.hip); 0 (default) = only where
                                                           // the fp32 FMA kernels do not apply (planes / groups outside {1, 2, 4, 8, 16})
