// vit_tail.hip -- the LAST encoder block of a ViT that pools token 0 (ViT.py:180-192: head(x[:, 0])) as ONE C call that computes only what
// that token needs.  Of TransformerEncoder.forward (ViT.py:116-119) the result reads row 0 of every image; inside the block
//   * LayerNorm 1 and the k / v columns of the qkv projection are needed for every token (token 0 attends to all of them),
//   * the q columns, softmax . V, proj, LayerNorm 2, fc1, GELU, fc2, GELU and both residual adds for ONE row per image.
// Nothing new in arithmetic: the entry composes the library's own kernels on the caller's stream -- layernorm16, the 16-bit GEMM engine on
// the k / v rows of the qkv weight (written into columns C .. 3C of a (B, N, 3C) buffer, so the core's [q | k | v] addressing stays), the
// K/V-resident core limited to the first query row (attn.hip, QLIM), and the B-row products on the engine's 32 x 64 ring tiles with row
// strides instead of gather copies.  Every kernel involved is row-independent and keeps the engine's K order, so the (B, C) result equals
// row 0 of the full block bit for bit.  No host state, no exchange between workgroups, no memset: records under hipGraph stream capture.
#include "gemm16.h"

using g16::G16Args;

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

namespace {
struct TailWs {
    size_t u16, qkv16, ctx16, t32, x1, v16, h16, lin, lin_bytes, total;
};
TailWs tail_ws(int B, int N, int C, int hidden) {
    const size_t M = (size_t)B * N;
    TailWs w{};
    size_t o = 0;
    w.u16 = o;   o += up256(M * C * 2);                  // LayerNorm 1 of every token, operand format
    w.qkv16 = o; o += up256(M * 3 * C * 2);              // [q | k | v]: k / v of every token, q of token 0
    w.ctx16 = o; o += up256((size_t)B * C * 2);          // context of token 0
    w.t32 = o;   o += up256((size_t)B * C * 4);          // proj(context) + bias
    w.x1 = o;    o += up256((size_t)B * C * 4);          // x[:, 0] + proj: the residual stream of the MLP half
    w.v16 = o;   o += up256((size_t)B * C * 2);          // LayerNorm 2
    w.h16 = o;   o += up256((size_t)B * hidden * 2);     // gelu(fc1)
    w.lin = o;
    w.lin_bytes = mi355_linear16_workspace_bytes((int)M, 2 * C, C);
    o += up256(w.lin_bytes);
    w.total = o + 256;
    return w;
}

// one B-row product on the 32 x 64 ring tiles; the fp16 range word for 16-bit outputs as in mi355_linear16_ws_fwd
int rows_gemm(const void* X16, int ldx, const void* W16, const float* bias, const float* resid, void* Y, int ldy, int M, int N, int K, int act,
              int out16, int precision, hipStream_t st) {
    G16Args g{};
    g.A = X16; g.B = W16; g.C = Y; g.bias = bias; g.resid = resid;
    g.M = M; g.N = N; g.K = K; g.lda = ldx; g.ldb = K; g.ldc = ldy; g.act = act;
    if (out16 && precision == MI355_PREC_FP16) g.ovf = mi355::range_word(st);
    return mi355::gemm16_rows(g, out16, precision, st);
}
}  // namespace

extern "C" {

size_t mi355_vit_tail_workspace_bytes(int B, int N, int C, int hidden) {
    if (B <= 0 || N <= 0 || C <= 0 || hidden <= 0) return 0;
    return tail_ws(B, N, C, hidden).total;
}

int mi355_vit_tail_fwd(const float* x, const float* ln1_w, const float* ln1_b, float eps1, const void* Wqkv16, const float* b_qkv,
                       const void* Wproj16, const float* b_proj, const float* ln2_w, const float* ln2_b, float eps2, const void* Wfc1_16,
                       const float* b_fc1, const void* Wfc2_16, const float* b_fc2, float* y, int B, int N, int C, int hidden, int heads,
                       float scale, int precision, void* workspace, size_t workspace_bytes, mi355_stream_t stream) {
    MI355_CHECK_ARG(x && ln1_w && ln1_b && Wqkv16 && Wproj16 && ln2_w && ln2_b && Wfc1_16 && Wfc2_16 && y && workspace);
    MI355_CHECK_ARG(B > 0 && N > 0 && C > 0 && hidden > 0 && heads > 0);
    if (!(precision == MI355_PREC_FP16 || precision == MI355_PREC_BF16))
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_vit_tail_fwd: precision 1 (fp16) or 2 (bf16) (got %d)", precision);
    if ((C % heads) || (C % 64) || (hidden % 64) || C > 2048)
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_vit_tail_fwd: C %% heads == 0, C %% 64 == 0, C <= 2048, hidden %% 64 == 0 (C=%d heads=%d hidden=%d)",
                           C, heads, hidden);
    const int d = C / heads;
    if (!(d == 32 || d == 64)) return mi355::fail(MI355_EUNSUPPORTED, "mi355_vit_tail_fwd: head_dim %d (built: 32, 64)", d);
    if (N > 224) return mi355::fail(MI355_EUNSUPPORTED, "mi355_vit_tail_fwd: %d tokens > 224 (K/V-resident core)", N);
    const size_t M = (size_t)B * N;
    if (M > (size_t)0x7fffffff || (size_t)N * 3 * C > (size_t)0x7fffffff)
        return mi355::fail(MI355_EUNSUPPORTED, "mi355_vit_tail_fwd: B * N or N * 3C too large");
    const TailWs ws = tail_ws(B, N, C, hidden);
    MI355_CHECK_ARG(workspace_bytes >= ws.total && aligned16(workspace));
    MI355_CHECK_ARG(aligned16(x) && aligned16(y) && aligned16(Wqkv16) && aligned16(Wproj16) && aligned16(Wfc1_16) && aligned16(Wfc2_16));
    MI355_CHECK_ARG(aligned16(ln1_w) && aligned16(ln1_b) && aligned16(ln2_w) && aligned16(ln2_b));
    MI355_CHECK_ARG((!b_qkv || aligned16(b_qkv)) && (!b_proj || aligned16(b_proj)) && (!b_fc1 || aligned16(b_fc1)) && (!b_fc2 || aligned16(b_fc2)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(workspace);
    void* u16 = w + ws.u16;
    char* qkv16 = w + ws.qkv16;
    void* ctx16 = w + ws.ctx16;
    float* t32 = reinterpret_cast<float*>(w + ws.t32);
    float* x1 = reinterpret_cast<float*>(w + ws.x1);
    void* v16 = w + ws.v16;
    void* h16 = w + ws.h16;
    const char* Wq = static_cast<const char*>(Wqkv16);

    // LayerNorm 1 of every token
    if (int rc = mi355_layernorm16_fwd(x, ln1_w, ln1_b, u16, (int)M, C, eps1, precision, stream)) return rc;
    // k / v of every token: rows C .. 3C of the qkv weight are one contiguous (2C, C) slice; columns C .. 3C of the (B, N, 3C) buffer
    if (int rc = mi355_linear16_ws_fwd(u16, Wq + (size_t)C * C * 2, b_qkv ? b_qkv + C : nullptr, nullptr, nullptr, qkv16 + (size_t)C * 2, (int)M,
                                       2 * C, C, C, 3 * C, MI355_ACT_NONE, 1, precision, ws.lin_bytes ? w + ws.lin : nullptr, ws.lin_bytes, stream))
        return rc;
    // q of token 0 of every image: B rows, N * C apart in the LayerNorm output, N * 3C apart in the buffer
    if (int rc = rows_gemm(u16, N * C, Wq, b_qkv, nullptr, qkv16, N * 3 * C, B, C, C, MI355_ACT_NONE, 1, precision, st)) return rc;
    // softmax(q0 K^T scale) V: one query row per (image, head), context written densely as (B, 1, C)
    if (int rc = mi355_sdpa16_rows_fwd(qkv16, ctx16, B, N, heads, d, scale, 1, 1, precision, stream)) return rc;
    // proj + bias (the residual add rides in the LayerNorm kernel, which reads row 0 of x where it lies)
    if (int rc = rows_gemm(ctx16, C, Wproj16, b_proj, nullptr, t32, C, B, C, C, MI355_ACT_NONE, 0, precision, st)) return rc;
    // x1 = x[:, 0] + proj;  LayerNorm 2 of x1 in the operand format
    if (int rc = mi355::layernorm16_rows(x, (long)N * C, t32, x1, ln2_w, ln2_b, v16, B, C, eps2, precision, st))
        return rc == MI355_EUNSUPPORTED ? mi355::fail(rc, "mi355_vit_tail_fwd: LayerNorm 2 rows need C %% 4 == 0 and 16-byte aligned rows") : rc;
    // gelu(fc1), then y = x1 + gelu(fc2) (ViT.py:58-65: GELU behind both layers)
    if (int rc = rows_gemm(v16, C, Wfc1_16, b_fc1, nullptr, h16, hidden, B, hidden, C, MI355_ACT_GELU, 1, precision, st)) return rc;
    return rows_gemm(h16, hidden, Wfc2_16, b_fc2, x1, y, C, B, C, hidden, MI355_ACT_GELU, 0, precision, st);
}

}  // extern "C"
