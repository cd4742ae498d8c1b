"""Drop-in ViT modules (reference: vision_transformers/ViT.py), forward composed from libmi355attn ops.

  Attention           ViT.py:67-89      qkv GEMM -> fused QK^T-softmax-PV core -> proj GEMM(+bias)
  Mlp                 ViT.py:47-65      GELU after fc1 AND after fc2 (reference behaviour, kept)
  TransformerEncoder  ViT.py:107-119    pre-LN block, residual adds fused into the GEMM epilogues
  PatchEmbedding      ViT.py:91-105     per-patch GEMM, im2col folded into the A-operand load
  VisionTransformer   ViT.py:121-192    cls token appended LAST, logits from token 0, no final LayerNorm

Sub-modules hold parameters only (same creation order as the reference => same init stream under a seed).
``precision`` (None = package default) selects the MFMA operand format for every GEMM of the module.

Precision 3 ("logit-compensated", F.PREC_LOGIT) is precision 1 with the logit path of `Attention` -- the q / k columns of the qkv
projection, the stored q and k, Q K^T -- in the strict operand format (bf16 hi + lo, three MFMAs): the 16-bit error of the block that
grows with the logit size is made there, the value path is scale-free (profiles/logit_mode.md).  Pick it for weights whose pre-softmax
logits have a standard deviation above ~1, i.e. anything trained.  Everything outside `Attention` runs exactly as in precision 1.

`TransformerEncoder`, `PatchEmbedding` and `VisionTransformer` also take an fp16 / bf16 tensor and return that type (the operand format
is then the tensor's type; see TransformerEncoder._forward16).  `Attention` and `Mlp` on their own keep their internal convention on a
16-bit x: an operand in, an fp32 result out.
"""
import torch
from torch import nn

from .. import functional as F
from ._io16 import _fast, _half16, _io_precision, _is16, _layernorm, _lin, _mlp_run, _p32, _patch_embed16, _same


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, drop=0):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
        self.precision = None
        self.drop = drop                     # inference engine: dropout is the identity (eval semantics)

    def forward(self, x, resid=None):
        return self._run(x, resid, self.precision, _same)

    def _run(self, x, resid, precision, P):
        """The forward at `precision` (the setting; None = the default) with the parameters as P hands them over: _same from forward(),
        _p32 behind a widened 16-bit x (TransformerEncoder._forward16)."""
        return _mlp_run(self.fc1, self.fc2, x, resid, precision, P, second_gelu=True)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=4, qkv_bias=False, attn_drop=0, proj_drop=0, precision=None):
        super().__init__()
        assert dim % num_heads == 0
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.precision = precision
        self.attn_drop, self.proj_drop = attn_drop, proj_drop   # identity at inference

    def fast_ok(self, n_tokens=None):
        """16-bit dataflow applies: 16-bit operand mode, GEMM shapes in the fast envelope, a core kernel built for the head width
        (the K/V-resident kernel for d in {32, 64} and N <= 224, the streaming kernel for any N and d in F.SDPA_WIDTHS)."""
        d = self.qkv.in_features // self.num_heads
        return _fast(self.precision, self.qkv, self.proj) and d in F.SDPA_WIDTHS

    def _core(self, qkv, fast, precision=None):
        """softmax(q k^T scale) v on the (B,N,3C) projection.  Short sequences of 32 / 64 wide heads stay in LDS (attn.hip); longer
        sequences (384 px input: N = 577) and wider heads (ViT.py:68 defaults to 4 heads: d = 192 at dim 768) stream K / V
        (sdpa_general.hip); any other width runs zero padded to the next built one.  `precision`: the operand format where it is not
        the module's setting (a block on 16-bit activations: the type of its x)."""
        p = self.precision if precision is None else precision
        B, N, C3 = qkv.shape
        C = C3 // 3
        d = C // self.num_heads
        if d in (32, 64) and N <= 224:
            return F.sdpa16(qkv, self.num_heads, self.scale, precision=p) if fast else \
                F.sdpa(qkv, self.num_heads, self.scale, precision=p)
        return F.sdpa_general(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], self.num_heads, self.scale, precision=p)

    def _forward_logit(self, x, resid):
        """Precision 3: one projection launch that computes the q / k columns on bf16 hi / lo pairs and the v columns in fp16
        (F.qkv_split16), the core with Q K^T on the pairs and P V in fp16 (F.sdpa16_split), then precision 1's fp16 proj GEMM with the
        residual fused.  Outside those kernels' envelope (head width not 32 / 64, more than 224 tokens, in_features % 64 != 0) the block
        runs its precision-0 path instead -- slower, never less accurate than asked."""
        C = self.qkv.in_features
        if not F.logit_envelope(C, C, self.num_heads, x.shape[-2]):
            with F._forced_strict(self):
                return self.forward(x, resid)
        x = x if x.dtype == torch.float32 else x.float()
        qkv5 = F.qkv_split16(x, *F.weight_split16(self.qkv.weight), self.qkv.bias)                    # (B,N,5C)
        ctx = F.sdpa16_split(qkv5, self.num_heads, self.scale)                                           # (B,N,C) fp16
        return F.linear16(ctx, F.weight16(self.proj.weight, F.PREC_FP16), self.proj.bias, resid=resid, precision=F.PREC_FP16)

    def forward(self, x, resid=None):
        if F.logit_mode(self.precision):
            return self._forward_logit(x, resid)
        return self._run(x, resid, self.precision, _same)

    def _run(self, x, resid, precision, P):
        """The forward outside precision 3 at `precision` (the setting; None = the default) with the parameters as P hands them over:
        _same from forward(), _p32 behind a widened 16-bit x (TransformerEncoder._forward16)."""
        qkv_, proj = _lin(self.qkv, P, "qkv"), _lin(self.proj, P, "proj")
        d = self.qkv.in_features // self.num_heads
        if d not in F.SDPA_WIDTHS:                                                           # odd head width: padded projections
            from .mhsa import _fused_qkv_attention
            out, _, _ = _fused_qkv_attention(x if x.dtype == torch.float32 else x.float(), qkv_, proj, self.num_heads, d,
                                             self.scale, precision)
            return out if resid is None else F.axpby(out, torch.empty_like(out), out.numel() // out.shape[-1], out.shape[-1],
                                                     out.shape[-1], out.shape[-1], u=resid, ldu=out.shape[-1])
        if _fast(precision, self.qkv, self.proj):
            # q / k / v / ctx stay 16-bit in HBM; the whole block is ONE C call (mi355_mhsa_fwd: cast -> qkv GEMM -> core -> proj GEMM,
            # the same kernels the three-call composition of rounds 1-2 launched)
            p = F._prec(precision)
            return F.mhsa16(x, F.weight16(qkv_.weight, p), qkv_.bias, F.weight16(proj.weight, p), proj.bias,
                            self.num_heads, self.scale, resid=resid, precision=p)
        qkv = F.linear(x, qkv_.weight, qkv_.bias, precision=precision)                   # (B,N,3C)
        ctx = self._core(qkv, False, precision)                                             # (B,N,C)
        return F.linear(ctx, proj.weight, proj.bias, resid=resid, precision=precision)


class PatchEmbedding(nn.Module):
    def __init__(self, image_size=224, patch_size=16, in_channels=3, embedding_dim=768):
        super().__init__()
        assert image_size % patch_size == 0
        self.patch_size = patch_size
        self.num_patches = (image_size // patch_size) ** 2
        self.proj = nn.Conv2d(in_channels, embedding_dim, kernel_size=patch_size, stride=patch_size)
        self.precision = None

    _mi355_fp16_io_saturates = True          # fp16 tokens beyond 65504 are reported by the GEMM epilogue

    def forward(self, x):
        """x (B, Cin, H, W) fp32 -> fp32 tokens, or fp16 / bf16 -> tokens of that type, as mixer.PatchEmbedding has it (_patch_embed16)."""
        if _is16(x):
            return _patch_embed16(self, x)
        return F.patch_embed(x, self.proj.weight, self.proj.bias, None, None, self.patch_size, self.precision)


class TransformerEncoder(nn.Module):
    def __init__(self, dim, num_heads=4, mlp_ratio=4, qkv_bias=False, attn_drop=0, proj_drop=0, precision=None):
        super().__init__()
        self.attn = Attention(dim, num_heads, qkv_bias, attn_drop, proj_drop, precision)
        self.layernorm1 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.mlp.precision = precision
        self.layernorm2 = nn.LayerNorm(dim)

    _mi355_fp16_io_saturates = True          # an fp16 x is guarded like an fp32 one: the fp16 LN operand and the 16-bit epilogues can saturate

    def forward(self, x):
        """x (B, N, C) fp32, or fp16 / bf16 (the result has the type of x; see _forward16)."""
        if _is16(x):
            return self._forward16(x)
        if self.fold_ok(x):
            return self.forward_folded(x)[0]
        return self._run(x, self.attn.precision, _same)

    def _forward16(self, x):
        """The block on an fp16 / bf16 x; the result has the type of x.  The MFMA operand format is that type (fp16: the precision-1
        arithmetic, bf16: precision 2) and a `precision` of None / 1 / 2 / 3 is ignored; precision 0 (explicit, the package default, or
        a strict re-run) widens x, runs the strict route and rounds.  On the fast route x enters the arithmetic unrounded -- LayerNorm 1
        reads it in 16 bit (layernorm_x16_kernel), proj adds it as a 16-bit residual -- the residual stream x1 behind the attention
        half stays fp32, and y = x1 + gelu(fc2(..)) is rounded once, in the epilogue of the last GEMM (gemm16_res_kernel; an fp16 y
        beyond 65504 is reported to the range guard, code 3, so the block re-runs strict and returns inf).  No widen, round or cast
        launch.  Outside that envelope (head widths off F.SDPA_WIDTHS, in_features % 64 != 0, precision 0) one launch widens x, the
        fp32 body (_run) runs at the precision of the type, and one launch rounds.  Neither the LayerNorm fold nor the pooled-token tail
        applies to a 16-bit tensor."""
        x, io = F._require_io16(x, "x")
        p = _io_precision(self.attn.precision, io)
        at, mlp, ln1 = self.attn, self.mlp, self.layernorm1
        if p and x.dim() == 3 and at.fast_ok(x.shape[1]) and _fast(p, at.qkv, at.proj, mlp.fc1, mlp.fc2):
            u = F.layernorm16_x16(x, ln1.weight, ln1.bias, ln1.eps)
            qkv = F.linear16(u, F.weight16(at.qkv.weight, p), _p32(at.qkv.bias, "qkv.bias"), out16=True, precision=p)
            ctx = at._core(qkv, True, p)
            x1 = F.linear16_res(ctx, F.weight16(at.proj.weight, p), at.proj.bias, x, precision=p)         # 16-bit residual, fp32 stream
            return _half16(self.layernorm2, "layernorm2", mlp.fc1, x1, p, lambda h: F.linear16_res(
                h, F.weight16(mlp.fc2.weight, p), mlp.fc2.bias, x1, act=F.ACT_GELU, out_dtype=x.dtype, precision=p))
        return F.round16(self._run(F.widen16(x), p, _p32), x.dtype)

    def _run(self, x, precision, P):
        """The fp32 block outside the LayerNorm fold: one LayerNorm launch in front of each half (the fold is opt-in: measured slower,
        DESIGN.md 6.2c).  forward() passes attn.precision and _same: attn and mlp are called as modules, each at its own setting.
        _forward16 passes the widened x, the precision of its type (or 0) and _p32: both run at that precision, whatever their setting."""
        at, mlp = self.attn, self.mlp
        own = P is _same
        fast1 = fast2 = _fast(precision, at.qkv, at.proj, mlp.fc1, mlp.fc2) and at.qkv.in_features // at.num_heads in F.SDPA_WIDTHS
        if own and F.logit_mode(precision):
            # precision 3 (an fp32 x only): the projection kernel splits fp32 rows itself, so LayerNorm 1 stays fp32 (a 16-bit LayerNorm
            # output would put the rounding the mode removes back in front of the q / k columns); the MLP half is precision 1's
            fast1, fast2 = False, _fast(precision, mlp.fc1, mlp.fc2)
        u = _layernorm(self.layernorm1, x, P, "layernorm1", fast1, precision)     # fast: LayerNorm writes the GEMM's operand format directly
        x = at(u, resid=x) if own else at._run(u, x, precision, P)
        u = _layernorm(self.layernorm2, x, P, "layernorm2", fast2, precision)
        return mlp(u, resid=x) if own else mlp._run(u, x, precision, P)

    # ---- LayerNorm folded into the GEMMs around it (csrc/ln_fold.hip): no LayerNorm launch between proj and fc1, nor between fc2 and
    #      the next block's qkv; the first LayerNorm of a chain is one mi355_ln_center16_fwd ---------------------------------------
    def fold_ok(self, x):
        """The folded path applies: 16-bit dataflow, K/V-resident attention core, the producer kernel's shape envelope
        (rows % 128 == 0: B = 128, 256, ... at 197 tokens) and LayerNorm gains that keep gamma * W inside fp16."""
        if not F.ln_fold_enabled() or x.dim() != 3 or x.dtype != torch.float32 or not x.is_cuda:   # the option first: off by default
            return False
        if F.logit_mode(self.attn.precision):                   # the fold feeds the qkv GEMM 16-bit rows: not in precision 3
            return False
        B, N, C = x.shape
        p = F._prec(self.attn.precision)
        d = C // self.attn.num_heads
        if not (self.attn.fast_ok(N) and _fast(p, self.mlp.fc1, self.mlp.fc2) and d in (32, 64) and N <= 224):
            return False
        if not (F.ln_fold_ok(B * N, C, C, C, p) and F.ln_fold_ok(B * N, C, C, self.mlp.fc1.out_features, p)):
            return False
        return (F.lnfold_weights(self.layernorm1, self.attn.qkv, p) is not None and
                F.lnfold_weights(self.layernorm2, self.mlp.fc1, p) is not None)

    def forward_folded(self, x, state=None, next_eps=None):
        """x (B,N,C) fp32 -> (y, LnState of the NEXT block's LayerNorm 1 or None).  `state`: the LnState of THIS block's LayerNorm 1
        when the previous block emitted it (else computed here from x); `next_eps`: eps of the next block's LayerNorm 1 when fc2
        should emit for it."""
        p = F._prec(self.attn.precision)
        ln1, ln2, at, mlp = self.layernorm1, self.layernorm2, self.attn, self.mlp
        wq, sq, bq = F.lnfold_weights(ln1, at.qkv, p)
        w1, s1, b1 = F.lnfold_weights(ln2, mlp.fc1, p)
        if state is None:
            state = F.ln_center16(x, ln1.eps, p)
        qkv = F.linear16_lnfold(state, wq, bq, sq, precision=p)                                  # LayerNorm 1 + qkv (+ bias)
        ctx = F.sdpa16(qkv, at.num_heads, at.scale, precision=p)
        x1, st = F.linear16_emit(ctx, F.weight16(at.proj.weight, p), at.proj.bias, x, state.cvec, ln2.eps, precision=p)   # proj + residual, emits LN2
        h = F.linear16_lnfold(st, w1, b1, s1, act=F.ACT_GELU, precision=p)                     # LayerNorm 2 + fc1 + GELU
        w2 = F.weight16(mlp.fc2.weight, p)
        if next_eps is None:
            return F.linear16(h, w2, mlp.fc2.bias, act=F.ACT_GELU, resid=x1, precision=p), None
        return F.linear16_emit(h, w2, mlp.fc2.bias, x1, st.cvec, next_eps, act=F.ACT_GELU, precision=p)   # fc2 + GELU + residual, emits the next LN1


class VisionTransformer(nn.Module):
    def __init__(self, image_size=224, patch_size=16, in_channels=3, depths=12, num_heads=4, mlp_ratio=4,
                 embedding_dim=768, qkv_bias=False, attn_drop=0, proj_drop=0, global_pool="token",
                 num_classes=1000, precision=None):
        super().__init__()
        self.patch_embedding = PatchEmbedding(image_size, patch_size, in_channels, embedding_dim)
        self.patch_embedding.precision = precision
        self.global_pool = global_pool
        self.precision = precision
        n = self.patch_embedding.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embedding_dim))
        self.position_embedding = nn.Parameter(torch.zeros(1, n + 1, embedding_dim))
        self.blocks = nn.Sequential(*(TransformerEncoder(embedding_dim, num_heads, mlp_ratio, qkv_bias, attn_drop,
                                                         proj_drop, precision) for _ in range(depths)))
        self.head = nn.Linear(embedding_dim, num_classes)
        # same init stream as ViT.py:147-158: pos, cls, then every Linear (trunc-normal .02, zero bias) / LayerNorm
        nn.init.trunc_normal_(self.position_embedding, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        self.apply(self._reset)

    @staticmethod
    def _reset(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.LayerNorm):
            nn.init.zeros_(m.bias)
            nn.init.ones_(m.weight)

    def _tail_ok(self, blk, tok):
        """The last block may compute the pooled token's rows only (F.vit_tail16, csrc/vit_tail.hip): logits come from token 0, the
        option is on and the fold off, the block is the plain 16-bit dataflow inside the entry's envelope, and nobody can observe the
        block's full output -- a forward (pre-)hook on the block or on anything inside it keeps the full path."""
        if self.global_pool != "token" or F.ln_fold_enabled() or not F.vit_tail_enabled():
            return False
        if type(blk) is not TransformerEncoder or type(blk.attn) is not Attention or type(blk.mlp) is not Mlp:
            return False
        at, mlp = blk.attn, blk.mlp
        if F.logit_mode(at.precision) or tok.dim() != 3 or tok.dtype != torch.float32 or not tok.is_cuda:
            return False
        p = F._prec(at.precision)
        B, N, C = tok.shape
        if p not in (F.PREC_FP16, F.PREC_BF16) or F._prec(mlp.precision) != p or mlp.fc1.in_features != C or mlp.fc2.out_features != C:
            return False
        if not (at.fast_ok(N) and _fast(p, mlp.fc1, mlp.fc2) and F.vit_tail_envelope(C, mlp.fc1.out_features, at.num_heads, N)):
            return False
        if nn.modules.module._global_forward_hooks or nn.modules.module._global_forward_pre_hooks:
            return False
        return not any(m._forward_hooks or m._forward_pre_hooks for m in blk.modules())

    _mi355_fp16_io_saturates = True

    def _forward16(self, img):
        """The model on an fp16 / bf16 image: the composition of its parts on 16-bit tensors, logits in the type of the image.  The
        tokens are the fp32 tokens of the embedding (patches, cls token, position rows; operand format = the type) computed from the
        widened image and rounded once -- one widen and one round launch per forward, no torch cast over activations; every block is
        16-bit in, 16-bit out and runs in full (neither the LayerNorm fold nor the pooled-token tail takes a 16-bit tensor); the
        pooled row and the head are fp32, and the (B, classes) logits are the one torch cast."""
        img, io = F._require_io16(img, "img")
        p = _io_precision(self.precision, io)
        pe = self.patch_embedding
        pos = F.vit_pos_table(_p32(self.position_embedding, "position_embedding"), pe.patch_size, img.shape[2], img.shape[3])
        tok = F.patch_embed(F.widen16(img), _p32(pe.proj.weight, "proj.weight"), _p32(pe.proj.bias, "proj.bias"),
                            _p32(self.cls_token, "cls_token").reshape(-1), pos, pe.patch_size, p)
        tok = F.round16(tok, img.dtype)
        for blk in self.blocks:
            tok = blk(tok)
        if self.global_pool == "token":
            pooled = tok[:, 0].float()                           # (B, C): not a pass over the activations
        elif self.global_pool == "avg":
            pooled = F.token_mean16(tok, skip_first=1)
        else:
            pooled = F.widen16(tok)
        logits = F.linear(pooled, _p32(self.head.weight, "head.weight"), _p32(self.head.bias, "head.bias"), precision=p)
        return logits.to(img.dtype)

    def forward(self, x):
        if _is16(x):
            return self._forward16(x)
        B, _, H, W = x.shape
        ps = self.patch_embedding.patch_size
        pos = F.vit_pos_table(self.position_embedding, ps, H, W)     # ViT.py:160-178: bicubic resize off the native grid (cached)
        tok = F.patch_embed(x, self.patch_embedding.proj.weight, self.patch_embedding.proj.bias,
                            self.cls_token.reshape(-1), pos, ps, self.precision)
        blocks, state = list(self.blocks), None
        # fold eligibility is decided ONCE per forward (the token tensor keeps its shape through the blocks): with the option off -- the
        # default -- no per-block option reads / envelope checks / cache look-ups happen at all
        elig = [blk.fold_ok(tok) for blk in blocks] if F.ln_fold_enabled() else None
        tail = blocks.pop() if blocks and self._tail_ok(blocks[-1], tok) else None
        for i, blk in enumerate(blocks):
            if elig is not None and elig[i]:                      # LayerNorms folded into the GEMMs; the state travels block to block
                nxt_ok = i + 1 < len(blocks) and elig[i + 1]
                tok, state = blk.forward_folded(tok, state, blocks[i + 1].layernorm1.eps if nxt_ok else None)
            else:
                tok, state = blk(tok), None                       # module call (hooks intact); its own fold check is one option read
        if tail is not None:
            # nothing but row 0 of the last block's output is read below: LayerNorm 1 and k / v for every token, everything else for one
            # row per image, in one C call; the same kernels' arithmetic, bit-identical logits (option "vit_tail" = 0: the full block)
            at, mlp = tail.attn, tail.mlp
            p = F._prec(at.precision)
            pooled = F.vit_tail16(tok, tail.layernorm1, F.weight16(at.qkv.weight, p), at.qkv.bias, F.weight16(at.proj.weight, p),
                                  at.proj.bias, tail.layernorm2, F.weight16(mlp.fc1.weight, p), mlp.fc1.bias,
                                  F.weight16(mlp.fc2.weight, p), mlp.fc2.bias, at.num_heads, at.scale, precision=p)
        elif self.global_pool == "token":
            pooled = tok[:, 0]                                   # row-strided view, consumed in place by the GEMM
        elif self.global_pool == "avg":
            pooled = F.token_mean(tok, skip_first=1)
        else:
            pooled = tok                                         # ViT.py:187-190: any other value pools nothing, head on every token
        return F.linear(pooled, self.head.weight, self.head.bias, precision=self.precision)
