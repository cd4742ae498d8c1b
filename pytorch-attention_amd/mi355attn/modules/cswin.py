"""Drop-in CSWin modules (reference: vision_transformers/cswin.py), forward routed to libmi355attn.

  LePEAttention  cswin.py:51-127   stripe-window MHSA + locally-enhanced positional encoding (dw 3x3 on v)
  CSWinBlock     cswin.py:130-197  LN -> qkv -> two stripe branches on channel halves -> proj -> MLP

The window partition (img2windows / windows2img, cswin.py:199-216) never materialises: the attention
kernel gathers q/k/v straight from the (B,L,3,C) qkv buffer with window index math and scatters its
output back in (B,L,C) order.

`CSWinBlock`, `LePEAttention`, `Merge_Block`, `CSWinTransformer` and the two factories also take an fp16 / bf16 tensor and return that
type (the operand format is then the tensor's type; see CSWinBlock._forward16).
"""
import torch
from torch import nn

from .. import functional as F
from ._io16 import _fast, _half16, _io_precision, _is16, _layernorm, _mlp_run, _p32, _same


def _stripe(resolution, idx, split_size):
    if idx == -1:
        return resolution, resolution
    if idx == 0:
        return resolution, split_size
    if idx == 1:
        return split_size, resolution
    raise ValueError(f"LePEAttention: idx must be -1, 0 or 1, got {idx}")


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        if act_layer is not nn.GELU:
            raise NotImplementedError("only the exact-erf GELU epilogue is built")
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
        self.precision = None

    def forward(self, x, resid=None):
        return self._run(x, resid, self.precision, _same)

    def _run(self, x, resid, precision, P):
        return _mlp_run(self.fc1, self.fc2, x, resid, precision, P)


class LePEAttention(nn.Module):
    def __init__(self, dim, resolution, idx, split_size=7, dim_out=None, num_heads=8, attn_drop=0., proj_drop=0.,
                 qk_scale=None, precision=None):
        super().__init__()
        self.dim, self.dim_out = dim, dim_out or dim
        self.resolution, self.split_size, self.num_heads = resolution, split_size, num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.H_sp, self.W_sp = _stripe(resolution, idx, split_size)
        self.get_v = nn.Conv2d(dim, dim, kernel_size=3, stride=1, padding=1, groups=dim)
        self.precision = precision

    def run(self, qkv_blc, out, c0, precision=None, P=_same):
        """Attend over channels [c0, c0+dim) of a (B,L,3,Ctot) buffer, writing the same slice of `out` (B,L,Ctot).
        fp32 buffers use the converting kernel, 16-bit buffers the 16-bit-I/O kernel.  `precision`: the operand format where it is not
        the module's setting, P: how the parameters are handed over (_p32 for a block on 16-bit activations: the type of its x)."""
        fn = F.cswin_lepe_attention if qkv_blc.dtype == torch.float32 else F.cswin_lepe_attention16
        return fn(qkv_blc, P(self.get_v.weight, "get_v.weight"), P(self.get_v.bias, "get_v.bias"), out, self.resolution, c0, self.dim,
                  self.num_heads, self.H_sp, self.W_sp, self.scale, self.precision if precision is None else precision)

    _mi355_fp16_io_saturates = True          # an fp16 qkv is guarded like an fp32 one: the core's fp16 context can saturate

    def forward(self, qkv):
        """qkv: (3,B,L,C) as in the reference (cswin.py:101-105); returns (B,L,C).  fp32, or fp16 / bf16: the result then has the type
        of qkv, which is the operand format of the 16-bit core whatever `precision` says; precision 0 (or a strict re-run) widens,
        runs the strict core and rounds."""
        three, B, L, C = qkv.shape
        assert three == 3 and C == self.dim and L == self.resolution * self.resolution, "flatten img_tokens has wrong size"
        if _is16(qkv):
            qkv, io = F._require_io16(qkv, "qkv")
            p = _io_precision(self.precision, io)
            buf = qkv.permute(1, 2, 0, 3).contiguous().view(B, L, 3 * C)
            if p:
                return self.run(buf, torch.empty(B, L, C, dtype=qkv.dtype, device=qkv.device), 0, p, _p32)
            out = torch.empty(B, L, C, dtype=torch.float32, device=qkv.device)
            return F.round16(self.run(F.widen16(buf), out, 0, p, _p32), qkv.dtype)
        buf = qkv.permute(1, 2, 0, 3).contiguous().view(B, L, 3 * C)     # no copy when qkv is the usual permuted view
        out = torch.empty(B, L, C, dtype=torch.float32, device=qkv.device)
        return self.run(buf, out, 0)


class CSWinBlock(nn.Module):
    def __init__(self, dim, reso, num_heads, split_size=7, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0.,
                 attn_drop=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, last_stage=False, precision=None):
        super().__init__()
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError("only nn.LayerNorm is built")
        self.dim, self.num_heads, self.patches_resolution = dim, num_heads, reso
        self.split_size, self.mlp_ratio, self.precision = split_size, mlp_ratio, precision
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.norm1 = norm_layer(dim)
        last_stage = last_stage or reso == split_size                   # cswin.py:146-147
        self.branch_num = 1 if last_stage else 2
        self.proj = nn.Linear(dim, dim)
        if last_stage:
            branches = [LePEAttention(dim, reso, -1, split_size, dim, num_heads, attn_drop, drop, qk_scale, precision)]
        else:
            branches = [LePEAttention(dim // 2, reso, i, split_size, dim // 2, num_heads // 2, attn_drop, drop, qk_scale,
                                      precision) for i in range(2)]
        self.attns = nn.ModuleList(branches)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), dim, act_layer, drop)
        self.mlp.precision = precision
        self.norm2 = norm_layer(dim)

    _mi355_fp16_io_saturates = True          # an fp16 x is guarded like an fp32 one: fp16 operands and the 16-bit y store can saturate

    def _forward16(self, x):
        """The block on an fp16 / bf16 x; the result has the type of x.  The MFMA operand format is that type (fp16: the precision-1
        arithmetic, bf16: precision 2) and a `precision` of None / 1 / 2 / 3 is ignored; precision 0 (explicit, the package default, or
        a strict re-run) widens x, runs the strict route and rounds.  Parameters may be fp32 or 16-bit.  The residual stream inside the
        block stays fp32 and y is rounded once.
          A  narrow stages (F.cswin_stripe_ok): the stripe kernel reads x16 itself (cswin_stripe_kernel<.., x16>), the proj + MLP kernel
             reads x16 and writes y16 (mlp_fused_kernel<.., proj, x16>) -- two launches, no widen, round or cast of an activation.  With
             an MLP the fused kernel is not built for (mlp_ratio != 4): proj adds x16 as a 16-bit residual into the fp32 stream,
             LayerNorm, fc1, and fc2 rounds y in its epilogue (gemm16_res_kernel).
          B  head width 32 on the fast GEMMs, stripe kernel not applicable (C = 256 / 512, the one-branch last stage, stripes above 64
             tokens): LayerNorm 1 reads x16 (layernorm_x16_kernel), qkv GEMM, the 16-bit LePE core, then the second half as in A.
          C  everything else (precision 0, widths off the fast GEMM; another head width raises as it does in fp32): one widen launch,
             the fp32 body (_run), one round launch.
        An fp16 y beyond 65504 is reported to the range guard (code 3) on every route but C, so the block re-runs strict and returns inf."""
        x, io = F._require_io16(x, "x")
        B, L, C = x.shape
        assert L == self.patches_resolution ** 2, "flatten img_tokens has wrong size"
        p = _io_precision(self.precision, io)
        n1, n2, fc1, fc2 = self.norm1, self.norm2, self.mlp.fc1, self.mlp.fc2
        a0 = self.attns[0]
        if not (p and _fast(p, self.qkv, self.proj, fc1, fc2) and a0.dim // a0.num_heads == 32):
            return F.round16(self._run(F.widen16(x), p, _p32), x.dtype)
        if self.branch_num == 2 and F.cswin_stripe_ok(C, self.patches_resolution, self.split_size, self.num_heads, p):
            att = F.cswin_stripe_attention16(x, n1, self.qkv, a0.get_v, self.attns[1].get_v, self.patches_resolution, self.num_heads,
                                             self.split_size, a0.scale)
        else:
            u = F.layernorm16_x16(x, n1.weight, n1.bias, n1.eps)
            qkv = F.linear16(u, F.weight16(self.qkv.weight, p), _p32(self.qkv.bias, "qkv.bias"), out16=True, precision=p)
            att = torch.empty(B, L, C, dtype=x.dtype, device=x.device)
            if self.branch_num == 2:
                a1 = self.attns[1]
                F.cswin_lepe_attention16_pair(qkv, _p32(a0.get_v.weight, "attns.0.get_v.weight"), _p32(a0.get_v.bias, "attns.0.get_v.bias"),
                                              _p32(a1.get_v.weight, "attns.1.get_v.weight"), _p32(a1.get_v.bias, "attns.1.get_v.bias"), att,
                                              self.patches_resolution, a0.num_heads, self.split_size, a0.scale, p)
            else:
                a0.run(qkv, att, 0, p, _p32)
        if F.proj_mlp_fused_ok(C, fc1.weight.shape[0], p) and fc1.bias is not None:
            return F.proj_mlp_fused16(x, att, self.proj, n2, fc1, fc2)
        x1 = F.linear16_res(att, F.weight16(self.proj.weight, p), self.proj.bias, x, precision=p)          # 16-bit residual, fp32 stream
        return _half16(n2, "norm2", fc1, x1, p, lambda h: F.linear16_res(h, F.weight16(fc2.weight, p), fc2.bias, x1, out_dtype=x.dtype,
                                                                        precision=p))

    def forward(self, x):
        """x (B, L, C) fp32, or fp16 / bf16 (the result has the type of x; see _forward16)."""
        if _is16(x):
            return self._forward16(x)
        return self._run(x, self.precision, _same)

    def _run(self, x, precision, P):
        """The fp32 block at `precision` (the setting; None = the default).  forward() passes _same; route C of _forward16 the widened x,
        the precision of its type (or 0) and _p32.  Route C is taken exactly when the test of the 16-bit dataflow below fails, so only
        the fp32 route, written first, hands its parameters through P and overrides the sub-modules' settings; the stripe route and
        the 16-bit GEMM route after it see an fp32 x from forward() only."""
        B, L, C = x.shape
        assert L == self.patches_resolution ** 2, "flatten img_tokens has wrong size"
        p = F._prec(precision)
        n1, n2, mlp, a0 = self.norm1, self.norm2, self.mlp, self.attns[0]
        reso, split = self.patches_resolution, self.split_size
        if not (_fast(p, self.qkv, self.proj, mlp.fc1, mlp.fc2) and a0.dim // a0.num_heads == 32):
            own = None if P is _same else precision                  # the branches' own setting, or the caller's
            qkv = F.linear(_layernorm(n1, x, P, "norm1"), P(self.qkv.weight, "qkv.weight"), P(self.qkv.bias, "qkv.bias"),
                           precision=precision)                      # (B,L,3C) == (B,L,3,C)
            att = torch.empty(B, L, C, dtype=torch.float32, device=x.device)
            a0.run(qkv, att, 0, own, P)
            if self.branch_num == 2:
                self.attns[1].run(qkv, att, C // 2, own, P)
            x = F.linear(att, P(self.proj.weight, "proj.weight"), P(self.proj.bias, "proj.bias"), resid=x, precision=precision)
            u = _layernorm(n2, x, P, "norm2")
            return mlp(u, resid=x) if P is _same else mlp._run(u, x, precision, P)
        if self.branch_num == 2 and F.cswin_stripe_ok(C, reso, split, self.num_heads, p):
            # narrow stages: LN -> qkv -> both stripe attentions in one kernel, qkv never reaches HBM
            att = F.cswin_stripe_attention(x, n1, self.qkv, a0.get_v, self.attns[1].get_v, reso, self.num_heads, split, a0.scale, p)
        else:                        # LN -> qkv -> attention with every GEMM operand kept 16-bit in HBM
            if F.ln_linear16_ok(C, 3 * C, p):        # narrow stages: LayerNorm applied on the way into the qkv GEMM
                qkv = F.ln_linear16(x, n1, self.qkv, out16=True, precision=p)
            else:
                qkv = F.linear16(F.layernorm16(x, n1.weight, n1.bias, n1.eps, p), F.weight16(self.qkv.weight, p), self.qkv.bias,
                                 out16=True, precision=p)
            att = torch.empty(B, L, C, dtype=qkv.dtype, device=x.device)
            if self.branch_num == 2:
                a1 = self.attns[1]                                   # both stripe branches in one launch
                F.cswin_lepe_attention16_pair(qkv, a0.get_v.weight, a0.get_v.bias, a1.get_v.weight, a1.get_v.bias, att, reso,
                                              a0.num_heads, split, a0.scale, p)
            else:
                a0.run(qkv, att, 0)
        if F.proj_mlp_fused_ok(C, mlp.fc1.weight.shape[0], p) and mlp.fc1.bias is not None:
            # proj + residual + LN2 + fc1 + GELU + fc2 + residual in one launch: x1 never reaches HBM
            return F.mlp_fused(x, n2, mlp.fc1, mlp.fc2, precision=p, ctx16=att, proj=self.proj)
        fused_mlp = F.mlp_fused_ok(C, mlp.fc1.weight.shape[0], p) and mlp.fc1.bias is not None
        if not fused_mlp:
            # stage 3 (C = 256): the proj GEMM owns whole rows, so it also writes norm2(x) in the operand format (no LayerNorm launch)
            got = F.linear16_ln16(att, F.weight16(self.proj.weight, p), self.proj.bias, x, n2, p)
            if got is not None:
                x, u = got
                return mlp(u, resid=x)
        x = F.linear16(att, F.weight16(self.proj.weight, p), self.proj.bias, resid=x, precision=p)
        if fused_mlp:
            return F.mlp_fused(x, n2, mlp.fc1, mlp.fc2, precision=p)      # LN2 + fc1 + GELU + fc2 + residual
        return mlp(F.layernorm16(x, n2.weight, n2.bias, n2.eps, p), resid=x)


class Merge_Block(nn.Module):
    """cswin.py:218-233: conv 3x3 stride 2 between stages, as an implicit GEMM straight on the token-major activations."""

    def __init__(self, dim, dim_out, norm_layer=nn.LayerNorm, precision=None):
        super().__init__()
        self.conv = nn.Conv2d(dim, dim_out, 3, 2, 1)
        self.norm = norm_layer(dim_out)
        self.precision = precision

    _mi355_fp16_io_saturates = True          # the conv stages its operands in the format of the type: guarded like an fp32 x

    def forward(self, x):
        """x (B, L, C) fp32, or fp16 / bf16: widened, the fp32 conv (operand format = the type; precision 0 stays strict) and LayerNorm,
        rounded once -- the result has the type of x.  It runs three times per model: no 16-bit kernel of its own."""
        B, L, C = x.shape
        H = W = int(round(L ** 0.5))
        if _is16(x):
            x, io = F._require_io16(x, "x")
            y, _ = F.conv2d_tokens(F.widen16(x), _p32(self.conv.weight, "conv.weight"), _p32(self.conv.bias, "conv.bias"), 3, 2, 1, in_layout=1,
                                   hw=(H, W), precision=_io_precision(self.precision, io))
            return F.round16(F.layernorm(y, _p32(self.norm.weight, "norm.weight"), _p32(self.norm.bias, "norm.bias"), self.norm.eps), x.dtype)
        y, _ = F.conv2d_tokens(x, self.conv.weight, self.conv.bias, 3, 2, 1, in_layout=1, hw=(H, W), precision=self.precision)
        return F.layernorm(y, self.norm.weight, self.norm.bias, self.norm.eps)


class CSWinTransformer(nn.Module):
    """Full CSWin (cswin.py:235-346): stem conv 7x7/4 + LN, four stages of CSWinBlocks with Merge_Blocks between, LN, token mean,
    head.  Same constructor, state_dict and init stream as the reference (activation checkpointing is a training feature: ignored)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=96, depth=[2, 2, 6, 2],
                 split_size=[3, 5, 7], num_heads=12, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0.,
                 hybrid_backbone=None, norm_layer=nn.LayerNorm, use_chk=False, precision=None):
        super().__init__()
        self.use_chk = use_chk
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.precision = precision
        heads = num_heads
        self.stage1_conv_embed = nn.Sequential(nn.Conv2d(in_chans, embed_dim, 7, 4, 2), nn.Identity(), nn.LayerNorm(embed_dim))

        def stage(dim, n, head, reso, split, last=False):
            return nn.ModuleList([CSWinBlock(dim=dim, num_heads=head, reso=reso, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                             qk_scale=qk_scale, split_size=split, drop=drop_rate, attn_drop=attn_drop_rate,
                                             norm_layer=norm_layer, last_stage=last, precision=precision) for _ in range(n)])

        d = embed_dim
        self.stage1 = stage(d, depth[0], heads[0], img_size // 4, split_size[0])
        self.merge1 = Merge_Block(d, d * 2, precision=precision)
        d *= 2
        self.stage2 = stage(d, depth[1], heads[1], img_size // 8, split_size[1])
        self.merge2 = Merge_Block(d, d * 2, precision=precision)
        d *= 2
        self.stage3 = stage(d, depth[2], heads[2], img_size // 16, split_size[2])
        self.merge3 = Merge_Block(d, d * 2, precision=precision)
        d *= 2
        self.stage4 = stage(d, depth[-1], heads[3], img_size // 32, split_size[-1], last=True)
        self.norm = norm_layer(d)
        self.head = nn.Linear(d, num_classes) if num_classes > 0 else nn.Identity()
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, (nn.LayerNorm, nn.BatchNorm2d)):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def forward_features(self, x):
        stem, ln = self.stage1_conv_embed[0], self.stage1_conv_embed[2]
        x, _ = F.conv2d_tokens(x, stem.weight, stem.bias, 7, 4, 2, in_layout=0, precision=self.precision)
        x = F.layernorm(x, ln.weight, ln.bias, ln.eps)
        for blk in self.stage1:
            x = blk(x)
        for pre, blocks in ((self.merge1, self.stage2), (self.merge2, self.stage3), (self.merge3, self.stage4)):
            x = pre(x)
            for blk in blocks:
                x = blk(x)
        x = F.layernorm(x, self.norm.weight, self.norm.bias, self.norm.eps)
        return F.token_mean(x)

    _mi355_fp16_io_saturates = True

    def _forward16(self, img):
        """The model on an fp16 / bf16 image: the composition of its parts on 16-bit tensors, logits in the type of the image.  The stem
        (conv + LayerNorm) runs on the widened image and is rounded once; every block and merge is 16-bit in, 16-bit out; the final
        LayerNorm reads the 16-bit stream (layernorm_x16_kernel), the token mean accumulates it in fp32, the head is fp32 and the
        (B, classes) logits are the one torch cast.  Precision 0 (or a strict re-run): the final LayerNorm is the fp32 one on the widened
        stream."""
        img, io = F._require_io16(img, "img")
        p = _io_precision(self.precision, io)
        stem, ln = self.stage1_conv_embed[0], self.stage1_conv_embed[2]
        x, _ = F.conv2d_tokens(F.widen16(img), _p32(stem.weight, "stem.weight"), _p32(stem.bias, "stem.bias"), 7, 4, 2, in_layout=0, precision=p)
        x = F.round16(F.layernorm(x, _p32(ln.weight, "stem.norm.weight"), _p32(ln.bias, "stem.norm.bias"), ln.eps), img.dtype)
        for blk in self.stage1:
            x = blk(x)
        for pre, blocks in ((self.merge1, self.stage2), (self.merge2, self.stage3), (self.merge3, self.stage4)):
            x = pre(x)
            for blk in blocks:
                x = blk(x)
        if p:
            pooled = F.token_mean16(F.layernorm16_x16(x, self.norm.weight, self.norm.bias, self.norm.eps))
        else:
            pooled = F.token_mean(F.layernorm(F.widen16(x), _p32(self.norm.weight, "norm.weight"), _p32(self.norm.bias, "norm.bias"), self.norm.eps))
        if isinstance(self.head, nn.Identity):
            return pooled.to(img.dtype)
        return F.linear(pooled, _p32(self.head.weight, "head.weight"), _p32(self.head.bias, "head.bias"), precision=p).to(img.dtype)

    def forward(self, x):
        """x (B, 3, H, W) fp32, or fp16 / bf16 (logits in the type of x; see _forward16)."""
        if _is16(x):
            return self._forward16(x)
        x = self.forward_features(x)
        if isinstance(self.head, nn.Identity):
            return x
        return F.linear(x, self.head.weight, self.head.bias, precision=self.precision)


def CSWin_64_12211_tiny_224(pretrained=False, **kwargs):
    return CSWinTransformer(patch_size=4, embed_dim=64, depth=[1, 2, 21, 1], split_size=[1, 2, 7, 7], num_heads=[2, 4, 8, 16],
                            mlp_ratio=4., **kwargs)


def CSWin_64_24322_small_224(pretrained=False, **kwargs):
    return CSWinTransformer(patch_size=4, embed_dim=64, depth=[2, 4, 32, 2], split_size=[1, 2, 7, 7], num_heads=[2, 4, 8, 16],
                            mlp_ratio=4., **kwargs)
