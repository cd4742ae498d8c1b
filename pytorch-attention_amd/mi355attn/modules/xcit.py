"""Drop-in XCiT modules (reference: vision_transformers/xcit.py), forward routed to libmi355attn.

  XCA       xcit.py:233-265  cross-covariance attention: (d x d) attention over channels, L2-normalised q/k
  LPI       xcit.py:128-157  dw3x3 -> GELU -> BatchNorm2d(eval) -> dw3x3 on the token grid
  XCABlock  xcit.py:267-294  x += g1*XCA(LN1 x); x += g3*LPI(LN3 x); x += g2*Mlp(LN2 x)

  PositionalEncodingFourier  xcit.py:42-77   input-independent sin/cos table -> 1x1 conv (one small GEMM, cached)
  ConvPatchEmbed             xcit.py:79-126  3x3 stride-2 conv + BatchNorm (+GELU) chain as implicit GEMMs, BN folded
  ClassAttention(Block)      xcit.py:159-231 cls-token attention stage, including the reference's token-path quirks
  XCiT, xcit_nano_12_p16     xcit.py:296-414

BatchNorm runs with its running statistics (inference engine); compare against the reference in .eval().

Envelope of XCA, XCABlock, ClassAttention(Block) and XCiT: every `num_heads` that divides `dim`, head width dim // num_heads up to 256,
dim % 4 == 0 (the condition of functional.linear).  Head widths 32 / 48 / 64 (class attention: 16 / 32 / 48 / 64) run template kernels,
every other width the run-time-width kernels of the same entries (xca_any_kernel, class_attn_any_kernel): same arithmetic, the softmax
over a head's channels masked to the d live columns.  A wider head raises Mi355Error in forward().

fp16 / bf16 activations: XCA, LPI, Mlp, XCABlock, ClassAttention, ClassAttentionBlock, ConvPatchEmbed, XCiT and xcit_nano_12_p16 take a
16-bit device tensor and return that type (ConvPatchEmbed: (tokens16, (Hp, Wp))).  The MFMA operand format is then the tensor's type
(fp16: the precision-1 arithmetic, bf16: precision 2) and a `precision` of None / 1 / 2 / 3 is ignored; precision 0 (explicit, the package
default, or a strict re-run) widens x, runs the strict route and rounds.  Parameters may be fp32 or 16-bit (module.half()).  XCABlock has
a 16-bit dataflow of its own (XCABlock._forward16); XCA and Mlp run their GEMMs on the 16-bit x directly; the other modules widen x
once, run their fp32 body at the precision of the type and round once.  Every fp32 body below is written once, as `_run(.., precision,
P)`: forward() passes the module's setting and the parameters as they are (_same), the 16-bit callers the resolved precision and _p32.
"""
import math

import torch
from torch import nn

from .. import _ffi
from .. import functional as F
from ._io16 import _fast, _half16, _io_precision, _is16, _layernorm, _lin, _ln, _mlp_run, _p32, _round, _same, _wide
from .mhsa import _dropout_is_identity, _no_dropout


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, bias=True, drop=0.):
        super().__init__()
        if act_layer is not nn.GELU:
            raise NotImplementedError("only the exact-erf GELU epilogue is built")
        _no_dropout(drop)
        self.fc1 = nn.Linear(in_features, hidden_features or in_features, bias=bias)
        self.drop1 = nn.Dropout(drop)                      # xcit.py:28,30: the identity in eval mode, refused in train mode
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features, bias=bias)
        self.drop2 = nn.Dropout(drop)
        self.precision = None

    _mi355_fp16_io_saturates = True          # an fp16 x is guarded like an fp32 one: the 16-bit GEMM epilogues can saturate

    def forward(self, x, gamma=None, resid=None):
        """x (.., C) fp32, or fp16 / bf16 (the result has the type of x: fc1 with the GELU 16-bit epilogue, fc2 with a 16-bit store;
        off the fast GEMM widths, at precision 0 or with a gamma / resid: widen, the fp32 body, round)."""
        _dropout_is_identity(self)
        if _is16(x):
            x, io = F._require_io16(x, "x")
            p = _io_precision(self.precision, io)
            fc1, fc2 = self.fc1, self.fc2
            if p and gamma is None and resid is None and fc1.bias is not None and _fast(p, fc1, fc2):
                h = F.linear16(x, F.weight16(fc1.weight, p), _p32(fc1.bias, "fc1.bias"), act=F.ACT_GELU, out16=True, precision=p)
                return F.linear16(h, F.weight16(fc2.weight, p), _p32(fc2.bias, "fc2.bias"), out16=True, precision=p)
            return F.round16(self._run(F.widen16(x), gamma, _wide(resid), p, _p32), x.dtype)
        return self._run(x, gamma, resid, self.precision, _same)

    def _run(self, x, gamma, resid, precision, P):
        """The fp32 forward at `precision` (the setting; None = the default) with the parameters as P hands them over."""
        return _mlp_run(self.fc1, self.fc2, x, resid, precision, P, gamma=gamma)


class LPI(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0., kernel_size=3):
        super().__init__()
        out_features = out_features or in_features
        if kernel_size != 3 or out_features != in_features or act_layer is not nn.GELU:
            raise NotImplementedError("LPI kernel is built for depth-wise 3x3 + GELU only")
        self.conv1 = nn.Conv2d(in_features, out_features, kernel_size=3, padding=1, groups=out_features)
        self.bn = nn.BatchNorm2d(in_features)
        self.conv2 = nn.Conv2d(in_features, out_features, kernel_size=3, padding=1, groups=out_features)

    def forward(self, x, H, W, gamma=None, resid=None, ln=None, stats=None):
        """`ln`: the LayerNorm in front of the block (XCABlock passes norm3 with the un-normalised x): fused into the kernel.  `stats`: that
        LayerNorm's (mean, rstd) per token when the producer of x has already written them (XCA's proj GEMM).
        x fp32, or fp16 / bf16: widened once, the fp32 kernels (there is no 16-bit operand in LPI: nothing to report), rounded once."""
        if _is16(x):
            x, _ = F._require_io16(x, "x")
            return F.round16(self._run(F.widen16(x), H, W, gamma, _wide(resid), ln, stats, _p32), x.dtype)
        return self._run(x, H, W, gamma, resid, ln, stats, _same)

    def _run(self, x, H, W, gamma, resid, ln, stats, P):
        bn = self.bn
        return F.lpi(x, P(self.conv1.weight, "conv1.weight"), P(self.conv1.bias, "conv1.bias"), P(bn.weight, "bn.weight"), P(bn.bias, "bn.bias"),
                     P(bn.running_mean, "bn.running_mean"), P(bn.running_var, "bn.running_var"), bn.eps, P(self.conv2.weight, "conv2.weight"),
                     P(self.conv2.bias, "conv2.bias"), H, W, gamma=None if gamma is None else P(gamma, "gamma"), resid=resid,
                     ln=_ln(ln, P, "ln"), stats=stats)


class XCA(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., precision=None):
        super().__init__()
        self.num_heads = num_heads
        _no_dropout(attn_drop, proj_drop)
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)             # xcit.py:241,243: eval-mode identities
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.precision = precision

    def forward(self, x, gamma=None, resid=None, ln=None, stats_eps=None):
        """`ln`: the LayerNorm in front of the block (XCABlock passes norm1 with the un-normalised x) -- applied on the way into the qkv
        GEMM when the width allows (functional.ln_linear16), else by the caller.  `stats_eps` (round 6): the caller wants the LayerNorm
        statistics of the OUTPUT rows (eps of the LayerNorm that follows: XCABlock's norm3) -- the return value is then (y, stats) with
        stats None where the projection kernel does not own whole rows."""
        _dropout_is_identity(self)
        if _is16(x):
            return self._forward16(x, gamma, resid, ln, stats_eps)
        return self._run(x, gamma, resid, ln, stats_eps, self.precision, _same)

    _mi355_fp16_io_saturates = True          # an fp16 x is guarded like an fp32 one: the 16-bit GEMM epilogues can saturate

    def _forward16(self, x, gamma, resid, ln, stats_eps):
        """XCA on an fp16 / bf16 x; the result has the type of x.  On the fast GEMM widths: qkv GEMM on x itself, the 16-bit core, proj with
        a 16-bit store.  LayerScale, residual and the LayerNorm in front are the block's business (XCABlock._forward16 composes the
        pieces itself); a standalone call that passes one, a width off the fast GEMM and precision 0 widen, run the fp32 body, round."""
        x, io = F._require_io16(x, "x")
        p = _io_precision(self.precision, io)
        if p and gamma is None and resid is None and ln is None and stats_eps is None and _fast(p, self.qkv, self.proj):
            qkv = F.linear16(x, F.weight16(self.qkv.weight, p), _p32(self.qkv.bias, "qkv.bias"), out16=True, precision=p)
            ctx16 = F.xca_core(qkv, _p32(self.temperature, "temperature"), self.num_heads, precision=p, out16=True)
            return F.linear16(ctx16, F.weight16(self.proj.weight, p), _p32(self.proj.bias, "proj.bias"), out16=True, precision=p)
        return _round(self._run(F.widen16(x), gamma, _wide(resid), ln, stats_eps, p, _p32), x.dtype)

    def _run(self, x, gamma, resid, ln, stats_eps, precision, P):
        """The fp32 forward at `precision` (the setting; None = the default) with the parameters as P hands them over: _same from forward(),
        _p32 behind a widened 16-bit x."""
        want_stats = stats_eps is not None
        qkv_, proj = _lin(self.qkv, P, "qkv"), _lin(self.proj, P, "proj")
        temperature = P(self.temperature, "temperature")
        gamma = None if gamma is None else P(gamma, "gamma")
        if _fast(precision, qkv_, proj):
            p = F._prec(precision)      # GEMMs on 16-bit operands; the d x d covariance core itself is exact fp32
            if ln is not None:
                qkv = F.ln_linear16(x, ln, self.qkv, out16=True, precision=p)
            else:
                qkv = F.cast_linear16(x, F.weight16(qkv_.weight, p), qkv_.bias, precision=p)    # fp32 x: the cast rides in the GEMM
            ctx16 = F.xca_core(qkv, temperature, self.num_heads, precision=p, out16=True)
            folded = F.weight16_scaled(proj.weight, proj.bias, gamma, p) if gamma is not None else None
            if folded is not None:                            # LayerScale folded into the projection (no activation in between)
                w16, b = folded
                if want_stats and resid is not None:
                    got = F.linear16_stats(ctx16, w16, b, resid, stats_eps, p)
                    if got is not None:
                        return got
                y = F.linear16(ctx16, w16, b, resid=resid, precision=p)
                return (y, None) if want_stats else y
            # no LayerScale, or gamma * W would leave the fp16 normal range (eta = 1e-5 initialisations): gamma in the fp32 epilogue
            y = F.linear16(ctx16, F.weight16(proj.weight, p), proj.bias, gamma=gamma, resid=resid, precision=p)
            return (y, None) if want_stats else y
        qkv = F.linear(x, qkv_.weight, qkv_.bias, precision=precision)
        ctx = F.xca_core(qkv, temperature, self.num_heads, precision=precision)
        y = F.linear(ctx, proj.weight, proj.bias, gamma=gamma, resid=resid, precision=precision)
        return (y, None) if want_stats else y


class XCABlock(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, num_tokens=196, eta=None, precision=None):
        super().__init__()
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError("only nn.LayerNorm is built")
        self.norm1 = norm_layer(dim)
        self.attn = XCA(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                        proj_drop=drop, precision=precision)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.mlp.precision = precision
        self.norm3 = norm_layer(dim)
        self.local_mp = LPI(in_features=dim, act_layer=act_layer)
        # eta=None multiplies None by a tensor in the reference (xcit.py:286): same TypeError here
        self.gamma1 = nn.Parameter(eta * torch.ones(dim), requires_grad=True)
        self.gamma2 = nn.Parameter(eta * torch.ones(dim), requires_grad=True)
        self.gamma3 = nn.Parameter(eta * torch.ones(dim), requires_grad=True)

    _mi355_fp16_io_saturates = True          # an fp16 x is guarded like an fp32 one: the fp16 LN operand and the 16-bit epilogues can saturate

    def forward(self, x, H, W):
        """x (B, N, C) fp32, or fp16 / bf16 (the result has the type of x; see _forward16)."""
        _dropout_is_identity(self)
        if _is16(x):
            return self._forward16(x, H, W)
        return self._run(x, H, W, self.attn.precision, _same)

    def _run(self, x, H, W, precision, P):
        """The fp32 block at `precision` (the setting; None = the default) with the parameters as P hands them over: _same from forward(),
        _p32 behind the widened x of _forward16 (whose precision is 0 or the type of the 16-bit x)."""
        p = F._prec(precision)
        attn, mlp = self.attn, self.mlp
        fast = _fast(p, attn.qkv, attn.proj, mlp.fc1, mlp.fc2)

        # the proj GEMM of the attention branch writes norm3's statistics of x beside x where it owns whole rows (gemm16_wreg, round 6)
        if fast and F.ln_linear16_ok(x.shape[-1], 3 * x.shape[-1], p):
            x, st = attn._run(x, self.gamma1, x, self.norm1, self.norm3.eps, precision, P)        # LayerNorm fused into the qkv GEMM
        else:
            x, st = attn._run(_layernorm(self.norm1, x, P, "norm1", fast, p), self.gamma1, x, None, self.norm3.eps, precision, P)
        x = self.local_mp._run(x, H, W, self.gamma3, x, self.norm3, st, P)                        # norm3 fused into the LPI kernel
        if fast and F.mlp_fused_ok(x.shape[-1], mlp.fc1.weight.shape[0], p) and mlp.fc1.bias is not None:
            return F.mlp_fused(x, self.norm2, mlp.fc1, mlp.fc2, gamma=P(self.gamma2, "gamma2"), precision=p)   # LN2 + MLP + LayerScale + residual
        return mlp._run(_layernorm(self.norm2, x, P, "norm2", fast, p), self.gamma2, x, mlp.precision if P is _same else precision, P)

    def _forward16(self, x, H, W):
        """The block on an fp16 / bf16 x; the result has the type of x.  The MFMA operand format is that type (fp16: the precision-1
        arithmetic, bf16: precision 2) and a `precision` of None / 1 / 2 / 3 is ignored; precision 0 (explicit, the package default, or a
        strict re-run) widens x, runs the strict route and rounds.  Parameters may be fp32 or 16-bit.
          G  every GEMM on the fast widths (p != 0): LayerNorm 1 reads x in 16 bit (layernorm_x16_kernel), the qkv GEMM and the XCA core
             stay 16-bit, and proj + LayerScale adds x as a 16-BIT RESIDUAL into the fp32 stream x1 -- on gemm16_wreg_kernel<..,
             resid16+stats> where LayerScale folds into the weights at N = K = 256 / 384 (norm3's statistics come with x1), else on
             gemm16_res_kernel (gamma in its epilogue where the fold is refused: fp16 at eta = 1e-5).  LPI runs its fp32 kernels on x1.
             The last third rounds y ONCE in its epilogue: mlp_fused_kernel<.., o16> at C = 64 / 128 (LayerNorm 2, both products,
             LayerScale and residual in one launch), else LayerNorm 2, fc1 + GELU and fc2 + LayerScale + the fp32 residual x2 on
             gemm16_res_kernel with a 16-bit store.  No widen, round or cast launch over the activations.  The weight-split MLP kernel
             (option "mlp_wide" = 1, C = 256 / 384) has no 16-bit store: the option is ignored here.  The LayerNorm-into-qkv fold of the
             fp32 block at C = 64 / 128 (mi355_ln_linear16_fwd) reads fp32 rows only: this route runs LayerNorm 1 and the qkv GEMM instead.
          W  everything else (precision 0, dim % 64 != 0, MLP widths off the fast GEMM): one widen launch, the fp32 body (_run) at the
             precision of the type or 0, one round launch.
        An fp16 y beyond 65504 is reported to the range guard (code 3) on route G, so the block re-runs strict and returns inf."""
        x, io = F._require_io16(x, "x")
        p = _io_precision(self.attn.precision, io)
        attn, mlp = self.attn, self.mlp
        qkv_, proj, fc1, fc2, n1, n2 = attn.qkv, attn.proj, mlp.fc1, mlp.fc2, self.norm1, self.norm2
        if not (p and x.dim() == 3 and _fast(p, qkv_, proj, fc1, fc2)):
            return F.round16(self._run(F.widen16(x), H, W, p, _p32), x.dtype)
        u = F.layernorm16_x16(x, n1.weight, n1.bias, n1.eps)
        qkv = F.linear16(u, F.weight16(qkv_.weight, p), _p32(qkv_.bias, "qkv.bias"), out16=True, precision=p)
        ctx16 = F.xca_core(qkv, _p32(attn.temperature, "temperature"), attn.num_heads, precision=p, out16=True)
        x1, st = self._scaled_res(ctx16, proj, self.gamma1, x, torch.float32, p, stats_eps=self.norm3.eps)
        x2 = self.local_mp._run(x1, H, W, self.gamma3, x1, self.norm3, st, _p32)
        y = F.mlp_fused_o16(x2, n2, fc1, fc2, gamma=self.gamma2, precision=p)         # None: not built for the width
        if y is not None:
            return y
        return _half16(n2, "norm2", fc1, x2, p, lambda h: self._scaled_res(h, fc2, self.gamma2, x2, x.dtype, p)[0])

    @staticmethod
    def _scaled_res(a16, lin, gamma, resid, out_dtype, p, stats_eps=None):
        """(resid + gamma * lin(a16), row statistics or None) with a 16-bit residual or a 16-bit result: the LayerScale folded into the
        weights where F.weight16_scaled takes it (as XCA._run does), else in the epilogue of gemm16_res_kernel."""
        folded = F.weight16_scaled(_p32(lin.weight, "weight"), _p32(lin.bias, "bias"), _p32(gamma, "gamma"), p)
        if folded is not None:
            w16, b = folded
            if stats_eps is not None:
                got = F.linear16_stats_r16(a16, w16, b, resid, stats_eps, p)
                if got is not None:
                    return got
            return F.linear16_res_scale(a16, w16, b, None, resid, out_dtype=out_dtype, precision=p), None
        return F.linear16_res_scale(a16, F.weight16(lin.weight, p), lin.bias, gamma, resid, out_dtype=out_dtype, precision=p), None


class PositionalEncodingFourier(nn.Module):
    """xcit.py:42-77.  The encoding depends on (H, W) and on token_projection only, never on the input: the sin/cos feature
    table is built once per grid with the reference's own fp32 formula (host torch ops on index ranges -- constants, no
    activations involved) and the 1x1 conv runs as a GEMM on the device; the result (H*W, dim) is cached per weight version."""

    def __init__(self, hidden_dim=32, dim=768, temperature=10000):
        super().__init__()
        self.token_projection = nn.Conv2d(hidden_dim * 2, dim, kernel_size=1)
        self.scale = 2 * math.pi
        self.temperature = temperature
        self.hidden_dim = hidden_dim
        self.dim = dim
        self._cache = {}

    def features(self, H, W):
        """(H*W, 2*hidden_dim) rows [pos_y | pos_x] of xcit.py:57-74, batch-independent.  Closed form of the reference's cumsum-of-mask
        construction: pixel (i, j) has the normalised coordinates (i+1) / (H + 1e-6) * 2 pi and (j+1) / (W + 1e-6) * 2 pi; feature pair p
        of an axis holds sin / cos of coordinate / temperature^(2p / hidden_dim).  Every step is the same fp32 operation the reference
        performs (the sums of ones are exact integers), so the table matches it to the bit."""
        f32 = torch.float32
        half = self.hidden_dim // 2

        def axis(n):                                              # (n, hidden_dim): [sin f0, cos f0, sin f1, cos f1, ...]
            coord = torch.arange(1, n + 1, dtype=f32) / (torch.tensor(float(n), dtype=f32) + 1e-6) * self.scale
            freq = self.temperature ** (2 * torch.arange(half, dtype=f32) / self.hidden_dim)
            ang = coord[:, None] / freq[None, :]
            out = torch.empty(n, 2 * half, dtype=f32)
            out[:, 0::2], out[:, 1::2] = ang.sin(), ang.cos()
            return out

        if self.hidden_dim % 2:
            raise ValueError("PositionalEncodingFourier: hidden_dim must be even (sin / cos pairs)")
        fy, fx = axis(H), axis(W)
        feat = torch.empty(H, W, 2 * self.hidden_dim, dtype=f32)
        feat[:, :, :self.hidden_dim] = fy[:, None, :]
        feat[:, :, self.hidden_dim:] = fx[None, :, :]
        return feat.reshape(H * W, 2 * self.hidden_dim)

    def tokens(self, H, W, P=_same):
        """Position rows (H*W, dim) = token_projection(features), the layout forward_features adds to the patch tokens.  Always fp32;
        P = _p32 (XCiT on a 16-bit image): 16-bit parameters through their cached fp32 copies."""
        w, b = self.token_projection.weight, self.token_projection.bias
        tag = (w._version, w.data_ptr(), b._version, b.data_ptr())
        hit = self._cache.get((H, W))
        if hit is None or hit[0] != tag:
            feat = self.features(H, W).to(w.device)
            pos = F.linear(feat, P(w, "token_projection.weight").reshape(self.dim, -1), P(b, "token_projection.bias"), precision=F.PREC_STRICT)
            hit = (tag, pos)
            self._cache[(H, W)] = hit
        return hit[1]

    def forward(self, B, H, W):
        """xcit.py:56-77: the encoding as a (B, dim, H, W) map.  (XCiT itself uses tokens(H, W): the rows are added inside the last
        patch-embedding conv.)  The batch axis is a broadcast view, as every image gets the same table."""
        pos = self.tokens(H, W)                                            # (H*W, dim) on the device
        return F.tokens_to_nchw(pos.reshape(1, H * W, self.dim), H, W).expand(B, -1, -1, -1)


def conv3x3(in_channels, out_channels, stride=1):
    return nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=stride, padding=1, bias=False),
                         nn.BatchNorm2d(out_channels))


class ConvPatchEmbed(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, precision=None):
        super().__init__()
        self.img_size = img_size
        self.patch_size = patch_size
        self.num_patches = (img_size // patch_size) ** 2
        self.precision = precision
        if patch_size == 16:
            self.proj = nn.Sequential(conv3x3(3, embed_dim // 8, 2), nn.GELU(), conv3x3(embed_dim // 8, embed_dim // 4, 2), nn.GELU(),
                                      conv3x3(embed_dim // 4, embed_dim // 2, 2), nn.GELU(), conv3x3(embed_dim // 2, embed_dim, 2))
        elif patch_size == 8:
            self.proj = nn.Sequential(conv3x3(3, embed_dim // 4, 2), nn.GELU(), conv3x3(embed_dim // 4, embed_dim // 2, 2), nn.GELU(),
                                      conv3x3(embed_dim // 2, embed_dim, 2))
        else:
            raise ValueError("For convolutional projection, patch size has to be in [8, 16]")

    _mi355_fp16_io_saturates = True          # the convs stage their operands in the format of the type: guarded like an fp32 image

    def forward(self, x, padding_size=None, pos=None):
        """Returns (tokens (B, Hp*Wp, E), (Hp, Wp)).  Layer 1 gathers from NCHW, the rest from the token-major output of the
        previous layer; BatchNorm is folded into weights/bias, GELU and (last layer) the position rows ride in the epilogue.
        A 16-bit image gives 16-bit tokens: widened once, the fp32 chain at the precision of the type (pos, fp32, still in the last
        conv's epilogue), rounded once."""
        if _is16(x):
            x, io = F._require_io16(x, "img")
            tok, hw = self._run(F.widen16(x), pos, _io_precision(self.precision, io))
            return F.round16(tok, x.dtype), hw
        return self._run(x, pos, self.precision)

    def _run(self, x, pos, precision):
        stages = [m for m in self.proj if isinstance(m, nn.Sequential)]
        hw = None
        for li, st in enumerate(stages):
            layout = 0 if li == 0 else 1
            wrows, bias = F.conv_bn_rows(st[0].weight, st[1], layout)
            last = li == len(stages) - 1
            x, hw = F.conv2d_tokens(x, None, bias, 3, 2, 1, layout, hw=hw, precision=precision,
                                    act=F.ACT_NONE if last else F.ACT_GELU, pos=pos if last else None, wrows=wrows)
        return x, hw


class ClassAttention(nn.Module):
    """xcit.py:159-188.  Only the cls query is ever used (:180), so q is projected for the cls rows alone; k, v for all tokens."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., precision=None):
        super().__init__()
        self.num_heads = num_heads
        _no_dropout(attn_drop, proj_drop)
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)             # xcit.py:170,172: eval-mode identities
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.precision = precision

    def cls_out(self, u, precision="own", P=_same):
        """proj(attention of the cls query over all tokens) for normed tokens u (B,N,C) fp32 -> (B,C), at `precision` (default: the
        module's setting) with the parameters as P hands them over (_p32 behind a widened 16-bit x)."""
        precision = self.precision if isinstance(precision, str) else precision
        B, N, C = u.shape
        w, b = P(self.qkv.weight, "qkv.weight"), P(self.qkv.bias, "qkv.bias") if self.qkv.bias is not None else None
        kv = F.linear(u, w[C:], None if b is None else b[C:], precision=precision)                  # (B,N,2C)
        qc = F.linear(u[:, 0], w[:C], None if b is None else b[:C], precision=precision)          # (B,C), cls rows in place
        att = F.class_attention(qc, kv, kv[:, :, C:], self.num_heads, self.scale, N, C, 2 * C)
        return F.linear(att, P(self.proj.weight, "proj.weight"), P(self.proj.bias, "proj.bias"), precision=precision)

    _mi355_fp16_io_saturates = True          # the GEMMs stage their operands in the format of the type: guarded like an fp32 x

    def forward(self, x):
        """x (B, N, C) fp32, or fp16 / bf16: widened once, the fp32 body at the precision of the type (0: strict), rounded once."""
        _dropout_is_identity(self)
        if _is16(x):
            x, io = F._require_io16(x, "x")
            return F.round16(self._run(F.widen16(x), _io_precision(self.precision, io), _p32), x.dtype)
        return self._run(x, self.precision, _same)

    def _run(self, x, precision, P):
        B, N, C = x.shape
        out = torch.empty_like(x)
        F.axpby(x[:, 1:], out[:, 1:], B, (N - 1) * C, N * C, N * C)                  # tokens pass through (xcit.py:187)
        F.axpby(self.cls_out(x, precision, P), out, B, C, C, N * C)
        return out


class ClassAttentionBlock(nn.Module):
    """xcit.py:190-231, reproduced with its token-path behaviour: the attention returns the NORMED patch tokens (:187), so
    patch tokens become x + gamma1*LN1(x) (:219); the second residual adds them to themselves (:226-230), i.e. doubles them."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., act_layer=nn.GELU,
                 norm_layer=nn.LayerNorm, eta=None, tokens_norm=False, precision=None):
        super().__init__()
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError("only nn.LayerNorm is built")
        self.norm1 = norm_layer(dim)
        self.attn = ClassAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                                   proj_drop=drop, precision=precision)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.mlp.precision = precision
        if eta is not None:
            self.gamma1 = nn.Parameter(eta * torch.ones(dim), requires_grad=True)
            self.gamma2 = nn.Parameter(eta * torch.ones(dim), requires_grad=True)
        else:
            self.gamma1, self.gamma2 = 1.0, 1.0
        self.tokens_norm = tokens_norm           # xcit.py:221-222: norm2 over every token instead of the cls token only

    _mi355_fp16_io_saturates = True          # the GEMMs stage their operands in the format of the type: guarded like an fp32 x

    def forward(self, x, H, W, mask=None):
        """x (B, N, C) fp32, or fp16 / bf16: widened once, the fp32 body at the precision of the type (0: strict), rounded once."""
        if _is16(x):
            x, io = F._require_io16(x, "x")
            return F.round16(self._run(F.widen16(x), _io_precision(self.attn.precision, io), _p32), x.dtype)
        return self._run(x, "own", _same)

    def _run(self, x, precision, P):
        """The fp32 body.  precision "own": the sub-modules' settings (forward()); else the resolved precision of a 16-bit caller, with
        the parameters through P (_p32)."""
        own = isinstance(precision, str)
        B, N, C = x.shape
        g1 = P(self.gamma1, "gamma1") if isinstance(self.gamma1, torch.Tensor) else None
        g2 = P(self.gamma2, "gamma2") if isinstance(self.gamma2, torch.Tensor) else None
        n2w, n2b = P(self.norm2.weight, "norm2.weight"), P(self.norm2.bias, "norm2.bias")
        u = _layernorm(self.norm1, x, P, "norm1")
        if self.tokens_norm:
            # patch tokens: 2 * LN2(x + g1 * LN1(x)) -- the doubling of the second residual rides in the LayerNorm's affine part
            t1 = torch.empty_like(x)
            F.axpby(x, t1, B * N, C, C, C, alpha=1.0, u=u, ldu=C, gamma=g1)
            w2, b2 = _twice(self, n2w, "_n2w"), _twice(self, n2b, "_n2b")
            out = F.layernorm(t1, w2, b2, self.norm2.eps)
        else:
            out = torch.empty_like(x)
            # patch tokens: 2 * (x + g1 * LN1(x)), g1 = 1.0 without LayerScale; the cls rows written here are replaced below
            F.axpby(x, out, B * N, C, C, C, alpha=2.0, u=u, ldu=C, gamma=_twos(self, C, x.device) if g1 is None else _twice(self, g1))
        # cls token: c1 = x0 + g1 * proj(attn); c2 = LN2(c1); out0 = c2 + g2 * mlp(c2)
        c1 = torch.empty(B, C, dtype=torch.float32, device=x.device)
        F.axpby(x, c1, B, C, N * C, C, u=self.attn.cls_out(u, "own" if own else precision, P), ldu=C, gamma=g1)
        c2 = F.layernorm(c1, n2w, n2b, self.norm2.eps)
        c3 = self.mlp(c2, gamma=g2, resid=c2) if own else self.mlp._run(c2, g2, c2, precision, P)
        F.axpby(c3, out, B, C, C, N * C)
        return out


def _twice(owner, g, slot="_g1x2"):
    """2 * parameter for the doubled patch-token path, cached per parameter version on the block."""
    tag = (g._version, g.data_ptr())
    hit = getattr(owner, slot, None)
    if hit is None or hit[0] != tag:
        buf = torch.empty_like(g.detach())
        F.axpby(g.detach(), buf, 1, g.numel(), g.numel(), g.numel(), alpha=2.0)
        hit = (tag, buf)
        setattr(owner, slot, hit)
    return hit[1]


def _twos(owner, C, device):
    """The doubled gamma1 of a block without LayerScale (eta=None: gamma1 is the number 1.0, xcit.py:214): a constant row of 2s."""
    hit = getattr(owner, "_twos", None)
    if hit is None or hit.numel() != C or hit.device != device:
        hit = torch.full((C,), 2.0, dtype=torch.float32, device=device)
        owner._twos = hit
    return hit


class XCiT(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., norm_layer=None, cls_attn_layers=2,
                 use_pos=True, patch_proj='linear', eta=None, tokens_norm=False, precision=None):
        super().__init__()
        _no_dropout(drop_rate, attn_drop_rate)             # accepted as the reference accepts them: eval-mode identities (xcit.py:333-346)
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.patch_embed = ConvPatchEmbed(img_size=img_size, embed_dim=embed_dim, patch_size=patch_size, precision=precision)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_drop = nn.Dropout(p=drop_rate)
        self.blocks = nn.ModuleList([
            XCABlock(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate,
                     attn_drop=attn_drop_rate, norm_layer=norm_layer, num_tokens=num_patches, eta=eta, precision=precision)
            for _ in range(depth)])
        self.cls_attn_blocks = nn.ModuleList([
            ClassAttentionBlock(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                drop=drop_rate, attn_drop=attn_drop_rate, norm_layer=norm_layer, eta=eta, tokens_norm=tokens_norm,
                                precision=precision)
            for _ in range(cls_attn_layers)])
        self.norm = norm_layer(embed_dim)
        self.head = nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()
        self.pos_embeder = PositionalEncodingFourier(dim=embed_dim)
        self.use_pos = use_pos
        self.precision = precision
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    _mi355_fp16_io_saturates = True

    def forward_features(self, x):
        """img (B, 3, H, W) fp32 -> the normed cls row (B, C) fp32.  A 16-bit image: the composition of the model's 16-bit parts up to the
        last XCABlock, then the fp32 tail -- ConvPatchEmbed gives 16-bit tokens (the position rows ride in the last conv's fp32
        epilogue, before the one rounding), every XCABlock is 16-bit in and out, and the class-attention tail is ONE fp32 unit: one
        widen of the last block's tokens, the cls concatenation, the ClassAttentionBlocks and the final LayerNorm of the cls row, all
        at the precision of the type (0: strict) with the parameters through _p32.  The result is fp32 either way."""
        _dropout_is_identity(self)
        ps = self.patch_embed.patch_size
        Hp, Wp = x.shape[2] // ps, x.shape[3] // ps
        if _is16(x):
            x, io = F._require_io16(x, "img")
            p, P = _io_precision(self.precision, io), _p32
        else:
            p, P = "own", _same
        pos = self.pos_embeder.tokens(Hp, Wp, P) if self.use_pos else None
        x, (Hp, Wp) = self.patch_embed(x, pos=pos)                    # + position rows in the last conv's epilogue (:398-400)
        for blk in self.blocks:
            x = blk(x, Hp, Wp)
        if P is _p32:
            x = F.widen16(x)                                          # the tail is fp32: one widen per forward
        B, N, C = x.shape
        tok = torch.empty(B, N + 1, C, dtype=torch.float32, device=x.device)       # cat(cls, x) (:405-406)
        F.axpby(P(self.cls_token, "cls_token"), tok, B, C, 0, (N + 1) * C)
        F.axpby(x, tok[:, 1:], B, N * C, N * C, (N + 1) * C)
        x = tok
        for blk in self.cls_attn_blocks:
            x = blk(x, Hp, Wp) if P is _same else blk._run(x, p, P)
        cls = torch.empty(B, C, dtype=torch.float32, device=x.device)
        F.axpby(x, cls, B, C, (N + 1) * C, C)                                       # gather the cls rows
        return _layernorm(self.norm, cls, P, "norm")                                # norm(x)[:, 0]: LayerNorm is per token

    def forward(self, x):
        """Logits in the type of the image: fp32, or fp16 / bf16 (the head runs in fp32 at the precision of the type; the (B, classes)
        logits are cast by torch -- no pass over activations is)."""
        if _is16(x):
            dtype, p = x.dtype, _io_precision(self.precision, _ffi.IO_CODES[x.dtype])
            x = self.forward_features(x)
            if not isinstance(self.head, nn.Identity):
                x = F.linear(x, _p32(self.head.weight, "head.weight"), _p32(self.head.bias, "head.bias"), precision=p)
            return x.to(dtype)
        x = self.forward_features(x)
        if isinstance(self.head, nn.Identity):
            return x
        return F.linear(x, self.head.weight, self.head.bias, precision=self.precision)


def xcit_nano_12_p16(pretrained=False, **kwargs):
    if pretrained:
        raise NotImplementedError("no checkpoints are bundled (the reference ships none either)")
    return XCiT(patch_size=16, embed_dim=128, depth=12, num_heads=4, mlp_ratio=4, qkv_bias=True, norm_layer=nn.LayerNorm, eta=1.0,
                tokens_norm=False, **kwargs)
