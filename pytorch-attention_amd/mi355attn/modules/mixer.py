"""Drop-in MLP-Mixer layer (reference: mlps/mlp_mixer.py:16-50), forward routed to libmi355attn.

Token mixing is a LEFT multiplication of each image's (N x C) matrix, so the reference's two transposes
(mlp_mixer.py:47) never materialise: the batched GEMM reads the activation as its K-major operand.
"""
from torch import nn

from .. import _ffi
from .. import functional as F
from ._io16 import _fast, _half16, _io_precision, _is16, _layernorm, _mlp_run, _p32, _patch_embed16, _same


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, drop=0):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
        self.precision = None

    def forward(self, x, resid=None):
        return self._run(x, resid, self.precision, _same)

    def _run(self, x, resid, precision, P):
        return _mlp_run(self.fc1, self.fc2, x, resid, precision, P)


class MixerLayer(nn.Module):
    def __init__(self, embedding_dim, sequence_len, mlp_ratio=[0.5, 4], drop=0, precision=None):
        super().__init__()
        self.norm1 = nn.LayerNorm(embedding_dim)
        self.token_mlp = Mlp(sequence_len, int(embedding_dim * mlp_ratio[0]), drop=drop)
        self.norm2 = nn.LayerNorm(embedding_dim)
        self.channel_mlp = Mlp(embedding_dim, int(embedding_dim * mlp_ratio[1]), drop=drop)
        self.precision = precision
        self.channel_mlp.precision = precision

    _mi355_fp16_io_saturates = True          # an fp16 x is guarded like an fp32 one: LN(x), gelu(H) and the 16-bit epilogues can saturate

    def forward(self, x):
        """x (B, N, C) fp32, or fp16 / bf16 (the result has the type of x; see _forward16)."""
        if _is16(x):
            return self._forward16(x)
        t = self.token_mlp
        T, N = t.fc1.weight.shape
        if x.dim() == 3 and t.fc1.bias is not None and t.fc2.bias is not None and F.mixer_token_ok(N, T, x.shape[-1], self.precision):
            # the whole half in one kernel: neither LN(x)^T nor the hidden tensor exists in HBM (csrc/mixer_fused.hip)
            x = F.mixer_token_mlp(x.contiguous(), self.norm1, t.fc1, t.fc2, F._prec(self.precision))
        else:
            x = self._token_mix(x, self.precision, _same)
        return self._channel_mix(x, self.precision, _same, x.dtype)

    def _token_mix(self, x, precision, P):
        """x + token_mlp(norm1(x)^T)^T for an fp32 x outside the fused kernel's envelope.  `precision`: the setting (None = the default);
        P(param, name): the parameter as the fp32 kernels take it (the identity on the fp32 path, _p32 behind a 16-bit x)."""
        t = self.token_mlp
        p = F._prec(precision)
        T, N = t.fc1.weight.shape
        if p in (F.PREC_FP16, F.PREC_BF16) and T % 64 == 0 and x.shape[-1] % 4 == 0 and x.shape[-1] <= 1024:
            # channel-major on the 16-bit GEMM engine: LN(x)^T (B,C,NP) -> gelu(. W1^T + b1) (B,C,T) -> (. W2^T + b2)^T + x
            NP = -(-N // 64) * 64
            ut = F.layernorm16_t(x, P(self.norm1.weight, "norm1.weight"), P(self.norm1.bias, "norm1.bias"), self.norm1.eps, NP, p)
            ht = F.linear16(ut, F.weight16_padk(t.fc1.weight, NP, p), P(t.fc1.bias, "fc1.bias"), act=F.ACT_GELU, out16=True, precision=p)
            return F.linear16_tr(ht, F.weight16(t.fc2.weight, p), P(t.fc2.bias, "fc2.bias"), x, p)
        u = F.layernorm(x, P(self.norm1.weight, "norm1.weight"), P(self.norm1.bias, "norm1.bias"), self.norm1.eps)
        hid = F.token_mix(P(t.fc1.weight, "fc1.weight"), u, P(t.fc1.bias, "fc1.bias"), act=F.ACT_GELU, precision=precision)     # (B,T,C)
        return F.token_mix(P(t.fc2.weight, "fc2.weight"), hid, P(t.fc2.bias, "fc2.bias"), resid=x, precision=precision)         # (B,N,C)

    def _forward16(self, x):
        """The layer on an fp16 / bf16 x; the result has the type of x.  The MFMA operand format is that type (fp16: the precision-1
        arithmetic, bf16: precision 2) and a `precision` of None / 1 / 2 / 3 is ignored; precision 0 (explicit, the package default, or
        a strict re-run) widens x, runs the strict route and rounds.  x enters the arithmetic unrounded, the residual stream x1 behind the
        token mixing stays fp32, and y = fc2(..) + x1 is rounded once, in the epilogue of the last GEMM (an fp16 y beyond 65504 is what
        every 16-bit GEMM epilogue makes of it: reported to the range guard, code 3, so the module re-runs strict and returns inf).
        Inside the fused token kernel's envelope x is read in 16 bit by that kernel (mi355_mixer_token_x16_fwd); outside it (N != 196,
        C > 1024, ...) one launch widens x (widen16_kernel) and the fp32 routes run; the final store is 16-bit either way."""
        x, io = F._require_io16(x, "x")
        p = _io_precision(self.precision, io)
        t = self.token_mlp
        T, N = t.fc1.weight.shape
        if p and x.dim() == 3 and t.fc1.bias is not None and t.fc2.bias is not None and F.mixer_token_ok(N, T, x.shape[-1], p):
            x1 = F.mixer_token_mlp16(x, self.norm1, t.fc1, t.fc2)
        else:
            x1 = self._token_mix(F.widen16(x), p, _p32)
        return self._channel_mix(x1, p, _p32, x.dtype)

    def _channel_mix(self, x1, precision, P, out_dtype):
        """x1 + channel_mlp(norm2(x1)) for the fp32 stream x1, in out_dtype.  forward() passes the layer's setting, _same and fp32: the
        channel MLP is called as a module, at its own setting.  _forward16 passes the precision of its x (or 0), _p32 and the type of its
        x: on the fast GEMM widths fc2 stores that type in its own epilogue, else the fp32 MLP runs and one launch rounds."""
        c, n2 = self.channel_mlp, self.norm2
        fast, out16 = _fast(precision, c.fc1, c.fc2), out_dtype in _ffi.IO_CODES
        if fast and out16:
            p = F._prec(precision)
            return _half16(n2, "norm2", c.fc1, x1, p, lambda h: F.linear16(h, F.weight16(c.fc2.weight, p), _p32(c.fc2.bias, "fc2.bias"),
                                                                          resid=x1, out16=True, precision=p))
        u = _layernorm(n2, x1, P, "norm2", fast, precision)
        y = c(u, resid=x1) if P is _same else c._run(u, x1, precision, P)
        return F.round16(y, out_dtype) if out16 else y


class PatchEmbedding(nn.Module):
    """mlp_mixer.py:52-63 (the argument really is spelled `in_chanels` in the reference)."""

    def __init__(self, image_size, patch_size, in_chanels=3, embedding_dim=768):
        super().__init__()
        assert image_size % patch_size == 0
        self.patch_size = patch_size
        self.num_patches = (image_size // patch_size) ** 2
        self.proj = nn.Conv2d(in_chanels, embedding_dim, kernel_size=patch_size, stride=patch_size)
        self.precision = None

    _mi355_fp16_io_saturates = True          # fp16 tokens beyond 65504 are reported by the GEMM epilogue

    def forward(self, x):
        """x (B, Cin, H, W) fp32 -> fp32 tokens, or fp16 / bf16 -> tokens of that type (_patch_embed16)."""
        if _is16(x):
            return _patch_embed16(self, x)
        return F.patch_embed(x, self.proj.weight, self.proj.bias, None, None, self.patch_size, self.precision)


class MLP_Mixer(nn.Module):
    """Full MLP-Mixer (mlp_mixer.py:65-79): patch GEMM -> `depth` MixerLayers -> token mean -> head."""

    def __init__(self, dim=512, depth=12, image_size=224, patch_size=16, in_channels=3, drop=0, num_classes=1000, precision=None):
        super().__init__()
        self.patch_embedding = PatchEmbedding(image_size, patch_size, in_channels, dim)
        self.patch_embedding.precision = precision
        self.blocks = nn.Sequential(*[MixerLayer(dim, self.patch_embedding.num_patches, drop=drop, precision=precision)
                                      for _ in range(depth)])
        self.head = nn.Linear(dim, num_classes)
        self.precision = precision

    _mi355_fp16_io_saturates = True

    def forward(self, x):
        """fp32 image -> fp32 logits.  An fp16 / bf16 image runs the composition of the parts on 16-bit tensors -- embedding, every layer
        (16-bit in, 16-bit out), token mean (fp32 accumulation, fp32 pooled row), head -- and returns the logits in that type."""
        io16 = _is16(x)
        x = self.patch_embedding(x)
        for blk in self.blocks:
            x = blk(x)
        if io16:
            p = _io_precision(self.precision, _ffi.IO_CODES[x.dtype])
            logits = F.linear(F.token_mean16(x), _p32(self.head.weight, "head.weight"), _p32(self.head.bias, "head.bias"), precision=p)
            return logits.to(x.dtype)                # (B, classes): the one torch cast, not a pass over activations
        return F.linear(F.token_mean(x), self.head.weight, self.head.bias, precision=self.precision)
