"""What the transformer drop-ins (vit.py, cswin.py, mixer.py, xcit.py) share on the host side: one fp32 body per module for fp32 and
16-bit input.

Every fp32 body of those files is written once, as `_run(.., precision, P)`.  forward() passes the module's setting and the parameters as
they are (_same); the callers behind a widened fp16 / bf16 x pass the resolved precision (_io_precision: the type of x, or 0) and _p32,
which hands 16-bit parameters (module.half() / .bfloat16()) over as their cached fp32 copies.  With P is _same a body calls its
sub-modules as modules (forward hooks fire, each resolves its own `precision`); behind a widened x it calls their `_run` at the one
resolved precision.
"""
import torch

from .. import _ffi
from .. import functional as F


def _is16(x):
    return isinstance(x, torch.Tensor) and x.dtype in _ffi.IO_CODES


def _same(t, name):
    return t


def _p32(t, name):
    """A parameter of a module that runs on 16-bit activations, as fp32: fp32 (autocast) as it is, 16-bit (module.half() / .bfloat16())
    through its cached fp32 copy (F.param32); None stays None."""
    return None if t is None else F.param32(t, name)


def _io_precision(precision, io):
    """The arithmetic of a module on a 16-bit tensor of type code `io`: the tensor's type, unless the setting (or a strict re-run) asks
    for precision 0."""
    return F.PREC_STRICT if F._prec(precision) == F.PREC_STRICT else io


def _wide(resid):
    """The residual of a widened 16-bit x as the fp32 body takes it: a 16-bit one widened, an fp32 one or None as it is."""
    return F.widen16(resid) if _is16(resid) else resid


class _Lin32:
    """A Linear as the fp32 routes behind a widened 16-bit x take it: its parameters as fp32 tensors (_p32), its feature counts."""

    def __init__(self, lin, name):
        self.weight, self.bias = _p32(lin.weight, name + ".weight"), _p32(lin.bias, name + ".bias")
        self.in_features, self.out_features = lin.in_features, lin.out_features


def _lin(lin, P, name):
    return lin if P is _same else _Lin32(lin, name)


class _LN32:
    """A LayerNorm as the fp32 routes behind a widened 16-bit x take it: its parameters as fp32 tensors (_p32), its eps."""

    def __init__(self, ln, name):
        self.weight, self.bias, self.eps = _p32(ln.weight, name + ".weight"), _p32(ln.bias, name + ".bias"), ln.eps


def _ln(ln, P, name):
    return ln if P is _same or ln is None else _LN32(ln, name)


def _layernorm(ln, x, P, name, to16=False, precision=None):
    """LayerNorm of an fp32 x with the parameters through P: fp32, or (to16) written in the MFMA operand format of `precision`."""
    w, b = P(ln.weight, name + ".weight"), P(ln.bias, name + ".bias")
    return F.layernorm16(x, w, b, ln.eps, F._prec(precision)) if to16 else F.layernorm(x, w, b, ln.eps)


def _round(y, dtype):
    """round16 of an fp32 result, or of the tensor part of a (tensor, other) pair."""
    return (F.round16(y[0], dtype),) + tuple(y[1:]) if isinstance(y, tuple) else F.round16(y, dtype)


def _fast(precision, *linears):
    """True when the 16-bit dataflow applies: a 16-bit operand mode and every GEMM inside the fast kernel's envelope."""
    return F._prec(precision) != F.PREC_STRICT and all(F.fast_gemm_ok(l.in_features, l.out_features) for l in linears)


def _mlp16(x, fc1, fc2, precision, second_gelu, gamma=None, resid=None):
    """fc1 -> GELU -> fc2 (-> GELU) with the hidden activation kept in the MFMA operand format; x is fp32 or 16-bit."""
    p = F._prec(precision)
    h16 = F.cast_linear16(x, F.weight16(fc1.weight, p), fc1.bias, act=F.ACT_GELU, precision=p)    # fp32 x: the cast rides in the GEMM where it can
    folded = F.weight16_scaled(fc2.weight, fc2.bias, gamma, p) if gamma is not None and not second_gelu else None
    if folded is not None:                                    # LayerScale folded into fc2 (XCiT: no activation behind fc2); None =
        w16, b = folded                                       # gamma * W would leave the fp16 normal range: gamma stays in the epilogue
        return F.linear16(h16, w16, b, resid=resid, precision=p)
    return F.linear16(h16, F.weight16(fc2.weight, p), fc2.bias, act=F.ACT_GELU if second_gelu else F.ACT_NONE, gamma=gamma,
                      resid=resid, precision=p)


def _mlp_run(fc1, fc2, x, resid, precision, P, second_gelu=False, gamma=None):
    """The fp32 body of every Mlp class: resid + gamma * (GELU?)(fc2(GELU(fc1(x)))) at `precision` (the setting; None = the default) with
    the parameters as P hands them over.  x is fp32, or the 16-bit LayerNorm output of a block on its 16-bit dataflow."""
    fc1, fc2 = _lin(fc1, P, "fc1"), _lin(fc2, P, "fc2")
    gamma = None if gamma is None else P(gamma, "gamma")
    if fc1.bias is not None and _fast(precision, fc1, fc2):
        return _mlp16(x, fc1, fc2, precision, second_gelu, gamma=gamma, resid=resid)
    h = F.linear(x, fc1.weight, fc1.bias, act=F.ACT_GELU, precision=precision)
    return F.linear(h, fc2.weight, fc2.bias, act=F.ACT_GELU if second_gelu else F.ACT_NONE, gamma=gamma, resid=resid,
                    precision=precision)


def _half16(ln, name, fc1, x1, p, last):
    """The second half of a block's 16-bit fast route on its fp32 stream x1: LayerNorm in the operand format p, fc1 + GELU with a 16-bit
    store, then last(h) -- the caller's fc2 GEMM, which adds x1 in fp32 and rounds the block's result once in its epilogue."""
    u = F.layernorm16(x1, _p32(ln.weight, name + ".weight"), _p32(ln.bias, name + ".bias"), ln.eps, p)
    return last(F.linear16(u, F.weight16(fc1.weight, p), _p32(fc1.bias, "fc1.bias"), act=F.ACT_GELU, out16=True, precision=p))


def _patch_embed16(mod, x):
    """A PatchEmbedding (ViT, MLP-Mixer) on an fp16 / bf16 image (B, Cin, H, W): tokens of that type.  The operand format is the type;
    precision 0 widens, runs the strict route and rounds; so does a geometry outside the envelope of mi355_patch_embed_x16_fwd, in the
    format of x."""
    w, b = mod.proj.weight, mod.proj.bias
    x, io = F._require_io16(x, "img")
    p = _io_precision(mod.precision, io)
    t = F.patch_embed16(x, w, b, mod.patch_size) if p else None
    if t is not None:
        return t
    t = F.patch_embed(F.widen16(x), _p32(w, "proj.weight"), _p32(b, "proj.bias"), None, None, mod.patch_size, p)
    return F.round16(t, x.dtype)
