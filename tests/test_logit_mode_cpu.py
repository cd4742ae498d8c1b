"""Precision 3 ("logit-compensated"), the parts a CPU can check: the public constant and default-precision round trip, the pre-split qkv
weight, and WHY the mode exists -- an fp64 emulation of ViT `Attention(768, 12)` (ViT.py:79-89) with every 16-bit rounding point of the
engine's dataflow modelled, against the fp64 oracle:

  mode 1 (all fp16):  x, W_qkv -> fp16; q, k, v stored fp16; P -> fp16 (the row sum is the sum of the rounded P); ctx -> fp16; W_proj -> fp16
  mode 3:             the logit path -- x and the q / k rows of W_qkv as bf16 hi + lo, products hi.hi + hi.lo + lo.hi, q and k stored as
                      bf16 pairs, Q K^T as three products of the pairs -- and the value path exactly as in mode 1.

The fp32 accumulation of the MFMAs is not modelled (fp64 sums): its error is ~1e-6, two orders below what is measured here.  Emulated
mode 1 leaves the 1e-3 bar at weight scale 4 (logit std ~5) while emulated mode 3 stays inside it at every scale: the error that grows
with the logits is made on the logit path, the qkv GEMM's q / k columns included (profiles/logit_mode.md).
"""
import pytest
import torch

import oracle as O
from conftest import max_abs_ratio, rel_fro


def test_constant_and_default_round_trip():
    import mi355attn
    assert mi355attn.PREC_LOGIT == 3
    assert mi355attn.default_precision() == 1
    try:
        mi355attn.set_default_precision(3)
        assert mi355attn.default_precision() == 3
        from mi355attn import functional as F
        assert F._prec(None) == 1 and F._prec(3) == 1 and F.logit_mode(None) and F.logit_mode(3)      # 3 is 1 to everything but ViT attention
        assert not F.logit_mode(1) and F._prec(0) == 0 and F._prec(2) == 2
        with F._forced_strict():
            assert F._prec(3) == 0 and not F.logit_mode(3) and mi355attn.default_precision() == 0     # a strict re-run wins over 3
        for bad in (4, -1):
            with pytest.raises(ValueError):
                mi355attn.set_default_precision(bad)
        assert mi355attn.default_precision() == 3
    finally:
        mi355attn.set_default_precision(1)
    assert mi355attn.default_precision() == 1


def test_split_weight_parts():
    from mi355attn import functional as F
    torch.manual_seed(5)
    C = 128
    w = torch.nn.init.trunc_normal_(torch.empty(3 * C, C), std=.02) * 3.0
    hi, lo, v = F.split_qkv_weight(w)
    assert hi.dtype == lo.dtype == torch.bfloat16 and v.dtype == torch.float16
    assert tuple(hi.shape) == tuple(lo.shape) == (2 * C, C) and tuple(v.shape) == (C, C)
    back = hi.double() + lo.double()
    ref = w[:2 * C].double()
    nz = ref != 0
    assert float(((back - ref).abs()[nz] / ref.abs()[nz]).max()) <= 2.0 ** -16
    assert torch.equal(v, w[2 * C:].half())


# ---- the emulation ---------------------------------------------------------------------------------------------------------------
def _h(t):
    return t.float().half().double()


def _pair(t):
    """bf16 hi / lo parts of an fp32 tensor, as fp64."""
    t32 = t.float()
    hi = t32.to(torch.bfloat16)
    lo = (t32 - hi.float()).to(torch.bfloat16)
    return hi.double(), lo.double()


def _prod3(a, b):
    """a . b^T in the strict operand format: hi.hi + hi.lo + lo.hi of the bf16 pairs (lo.lo dropped), fp64 accumulate."""
    ah, al = _pair(a)
    bh, bl = _pair(b)
    return ah @ bh.transpose(-1, -2) + ah @ bl.transpose(-1, -2) + al @ bh.transpose(-1, -2)


def _emulate(x, sd, heads, mode):
    B, N, C = x.shape
    d = C // heads
    wq = sd["qkv.weight"]
    v = _h(_h(x) @ _h(wq[2 * C:]).t())                                   # value path: fp16 operands, v stored fp16 (both modes)
    if mode == 1:
        qk = _h(_h(x) @ _h(wq[:2 * C]).t())                              # q, k stored fp16
    else:
        qk = _prod3(x, wq[:2 * C])                                       # q, k at fp32 class; their pair storage is applied in _prod3 below
    out = torch.empty(B, N, C, dtype=torch.float64)
    for i in range(heads):
        q, k = qk[..., i * d:(i + 1) * d], qk[..., C + i * d:C + (i + 1) * d]
        s = q @ k.transpose(-1, -2) if mode == 1 else _prod3(q, k)
        s = s * d ** -0.5
        p = _h(torch.exp(s - s.amax(-1, keepdim=True)))                  # P rounded to fp16; the normaliser is the sum of the rounded values
        out[..., i * d:(i + 1) * d] = (p @ v[..., i * d:(i + 1) * d]) / p.sum(-1, keepdim=True)
    return _h(out) @ _h(sd["proj.weight"]).t() + sd["proj.bias"].double()


def _case(scale):
    torch.manual_seed(1234)
    C, heads = 768, 12
    sd = {"qkv.weight": torch.nn.init.trunc_normal_(torch.empty(3 * C, C), std=.02) * scale,
          "proj.weight": torch.nn.init.trunc_normal_(torch.empty(C, C), std=.02) * scale,
          "proj.bias": torch.zeros(C)}
    torch.manual_seed(4321)
    x = torch.randn(1, 197, C)
    return x, sd, heads


@pytest.mark.parametrize("scale", [1.0, 2.0, 3.0, 4.0])
def test_emulated_mode3_inside_bar(scale):
    x, sd, heads = _case(scale)
    ref = O.vit_attention_forward(x, sd, heads, dtype=torch.float64)
    y = _emulate(x, sd, heads, 3)
    rf, ma = rel_fro(y, ref), max_abs_ratio(y, ref)
    print("[logit-mode emulation] scale %.0fx mode 3: rel_fro %.2e max_abs %.2e" % (scale, rf, ma))
    assert rf <= 1e-3 and ma <= 1e-3, (scale, rf, ma)


def test_emulated_mode1_outside_bar_at_scale_4():
    x, sd, heads = _case(4.0)
    ref = O.vit_attention_forward(x, sd, heads, dtype=torch.float64)
    y = _emulate(x, sd, heads, 1)
    rf, ma = rel_fro(y, ref), max_abs_ratio(y, ref)
    print("[logit-mode emulation] scale 4x mode 1: rel_fro %.2e max_abs %.2e" % (rf, ma))
    assert rf > 1e-3 or ma > 1e-3, (rf, ma)
