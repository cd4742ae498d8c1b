"""CPU tests: the ATen-operator-sequence restatements bench.py times on the host (oracle/aten_seq.py) agree with the math restatements
of the oracle, and with the outputs of the reference modules they restate (same operators in the same order), recorded in
tests/golden/live/."""
import os

import numpy as np
import pytest
import torch

import oracle as O
from oracle import aten_seq as A
from conftest import ROOT, rel_fro


def _mods():
    from mi355attn.modules import (CBAM, Attention, DoubleAttention, ECALayer, MixerLayer, SELayer, TransformerEncoder, VisionTransformer,
                                   XCA, XCABlock)
    return dict(SELayer=SELayer, CBAM=CBAM, ECALayer=ECALayer, DoubleAttention=DoubleAttention, Attention=Attention,
                TransformerEncoder=TransformerEncoder, VisionTransformer=VisionTransformer, XCA=XCA, XCABlock=XCABlock, MixerLayer=MixerLayer)


def _sd(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


CASES = [
    # name, ctor, input shape, aten function, math-oracle function
    ("se", lambda M: M["SELayer"](64), (3, 64, 14, 10), lambda x, p: A.se_aten(x, p),
     lambda x, p: O.se_forward(x, p["fc.0.weight"], p["fc.2.weight"])),
    ("eca", lambda M: M["ECALayer"](64), (3, 64, 14, 10), lambda x, p: A.eca_aten(x, p), lambda x, p: O.eca_forward(x, p["conv.weight"])),
    ("cbam", lambda M: M["CBAM"](64), (3, 64, 14, 10), lambda x, p: A.cbam_aten(x, p),
     lambda x, p: O.cbam_forward(x, p["ca.fc.0.weight"], p["ca.fc.2.weight"], p["sa.conv.weight"])),
    ("da", lambda M: M["DoubleAttention"](64, 32, 32), (2, 64, 12, 12), lambda x, p: A.double_attention_aten(x, p),
     lambda x, p: O.double_attention_forward(x, *[p[k] for k in ("convA.weight", "convA.bias", "convB.weight", "convB.bias",
                                                                  "convV.weight", "convV.bias", "proj.weight", "proj.bias")])),
    ("vit_attn", lambda M: M["Attention"](192, 6), (2, 50, 192), lambda x, p: A.vit_attention_aten(x, p, 6),
     lambda x, p: O.vit_attention_forward(x, p, 6)),
    ("vit_enc", lambda M: M["TransformerEncoder"](192, 6), (2, 50, 192), lambda x, p: A.vit_encoder_aten(x, p, 6),
     lambda x, p: O.vit_encoder_forward(x, p, 6)),
    ("vit", lambda M: M["VisionTransformer"](image_size=32, patch_size=8, depths=2, num_heads=4, embedding_dim=64, num_classes=10),
     (2, 3, 32, 32), lambda x, p: A.vit_aten(x, p, 4, 2), lambda x, p: O.vit_forward(x, p, 4, 2)),
    ("xca", lambda M: M["XCA"](96, 4, qkv_bias=True), (2, 36, 96), lambda x, p: A.xca_aten(x, p, 4), lambda x, p: O.xca_forward(x, p, 4)),
    ("xca_block", lambda M: M["XCABlock"](96, 4, qkv_bias=True, eta=1.0), (2, 36, 96), lambda x, p: A.xca_block_aten(x, p, 4, 6, 6),
     lambda x, p: O.xca_block_forward(x, p, 4, 6, 6)),
    ("mixer", lambda M: M["MixerLayer"](64, 49), (2, 49, 64), lambda x, p: A.mixer_layer_aten(x, p), lambda x, p: O.mixer_layer_forward(x, p)),
]


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_aten_sequence_equals_math_restatement(name):
    _, ctor, shape, f_aten, f_math = next(c for c in CASES if c[0] == name)
    torch.manual_seed(1234)
    m = ctor(_mods()).eval()
    for k, v in m.state_dict().items():                        # non-trivial LayerNorm / BatchNorm / LayerScale parameters
        if v.dtype.is_floating_point and v.ndim == 1:
            v.copy_(v + 0.1 * torch.randn_like(v))
        if k.endswith("running_var"):
            v.copy_(v.abs() + 0.5)
    torch.manual_seed(4321)
    x = torch.randn(*shape)
    p = _sd(m)
    with torch.no_grad():
        ya, ym = f_aten(x, p), f_math(x, p)
    assert ya.shape == ym.shape
    assert rel_fro(ya, ym) <= 5e-6, name


LIVE = os.path.join(ROOT, "tests", "golden", "live")       # recorded from the reference by tests/golden/make_live_reference.py


def _close(got, want, scale):
    """fp64 checksums of float32 tensors drawn from the same seed: equal up to the last-bit differences of torch's vectorised CPU
    random kernels between host CPUs (~1e-9 relative); a different init stream or input would miss by orders of magnitude more."""
    return abs(got - want) <= 1e-6 * scale + 1e-12


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_aten_sequence_equals_live_reference(name):
    """Same operators in the same order as the reference module: agreement to fp32 rounding noise of the threaded kernels.  The
    reference module's output on the seeded input is recorded with checksums of its parameters and of that input; the drop-in module
    built under the same seed carries the same parameters (checked against the checksums), so f_aten runs on what the reference ran on."""
    _, ctor, shape, f_aten, _ = next(c for c in CASES if c[0] == name)
    rec = np.load(os.path.join(LIVE, "aten_%s.npz" % name))
    torch.manual_seed(1234)
    m = ctor(_mods()).eval()
    torch.manual_seed(4321)
    x = torch.randn(*shape)
    sd = _sd(m)
    assert list(sd) == [str(k) for k in rec["p_keys"]], name
    for k, s, sa in zip(sd, rec["p_sum"], rec["p_abs"]):
        v = sd[k].double()
        assert _close(float(v.sum()), s, sa) and _close(float(v.abs().sum()), sa, sa), (name, k)
    assert _close(float(x.double().sum()), float(rec["x_sum"]), float(x.double().abs().sum()))
    yr = torch.from_numpy(rec["y"])
    with torch.no_grad():
        ya = f_aten(x, sd)
    assert ya.shape == yr.shape
    assert rel_fro(ya, yr) <= 2e-6, name
