"""CPU checks of host-side pieces added in round 3: the Fourier position features in the engine's own closed form against samples
recorded from the real reference (tests/golden/fourier.json, made by tests/golden/make_fourier.py) and against whole feature maps
of the reference bit for bit (tests/golden/live/fourier.npz); dropout rates are accepted the way the reference accepts them."""
import json
import os

import pytest
import torch

from conftest import ROOT


def _features(H, W, hidden, temperature):
    from mi355attn.modules.xcit import PositionalEncodingFourier
    m = PositionalEncodingFourier(hidden_dim=hidden, dim=2 * hidden, temperature=temperature)
    return m.features(H, W)


def test_fourier_features_match_recorded_reference_samples():
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "fourier.json")))
    assert len(rec) >= 4
    for name, r in rec.items():
        f = _features(r["H"], r["W"], r["hidden"], r["temperature"]).reshape(-1)
        assert f.numel() == r["H"] * r["W"] * 2 * r["hidden"]
        got = f[torch.tensor(r["idx"])].double()
        assert torch.equal(got, torch.tensor(r["samples"], dtype=torch.float64)), f"{name}: samples differ from the reference"
        assert float(f.double().sum()) == r["sum"] and float(f.double().abs().sum()) == r["abssum"], name


def test_fourier_features_bit_identical_to_live_reference():
    """The whole feature maps of four grids, as the reference's own module computes them (identity 1x1 projection; recorded in
    tests/golden/live/fourier.npz by tests/golden/make_live_reference.py): equal bit for bit."""
    import numpy as np
    rec = np.load(os.path.join(ROOT, "tests", "golden", "live", "fourier.npz"))
    for H, W, hidden, temp in ((14, 14, 32, 10000), (5, 11, 8, 50), (1, 1, 4, 10000), (31, 2, 6, 1000)):
        ref = torch.from_numpy(rec["%dx%dx%dx%d" % (H, W, hidden, temp)])
        assert torch.equal(_features(H, W, hidden, temp), ref), (H, W, hidden, temp)


def test_dropout_rates_are_accepted_as_eval_identity():
    """A model built with its training configuration (attn_drop / proj_drop > 0) must construct; in eval mode nn.Dropout is the
    identity in the reference too.  Only the stochastic training-mode forward is refused (checked on the GPU suite's side as well)."""
    from mi355attn.modules import mhsa
    m = mhsa.Attention(64, num_heads=2, attn_drop=0.1, proj_drop=0.2)
    assert m.attn_drop.p == 0.1 and m.proj_drop.p == 0.2
    with pytest.raises(ValueError):
        mhsa.Attention(64, num_heads=2, attn_drop=1.5)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m(torch.randn(1, 4, 64))
