"""CPU guard of the whole-model table (tests/model_cases.py).

1. Every model class and public option listed in COVERAGE keeps a row: dropping one fails here.
2. The drop-in rebuilds each row's parameters and input to the checksums the reference recorded (tests/golden/live/models.npz,
   written by tests/golden/make_live_reference.py --models-only), and the fp64 oracle reproduces the reference's output at the
   bar of tests/test_routes_cpu.py.
3. `error` rows: the drop-in refuses the configuration with the exception type the reference raised.
4. Each row's in-place update of its cached parameters, and the second state dict, move the oracle's output well past the fp16 bar,
   so that tests/test_models_gpu.py would see a stale cache.
"""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_fro
from model_cases import BY_ID, ROWS, build_row, rescale_cached, second_state

FP16_BAR = 1e-3                 # tests/test_routes_gpu.py TOL[1]

COVERAGE = {
    ("VisionTransformer", "global_pool=token"), ("VisionTransformer", "global_pool=avg"), ("VisionTransformer", "global_pool=other"),
    ("VisionTransformer", "image size != image_size"), ("VisionTransformer", "num_heads=8"), ("VisionTransformer", "num_heads=4"),
    ("VisionTransformer", "ln_fold"), ("VisionTransformer", "qkv_bias"),
    ("CSWinTransformer", "num_classes>0"), ("CSWinTransformer", "num_classes=0"), ("CSWin_64_12211_tiny_224", "factory"),
    ("MLP_Mixer", "patch_size=16"), ("MLP_Mixer", "patch_size=32"), ("MLP_Mixer", "dim=256"),
    ("XCiT", "patch_size=16"), ("XCiT", "patch_size=8"), ("XCiT", "tokens_norm=False"), ("XCiT", "tokens_norm=True"),
    ("XCiT", "eta=1.0"), ("XCiT", "eta=1e-5"), ("XCiT", "eta=None"), ("XCiT", "cls_attn_layers=2"), ("XCiT", "cls_attn_layers=1"),
    ("XCiT", "use_pos=False"), ("XCiT", "qkv_bias=False"), ("XCiT", "num_classes=0"), ("xcit_nano_12_p16", "factory"),
    ("ClassAttentionBlock", "eta=1.0"), ("ClassAttentionBlock", "eta=None"), ("ClassAttentionBlock", "tokens_norm=False"),
    ("ClassAttentionBlock", "tokens_norm=True"), ("ClassAttentionBlock", "qkv_bias=False"), ("ClassAttentionBlock", "qk_scale"),
}
MODEL_CLASSES = {"VisionTransformer", "CSWinTransformer", "CSWin_64_12211_tiny_224", "MLP_Mixer", "XCiT", "xcit_nano_12_p16",
                 "ClassAttentionBlock"}


def _cls(row):
    return getattr(importlib.import_module(row["mod"]), row["cls"])


def _live_models():
    return np.load(os.path.join(ROOT, "tests", "golden", "live", "models.npz"))


def test_row_ids_are_unique_and_fields_complete():
    assert len(BY_ID) == len(ROWS)
    for r in ROWS:
        for k in ("mod", "cls", "shape", "oracle", "route", "tags", "absent", "cached", "covers"):
            assert k in r, f"{r['id']}: no {k}"
        assert r["cls"] in MODEL_CLASSES, r["id"]
        assert ("error" in r) == (r["oracle"] is None), r["id"]


def test_every_model_class_and_option_has_a_row():
    covered = {c for r in ROWS for c in r["covers"]}
    assert COVERAGE <= covered, f"no row for {sorted(COVERAGE - covered)}"
    assert {c for c, _ in covered} == MODEL_CLASSES


def test_live_models_record_covers_every_row():
    assert sorted(str(s) for s in _live_models()["ids"]) == sorted(r["id"] for r in ROWS)


def _record(rid):
    return {k.split("__", 1)[1]: v for k, v in _live_models().items() if k.startswith(rid + "__")}


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS if "error" in r])
def test_error_rows_raise_the_reference_exception(rid):
    row = BY_ID[rid]
    assert str(_record(rid)["error"]) == row["error"].__name__
    with pytest.raises(row["error"]):
        build_row(row, _cls(row))


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS if "error" not in r])
def test_oracle_vs_live_reference_model_rows(rid):
    from cases import sample_index
    row = BY_ID[rid]
    rec = _record(rid)
    m, x = build_row(row, _cls(row))
    sd = m.state_dict()
    assert [str(k) for k in rec["p_keys"]] == list(sd), "state_dict keys / order differ from the reference"
    assert np.allclose([float(v.double().sum()) for v in sd.values()], rec["p_sum"], rtol=1e-10, atol=1e-10), \
        "non-trivial parameters differ from the reference's"
    assert np.allclose([float(v.double().abs().sum()) for v in sd.values()], rec["p_abs"], rtol=1e-10, atol=1e-10)
    assert float(x.double().sum()) == pytest.approx(float(rec["x_sum"]), rel=1e-12, abs=1e-12)
    y = row["oracle"](x, sd, torch.float64)
    assert list(y.shape) == [int(s) for s in rec["y_shape"]]
    yf = y.reshape(-1)
    ref = torch.from_numpy(rec["y"]).double()
    got = yf if yf.numel() <= 257 else yf[sample_index(yf.numel())]
    assert got.shape == ref.shape
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= 1e-5 * scale, "output differs from the reference's"
    assert float(yf.abs().sum()) == pytest.approx(float(rec["y_abs"]), rel=1e-5)
    assert abs(float(yf.sum()) - float(rec["y_sum"])) <= 1e-5 * float(rec["y_abs"])


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS if "error" not in r])
def test_updates_move_the_output(rid):
    """fp32 oracle suffices: the moves are compared with 10x the fp16 bar."""
    row = BY_ID[rid]
    m, x = build_row(row, _cls(row))
    y = row["oracle"](x, m.state_dict(), torch.float32)
    if row["cached"]:
        rescale_cached(m, row["cached"])
        assert rel_fro(row["oracle"](x, m.state_dict(), torch.float32), y) > 10 * FP16_BAR, f"{rid}: {row['cached']}"
    assert rel_fro(row["oracle"](x, second_state(row, _cls(row)), torch.float32), y) > 10 * FP16_BAR
