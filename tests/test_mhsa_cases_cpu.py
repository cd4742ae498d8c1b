"""CPU guard of the branch table of the multi-head attention copies (tests/mhsa_cases.py).

1. Table integrity: unique ids, complete fields, at least two rows for every class that mi355attn/modules/mhsa.py defines.
2. The fp64 oracle reproduces the reference's own classes at the rows' configurations with the rows' non-trivial parameters
   (tests/golden/live/mhsa.npz, recorded by tests/golden/make_live_reference.py --mhsa-only); the reference's outcome on the error
   rows is the recorded one.
3. Every row is sensitive to what it pins: each of its perturbations (H and W swapped, half-up pooled sizes, relative_pos dropped,
   norm.bias zeroed, BatchNorm statistics reset, qk_scale ignored, topk off by one, ...) moves the fp64 output by more than
   10 * 1e-3 rel-Frobenius -- ten times the default-precision bar the GPU test holds the row to.
4. KNN rows: at most 10 % of the tokens are left out as ambiguous, from the oracle alone.
"""
import importlib
import inspect
import os

import numpy as np
import pytest
import torch

from cases import flat_out, sample_index
from conftest import ROOT, rel_fro
from mhsa_cases import ALL_ROWS, BY_ID, ERROR_ROWS, KNN_MAX_AMBIGUOUS, ROWS, SENSITIVITY, build_row, knn_unambiguous

FIELDS = ("id", "mod", "cls", "args", "kwargs", "shape", "fwd_args", "oracle", "branch", "tags", "absent", "cached")
_BUILT = {}


def _cls(row):
    return getattr(importlib.import_module(row["mod"]), row["cls"])


def _built(rid):
    """(x, state_dict, fp64 oracle output) of a row, computed once and left unchanged."""
    if rid not in _BUILT:
        row = BY_ID[rid]
        m, x = build_row(row, _cls(row))
        sd = m.state_dict()
        _BUILT[rid] = (x, sd, row["oracle"](x, sd, torch.float64))
    return _BUILT[rid]


def test_row_ids_are_unique_and_fields_complete():
    assert len(BY_ID) == len(ALL_ROWS)
    for r in ALL_ROWS:
        for k in FIELDS:
            assert k in r, f"{r['id']}: no {k}"
        assert r["branch"], r["id"]
        assert r["shape"][0] <= 3, f"{r['id']}: batch > 3"
    for r in ROWS:
        assert "error" not in r and r["perturb"] and 1 <= len(r["perturb"]) <= 2, r["id"]
        assert any(t.startswith("sdpa_stream_kernel<d=") for t in r["tags"]), f"{r['id']}: no attention width tag"
        assert r["gemms"], r["id"]
    for r in ERROR_ROWS:
        assert r["error"] in ("RuntimeError", "ValueError", "TypeError", "Mi355Error"), r["id"]


def test_every_class_of_the_module_has_two_rows():
    from mi355attn.modules import mhsa
    classes = [c for _, c in inspect.getmembers(mhsa, inspect.isclass) if c.__module__ == mhsa.__name__ and issubclass(c, torch.nn.Module)]
    assert len(classes) == 10, [c.__name__ for c in classes]
    for c in classes:
        rows = [r["id"] for r in ROWS if _cls(r) is c]
        assert len(rows) >= 2, f"{c.__name__}: rows {rows}"
        assert any(_cls(r) is c for r in ERROR_ROWS), f"{c.__name__}: no error row"


# ---- the oracle against the reference ------------------------------------------------------------------------------------------
def _live():
    return np.load(os.path.join(ROOT, "tests", "golden", "live", "mhsa.npz"))


def test_live_record_covers_every_row():
    assert [str(s) for s in _live()["ids"]] == [r["id"] for r in ALL_ROWS]


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS])
def test_oracle_vs_live_reference(rid):
    rec = {k.split("__", 1)[1]: v for k, v in _live().items() if k.startswith(rid + "__")}
    x, sd, y = _built(rid)
    assert [str(k) for k in rec["p_keys"]] == list(sd), "state_dict keys / order differ from the reference"
    assert np.allclose([float(v.double().sum()) for v in sd.values()], rec["p_sum"], rtol=1e-10, atol=1e-10), \
        "non-trivial parameters differ from the reference's"
    assert np.allclose([float(v.double().abs().sum()) for v in sd.values()], rec["p_abs"], rtol=1e-10, atol=1e-10)
    assert float(x.double().sum()) == pytest.approx(float(rec["x_sum"]), rel=1e-12, abs=1e-12)
    y = flat_out(y)
    assert list(y.shape) == [int(s) for s in rec["y_shape"]]
    yf = y.reshape(-1)
    ref = torch.from_numpy(rec["y_samples"]).double()
    got = yf[sample_index(yf.numel())]
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= 1e-5 * scale, "strided samples differ from the reference"
    assert float(yf.abs().sum()) == pytest.approx(float(rec["y_abs"]), rel=1e-5)
    assert abs(float(yf.sum()) - float(rec["y_sum"])) <= 1e-5 * float(rec["y_abs"])


@pytest.mark.parametrize("rid", [r["id"] for r in ERROR_ROWS])
def test_reference_outcome_on_error_rows(rid):
    """What the reference does with the configuration the drop-in refuses (it runs: None) is the recorded one."""
    assert (str(_live()[rid + "__error"]) or None) == BY_ID[rid]["ref_raises"]


# ---- every row notices the slip it pins --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", [r["id"] for r in ROWS])
def test_row_is_sensitive_to_what_it_pins(rid):
    row = BY_ID[rid]
    x, sd, y = _built(rid)
    y = flat_out(y)
    for what, orc, edit in row["perturb"]:
        sd2 = {k: v.clone() for k, v in sd.items()}
        if edit is not None:
            edit(sd2)
        y2 = flat_out((orc or row["oracle"])(x, sd2, torch.float64))
        moved = rel_fro(y2, y)
        print(f"{rid}: {what}: {moved:.3e}")
        assert moved > SENSITIVITY, f"{rid}: '{what}' moves the output by {moved:.3e} only -- the wrong row for it"


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS if "knn" in r])
def test_knn_rows_leave_out_at_most_a_tenth(rid):
    row = BY_ID[rid]
    x, sd, _ = _built(rid)
    ok = knn_unambiguous(x, sd, *row["knn"])
    share = 1.0 - float(ok.float().mean())
    print(f"{rid}: {share:.2%} of the tokens are ambiguous")
    assert share <= KNN_MAX_AMBIGUOUS, f"{rid}: {share:.1%} of the tokens are ambiguous"
