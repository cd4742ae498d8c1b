"""CPU guard of the dispatch-route table (tests/route_cases.py).

1. Every row's claimed predicate values hold for its configuration at precision 1 and 2 (predicates that read a library option are
   checked by tests/test_routes_gpu.py, where the library runs).
2. Every `F.*_ok(` predicate and every `SDPA_WIDTHS` test that the four transformer module files consult is claimed true by some row and
   false by another: a dispatch predicate added later without rows fails here.
3. The fp64 oracle reproduces the reference modules' outputs at the rows' configurations with the rows' non-trivial parameters
   (tests/golden/live/routes.npz, recorded by tests/golden/make_live_reference.py).
"""
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from route_cases import BY_ID, ROWS, build_row, predicate_values

MODULE_FILES = ("vit.py", "cswin.py", "xcit.py", "mixer.py", "_io16.py")


class _OptionRead(Exception):
    pass


def _no_options(*_a, **_k):
    raise _OptionRead


def _cls(row):
    return getattr(importlib.import_module(row["mod"]), row["cls"])


def _claimed_values(row, monkeypatch, p):
    from mi355attn import _ffi
    from mi355attn import functional as F
    monkeypatch.setattr(F, "lib", _no_options)
    monkeypatch.setattr(_ffi, "get_option", _no_options)
    m, _ = build_row(row, _cls(row))
    got = {}
    for name, v in predicate_values(row, m, p).items():
        try:
            got[name] = v() if callable(v) else v
        except _OptionRead:
            got[name] = None                    # reads a library option: the GPU test checks it
    return got


def test_row_ids_are_unique_and_fields_complete():
    assert len(BY_ID) == len(ROWS)
    for r in ROWS:
        for k in ("mod", "cls", "shape", "oracle", "route", "tags", "absent", "claims", "cached"):
            assert k in r, f"{r['id']}: no {k}"
        assert r["claims"], r["id"]


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS])
def test_claimed_predicates_hold(rid, monkeypatch):
    row = BY_ID[rid]
    for p in (1, 2):
        got = _claimed_values(row, monkeypatch, p)
        for name, want in row["claims"].items():
            assert name in got, f"{rid}: claim {name} is not a predicate of {row['cls']}"
            if got[name] is not None:
                assert got[name] == want, f"{rid}: {name} is {got[name]} at precision {p}, the row claims {want}"


def _module_predicates():
    names = set()
    for f in MODULE_FILES:
        with open(os.path.join(PKG, "mi355attn", "modules", f)) as fh:
            src = fh.read()
        names |= set(re.findall(r"\bF\.(\w+_ok)\(", src))
        if re.search(r"\bF\.SDPA_WIDTHS\b", src):
            names.add("sdpa_widths")
    return names


def test_every_dispatch_predicate_is_claimed_both_ways():
    names = _module_predicates()
    assert {"cswin_stripe_ok", "ln_linear16_ok", "proj_mlp_fused_ok", "mlp_fused_ok", "mixer_token_ok", "fast_gemm_ok",
            "sdpa_widths"} <= names, names
    for n in sorted(names):
        seen = {r["claims"][n] for r in ROWS if n in r["claims"]}
        assert seen == {True, False}, f"predicate {n}: rows claim only {seen or 'nothing'} -- add a row for the other side"


def test_strict_precision_turns_every_16bit_predicate_off(monkeypatch):
    """Precision 0 must never pick a 16-bit route: every precision-taking predicate is false there."""
    for row in ROWS:
        got = _claimed_values(row, monkeypatch, 0)
        for name in ("cswin_stripe_ok", "ln_linear16_ok", "proj_mlp_fused_ok", "mlp_fused_ok", "mixer_token_ok", "ln_fold_ok"):
            if name in got:
                assert got[name] in (False, None), f"{row['id']}: {name} true at precision 0"


# ---- the oracle against the reference at the route configurations ----------------------------------------------------------
def _live_routes():
    return np.load(os.path.join(ROOT, "tests", "golden", "live", "routes.npz"))


def test_live_routes_record_covers_every_row():
    rec = _live_routes()
    assert sorted(str(s) for s in rec["ids"]) == sorted(r["id"] for r in ROWS)


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS])
def test_oracle_vs_live_reference_route_rows(rid):
    from cases import sample_index
    row = BY_ID[rid]
    rec = {k.split("__", 1)[1]: v for k, v in _live_routes().items() if k.startswith(rid + "__")}
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
    ref = torch.from_numpy(rec["y_samples"]).double()
    got = yf[sample_index(yf.numel())]
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= 1e-5 * scale, "strided samples differ from the reference"
    assert float(yf.abs().sum()) == pytest.approx(float(rec["y_abs"]), rel=1e-5)
    assert abs(float(yf.sum()) - float(rec["y_sum"])) <= 1e-5 * float(rec["y_abs"])
