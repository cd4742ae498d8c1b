"""Every whole-model configuration of tests/model_cases.py against fp64, with non-trivial LayerNorm / bias / BatchNorm / LayerScale /
cls-token parameters.

Per row and precision (1 = fp16 default, 0 = strict, 2 = bf16):
  * the output matches the fp64 oracle at the bars of tests/test_routes_gpu.py (TOL);
  * the range fallback stayed silent (a strict re-run would hide the route under test);
  * precision 0 runs no 16-bit kernel, precision 1 / 2 show the row's tags (test_routes_gpu._check_route);
  * after the first forward, the row's cached parameters are rescaled in place and the re-run follows the oracle of the new state;
    then a second, differently seeded state dict is loaded (a trained checkpoint arriving after a warm-up) and followed too;
  * `error` rows: the drop-in refuses the configuration with the reference's exception type.
The golden cases run these models at default init only, where a dropped LayerNorm beta, a misplaced cls row or an undoubled
patch-token term leave the output unchanged.
"""
import importlib

import pytest
import torch

from conftest import assert_parity, rel_fro
from model_cases import BY_ID, ROWS, build_row, rescale_cached, second_state
from test_routes_gpu import TOL, _check_route, _run

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _cls(row):
    return getattr(importlib.import_module(row["mod"]), row["cls"])


def _oracle(row, stage, sd, x):
    """fp64 oracle of the row at `stage` ("base", "rescaled", "second"): each stage's state is the same at every precision."""
    key = (row["id"], stage)
    if key not in _ORACLE:
        _ORACLE[key] = row["oracle"](x, {k: v.detach().cpu() for k, v in sd.items()}, torch.float64).float()
    return _ORACLE[key]


def _check(row, prec, m, xd, ref, what):
    y, tags, fired = _run(m, xd, row.get("fwd_args", ()))
    assert not fired, f"{row['id']} p{prec} {what}: range fallback fired: {fired}"
    _check_route(row, prec, tags)
    assert_parity(y.cpu(), ref, TOL[prec], f"{row['id']} p{prec} {what} ({row['route']})")


@pytest.mark.parametrize("prec", [1, 0, 2])
@pytest.mark.parametrize("rid", [r["id"] for r in ROWS])
def test_model_matches_fp64(rid, prec):
    import mi355attn
    row = BY_ID[rid]
    assert mi355attn.get_option("range_fallback") == 1
    if "error" in row:
        with pytest.raises(row["error"]):
            build_row(row, _cls(row))
        return
    m, x = build_row(row, _cls(row))
    for sub in m.modules():
        if hasattr(sub, "precision"):
            sub.precision = prec
    ref = _oracle(row, "base", m.state_dict(), x)
    m = m.cuda()
    xd = x.cuda()
    with mi355attn.options(**row.get("options", {})):
        _check(row, prec, m, xd, ref, "first forward")
        if row["cached"]:
            # the model caches tensors derived from these parameters: rescale them in place, the result must follow
            rescale_cached(m, row["cached"])
            ref2 = _oracle(row, "rescaled", m.state_dict(), x)
            assert rel_fro(ref2, ref) > 10 * TOL[1], f"{rid}: the update of {row['cached']} does not move the output"
            _check(row, prec, m, xd, ref2, f"after an in-place update of {row['cached']}")
        sd3 = second_state(row, _cls(row))
        m.load_state_dict(sd3)
        ref3 = _oracle(row, "second", sd3, x)
        assert rel_fro(ref3, ref) > 10 * TOL[1], f"{rid}: the second state dict does not move the output"
        _check(row, prec, m, xd, ref3, "after load_state_dict of a second state")
