"""Every dispatch route of the transformer drop-ins against fp64, with non-trivial LayerNorm / bias / LayerScale parameters
(tests/route_cases.py).

Per row and precision (1 = fp16 default, 0 = strict, 2 = bf16):
  * the output matches the fp64 oracle at the bar of tests/test_ops_gpu.py (TOL);
  * precision 1 / 2: the kernel trace holds the row's tags and none of its absent ones, and the option-reading predicates (and the
    fp16 LayerScale fold decision) come out as claimed; precision 0: the trace shows the fp32 route and no 16-bit kernel;
  * the range fallback stayed silent (a strict re-run would hide the fast route);
  * rows whose route caches a parameter-derived tensor: the cached parameters are rescaled in place, and the re-run follows the oracle.
The golden cases run default init (LayerNorm gamma = 1, beta = 0, uniform LayerScales), where a dropped beta, a doubled gamma or
gamma1 in place of gamma3 leave the output unchanged; here each of them moves it by far more than the bar.
"""
import importlib
import warnings

import pytest
import torch

from conftest import assert_parity, rel_fro
from route_cases import BY_ID, ROWS, build_row, predicate_values

pytestmark = pytest.mark.gpu

TOL = {0: 5e-5, 1: 1e-3, 2: 1.2e-2}
STRICT_FORBIDDEN = ("gemm16", "io16", "out16", "in16", "cast16", "mlp_fused", "mlp_wide", "cswin_stripe", "mixer_token", "layernorm16_t",
                    "ln_center16")
_ORACLE = {}


def _oracle(row, sd, x):
    return row["oracle"](x, sd, torch.float64).float()


def _base_oracle(row, sd, x):
    if row["id"] not in _ORACLE:
        _ORACLE[row["id"]] = _oracle(row, sd, x)
    return _ORACLE[row["id"]]


def _built(row, p):
    cls = getattr(importlib.import_module(row["mod"]), row["cls"])
    m, x = build_row(row, cls)
    for sub in m.modules():
        if hasattr(sub, "precision"):
            sub.precision = p
    return m, x


def _run(m, x, fwd_args):
    """(output, kernel tags, range-fallback warnings) of one forward."""
    import mi355attn
    out = []
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            rows = mi355attn.kernel_trace(lambda: out.append(m(x, *fwd_args)))
        torch.cuda.synchronize()
    fired = [str(w.message) for w in rec if "overflowed" in str(w.message)]
    return out[0], [t for t, *_ in rows], fired


def _check_route(row, p, tags):
    if p == 0:
        bad = [t for t in tags if any(s in t for s in STRICT_FORBIDDEN)]
        assert not bad, f"{row['id']} p0: 16-bit kernels on the strict route: {bad}"
        assert any("prec 0" in t for t in tags), f"{row['id']} p0: no strict GEMM in {tags}"
        return
    for s in row["tags"]:
        assert any(s in t for t in tags), f"{row['id']} p{p} ({row['route']}): no '{s}' in {tags}"
    for s in row["absent"] + (row.get("absent_fp16", ()) if p == 1 else ()):
        hit = [t for t in tags if s in t]
        assert not hit, f"{row['id']} p{p} ({row['route']}): '{s}' ran: {hit}"


@pytest.mark.parametrize("prec", [1, 0, 2])
@pytest.mark.parametrize("rid", [r["id"] for r in ROWS])
def test_route_matches_fp64(rid, prec):
    import mi355attn
    from mi355attn import functional as F
    row = BY_ID[rid]
    assert mi355attn.get_option("range_fallback") == 1
    m, x = _built(row, prec)
    fwd_args = row.get("fwd_args", ())
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.cuda()
    xd = x.cuda()
    with mi355attn.options(**row.get("options", {})):
        if "error" in row:
            with pytest.raises(mi355attn.Mi355Error, match=row["error"]):
                with torch.no_grad():
                    m(xd, *fwd_args)
            return
        ref = _base_oracle(row, sd, x)
        if prec != 0:
            for name, v in predicate_values(row, m, prec).items():
                if name in row["claims"]:
                    assert (v() if callable(v) else v) == row["claims"][name], f"{rid} p{prec}: {name}"
            if "fold16" in row and prec == 1:
                folded = F.weight16_scaled(m.attn.proj.weight, m.attn.proj.bias, m.gamma1, prec) is not None
                assert folded == row["fold16"], f"{rid}: LayerScale fold decision {folded}"
        y, tags, fired = _run(m, xd, fwd_args)
        assert not fired, f"{rid} p{prec}: range fallback fired: {fired}"
        _check_route(row, prec, tags)
        assert_parity(y.cpu(), ref, TOL[prec], f"{rid} p{prec} ({row['route']})")
        if not row["cached"] or prec == 0:
            return
        # the route caches tensors derived from these parameters: rescale them in place, the result must follow
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for name in row["cached"]:
                t = m.get_parameter(name)
                t.mul_((0.6 + 0.8 * torch.rand(t.shape, generator=g)).to(t.device))
        sd2 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        ref2 = _oracle(row, sd2, x)
        assert rel_fro(ref2, ref) > 10 * TOL[1], f"{rid}: the update does not move the output"
        y2, tags2, fired2 = _run(m, xd, fwd_args)
        assert not fired2, f"{rid} p{prec} after the update: range fallback fired: {fired2}"
        _check_route(row, prec, tags2)
        assert_parity(y2.cpu(), ref2, TOL[prec], f"{rid} p{prec} after an in-place update of {row['cached']}")
