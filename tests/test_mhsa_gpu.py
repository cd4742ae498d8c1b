"""Every branch of the multi-head attention copies (mi355attn/modules/mhsa.py) against fp64, with non-trivial bias / LayerNorm /
BatchNorm parameters (tests/mhsa_cases.py).

Per row and precision (1 = fp16 default, 0 = strict, 2 = bf16):
  * the output matches the fp64 oracle at the bar of tests/test_routes_gpu.py (TOL); KNNAttention rows on the tokens whose top-k
    selection is unambiguous in fp64 (mhsa_cases.knn_unambiguous); Broad_Attention on each of its four outputs;
  * the range fallback stayed silent (a strict re-run would hide the fast route);
  * the kernel trace holds the row's tags and none of its absent ones, and its GEMM launches are exactly the row's `gemms`: the
    attention kernel runs at the claimed width, and a row at a kernel width runs no second, padded GEMM;
  * rows that cache parameter-derived tensors (precision 1 and 2): the named parameters and buffers are rescaled in place, then a second
    state is loaded with load_state_dict; after each step the re-run follows the oracle.
One row per class also runs with a non-contiguous input, which must equal the dense run bit for bit, and the error rows raise exactly
what the table says at every precision, after which a valid forward on the same device still succeeds.
"""
import importlib
import re
import warnings

import pytest
import torch

from conftest import assert_parity, rel_fro
from mhsa_cases import BY_ID, ERROR_ROWS, ROWS, build_row, fwd_args, knn_unambiguous

pytestmark = pytest.mark.gpu

TOL = {0: 5e-5, 1: 1e-3, 2: 1.2e-2}            # tests/test_routes_gpu.py
NONCONTIGUOUS = ("attn_d48_padded", "pvt_sr2_rect", "cmt_sr2_relpos_rect", "seg_sr4_rect", "dilate_rect_qkscale", "bvit_identity_padded",
                 "eff_dq_gt_dv", "kvt_k7", "cvt_ks3_rect", "p2t_d40_qkscale")
_ORACLE = {}


def _cls(row):
    return getattr(importlib.import_module(row["mod"]), row["cls"])


def _tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def _oracle(row, sd, x):
    return tuple(t.float() for t in _tuple(row["oracle"](x, sd, torch.float64)))


def _base_oracle(row, sd, x):
    """The row's fp64 reference, computed once for the three precisions and left unchanged."""
    if row["id"] not in _ORACLE:
        _ORACLE[row["id"]] = _oracle(row, sd, x)
    return _ORACLE[row["id"]]


def _built(row, p, **kw):
    m, x = build_row(row, _cls(row), **kw)
    for sub in m.modules():
        if hasattr(sub, "precision"):
            sub.precision = p
    return m, x


def _cpu_state(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _run(m, x, args):
    """(outputs, [(kernel tag, launches)], range-fallback warnings) of one forward."""
    import mi355attn
    out = []
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            rows = mi355attn.kernel_trace(lambda: out.append(m(x, *args)))
        torch.cuda.synchronize()
    fired = [str(w.message) for w in rec if "overflowed" in str(w.message)]
    return _tuple(out[0]), [(t, n) for t, n, *_ in rows], fired


def _check_trace(row, p, trace):
    tags = [t for t, _ in trace]
    what = f"{row['id']} p{p} ({row['branch']})"
    for s in row["tags"]:
        assert any(s in t for t in tags), f"{what}: no '{s}' in {tags}"
    for s in row["absent"]:
        hit = [t for t in tags if s in t]
        assert not hit, f"{what}: '{s}' ran: {hit}"
    gemms = []
    for t, n in trace:
        g = re.search(r"\bN=(\d+) K=(\d+)", t)
        if g and t.startswith("gemm"):
            gemms += [(int(g.group(1)), int(g.group(2)))] * n
    assert tuple(sorted(gemms)) == tuple(row["gemms"]), f"{what}: GEMM launches (N, K) {sorted(gemms)}, the row states {row['gemms']}"


def _check_parity(row, p, ys, refs, x, sd, what):
    assert len(ys) == len(refs), f"{what}: {len(ys)} outputs, the oracle has {len(refs)}"
    keep = knn_unambiguous(x, sd, *row["knn"]) if "knn" in row else None
    for i, (y, r) in enumerate(zip(ys, refs)):
        y = y.cpu()
        assert tuple(y.shape) == tuple(r.shape), f"{what}: output {i} has shape {tuple(y.shape)}, the oracle {tuple(r.shape)}"
        if keep is not None:
            y, r = y[keep], r[keep]
        rf, ma = assert_parity(y, r, TOL[p], f"{what}, output {i}")
        print(f"{what}, output {i}: rel_fro {rf:.3e} max_abs_ratio {ma:.3e}")


@pytest.mark.parametrize("prec", [1, 0, 2])
@pytest.mark.parametrize("rid", [r["id"] for r in ROWS])
def test_branch_matches_fp64(rid, prec):
    import mi355attn
    row = BY_ID[rid]
    assert mi355attn.get_option("range_fallback") == 1
    m, x = _built(row, prec)
    sd = _cpu_state(m)
    m = m.cuda()
    xd = x.cuda()
    args = fwd_args(row, "cuda")
    what = f"{rid} p{prec} ({row['branch']})"
    ref = _base_oracle(row, sd, x)
    y, trace, fired = _run(m, xd, args)
    assert not fired, f"{what}: range fallback fired: {fired}"
    _check_trace(row, prec, trace)
    _check_parity(row, prec, y, ref, x, sd, what)
    if not row["cached"] or prec == 0:
        return
    # 1. the branch caches tensors derived from these parameters / buffers: rescale them in place, the result must follow
    g = torch.Generator().manual_seed(5)
    named = dict(m.named_parameters())
    with torch.no_grad():
        for name in row["cached"]:
            t = m.get_parameter(name) if name in named else m.get_buffer(name)
            t.mul_((0.6 + 0.8 * torch.rand(t.shape, generator=g)).to(t.device))
    sd2 = _cpu_state(m)
    ref2 = _oracle(row, sd2, x)
    moved = rel_fro(torch.cat([t.reshape(-1) for t in ref2]), torch.cat([t.reshape(-1) for t in ref]))
    assert moved > 10 * TOL[1], f"{rid}: the update moves the output by {moved:.3e} only"
    y2, trace2, fired2 = _run(m, xd, args)
    assert not fired2, f"{what} after the update: range fallback fired: {fired2}"
    _check_trace(row, prec, trace2)
    _check_parity(row, prec, y2, ref2, x, sd2, f"{what} after an in-place update of {row['cached']}")
    # 2. a second state loaded into the module that has already run
    m3, _ = build_row(row, _cls(row), weight_seed=2345, prep_seed=98)
    sd3 = {k: v.detach().clone() for k, v in m3.state_dict().items()}
    m.load_state_dict(sd3)
    ref3 = _oracle(row, sd3, x)
    y3, trace3, fired3 = _run(m, xd, args)
    assert not fired3, f"{what} after load_state_dict: range fallback fired: {fired3}"
    _check_trace(row, prec, trace3)
    _check_parity(row, prec, y3, ref3, x, sd3, f"{what} after load_state_dict")


@pytest.mark.parametrize("rid", NONCONTIGUOUS)
def test_noncontiguous_input_equals_dense(rid):
    row = BY_ID[rid]
    m, x = _built(row, 1)
    m = m.cuda()
    xd = x.cuda()
    args = fwd_args(row, "cuda")
    with torch.no_grad():
        dense = _tuple(m(xd, *args))
        C = xd.shape[-1]
        wide = torch.zeros(*xd.shape[:-1], C + 8, device="cuda")
        wide[..., 4:4 + C] = xd
        views = {"a slice of a wider tensor": wide[..., 4:4 + C], "a transposed-and-back view": xd.transpose(1, 2).contiguous().transpose(1, 2)}
        for name, xv in views.items():
            assert not xv.is_contiguous() and torch.equal(xv, xd)
            for i, (a, b) in enumerate(zip(_tuple(m(xv, *args)), dense)):
                assert torch.equal(a, b), f"{rid}: output {i} on {name} differs from the dense run"
    assert {_cls(BY_ID[r]) for r in NONCONTIGUOUS} == {_cls(r) for r in ROWS}, "one row per class"


@pytest.mark.parametrize("prec", [1, 0, 2])
@pytest.mark.parametrize("rid", [r["id"] for r in ERROR_ROWS])
def test_error_rows_raise_what_the_table_says(rid, prec):
    import mi355attn
    row = BY_ID[rid]
    want = {"Mi355Error": mi355attn.Mi355Error, "RuntimeError": RuntimeError, "ValueError": ValueError, "TypeError": TypeError}[row["error"]]
    m, x = _built(row, prec)
    m = m.cuda()
    with pytest.raises(want, match=row.get("match")) as ei:
        with torch.no_grad():
            m(x.cuda(), *fwd_args(row, "cuda"))
    assert ei.type is want, f"{rid} p{prec}: raised {ei.type.__name__}, the table says {row['error']}"
    # the device is still usable: a valid row runs and matches
    ok = BY_ID["attn_d32_nobias"]
    m2, x2 = _built(ok, prec)
    sd = _cpu_state(m2)
    with torch.no_grad():
        y = m2.cuda()(x2.cuda())
    torch.cuda.synchronize()
    assert_parity(y.cpu(), _base_oracle(ok, sd, x2)[0], TOL[prec], f"a valid forward after {rid} p{prec}")
