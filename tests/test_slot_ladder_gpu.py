"""GPU tests (-m gpu): every template instantiation of the single-read channel gates -- SE, ECA, CBAM, SimAM, SRM, GaussianGCT, LCT, GCT
in fp32, fp16 and bf16 -- against the fp64 oracle, slot count by slot count.

The cases come from tests/slot_cases.py (derived from a restatement of the host's choice that tests/test_slot_cases_cpu.py pins to the
source and to the built library).  Per case:
  * the module runs twice on the `spread` and on the `planted` input: bit-equal runs, and every element within the bar the existing
    tests of that module use -- assert_parity 1e-5 (SE, ECA, CBAM) / 2e-5 (statistics gates) as in tests/test_chan_attn_gpu.py,
    io16_common._check_chan for fp16 / bf16 -- against the oracle in fp64;
  * the kernel trace of the call is exactly the tag `choice` predicts, which names the template arguments; over a test function the
    instantiations seen are the ones slot_cases.reachable lists, measured, for that operator and I/O type;
  * the same input through the general form (single read switched off) stays within 1e-6 (SE, ECA) / 2e-6 (CBAM, statistics gates) of
    the single-read result, one ulp of the I/O type for 16-bit activations (tests/test_chan_attn_gpu.py, tests/test_io16_gpu.py);
  * `place` (SE, ECA, CBAM, GCT): through the C entry into an output buffer of NaNs, the result is the stated power of two times a ramp
    of distinct values, bit for bit.
In the bucket above 4 chunks per lane a batch with more slices than resident workgroups repeats a judged three-image batch and must
reproduce it bit for bit."""
import ctypes

import pytest
import torch

import slot_cases as S
from conftest import assert_parity
from io16_common import _check_chan, _run, _status, _ulps

pytestmark = pytest.mark.gpu

PAIRS = [(op, io) for op in S.OPS for io in S.IOS]


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count     # resident_slots(n) = this * n (csrc/api.hip)


def _load(param, value):
    with torch.no_grad():
        param.copy_(value.reshape(param.shape))


def _module(c, p):
    """The drop-in module of case c with parameters p, on the device."""
    from mi355attn import modules as M
    if c.op == "se" and c.extra == "bias":
        m = M.SELayerBias(c.C, c.C // c.Cr)
        for t, k in ((m.fc[0].weight, "w1"), (m.fc[0].bias, "b1"), (m.fc[2].weight, "w2"), (m.fc[2].bias, "b2")):
            _load(t, p[k])
    elif c.op == "se" and c.extra == "hsig":
        m = M.SqueezeExcite(c.C)
        for t, k in ((m.conv_reduce.weight, "w1"), (m.conv_reduce.bias, "b1"), (m.conv_expand.weight, "w2"), (m.conv_expand.bias, "b2")):
            _load(t, p[k])
    elif c.op == "se":
        m = M.SELayer(c.C, c.C // c.Cr)
        _load(m.fc[0].weight, p["w1"])
        _load(m.fc[2].weight, p["w2"])
    elif c.op == "eca":
        m = M.ECALayer(c.C)
        _load(m.conv.weight, p["taps"])
    elif c.op == "cbam":
        m = M.CBAM(c.C, 16, c.ks)
        for t, k in ((m.ca.fc[0].weight, "w1"), (m.ca.fc[2].weight, "w2"), (m.sa.conv.weight, "wconv")):
            _load(t, p[k])
    elif c.op == "simam":
        m = M.simam_module()
    elif c.op == "srm":
        m = M.SRM(c.C)
        for t, k in ((m.cfc.weight, "cfc"), (m.bn.weight, "bn_w"), (m.bn.bias, "bn_b"), (m.bn.running_mean, "bn_mean"), (m.bn.running_var, "bn_var")):
            _load(t, p[k])
    elif c.op == "gctg":
        m = M.GaussianGCT(c.C)
    elif c.op == "lct":
        m = M.LCT(c.C, S.LCT_GROUPS)
        _load(m.w, p["w"])
        _load(m.b, p["b"])
    else:
        m = M.GCT(c.C, mode="l2" if c.op == "gct_l2" else "l1")
        for k in ("alpha", "gamma", "beta"):
            _load(getattr(m, k), p[k])
    return m.eval().cuda()


def _judge(c, y, ref, what):
    if c.io == "fp32":
        rf, ma = assert_parity(y.cpu(), ref, S.TOL32[c.op], what)
        print(f"[slots] {what}: rel_fro {rf:.2e} max_abs_ratio {ma:.2e} (bar {S.TOL32[c.op]:g})")
    else:
        _check_chan(y, ref, c.dtype, what)


def _forward(m, xd):
    with torch.no_grad():
        return m(xd)


@pytest.mark.parametrize("op,io", PAIRS)
def test_every_instantiation_vs_fp64_oracle(op, io, cus, monkeypatch):
    import mi355attn
    monkeypatch.setenv("MI355_CHECK_SYNC", "1")                         # every forward waits and reads the exchange kernels' error word
    general = {S.SINGLE_OPTION.get(op, "zoo_single"): 0}
    seen = set()
    for c in S.cases(op, io):
        want = c.choice(cus)
        assert want is not None, c.id
        p = S.case_params(c)
        m = _module(c, p)
        with mi355attn.options(**c.options):
            for kind in ("spread", "planted"):
                x = S.make_input(c, kind)
                xd = x.cuda()
                y, tags = _run(m, xd)
                assert tags == [want.tag], (c.id, kind, tags, want.tag)
                seen.add(S.inst_of_tag(tags[0]))
                assert torch.equal(y, _forward(m, xd)), f"{c.id} {kind}: two runs differ"
                _judge(c, y, S.oracle(c, x, p), f"{c.id} {kind}")
            with mi355attn.options(**general):
                y0, tags0 = _run(m, xd)
            assert not any(S.inst_of_tag(t) for t in tags0), (c.id, tags0)
            if io == "fp32":
                assert_parity(y.cpu(), y0.cpu(), S.TOL32_GENERAL[op], f"{c.id}: single read vs general form")
            else:
                d = _ulps(y, y0)
                assert d <= 1, f"{c.id}: single read and general form differ by {d} ulps"
    want_all = S.reachable(op, io, cus)
    print(f"[slots] {op} {io}: {len(seen)} instantiations seen in the trace, {len(want_all)} reachable")
    assert seen == want_all, sorted(seen ^ want_all)
    _status()


# ---- place: the C entry writes every element of a NaN-filled output, each into its own place ---------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _entry(lib, c, xd, p, y, ws):
    """Call the C entry of case c's operator (fp32 or 16-bit) on caller-owned buffers."""
    from mi355attn._ffi import stream_ptr
    Bn, C, H, W = c.shape
    io = (S.IO_CODE[c.io],) if c.io != "fp32" else ()
    tail = (*io, _p(ws), ws.numel(), stream_ptr(xd.device))
    x16 = "16" if io else ""
    if c.op == "se":
        rc = getattr(lib, f"mi355_se{x16}_fwd")(_p(xd), _p(p["w1"]), _p(p["w2"]), _p(y), Bn, C, c.Cr, H, W, *tail)
    elif c.op == "eca":
        rc = getattr(lib, f"mi355_eca{x16}_fwd")(_p(xd), _p(p["taps"]), _p(y), Bn, C, c.ks, H, W, *tail)
    elif c.op == "cbam":
        rc = getattr(lib, f"mi355_cbam{x16}_fwd")(_p(xd), _p(p["w1"]), _p(p["w2"]), _p(p["wconv"]), _p(y), Bn, C, c.Cr, c.ks, H, W, 0, *tail)
    else:
        rc = getattr(lib, f"mi355_gct{x16}_fwd")(_p(xd), _p(p["alpha"]), _p(p["gamma"]), _p(p["beta"]), _p(y), Bn, C, H, W, 1e-5, 0, 0, *tail)
    assert rc == 0, (c.id, lib.mi355_last_error())


def _ws_bytes(lib, c):
    Bn, C, H, W = c.shape
    if c.op == "se":
        return lib.mi355_se_workspace_bytes(Bn, C, H, W)
    if c.op == "eca":
        return lib.mi355_eca_workspace_bytes(Bn, C, H, W)
    if c.op == "cbam":
        return (lib.mi355_cbam_workspace_bytes if c.io == "fp32" else lib.mi355_cbam16_workspace_bytes)(Bn, C, H, W)
    return lib.mi355_chan_stat_workspace_bytes(Bn, C)


@pytest.mark.parametrize("io", S.IOS)
@pytest.mark.parametrize("op", S.PLACE_OPS)
def test_every_element_lands_in_its_place(op, io, cus):
    import mi355attn
    from mi355attn._ffi import lib as _lib
    lib = _lib()
    bits = torch.int32 if io == "fp32" else torch.int16
    held = []
    try:
        for c in S.cases(op, io):
            if c.extra or c.opts:
                continue
            want = c.choice(cus)
            x = S.make_input(c, "place")
            xd = x.cuda()
            p = {k: v.contiguous().cuda() for k, v in S.place_params(c).items()}
            y = torch.full_like(xd, float("nan"))
            ws = torch.zeros(max(16, _ws_bytes(lib, c)), dtype=torch.uint8, device="cuda")
            held.append(ws)
            rows = mi355attn.kernel_trace(lambda: _entry(lib, c, xd, p, y, ws))
            assert [r[0] for r in rows] == [want.tag], (c.id, rows)
            expect = (x.double() * S.PLACE_GATE[op]).to(c.dtype)
            got = y.cpu()
            assert not torch.isnan(got).any(), f"{c.id}: {int(torch.isnan(got).sum())} elements were never written"
            assert torch.equal(got.view(bits), expect.view(bits)), \
                f"{c.id}: {int((got.view(bits) != expect.view(bits)).sum())} elements differ from {S.PLACE_GATE[op]} x"
        torch.cuda.synchronize()
        assert lib.mi355_sync_status() == 0, lib.mi355_last_error()
    finally:
        torch.cuda.synchronize()
        for t in held:                                                  # before the buffers are freed (include/mi355attn.h, "ws_persistent")
            lib.mi355_workspace_forget(_p(t), t.numel())


# ---- more slices than resident workgroups ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,io", [pr for pr in PAIRS if pr[0] != "cbam"])
def test_more_slices_than_resident_workgroups(op, io, cus, monkeypatch):
    """3 * CUs / (C / 8) + 1 images at nv = 7 (fp32) / 6 (16-bit): more slices than the grid has workgroups (three per CU at most), so
    workgroups go round their slice loop again.  The batch repeats the case's three `planted` images, which the oracle judges here once;
    every image of the long batch must equal its original bit for bit."""
    monkeypatch.setenv("MI355_CHECK_SYNC", "1")
    base, n = S.many_slices_case(op, io, cus)
    want = base.choice(cus)
    assert want.nv == (7 if io == "fp32" else 6) and want.NV in (7, 8)
    slices = n * (base.C // S.ECW)
    assert want.wg_per_cu <= 3 and slices > 3 * cus
    p = S.case_params(base)
    m = _module(base, p)
    x3 = S.make_input(base, "planted")
    y3, tags3 = _run(m, x3.cuda())
    _judge(base, y3, S.oracle(base, x3, p), f"{base.id} planted (three images)")
    xb = x3.repeat((n + 2) // 3, 1, 1, 1)[:n].contiguous().cuda()
    yb, tagsb = _run(m, xb)
    assert tags3 == tagsb == [want.tag], (tags3, tagsb, want.tag)
    assert torch.equal(yb[:3], y3) and torch.equal(yb[-3:], y3[[(n - 3 + i) % 3 for i in range(3)]]), f"{base.id}: first / last images differ"
    assert torch.equal(yb, y3.repeat((n + 2) // 3, 1, 1, 1)[:n]), f"{base.id}: an image of the long batch differs from its original"
    _status()
