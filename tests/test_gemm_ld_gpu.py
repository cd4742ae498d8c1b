"""GPU tests (-m gpu): the row strides (ldx / ldy / ldu / lda) of every GEMM entry of include/mi355attn.h, against float64, inside the
poisoned arena of tests/arena.py.  The rows are tests/gemm_ld_cases.py: one per entry, kernel and epilogue, each called through the C ABI
with the options that force its kernel, once per stride pattern ("pad": the smallest stride above the width the header allows; "block":
column block 1 of a matrix three times as wide, X between live neighbours, Y between poisoned ones).

Per case:
  1. the entry answers MI355_OK and, on a 256-CU part, the row's kernel tag is in the trace of the call;
  2. the live columns match a float64 reference of the same operation at arena_cases.TOL[precision];
  3. the same call on dense operands (ld = width) runs the same kernel and returns the same bits in the live columns, statistics and U16
     included (split-K: compared at the tolerance instead);
  4. arena.verify(): no guard byte written, every input intact with its padding, every padding byte of the outputs still 0xFF;
  5. nothing non-finite in the live columns (the padding of the inputs is NaN: a read past column K would show).
Every comparison happens after the kernels have finished; no row is written to make a kernel fault.
"""
import pytest
import torch

import gemm_ld_cases as G
from conftest import assert_parity
from test_abi_memory_gpu import arena  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

_slot = {}                                  # (row id, precision) -> inputs, reference, dense run: shared by the patterns of a row, one at a time


def _place(arena, r, p, inp, ld, pattern):  # noqa: F811
    """Every buffer of the row carved from the arena: {name: view}."""
    views = {}
    for name, rows, width, dtype, key, role in G.buffers(r, p):
        if role == "in" and key is None:
            views[name] = arena.place(inp[name], name)
        elif role == "in" and pattern == "block" and name == "x":
            # column block 1 of a live matrix three times as wide: finite neighbours that must not enter the sums
            full = torch.randn(rows, 3 * width, generator=torch.Generator().manual_seed(99)).to(dtype)
            full[:, width:2 * width] = inp[name]
            views[name] = arena.place(full, name)[:, width:2 * width]
        elif role == "in":
            views[name] = arena.place_rows(inp[name], ld[key], name)
        elif key is None:
            views[name] = arena.place_empty((rows, width), dtype, name)
        else:
            views[name] = arena.place_empty_rows(rows, width, ld[key], dtype, name)
        assert views[name].shape == (rows, width) and views[name].stride() == (ld[key] if key else width, 1), name
    return views


def _run(arena, r, p, inp, pattern):  # noqa: F811
    """One call of the row inside the arena: (rc, error text, {output: live columns on the CPU}, sorted kernel tags)."""
    import mi355attn
    from mi355attn import _ffi
    from mi355attn import functional as F
    lib = _ffi.lib()
    arena.reset()
    ld = G.strides(r, p, pattern)
    views = _place(arena, r, p, inp, ld, pattern)
    P = {name: _ffi.dptr(v) for name, v in views.items()}
    st = _ffi.stream_ptr(arena.device)
    res = {}
    with mi355attn.options(**r["opts"]):
        ws, ws_bytes = None, 0
        if r["ws"]:
            ws_bytes = lib.mi355_linear16_workspace_bytes(*r["shape"])
            if torch.cuda.get_device_properties(0).multi_processor_count == 256:
                assert ws_bytes > 0, f"{r['id']}: the row is no split-K row on this part"
            if ws_bytes:
                ws = _ffi.dptr(arena.workspace(ws_bytes, "ws"))

        def call():
            res["rc"] = G.invoke(lib, r, p, P, ld, st, ws, ws_bytes)
        tally = mi355attn.kernel_trace(call)
        torch.cuda.synchronize()
    err = lib.mi355_last_error() if res["rc"] else b""
    if res["rc"] == 0:
        F.sync_status()
        F.range_status()
    outs = {name: views[name].clone().cpu() for name, rows, width, dtype, key, role in G.buffers(r, p) if role == "out"}
    return res["rc"], (err or b"").decode(), outs, sorted(t[0] for t in tally)


def _tags(want, p):
    return [t.replace("{p}", "f16" if p == 1 else "bf16").replace("{prec}", str(p)) for t in want]


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("case", G.CASES, ids=[G.case_id(c) for c in G.CASES])
def test_strided_rows_match_fp64_and_the_dense_call(case, arena):  # noqa: F811
    rid, p, pattern = case
    r = G.BY_ID[rid]
    cu256 = torch.cuda.get_device_properties(0).multi_processor_count == 256
    if (rid, p) not in _slot:
        _slot.clear()
        inp = G.make(r, p)
        ref = G.reference(r, p, inp, device="cuda" if r.get("ref_on_device") else "cpu")
        _slot[(rid, p)] = dict(inp=inp, ref=ref, dense=_run(arena, r, p, inp, "dense"))
        arena.verify()
    s = _slot[(rid, p)]
    d_rc, d_err, d_out, d_tags = s["dense"]
    assert d_rc == G.OK, f"{rid}: the dense call failed (code {d_rc}): {d_err}"

    rc, err, out, tags = _run(arena, r, p, s["inp"], pattern)
    # 1. return code and kernel
    assert rc == G.OK, f"{rid} {pattern} {G.strides(r, p, pattern)}: code {rc}: {err}"
    bad = []                                # every check runs; the failures are reported together, each under its number
    if cu256:
        for t in _tags(r["tags"], p):
            if not any(t in have for have in tags):
                bad.append(f"[1] no kernel tagged {t!r} ran; trace {tags}")
        if r["dense_tags"] is None:
            if tags != d_tags:
                bad.append(f"[3] the stride changed the kernel: {tags} vs dense {d_tags}")
        else:
            for t in _tags(r["dense_tags"], p):
                if not any(t in have for have in d_tags):
                    bad.append(f"[1] dense call: no kernel tagged {t!r} ran; trace {d_tags}")
    # 4. memory: guards, inputs with their padding, output padding
    bad += [f"[4] {v}" for v in arena.violations()]
    # 5. + 2. finite, and parity with float64 (the dense call as well: the anchor of check 3)
    for what, o in ((pattern, out), ("dense", d_out)):
        for name, t in o.items():
            n = int((~torch.isfinite(t.float())).sum()) if t.is_floating_point() else 0
            if n:
                bad.append(f"[5] {what}: {n} non-finite values in the live columns of {name}")
        got = G.values(r, o)
        for name, want in s["ref"].items():
            bar = G.TOL[r.get("tol_prec", {}).get(name, p)]
            try:
                rf, ma = assert_parity(got[name].double(), want.reshape(got[name].shape), bar, f"p{p} {what}: {name}")
                print(f"{rid} p{p} {what} {name}: rel_fro {rf:.3e} max_abs_ratio {ma:.3e} (tol {bar:g})")
            except AssertionError as e:
                bad.append(f"[2] {e}")
    # 3. independence of stride
    for name in out if r["bits"] else ():
        if not _bits_equal(out[name], d_out[name]):
            diff = torch.nonzero((out[name].contiguous().view(torch.uint8) != d_out[name].contiguous().view(torch.uint8)).reshape(out[name].shape[0], -1))
            bad.append(f"[3] {name} differs from the dense call's in {diff.shape[0]} bytes, first in row {int(diff[0, 0])}, byte "
                       f"{int(diff[0, 1])} of the row")
    assert not bad, f"{rid} p{p} {pattern} {G.strides(r, p, pattern)}:\n  " + "\n  ".join(bad)
