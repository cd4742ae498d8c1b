"""GPU tests (-m gpu): the memory contract of the C ABI (include/mi355attn.h, "Conventions"), for every entry point.

Each row of tests/arena_cases.py runs three times:
  1. plain   ordinary tensors, stock workspaces; the result must pass assert_parity against the row's fp64 reference at the bar the
             existing tests use for the kernel family -- the anchor of everything below;
  2. arena   every input, parameter, output and workspace carved out of one 0xFF-poisoned buffer (tests/arena.py): pointers aligned
             to 16 bytes and no more, workspaces of exactly the declared size, NaN in every byte the call does not own.  Afterwards:
             every guard byte still 0xFF, every input bit-equal to its copy, every symbol of the row called and answered MI355_OK, the
             error words clean,
             the outputs torch.equal to the plain run (an over-read that leaks into a result shows here);
  3. junk    the arena run again with the workspaces pre-filled with 0x7F and then with zeros: the same bits, so "contents undefined
             on entry" really holds and nothing depends on 0xFF being a NaN.
A violation is reported by comparisons after the kernels have finished; no row is written to make a kernel fault.
"""
import copy
import ctypes

import pytest
import torch

import arena_cases
from arena import Arena, RecordingLib
from conftest import assert_parity

pytestmark = pytest.mark.gpu

ARENA_BYTES = 448 << 20
REFUSALS = {-1: "MI355_EINVAL", -2: "MI355_EUNSUPPORTED"}          # include/mi355attn.h


@pytest.fixture(scope="module")
def arena():
    from mi355attn import _ffi
    lib = _ffi.lib()

    def forget(ptr, nbytes):
        assert lib.mi355_workspace_forget(ctypes.c_void_p(ptr), nbytes) == 0
    a = Arena(ARENA_BYTES, torch.device("cuda", torch.cuda.current_device()), forget=forget)
    yield a
    forget(a.base, a.nbytes)


def _to_device(inp, put):
    """CPU inputs of a row -> the same structure on the device; every tensor, parameter and buffer goes through `put`."""
    out = {}
    for k, v in inp.items():
        if isinstance(v, torch.Tensor):
            out[k] = put(v, k)
        elif isinstance(v, torch.nn.Module):
            m = copy.deepcopy(v).to("cuda")
            for name, p in list(m.named_parameters()) + list(m.named_buffers()):
                p.data = put(p.data, f"{k}.{name}")
            out[k] = m
        else:
            out[k] = v
    return out


def _tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def _status_clean():
    from mi355attn import functional as F
    torch.cuda.synchronize()
    F.sync_status()
    F.range_status()


def _run(row, inp, put):
    import mi355attn
    from mi355attn import functional as F
    F._derived.clear()                       # derived copies of a previous run may live in memory the arena has handed out again
    old = mi355attn.default_precision()
    mi355attn.set_default_precision(row["prec"])
    try:
        with mi355attn.options(**row["opts"]), torch.no_grad():
            d = _to_device(inp, put)
            y = _tuple(row["run"](F, d))
            _status_clean()
    finally:
        mi355attn.set_default_precision(old)
        F._derived.clear()
    return y


def _arena_run(row, inp, arena, monkeypatch, ws_fill, trace=False):
    import mi355attn
    from mi355attn import _ffi
    from mi355attn import functional as F
    arena.reset(ws_fill=ws_fill)
    rec = RecordingLib(_ffi.lib())
    ws, ws_named, ws_dedicated = arena.workspace_hooks()
    tally = {}
    with monkeypatch.context() as mp:
        mp.setattr(F, "torch", arena.torch_proxy())
        mp.setattr(F, "workspace", ws)
        mp.setattr(_ffi, "workspace", ws)
        mp.setattr(_ffi, "workspace_named", ws_named)
        mp.setattr(_ffi, "workspace_dedicated", ws_dedicated)
        mp.setattr(F, "lib", lambda: rec)
        mp.setattr(_ffi, "lib", lambda: rec)
        try:
            if trace:
                out = {}

                def call():
                    out["y"] = _run(row, inp, lambda t, name: arena.place(t, name))
                for tag, count, *_ in mi355attn.kernel_trace(call):
                    tally[tag] = tally.get(tag, 0) + count
                y = out["y"]
            else:
                y = _run(row, inp, lambda t, name: arena.place(t, name))
        except mi355attn.Mi355Error as e:
            e.calls = list(rec.calls)                   # what the library answered, call by call: the test tells a refusal from a fault
            raise
    torch.cuda.synchronize()
    return y, rec.reached, tally


def _same(a, b, row, what):
    assert len(a) == len(b), f"{what}: {len(a)} outputs vs {len(b)}"
    for i, (u, v) in enumerate(zip(a, b)):
        if u is None or v is None:
            assert u is None and v is None, f"{what}: output {i} present in one run only"
            continue
        assert u.shape == v.shape and u.dtype == v.dtype, f"{what}: output {i} {u.shape} {u.dtype} vs {v.shape} {v.dtype}"
        if row["bits"]:
            bu, bv = u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)        # bit equality, also for NaN
            if not torch.equal(bu, bv):
                diff = (u.float() != v.float()) | (torch.isnan(u.float()) != torch.isnan(v.float()))
                idx = torch.nonzero(diff.reshape(-1)).reshape(-1)
                first = int(idx[0]) if idx.numel() else -1
                raise AssertionError(f"{what}: output {i} differs in {int(idx.numel())} of {u.numel()} elements, first at flat index "
                                     f"{first}: {u.reshape(-1)[first].item()!r} vs {v.reshape(-1)[first].item()!r}; "
                                     f"non-finite: {int((~torch.isfinite(v.float())).sum())}")
        else:
            assert_parity(v.float().cpu(), u.double().cpu(), row["tol"], f"{what}: output {i}")


@pytest.mark.parametrize("rid", [r["id"] for r in arena_cases.ROWS])
def test_entry_keeps_the_memory_contract(rid, arena, monkeypatch):
    import mi355attn
    row = arena_cases.BY_ID[rid]
    inp = row["make"](1234)
    refs = _tuple(row["ref"](inp))
    # 1. plain run, anchored to fp64
    plain = _run(row, inp, lambda t, name: t.to("cuda"))
    assert len(plain) == len(refs), f"{rid}: {len(plain)} outputs, {len(refs)} references"
    for i, (y, r) in enumerate(zip(plain, refs)):
        if r is not None:
            if row["tol"] == 0.0:
                assert torch.equal(y.cpu().double(), r.double()), f"{rid}: output {i} is not an exact copy"
            else:
                assert_parity(y.float().cpu(), r.reshape(y.shape).double(), row["tol"], f"{rid} plain run, output {i}")
    # 2. arena run
    trace = bool(row["tags"]) and torch.cuda.get_device_properties(0).multi_processor_count == 256
    try:
        got, reached, tally = _arena_run(row, inp, arena, monkeypatch, 0xFF, trace=trace)
    except mi355attn.Mi355Error as e:
        failed = [(s, rc) for s, rc in getattr(e, "calls", ()) if isinstance(rc, int) and rc < 0]       # the last one raised
        if not failed or failed[-1][1] not in REFUSALS:
            # an exchange time-out, a range report, a HIP error: the buffers were accepted, something else is wrong
            raise AssertionError(f"{rid}: the arena run failed, and not because an entry refused its buffers: {e}") from e
        assert row["refuses_at_16B"], (f"{rid}: {failed[-1][0]} refused 16-byte-aligned buffers of the declared size with "
                                       f"{REFUSALS[failed[-1][1]]}: {e}")
        arena.verify()                                   # a clean error: nothing written
        return
    assert not row["refuses_at_16B"], f"{rid}: marked refuses_at_16B but the call went through"
    missing = [s for s in row["entries"] if s not in reached]
    assert not missing, (f"{rid}: the row did not run {missing} to MI355_OK; the entries that returned 0: "
                         f"{sorted(c for c in reached if c.endswith('_fwd'))}")
    arena.verify()
    for tag in row["tags"] if trace else ():
        assert any(tag in t for t in tally), f"{rid}: no kernel tagged {tag!r} ran; tally {sorted(tally)}"
    if row["alignment_route"]:
        for i, (y, r) in enumerate(zip(got, refs)):
            if r is not None:
                assert_parity(y.float().cpu(), r.reshape(y.shape).double(), row["tol"], f"{rid} arena run, output {i}")
    else:
        _same(plain, got, row, f"{rid}: arena run vs plain run")
    # 3. junk runs: other workspace contents, the same bits
    for fill in (0x7F, 0x00):
        junk, _, _ = _arena_run(row, inp, arena, monkeypatch, fill)
        arena.verify()
        _same(got if row["bits"] else plain, junk, row, f"{rid}: workspace pre-filled with 0x{fill:02X} vs 0xFF")
