"""CPU tests of the ABI memory-contract harness: the arena's bookkeeping on CPU tensors, and that the row table of
tests/arena_cases.py covers every entry point of include/mi355attn.h and every kernel-selecting option of csrc/options.h."""
import os
import re

import pytest
import torch

from arena import ALIGN, MARGIN, PHASE, POISON, Arena, ArenaViolation, RecordingLib
from conftest import PKG, ROOT
from test_abi import _declared

SIZE = 2 * MARGIN + (1 << 20)


def _filled():
    a = Arena(SIZE, "cpu")
    x = a.place(torch.arange(1000, dtype=torch.float32).reshape(10, 100), "X")
    w = a.place(torch.ones(33, dtype=torch.float16), "W")
    y = a.place_empty((7, 5), torch.float32, "Y")
    ws = a.workspace(1000, "scratch")
    return a, x, w, y, ws


def test_placement_is_16_mod_256_and_disjoint():
    a, x, w, y, ws = _filled()
    z = a.torch_proxy().zeros(3, 4, dtype=torch.bfloat16, device="cpu")
    for t in (x, w, y, ws, z):
        assert t.data_ptr() % ALIGN == PHASE, hex(t.data_ptr())
    spans = sorted((r.off, r.end) for r in a.regions)
    assert spans[0][0] >= MARGIN and spans[-1][1] <= a.nbytes - MARGIN
    assert all(e0 + 256 <= s1 for (_, e0), (s1, _) in zip(spans, spans[1:])), spans
    assert ws.numel() == 1008 and bool((ws == POISON).all())            # the declared size rounded up to 16, poisoned
    assert bool((z == 0).all()) and torch.equal(x, torch.arange(1000, dtype=torch.float32).reshape(10, 100))
    assert torch.isnan(y).all()                                         # 0xFF is a NaN in fp32 (and in fp16 / bf16)
    assert torch.isnan(a.place_empty((4,), torch.float16)).all() and torch.isnan(a.place_empty((4,), torch.bfloat16)).all()


def test_untouched_arena_verifies_and_outputs_may_be_written():
    a, x, w, y, ws = _filled()
    y.fill_(1.0)
    ws.fill_(3)
    a.verify()


@pytest.mark.parametrize("where,text", [
    (lambda a, x, w, y, ws: a.buf[a.regions[0].off - 1:a.regions[0].off], "1 bytes before the start of input `X`"),
    (lambda a, x, w, y, ws: a.buf[a.regions[2].end + 16:a.regions[2].end + 17], "17 bytes past the end of output `Y`"),
    (lambda a, x, w, y, ws: a.buf[a.regions[1].off + 5:a.regions[1].off + 6], "byte 5 of input `W`"),
    (lambda a, x, w, y, ws: a.buf[a.regions[3].end:a.regions[3].end + 1], "1 bytes past the end of workspace `scratch`"),
    (lambda a, x, w, y, ws: a.buf[3:4], "bytes before the start of input `X`"),
    (lambda a, x, w, y, ws: a.buf[a.nbytes - 1:], "bytes past the end of workspace `scratch`"),
])
def test_one_planted_byte_is_caught_and_named(where, text):
    parts = _filled()
    parts[0].verify()
    where(*parts).fill_(0)
    with pytest.raises(ArenaViolation) as e:
        parts[0].verify()
    assert text in str(e.value), str(e.value)
    assert len(parts[0].violations()) == 1


def test_reset_forgets_then_poisons():
    seen = []
    a = Arena(SIZE, "cpu", forget=lambda ptr, n: seen.append((ptr, n)))
    a.place(torch.zeros(8), "X")
    a.reset(ws_fill=0x7F)
    assert seen == [(a.base, a.nbytes)] and not a.regions and bool((a.buf == POISON).all())
    assert bool((a.workspace(32) == 0x7F).all())
    a.verify()


def test_proxy_forwards_everything_else_to_torch():
    a = Arena(SIZE, "cpu")
    tp = a.torch_proxy()
    assert tp.float32 is torch.float32 and tp.nn is torch.nn and tp.cat is torch.cat
    e = tp.empty_like(torch.zeros(2, 3, dtype=torch.float16))
    assert e.shape == (2, 3) and e.dtype == torch.float16 and a.regions[-1].kind == "output"
    n = len(a.regions)
    tp.empty(4, device="meta")                                           # another device: torch's own allocator
    assert len(a.regions) == n
    assert tp.empty((2, 2), dtype=torch.int16, device="cpu").shape == (2, 2) and tp.zeros_like(e).dtype == torch.float16


def test_recorder_counts_calls_that_returned_ok_not_lookups():
    class Lib:
        version = 3

        @staticmethod
        def mi355_a_fwd(x):
            return 0

        @staticmethod
        def mi355_b_fwd(x):
            return -2                                                    # MI355_EUNSUPPORTED: a wrapper would fall back

        @staticmethod
        def mi355_c_fwd(x):
            return 0
    rec = RecordingLib(Lib)
    rec.mi355_c_fwd                                                      # looked up, never called
    assert rec.mi355_a_fwd(1) == 0 and rec.mi355_b_fwd(1) == -2 and rec.version == 3
    assert rec.reached == {"mi355_a_fwd"} and rec.calls == [("mi355_a_fwd", 0), ("mi355_b_fwd", -2)]


# ---- row-strided regions ------------------------------------------------------------------------------------------------------
def _strided():
    a = Arena(SIZE, "cpu")
    src = torch.arange(6 * 10, dtype=torch.float16).reshape(6, 10)
    x = a.place_rows(src, 24, "X")
    y = a.place_empty_rows(5, 7, 12, torch.float32, "Y")
    return a, src, x, y


def test_row_strided_regions_have_the_minimal_extent_and_poisoned_padding():
    a, src, x, y = _strided()
    rx, ry = a.regions
    assert (rx.kind, rx.nbytes) == ("input", (5 * 24 + 10) * 2) and (ry.kind, ry.nbytes) == ("output", (4 * 12 + 7) * 4)
    assert x.shape == (6, 10) and x.stride() == (24, 1) and y.shape == (5, 7) and y.stride() == (12, 1)
    assert x.data_ptr() == a.base + rx.off and y.data_ptr() == a.base + ry.off
    assert x.data_ptr() % ALIGN == PHASE and y.data_ptr() % ALIGN == PHASE
    assert torch.equal(x, src) and torch.isnan(y).all()
    # the padding behind every row but the last is POISON (a NaN in the region's type); behind the last row the guard begins
    flat = a.buf[rx.off:rx.end].view(torch.float16)
    assert flat.numel() == 5 * 24 + 10
    pad = flat[:5 * 24].view(5, 24)[:, 10:]
    assert torch.isnan(pad).all() and bool((pad.contiguous().view(torch.uint8) == POISON).all())
    assert bool((a.buf[ry.off:ry.end] == POISON).all()) and bool((a.buf[ry.end:ry.end + 256] == POISON).all())
    a.verify()
    y.fill_(2.0)                                                         # the live columns are the kernel's to write
    a.verify()
    assert bool((a.buf[ry.off:ry.off + 4 * 48].view(4, 48)[:, 28:] == POISON).all())
    with pytest.raises(ValueError):
        a.place_rows(src, 9)                                             # ld < width
    with pytest.raises(ValueError):
        a.place_empty_rows(3, 8, 7, torch.float32)
    one = a.place_empty_rows(1, 5, 100, torch.bfloat16, "one_row")      # one row: no padding at all
    assert a.regions[-1].nbytes == 10 and one.shape == (1, 5)
    a.verify()


def test_a_write_into_output_padding_is_reported_with_its_row_and_column():
    a, src, x, y = _strided()
    y.fill_(1.0)
    ry = a.regions[1]
    a.buf[ry.off + (2 * 12 + 9) * 4 + 1] = 0                            # row 2, column 9 (width 7), second byte of the element
    with pytest.raises(ArenaViolation) as e:
        a.verify()
    text = str(e.value)
    assert "output padding written: 1 byte(s)" in text and "output `Y`" in text and "row 2, column 9" in text and "padding behind width 7" in text
    assert len(a.violations()) == 1
    a.buf[ry.off + (0 * 12 + 7) * 4] = 3                                 # an earlier one: the FIRST is named
    assert "2 byte(s)" in a.violations()[0] and "row 0, column 7" in a.violations()[0]


def test_a_write_behind_the_last_row_of_a_strided_output_hits_the_guard():
    a, src, x, y = _strided()
    ry = a.regions[1]
    a.buf[ry.end] = 0                                                    # column `width` of the last row: not the caller's
    with pytest.raises(ArenaViolation, match="guard written: 1 byte.*1 bytes past the end of output `Y`"):
        a.verify()


def test_a_change_of_input_padding_or_of_a_live_input_element_is_reported():
    a, src, x, y = _strided()
    rx = a.regions[0]
    a.buf[rx.off + (3 * 24 + 17) * 2] = 0                                # row 3, column 17: padding of X
    with pytest.raises(ArenaViolation) as e:
        a.verify()
    assert "input modified: 1 byte(s)" in str(e.value) and "row 3, column 17: padding behind width 10" in str(e.value)
    a.buf[rx.off + (3 * 24 + 17) * 2] = POISON
    a.verify()
    x[4, 2] = 5.0
    with pytest.raises(ArenaViolation) as e:
        a.verify()
    assert "input modified" in str(e.value) and "row 4, column 2: live" in str(e.value)


# ---- coverage of the header and of the option table ---------------------------------------------------------------------------
def _device_entries():
    """Every header symbol that takes a device buffer: the forwards, the two stream helpers and the all-gather."""
    return sorted(n for n in _declared() if n.endswith("_fwd") or n in ("mi355_stream_copy", "mi355_stream_read", "mi355_allgather_f32",
                                                                       "mi355_mfma_yardstick"))


def test_every_header_entry_has_a_row_or_a_reason():
    import arena_cases
    covered = {s for r in arena_cases.ROWS for s in r["entries"]}
    header = set(_device_entries())
    stale = sorted((covered | set(arena_cases.EXEMPT)) - set(_declared()))
    assert not stale, f"named by a row or by EXEMPT but no longer in the header: {stale}"
    uncovered = sorted(header - covered - set(arena_cases.EXEMPT))
    assert not uncovered, f"header entries without a row in tests/arena_cases.py: {uncovered}"
    assert not covered & set(arena_cases.EXEMPT)


def test_exempt_holds_only_the_allowed_categories():
    import arena_cases
    api = open(os.path.join(PKG, "csrc", "api.hip")).read()
    covered = {s for r in arena_cases.ROWS for s in r["entries"]}
    for name, reason in arena_cases.EXEMPT.items():
        assert reason.strip(), name
        if name.startswith("mi355_comm_") or name in ("mi355_allgather_f32", "mi355_mfma_yardstick", "mi355_stream_read") \
                or name.startswith("mi355_event_time_"):
            continue
        # otherwise: an alias whose whole body is one forwarding call to a covered entry
        m = re.search(r"\b%s\s*\([^)]*\)\s*\{\s*return\s+(mi355_[a-z0-9_]+)\s*\([^;{}]*\)\s*;\s*\}" % re.escape(name), api, flags=re.S)
        assert m, f"{name} is exempt as an alias, but csrc/api.hip does not define it as a single forwarding call"
        assert m.group(1) in covered, f"{name} forwards to {m.group(1)}, which no row covers"
        line = api.count("\n", 0, m.start(1)) + 1                        # the line of the forwarding call: the reason must cite it
        assert f"csrc/api.hip:{line} forwards to {m.group(1)}" in reason, f"{name}: the forwarding call is at csrc/api.hip:{line}; reason: {reason!r}"


def _precisions_by_entry():
    """Header entry with an `int precision` parameter -> the precisions it takes.  The header's convention: 0, 1 or 2; an entry with a
    16-bit operand or result buffer (a `void*` parameter whose name carries "16") runs in that buffer's format, 1 or 2."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355attn.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(mi355_[a-z0-9_]+_fwd)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        if re.search(r"\bint\s+precision\b", m.group(2)):
            out[m.group(1)] = (1, 2) if re.search(r"\bvoid\s*\*\s*\w*16\w*", m.group(2)) else (0, 1, 2)
    return out


# entries without a 16-bit buffer in their prototype that the header still limits to the 16-bit modes, each with the header's words
PRECISION_1_2_ONLY = {
    "mi355_patch_embed_ws_fwd": "the im2col + 16-bit GEMM path: mi355_patch_embed_workspace_bytes is 0 in precision 0 (mi355_patch_embed_fwd runs)",
}


def test_every_precision_of_every_entry_has_a_row():
    import arena_cases
    takes = _precisions_by_entry()
    assert len(takes) >= 35 and takes["mi355_linear_fwd"] == (0, 1, 2) and takes["mi355_linear16_ws_fwd"] == (1, 2), takes
    assert set(PRECISION_1_2_ONLY) <= {n for n, p in takes.items() if p == (0, 1, 2)}
    have = {}
    for r in arena_cases.ROWS:
        for sym in r["entries"]:
            have.setdefault(sym, set()).add(r["prec"])
    missing = {}
    for sym, precs in takes.items():
        if sym in arena_cases.EXEMPT:
            continue
        want = {1, 2} if sym in PRECISION_1_2_ONLY else set(precs)
        if want - have.get(sym, set()):
            missing[sym] = sorted(want - have.get(sym, set()))
    assert not missing, f"entries with a precision parameter and no row at: {missing}"


def test_every_kernel_selecting_option_is_set_by_some_row():
    import arena_cases
    keys = re.findall(r'^MI355_OPT\(\w+,\s*"(\w+)"', open(os.path.join(PKG, "csrc", "options.h")).read(), flags=re.M)
    assert len(keys) >= 30
    used = {k for r in arena_cases.ROWS for k in r["opts"]}
    excluded = arena_cases.OPTIONS_NOT_COVERED
    assert set(excluded) <= {"chunk_images", "nt", "reverse", "spin_limit", "range_fallback", "vit_tail", "ws_persistent", "gemm_pa_block",
                             "gemm_pa_tail"} and all(excluded.values())
    assert not (used | set(excluded)) - set(keys), "an option named by a row or an exclusion is not in csrc/options.h"
    missing = sorted(set(keys) - used - set(excluded))
    assert not missing, f"options that select a kernel but are set by no row: {missing}"


def test_rows_are_well_formed():
    import arena_cases
    ids = [r["id"] for r in arena_cases.ROWS]
    assert len(ids) == len(set(ids)) and len(ids) > 300
    for r in arena_cases.ROWS:
        assert r["entries"] and all(s.startswith("mi355_") for s in r["entries"]), r["id"]
        assert r["prec"] in (0, 1, 2) and callable(r["make"]) and callable(r["run"]) and callable(r["ref"]), r["id"]
        assert r["tol"] in (0.0, 1e-5, 3e-5, 5e-5, 1e-3, 1.2e-2), (r["id"], r["tol"])        # bars the suite already uses, nothing new
        if r["bits"]:
            assert r["opts"].get("gemm_splitk", 0) == 0, r["id"]
    assert sum(1 for r in arena_cases.ROWS if not r["bits"]) >= 1 and all(r["opts"]["gemm_splitk"] == 1 for r in arena_cases.ROWS if not r["bits"])
    assert not [r["id"] for r in arena_cases.ROWS if r["refuses_at_16B"] or r["alignment_route"]], "update the header and DESIGN.md with the exception"
