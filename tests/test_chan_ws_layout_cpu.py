"""CPU test of the workspace sizes of the channel gates (SE, ECA, CBAM fp32 and 16-bit, the channel-statistics gates): they are what a
library built from the recorded commit reported (tests/golden/chan_ws_bytes.json, written by tests/golden/make_chan_ws_bytes.py from
THAT library, not from the code under test).  The sizes come from layout functions that several files share (csrc/common.h,
csrc/cbam_band.h); a caller sizes its buffer with them and the kernels carve it with them, so they may only change on purpose."""
import ctypes
import json
import os

import pytest

from conftest import ROOT

from make_chan_ws_bytes import ENTRIES, SHAPES, sizes

with open(os.path.join(ROOT, "tests", "golden", "chan_ws_bytes.json")) as f:
    RECORD = json.load(f)["rows"]


def _r16(n):
    return (n + 15) & ~15


def _multipass(B, C, H, W):
    """avg[B*C] | max[B*C] | smap[B*2*HW] of the multi-pass CBAM, each rounded to 16 bytes: the workspace without an exchange area."""
    return 2 * _r16(B * C * 4) + _r16(B * 2 * H * W * 4)


def test_the_record_covers_the_table():
    assert [(r["B"], r["C"], r["H"], r["W"]) for r in RECORD] == SHAPES
    assert all(set(ENTRIES) <= set(r) for r in RECORD)
    shapes = set(SHAPES)
    assert {B for B, _, _, _ in shapes} == {1, 5} and {C for _, C, _, _ in shapes} == {64, 100, 400, 512}
    extra = {(r["H"], r["W"]): r["cbam"] - _multipass(r["B"], r["C"], r["H"], r["W"]) for r in RECORD}
    assert extra[(3, 5)] == 0 and extra[(7, 7)] == 0                   # no band geometry: no exchange area
    assert all(extra[hw] > 0 for hw in ((8, 8), (16, 16), (14, 14), (56, 56)))


@pytest.mark.parametrize("row", RECORD, ids=lambda r: "B%d-C%d-%dx%d" % (r["B"], r["C"], r["H"], r["W"]))
def test_workspace_sizes_are_the_recorded_ones(built_lib, row):
    B, C, H, W = row["B"], row["C"], row["H"], row["W"]
    got = sizes(ctypes.CDLL(built_lib), B, C, H, W)
    assert got == {k: row[k] for k in ENTRIES}, (B, C, H, W)
    assert got["cbam16"] == got["cbam"] + _r16(B * H * W * 4)         # the 16-bit entry adds the fp32 spatial gate of its general form
