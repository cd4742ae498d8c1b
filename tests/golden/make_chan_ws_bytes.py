#!/usr/bin/env python
"""Record the workspace sizes of the channel gates as a library built from a given commit reports them.

    python tests/golden/make_chan_ws_bytes.py --lib /path/to/libmi355attn.so --commit <hash the library was built from>

Writes tests/golden/chan_ws_bytes.json: for every shape of SHAPES the five sizes mi355_se_workspace_bytes, mi355_eca_workspace_bytes,
mi355_cbam_workspace_bytes, mi355_cbam16_workspace_bytes and mi355_chan_stat_workspace_bytes.  The sizes are host arithmetic, no GPU is
needed.  tests/test_chan_ws_layout_cpu.py compares the library under test against this record, so the record must come from a library
built BEFORE the change it is meant to pin (the committed one: 98f9291, the parent of the commit that moved the CBAM band geometry
and the workspace layout functions into shared headers), never from the tree under test.
"""
import argparse
import ctypes
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

# (B, C, H, W).  Bands of the single-read CBAM (at most 128 pixels, whole rows, a multiple of 4 pixels): 8x8 is one band of 16 pixel
# quads (segment width 16), 16x16 two bands of 32 quads (width 32), 14x14 seven bands at width 16, 56x56 28 bands at width 32; 3x5 and
# 7x7 have no band geometry (extra bytes 0).  C = 64 and 512 fill the last register slot of a lane at both widths, 100 and 400 do not.
SHAPES = [(B, C, H, W) for (H, W) in ((8, 8), (16, 16)) for C in (64, 100, 400, 512) for B in (1, 5)] + [
    (1, 64, 56, 56), (5, 100, 56, 56), (5, 400, 14, 14), (1, 64, 3, 5), (5, 100, 3, 5), (1, 512, 7, 7)]

ENTRIES = {"se": ("mi355_se_workspace_bytes", 4), "eca": ("mi355_eca_workspace_bytes", 4), "cbam": ("mi355_cbam_workspace_bytes", 4),
           "cbam16": ("mi355_cbam16_workspace_bytes", 4), "chan_stat": ("mi355_chan_stat_workspace_bytes", 2)}


def sizes(handle, B, C, H, W):
    """The five sizes of one shape from a loaded library (ctypes.CDLL)."""
    out = {}
    for key, (name, nargs) in ENTRIES.items():
        fn = getattr(handle, name)
        fn.restype = ctypes.c_size_t
        fn.argtypes = [ctypes.c_int] * nargs
        out[key] = int(fn(*(B, C, H, W)[:nargs]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libmi355attn.so built from the commit to record")
    ap.add_argument("--commit", required=True, help="that commit's hash (kept in the record)")
    args = ap.parse_args()
    handle = ctypes.CDLL(os.path.abspath(args.lib))
    rows = [dict(B=B, C=C, H=H, W=W, **sizes(handle, B, C, H, W)) for (B, C, H, W) in SHAPES]
    with open(os.path.join(HERE, "chan_ws_bytes.json"), "w") as f:
        json.dump({"commit": args.commit, "rows": rows}, f, indent=1)
        f.write("\n")
    print("wrote", len(rows), "rows")


if __name__ == "__main__":
    main()
