#!/usr/bin/env python
"""Time the residual (+ ReLU) epilogue of SELayer / ECALayer / CBAM against the three lines a user writes without it.

    python tools/gate_resid_bench.py [--shape 256 256 56 56] [--rounds 9] [--iters 20] [--json out.json]

The protocol of tools/io16_bench.py: one process, one device, all variants interleaved round by round (a round times every variant
once, `iters` calls between two events), so drift hits every variant alike.  Per gate and I/O type (fp32, fp16, bf16):
    row 1   m(x, resid=r, relu=True)         the residual epilogue: 2 reads + 1 write of the map
    row 1m  the same, *_single options off   its multi-pass form
    row 2   y = m(x); y += r; y.relu_()      what a user writes today: 7 passes over the map
    row 3   m(x)                             the unchanged plain kernel, for scale: 1 read + 1 write
Prints a markdown table (median, min .. max over the rounds, achieved GB/s at the row's algorithmic bytes), the two targets per gate
and type as met / NOT met, and one JSON line:
    target A   row 1 below row 2 with min .. max ranges that do not overlap
    target B   row 1 median not above 3/2 of row 3's median plus the spread (max - min) of row 3 (3/2: the ratio of their bytes)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-attention_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from io16_bench import SINGLE_OPTS, time_variants  # noqa: E402

PASSES = {"1": 3, "1m": 3, "2": 7, "3": 2}                             # algorithmic passes over the map


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[256, 256, 56, 56])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import mi355attn
    from mi355attn.modules import CBAM, ECALayer, SELayer
    B, C, H, W = a.shape
    torch.manual_seed(1234)
    mods = {"SE": SELayer(C).eval().cuda(), "ECA": ECALayer(C).eval().cuda(), "CBAM": CBAM(C).eval().cuda()}
    torch.manual_seed(4321)
    x32 = torch.randn(B, C, H, W, device="cuda")
    r32 = torch.randn(B, C, H, W, device="cuda")

    def multi(m, x, r):
        with mi355attn.options(**{k: 0 for k in SINGLE_OPTS}):
            return m(x, resid=r, relu=True)

    def today(m, x, r):
        y = m(x)
        y += r
        return y.relu_()

    variants = []
    for dt, tag in ((torch.float32, "fp32"), (torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        x, r = x32.to(dt), r32.to(dt)
        for name, m in mods.items():
            variants.append(((name, tag, "1"), lambda m=m, x=x, r=r: m(x, resid=r, relu=True)))
            variants.append(((name, tag, "1m"), lambda m=m, x=x, r=r: multi(m, x, r)))
            variants.append(((name, tag, "2"), lambda m=m, x=x, r=r: today(m, x, r)))
            variants.append(((name, tag, "3"), lambda m=m, x=x: m(x)))
    times = time_variants(variants, a.rounds, a.iters)
    mi355attn.sync_status(wait=True)
    n = B * C * H * W
    out, targets = [], []
    print(f"shape {tuple(a.shape)}, {a.rounds} rounds x {a.iters} calls, ms per call")
    print("| gate | io | row | median ms | min .. max ms | GB/s at algorithmic bytes |")
    print("|---|---|---|---|---|---|")
    for (name, tag, row), ts in times.items():
        med = statistics.median(ts)
        gbs = n * (4 if tag == "fp32" else 2) * PASSES[row] / (med * 1e-3) / 1e9
        print(f"| {name} | {tag} | {row} | {med:.4f} | {min(ts):.4f} .. {max(ts):.4f} | {gbs:.0f} |")
        out.append({"gate": name, "io": tag, "row": row, "median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "gbs": gbs})
    print("| gate | io | A: row 1 below row 2, ranges apart | B: row 1 <= 3/2 row 3 + spread of row 3 | row 1 vs its multi-pass form |")
    print("|---|---|---|---|---|")
    for tag in ("fp32", "fp16", "bf16"):
        for name in mods:
            t1, tm, t2, t3 = (times[(name, tag, k)] for k in ("1", "1m", "2", "3"))
            ta = max(t1) < min(t2)
            tb = statistics.median(t1) <= 1.5 * statistics.median(t3) + (max(t3) - min(t3))
            faster = statistics.median(t1) <= statistics.median(tm)
            print(f"| {name} | {tag} | {'met' if ta else 'NOT met'} | {'met' if tb else 'NOT met'} | {'single-read faster' if faster else 'multi-pass faster'} |")
            targets.append({"gate": name, "io": tag, "A": ta, "B": tb, "single_read_faster": faster})
    line = json.dumps({"shape": a.shape, "rounds": a.rounds, "iters": a.iters, "rows": out, "targets": targets})
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
