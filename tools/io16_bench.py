#!/usr/bin/env python
"""Time SELayer / ECALayer / CBAM on 16-bit activations against the fp32 kernels and against the cast-around a user had to write before.

    python tools/io16_bench.py [--shape 256 256 56 56] [--rounds 9] [--iters 20] [--json out.json]
    python tools/io16_bench.py --da [--rounds 9] [--iters 20] [--json out.json]

One process, one device, all variants interleaved round by round (a round times every variant once, `iters` calls between two events),
so drift hits every variant alike.  Per block and I/O type:
    row 1   m(x16)                          the 16-bit kernels, single-read form where the shape allows   4 B / element
    row 1g  m(x16), *_single options off    the 16-bit general form (pool, gates, scale)                  (reads x twice or three times)
    row 2   m(x32)                          the fp32 kernels on the fp32 copy of the same tensor          8 B / element
    row 3   m(x16.float()).to(x16.dtype)    what a user wrote before this path existed                    20 B / element
--da times DoubleAttention instead, at its two bench shapes -- DoubleAttention(64, 32, 32) on (256, 64, 32, 32), the one-kernel path,
and DoubleAttention(256, 128, 128) on (256, 256, 56, 56), the two-pass path -- with the same four rows (row 1g: option "da_fused" = 0,
the general route; the bytes per element are those of x and y alone, the two-pass path also moves its 16-bit V tensor twice).
Prints a markdown table (median, min .. max over the rounds, achieved GB/s at the row's algorithmic bytes) and one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-attention_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

BYTES = {"1": 4, "1g": 4, "2": 8, "3": 20}
SINGLE_OPTS = ("se_single", "eca_single", "cbam_single")


def time_variants(variants, rounds, iters):
    """variants: [(key, fn)].  Every round times every variant once, `iters` calls between two events."""
    times = {k: [] for k, _ in variants}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        for _, fn in variants:                                         # warm-up: workspaces, first-use zeroing, clocks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for key, fn in variants:
                start.record()
                for _ in range(iters):
                    fn()
                stop.record()
                stop.synchronize()
                times[key].append(start.elapsed_time(stop) / iters)
    return times


def report(title, times, n, out):
    print(title)
    print("| block | io | row | median ms | min .. max ms | GB/s at algorithmic bytes |")
    print("|---|---|---|---|---|---|")
    for (name, tag, row), ts in times.items():
        med = statistics.median(ts)
        gbs = n * BYTES[row] / (med * 1e-3) / 1e9
        print(f"| {name} | {tag} | {row} | {med:.4f} | {min(ts):.4f} .. {max(ts):.4f} | {gbs:.0f} |")
        out.append({"block": name, "io": tag, "row": row, "median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "gbs": gbs})


def rows_of(name, m, x32, general):
    """The four rows of one block in both I/O types."""
    variants = []
    for dt, tag in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        x16 = x32.to(dt)
        xf = x16.float()
        variants.append(((name, tag, "1"), lambda m=m, x=x16: m(x)))
        variants.append(((name, tag, "1g"), lambda m=m, x=x16: general(m, x)))
        variants.append(((name, tag, "2"), lambda m=m, x=xf: m(x)))
        variants.append(((name, tag, "3"), lambda m=m, x=x16: m(x.float()).to(x.dtype)))
    return variants


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[256, 256, 56, 56])
    ap.add_argument("--da", action="store_true", help="time DoubleAttention at its two bench shapes instead of SE / ECA / CBAM")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import mi355attn
    from mi355attn.modules import CBAM, DoubleAttention, ECALayer, SELayer
    out = []
    if a.da:
        def general(m, x):
            with mi355attn.options(da_fused=0):
                return m(x)
        shapes = []
        for name, (C, c), shape in (("DA64", (64, 32), (256, 64, 32, 32)), ("DA256", (256, 128), (256, 256, 56, 56))):
            torch.manual_seed(1234)
            m = DoubleAttention(C, c, c).eval().cuda()
            torch.manual_seed(4321)
            x32 = torch.randn(*shape, device="cuda")
            times = time_variants(rows_of(name, m, x32, general), a.rounds, a.iters)
            del x32
            mi355attn.sync_status(wait=True)
            mi355attn.range_status(wait=True)
            report(f"shape {shape}, {a.rounds} rounds x {a.iters} calls, ms per call", times, shape[0] * shape[1] * shape[2] * shape[3], out)
            shapes.append(list(shape))
            torch.cuda.empty_cache()
        line = json.dumps({"shapes": shapes, "rounds": a.rounds, "iters": a.iters, "rows": out})
    else:
        B, C, H, W = a.shape
        torch.manual_seed(1234)
        mods = {"SE": SELayer(C).eval().cuda(), "ECA": ECALayer(C).eval().cuda(), "CBAM": CBAM(C).eval().cuda()}
        torch.manual_seed(4321)
        x32 = torch.randn(B, C, H, W, device="cuda")

        def general(m, x):
            with mi355attn.options(**{k: 0 for k in SINGLE_OPTS}):
                return m(x)
        variants = []
        for name, m in mods.items():
            variants += rows_of(name, m, x32, general)
        times = time_variants(variants, a.rounds, a.iters)
        mi355attn.sync_status(wait=True)
        report(f"shape {tuple(a.shape)}, {a.rounds} rounds x {a.iters} calls, ms per call", times, B * C * H * W, out)
        line = json.dumps({"shape": a.shape, "rounds": a.rounds, "iters": a.iters, "rows": out})
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
