#!/usr/bin/env python
"""Time CoordinateAttention, TripletAttention, AttentionGate and BAM on 16-bit activations against the fp32 kernels and against the
cast-around a user had to write before.

    python tools/axis_io16_bench.py [--shape 256 256 56 56] [--rounds 9] [--iters 20] [--json out.json]

One process, one device, per shape all variants interleaved round by round (a round times every variant once, `iters` calls between
two events), so drift hits every variant alike.  Per module and I/O type:
    row 1   m(x16)                          the 16-bit sweeps of csrc/axis_attn_io16.hip (CoordAtt: 6 B / element)
    row 2   m(x32)                          the fp32 kernels on the fp32 copy of the same tensor (12 B / element)
    row 3   m(x16.float()).to(x16.dtype)    what a user wrote before this path existed, on code this path leaves untouched: the baseline
                                            (24 B / element)
Prints a markdown table (median, min .. max over the rounds, row 3 / row 1 and row 2 / row 1) and one JSON line.  The last column is the
shipping condition of the 16-bit path: row 1 is faster than row 3 by more than row 3's own min .. max spread in this run."""
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


def modules(C):
    from mi355attn.modules import BAM, CoordinateAttention, TripletAttention
    from mi355attn.modules.axis import AttentionGate
    torch.manual_seed(1234)
    mods = {"CoordinateAttention": CoordinateAttention(C, C), "TripletAttention": TripletAttention(7), "AttentionGate": AttentionGate(7), "BAM": BAM(C)}
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():                                              # the default BatchNorm is the identity
        for m in mods.values():
            for mod in m.modules():
                if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                    mod.weight.copy_(0.5 + torch.rand(mod.weight.shape, generator=g))
                    mod.bias.copy_(0.2 * torch.randn(mod.bias.shape, generator=g))
                    mod.running_mean.copy_(0.2 * torch.randn(mod.running_mean.shape, generator=g))
                    mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
    return {k: m.eval().cuda() for k, m in mods.items()}


def bench(shape, rounds, iters):
    import mi355attn
    B, C, H, W = shape
    mods = modules(C)
    torch.manual_seed(4321)
    x32 = torch.randn(B, C, H, W, device="cuda")
    xs = {"fp16": x32.half(), "bf16": x32.bfloat16()}
    xfs = {tag: x16.float() for tag, x16 in xs.items()}                # the fp32 copy of each 16-bit tensor, shared by the modules
    del x32
    variants = []
    for name, m in mods.items():
        for tag, x16 in xs.items():
            xf = xfs[tag]
            variants.append((name, tag, "1", lambda m=m, x=x16: m(x)))
            variants.append((name, tag, "2", lambda m=m, x=xf: m(x)))
            variants.append((name, tag, "3", lambda m=m, x=x16: m(x.float()).to(x.dtype)))
    times = {v[:3]: [] for v in variants}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        for _, _, _, fn in variants:                                   # warm-up: workspaces, first-use zeroing, clocks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, tag, row, fn in variants:
                start.record()
                for _ in range(iters):
                    fn()
                stop.record()
                stop.synchronize()
                times[(name, tag, row)].append(start.elapsed_time(stop) / iters)
    mi355attn.sync_status(wait=True)
    print(f"shape {tuple(shape)}, {rounds} rounds x {iters} calls, ms per call")
    print("| module | io | 16-bit ms (min .. max) | fp32 ms (min .. max) | cast-around ms (min .. max) | cast-around / 16-bit | fp32 / 16-bit | "
          "faster than the cast-around by more than its spread |")
    print("|---|---|---|---|---|---|---|---|")
    out = []
    for name in mods:
        for tag in xs:
            t1, t2, t3 = (times[(name, tag, r)] for r in ("1", "2", "3"))
            m1, m2, m3 = (statistics.median(t) for t in (t1, t2, t3))
            ships = m3 - m1 > max(t3) - min(t3)
            print(f"| {name} | {tag} | {m1:.4f} ({min(t1):.4f} .. {max(t1):.4f}) | {m2:.4f} ({min(t2):.4f} .. {max(t2):.4f}) | "
                  f"{m3:.4f} ({min(t3):.4f} .. {max(t3):.4f}) | {m3 / m1:.2f} | {m2 / m1:.2f} | {'yes' if ships else 'NO'} |")
            out.append({"module": name, "io": tag, "io16_ms": m1, "io16_min_ms": min(t1), "io16_max_ms": max(t1), "fp32_ms": m2, "cast_ms": m3,
                        "cast_min_ms": min(t3), "cast_max_ms": max(t3), "ships": ships})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[256, 256, 56, 56])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {"rounds": a.rounds, "iters": a.iters, "shape": a.shape, "rows": bench(a.shape, a.rounds, a.iters)}
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
