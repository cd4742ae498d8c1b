#!/usr/bin/env python
"""What the matrix-core branch kernel of SKLayer costs (csrc/sk_wide.hip): the four SK units of SKNet-50 at B = 64 and the `zoo2` bench
shape SKLayer(256, 256) on (256, 256, 56, 56), option sk_wide = 0 (the fp32 FMA kernels, where they apply) against sk_wide = 1, one
process, interleaved.

    python tools/sk_wide_cost.py [--repeats 15] [--warmup 3] [--out FILE]

Each repeat times one forward of every route in turn (HIP events on the launch stream, mi355attn.StreamTimer), so clock and thermal
drift hit both alike; reported are the median and the spread (min .. max) over the repeats.  The per-launch split (pack, branches,
select, apply) comes from a separate traced pass (mi355attn.kernel_trace), which is not mixed into the timed repeats.  Nothing is
gated: the figures go to profiles/sk_wide.md.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-attention_amd"))

# (label, inplanes, planes, groups, x shape)
SHAPES = [
    ("SKNet-50 stage 1", 128, 128, 32, (64, 128, 56, 56)),
    ("SKNet-50 stage 2", 256, 256, 32, (64, 256, 28, 28)),
    ("SKNet-50 stage 3", 512, 512, 32, (64, 512, 14, 14)),
    ("SKNet-50 stage 4", 1024, 1024, 32, (64, 1024, 7, 7)),
    ("zoo2 SKLayer(256,256)", 256, 256, 32, (256, 256, 56, 56)),
]
FMA_WIDTHS = (1, 2, 4, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report (markdown) to this file")
    a = ap.parse_args()
    import torch
    import mi355attn
    from mi355attn.modules import SKLayer

    lines = ["%d interleaved timed forwards per route after %d warm-up rounds (HIP events), us; flop = two grouped 3x3 branches." % (
        a.repeats, a.warmup), "",
        "| unit | x | sk_wide | median | min | max | TFLOP/s | vs sk_wide=0 |", "|---|---|---|---|---|---|---|---|"]
    splits = []
    for label, cin, planes, groups, shape in SHAPES:
        torch.manual_seed(1234)
        m = SKLayer(cin, planes, groups=groups).eval().cuda()
        torch.manual_seed(4321)
        x = torch.randn(*shape, device="cuda")
        routes = ([0] if planes // groups in FMA_WIDTHS else []) + [1]
        flop = 2.0 * 2 * shape[0] * shape[2] * shape[3] * planes * (cin // groups) * 9
        times = {r: [] for r in routes}
        timer = mi355attn.StreamTimer(x.device)
        traces = {}
        with torch.no_grad():
            for _ in range(a.warmup):
                for r in routes:
                    with mi355attn.options(sk_wide=r):
                        m(x)
            torch.cuda.synchronize()
            for _ in range(a.repeats):
                for r in routes:
                    with mi355attn.options(sk_wide=r):
                        timer.start()
                        m(x)
                        times[r].append(timer.stop_ms() * 1e3)
            for r in routes:
                def run(r=r):
                    with mi355attn.options(sk_wide=r):
                        for _ in range(3):
                            m(x)
                    torch.cuda.synchronize()
                traces[r] = mi355attn.kernel_trace(run)
        med = {r: statistics.median(times[r]) for r in routes}
        for r in routes:
            lines.append("| %s | %s | %d | %.1f | %.1f | %.1f | %.1f | %s |" % (
                label, "x".join(map(str, shape)), r, med[r], min(times[r]), max(times[r]), flop / med[r] * 1e-6,
                "%.2fx" % (med[r] / med[0]) if 0 in med else "n/a (refused before)"))
        if 0 in med:
            spread = max(max(times[r]) - min(times[r]) for r in routes)
            gap = med[0] - med[1]
            lines.append("| | | | | | | | median gap %.1f us, larger min..max spread %.1f us: sk_wide=1 %s |" % (
                gap, spread, "wins" if gap > spread else "loses" if -gap > spread else "ties"))
        for r in routes:
            splits += ["%s, sk_wide=%d (traced pass of 3 forwards; mean us per launch):" % (label, r), "",
                       "| kernel | launches | mean us | min us | max us |", "|---|---|---|---|---|"]
            splits += ["| `%s` | %d | %.1f | %.1f | %.1f |" % (tag, cnt, tot / max(cnt, 1), mn, mx) for tag, cnt, tot, mn, mx in traces[r]]
            splits.append("")
        del m, x
        torch.cuda.empty_cache()
    text = "\n".join(lines + ["", "Per-launch split", ""] + splits) + "\n"
    print(text)
    if a.out:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        except OSError as e:
            print("not written: %s" % e, file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
