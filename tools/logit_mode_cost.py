#!/usr/bin/env python
"""What precision 3 costs: ViT `Attention(768, 12)` (C3) at B = 256 in precisions 1, 3 and 0, one process, interleaved.

    python tools/logit_mode_cost.py [--batch 256] [--repeats 25] [--warmup 5] [--out FILE]

Each repeat times one forward of every mode in turn (HIP events on the launch stream, mi355attn.StreamTimer), so clock and thermal drift
hit the three modes alike; reported are the median and the spread (min .. max, and the quartiles) over the repeats.  The per-kernel split
of every mode comes from a separate traced pass (mi355attn.kernel_trace: a HIP event pair around each launch), which is not mixed into
the timed repeats.  The yardsticks are this run's own precision 0 and precision 1.  Exit status 1 if precision 3 is not faster than
precision 0 by more than the run's spread (then the mode has no reason to exist).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-attention_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report (markdown) to this file")
    a = ap.parse_args()
    import torch
    import mi355attn
    from mi355attn.modules import Attention

    torch.manual_seed(1234)
    mods = {p: Attention(768, 12, precision=p).eval() for p in (1, 3, 0)}
    for p in (3, 0):
        mods[p].load_state_dict(mods[1].state_dict())
    mods = {p: m.cuda() for p, m in mods.items()}
    torch.manual_seed(4321)
    x = torch.randn(a.batch, 197, 768, device="cuda")
    order = (1, 3, 0)
    times = {p: [] for p in order}
    timer = mi355attn.StreamTimer(x.device)
    with torch.no_grad():
        for _ in range(a.warmup):
            for p in order:
                mods[p](x)
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for p in order:
                timer.start()
                mods[p](x)
                times[p].append(timer.stop_ms() * 1e3)
        traces = {}
        for p in order:
            def run(p=p):
                for _ in range(5):
                    mods[p](x)
                torch.cuda.synchronize()
            traces[p] = mi355attn.kernel_trace(run)

    def stats(v):
        q = statistics.quantiles(v, n=4)
        return statistics.median(v), min(v), max(v), q[0], q[2]

    st = {p: stats(times[p]) for p in order}
    lines = ["C3 `Attention(768, 12)`, B = %d, N = 197: %d interleaved timed forwards per mode after %d warm-up rounds (HIP events), us." % (
        a.batch, a.repeats, a.warmup), "",
        "| precision | median | min | max | quartiles | vs precision 1 | vs precision 0 |", "|---|---|---|---|---|---|---|"]
    for p in order:
        med, lo, hi, q1, q3 = st[p]
        lines.append("| %d | %.1f | %.1f | %.1f | %.1f .. %.1f | %.2fx | %.2fx |" % (p, med, lo, hi, q1, q3, med / st[1][0], med / st[0][0]))
    lines += ["", "Per-kernel split (traced pass of 5 forwards per mode; mean us per launch):", ""]
    for p in order:
        lines.append("precision %d:" % p)
        lines.append("")
        lines.append("| kernel | launches | mean us | min us | max us |")
        lines.append("|---|---|---|---|---|")
        for tag, cnt, tot, mn, mx in traces[p]:
            lines.append("| `%s` | %d | %.1f | %.1f | %.1f |" % (tag, cnt, tot / max(cnt, 1), mn, mx))
        lines.append("")
    spread = max(st[3][2] - st[3][1], st[0][2] - st[0][1])
    gap = st[0][0] - st[3][0]
    ok = gap > spread
    lines.append("Condition: precision 3 faster than precision 0 by more than the run's spread -- median gap %.1f us, larger min..max spread of the two "
                 "%.1f us: %s." % (gap, spread, "met" if ok else "NOT met"))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        except OSError as e:
            print("not written: %s" % e, file=sys.stderr)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
