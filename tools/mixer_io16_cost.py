#!/usr/bin/env python
"""What the 16-bit path of the MLP-Mixer layer saves: `MixerLayer(512, 196)` at B = 256 on an fp16 and on a bf16 x, one process, interleaved.

    python tools/mixer_io16_cost.py [--batch 256] [--repeats 25] [--warmup 5] [--out FILE]

Three ways to serve a 16-bit x, per type:
    io16         the layer on the 16-bit tensor (16-bit in, 16-bit out: csrc/mixer_fused.hip mixer_token16_kernel + the 16-bit GEMM epilogue)
    cast-around  what a user had to write before: x.float() -> the fp32-I/O layer at precision = the type -> .half() / .bfloat16()
    fp32         the fp32-I/O layer alone on an fp32 x (the two torch casts of cast-around left out)
The cast-around and the fp32 layer run only kernels the 16-bit path does not touch.  Each repeat times one forward of every variant in
turn (HIP events on the launch stream, mi355attn.StreamTimer), so clock and thermal drift hit all of them alike; reported are the median
and the spread (min .. max, and the quartiles) over the repeats.  The per-kernel split comes from a separate traced pass
(mi355attn.kernel_trace: a HIP event pair around each launch; torch's cast kernels are not instrumented and do not appear), which is not
mixed into the timed repeats.  Exit status 1 if, for either type, io16 is not faster than cast-around by more than the larger min..max
spread of the two.
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
    from mi355attn.modules import MixerLayer

    types = (("fp16", torch.float16, 1), ("bf16", torch.bfloat16, 2))
    torch.manual_seed(1234)
    base = MixerLayer(512, 196).eval()
    mods = {}
    for name, _, p in types:
        mods[name] = MixerLayer(512, 196, precision=p).eval()
        mods[name].load_state_dict(base.state_dict())
        mods[name] = mods[name].cuda()
    torch.manual_seed(4321)
    x32 = torch.randn(a.batch, 196, 512, device="cuda")
    xs = {name: x32.to(dt) for name, dt, _ in types}
    runs = {}
    for name, dt, _ in types:
        runs[name + " io16"] = lambda m=mods[name], x=xs[name]: m(x)
        runs[name + " cast-around"] = lambda m=mods[name], x=xs[name], dt=dt: m(x.float()).to(dt)
        runs[name + " fp32"] = lambda m=mods[name]: m(x32)
    order = list(runs)
    times = {k: [] for k in order}
    timer = mi355attn.StreamTimer(x32.device)
    with torch.no_grad():
        for _ in range(a.warmup):
            for k in order:
                runs[k]()
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for k in order:
                timer.start()
                runs[k]()
                times[k].append(timer.stop_ms() * 1e3)
        traces = {}
        for k in order:
            def run(k=k):
                for _ in range(5):
                    runs[k]()
                torch.cuda.synchronize()
            traces[k] = mi355attn.kernel_trace(run)

    def stats(v):
        q = statistics.quantiles(v, n=4)
        return statistics.median(v), min(v), max(v), q[0], q[2]

    st = {k: stats(times[k]) for k in order}
    lines = ["`MixerLayer(512, 196)`, B = %d: %d interleaved timed forwards per variant after %d warm-up rounds (HIP events), us." % (
        a.batch, a.repeats, a.warmup), "",
        "| variant | median | min | max | quartiles | vs cast-around | vs fp32 layer |", "|---|---|---|---|---|---|---|"]
    for k in order:
        t = k.split()[0]
        med, lo, hi, q1, q3 = st[k]
        lines.append("| %s | %.1f | %.1f | %.1f | %.1f .. %.1f | %.2fx | %.2fx |" % (k, med, lo, hi, q1, q3, med / st[t + " cast-around"][0],
                                                                                   med / st[t + " fp32"][0]))
    lines += ["", "Per-kernel split (traced pass of 5 forwards per variant; mean us per launch; torch's own cast kernels are not traced):", ""]
    for k in order:
        if k.endswith("cast-around"):
            continue                                     # its library kernels are those of the fp32 variant
        lines.append("%s:" % k)
        lines.append("")
        lines.append("| kernel | launches | mean us | min us | max us |")
        lines.append("|---|---|---|---|---|")
        for tag, cnt, tot, mn, mx in traces[k]:
            lines.append("| `%s` | %d | %.1f | %.1f | %.1f |" % (tag, cnt, tot / max(cnt, 1), mn, mx))
        lines.append("")
    ok = True
    for name, _, _ in types:
        io, ca = st[name + " io16"], st[name + " cast-around"]
        spread = max(io[2] - io[1], ca[2] - ca[1])
        gap = ca[0] - io[0]
        met = gap > spread
        ok = ok and met
        lines.append("Condition (%s): the 16-bit layer beats the cast-around by more than the larger min..max spread of the two -- median gap "
                     "%.1f us, spread %.1f us: %s." % (name, gap, spread, "met" if met else "NOT met"))
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
