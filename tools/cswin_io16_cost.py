#!/usr/bin/env python
"""What the 16-bit path of CSWinBlock saves: the four CSWin-T blocks of the bench step at B = 256 -- (256, 3136, 64), (256, 784, 128),
(256, 196, 256), (256, 49, 512) -- on an fp16 and on a bf16 x, one process, interleaved.

    python tools/cswin_io16_cost.py [--batch 256] [--repeats 25] [--warmup 5] [--out FILE]

Three ways to serve a 16-bit x, per shape and type:
    io16         the block on the 16-bit tensor (16-bit in, 16-bit out; stages 1-2: cswin_stripe_kernel<.., x16> and
                 mlp_fused_kernel<.., proj, x16>, two launches; stages 3-4: layernorm_x16_kernel, the existing GEMMs and LePE core,
                 gemm16_res_kernel twice)
    cast-around  what a user had to write before: x16.float() -> the fp32-I/O block at precision = the type -> .to(dtype)
    fp32         the fp32-I/O block alone on an fp32 x (the two torch casts of cast-around left out)
Each repeat times one run of every variant in turn (HIP events on the launch stream, mi355attn.StreamTimer), so clock and thermal drift
hit all of them alike; the order is reversed on every other repeat.  Reported are the median and the spread (min .. max, and the
quartiles) over the repeats.  The per-kernel tally comes from a separate traced pass (mi355attn.kernel_trace: a HIP event pair around
each launch; torch's cast kernels are not instrumented and do not appear), which is not mixed into the timed repeats.  The condition,
per shape and type: the 16-bit block beats the cast-around by more than the larger min..max spread of the two.  It is reported (met /
NOT met), not gated: the exit status is 0 either way.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-attention_amd"))

SHAPES = (("s1", (64, 56, 2), dict(split_size=1, qkv_bias=True)), ("s2", (128, 28, 4), dict(split_size=2, qkv_bias=True)),
          ("s3", (256, 14, 8), dict(split_size=7, qkv_bias=True)), ("s4", (512, 7, 16), dict(split_size=7, qkv_bias=True, last_stage=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report (markdown) to this file")
    a = ap.parse_args()
    import torch
    import mi355attn
    from mi355attn.modules import CSWinBlock

    types = (("fp16", torch.float16, 1), ("bf16", torch.bfloat16, 2))
    lines = ["`CSWinBlock` at the four bench shapes, B = %d: %d interleaved timed runs per variant after %d warm-up rounds (HIP events), us."
             % (a.batch, a.repeats, a.warmup), ""]
    verdicts, splits = [], []
    for sname, args, kw in SHAPES:
        C, reso, _ = args
        torch.manual_seed(1234)
        base = CSWinBlock(*args, **kw).eval()
        torch.manual_seed(4321)
        x32 = torch.randn(a.batch, reso * reso, C, device="cuda")
        runs = {}
        for name, dt, p in types:
            m = CSWinBlock(*args, precision=p, **kw).eval()
            m.load_state_dict(base.state_dict())
            m = m.cuda().requires_grad_(False)
            x = x32.to(dt)
            runs[name + " io16"] = lambda m=m, x=x: m(x)
            runs[name + " cast-around"] = lambda m=m, x=x, dt=dt: m(x.float()).to(dt)
            runs[name + " fp32"] = lambda m=m: m(x32)
        order = list(runs)
        times = {k: [] for k in order}
        timer = mi355attn.StreamTimer(x32.device)
        with torch.no_grad():
            for _ in range(a.warmup):
                for k in order:
                    runs[k]()
            torch.cuda.synchronize()
            for rep in range(a.repeats):
                for k in (order if rep % 2 == 0 else order[::-1]):
                    timer.start()
                    runs[k]()
                    times[k].append(timer.stop_ms() * 1e3)
            traces = {}
            for k in order:
                if k.endswith("cast-around"):
                    continue                                 # its library kernels are those of the fp32 variant
                def run(k=k):
                    for _ in range(5):
                        runs[k]()
                    torch.cuda.synchronize()
                traces[k] = mi355attn.kernel_trace(run)

        def stats(v):
            q = statistics.quantiles(v, n=4)
            return statistics.median(v), min(v), max(v), q[0], q[2]

        st = {k: stats(times[k]) for k in order}
        lines += ["%s: `CSWinBlock%s` on (%d, %d, %d)" % (sname, (args, kw), a.batch, reso * reso, C), "",
                  "| variant | median | min | max | quartiles | vs cast-around |", "|---|---|---|---|---|---|"]
        for k in order:
            t = k.split()[0]
            med, lo, hi, q1, q3 = st[k]
            ratio = "--" if k.endswith("cast-around") else "%.2fx" % (med / st[t + " cast-around"][0])
            lines.append("| %s | %.1f | %.1f | %.1f | %.1f .. %.1f | %s |" % (k, med, lo, hi, q1, q3, ratio))
        lines.append("")
        for name, _, _ in types:
            io, ca = st[name + " io16"], st[name + " cast-around"]
            spread = max(io[2] - io[1], ca[2] - ca[1])
            gap = ca[0] - io[0]
            verdicts.append("Condition (%s, %s): the 16-bit block beats the cast-around by more than the larger min..max spread of the two -- "
                            "median gap %.1f us, spread %.1f us: %s." % (sname, name, gap, spread, "met" if gap > spread else "NOT met"))
        for k, rows in traces.items():
            splits += ["%s %s:" % (sname, k), "", "| kernel | launches | mean us | min us | max us |", "|---|---|---|---|---|"]
            splits += ["| `%s` | %d | %.1f | %.1f | %.1f |" % (tag, cnt, tot / max(cnt, 1), mn, mx) for tag, cnt, tot, mn, mx in rows]
            splits.append("")
        del runs, x32
        torch.cuda.empty_cache()
    lines += verdicts + ["", "Per-kernel tally (traced pass of 5 runs per variant; mean us per launch; torch's own cast kernels are not traced):", ""] + splits
    text = "\n".join(lines) + "\n"
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
