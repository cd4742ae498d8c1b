#!/usr/bin/env python
"""What the run-time-width XCA core costs (xca_any_kernel of csrc/xcit.hip) next to the template kernel: B = 256, N = 196, 16-bit qkv
and context (mi355_xca16_fwd, qkv_is16 = 1), (heads, d) = (8, 48) on the template kernels against (8, 40), (8, 56), (8, 16), (16, 24),
(4, 96) and (3, 128) on the general one, one process, interleaved.

    python tools/xca_any_cost.py [--repeats 15] [--warmup 3] [--dtype fp16|bf16] [--out FILE]

Each repeat times one call of every shape in turn (HIP events on the launch stream, mi355attn.StreamTimer), so clock and thermal drift
hit all alike; reported are the median and the spread (min .. max) over the repeats, as us and as GB/s of the bytes the core has to
move (q + k + v in, the context out).  The comparison that matters is us per byte at d = 40 / 56 against the d = 48 template in the
same process.  The per-launch figures of a separate traced pass (mi355attn.kernel_trace) follow; they are not mixed into the timed
repeats.  Nothing is gated: the figures go to profiles/xca_any.md.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-attention_amd"))

B, N = 256, 196
TEMPLATE = (8, 48)
SHAPES = [TEMPLATE, (8, 40), (8, 56), (8, 16), (16, 24), (4, 96), (3, 128)]      # (heads, d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    ap.add_argument("--out", default=None, help="also write the report (markdown) to this file")
    a = ap.parse_args()
    import torch
    import mi355attn
    from mi355attn import functional as F

    prec, dt = (1, torch.float16) if a.dtype == "fp16" else (2, torch.bfloat16)
    data = {}
    for h, d in SHAPES:
        g = torch.Generator().manual_seed(100 * h + d)
        data[(h, d)] = (torch.randn(B, N, 3 * h * d, generator=g).to(dt).cuda(), (torch.rand(h, generator=g) + 0.5).cuda())
    nbytes = {(h, d): B * N * 4 * h * d * 2 for h, d in SHAPES}                   # q + k + v in, context out, 2 bytes each

    def call(s):
        return F.xca_core(data[s][0], data[s][1], s[0], precision=prec, out16=True)

    times = {s: [] for s in SHAPES}
    timer = mi355attn.StreamTimer(torch.device("cuda", torch.cuda.current_device()))
    with torch.no_grad():
        for _ in range(a.warmup):
            for s in SHAPES:
                call(s)
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for s in SHAPES:
                timer.start()
                call(s)
                times[s].append(timer.stop_ms() * 1e3)

        def traced():
            for _ in range(3):
                for s in SHAPES:
                    call(s)
            torch.cuda.synchronize()
        trace = mi355attn.kernel_trace(traced)
    med = {s: statistics.median(times[s]) for s in SHAPES}
    per_byte = {s: med[s] / nbytes[s] for s in SHAPES}
    lines = ["XCA core, B = %d, N = %d, %s qkv and context; %d interleaved timed calls per shape after %d warm-up rounds (HIP events)." % (
        B, N, a.dtype, a.repeats, a.warmup), "",
        "| heads | d | kernel | MB moved | median us | min | max | GB/s | us per byte vs d = 48 |", "|---|---|---|---|---|---|---|---|---|"]
    for s in SHAPES:
        lines.append("| %d | %d | %s | %.1f | %.1f | %.1f | %.1f | %.0f | %.2fx |" % (
            s[0], s[1], "template" if s == TEMPLATE else "xca_any_kernel", nbytes[s] * 1e-6, med[s], min(times[s]), max(times[s]),
            nbytes[s] / med[s] * 1e-3, per_byte[s] / per_byte[TEMPLATE]))
    lines += ["", "Per-launch figures (traced pass of 3 calls per shape; mean us per launch)", "",
              "| kernel | launches | mean us | min us | max us |", "|---|---|---|---|---|"]
    lines += ["| `%s` | %d | %.1f | %.1f | %.1f |" % (tag, cnt, tot / max(cnt, 1), mn, mx) for tag, cnt, tot, mn, mx in trace]
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
