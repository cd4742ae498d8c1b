#!/usr/bin/env python
"""What the 16-bit path of XCABlock saves: XCABlock(384, 8) (the C4 shape) and XCABlock(128, 4) (the nano model's width) at B = 256 on
14 x 14 tokens, on an fp16 and on a bf16 x, one process, interleaved.

    python tools/xcit_io16_cost.py [--batch 256] [--repeats 25] [--warmup 5] [--out FILE]

Three ways to serve a 16-bit x, per block and type:
    io16         the block on the 16-bit tensor (16-bit in, 16-bit out: XCABlock._forward16)
    cast-around  what a user had to write before: x16.float() -> the fp32-I/O block at precision = the type -> .to(dtype), all three timed
    fp32         the fp32-I/O block alone on an fp32 x (the two torch casts of cast-around left out)
and three kernel pairs, per type, on the same rows (M = B * 196):
    proj         linear16_stats_r16 (the 16-bit residual read by the GEMM)       against  widen16 + linear16_stats        (N = K = 384)
    fc2          linear16_res_scale (fp32 residual, 16-bit store)                against  linear16 with the fp32 residual: the kernel the
                                                                                          fp32 block runs, fp32 store     (N = 384, K = 1536)
    mlp          mlp_fused_o16 (16-bit store in the epilogue)                    against  mlp_fused + round16, and mlp_fused alone (C = 128)
Each repeat times one run of every variant in turn (HIP events on the launch stream, mi355attn.StreamTimer), so clock and thermal drift
hit all of them alike; the order is reversed on every other repeat.  Reported are the median, the quartiles and min .. max over the
repeats.  A target counts as met only when the min .. max ranges of the two variants do not overlap; otherwise it is reported as NOT
met, with the medians.  Nothing is gated: the exit status is 0 either way.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-attention_amd"))

BLOCKS = (("C4", 384, 8), ("nano", 128, 4))
GRID = 14


def timed(runs, repeats, warmup, device):
    import torch
    import mi355attn
    order = list(runs)
    times = {k: [] for k in order}
    timer = mi355attn.StreamTimer(device)
    with torch.no_grad():
        for _ in range(warmup):
            for k in order:
                runs[k]()
        torch.cuda.synchronize()
        for rep in range(repeats):
            for k in (order if rep % 2 == 0 else order[::-1]):
                timer.start()
                runs[k]()
                times[k].append(timer.stop_ms() * 1e3)

    def stats(v):
        q = statistics.quantiles(v, n=4)
        return statistics.median(v), min(v), max(v), q[0], q[2]
    return {k: stats(times[k]) for k in order}


def table(st, lines):
    lines += ["| variant | median | quartiles | min | max |", "|---|---|---|---|---|"]
    for k, (med, lo, hi, q1, q3) in st.items():
        lines.append("| %s | %.1f | %.1f .. %.1f | %.1f | %.1f |" % (k, med, q1, q3, lo, hi))
    lines.append("")


def verdict(what, fast, slow, st, strict=True):
    """`fast` is faster than `slow` (strict) or no slower: counted as met only when the two min .. max ranges do not overlap, `fast` below."""
    f, s = st[fast], st[slow]
    return "Target (%s): %s %s %s -- medians %.1f vs %.1f us, ranges %.1f .. %.1f vs %.1f .. %.1f: %s." % (
        what, fast, "faster than" if strict else "no slower than", slow, f[0], s[0], f[1], f[2], s[1], s[2], "met" if f[2] < s[1] else "NOT met")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report (markdown) to this file")
    a = ap.parse_args()
    import torch
    import mi355attn
    from mi355attn import functional as F
    from mi355attn.modules import XCABlock

    types = (("fp16", torch.float16, 1), ("bf16", torch.bfloat16, 2))
    N = GRID * GRID
    M = a.batch * N
    dev = torch.device("cuda", 0)
    lines = ["`XCABlock` at B = %d on %d x %d tokens: %d interleaved timed runs per variant after %d warm-up rounds (HIP events), us."
             % (a.batch, GRID, GRID, a.repeats, a.warmup), ""]
    verdicts, splits = [], []
    for bname, C, heads in BLOCKS:
        torch.manual_seed(1234)
        base = XCABlock(C, heads, eta=1.0).eval()
        torch.manual_seed(4321)
        x32 = torch.randn(a.batch, N, C, device=dev)
        runs = {}
        for name, dt, p in types:
            m = XCABlock(C, heads, eta=1.0, precision=p).eval()
            m.load_state_dict(base.state_dict())
            m = m.cuda().requires_grad_(False)
            x = x32.to(dt)
            runs[name + " io16"] = lambda m=m, x=x: m(x, GRID, GRID)
            runs[name + " cast-around"] = lambda m=m, x=x, dt=dt: m(x.float(), GRID, GRID).to(dt)
            runs[name + " fp32"] = lambda m=m: m(x32, GRID, GRID)
        st = timed(runs, a.repeats, a.warmup, dev)
        lines += ["%s: `XCABlock(%d, %d)` on (%d, %d, %d)" % (bname, C, heads, a.batch, N, C), ""]
        table(st, lines)
        for name, _, _ in types:
            verdicts.append(verdict("%s block, %s" % (bname, name), name + " io16", name + " cast-around", st))
        with torch.no_grad():
            for k in runs:
                if k.endswith("cast-around"):
                    continue                                 # its library kernels are those of the fp32 variant

                def run(k=k):
                    for _ in range(5):
                        runs[k]()
                    torch.cuda.synchronize()
                rows = mi355attn.kernel_trace(run)
                splits += ["%s %s:" % (bname, k), "", "| kernel | launches | mean us | min us | max us |", "|---|---|---|---|---|"]
                splits += ["| `%s` | %d | %.1f | %.1f | %.1f |" % (tag, cnt, tot / max(cnt, 1), mn, mx) for tag, cnt, tot, mn, mx in rows]
                splits.append("")
        del runs, x32
        torch.cuda.empty_cache()
    # ---- the three kernel pairs ------------------------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(99)
    ln, fc1, fc2 = torch.nn.LayerNorm(128).cuda(), torch.nn.Linear(128, 512).cuda(), torch.nn.Linear(512, 128).cuda()
    for name, dt, p in types:
        ctx = torch.randn(M, 384, generator=g).to(dt).to(dev)
        wp = (torch.randn(384, 384, generator=g) / 384 ** 0.5).to(dt).to(dev)
        b = (0.1 * torch.randn(384, generator=g)).to(dev)
        r16 = torch.randn(M, 384, generator=g).to(dt).to(dev)
        r32 = r16.float()
        h = torch.randn(M, 1536, generator=g).to(dt).to(dev)
        w2 = (torch.randn(384, 1536, generator=g) / 1536 ** 0.5).to(dt).to(dev)
        x128 = torch.randn(M, 128, generator=g).to(dev)
        gam = (0.5 + torch.rand(128, generator=g)).to(dev)
        runs = {
            "proj stats_r16": lambda: F.linear16_stats_r16(ctx, wp, b, r16, 1e-6, precision=p),
            "proj widen16 + stats": lambda: F.linear16_stats(ctx, wp, b, F.widen16(r16), 1e-6, precision=p),
            "fc2 res_scale r32,o16": lambda: F.linear16_res_scale(h, w2, b, None, r32, out_dtype=dt, precision=p),
            "fc2 linear16 r32,o32": lambda: F.linear16(h, w2, b, resid=r32, precision=p),
            "mlp mlp_fused_o16": lambda: F.mlp_fused_o16(x128, ln, fc1, fc2, gamma=gam, precision=p),
            "mlp mlp_fused + round16": lambda: F.round16(F.mlp_fused(x128, ln, fc1, fc2, gamma=gam, precision=p), dt),
            "mlp mlp_fused": lambda: F.mlp_fused(x128, ln, fc1, fc2, gamma=gam, precision=p),
        }
        st = timed(runs, a.repeats, a.warmup, dev)
        lines += ["Kernel pairs, %s, M = %d:" % (name, M), ""]
        table(st, lines)
        verdicts.append(verdict("r16 proj, %s" % name, "proj stats_r16", "proj widen16 + stats", st))
        verdicts.append(verdict("o16 MLP, %s" % name, "mlp mlp_fused_o16", "mlp mlp_fused", st, strict=False))
        verdicts.append("Reported (fc2, %s): linear16_res_scale with a 16-bit store %.1f us against the fp32 block's fc2 kernel %.1f us (medians)."
                        % (name, st["fc2 res_scale r32,o16"][0], st["fc2 linear16 r32,o32"][0]))
        del runs
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
