#!/usr/bin/env python
"""What the 16-bit path of the ViT encoder block saves: `TransformerEncoder(768, 12, qkv_bias=True)` at B = 64, N = 197 on an fp16 and on
a bf16 x, and its two residual products alone, one process, interleaved.

    python tools/vit_io16_cost.py [--batch 64] [--repeats 25] [--warmup 5] [--out FILE]

Three ways to serve a 16-bit x, per type:
    io16         the block on the 16-bit tensor (16-bit in, 16-bit out: layernorm_x16_kernel, gemm16_res_kernel twice)
    cast-around  what a user had to write before: x.float() -> the fp32-I/O block at precision = the type -> .half() / .bfloat16()
    fp32         the fp32-I/O block alone on an fp32 x (the two torch casts of cast-around left out)
and the two products of gemm16_res_kernel at the block's shapes (M = B * 197 rows) against the route they had before that kernel:
    proj  (N, K) = (768, 768),  16-bit residual, fp32 result    vs  widen16(residual) + linear16(resid fp32)
    fc2   (N, K) = (768, 3072), GELU, fp32 residual, 16-bit result  vs  linear16(resid fp32, out16) on the plain tile kernel
Each repeat times one run of every variant in turn (HIP events on the launch stream, mi355attn.StreamTimer), so clock and thermal drift
hit all of them alike; the order is reversed on every other repeat, because the two routes of a product read the same operands and the
one that runs second finds them in the cache (first-come order alone put 10 us of a 100 us product on whichever ran first).  Reported are the median and the spread (min .. max, and the quartiles) over the repeats.  The per-kernel split
comes from a separate traced pass (mi355attn.kernel_trace: a HIP event pair around each launch; torch's cast kernels are not
instrumented and do not appear), which is not mixed into the timed repeats.  Targets, each with the larger min..max spread of the
compared pair as its margin: a product is not slower than its earlier route beyond that spread; the io16 block beats the cast-around by
more than it.  Exit status 1 if a target is missed.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-attention_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report (markdown) to this file")
    a = ap.parse_args()
    import torch
    import mi355attn
    from mi355attn import functional as F
    from mi355attn.modules import TransformerEncoder

    types = (("fp16", torch.float16, 1), ("bf16", torch.bfloat16, 2))
    C, N = 768, 197
    M = a.batch * N
    torch.manual_seed(1234)
    base = TransformerEncoder(C, 12, qkv_bias=True).eval()
    mods = {}
    for name, _, p in types:
        mods[name] = TransformerEncoder(C, 12, qkv_bias=True, precision=p).eval()
        mods[name].load_state_dict(base.state_dict())
        mods[name] = mods[name].cuda().requires_grad_(False)
    torch.manual_seed(4321)
    x32 = torch.randn(a.batch, N, C, device="cuda")
    xs = {name: x32.to(dt) for name, dt, _ in types}
    runs = {}
    for name, dt, p in types:
        m, x = mods[name], xs[name]
        runs[name + " io16"] = lambda m=m, x=x: m(x)
        runs[name + " cast-around"] = lambda m=m, x=x, dt=dt: m(x.float()).to(dt)
        runs[name + " fp32"] = lambda m=m: m(x32)
        # the two products alone: operands of the block's shapes
        ctx = torch.randn(M, C, device="cuda").to(dt)
        hid = torch.randn(M, 4 * C, device="cuda").to(dt)
        wp, w2 = F.weight16(m.attn.proj.weight, p), F.weight16(m.mlp.fc2.weight, p)
        bp, b2 = m.attn.proj.bias, m.mlp.fc2.bias
        r16, r32 = x.reshape(M, C), x32.reshape(M, C)
        runs[name + " proj r16,o32"] = lambda ctx=ctx, wp=wp, bp=bp, r16=r16, p=p: F.linear16_res(ctx, wp, bp, r16, precision=p)
        runs[name + " proj widen16 + linear16"] = lambda ctx=ctx, wp=wp, bp=bp, r16=r16, p=p: F.linear16(ctx, wp, bp, resid=F.widen16(r16), precision=p)
        runs[name + " fc2 r32,o16"] = lambda hid=hid, w2=w2, b2=b2, p=p, dt=dt: F.linear16_res(hid, w2, b2, r32, act=F.ACT_GELU, out_dtype=dt, precision=p)
        runs[name + " fc2 linear16 out16"] = lambda hid=hid, w2=w2, b2=b2, p=p: F.linear16(hid, w2, b2, act=F.ACT_GELU, resid=r32, out16=True, precision=p)
    order = list(runs)
    times = {k: [] for k in order}
    timer = mi355attn.StreamTimer(x32.device)
    with torch.no_grad():
        for _ in range(a.warmup):
            for k in order:
                runs[k]()
        torch.cuda.synchronize()
        for rep in range(a.repeats):
            for k in (order if rep % 2 == 0 else order[::-1]):     # alternate: the second of a compared pair finds its operands in the cache
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
    lines = ["`TransformerEncoder(768, 12, qkv_bias=True)`, B = %d, N = %d (M = %d rows): %d interleaved timed runs per variant after %d "
             "warm-up rounds (HIP events), us." % (a.batch, N, M, a.repeats, a.warmup), "",
             "| variant | median | min | max | quartiles | vs its comparison |", "|---|---|---|---|---|---|"]
    versus = {" io16": " cast-around", " fp32": " cast-around", " proj r16,o32": " proj widen16 + linear16", " fc2 r32,o16": " fc2 linear16 out16"}
    for k in order:
        t = k.split()[0]
        med, lo, hi, q1, q3 = st[k]
        other = versus.get(k[len(t):])
        ratio = "%.2fx" % (med / st[t + other][0]) if other else "--"
        lines.append("| %s | %.1f | %.1f | %.1f | %.1f .. %.1f | %s |" % (k, med, lo, hi, q1, q3, ratio))
    lines += ["", "Per-kernel split (traced pass of 5 runs per variant; mean us per launch; torch's own cast kernels are not traced):", ""]
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
        for new, old, what in ((" proj r16,o32", " proj widen16 + linear16", "proj (768, 768), 16-bit residual, fp32 result"),
                               (" fc2 r32,o16", " fc2 linear16 out16", "fc2 (768, 3072), GELU, fp32 residual, 16-bit result")):
            nw, od = st[name + new], st[name + old]
            spread = max(nw[2] - nw[1], od[2] - od[1])
            met = nw[0] - od[0] <= spread
            ok = ok and met
            lines.append("Target (%s, %s): gemm16_res_kernel is not slower than the earlier route beyond the larger min..max spread of the two -- "
                         "median %.1f us against %.1f us, spread %.1f us: %s." % (name, what, nw[0], od[0], spread, "met" if met else "NOT met"))
        io, ca = st[name + " io16"], st[name + " cast-around"]
        spread = max(io[2] - io[1], ca[2] - ca[1])
        gap = ca[0] - io[0]
        met = gap > spread
        ok = ok and met
        lines.append("Target (%s, block): the 16-bit block beats the cast-around by more than the larger min..max spread of the two -- median gap "
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
