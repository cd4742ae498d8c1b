#!/usr/bin/env python
"""lpi_tile_kernel (token grids above 16 x 16) against lpi_kernel (option lpi_patch = 0) at EQUAL token count, C = 384:
    baseline   B = 256, 14 x 14   (50 176 tokens, the whole grid of 32 channels in LDS)
    tiled      B = 64,  28 x 28   (50 176 tokens, 4 bands of 7 rows)   and   B = 64, 24 x 24 (36 864 tokens, 3 bands of 8 rows)
each as y = x + gamma * LPI(x) (mi355_lpi_fwd) and with the LayerNorm on the way in from given statistics (mi355_ln_lpi_stats_fwd: only the
stencil kernel is timed).  One process, HIP events on the launch stream around 20 launches, inputs and outputs rotated through NB buffer
pairs larger than L2 + Infinity Cache together, interleaved rounds, best and worst round reported.  Prints a markdown table.
    python tools/lpi_tile_bench.py [rounds]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-attention_amd"))
import mi355attn  # noqa: E402
from mi355attn import StreamTimer, _ffi  # noqa: E402

dev = torch.device("cuda", 0)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
C, NB, IT = 384, 4, 20
SHAPES = (("lpi_kernel", 256, 14, 14), ("lpi_tile_kernel", 64, 28, 28), ("lpi_tile_kernel", 64, 24, 24))
torch.manual_seed(0)
par = dict(w1=torch.randn(C, 1, 3, 3) / 3, b1=torch.randn(C), bn_w=torch.rand(C) + 0.5, bn_b=torch.randn(C), bn_m=torch.randn(C) * 0.1,
           bn_v=torch.rand(C) + 0.5, w2=torch.randn(C, 1, 3, 3) / 3, b2=torch.randn(C), gamma=torch.rand(C) + 0.5, ln_w=torch.rand(C) + 0.5,
           ln_b=torch.randn(C) * 0.2)
par = {k: v.to(dev) for k, v in par.items()}
P = {k: _ffi.dptr(v) for k, v in par.items()}
lib = _ffi.lib()
st = _ffi.stream_ptr(dev)


def launcher(B, H, W, ln):
    xs = [torch.randn(B, H * W, C, device=dev) for _ in range(NB)]
    ys = [torch.empty_like(x) for x in xs]
    stats = torch.stack([xs[0].mean(-1), 1.0 / torch.sqrt(xs[0].var(-1, unbiased=False) + 1e-5)], -1).contiguous()

    def go(i):
        x, y = _ffi.dptr(xs[i % NB]), _ffi.dptr(ys[i % NB])
        if ln:
            rc = lib.mi355_ln_lpi_stats_fwd(x, _ffi.dptr(stats), P["ln_w"], P["ln_b"], P["w1"], P["b1"], P["bn_w"], P["bn_b"], P["bn_m"], P["bn_v"],
                                            1e-5, P["w2"], P["b2"], P["gamma"], x, y, B, H, W, C, st)
        else:
            rc = lib.mi355_lpi_fwd(x, P["w1"], P["b1"], P["bn_w"], P["bn_b"], P["bn_m"], P["bn_v"], 1e-5, P["w2"], P["b2"], P["gamma"], x, y,
                                   B, H, W, C, None, 0, st)
        _ffi.check(rc, "lpi")
    return go, (xs, ys, stats)


with mi355attn.options(lpi_patch=0):
    runs = []
    for ln in (False, True):
        for name, B, H, W in SHAPES:
            go, keep = launcher(B, H, W, ln)
            tag = [t for t, *_ in mi355attn.kernel_trace(lambda: go(0))][0]
            assert tag.startswith(name), tag
            runs.append(dict(tag=tag, tokens=B * H * W, go=go, keep=keep, us=[]))
    for r in range(rounds):
        for run in runs:
            for i in range(3):
                run["go"](i)
            torch.cuda.synchronize()
            tm = StreamTimer(dev)
            tm.start()
            for i in range(IT):
                run["go"](i)
            run["us"].append(tm.stop_ms() / IT * 1e3)
print("| kernel | tokens | us best | us worst | ns / token (best) | vs baseline per token |")
print("|---|---|---|---|---|---|")
for run in runs:
    base = [b for b in runs if b["tag"].startswith("lpi_kernel") and ("<ln>" in b["tag"]) == ("<ln>" in run["tag"])][0]
    per, per0 = min(run["us"]) / run["tokens"], min(base["us"]) / base["tokens"]
    print("| `%s` | %d | %.1f | %.1f | %.3f | %.2f |" % (run["tag"], run["tokens"], min(run["us"]), max(run["us"]), per * 1e3, per / per0), flush=True)
