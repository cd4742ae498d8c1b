#!/usr/bin/env python
"""Static issue budget of a hand-scheduled MFMA stream: what sits between consecutive v_mfma instructions of a kernel, and what it costs.

    python tools/mfma_slot_budget.py [--src csrc/gemm16_wst.hip] [--kernel gemm16_wst1_kernel] [--top 8] [--isa file.s]

The tool compiles ONE csrc file to ISA with the flags of build.py (device only, into a temporary directory; --isa reads a listing made
earlier instead), picks the kernels whose mangled name contains --kernel, and cuts each kernel into BODIES: maximal runs of straight-line text
that neither the header / back edge of the kernel's largest loop nor the target of a forward branch over at least one MFMA interrupts.  A body
with N MFMAs has N - 1 GAPS (the instructions between MFMA i and MFMA i + 1); what stands between the last MFMA of a body and the first one
of the next trip (loop tail, loop head: the tile boundary) is reported on its own and is in none of the sums.

A one-wave-per-SIMD kernel has nobody else to fill an issue cycle, so a gap runs about max(FLOOR, MFMA issue + the sum of its instructions'
issue costs).  The prices are in PRICE below -- the only place -- and instructions are classified by PREFIX only (first match in CLASSES).
Nothing here knows about dependencies, LDS or memory latency, or dual issue of scalar and vector instructions: it is a lower bound on the
serial issue time of ONE wave, good for comparing two schedules of the same work.
"""
import argparse
import collections
import math
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-attention_amd")

# Issue cost in cycles for ONE wave on a SIMD.  MI355X_MICROARCH.md, table row "vector-instruction ISSUE cost": a 16x16x32 MFMA holds vector
# issue for 8 of its 16 cycles, v_exp_f32 and the other quarter-rate (transcendental) operations 8, any other VALU instruction 4, `s_nop 0` 4;
# an LDS-DMA piece measured 25-185 there, priced at 60.  ASSUMED, given by no guide and measured by nobody: 4 for scalar ALU / branch
# instructions, s_waitcnt and ds_* instructions, 16 for a store or a plain load.
FLOOR = 16                                                             # an MFMA 16x16x32 occupies the matrix pipe for 16 cycles
PRICE = {"mfma": 8, "trans": 8, "valu": 4, "nop": 4, "dma": 60, "scalar": 4, "waitcnt": 4, "lds": 4, "store": 16, "load": 16, "other": 4}
ASSUMED = ("scalar", "waitcnt", "lds", "store", "load", "other")
# class by prefix, first match wins
CLASSES = (
    ("v_mfma", "mfma"), ("v_smfma", "mfma"),
    ("v_exp_", "trans"), ("v_log_", "trans"), ("v_rcp_", "trans"), ("v_rsq_", "trans"), ("v_sqrt_", "trans"), ("v_sin_", "trans"),
    ("v_cos_", "trans"),
    ("v_", "valu"),
    ("s_nop", "nop"), ("s_waitcnt", "waitcnt"), ("s_", "scalar"),
    ("ds_", "lds"),
    ("global_load_lds", "dma"), ("buffer_load_lds", "dma"),
    ("global_store", "store"), ("buffer_store", "store"), ("flat_store", "store"), ("scratch_store", "store"),
    ("global_atomic", "store"), ("buffer_atomic", "store"), ("flat_atomic", "store"),
    ("global_load", "load"), ("buffer_load", "load"), ("flat_load", "load"), ("scratch_load", "load"),
)
SPECIAL = ("dma", "store")                                             # gaps holding one of these are the schedule's reserved slots


def classify(op):
    for prefix, cls in CLASSES:
        if op.startswith(prefix):
            return cls
    return "other"


def build_flags():
    """CXXFLAGS (+ the per-file additions) of pytorch-attention_amd/build.py, read from that file so that the two cannot drift apart."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mi355_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_isa(src):
    """The device-only assembly listing of one csrc file, compiled with build.py's flags in a temporary directory."""
    mod = build_flags()
    src = os.path.abspath(src)
    with tempfile.TemporaryDirectory(prefix="mfma_slots_") as tmp:
        out = os.path.join(tmp, "kernel.s")
        cmd = [mod.hipcc()] + mod.CXXFLAGS + mod.EXTRA_FLAGS.get(os.path.basename(src), []) + ["--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
        if r.returncode:
            sys.stderr.write(r.stderr)
            raise RuntimeError("hipcc failed on %s" % src)
        with open(out) as f:
            return f.read()


_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_BRANCH = re.compile(r"^s_c?branch\w*\s+([A-Za-z_.$][\w.$]*)")


def _kernel_lines(text, name):
    """[(kind, payload)] of one kernel: ('label', name) and ('ins', (opcode, full text)) in text order."""
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    out = []
    for l in lines[start + 1:]:
        s = l.strip()
        if not s or s.startswith((";", "//")):
            continue
        m = _LABEL.match(s)
        if m:
            if m.group(1).startswith(".Lfunc_end"):                    # not the first s_endpgm: blocks may be laid out behind it
                break
            out.append(("label", m.group(1)))
            continue
        if s.startswith("."):
            continue
        s = s.split(";")[0].strip()
        if not s:
            continue
        op = s.split()[0]
        out.append(("ins", (op, s)))
    return out


def kernel_names(text, substr):
    names = re.findall(r"^(_Z\w+):", text, re.M)
    return [n for n in names if substr in n]


def short_name(name):
    """f16 / bf16 and GELU / plain from the template arguments in the mangled name, where they are there."""
    m = re.search(r"I(DF16_|DF16b|f|Dh)?(?:Lb([01]))?E", name)
    if not m:
        return name
    t = {"DF16_": "f16", "DF16b": "bf16", "f": "f32", "Dh": "f16"}.get(m.group(1), "?")
    return t + ("" if m.group(2) is None else (", GELU" if m.group(2) == "1" else ", plain"))


def _price(cls_list):
    return sum(PRICE[c] for c in cls_list)


def bodies(text, name):
    """The bodies of one kernel, each a dict (see analyse)."""
    items = _kernel_lines(text, name)
    label_at = {p: i for i, (k, p) in enumerate(items) if k == "label"}
    is_mfma = [k == "ins" and classify(p[0]) == "mfma" for k, p in items]
    pre = [0]
    for f in is_mfma:
        pre.append(pre[-1] + int(f))
    loops, cuts = [], set()
    for i, (k, p) in enumerate(items):
        if k != "ins":
            continue
        if p[0] in ("s_endpgm", "s_branch"):                            # nothing falls through these
            cuts.add(i + 1)
        m = _BRANCH.match(p[1])
        if not m or m.group(1) not in label_at:
            continue
        j = label_at[m.group(1)]
        if j < i:
            loops.append((j, i))
        elif pre[j] - pre[i] >= 1:
            cuts.add(j)
    loop = max(loops, key=lambda ab: pre[ab[1]] - pre[ab[0]]) if loops else None
    if loop:
        cuts.update((loop[0], loop[1] + 1))
    edges = sorted(cuts | {0, len(items)})
    out = []
    for a, b in zip(edges, edges[1:]):
        if pre[b] - pre[a] < 2:
            continue
        ins = [(i, p) for i, (k, p) in enumerate(items[a:b], a) if k == "ins"]
        pos = [n for n, (i, p) in enumerate(ins) if classify(p[0]) == "mfma"]
        gaps = [[p for _, p in ins[pos[g] + 1:pos[g + 1]]] for g in range(len(pos) - 1)]
        in_loop = bool(loop) and loop[0] <= a and b <= loop[1] + 1
        head = [p for _, p in ins[:pos[0]]]
        tail = [p for _, p in ins[pos[-1] + 1:]]
        if in_loop:                                                     # the MFMA-free rest of the loop belongs to the boundary as well
            extra = [p for i, (k, p) in enumerate(items[loop[0]:loop[1] + 1], loop[0]) if k == "ins" and not (a <= i < b)
                     and not any(a2 <= i < b2 and pre[b2] - pre[a2] >= 2 for a2, b2 in zip(edges, edges[1:]))]
        else:
            extra = []
        out.append(_summarise(gaps, head + tail + extra, in_loop))
        out[-1]["after_last"] = [t for _, t in tail]                    # what the body's own text holds behind its last MFMA
        out[-1]["mfma_text"] = [ins[n][1][1] for n in pos]
    return out


def _summarise(gaps, boundary, in_loop):
    cls = [[classify(op) for op, _ in g] for g in gaps]
    cost = [PRICE["mfma"] + _price(c) for c in cls]
    special = [any(c in SPECIAL for c in cs) for cs in cls]
    counts = collections.Counter(c for cs in cls for c in cs)
    n_special_cost = sum(PRICE[c] for cs in cls for c in cs if c in SPECIAL)
    avg = (sum(cost) - n_special_cost) / max(1, len(gaps))
    return {
        "in_loop": in_loop,
        "dma": counts["dma"] > 0,
        "mfma": len(gaps) + 1,
        "gaps": len(gaps),
        "empty": sum(1 for g in gaps if not g),
        "hist": dict(sorted(collections.Counter(len(g) for g in gaps).items())),
        "counts": dict(counts),
        "sum_floor": sum(max(FLOOR, c) for c in cost),
        "sum_raw": sum(cost),
        "floor": FLOOR * len(gaps),
        "avg_plain": avg,                                               # priced cost per gap without DMA pieces and stores
        "bound": 4 * math.ceil(avg / 4) + 12,                           # what a gap without a DMA piece or a store may cost
        "max_plain": max([c for c, s in zip(cost, special) if not s] or [0]),
        "cost": cost,
        "special": special,
        "text": [[t for _, t in g] for g in gaps],
        "boundary_cost": _price([classify(op) for op, _ in boundary]),
        "boundary_n": len(boundary),
    }


def analyse(text, substr):
    """{kernel name: [body, ...]} for every kernel whose name contains `substr`.  A body: in_loop, dma (it issues LDS-DMA pieces), mfma, gaps,
    empty, hist {instructions in a gap: gaps}, counts {class: instructions}, sum_floor = sum of max(FLOOR, gap cost), sum_raw, floor,
    avg_plain, bound, max_plain (the costliest gap without a DMA piece or a store), cost / special / text per gap, boundary_cost / boundary_n."""
    return {n: bodies(text, n) for n in kernel_names(text, substr)}


def steady_state(bodies_):
    """The body a long stream spends its time in: inside the loop, issuing DMA pieces."""
    c = [b for b in bodies_ if b["in_loop"] and b["dma"]]
    if len(c) != 1:
        raise RuntimeError("expected one steady-state body, found %d" % len(c))
    return c[0]


def body_tag(b):
    return ("loop" if b["in_loop"] else "peeled") + (", DMA" if b["dma"] else ", no DMA")


COLS = ("valu", "trans", "nop", "scalar", "waitcnt", "lds", "dma", "store", "load", "other")


def report(res, top=8, out=sys.stdout):
    w = out.write
    w("prices (cycles): " + ", ".join("%s %d%s" % (k, v, "*" if k in ASSUMED else "") for k, v in PRICE.items()) + "; floor %d; * = assumed\n\n" % FLOOR)
    w("| kernel | body | MFMAs | sum max(%d, gap) | sum raw | floor | empty gaps | costliest plain gap / bound | boundary | %s |\n" % (FLOOR, " | ".join(COLS)))
    w("|---|---|---|---|---|---|---|---|---|" + "---|" * len(COLS) + "\n")
    for name, bs in res.items():
        for b in bs:
            w("| %s | %s | %d | %d | %d | %d | %d of %d | %d / %d | %d (%d instr.) | %s |\n" % (
                short_name(name), body_tag(b), b["mfma"], b["sum_floor"], b["sum_raw"], b["floor"], b["empty"], b["gaps"], b["max_plain"],
                b["bound"], b["boundary_cost"], b["boundary_n"], " | ".join(str(b["counts"].get(c, 0)) for c in COLS)))
    w("\ngap histogram (instructions in a gap: number of gaps)\n\n")
    for name, bs in res.items():
        for b in bs:
            w("- %s, %s: %s\n" % (short_name(name), body_tag(b), ", ".join("%d: %d" % kv for kv in b["hist"].items())))
    if top:
        w("\ncostliest gaps\n")
        for name, bs in res.items():
            for b in bs:
                w("\n%s, %s\n" % (short_name(name), body_tag(b)))
                order = sorted(range(b["gaps"]), key=lambda g: -b["cost"][g])[:top]
                for g in order:
                    w("  gap %3d  %3d cycles%s  %s\n" % (g, b["cost"][g], " (reserved)" if b["special"][g] else "",
                                                        "; ".join(t.split()[0] for t in b["text"][g])))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--src", default=os.path.join(PKG, "csrc", "gemm16_wst.hip"))
    ap.add_argument("--kernel", default="gemm16_wst1_kernel", help="substring of the (mangled) kernel name")
    ap.add_argument("--isa", default=None, help="read this listing instead of compiling --src")
    ap.add_argument("--top", type=int, default=8, help="how many of the costliest gaps to list per body")
    a = ap.parse_args()
    if a.isa:
        with open(a.isa) as f:
            text = f.read()
    else:
        text = compile_isa(a.src)
    res = analyse(text, a.kernel)
    if not res:
        sys.exit("no kernel name contains %r" % a.kernel)
    report(res, top=a.top)


if __name__ == "__main__":
    main()
