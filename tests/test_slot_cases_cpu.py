"""CPU tests of tests/slot_cases.py, the cases of tests/test_slot_ladder_gpu.py:

  * the ladders, predicates and launch tables `choice` restates are the ones in csrc/ (read from the source text);
  * every single-read instantiation in the built library is reached by a case or listed in UNREACHABLE with its reason;
  * every nv, every bucket top and every CBAM class has a case, for every operator and I/O type;
  * the three input constructions have, in the fp64 oracle alone, the properties they are named for;
  * the oracle evaluated in fp32 stays within a quarter of the bar the GPU test applies, so the bars are reachable."""
import collections
import os
import re
import sys

import pytest
import torch

import slot_cases as S
from conftest import PKG, ROOT, max_abs_ratio, rel_fro

CSRC = os.path.join(PKG, "csrc")
PAIRS = [(op, io) for op in S.OPS for io in S.IOS]
F64 = torch.float64


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _between(text, start, end):
    a = text.index(start)
    return text[a:text.index(end, a)]


def if_ladder(body, call):
    """Buckets of `if (nv <= a) CALL a ...; else if (nv <= b) CALL b ...; else CALL z ...`: every bound picks its own bucket."""
    steps = re.findall(r"if \(nv <= (\d+)\) %s(\d+)" % call, body)
    last = re.findall(r"else %s(\d+)" % call, body)
    assert steps and len(last) == 1, (steps, last)
    assert all(a == b for a, b in steps), steps
    assert len(re.findall(r"nv <= \d+", body)) == len(steps), "a rung of the ladder was not understood"
    return tuple(int(a) for a, _ in steps) + (int(last[0]),)


def ternary_ladder(line):
    """Buckets of `nv <= a ? a : (nv <= b ? b : ... z)`."""
    steps = re.findall(r"nv <= (\d+) \? (\d+)", line)
    last = re.search(r": (\d+)\)*; }", line)
    assert steps and last and all(a == b for a, b in steps), line
    return tuple(int(a) for a, _ in steps) + (int(last.group(1)),)


def switch_ladder(body):
    cases = [int(v) for v in re.findall(r"case (\d+):", body)]
    default = re.findall(r"default:[^\n]*?(\d+)(?:, EXTRA)?[>)]", body)
    assert cases and len(default) == 1, (cases, default)
    return tuple(cases) + (int(default[0]),)


# ---- the restatement is the source's ---------------------------------------------------------------------------------------------------
def test_fp32_ladders_match_the_source():
    fused, stat = _src("chan_fused.hip"), _src("chan_stat.hip")
    for key, got in ((("se", 32), if_ladder(_between(fused, "static void se_launch_nv(", "\n}\n"), r"se_launch<")),
                     (("eca", 32), if_ladder(_between(fused, "int eca_single(", "#undef GO"), r"GO\(")),
                     (("stat", 32), if_ladder(_between(stat, "static void single(", "#undef GO"), r"GO\("))):
        assert got == S.LADDERS[key], f"the source's ladder of {key} is {got}, slot_cases.LADDERS has {S.LADDERS[key]}: move the cases with it"
    # what the occupancy-3 branch of se_launch builds: non-temporal stores only, and only below 14 chunks per lane
    launch = _between(fused, "static void se_launch(", "\n}\n")
    assert "if constexpr (NV <= 13) {" in launch
    assert re.findall(r"se_single_kernel<NV, (\w+), (\w+), 3, EXTRA>", launch) == [("true", "true"), ("true", "false")]
    assert sorted(re.findall(r"se_single_kernel<NV, (\w+), (\w+), 2, EXTRA>", launch)) == sorted((a, b) for a in ("true", "false") for b in ("true", "false"))


def test_16bit_ladders_match_the_source():
    io16, stat16 = _src("chan_io16.hip"), _src("chan_stat_io16.hip")
    for text, fn, key in ((io16, "se16_nv", ("se", 16)), (io16, "eca16_nv", ("eca", 16)), (stat16, "stat16_nv", ("stat", 16))):
        line = next(l for l in text.splitlines() if l.startswith("constexpr int %s(int nv)" % fn))
        assert ternary_ladder(line) == S.LADDERS[key], f"{fn} is {ternary_ladder(line)}, slot_cases.LADDERS has {S.LADDERS[key]}"
    # the launch tables switch over the same functions and name every bucket
    assert switch_ladder(_between(io16, "static void se16_go_nv(", "\n}\n")) == S.LADDERS["se", 16]
    assert "switch (se16_nv(nv))" in io16 and "switch (eca16_nv(nv))" in io16 and "switch (stat16_nv(nv))" in stat16
    assert switch_ladder(_between(io16, "#define GO_IO(IO_)", "BY_IO(io, GO_IO);")) == S.LADDERS["eca", 16]
    assert switch_ladder(_between(stat16, "void go_single(", "\n}\n")) == S.LADDERS["stat", 16]


def test_cbam_launch_tables_match_the_source():
    for name, kern in (("cbam_single.hip", "cbam_single_kernel<512, "), ("chan_io16.hip", "cbam16_single_kernel<IO_, ")):
        text = _src(name)
        body = _between(text, "#define GO(%sSEG_, NV_)" % ("IO_, " if "16" in name else ""), "#undef GO")
        pairs = {(int(a), int(b)) for a, b in re.findall(r"GO\((?:IO_, )?(\d+), (\d+)\)", body)}
        pairs |= {(int(a), int(b)) for a, b in re.findall(re.escape(kern) + r"(\d+), (\d+), true>", body)}
        assert pairs == {(s, n) for s in S.CBAM_SEGS for n in S.CBAM_NVS}, (name, pairs)
    # the 16-bit table names NV = 16 with FULL alone
    assert len(re.findall(r"cbam16_single_kernel<IO_, (?:16|32), 16, true>", _src("chan_io16.hip"))) == 2


def test_cited_lines_hold_the_restated_predicates():
    files = {}
    for name, line, text in S.CITED:
        lines = files.setdefault(name, _src(name).splitlines())
        assert text in lines[line - 1], f"csrc/{name}:{line} is now {lines[line - 1].strip()!r}, slot_cases.choice restates {text!r}"
    opts = _src("options.h")
    for key, val in S.DEFAULTS.items():
        assert re.search(r'MI355_OPT\(\w+, "%s", %d,' % (key, val), opts), key


def test_tags_in_the_source_end_with_the_template_arguments():
    """The eight launch sites file their launch under the tag `choice` predicts: kernel name first, template arguments last."""
    want = {
        "chan_fused.hip": ['"se_single_kernel C=%d HW=%d nv=%d NV=%d occ=%d wlds=%d extra=%d nts=%d"', '"eca_halo_kernel C=%d HW=%d k=%d nv=%d NV=%d nts=%d"'],
        "chan_stat.hip": ['"stat_single_kernel mode=%d C=%d HW=%d nv=%d NV=%d nts=%d"'],
        "cbam_single.hip": ['"cbam_single_kernel C=%d H=%d W=%d ks=%d SEG=%d NV=%d full=%d"'],
        "chan_io16.hip": ['"se16_single_kernel io=%d C=%d HW=%d nv=%d NV=%d wlds=%d extra=%d"', '"eca16_halo_kernel io=%d C=%d HW=%d k=%d nv=%d NV=%d"',
                          '"cbam16_single_kernel io=%d C=%d H=%d W=%d ks=%d SEG=%d NV=%d full=%d"'],
        "chan_stat_io16.hip": ['"stat16_single_kernel io=%d mode=%d C=%d HW=%d nv=%d NV=%d"'],
    }
    for name, fmts in want.items():
        text = _src(name)
        for f in fmts:
            assert text.count("MI355_TRACE(st, " + f) == 1, (name, f)
    for c in S.all_cases():
        ch = c.choice()
        assert S.inst_of_tag(ch.tag) == S.inst(ch), (c.id, ch)
    assert S.inst_of_tag("scale16_kernel io=1 HW=64") is None


# ---- coverage --------------------------------------------------------------------------------------------------------------------------
def test_every_compiled_instantiation_is_reached_or_excluded(built_lib):
    pytest.importorskip("msgpack")                                     # tools/kernel_resources.py decodes the metadata notes with it
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    compiled = set()
    for r in kernel_resources.kernels(built_lib):
        for k in S.KERNELS:
            m = re.search(r"\b%s<([^>]*)>" % k, r["demangled"])
            if m:
                compiled.add((k, m.group(1)))
    reached = {(k, S.targs_text(t)) for k, t in S.reachable()}
    excluded = {(k, S.targs_text(t)) for k, t in S.UNREACHABLE}
    assert all(S.UNREACHABLE.values()), "every excluded instantiation names the host line that excludes it"
    for k in S.KERNELS:
        n = lambda s: sum(1 for kk, _ in s if kk == k)
        print(f"[slots] {k}: {n(compiled)} compiled, {n(reached)} reached by a case, {n(excluded)} listed unreachable")
    assert not reached & excluded, sorted(reached & excluded)
    assert reached <= compiled, f"cases expect bodies the library does not hold: {sorted(reached - compiled)}"
    assert excluded <= compiled, f"UNREACHABLE lists bodies the library does not hold: {sorted(excluded - compiled)}"
    left = compiled - reached - excluded
    assert not left, f"compiled, but neither reached by a case nor listed in UNREACHABLE: {sorted(left)}"


@pytest.mark.parametrize("op,io", PAIRS)
def test_every_slot_count_and_class_has_a_case(op, io):
    cs = S.cases(op, io)
    bits = 32 if io == "fp32" else 16
    if op == "cbam":
        classes = collections.Counter(c.choice().targs[-3:] for c in cs if c.ks == 7)
        want = {(s, n, f) for s in S.CBAM_SEGS for n in S.CBAM_NVS for f in (True, False) if bits == 32 or f or n != 16}
        assert set(classes) == want and len(want) == (12 if bits == 32 else 10)
        assert all(v == 2 for v in classes.values())                   # one band and several bands per image
        assert {c.choice().targs[-3] for c in cs if c.ks == 3} == set(S.CBAM_SEGS)
        for c in cs:
            g = S.geometry(c.C, c.Cr, c.H, c.W, c.ks, bits == 16)
            assert g.Q in (12, 20) and g.Q < g.SEG and (g.NB > 1) == c.kind.endswith("-bands"), (c.id, g)
        return
    ladder = S.LADDERS[op if op in ("se", "eca") else "stat", bits]
    plain = [c for c in cs if not c.opts and not c.extra and c.C == S.C_ROWS]
    ragged = {c.choice().nv: c for c in plain if c.kind.startswith("ragged")}
    assert sorted(ragged) == list(range(1, S.MAX_NV[bits] + 1))
    for nv, c in ragged.items():
        assert c.H * c.W // S.EPC[bits] == 64 * (nv - 1) + 5 and c.B == 3 and c.C == 16
    full = {c.choice().nv for c in plain if c.kind.startswith("full")}
    assert full == set(ladder) and all(c.H * c.W // S.EPC[bits] == 64 * c.choice().nv for c in plain if c.kind.startswith("full"))
    assert {c.choice().nv for c in cs if c.options == dict(nt=1) and not c.extra and c.C == S.C_ROWS} == set(ladder)
    if op == "eca":
        assert all(c.ks == 3 for c in cs)                              # pad 1: the halo crosses the slice boundary and both zero pads
    if op == "se":
        tops = lambda pred: {c.choice().NV for c in cs if pred(c)}
        assert tops(lambda c: c.extra and c.C == S.C_ROWS) == set(ladder)                          # the EXTRA body at every bucket top
        wide = S.smallest_unstaged_c(io)
        assert S.choice("se", io, wide - 8, (wide - 8) // 16, 16, 16).targs[2] is True   # the smallest such C
        assert tops(lambda c: c.C == wide and not c.choice().targs[2]) == set(ladder)
        if bits == 32:
            assert wide * (wide // 16) > 6144 >= (wide - 8) * ((wide - 8) // 16)
            assert tops(lambda c: c.options.get("se_occ") == 2 and c.choice().targs[3] == 2 and c.choice().NV <= 13) == set(ladder) - {16}
            corner = [c for c in cs if c.kind.startswith("ldscorner")]
            assert len(corner) == 1 and (corner[0].C, corner[0].Cr) == (768, 8) and corner[0].choice().targs[3] == 2 and not corner[0].opts


def test_general_form_outside_the_envelope():
    """`choice` says None where the host takes the general form: switched off, ragged rows, too many chunks, 16 partly filled CBAM slots."""
    assert S.choice("se", "fp32", 16, 4, 4, 5, options=dict(se_single=0)) is None
    assert S.choice("se", "fp32", 16, 4, 3, 3) is None and S.choice("se", "fp16", 16, 4, 2, 2) is None
    assert S.choice("eca", "fp32", 12, 0, 4, 4, 3) is None and S.choice("eca", "fp32", 16, 0, 4, 4, 11) is None
    assert S.choice("gctg", "fp32", 16, 0, 4, 16 * 64 + 1) is None and S.choice("gctg", "bf16", 16, 0, 8, 8 * 64 + 1) is None
    assert S.choice("cbam", "fp32", 509, 31, 6, 8, 7) is not None and S.choice("cbam", "fp16", 509, 31, 6, 8, 7) is None
    assert S.choice("cbam", "fp32", 513, 32, 6, 8, 7) is None and S.choice("cbam", "fp32", 64, 4, 5, 5, 7) is None
    assert S.choice("se", "fp32", 16, 4, 16, 16 * 16).targs == (16, True, True, 2, False)          # 16 chunks per lane: two per CU
    assert S.choice("se", "fp32", 16, 4, 16, 16, options=dict(nt=1)).targs == (1, True, True, 3, False)   # three per CU keeps NT stores
    assert S.choice("se", "fp32", 8 * 513, 256, 4, 4, cus=256) is None and S.choice("se", "fp32", 8 * 512, 256, 4, 4, cus=256) is not None


# ---- the constructions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,io", PAIRS)
def test_constructions_hold_their_properties(op, io):
    epc = S.EPC[32 if io == "fp32" else 16]
    for c in S.cases(op, io):
        if c.C > 64 and op == "se" and c.kind not in ("full1", "full16", "full8", "ldscorner2"):
            continue                                                    # the wide SE variants share one builder: first and last bucket suffice
        HW = c.H * c.W
        sp, pl = (S.make_input(c, k).double().reshape(c.B, c.C, HW) for k in ("spread", "planted"))
        assert sp.dtype == F64 and S.make_input(c, "spread").dtype == c.dtype
        assert float(sp.mean(dim=2).abs().max()) <= 2.0 + 5.0 / HW ** 0.5 and float(sp.mean(dim=2).std()) > 0.8     # offsets spread the row means
        lo, hi = S.planted_at(c)
        assert lo // epc == 0 and hi // epc == HW // epc - 1
        body = pl[:-1]
        assert torch.equal(body.argmax(dim=2)[:, 0::2], torch.full_like(body.argmax(dim=2)[:, 0::2], lo)), c.id
        assert torch.equal(body.argmax(dim=2)[:, 1::2], torch.full_like(body.argmax(dim=2)[:, 1::2], hi)), c.id
        top2 = body.topk(2, dim=2).values
        assert float((top2[..., 0] - top2[..., 1]).min()) > 1.0, c.id    # the planted value is the row maximum, by a margin
        assert float(pl[-1].max()) <= -0.0125, c.id                         # the last image is negative throughout
        if op in S.PLACE_OPS and not c.extra and not c.opts:
            x = S.make_input(c, "place")
            assert x.dtype == c.dtype and torch.isfinite(x.float()).all()
            rows = x.reshape(c.B * c.C, HW)
            if io == "fp32":
                assert x.unique().numel() == x.numel(), c.id
            else:
                srt = rows.float().sort(dim=1).values
                assert bool((srt[:, 1:] > srt[:, :-1]).all()), c.id     # no repeated value inside a row after rounding to the I/O type
                assert len({tuple(r[:2].tolist()) for r in rows.float()}) == rows.shape[0], c.id   # rows start at different values
            k = S.PLACE_GATE[op]
            ref = S.oracle(c, x, S.place_params(c), F64)
            assert torch.equal(ref, x.double() * k), c.id                # the oracle's gate is exactly the stated constant
            assert torch.equal((x.double() * k).to(c.dtype).double(), x.double() * k), c.id   # ... and the product is exact in the I/O type


@pytest.mark.parametrize("op,io", PAIRS)
def test_fp32_oracle_stays_within_a_quarter_of_the_bar(op, io):
    """The GPU test's bars (assert_parity 1e-5 / 2e-5 in fp32; u |ref| + 1e-5 max|ref| per element in 16 bit) against the fp64 oracle are
    reachable by fp32 arithmetic on these inputs: the oracle run in fp32 uses at most a quarter of the fp32 allowance."""
    worst = 0.0
    for c in S.cases(op, io):
        p = S.case_params(c)
        for kind in ("spread", "planted"):
            x = S.make_input(c, kind)
            r64, y32 = S.oracle(c, x, p, F64), S.oracle(c, x, p, torch.float32)
            assert y32.dtype == torch.float32 and torch.isfinite(y32).all()
            if io == "fp32":
                use = max(rel_fro(y32, r64), max_abs_ratio(y32, r64)) / S.TOL32[op]
            else:
                use = float((y32.double() - r64).abs().max() / (S.T32_IO16 * r64.abs().max()))
            worst = max(worst, use)
            assert use <= 0.25, f"{c.id} {kind}: the fp32 oracle uses {use:.3f} of the bar"
    print(f"[slots] {op} {io}: the fp32 oracle uses at most {worst:.4f} of the bar")
