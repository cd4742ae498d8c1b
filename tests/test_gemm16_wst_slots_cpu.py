"""The instruction stream of gemm16_wst1_kernel (gemm16_wst.hip) as hipcc compiles it: what sits between consecutive MFMAs of the steady-state
tile body (inside the loop, issuing DMA pieces) of each of the four instantiations, priced by tools/mfma_slot_budget.py.  The epilogue pieces
are placed by hand (WstPlan); this is the check that the compiler left them where the plan put them.  One compilation per session, about half
a minute."""
import math
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pytorch-attention_amd", "csrc", "gemm16_wst.hip")
# sum of max(16, gap cost) over the 191 gaps of the steady-state body before the pieces became inline assembly (profiles/gemm_wst_slots.md)
BEFORE = {"f16, GELU": 5868, "bf16, GELU": 5624, "f16, plain": 4508, "bf16, plain": 4268}
_CACHE = {}


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_slot_budget
    return mfma_slot_budget


@pytest.fixture(scope="module")
def isa():
    if "isa" not in _CACHE:
        _CACHE["isa"] = _tool().compile_isa(SRC)
    return _CACHE["isa"]


@pytest.fixture(scope="module")
def steady(isa):
    tool = _tool()
    res = tool.analyse(isa, "gemm16_wst1_kernel")
    assert sorted(tool.short_name(n) for n in res) == sorted(BEFORE), list(res)
    return {tool.short_name(n): tool.steady_state(bs) for n, bs in res.items()}


@pytest.mark.parametrize("inst", sorted(BEFORE))
def test_steady_state_body_has_192_mfmas(steady, inst):
    assert steady[inst]["mfma"] == 192 and steady[inst]["gaps"] == 191


@pytest.mark.parametrize("inst", sorted(BEFORE))
def test_no_plain_gap_far_above_the_average(steady, inst):
    """The tile boundary is no gap of the body.  A gap without a DMA piece or a store may cost 4 * ceil(a / 4) + 12 cycles, a = the body's
    priced cost per gap without its DMA pieces and stores."""
    tool, b = _tool(), steady[inst]
    reserved = sum(tool.PRICE[c] * b["counts"].get(c, 0) for c in tool.SPECIAL)
    a = (b["sum_raw"] - reserved) / 191
    bound = 4 * math.ceil(a / 4) + 12
    assert bound == b["bound"]
    worst = [(g, c, b["text"][g]) for g, (c, s) in enumerate(zip(b["cost"], b["special"])) if not s and c > bound]
    assert not worst, (inst, bound, worst[:4])


@pytest.mark.parametrize("inst", ["f16, GELU", "bf16, GELU"])
def test_few_empty_gaps_with_gelu(steady, inst):
    assert steady[inst]["empty"] <= 40, (inst, steady[inst]["empty"], steady[inst]["hist"])


@pytest.mark.parametrize("inst", sorted(BEFORE))
def test_priced_tile_at_least_8_percent_below_the_form_before(steady, inst):
    b = steady[inst]
    print(inst, "sum of max(16, gap):", b["sum_floor"], "raw:", b["sum_raw"], "before:", BEFORE[inst])
    assert b["sum_floor"] <= 0.92 * BEFORE[inst], (inst, b["sum_floor"], BEFORE[inst])


def test_no_register_copies_between_the_mfmas(isa):
    """The MFMAs are inline assembly, so the compiler pads nothing between one of them and a VALU copy of its result.  Copies belong where
    the tile bodies meet, behind the wait states that close a tile -- never inside a body, peeled or in the loop."""
    tool = _tool()
    for name, bs in tool.analyse(isa, "gemm16_wst1_kernel").items():
        assert len(bs) == 4, (name, len(bs))                           # the first tile of a stream and the loop, each with and without DMA pieces
        for b in bs:
            accs = set()                                                # the registers the body's MFMAs write
            for t in b["mfma_text"]:
                lo, hi = map(int, re.match(r"\S+\s+v\[(\d+):(\d+)\]", t).groups())
                accs.update(range(lo, hi + 1))

            def reads_acc(t):
                src = t.split(",", 1)[1]
                regs = [range(int(a), int(b or a) + 1) for a, b in re.findall(r"\bv\[?(\d+)(?::(\d+)\])?", src)]
                return any(r in accs for rg in regs for r in rg)
            moved = [t for g in b["text"] for t in g if t.startswith(("v_mov_", "v_accvgpr_", "v_pk_mov_")) and reads_acc(t)]
            assert not moved, (name, tool.body_tag(b), moved[:4])
            ops = [t.split()[0] + " " + t.split()[1] if t.startswith("s_nop") else t.split()[0] for t in b["after_last"]]
            assert "s_nop 11" in ops, (name, tool.body_tag(b), ops[:8])
            assert not any(o.startswith(("v_mov_", "v_accvgpr_", "v_pk_mov_")) for o in ops[:ops.index("s_nop 11")]), (name, ops[:8])


def test_dma_pieces_are_the_only_lines_that_name_m0(isa):
    """wst_dma_so / wst_dma_piece write m0 and do not restore it: right as long as nothing else in these kernels reads or writes it."""
    tool = _tool()
    for name in tool.kernel_names(isa, "gemm16_wst1_kernel"):
        lines = [t for k, (op, t) in ((k, p) for k, p in tool._kernel_lines(isa, name) if k == "ins") if re.search(r"\bm0\b", t)]
        other = [t for t in lines if not re.match(r"s_(mov_b32|add_u32) m0, ", t)]
        assert lines and not other, (name, other[:4])
