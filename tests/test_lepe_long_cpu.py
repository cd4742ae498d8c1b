"""CPU tests of the long-window LePE core (stripe windows of 225 .. 512 tokens, win_attn_long_kernel of csrc/attn.hip):

  * the fp64 oracle (oracle/cswin.py) is pinned to the real reference at the new shapes through tests/golden/lepe_long.json, written by
    tests/golden/make_lepe_long.py from the reference run in fp64: every LePEAttention window of tests/lepe_long_cases.py, the two
    CSWinBlocks and the 384 px model.  The modules are built here from the drop-in classes under the same seed protocol, so the test also
    holds their constructor arguments and init stream to the reference's.  Bar: 1e-9 of the output's size on the 257 samples and the two
    checksums -- fp64 round-off over the longest sums here (512 keys, 1024 hidden units, 25 layers) is of order 1e-13, nothing else differs.
  * the three entries validate their arguments before any launch: null pointers -1, 529 tokens -2 (naming 512) without a pointer being
    read, 288 tokens with null pointers -1 and not -2;
  * every instantiation of the new kernel is in the built library with zero scratch and at most 163,840 B of LDS (all of it static: the
    kernel takes no dynamic LDS); the launch tag of the strict route holds no substring the route tests forbid there;
  * the arena rows of the three entries are registered.
"""
import json
import os
import re
import sys

import pytest
import torch

import lepe_long_arena_rows
import lepe_long_cases as LC
import oracle as O
from cases import sample_index
from conftest import ROOT

F64 = torch.float64
BAR = 1e-9


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "lepe_long.json")) as f:
        return json.load(f)["cases"]


def _check(rec, x, y, what):
    assert list(x.shape) == rec["x_shape"] and abs(float(x.double().sum()) - rec["x_sum"]) <= 1e-9 * max(1.0, abs(rec["x_sum"])), \
        f"{what}: the input does not follow the fixture's seed protocol"
    assert list(y.shape) == rec["y_shape"], f"{what}: {tuple(y.shape)} vs {rec['y_shape']}"
    yf = y.double().reshape(-1)
    want = torch.tensor(rec["samples"], dtype=F64)
    err = float((yf[sample_index(yf.numel())] - want).abs().max() / want.abs().max())
    s_err = abs(float(yf.sum()) - rec["sum"]) / rec["abs_sum"]
    a_err = abs(float(yf.abs().sum()) - rec["abs_sum"]) / rec["abs_sum"]
    print(f"[lepe_long oracle] {what}: samples {err:.2e} sum {s_err:.2e} abs_sum {a_err:.2e}")
    assert err <= BAR and s_err <= BAR and a_err <= BAR, f"{what}: samples {err:.3e}, sum {s_err:.3e}, abs_sum {a_err:.3e}"


def test_fixture_is_small_and_complete(fixture):
    want = ["lepe_" + LC.wid(c) for c in LC.WINDOWS] + ["block_" + r[0] for r in LC.BLOCKS] + ["model_384"]
    assert sorted(fixture) == sorted(want)
    assert all(len(r["samples"]) == 257 and set(r) == {"x_shape", "x_sum", "y_shape", "sum", "abs_sum", "samples"} for r in fixture.values())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "lepe_long.json")) < 256 << 10
    assert [LC.tokens(c) for c in LC.WINDOWS] == [225, 256, 288, 288, 300, 300, 512, 512]
    assert LC.tokens(LC.TOO_LONG) == 529 and LC.tokens(LC.SHORT_MAX) == 224


@pytest.mark.parametrize("case", LC.WINDOWS, ids=LC.wid)
def test_oracle_lepe_attention_matches_the_reference(case, fixture):
    from mi355attn.modules import LePEAttention
    reso, idx, split, dim, heads = case
    m, qkv = LC.lepe_inputs(LePEAttention, case)
    y = O.lepe_attention_forward(qkv.double(), m.get_v.weight, m.get_v.bias, reso, idx, split, heads, F64)
    _check(fixture["lepe_" + LC.wid(case)], qkv, y, "LePEAttention" + LC.wid(case))


@pytest.mark.parametrize("row", LC.BLOCKS, ids=lambda r: r[0])
def test_oracle_block_matches_the_reference(row, fixture):
    from mi355attn.modules import CSWinBlock
    m, x = LC.block_inputs(CSWinBlock, row)
    reso, heads, split = row[4]
    y = O.cswin_block_forward(x, LC.state(m), reso, heads, split, False, F64)
    _check(fixture["block_" + row[0]], x, y, "CSWinBlock " + row[0])


def test_oracle_model_384_matches_the_reference(fixture):
    from mi355attn.modules import CSWinTransformer
    m, x = LC.model_inputs(CSWinTransformer)
    kw = LC.MODEL_KW
    y = O.cswin_forward(x, LC.state(m), kw["embed_dim"], tuple(kw["depth"]), tuple(kw["split_size"]), tuple(kw["num_heads"]), F64)
    _check(fixture["model_384"], x, y, "CSWinTransformer 384 px")


# ---- argument validation, before any launch ---------------------------------------------------------------------------------------
def _entries(lib):
    """name -> call(ptr, reso, (Hsp, Wsp) or split) with one pointer value for every pointer argument; dim 32, one head, batch 1."""
    s = 32 ** -0.5
    return {
        "mi355_cswin_lepe_attn_fwd": lambda p, reso, hw, prec: lib.mi355_cswin_lepe_attn_fwd(p, p, p, p, 1, reso, 32, 0, 32, 1, hw[0], hw[1], s, prec, None),
        "mi355_cswin_lepe_attn16_fwd": lambda p, reso, hw, prec: lib.mi355_cswin_lepe_attn16_fwd(p, p, p, p, 1, reso, 32, 0, 32, 1, hw[0], hw[1], s, prec, None),
        "mi355_cswin_lepe_attn16_pair_fwd": lambda p, reso, hw, prec: lib.mi355_cswin_lepe_attn16_pair_fwd(p, p, p, p, p, p, 1, reso, 64, 1, hw[1], s, prec, None),
    }


def test_argument_validation_precedes_every_launch(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()
    for name, call in _entries(lib).items():
        for prec in (1, 2) if "16" in name else (0, 1, 2):
            assert call(None, 24, (24, 12), prec) == -1 and b"invalid argument" in lib.mi355_last_error(), (name, "288 tokens, null pointers")
            assert call(None, 23, (23, 23), prec) == -1, (name, "529 tokens, null pointers: the pointers are checked first")
            assert call(None, 8, (8, 2), prec) == -1, (name, "16 tokens, null pointers")
            # 529 tokens: refused as unsupported with the new limit in the text; 64 is no address of anything, it is never read
            assert call(64, 23, (23, 23), prec) == -2, (name, prec, lib.mi355_last_error())
            text = lib.mi355_last_error()
            assert b"529 tokens per stripe window > 512" in text and name.encode() in text, (name, text)
        assert call(64, 24, (24, 13), 1) == -1, (name, "a stripe that does not divide the grid")
        assert call(64, 0, (0, 0), 1) == -1, name
    assert _ffi.lib().mi355_version() == 1                             # no new entry, no prototype change: the ABI version stays


def test_header_states_the_new_envelope():
    src = open(os.path.join(ROOT, "include", "mi355attn.h")).read()
    for name in ("mi355_cswin_lepe_attn_fwd", "mi355_cswin_lepe_attn16_fwd", "mi355_cswin_lepe_attn16_pair_fwd"):
        at = src.index("int " + name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        assert "512" in comment, f"the comment in front of {name} does not state the 512-token envelope"


# ---- kernel metadata ------------------------------------------------------------------------------------------------------------
WANT = [(p, kt, io, 4 if (p == 0 and kt == 32) else 8) for p in (0, 1, 2) for kt in (20, 32) for io in (("false",) if p == 0 else ("false", "true"))]


def test_long_kernel_instantiations_have_no_scratch_and_fit_lds(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources                                            # needs msgpack: a missing package fails this test, it does not skip it
    rows = [r for r in kernel_resources.kernels(built_lib) if re.search(r"\bwin_attn_long_kernel<", r["demangled"])]
    names = [r["demangled"] for r in rows]
    for p, kt, io, nw in WANT:
        k = f"win_attn_long_kernel<{p}, {kt}, {io}, {nw}>"
        assert sum(k in n for n in names) == 1, f"no single instantiation {k} in {names}"
    assert len(rows) == len(WANT) == 10, names
    for r in rows:
        print(f"[lepe_long kernel] vgpr {r['vgpr']} agpr {r['agpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']}  {r['demangled'][:60]}")
        assert r["scratch"] == 0 and not r["spill_v"] and not r["spill_s"], (r["demangled"], r["scratch"], r["spill_v"], r["spill_s"])
        assert 0 < r["lds"] <= 163840, (r["demangled"], r["lds"])
        nw = int(re.search(r"win_attn_long_kernel<\d+, \d+, \w+, (\d+)>", r["demangled"]).group(1))
        assert r["vgpr"] + r["agpr"] <= (512 if nw == 4 else 256), (r["demangled"], r["vgpr"], r["agpr"])    # one workgroup per CU at least
    # the short kernel is still there for every launch at or below 224 tokens
    assert any(re.search(r"\bwin_attn_kernel<", r["demangled"]) for r in kernel_resources.kernels(built_lib))


def test_launch_tags_keep_the_grammar_and_the_strict_route_stays_clean():
    src = open(os.path.join(ROOT, "pytorch-attention_amd", "csrc", "attn.hip")).read()
    fmt = re.search(r'MI355_TRACE\(st, "(win_attn_long_kernel<[^"]*)"', src).group(1)
    assert fmt.startswith("win_attn_long_kernel<d=32,lepe%s> B=%d windows=%d heads=%d tokens=%d")
    forbidden = ("gemm16", "io16", "out16", "in16", "cast16", "mlp_fused", "mlp_wide", "cswin_stripe", "mixer_token", "layernorm16_t",
                 "ln_center16")                                          # STRICT_FORBIDDEN of tests/test_routes_gpu.py
    strict_tag = (fmt % ("", 2, 2, 4, 288))
    assert not [s for s in forbidden if s in strict_tag], strict_tag
    assert "win_attn_kernel<" not in strict_tag and ",io16>" in fmt % (",io16", 2, 2, 4, 288)


# ---- arena rows -----------------------------------------------------------------------------------------------------------------
def test_every_entry_has_arena_rows_at_both_windows_and_every_precision():
    import arena_cases
    assert len(lepe_long_arena_rows.IDS) == 14 and len(set(lepe_long_arena_rows.IDS)) == 14
    for name, precs in (("mi355_cswin_lepe_attn_fwd", {0, 1, 2}), ("mi355_cswin_lepe_attn16_fwd", {1, 2}),
                        ("mi355_cswin_lepe_attn16_pair_fwd", {1, 2})):
        rows = [r for r in arena_cases.ROWS if name in r["entries"] and r["id"] in lepe_long_arena_rows.IDS]
        assert len(rows) == 2 * len(precs) and {r["prec"] for r in rows} == precs, name
        assert {re.search(r"_(r\d+_s\d+)_p", r["id"]).group(1) for r in rows} == {"r24_s12", "r30_s10"}, name
        assert all(arena_cases.BY_ID[r["id"]] is r and r["tol"] == arena_cases.TOL[r["prec"]] for r in rows)
