"""CPU tests (-m "not gpu") of SKLayer on every planes / groups (csrc/sk_wide.hip behind mi355_sk_fwd): the case table of
tests/sk_wide_cases.py is well formed, its oracle equals the real reference's SKLayer on every row (where a reference checkout is
present), the arena rows are registered, the new workspace query is declared, exported and bound, and its values relate to the old
query as the header says."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

import arena_cases
import sk_wide_arena_rows
import sk_wide_cases as S
from conftest import PKG, ROOT, max_abs_ratio

REFERENCE = os.environ.get("MI355_REFERENCE", "/root/reference")
FMA_WIDTHS = (1, 2, 4, 8, 16)


def test_case_table_is_well_formed():
    ids = [c[0] for c in S.CASES + S.COVERED]
    assert len(ids) == len(set(ids)) and len(S.CASES) >= 10
    for cid, (Cin, planes), groups, shape, why in S.CASES + S.COVERED:
        assert Cin % groups == 0 and planes % groups == 0 and shape[1] == Cin and why, cid
        assert max(planes // 16, 32) + planes <= 12288, cid
    for cid, (_, planes), groups, *_ in S.CASES:
        assert planes // groups not in FMA_WIDTHS, f"{cid}: the FMA kernels take this width; the row would not reach the new kernel"
    for cid, (_, planes), groups, *_ in S.COVERED:
        assert planes // groups in FMA_WIDTHS, cid


def test_perturbation_leaves_no_identity_term():
    m = S.module(S.BY_ID["g3x5"])
    for seq in (m.split_3x3, m.split_5x5):
        conv, bn = seq[0], seq[1]
        assert float(conv.bias.detach().abs().min()) > 0 and float((bn.weight.detach() - 1).abs().min()) > 0 and float(bn.bias.detach().abs().min()) > 0
        assert float(bn.running_mean.abs().min()) > 0 and float((bn.running_var - 1).abs().min()) > 0
    assert float(m.fc[1].running_mean.abs().min()) > 0 and float(m.fc1.bias.detach().abs().min()) > 0 and float(m.fc2.bias.detach().abs().min()) > 0
    a, b = S.module(S.BY_ID["g3x5"]), S.input_of(S.BY_ID["g3x5"])
    assert all(torch.equal(p, q) for p, q in zip(m.state_dict().values(), a.state_dict().values()))      # deterministic
    assert torch.equal(b, S.input_of(S.BY_ID["g3x5"]))


def _reference_module(name):
    path = os.path.join(REFERENCE, "attention_mechanisms", name + ".py")
    if not os.path.exists(path):
        pytest.skip("no reference checkout (MI355_REFERENCE)")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("cid", S.IDS + S.COVERED_IDS)
def test_oracle_equals_the_reference_sklayer(cid):
    case = S.BY_ID[cid]
    ref_cls = _reference_module("sk_module").SKLayer
    m = S.module(case, cls=ref_cls)
    ours = S.module(case)
    assert all(torch.equal(p, q) for p, q in zip(m.state_dict().values(), ours.state_dict().values())), "the drop-in draws other parameters"
    x = S.input_of(case)
    with torch.no_grad():
        want = m(x)
    got = S.truth(case)
    d = float((got - want.double()).abs().max())
    print(f"[sk_wide] {cid}: oracle (fp64) vs the reference module (fp32): max-abs {d:.1e}, max-abs ratio {max_abs_ratio(got, want):.1e}")
    assert d <= 1e-6


def test_arena_rows_are_registered():
    ids = set(sk_wide_arena_rows.IDS)
    assert {"sk_wide_g32x32_ragged", "sk_wide_chunked_512", "sk_wide_g3x5", "sk_wide_covered_ragged"} <= ids
    rows = [arena_cases.BY_ID[i] for i in sk_wide_arena_rows.IDS]
    assert all(r in arena_cases.ROWS and r["entries"] == ("mi355_sk_fwd",) and r["tol"] == arena_cases.TOL[0] for r in rows)
    assert [r["id"] for r in rows if r["opts"].get("sk_wide") == 1] == ["sk_wide_covered_ragged"]
    assert all(S.WIDE_TAG in r["tags"] for r in rows)


def test_sk_ws_bytes_declared_exported_and_bound(built_lib):
    import mi355attn._ffi as ffi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355attn.h")).read(), flags=re.S)
    proto = re.search(r"\bsize_t\s+mi355_sk_ws_bytes\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert proto, "mi355_sk_ws_bytes is not declared in mi355attn.h"
    assert [a.split()[0] for a in proto.group(1).split(",")] == ["int"] * 6
    assert hasattr(ctypes.CDLL(built_lib), "mi355_sk_ws_bytes"), "mi355_sk_ws_bytes is not exported by the library"
    assert ffi.SIGNATURES["mi355_sk_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 6)
    assert ffi.SIGNATURES["mi355_sk_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)           # stays
    assert ffi.lib().mi355_version() == 1                              # additions only: the ABI version stays


def test_sk_workspace_queries(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()

    def fl(n):
        return (n + 63) & ~63
    for cid in S.IDS + S.COVERED_IDS:
        _, (Cin, planes), groups, (B, _, H, W), _ = S.BY_ID[cid]
        old = lib.mi355_sk_workspace_bytes(B, planes, H, W)
        assert old == 4 * (2 * fl(B * planes * H * W) + fl(B * planes * H) + fl(B * 2 * planes)) + 256, cid      # unchanged values
        new = lib.mi355_sk_ws_bytes(B, Cin, planes, groups, H, W)
        cogp = (planes // groups + 15) & ~15
        # at least both branches' weights as bf16 hi / lo pairs at the padded output width, and one pooled sum per (image, channel)
        assert new >= old + 2 * 2 * 2 * groups * cogp * 9 * (Cin // groups) + 4 * B * planes, cid
        assert new % 16 == 0
    for args in ((0, 64, 64, 2, 7, 7), (2, 0, 64, 2, 7, 7), (2, 64, 64, 0, 7, 7), (2, 64, 64, 2, 0, 7), (2, 64, 64, 2, 7, -1),
                 (2, 64, 64, 3, 7, 7), (2, 63, 64, 3, 7, 7)):
        assert lib.mi355_sk_ws_bytes(*args) == 0, args


def test_option_is_listed_with_default_off():
    src = open(os.path.join(PKG, "csrc", "options.h")).read()
    assert re.search(r'^MI355_OPT\(SK_WIDE,\s*"sk_wide",\s*0,\s*0,\s*1\)', src, flags=re.M)
