"""CPU tests (-m "not gpu") of XCiT on any head width (xca_any_kernel of csrc/xcit.hip, class_attn_any_kernel of csrc/cls_attn.hip):
the case table of tests/xca_any_cases.py is well formed, the arena rows are registered for each entry at each precision, the header
documents the 1..256 envelope of the three entries, and -- where a reference checkout is present -- the fp64 oracle of every module row
equals the real reference module in .eval()."""
import importlib.util
import os
import re

import pytest
import torch

import arena_cases
import xca_any_arena_rows
import xca_any_cases as X
from conftest import ROOT, max_abs_ratio

REFERENCE = os.environ.get("MI355_REFERENCE", "/root/reference")


def test_case_table_is_well_formed():
    new_kernel = X.CORE + X.MASK + [X.ZERO_CHANNEL] + X.BATCH_INDEPENDENCE + X.CLASS_ATTN + X.ARENA_XCA + X.ARENA_CLASS_ATTN
    for B, N, h, d in new_kernel:
        assert B >= 1 and N >= 1 and h >= 1 and 1 <= d <= X.D_MAX, (B, N, h, d)
        assert d not in X.TEMPLATE_WIDTHS, f"d = {d}: a template kernel takes this width; the row would not reach the new kernel"
        assert B * N * 3 * h * d <= 200000, "every case stays small: at most 2 x 196 x 3 x 128 elements"
    widths = {c[3] for c in X.CORE}
    assert any(d % 4 for d in widths) and any(d > 128 for d in widths) and 1 in widths and X.D_MAX in widths
    assert any(d % 8 and not d % 4 for d in widths), "a width with 16-byte fp32 accesses and element-wise 16-bit accesses"
    assert any(d > 64 and N > 32 for _, N, _, d in X.CORE), "more than one row block and more than one chunk"
    assert {c[3] for c in X.MASK} == {24, 5} and X.ZERO_CHANNEL[3] == 24 and {c[3] for c in X.BATCH_INDEPENDENCE} == {24, 72}
    assert all(c[0] == 3 for c in X.BATCH_INDEPENDENCE)
    assert set(X.ROUTING_TEMPLATE) == set(X.TEMPLATE_WIDTHS) and not set(X.ROUTING_ANY) & set(X.TEMPLATE_WIDTHS)
    assert X.ROUTING_REFUSED == X.D_MAX + 1
    for rid, row in X.MODULES.items():
        dim = row["args"][0] if "args" in row else row["kwargs"]["embed_dim"]
        heads = row["args"][1] if "args" in row else row["kwargs"]["num_heads"]
        assert dim % heads == 0 and dim // heads == row["d"] and dim % 4 == 0, rid
        assert row["d"] not in X.TEMPLATE_WIDTHS and row["d"] <= X.D_MAX, rid


def test_arena_rows_are_registered():
    rows = [arena_cases.BY_ID[i] for i in xca_any_arena_rows.IDS]
    assert len(rows) == len(set(xca_any_arena_rows.IDS)) and all(r in arena_cases.ROWS for r in rows)
    for B, N, h, d in X.ARENA_XCA:
        sid = f"{B}x{N}x{h}x{d}"
        mine = [r for r in rows if r["id"].endswith(tuple(f"{sid}_p{p}" for p in (0, 1, 2)))]
        assert sorted(r["prec"] for r in mine if r["entries"] == ("mi355_xca_fwd",)) == [0, 1, 2]
        x16 = [r for r in mine if r["entries"] == ("mi355_xca16_fwd",)]
        assert sorted(r["prec"] for r in x16 if "from32" in r["id"]) == [1, 2] and sorted(r["prec"] for r in x16 if "from32" not in r["id"]) == [1, 2]
        assert all(r["tol"] == arena_cases.TOL[r["prec"]] and r["tags"][0].startswith(f"xca_any_kernel<d={d}") for r in mine)
        assert all(("in16" in r["tags"][0]) == (r in x16 and "from32" not in r["id"]) for r in mine)
    for B, N, h, d in X.ARENA_CLASS_ATTN:
        r = arena_cases.BY_ID[f"class_attn_any_{B}x{N}x{h}x{d}"]
        assert r["entries"] == ("mi355_class_attn_fwd",) and r["tol"] == arena_cases.TOL[0] and r["tags"] == (f"class_attn_any_kernel<d={d}",)


def test_header_documents_the_envelope():
    text = open(os.path.join(ROOT, "include", "mi355attn.h")).read()
    for entry, dim in (("mi355_xca_fwd", "d"), ("mi355_xca16_fwd", "d"), ("mi355_class_attn_fwd", "head_dim")):
        at = text.index(f"int {entry}(")
        comment = text[text.rindex("/*", 0, at):at]
        if entry == "mi355_xca16_fwd":                          # "as above": its comment names the range and points at mi355_xca_fwd
            assert "as above" in comment
        assert re.search(rf"1 <= {dim} <= {X.D_MAX}", comment), entry
    src = open(os.path.join(ROOT, "pytorch-attention_amd", "csrc", "xcit.hip")).read()
    assert f"XCA_ANY_MAX = {X.D_MAX}" in src and "1 <= d <= 256" in src and "known gap" in src
    src = open(os.path.join(ROOT, "pytorch-attention_amd", "csrc", "cls_attn.hip")).read()
    assert f"CLS_ANY_MAX = {X.D_MAX}" in src


def test_dispatch_keeps_the_template_widths():
    """The host dispatch sends exactly 32 / 48 / 64 to the template kernels and refuses nothing else up to the maximum."""
    src = open(os.path.join(ROOT, "pytorch-attention_amd", "csrc", "xcit.hip")).read()
    assert src.count("if (d != 32 && d != 48 && d != 64) {") == 2 and src.count("d < 1 || d > XCA_ANY_MAX") == 2
    assert "built: 32, 48, 64" not in src


def _reference_xcit():
    path = os.path.join(REFERENCE, "vision_transformers", "xcit.py")
    if not os.path.exists(path):
        pytest.skip("no reference checkout (MI355_REFERENCE)")
    spec = importlib.util.spec_from_file_location("reference_xcit", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("rid", list(X.MODULES))
def test_oracle_equals_the_reference_module(rid):
    row = X.MODULES[rid]
    m, x = X.build(rid, namespace=_reference_xcit())
    ours, x2 = X.build(rid)
    assert torch.equal(x, x2)
    sd, sd2 = m.state_dict(), ours.state_dict()
    assert sd.keys() == sd2.keys() and all(torch.equal(sd[k], sd2[k]) for k in sd), "the drop-in draws other parameters"
    with torch.no_grad():
        want = m(x, *row.get("fwd_args", ()))
    got = row["oracle"](x, {k: v.detach().clone() for k, v in sd.items()}, torch.float64)
    ratio = max_abs_ratio(got, want)
    print(f"[xca_any] {rid}: oracle (fp64) vs the reference module (fp32): max-abs ratio {ratio:.1e}")
    assert tuple(got.shape) == tuple(want.shape) and ratio <= 2e-5      # fp32 rounding of the reference's own forward (the strict bar's scale)
