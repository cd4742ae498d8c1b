"""CPU tests (-m "not gpu") of the row-stride table tests/gemm_ld_cases.py: every entry of include/mi355attn.h with an ldx / ldy / ldu / lda
parameter has a row (or a stated reason); every entry of the table refuses a stride below the width with MI355_EINVAL and a stride off the
alignment its header states with MI355_EUNSUPPORTED, naming itself, before any HIP call (fake pointers, as tests/test_dual_io16_cpu.py uses
them); the table's strides keep the stated rules; the float64 references of the small rows are what the table says they are."""
import os
import re

import pytest
import torch

import gemm_ld_cases as G
from conftest import ROOT

P = 64                                      # a fake, 16-byte aligned, non-null pointer: never dereferenced
ISSUE_ENTRIES = {"mi355_linear_fwd", "mi355_gemm_bias_act_fwd", "mi355_linear16_fwd", "mi355_linear16_ws_fwd", "mi355_linear16_x32_fwd",
                 "mi355_linear16_stats_fwd", "mi355_linear16_ln16_fwd", "mi355_linear16_res_fwd", "mi355_linear16_tr_fwd", "mi355_ln_linear16_fwd",
                 "mi355_linear16_emit_fwd", "mi355_linear16_lnfold_fwd"}


def _entries_with_a_row_stride():
    """Header entry -> its leading-dimension parameters among ldx / ldy / ldu / lda, the names the GEMM entries use."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355attn.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(mi355_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        lds = re.findall(r"\b(?:int|long)\s+(ld[xyua])\b", m.group(2))
        if lds:
            out[m.group(1)] = lds
    return out


def test_every_header_entry_with_a_row_stride_has_a_row_or_a_reason():
    header = _entries_with_a_row_stride()
    assert len(header) >= 14 and ISSUE_ENTRIES <= set(header), sorted(header)
    rows = {r["entry"] for r in G.ROWS}
    assert not (rows | set(G.ELSEWHERE)) - set(header), "the table names an entry that has no ldx / ldy / ldu / lda parameter in the header"
    assert not rows & set(G.ELSEWHERE) and all(reason.strip() for reason in G.ELSEWHERE.values())
    missing = sorted(set(header) - rows - set(G.ELSEWHERE))
    assert not missing, f"header entries with a row-stride parameter and no row in tests/gemm_ld_cases.py: {missing}"
    for r in G.ROWS:                                                     # every stride parameter of the entry is one the row sets
        mine = {"lda" if (k == "ldx" and "lda" in header[r["entry"]]) else k for k in G.ld_keys(r)}
        assert mine == set(header[r["entry"]]), (r["id"], mine, header[r["entry"]])


def test_table_is_well_formed():
    import arena_cases
    assert G.TOL == arena_cases.TOL
    ids = [r["id"] for r in G.ROWS]
    assert len(ids) == len(set(ids)) and len(G.CASES) == len(set(G.CASES))
    for r in G.ROWS:
        assert r["precs"] == ((0, 1, 2) if r["kind"] == "linear32" else (1,) if r["kind"] == "qkv5" else (1, 2)), r["id"]
        assert r["bits"] or (r["ws"] and r["opts"]["gemm_splitk"] == 1), r["id"]          # only split-K may change bits
        assert r["tags"] and set(r.get("patterns", G.PATTERNS)) <= set(G.PATTERNS), r["id"]
        for p in r["precs"]:
            width = {b[4]: b[2] for b in G.buffers(r, p) if b[4] and G.PRIMARY[b[4]] == b[0]}
            assert G.strides(r, p, "dense") == width, r["id"]
            for pattern in r.get("patterns", G.PATTERNS):
                ld = G.strides(r, p, pattern)
                assert set(ld) == set(width) and any(ld[k] > width[k] for k in ld), (r["id"], pattern, ld)
                for k, a in G.RULES[r["kind"]].items():
                    assert ld[k] % a == 0, f"{r['id']} {pattern}: {k} = {ld[k]} is off the alignment the header states ({a})"
                if pattern == "block":
                    assert all(ld[k] == 3 * width[k] for k in ld), (r["id"], ld)
    # Row A: a 16-bit Y with ldy = 4 (mod 8) on the short-K product the weight-stationary kernel takes when dense
    a = G.BY_ID["ws_k64_out16_ldy4mod8"]
    assert a["out16"] == 1 and G.strides(a, 1, "pad")["ldy"] % 8 == 4 and a["dense_tags"] and a["shape"][2] == 64 and a["shape"][0] >= 2048
    # the scalar-store row and the small-kernel row of the fp32 engine
    assert G.strides(G.BY_ID["gemm32_scalar_store"], 0, "pad")["ldy"] == 133
    assert G.strides(G.BY_ID["gemm32_small"], 0, "pad") == {"ldx": 68, "ldy": 13}
    assert G.strides(G.BY_ID["ln16_256"], 1, "pad")["ldu"] != G.strides(G.BY_ID["ln16_256"], 1, "pad")["ldy"]


# an entry whose whole body forwards to another one reports under that entry's name (csrc/gemm16.hip, csrc/api.hip)
FORWARDS = {"mi355_linear16_fwd": b"mi355_linear16_ws_fwd", "mi355_gemm_bias_act_fwd": b"mi355_linear_fwd"}


def _fake(r, p):
    return {b[0]: P for b in G.buffers(r, p)}


@pytest.mark.parametrize("rid", [r["id"] for r in G.ROWS])
def test_entry_refuses_bad_strides_before_any_launch(rid, built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()
    r = G.BY_ID[rid]
    p = 0 if r["kind"] == "linear32" else 2       # bf16: an accepted call would not even touch the fp16 range word
    M, N, K = r["shape"]
    names = (r["entry"].encode(), FORWARDS.get(r["entry"], r["entry"].encode()))
    dense = G.strides(r, p, "dense")
    for key in dense:                                                    # ldx < K, ldy < N, ldu < N
        ld = dict(dense, **{key: dense[key] - 1})
        rc = G.invoke(lib, r, p, _fake(r, p), ld, None)
        text = lib.mi355_last_error()
        assert rc == G.EINVAL and text and b"invalid argument" in text and any(n in text for n in names), (rid, key, rc, text)
    for key, bad, a in G.misaligned(r):
        assert bad > dense[key] and bad % a, (rid, key, bad)
        ld = dict(dense, **{key: bad})
        rc = G.invoke(lib, r, p, _fake(r, p), ld, None)
        assert rc == G.EUNSUPPORTED, (rid, key, bad, rc, lib.mi355_last_error())
        if r["entry"] != "mi355_linear16_x32_fwd":                       # that entry declines without an error text (header): the caller falls back
            text = lib.mi355_last_error()
            assert text and any(n in text for n in names), (rid, key, text)


def test_forced_kernel_refuses_a_16_bit_y_with_rows_off_16_bytes(built_lib):
    """include/mi355attn.h, mi355_linear16_fwd: gemm_variant >= 15 forces a kernel that stores 16-byte units; a 16-bit Y at ldy % 8 == 4 is
    MI355_EUNSUPPORTED there (the default dispatch computes it on the plain tile kernels: row A of the GPU test)."""
    import mi355attn
    from mi355attn import _ffi
    lib = _ffi.lib()
    r = G.BY_ID["p8_out16_b"]
    with mi355attn.options(**r["opts"]):
        rc = G.invoke(lib, r, 2, _fake(r, 2), {"ldx": 256, "ldy": 516}, None)
        text = lib.mi355_last_error()
    assert rc == G.EUNSUPPORTED and b"ldy % 8 == 0" in text and b"ldy=516" in text, (rc, text)


@pytest.mark.parametrize("rid", ["tile_v1_out32_bgr_gelu", "res_r16_o32", "tr_3x68", "lnfold", "emit", "stats_256", "ln16_256", "lnlin_k64_out16"])
def test_reference_is_the_plain_formula(rid):
    """The float64 reference of a row, element by element from the header's formula, for one element of each output."""
    r = G.BY_ID[rid]
    p = 1
    d = G.make(r, p)
    ref = G.reference(r, p, d)
    M, N, K = r["shape"]
    m, n = M - 1, N - 3
    x, w = d["x"].double(), d["w"].double()
    if r["kind"] == "lnlin":
        mu = x.mean(-1, keepdim=True)
        x = (x - mu) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + G.LN_EPS)
    dot = float((x[m] * w[n]).sum())
    if r["kind"] == "lnfold":
        dot = float(d["rowtau"][m, 0]) * dot + float(d["rowtau"][m, 1]) * float(d["colsum"][0, n])
    v = dot + (float(d["bias"][0, n]) if "bias" in d else 0.0)
    if r["act"] == G.ACT_GELU:
        v = float(G.gelu64(torch.tensor(v, dtype=torch.float64)))
    if "gamma" in d:
        v *= float(d["gamma"][0, n])
    if r["kind"] == "tr":
        rpi = r["rows_per_image"]
        img, c = divmod(m, rpi)
        v += float(d["resid"].reshape(-1)[(img * N + n) * rpi + c])
        got = float(ref["y"].reshape(-1)[(img * N + n) * rpi + c])
    else:
        v += float(d["resid"].double()[m, n]) if "resid" in d else 0.0
        got = float(ref["y"][m, n])
    assert abs(got - v) <= 1e-12 * max(1.0, abs(v)), (rid, got, v)
    y = ref["y"]
    if r["kind"] == "stats":
        assert torch.allclose(ref["stats"][:, 0], y.mean(-1), rtol=0, atol=1e-12)
        assert torch.allclose(ref["stats"][:, 1], 1.0 / torch.sqrt(y.var(-1, unbiased=False) + G.LN_EPS), rtol=1e-12, atol=0)
    if r["kind"] == "ln16":
        want = torch.nn.functional.layer_norm(y, (N,), d["lnw"][0].double(), d["lnb"][0].double(), G.LN_EPS)
        assert torch.allclose(ref["u16"], want, rtol=1e-10, atol=1e-10)
    if r["kind"] == "emit":
        assert abs(float(ref["a16"][m, n]) - (got - float(d["cvec"][0, m]))) <= 1e-12
        grp = y[m, (n // 32) * 32:(n // 32) * 32 + 32]
        mean, m2 = ref["gstats"][(n // 32) * M + m]
        assert abs(float(mean) - float(grp.mean())) <= 1e-12 and abs(float(m2) - float(((grp - grp.mean()) ** 2).sum())) <= 1e-10
