"""CPU tests of PAM on any channel count (mi355attn/modules/axis.py PAM._route, sdpa_wide_kernel of csrc/sdpa_general.hip):

  * the routing table: every width served before keeps its route, 1 .. 2048 never raises, 2049 does;
  * the zero-padded fused b | c | d weight the module builds (on CPU tensors): the fp64 oracle run on the padded q / k / v blocks, padded
    output columns dropped, equals the unpadded result to 1e-12;
  * the C entry refuses wide heads in 16 bits or with a bias, widths above 2048 and widths that are no multiple of 64 before it
    touches a pointer;
  * the wide-head kernel is in the built library for precisions 0 / 1 / 2 with zero scratch and at most 163 840 B of LDS;
  * the header states the new envelope, the binding keeps its arity, the arena rows are registered.
"""
import os
import re
import sys

import pytest
import torch

import pam_wide_arena_rows
from conftest import ROOT


def test_route_table():
    from mi355attn import functional as F
    from mi355attn.modules import PAM
    assert F.SDPA_WIDTHS == (32, 64, 128, 192, 256) and F.SDPA_WIDE_MAX == 2048
    for c in F.SDPA_WIDTHS:                                            # served before: one head as it is
        assert PAM._route(c) == ("one", c)
    for c in (320, 384, 448, 512):                                     # served before: two channel halves
        assert PAM._route(c) == ("pair", c)
        assert PAM._split(c) in F.SDPA_WIDTHS and c - PAM._split(c) in F.SDPA_WIDTHS
    want = {1: ("padded", 32), 31: ("padded", 32), 33: ("padded", 64), 48: ("padded", 64), 50: ("padded", 64), 96: ("padded", 128),
            100: ("padded", 128), 160: ("padded", 192), 193: ("padded", 256), 255: ("padded", 256), 257: ("wide", 320), 321: ("wide", 384),
            400: ("wide", 448), 513: ("wide", 576), 576: ("wide", 576), 600: ("wide", 640), 640: ("wide", 640), 768: ("wide", 768),
            1000: ("wide", 1024), 1024: ("wide", 1024), 2047: ("wide", 2048), 2048: ("wide", 2048)}
    for c, r in want.items():
        assert PAM._route(c) == r, (c, PAM._route(c), r)
    for c in range(1, 2049):
        kind, cp = PAM._route(c)
        assert cp >= c and cp - c < 64 and kind in ("one", "padded", "pair", "wide"), (c, kind, cp)
        if kind in ("one", "padded"):
            assert cp in F.SDPA_WIDTHS
        elif kind == "wide":
            assert F.sdpa_wide_ok(cp)
    assert not F.sdpa_wide_ok(256) and not F.sdpa_wide_ok(352) and not F.sdpa_wide_ok(2112) and F.sdpa_wide_ok(320)
    for c in (2049, 4096):
        with pytest.raises(NotImplementedError, match="2048"):
            PAM._route(c)
    with pytest.raises(ValueError):
        F.attn_head_width(320)                                         # the MHSA classes' envelope stays where it was


@pytest.mark.parametrize("c", [50, 100, 600])
def test_padded_fused_weight_computes_the_unpadded_attention(c):
    import oracle as O
    from mi355attn.modules import PAM
    torch.manual_seed(1234)
    m = PAM(c).eval()
    with torch.no_grad():
        m.alpha.fill_(0.7)
    kind, cp = PAM._route(c)
    assert kind in ("padded", "wide") and cp > c
    rows, bias = m._fused(cp)
    assert rows.shape == (3 * cp, (c + 3) // 4 * 4) and bias.shape == (3 * cp,) and rows.dtype == torch.float32
    assert m._fused(cp)[0] is rows, "built once per parameter version"
    for i, conv in enumerate((m.b, m.c, m.d)):
        blk = rows[i * cp:(i + 1) * cp]
        assert torch.equal(blk[:c, :c], conv.weight.detach().reshape(c, c)) and not blk[c:].any() and not blk[:, c:].any()
        assert torch.equal(bias[i * cp:i * cp + c], conv.bias.detach()) and not bias[i * cp + c:(i + 1) * cp].any()
    torch.manual_seed(4321)
    x = torch.randn(2, c, 5, 7) * 0.5
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ref = O.pam_forward(x, sd, dtype=torch.float64)
    # the oracle on a cp-channel PAM whose three convs are the padded blocks (x padded with zero channels, which the zero weight columns
    # would ignore anyway); the padded output columns are dropped
    psd = {"alpha": sd["alpha"]}
    for i, name in enumerate("bcd"):
        w = torch.zeros(cp, cp, 1, 1, dtype=torch.float64)
        w[:, :c, 0, 0] = rows[i * cp:(i + 1) * cp, :c].double()
        psd[f"{name}.weight"], psd[f"{name}.bias"] = w, bias[i * cp:(i + 1) * cp].double()
    xp = torch.zeros(2, cp, 5, 7, dtype=torch.float64)
    xp[:, :c] = x.double()
    got = O.pam_forward(xp, psd, dtype=torch.float64)[:, :c]
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"[pam any width] padded weight c={c} -> {cp}: max error vs unpadded fp64 {err:.2e}")
    assert err <= 1e-12
    with torch.no_grad():
        m.b.weight.mul_(2.0)                                           # a new parameter version: rebuilt
    assert m._fused(cp)[0] is not rows and torch.equal(m._fused(cp)[0][:c, :c], m.b.weight.detach().reshape(c, c))


def test_c_entry_refuses_before_it_reads_a_pointer(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()

    def call(width, io16=0, bias=None, prec=0, p=64):                  # 64 is no address of anything: it is never read
        return lib.mi355_sdpa_general_fwd(p, p, p, bias, p, 1, 1, 8, 8, width, width, width, width, width, 0, 1.0, io16, prec, None)

    for kw, words in ((dict(width=512, io16=1, prec=1), (b"io16", b"bias")), (dict(width=512, bias=64), (b"io16", b"bias")),
                      (dict(width=2112), (b"2112", b"2048")), (dict(width=352), (b"352", b"multiple of 64")), (dict(width=288), (b"288",)),
                      (dict(width=24), (b"24",))):
        assert call(**kw) == -2, (kw, lib.mi355_last_error())          # MI355_EUNSUPPORTED
        text = lib.mi355_last_error()
        assert b"mi355_sdpa_general_fwd" in text and all(w in text for w in words), (kw, text)
    assert call(640, p=None) == -1 and b"invalid argument" in lib.mi355_last_error()
    assert lib.mi355_version() == 1


def test_wide_kernel_instantiations_have_no_scratch_and_fit_lds(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources                                            # needs msgpack: a missing package fails this test, it does not skip it
    rows = [r for r in kernel_resources.kernels(built_lib) if re.search(r"\bsdpa_wide_kernel<", r["demangled"])]
    names = [r["demangled"] for r in rows]
    for p in (0, 1, 2):
        assert sum(f"sdpa_wide_kernel<{p}>" in n for n in names) == 1, f"no single instantiation for precision {p} in {names}"
    assert len(rows) == 3, names
    for r in rows:
        print(f"[pam any width kernel] vgpr {r['vgpr']} agpr {r['agpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']}  {r['demangled'][:40]}")
        assert r["scratch"] == 0 and not r["spill_v"], (r["demangled"], r["scratch"], r["spill_v"])
        assert 0 < r["lds"] <= 163840, (r["demangled"], r["lds"])      # all of it static: the launch passes no dynamic LDS
        assert r["vgpr"] <= 512, (r["demangled"], r["vgpr"])           # the unified count (accumulation registers included): four waves, one per SIMD
    # the stream kernel's instantiations are all still there
    stream = [r["demangled"] for r in kernel_resources.kernels(built_lib) if re.search(r"\bsdpa_stream_kernel<", r["demangled"])]
    assert len(stream) == 5 * 5, stream                                # five widths x (precision 0 / 1 / 2 fp32 I/O + 1 / 2 16-bit I/O)


def test_header_binding_and_trace_tag():
    from mi355attn import _ffi
    src = open(os.path.join(ROOT, "include", "mi355attn.h")).read()
    at = src.index("int mi355_sdpa_general_fwd(")
    comment = src[src.rindex("/*", 0, at):at]
    assert "[320, 2048]" in comment and "{32, 64, 128, 192, 256}" in comment and "io16 = 0" in comment and "MI355_EUNSUPPORTED" in comment
    assert len(_ffi.SIGNATURES["mi355_sdpa_general_fwd"][1]) == 19    # no new parameter, no new symbol for the wide heads
    hip = open(os.path.join(ROOT, "pytorch-attention_amd", "csrc", "sdpa_general.hip")).read()
    assert re.search(r'MI355_TRACE\(st, "sdpa_wide_kernel<d=%d,prec %d> ', hip)


def test_arena_rows_are_registered():
    import arena_cases
    ids = pam_wide_arena_rows.IDS
    assert len(ids) == 6 and len(set(ids)) == 6
    rows = [arena_cases.BY_ID[i] for i in ids]
    assert {(int(re.search(r"_(\d+)_p", r["id"]).group(1)), r["prec"]) for r in rows} == {(w, p) for w in (320, 640) for p in (0, 1, 2)}
    assert all(r["entries"] == ("mi355_sdpa_general_fwd",) and r["tol"] == arena_cases.TOL[r["prec"]] and r["tags"] for r in rows)
    assert pam_wide_arena_rows.NQ == 70 and pam_wide_arena_rows.NKV == 35 and pam_wide_arena_rows.GAP > 0
