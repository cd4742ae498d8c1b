"""CPU tests of the residual (+ ReLU) epilogue of SELayer / ECALayer / CBAM (csrc/gate_res.h; mi355_se_res_fwd, mi355_eca_res_fwd,
mi355_cbam_res_fwd): the three entries are declared, exported, bound with the header's arity and documented; they validate their
arguments before any launch; the residual kernel forms exist for fp32, fp16 and bf16 without scratch; their arena rows are registered;
the Python wrappers refuse bad arguments without a device; and the bound of tests/test_gate_resid_gpu.py holds for the fp32
restatement of the reference rounded once."""
import ctypes
import os
import re
import sys

import pytest
import torch

import gate_resid_arena_rows                                           # registers the entries' rows with tests/arena_cases.py
import gate_resid_cases as G
from conftest import ROOT, max_abs_ratio, rel_fro

ENTRIES = ("mi355_se_res_fwd", "mi355_eca_res_fwd", "mi355_cbam_res_fwd")
WS = 1 << 26


def _header():
    return open(os.path.join(ROOT, "include", "mi355attn.h")).read()


def test_entries_declared_exported_bound_and_documented(built_lib):
    import mi355attn._ffi as ffi
    raw = _header()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    handle = ctypes.CDLL(built_lib)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, f"{name} is not declared in mi355attn.h"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert hasattr(handle, name), f"{name} is not exported by the library"
        assert name in ffi.SIGNATURES and len(ffi.SIGNATURES[name][1]) == len(params), (name, params)
        for p, c in zip(params, ffi.SIGNATURES[name][1]):              # pointers, ints and the size travel as what the header says
            want = ffi.c_vp if "*" in p or "mi355_stream_t" in p else (ffi.c_size if p.startswith("size_t") else ffi.c_int)
            assert c is want, (name, p)
        assert [p.split()[-1] for p in params[-5:]] == ["relu", "io", "ws", "ws_bytes", "stream"], params
        assert all(name not in pair for pair in ffi.IO_ENTRIES.values())               # bound beside IO_ENTRIES, not in it
    doc = raw[raw.index("with the shortcut add"):raw.index("mi355_se_res_fwd(")]
    for word in ("relu", "`io`", "must not overlap", "MI355_EINVAL", "MI355_EUNSUPPORTED", "mi355_cbam16_workspace_bytes"):
        assert word in doc, word
    assert ffi.lib().mi355_version() == 1                              # additions only: the ABI version stays


def _calls(lib, p, r, y, io=0, relu=0, B=1, C=16, H=4, W=4, Cr=4, k=3, ks=7, ws=WS):
    return {
        "se": lambda: lib.mi355_se_res_fwd(p, p, p, r, y, B, C, Cr, H, W, relu, io, p, ws, None),
        "eca": lambda: lib.mi355_eca_res_fwd(p, p, r, y, B, C, k, H, W, relu, io, p, ws, None),
        "cbam": lambda: lib.mi355_cbam_res_fwd(p, p, p, p, r, y, B, C, Cr, ks, H, W, relu, io, p, ws, None),
    }


def test_argument_validation_precedes_every_launch(built_lib):
    """Pointers are small integers that are never dereferenced: validation fails first (no device is needed)."""
    from mi355attn import _ffi
    lib = _ffi.lib()
    X, R, Y = 1 << 20, 2 << 20, 3 << 20                                # three disjoint "tensors"
    EINVAL, EUNSUPPORTED = -1, -2
    for io in (0, 1, 2):
        for name, call in _calls(lib, None, None, None, io=io).items():                # NULL everything
            assert call() == EINVAL and b"invalid argument" in lib.mi355_last_error(), (name, io)
        for name, call in _calls(lib, X, None, Y, io=io).items():                      # resid is non-NULL
            assert call() == EINVAL and b"resid" in lib.mi355_last_error(), (name, io)
        for name, call in _calls(lib, X, R, None, io=io).items():
            assert call() == EINVAL, (name, io)
        for kw in (dict(B=0), dict(C=0), dict(H=0), dict(W=-1)):                        # non-positive sizes
            for name, call in _calls(lib, X, R, Y, io=io, **kw).items():
                assert call() == EINVAL and b"invalid argument" in lib.mi355_last_error(), (name, kw)
        for relu in (-1, 2):
            for name, call in _calls(lib, X, R, Y, io=io, relu=relu).items():
                assert call() == EINVAL and b"relu" in lib.mi355_last_error(), (name, relu)
        for name, call in _calls(lib, X, R, Y, io=io, ws=8).items():                    # a workspace below the plain entry's query
            assert call() == EINVAL and b"ws_bytes" in lib.mi355_last_error(), (name, lib.mi355_last_error())
        # y must not overlap x or resid
        for name, call in _calls(lib, X, R, X, io=io).items():
            assert call() == EINVAL and b"overlap" in lib.mi355_last_error(), (name, lib.mi355_last_error())
        for name, call in _calls(lib, X, R, R + 8, io=io).items():
            assert call() == EINVAL and b"overlap" in lib.mi355_last_error(), (name, lib.mi355_last_error())
    for io in (3, -1):                                                                  # io outside 0 .. 2
        for name, call in _calls(lib, X, R, Y, io=io).items():
            assert call() == EINVAL and b"io" in lib.mi355_last_error(), (name, io)
    calls = _calls(lib, X, R, Y, k=4)
    assert calls["eca"]() == EINVAL                                                     # an even ECA kernel
    assert _calls(lib, X, R, Y, ks=2)["cbam"]() == EINVAL and _calls(lib, X, R, Y, Cr=0)["se"]() == EINVAL
    # a shape the plain entry refuses is refused with its code, before any launch: channel counts beyond the gate stage's LDS
    big = dict(B=1, C=20000, H=1, W=1, Cr=4, ws=1 << 30)
    plain = lib.mi355_se_fwd(X, X, X, Y, 1, 20000, 4, 1, 1, X, 1 << 30, None)
    assert plain == EUNSUPPORTED
    assert _calls(lib, X, R, Y, io=0, **big)["se"]() == EUNSUPPORTED and _calls(lib, X, R, Y, io=1, **big)["se"]() == EUNSUPPORTED
    assert _calls(lib, X, R, Y, io=0, **big)["eca"]() == EUNSUPPORTED


def test_python_wrappers_refuse_bad_arguments_without_a_device(built_lib):
    """What can be refused before x is looked at as a device tensor is refused on any machine: the rest is tests/test_gate_resid_gpu.py."""
    import mi355attn.functional as F
    x = torch.randn(2, 16, 4, 4)
    with pytest.raises(ValueError):
        F.cbam_forward(x, stage=1, resid=x)
    import inspect
    from mi355attn.modules import CBAM, ECALayer, SELayer
    for cls in (SELayer, ECALayer, CBAM):
        ps = list(inspect.signature(cls.forward).parameters.values())
        assert [p.name for p in ps] == ["self", "x", "resid", "relu"] and ps[2].default is None and ps[3].default is False
    for fn in (F.se_forward, F.eca_forward, F.cbam_forward):
        ps = inspect.signature(fn).parameters
        assert ps["resid"].default is None and ps["relu"].default is False and list(ps)[-2:] == ["resid", "relu"]


def test_arena_rows_cover_every_entry_type_form_and_relu():
    import arena_cases
    ids = gate_resid_arena_rows.IDS
    assert len(ids) == len(set(ids))
    for name in ENTRIES:
        rows = [r for r in arena_cases.ROWS if name in r["entries"] and r["id"] in ids]
        assert {r["prec"] for r in rows} == {0, 1, 2}, name
        for p in (0, 1, 2):
            mine = [r for r in rows if r["prec"] == p]
            assert {next(iter(r["opts"].values())) for r in mine} == {0, 1}, (name, p)
            assert {r["id"][-1] for r in mine} == {"0", "1"}, (name, p)                 # relu off and on
            assert {r["id"].split("_")[2] for r in mine} == {"2x64x32x32", "3x72x7x7"}, (name, p)
        assert all(arena_cases.BY_ID[r["id"]] is r for r in rows)


def test_residual_kernel_forms_exist_for_all_types_without_scratch(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources                                            # needs msgpack: a missing package fails this test, it does not skip it
    rows = [r for r in kernel_resources.kernels(built_lib) if re.search(r"\b\w+_res_kernel<", r["demangled"])
            and re.search(r"\b(se_single|eca_halo|cbam_single|gate_scale|cbam_apply_band|se16_single|eca16_halo|cbam16_single|scale16)_res_kernel<",
                          r["demangled"])]
    names = [r["demangled"] for r in rows]
    tf = ("true", "false")
    want = [f"se_single_res_kernel<{nv}, {a}, {b}, {c}>" for nv in (1, 2, 4, 8, 13, 16) for a in tf for b in tf for c in tf]
    want += [f"eca_halo_res_kernel<{nv}, {a}, {c}>" for nv in (1, 2, 4, 8, 13, 16) for a in tf for c in tf]
    want += [f"cbam_single_res_kernel<512, {s}, {nv}, {f}, {c}>" for s in (16, 32) for nv in (4, 8, 16) for f in tf for c in tf]
    want += [f"gate_scale_res_kernel<{m}, {v}, {a}, {b}, {c}>" for m in (0, 1) for v in tf for a in tf for b in tf for c in tf]
    want += [f"cbam_apply_band_res_kernel<{k}, {v}, {a}, {b}, {c}>" for k in (0, 3, 7) for v in tf for a in tf for b in tf for c in tf]
    want += [f"se16_single_res_kernel<{io}, {nv}, {w}, {c}>" for io in (1, 2) for nv in (1, 2, 4, 7, 8) for w in tf for c in tf]
    want += [f"eca16_halo_res_kernel<{io}, {nv}, {c}>" for io in (1, 2) for nv in (1, 2, 4, 7, 8) for c in tf]
    want += [f"cbam16_single_res_kernel<{io}, {s}, {nv}, {f}, {c}>" for io in (1, 2) for s in (16, 32) for nv in (4, 8, 16) for f in tf for c in tf
             if f == "true" or nv != 16]
    want += [f"scale16_res_kernel<{io}, {v}, {c}>" for io in (1, 2) for v in tf for c in tf]
    for k in want:
        assert sum(k in n for n in names) == 1, f"no single instantiation {k}"
    assert len(rows) == len(want), sorted(n for n in names if not any(k in n for k in want))
    for r in rows:
        assert not r["scratch"] and not r["spill_v"], (r["demangled"], r["scratch"])
        # 512-thread workgroups: two per CU (128 registers) everywhere except the 16-slot CBAM forms, which are built for one
        one_per_cu = re.search(r"cbam(16)?_single_res_kernel<[^>]*\b16, (true|false), (true|false)>", r["demangled"])
        assert r["vgpr"] + r["agpr"] <= (256 if one_per_cu or "scale" in r["demangled"] or "apply_band" in r["demangled"] else 128), \
            (r["demangled"], r["vgpr"], r["agpr"])


@pytest.mark.parametrize("io", ["fp32", "fp16", "bf16"])
def test_bound_holds_for_the_fp32_restatement_rounded_once(io):
    """The reference restated in fp32 (the oracle in fp32 on the widened inputs, the add and the ReLU in fp32) and rounded once to the I/O
    type stays inside the bound of tests/test_gate_resid_gpu.py for every input of the table: fp32 rel_fro and max-abs ratio <= 1e-5;
    16-bit u |ref| + 1e-5 max|ref| (+ 2^-25 below the fp16 normal range) on every element."""
    dt = G.DTYPES[io]
    for gate in G.GATES:
        for shape, _ in G.CASES:
            m = G.build(gate, shape[1])
            x, r = G.inputs(shape, dt)
            for relu in (False, True):
                ref = G.reference(gate, m, x, r, relu)
                y = G.reference(gate, m, x.float(), r.float(), relu, torch.float32).to(dt).double()
                if io == "fp32":
                    rf, ma = rel_fro(y, ref), max_abs_ratio(y, ref)
                    assert rf <= 1e-5 and ma <= 1e-5, (gate, shape, relu, rf, ma)
                    continue
                bound = G.U[dt] * ref.abs() + 1e-5 * float(ref.abs().max())
                if dt == torch.float16:
                    bound = bound + (ref.abs() < 2.0 ** -14).double() * 2.0 ** -25
                worst = float(((y - ref).abs() / bound).max())
                assert worst <= 1.0, (gate, shape, io, relu, worst)


def test_fp16_overflow_case_is_not_borderline():
    """The overflow case of the GPU test (x = resid = 60000 in fp16): no reference element lies between 6.5e4 and 6.6e4, for every gate."""
    for gate in G.GATES:
        m = G.build(gate, G.SINGLE[1])
        x = torch.full(G.SINGLE, 60000.0, dtype=torch.float16)
        for relu in (False, True):
            ref = G.reference(gate, m, x, x, relu)
            assert not ((ref.abs() > 6.5e4) & (ref.abs() < 6.6e4)).any(), gate
            assert torch.isinf(ref.to(torch.float16)).any(), gate
