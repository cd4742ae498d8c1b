"""CPU tests of the 16-bit activation path of CoordinateAttention, TripletAttention, AttentionGate and BAM (csrc/axis_attn_io16.hip, the
*16 entries of csrc/axis_attn.hip): the four C entries exist in the header, the built library and the binding; they validate their
arguments before any launch; their arena rows are registered; the TypeError of the fp32-only entries names the new modules; a CPU 16-bit
tensor raises the package's own error; the new kernels exist for both I/O types without scratch; and the bound of
tests/test_axis_io16_gpu.py holds for the fp32 oracle rounded once."""
import ctypes
import os
import re
import sys

import pytest
import torch

import axis_io16_arena_rows                                            # registers the entries' rows with tests/arena_cases.py
from axis_io16_arena_rows import build, reference
from conftest import ROOT

ENTRIES = ("mi355_coordatt16_fwd", "mi355_triplet16_fwd", "mi355_attention_gate16_fwd", "mi355_bam16_fwd")
WS = 1 << 24


def test_entries_declared_exported_and_bound(built_lib):
    import mi355attn._ffi as ffi
    src = open(os.path.join(ROOT, "include", "mi355attn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    handle = ctypes.CDLL(built_lib)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mi355attn.h"
        assert hasattr(handle, name), f"{name} is not exported by the library"
        assert name in ffi.SIGNATURES, f"{name} is missing from _ffi.SIGNATURES"
        f32 = ffi.SIGNATURES[name.replace("16_fwd", "_fwd")][1]        # the fp32 prototype with `int io` in front of the workspace
        assert ffi.SIGNATURES[name][1] == f32[:-3] + [ffi.c_int] + f32[-3:], name
    assert ffi.lib().mi355_version() == 1                              # additions only: the ABI version stays


def test_every_entry_has_arena_rows_in_both_types_and_shapes():
    import arena_cases
    assert len(axis_io16_arena_rows.IDS) == 16 and len(set(axis_io16_arena_rows.IDS)) == 16
    for name in ENTRIES:
        rows = [r for r in arena_cases.ROWS if name in r["entries"] and r["id"] in axis_io16_arena_rows.IDS]
        assert len(rows) == 4 and {r["prec"] for r in rows} == {1, 2}, name
        assert {r["id"].split("_")[1] for r in rows} == {"2x64x32x32", "3x40x13x70"}, name
        assert all(arena_cases.BY_ID[r["id"]] is r for r in rows)


def _calls(lib, io, p, table, B=1, C=16, H=2, W=2, ks=7, ws=WS):
    """name -> call of each entry with one pointer value for every pointer (never dereferenced: validation fails first)."""
    return {
        "coordatt16": lambda: lib.mi355_coordatt16_fwd(p, p, p, p, p, p, p, p, p, p, B, C, 8, H, W, io, p, ws, None),
        "triplet16": lambda: lib.mi355_triplet16_fwd(p, p, p, p, p, p, B, C, H, W, ks, io, p, ws, None),
        "attention_gate16": lambda: lib.mi355_attention_gate16_fwd(p, p, p, p, B, C, H, W, ks, io, p, ws, None),
        "bam16": lambda: lib.mi355_bam16_fwd(p, table, p, B, C, 1, H, W, 4, io, p, ws, None),
    }


def test_argument_validation_precedes_every_launch(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()
    table = (ctypes.c_void_p * 16)(*([64] * 16))                       # BAM's parameter table is a host array: read, its entries are not
    tp = ctypes.cast(table, ctypes.c_void_p)
    for io in (1, 2):                                                  # null x / y / parameters / workspace
        for name, call in _calls(lib, io, None, tp).items():
            assert call() == -1 and b"invalid argument" in lib.mi355_last_error(), (name, io, lib.mi355_last_error())
        assert lib.mi355_bam16_fwd(64, None, 64, 1, 16, 1, 2, 2, 4, io, 64, WS, None) == -1
        assert lib.mi355_coordatt16_fwd(None, 64, 64, 64, 64, 64, 64, 64, 64, 64, 1, 16, 8, 2, 2, io, 64, WS, None) == -1          # x alone
        assert lib.mi355_coordatt16_fwd(64, 64, 64, 64, 64, 64, 64, 64, 64, None, 1, 16, 8, 2, 2, io, 64, WS, None) == -1          # y alone
    for io in (0, 3, -1):                                              # io is checked before any pointer is looked at
        for ptr in (None, 64):
            for name, call in _calls(lib, io, ptr, tp).items():
                assert call() == -1, (name, io, ptr)
                text = lib.mi355_last_error()
                assert b"invalid argument" in text and b"io" in text, (name, text)
    for kw in (dict(B=0), dict(C=0), dict(H=0), dict(W=-1)):           # non-positive sizes
        for name, call in _calls(lib, 1, 64, tp, **kw).items():
            assert call() == -1 and b"invalid argument" in lib.mi355_last_error(), (name, kw)
    for name, call in _calls(lib, 2, 64, tp, ws=8).items():            # a workspace below the fp32 entry's query
        assert call() == -1 and b"workspace_bytes" in lib.mi355_last_error(), (name, lib.mi355_last_error())
    for ks in (0, 2, 17):
        calls = _calls(lib, 1, 64, tp, ks=ks)
        assert calls["triplet16"]() == -1 and calls["attention_gate16"]() == -1
    # shapes the fp32 entries refuse are refused with their code (MI355_EUNSUPPORTED), before any launch
    assert lib.mi355_coordatt16_fwd(64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 1, 16, 129, 2, 2, 1, 64, WS, None) == -2
    assert lib.mi355_bam16_fwd(64, tp, 64, 1, 16, 33, 2, 2, 4, 1, 64, WS, None) == -2


def test_type_error_text_names_the_new_modules_and_keeps_the_other_names():
    src = open(os.path.join(ROOT, "pytorch-attention_amd", "mi355attn", "_ffi.py")).read()
    text = " ".join(re.findall(r'"([^"]*)"', src[src.index("def require_device_f32"):src.index("IO_CODES =")]))
    for name in ("SELayer", "ECALayer", "CBAM", "ChannelAttention", "SpatialAttention", "SELayerBias", "SELayerBias4", "SELayerHidden",
                 "SqueezeExcite", "simam_module", "SRM", "GaussianGCT", "LCT", "GCT", "DoubleAttention",
                 "CoordinateAttention", "TripletAttention", "AttentionGate", "BAM"):
        assert re.search(r"\b%s\b" % name, text), name
    assert not re.search(r"\bGCModule\b", text)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_cpu_16bit_tensor_raises_the_package_error(built_lib, dtype):
    from mi355attn import Mi355Error
    x = torch.randn(2, 64, 8, 8).to(getattr(torch, dtype))
    for kind in ("coord", "triplet", "gate", "bam"):
        with pytest.raises(Mi355Error):
            build(kind, 64)(x)


# ---- the bound of the GPU test, shown to hold for the fp32 oracle with the one rounding of y ------------------------------------------
U = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}
EMU = [(2, 64, 32, 32), (3, 40, 13, 70), (2, 16, 70, 6)]


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_bound_holds_for_the_fp32_oracle_rounded_once(dtype):
    """|y - ref64| <= u |ref64| + 3e-5 max|ref64| (+ 2^-25 below the fp16 normal range) for y = the fp32 oracle on x16.float(), rounded
    to the I/O type: what a kernel that computes in fp32 and rounds once can promise."""
    import oracle.axis_attn as OA
    dt = getattr(torch, dtype)
    for kind, fn in (("coord", OA.coordatt_forward), ("triplet", OA.triplet_forward), ("bam", OA.bam_forward)):
        for shape in EMU:
            m = build(kind, shape[1])
            sd = m.state_dict()
            x16 = torch.randn(*shape, generator=torch.Generator().manual_seed(4321)).to(dt)
            ref = reference(kind, x16, sd)
            y = fn(x16.float(), sd).to(dt).double()
            bound = U[dtype] * ref.abs() + 3e-5 * float(ref.abs().max())
            if dtype == "float16":
                bound = bound + (ref.abs() < 2.0 ** -14).double() * 2.0 ** -25
            worst = float(((y - ref).abs() / bound).max())
            print(f"[axis16 emulation] {kind}{shape} {dtype}: max err / bound = {worst:.3f}")
            assert worst <= 1.0, (kind, shape, dtype, worst)


# ---- kernel metadata ----------------------------------------------------------------------------------------------------------------
def test_new_kernels_exist_for_both_types_without_scratch(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources                                            # needs msgpack: a missing package fails this test, it does not skip it
    rows = [r for r in kernel_resources.kernels(built_lib)
            if re.search(r"\b(chan_reduce16_kernel|plane_pool16_lds_kernel|plane_pool16_kernel|plane_dot16_kernel|apply16_kernel)<", r["demangled"])
            and "stat_apply16" not in r["demangled"]]
    names = [r["demangled"] for r in rows]
    want = [f"chan_reduce16_kernel<{io}, 0, {k}, {v}>" for io in (1, 2) for k, vs in ((4, (8, 1)), (8, (8, 1)), (16, (4, 1)), (32, (4, 1))) for v in vs]
    want += [f"chan_reduce16_kernel<{io}, 1, 1, {v}>" for io in (1, 2) for v in (8, 1)]
    want += [f"plane_pool16_lds_kernel<{io}, {mx}, {v}>" for io in (1, 2) for mx in ("true", "false") for v in (8, 1)]
    want += [f"plane_pool16_kernel<{io}, {mx}, {n}>" for io in (1, 2) for mx in ("true", "false") for n in (1, 2, 4)]
    want += [f"plane_dot16_kernel<{io}, {v}>" for io in (1, 2) for v in (8, 1)]
    want += [f"apply16_kernel<{io}, {mode}, {v}>" for io in (1, 2) for mode in (1, 2, 3, 4) for v in (8, 1)]
    for k in want:
        assert sum(k in n for n in names) == 1, f"no single instantiation {k}"
    assert len(rows) == len(want), sorted(set(names) - {n for n in names if any(k in n for k in want)})
    for r in rows:
        assert not r["scratch"] and not r["spill_v"], (r["demangled"], r["scratch"])
        assert r["vgpr"] + r["agpr"] <= 256, (r["demangled"], r["vgpr"], r["agpr"])     # two 256-thread workgroups per CU at least
