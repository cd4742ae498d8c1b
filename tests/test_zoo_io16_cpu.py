"""CPU tests of the 16-bit activation path of the CNN SE variants and of simam_module / SRM / GaussianGCT / LCT / GCT
(csrc/chan_io16.hip mi355_se16_ex_fwd, csrc/chan_stat_io16.hip): the six C entries exist in the header, the built library and the
binding; they validate their arguments before any HIP call; a CPU 16-bit tensor raises the package's own error; the single-read
kernels exist for both I/O types and every mode, use no scratch and fit the registers their launch bounds promise."""
import ctypes
import os
import re
import sys

import pytest

import zoo_io16_arena_rows                                             # registers the entries' rows with tests/arena_cases.py
from conftest import ROOT

ENTRIES = ("mi355_se16_ex_fwd", "mi355_simam16_fwd", "mi355_srm16_fwd", "mi355_gct_gauss16_fwd", "mi355_lct16_fwd", "mi355_gct16_fwd")
WS = 1 << 20


def test_entries_declared_exported_and_bound(built_lib):
    import mi355attn._ffi as ffi
    src = open(os.path.join(ROOT, "include", "mi355attn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    handle = ctypes.CDLL(built_lib)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mi355attn.h"
        assert hasattr(handle, name), f"{name} is not exported by the library"
        assert name in ffi.SIGNATURES, f"{name} is missing from _ffi.SIGNATURES"
    assert ffi.lib().mi355_version() == 1                              # additions only: the ABI version stays


def test_every_entry_has_arena_rows_in_both_types_and_forms():
    import arena_cases
    for name in ENTRIES:
        rows = [r for r in arena_cases.ROWS if name in r["entries"] and r["id"] in zoo_io16_arena_rows.IDS]
        assert {r["prec"] for r in rows} == {1, 2}, name
        key = "se_single" if name == "mi355_se16_ex_fwd" else "zoo_single"
        assert {r["opts"][key] for r in rows} == {0, 1}, name
        assert all(arena_cases.BY_ID[r["id"]] is r for r in rows)


def _calls(lib, io, p, B=1, C=8, H=2, W=2, groups=2, gate=0):
    """name -> call of each entry with one pointer value for every pointer (never dereferenced: validation fails first)."""
    return {
        "se16_ex": lambda: lib.mi355_se16_ex_fwd(p, p, p, p, p, p, B, C, 2, H, W, gate, io, p, WS, None),
        "simam16": lambda: lib.mi355_simam16_fwd(p, p, B, C, H, W, 1e-4, io, p, WS, None),
        "srm16": lambda: lib.mi355_srm16_fwd(p, p, p, p, p, p, 1e-5, p, B, C, H, W, io, p, WS, None),
        "gct_gauss16": lambda: lib.mi355_gct_gauss16_fwd(p, p, B, C, H, W, 2.0, 1e-5, io, p, WS, None),
        "lct16": lambda: lib.mi355_lct16_fwd(p, p, p, p, B, C, groups, H, W, 1e-5, io, p, WS, None),
        "gct16": lambda: lib.mi355_gct16_fwd(p, p, p, p, p, B, C, H, W, 1e-5, 0, 0, io, p, WS, None),
    }


def test_argument_validation_precedes_every_hip_call(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()
    for io in (1, 2):                                                  # null pointers
        for name, call in _calls(lib, io, None).items():
            assert call() == -1 and b"invalid argument" in lib.mi355_last_error(), (name, io, lib.mi355_last_error())
    for io in (0, 3):                                                  # io is checked before any pointer is looked at
        for ptr in (None, 64):
            for name, call in _calls(lib, io, ptr).items():
                assert call() == -1, (name, io, ptr)
                text = lib.mi355_last_error()
                assert b"invalid argument" in text and b"io" in text, (name, text)
    for kw in (dict(B=0), dict(C=0), dict(H=0), dict(W=-1)):           # non-positive sizes
        for name, call in _calls(lib, 1, 64, **kw).items():
            assert call() == -1 and b"invalid argument" in lib.mi355_last_error(), (name, kw)
    calls = _calls(lib, 2, 64, H=1, W=1)                               # one pixel: no unbiased variance
    assert calls["simam16"]() == -1 and calls["srm16"]() == -1
    assert _calls(lib, 1, 64, C=8, groups=3)["lct16"]() == -1          # C % groups != 0
    assert _calls(lib, 1, 64, C=8, groups=0)["lct16"]() == -1
    assert _calls(lib, 1, 64, gate=2)["se16_ex"]() == -1               # unknown gate code
    # a workspace below mi355_chan_stat_workspace_bytes / mi355_se_workspace_bytes
    assert lib.mi355_gct16_fwd(64, 64, 64, 64, 64, 1, 8, 2, 2, 1e-5, 0, 0, 1, 64, 8, None) == -1
    assert lib.mi355_se16_ex_fwd(64, 64, 64, 64, 64, 64, 1, 8, 2, 2, 2, 0, 1, 64, 8, None) == -1


def _modules():
    from mi355attn.modules import GCT, LCT, SRM, GaussianGCT, SELayerBias, SELayerBias4, SELayerHidden, SqueezeExcite, simam_module
    return [SELayerBias(64), SELayerBias4(64), SELayerHidden(64, 16), SqueezeExcite(64), simam_module(), SRM(64).eval(), GaussianGCT(64),
            LCT(64, 8), GCT(64)]


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_cpu_16bit_tensor_raises_the_package_error(built_lib, dtype):
    import torch
    from mi355attn import Mi355Error
    x = torch.randn(2, 64, 8, 8).to(getattr(torch, dtype))
    mods = _modules()
    assert len(mods) == 9
    for m in mods:
        with pytest.raises(Mi355Error):
            m(x)


# ---- kernel metadata ----------------------------------------------------------------------------------------------------------------
MODES = {1: "simam", 2: "srm", 3: "gct_gauss", 4: "lct", 5: "gct l2", 6: "gct l1"}
NVS = (1, 2, 4, 7, 8)


def _stat16_waves(mode, nv):
    """stat16_waves of csrc/chan_stat_io16.hip: waves per SIMD in the kernel's __launch_bounds__, and (halved: a 512-thread workgroup is
    two waves per SIMD) the workgroups per CU its launcher sizes the grid for."""
    return (6 if nv <= 4 else 4) if mode == 1 else (8 if nv <= 2 else (6 if nv <= 4 else 4))


def _vgpr_budget(waves):
    """Registers per lane at `waves` waves per SIMD: 512 per SIMD lane on gfx950, allocated in blocks of 8."""
    return 512 // waves // 8 * 8


def test_launch_bound_table_matches_the_source():
    """_stat16_waves above is the source's function, and the grid and the launch bounds both come from that one function."""
    src = open(os.path.join(ROOT, "pytorch-attention_amd", "csrc", "chan_stat_io16.hip")).read()
    assert "constexpr int stat16_waves(int mode, int nv) { return mode == M_SIMAM ? (nv <= 4 ? 6 : 4) : (nv <= 2 ? 8 : (nv <= 4 ? 6 : 4)); }" in src
    assert "__launch_bounds__(512, stat16_waves(MODE, NV))" in src and "stat16_waves(MODE, stat16_nv(nv)) / 2" in src


def test_single_read_kernels_exist_without_scratch_inside_their_register_budget(built_lib):
    pytest.importorskip("msgpack")                                     # tools/kernel_resources.py decodes the metadata notes with it
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.kernels(built_lib)
    stat = {}
    for r in rows:
        m = re.search(r"stat16_single_kernel<(\d+), (\d+), (\d+)>", r["demangled"])
        if m:
            stat[tuple(int(v) for v in m.groups())] = r
    want = {(io, mode, nv) for io in (1, 2) for mode in MODES for nv in NVS}
    assert set(stat) == want, sorted(want ^ set(stat))
    for (io, mode, nv), r in sorted(stat.items()):
        budget = _vgpr_budget(_stat16_waves(mode, nv))
        print(f"[zoo16] io={io} {MODES[mode]:9s} nv={nv}: vgpr {r['vgpr']} agpr {r['agpr']} (budget {budget}) sgpr {r['sgpr']} scratch {r['scratch']}")
        assert not r["scratch"] and not r["spill_v"], (io, mode, nv, r)
        assert r["vgpr"] + r["agpr"] <= budget, (io, mode, nv, r["vgpr"], r["agpr"], budget)
        assert r["vgpr"] + r["agpr"] <= 128                            # two workgroups per CU: what the exchange's residency test assumes
        assert r["lds"] <= 512                                         # static LDS beside the C published values (dynamic)
    # the general form and the SE variants, both I/O types
    names = [r["demangled"] for r in rows]
    for k in ("row_stats16_kernel<", "stat_apply16_kernel<"):
        for io in (1, 2):
            assert any(f"{k}{io}" in n for n in names), f"no instantiation {k}{io}, ...>"
    se_ex = [r for r in rows if re.search(r"se16_single_kernel<\d+, \d+, (true|false), true>", r["demangled"])]
    se_plain = [r for r in rows if re.search(r"se16_single_kernel<\d+, \d+, (true|false), false>", r["demangled"])]
    assert len(se_ex) == 20 and len(se_plain) == 20, (len(se_ex), len(se_plain))
    for r in se_ex:
        nv = int(re.search(r"se16_single_kernel<\d+, (\d+),", r["demangled"]).group(1))
        budget = _vgpr_budget(8 if nv <= 2 else (6 if nv <= 4 else 4))  # se16_waves of csrc/chan_io16.hip
        assert not r["scratch"] and r["vgpr"] + r["agpr"] <= budget, (r["demangled"], r["vgpr"], r["scratch"], budget)
