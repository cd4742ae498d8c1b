"""CPU tests of the 16-bit activation path of SELayer / ECALayer / CBAM (csrc/chan_io16.hip): the three C entries exist in the header,
the built library and the binding; they validate their arguments before any HIP call; a CPU tensor raises the package's own error;
the shipped kernels exist for both I/O types and the single-read ones do not spill."""
import ctypes
import os
import re
import sys

import pytest

from conftest import ROOT

ENTRIES = ("mi355_se16_fwd", "mi355_eca16_fwd", "mi355_cbam16_fwd")


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


def _calls(lib, io, ptr):
    """The three entries with sizes 1 and the given io / pointer value (never dereferenced: validation fails first)."""
    return [lib.mi355_se16_fwd(ptr, ptr, ptr, ptr, 1, 1, 1, 1, 1, io, ptr, 1 << 20, None),
            lib.mi355_eca16_fwd(ptr, ptr, ptr, 1, 1, 1, 1, 1, io, ptr, 1 << 20, None),
            lib.mi355_cbam16_fwd(ptr, ptr, ptr, ptr, ptr, 1, 1, 1, 1, 1, 1, 0, io, ptr, 1 << 20, None)]


def test_argument_validation_precedes_every_hip_call(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()
    for io in (1, 2):
        rcs = []
        for rc in _calls(lib, io, None):
            rcs.append(rc)
            assert rc == -1 and b"invalid argument" in lib.mi355_last_error(), (io, rcs, lib.mi355_last_error())
    for io in (0, 3):
        for ptr in (None, 64):                                         # 64: a non-null dummy; io is checked before any pointer is looked at
            lib_calls = (lambda: lib.mi355_se16_fwd(ptr, ptr, ptr, ptr, 1, 1, 1, 1, 1, io, ptr, 1 << 20, None),
                         lambda: lib.mi355_eca16_fwd(ptr, ptr, ptr, 1, 1, 1, 1, 1, io, ptr, 1 << 20, None),
                         lambda: lib.mi355_cbam16_fwd(ptr, ptr, ptr, ptr, ptr, 1, 1, 1, 1, 1, 1, 0, io, ptr, 1 << 20, None))
            for call in lib_calls:
                assert call() == -1
                text = lib.mi355_last_error()
                assert b"invalid argument" in text and b"io" in text, text
    # non-positive sizes
    assert lib.mi355_se16_fwd(64, 64, 64, 64, 0, 1, 1, 1, 1, 1, 64, 1 << 20, None) == -1
    assert lib.mi355_eca16_fwd(64, 64, 64, 1, 1, 2, 1, 1, 1, 64, 1 << 20, None) == -1          # even k
    assert lib.mi355_cbam16_fwd(64, 64, 64, 64, 64, 1, 1, 1, 1, 1, 1, 3, 1, 64, 1 << 20, None) == -1   # stage 3


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_cpu_16bit_tensor_raises_the_package_error(built_lib, dtype):
    import torch
    from mi355attn import Mi355Error
    from mi355attn.modules import CBAM, ECALayer, SELayer
    x = torch.randn(2, 64, 8, 8).to(getattr(torch, dtype))
    for m in (SELayer(64), ECALayer(64), CBAM(64)):
        with pytest.raises(Mi355Error):
            m(x)


def test_16bit_kernels_exist_and_single_read_ones_do_not_spill(built_lib):
    pytest.importorskip("msgpack")                                     # tools/kernel_resources.py decodes the metadata notes with it
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.kernels(built_lib)
    names = [r["demangled"] for r in rows]
    # first template argument = the I/O type: 1 IEEE half, 2 bfloat16
    blocks = {"SE": ("se16_single_kernel<", "scale16_kernel<"), "ECA": ("eca16_halo_kernel<", "scale16_kernel<"),
              "CBAM": ("cbam16_single_kernel<", "cbam16_stats_kernel<")}
    for block, kernels in blocks.items():
        for k in kernels:
            for io in (1, 2):
                assert any(f"{k}{io}" in n for n in names), f"{block}: no instantiation {k}{io}, ...>"
    single = [r for r in rows if any(k in r["demangled"] for k in ("se16_single_kernel<", "eca16_halo_kernel<", "cbam16_single_kernel<"))]
    assert len(single) >= 40, len(single)
    bad = [(r["demangled"], r["scratch"]) for r in single if r["scratch"]]
    assert not bad, bad
    # two workgroups of 512 threads per CU (what the exchange needs resident in every configuration) fit at <= 128 VGPRs
    wide = [(r["demangled"], r["vgpr"]) for r in single if r["vgpr"] > 128]
    assert not wide, wide
