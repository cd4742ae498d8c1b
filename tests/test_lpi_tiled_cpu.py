"""CPU tests of the tiled LPI kernel's host side: the kernel is in the built library without scratch, argument validation still comes
before any HIP call on a grid above 16 x 16, and the fused-LayerNorm workspace stays exact on such grids."""
import os
import sys

import pytest

from conftest import ROOT


def test_tile_kernel_instantiations_exist_without_scratch(built_lib):
    pytest.importorskip("msgpack")                                     # tools/kernel_resources.py decodes the metadata notes with it
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = [r for r in kernel_resources.kernels(built_lib) if "lpi_tile_kernel<" in r["demangled"]]
    names = [r["demangled"] for r in rows]
    for inst in ("lpi_tile_kernel<false>", "lpi_tile_kernel<true>"):       # plain, LayerNorm on the way in
        assert any(inst in n for n in names), f"no instantiation {inst} in {names}"
    bad = [(r["demangled"], r["scratch"], r["spill_v"]) for r in rows if r["scratch"] or r["spill_v"]]
    assert not bad, bad
    # __launch_bounds__(256, 3): three waves per SIMD need at most 168 vector registers per lane
    assert all(r["vgpr"] + r["agpr"] <= 168 for r in rows), [(r["demangled"], r["vgpr"], r["agpr"]) for r in rows]


def test_null_pointers_on_a_large_grid_are_refused_before_any_launch(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()
    rc = lib.mi355_lpi_fwd(None, None, None, None, None, None, None, 1e-5, None, None, None, None, None, 1, 40, 40, 32, None, 0, None)
    assert rc == -1 and b"invalid argument" in lib.mi355_last_error()


@pytest.mark.parametrize("B,C", [(1, 32), (3, 36), (64, 384)])
def test_workspace_is_exact_on_a_large_grid(built_lib, B, C):
    from mi355attn import _ffi
    assert _ffi.lib().mi355_lpi_workspace_bytes(B, 40, 40, C) == B * 1600 * 8 + 16
