"""CPU test of mi355attn._ffi.IO_ENTRIES, the table functional._call_io picks the fp32 or the 16-bit entry of a drop-in gate from: every
pair is declared, exported and bound with prototypes that differ by the one `int io`, and no 16-bit twin of an fp32 gate entry is
missing from the table -- a module ported later cannot bypass the helper unnoticed."""
import ctypes
import os
import re

from conftest import ROOT

OPS = ("se", "se_ex", "eca", "cbam", "coordatt", "triplet", "attention_gate", "bam", "simam", "srm", "gct_gauss", "lct", "gct", "double_attn")
# 16-bit entries with an fp32 twin that are NOT activation-type variants of a gate: the dense 16-bit dataflow (its `16` names the operand
# and buffer format, the prototypes differ in more than an `io`)
DENSE = {"mi355_xca16_fwd", "mi355_layernorm16_fwd", "mi355_linear16_fwd", "mi355_sdpa16_fwd", "mi355_cswin_lepe_attn16_fwd"}


def test_every_pair_is_declared_exported_bound_and_differs_by_io_only(built_lib):
    import mi355attn._ffi as ffi
    src = open(os.path.join(ROOT, "include", "mi355attn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    handle = ctypes.CDLL(built_lib)
    assert tuple(ffi.IO_ENTRIES) == OPS
    for op, pair in ffi.IO_ENTRIES.items():
        assert len(pair) == 2 and pair[0] != pair[1], op
        for name in pair:
            assert name in ffi.SIGNATURES, f"{name} is missing from _ffi.SIGNATURES"
            assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in mi355attn.h"
            assert hasattr(handle, name), f"{name} is not exported by the library"
        (res32, arg32), (res16, arg16) = ffi.SIGNATURES[pair[0]], ffi.SIGNATURES[pair[1]]
        assert res32 is res16 is ffi.c_int, op
        if op == "double_attn":                                        # io sits in the slot of the fp32 entry's precision
            assert arg16 == arg32 and arg32[-4] is ffi.c_int, op
        else:                                                          # `int io` in front of (workspace, workspace_bytes, stream)
            assert arg16 == arg32[:-3] + [ffi.c_int] + arg32[-3:], op


def test_no_16bit_twin_of_a_gate_entry_is_missing_from_the_table():
    import mi355attn._ffi as ffi
    listed = {pair[1] for pair in ffi.IO_ENTRIES.values()}
    twins = {n for n in ffi.SIGNATURES if re.fullmatch(r"mi355_\w*16\w*_fwd", n) and n.replace("16", "", 1) in ffi.SIGNATURES}
    assert listed <= twins and all(ffi.IO_ENTRIES[op][0] == ffi.IO_ENTRIES[op][1].replace("16", "", 1) for op in ffi.IO_ENTRIES)
    assert DENSE <= twins, DENSE - twins                               # the exclusion list names existing entries only
    assert twins - DENSE == listed, f"not in IO_ENTRIES: {sorted(twins - DENSE - listed)}"
