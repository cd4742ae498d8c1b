"""CPU tests of CSWin on fp16 / bf16 activations (no GPU): the two new C entries are declared, exported and bound with one arity, they
check their arguments before any launch, their arena rows are registered for both types, a CPU 16-bit tensor raises the package's
device error, the new kernel instantiations have no scratch and the LDS of their fp32 siblings, and the rounding of the 16-bit
interface alone -- emulated in fp64 on the shapes and seeds of tests/test_cswin_io16_gpu.py -- stays within half the bar the GPU test
holds the kernels to."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

import cswin_io16_arena_rows
import cswin_io16_cases as CC
from arena_cases import TOL
from conftest import ROOT, max_abs_ratio, rel_fro
from test_abi import _declared_arity

P = ctypes.c_void_p
OK_PTR, ODD_PTR = 64, 72                  # no address of anything: never read.  64 is 16-byte aligned, 72 only 8-byte aligned
NEW = ("mi355_cswin_stripe_attn_x16_fwd", "mi355_proj_mlp_fused_x16_fwd")


def _stripe(lib, x=OK_PTR, w=OK_PTR, b=OK_PTR, w0=OK_PTR, b0=OK_PTR, w1=OK_PTR, b1=OK_PTR, ctx=OK_PTR, B=2, reso=8, C=64, hb=1, split=2,
            prec=1):
    return lib.mi355_cswin_stripe_attn_x16_fwd(P(x), P(w), P(b), P(w0), P(b0), P(w1), P(b1), P(ctx), B, reso, C, hb, split, 32 ** -0.5, 1e-5,
                                               prec, P(None))


def _mlp(lib, x=OK_PTR, ctx=OK_PTR, wp=OK_PTR, bp=OK_PTR, w1=OK_PTR, b1=OK_PTR, w2=OK_PTR, b2=OK_PTR, y=OK_PTR, M=108, C=64, hidden=256,
         flags=1, prec=1):
    return lib.mi355_proj_mlp_fused_x16_fwd(P(x), P(ctx), P(wp), P(bp), P(w1), P(b1), P(w2), P(b2), P(None), P(y), M, C, hidden, flags, 1e-5,
                                            prec, P(None))


def test_entries_are_declared_exported_and_bound_with_one_arity(built_lib):
    from mi355attn import _ffi
    arity = _declared_arity()
    handle = ctypes.CDLL(built_lib)
    for name in NEW:
        assert name in arity and hasattr(handle, name), name
        assert len(_ffi.SIGNATURES[name][1]) == arity[name] == 17, (name, len(_ffi.SIGNATURES[name][1]), arity[name])
        assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES[name.replace("_x16", "")], "the envelope and arguments of the fp32-x entry"
    src = open(os.path.join(ROOT, "include", "mi355attn.h")).read()
    for name, words in (("mi355_cswin_stripe_attn_x16_fwd", ("two 16-byte loads", "16-byte aligned", "MI355_EUNSUPPORTED", "No workspace")),
                        ("mi355_proj_mlp_fused_x16_fwd", ("rounded ONCE", "code 3", "16-byte aligned", "MI355_EUNSUPPORTED", "No workspace"))):
        at = src.index("int " + name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        for w in words:
            assert w in comment, f"the comment in front of {name} does not state {w!r}"
        proto = src[at:src.index(";", at)]
        assert "x16" in proto and "ctx16" in proto and ("y16" in proto or "stripe" in name), proto


def test_new_entries_check_their_arguments_before_any_launch(built_lib):
    """No device in this process: an answer other than -1 / -2 would have needed a launch."""
    from mi355attn import _ffi
    lib = _ffi.lib()
    for prec in (1, 2):
        for null in ("x", "w", "b", "w0", "b0", "w1", "b1", "ctx"):
            assert _stripe(lib, prec=prec, **{null: None}) == -1 and b"invalid argument" in lib.mi355_last_error(), null
        assert _stripe(lib, prec=prec, B=0) == -1 and _stripe(lib, prec=prec, reso=8, split=3) == -1
        for bad in (dict(C=96), dict(C=128, hb=1), dict(reso=16, split=8), dict(reso=96, split=1), dict(x=ODD_PTR), dict(ctx=ODD_PTR),
                    dict(w=ODD_PTR), dict(b=ODD_PTR)):
            assert _stripe(lib, prec=prec, **bad) == -2, (bad, lib.mi355_last_error())
            assert b"mi355_cswin_stripe_attn_x16_fwd" in lib.mi355_last_error()
        for null in ("x", "ctx", "wp", "bp", "w1", "b1", "w2", "y"):
            assert _mlp(lib, prec=prec, **{null: None}) == -1 and b"invalid argument" in lib.mi355_last_error(), null
        assert _mlp(lib, prec=prec, M=0) == -1 and _mlp(lib, prec=prec, flags=4) == -1 and _mlp(lib, prec=prec, flags=-1) == -1
        for bad in (dict(C=96, hidden=384), dict(C=64, hidden=128), dict(C=128, hidden=256), dict(C=256, hidden=1024), dict(x=ODD_PTR),
                    dict(ctx=ODD_PTR), dict(y=ODD_PTR), dict(wp=ODD_PTR), dict(w1=ODD_PTR), dict(w2=ODD_PTR)):
            assert _mlp(lib, prec=prec, **bad) == -2, (bad, lib.mi355_last_error())
            assert b"mi355_proj_mlp_fused_x16_fwd" in lib.mi355_last_error()
    for prec in (0, 3, -1):
        assert _stripe(lib, prec=prec) == -1 and _mlp(lib, prec=prec) == -1, "precision must be 1 (fp16) or 2 (bf16)"
    assert lib.mi355_version() == _ffi.ABI_VERSION


def test_arena_rows_are_registered_for_both_types():
    import arena_cases
    rows = [arena_cases.BY_ID[i] for i in cswin_io16_arena_rows.IDS]
    for name in NEW:
        mine = [r for r in rows if name in r["entries"]]
        assert {r["prec"] for r in mine} == {1, 2} and all(r["tol"] == TOL[r["prec"]] and r["bits"] for r in mine), name
        assert len(mine) >= 4, "a ragged and a model-sized shape per type"
    assert any(r["opts"] == dict(mlp_tt4=1) for r in rows)
    assert all(r in arena_cases.ROWS for r in rows)


def test_cpu_16bit_tensor_raises_the_device_error_not_type_error():
    import mi355attn
    from mi355attn import _ffi
    from mi355attn import functional as F
    from mi355attn.modules import CSWinBlock, CSWinTransformer, LePEAttention, Merge_Block
    ln, lin, gv = torch.nn.LayerNorm(64), torch.nn.Linear(64, 192), torch.nn.Conv2d(32, 32, 3, 1, 1, groups=32)
    for dt in CC.DTYPES:
        for m, shape in ((CSWinBlock(64, 6, 2, split_size=2), (1, 36, 64)), (CSWinBlock(32, 8, 1, split_size=8), (1, 64, 32)),
                         (LePEAttention(64, 4, -1, 4, num_heads=2), (3, 1, 16, 64)), (Merge_Block(64, 128), (1, 16, 64)),
                         (CSWinTransformer(**CC.MODEL), (1, 3, 64, 64))):
            with pytest.raises(mi355attn.Mi355Error, match="no CPU path"):
                m.eval()(torch.zeros(*shape, dtype=dt))
        for call in (lambda: F.cswin_stripe_attention16(torch.zeros(1, 36, 64, dtype=dt), ln, lin, gv, gv, 6, 2, 2, 32 ** -0.5),
                     lambda: F.proj_mlp_fused16(torch.zeros(36, 64, dtype=dt), torch.zeros(36, 64, dtype=dt), lin, ln, lin, lin)):
            with pytest.raises(mi355attn.Mi355Error, match="no CPU path"):
                call()
    text = "".join(re.findall(r'"([^"]*)"', inspect.getsource(_ffi.require_device_f32)))      # the refusal of every other module keeps its wording
    assert text.rstrip().endswith("PAM and CAM only)")
    for word in ("CSWinBlock", "LePEAttention", "Merge_Block", "CSWinTransformer", "TransformerEncoder", "MixerLayer", "DoubleAttention", "BAM"):
        assert word in text, word


def test_new_kernel_instantiations_have_no_scratch_and_the_lds_of_their_fp32_siblings(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources                                            # needs msgpack: a missing package fails this test, it does not skip it
    by_name = {r["name"]: r for r in kernel_resources.kernels(built_lib)}

    def one(pattern):
        hits = [r for n, r in by_name.items() if pattern in n]
        assert len(hits) == 1, f"no single instantiation {pattern}: {[r['name'] for r in hits]}"
        return hits[0]
    pairs = []
    for prec in (1, 2):
        for C in (64, 128):
            for tfull in (0, 3):
                for l1d in (0, 1):
                    k = f"cswin_stripe_kernelILi{prec}ELi{C}ELi{tfull}ELb{l1d}ELi0ELb%dEEEv"
                    pairs.append((one(k % 1), one(k % 0)))
        for nwv, tt in ((16, 2), (8, 4)):
            k = f"mlp_fused_kernelILi{prec}ELi64ELi256ELb1ELi{nwv}ELi{tt}ELb%dEEEv"
            pairs.append((one(k % 1), one(k % 0)))
        k = f"mlp_fused_stream_kernelILi{prec}ELi128ELi512ELb1ELb%dEEEv"
        pairs.append((one(k % 1), one(k % 0)))
    assert len(pairs) == 22
    for new, old in pairs:
        print(f"[cswin_io16 kernel] vgpr {new['vgpr']} (fp32-x {old['vgpr']}) agpr {new['agpr']} sgpr {new['sgpr']} lds {new['lds']} "
              f"scratch {new['scratch']}  {new['name']}")
        assert new["scratch"] == 0 and not new["spill_v"] and not new["spill_s"], (new["name"], new["scratch"], new["spill_v"], new["spill_s"])
        assert new["lds"] == old["lds"] <= 163840, (new["name"], new["lds"], old["lds"])


# ---- the interface rounding alone, in fp64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", CC.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("cid", ["c64_r6_s2", "c64_r8_s1", "c128_r6_s3", "c64_r8_s2_mlp2", "c256_r7_s7", "c512_r7_last", "c32_r8_s8"])
def test_block_interface_rounding_stays_within_half_the_bar(cid, dtype):
    """The oracle on x rounded to the I/O type (the tensor a user hands over) with y rounded once, against the same oracle with y left
    wide: what the one rounding of the 16-bit store costs on assert_parity's two measures.  It is bounded by the unit roundoff of the
    type (2^-11 / 2^-8, below half of 1e-3 / 1.2e-2) whatever the seed, so at least half the bar of the GPU test is left to the kernels'
    own arithmetic.  The small cases only: the large ones share the bound and cost seconds of fp64 each."""
    plain, emu = CC.block_plain(cid, dtype), CC.block_emulated(cid, dtype)
    rf, ma = rel_fro(emu, plain), max_abs_ratio(emu, plain)
    half = TOL[CC.IO[dtype]] / 2
    print(f"[cswin_io16 emulation] {cid} {dtype}: rel_fro {rf:.3e} max_abs_ratio {ma:.3e} (half bar {half:.1e})")
    assert emu.dtype == dtype and tuple(emu.shape) == CC.block_shape(cid) and rf <= half and ma <= half, (cid, dtype, rf, ma)
