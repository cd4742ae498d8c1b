"""CPU tests of XCiT on fp16 / bf16 activations (no GPU): the three new C entries are declared, exported and bound with one arity, they
check their arguments before any launch, their arena rows are registered for both types, a CPU 16-bit tensor raises the package's
device error, the new kernel instantiations have no scratch and the LDS of their siblings, and the rounding of the 16-bit interface
alone -- emulated in fp64 on the shapes and seeds of tests/test_xcit_io16_gpu.py -- stays within half the bar the GPU test holds the
kernels to."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

import xcit_io16_arena_rows
import xcit_io16_cases as XC
from arena_cases import TOL
from conftest import ROOT, max_abs_ratio, rel_fro
from test_abi import _declared_arity

P = ctypes.c_void_p
OK_PTR, ODD_PTR = 64, 72                  # no address of anything: never read.  64 is 16-byte aligned, 72 only 8-byte aligned
NEW = {"mi355_linear16_res_scale_fwd": 16, "mi355_linear16_stats_r16_fwd": 14, "mi355_mlp_fused_o16_fwd": 14}


def _scale(lib, x=OK_PTR, w=OK_PTR, b=OK_PTR, g=OK_PTR, r=OK_PTR, rio=1, y=OK_PTR, oio=0, M=105, N=192, K=192, ldx=None, ldy=None, act=0, prec=1):
    return lib.mi355_linear16_res_scale_fwd(P(x), P(w), P(b), P(g), P(r), rio, P(y), oio, M, N, K, K if ldx is None else ldx,
                                            N if ldy is None else ldy, act, prec, P(None))


def _stats(lib, x=OK_PTR, w=OK_PTR, b=OK_PTR, r=OK_PTR, y=OK_PTR, M=105, N=256, K=256, ldx=None, ldy=None, prec=1, st=OK_PTR):
    return lib.mi355_linear16_stats_r16_fwd(P(x), P(w), P(b), P(r), P(y), M, N, K, K if ldx is None else ldx, N if ldy is None else ldy, prec,
                                            P(st), 1e-6, P(None))


def _mlp(lib, x=OK_PTR, w1=OK_PTR, b1=OK_PTR, w2=OK_PTR, b2=OK_PTR, g=OK_PTR, y=OK_PTR, M=105, C=64, hidden=256, flags=1, prec=1):
    return lib.mi355_mlp_fused_o16_fwd(P(x), P(w1), P(b1), P(w2), P(b2), P(g), P(y), M, C, hidden, flags, 1e-5, prec, P(None))


def test_entries_are_declared_exported_and_bound_with_one_arity(built_lib):
    from mi355attn import _ffi
    arity = _declared_arity()
    handle = ctypes.CDLL(built_lib)
    for name, n in NEW.items():
        assert name in arity and hasattr(handle, name), name
        assert len(_ffi.SIGNATURES[name][1]) == arity[name] == n, (name, len(_ffi.SIGNATURES[name][1]), arity[name])
    # the siblings keep prototype and arity; the scale entry is the residual entry plus gamma, the other two take their siblings' arguments
    assert arity["mi355_linear16_res_fwd"] == 15 and arity["mi355_linear16_stats_fwd"] == 14 and arity["mi355_mlp_fused_fwd"] == 14
    assert _ffi.SIGNATURES["mi355_linear16_stats_r16_fwd"] == _ffi.SIGNATURES["mi355_linear16_stats_fwd"]
    assert _ffi.SIGNATURES["mi355_mlp_fused_o16_fwd"] == _ffi.SIGNATURES["mi355_mlp_fused_fwd"]
    src = open(os.path.join(ROOT, "include", "mi355attn.h")).read()
    for name, words, args in (
            ("mi355_linear16_res_scale_fwd", ("ONCE", "code 3", "16-byte aligned", "MI355_EUNSUPPORTED", "No workspace"), ("gamma", "resid_io")),
            ("mi355_linear16_stats_r16_fwd", ("ONCE", "range code", "16-byte aligned", "MI355_EUNSUPPORTED", "No workspace"), ("resid16",)),
            ("mi355_mlp_fused_o16_fwd", ("ONCE", "code 3", "16-byte aligned", "MI355_EUNSUPPORTED", "No workspace"), ("y16", "const float* x"))):
        at = src.index("int " + name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        for w in words:
            assert w in comment, f"the comment in front of {name} does not state {w!r}"
        proto = src[at:src.index(";", at)]
        for a in args:
            assert a in proto, (name, a, proto)
    assert _ffi.ABI_VERSION == 1, "an additive change: no ABI version bump"


def test_new_entries_check_their_arguments_before_any_launch(built_lib):
    """No device in this process: an answer other than -1 / -2 would have needed a launch."""
    from mi355attn import _ffi
    lib = _ffi.lib()
    for prec in (1, 2):
        for null in ("x", "w", "r", "y"):
            assert _scale(lib, prec=prec, rio=prec, **{null: None}) == -1 and b"invalid argument" in lib.mi355_last_error(), null
            assert b"mi355_linear16_res_scale_fwd" in lib.mi355_last_error()
        assert _scale(lib, prec=prec, rio=prec, M=0) == -1 and _scale(lib, prec=prec, rio=3 - prec) == -1 and _scale(lib, prec=prec, rio=prec, act=2) == -1
        for bad in (dict(rio=0, oio=0), dict(K=96), dict(N=100), dict(x=ODD_PTR), dict(w=ODD_PTR), dict(r=ODD_PTR), dict(y=ODD_PTR), dict(b=ODD_PTR),
                    dict(g=ODD_PTR), dict(ldx=196), dict(ldy=196)):
            kw = dict(dict(rio=prec), **bad)
            assert _scale(lib, prec=prec, **kw) == -2, (bad, lib.mi355_last_error())
            assert b"mi355_linear16_res_scale_fwd" in lib.mi355_last_error()
        for null in ("x", "w", "r", "y", "st"):
            assert _stats(lib, prec=prec, **{null: None}) == -1 and b"invalid argument" in lib.mi355_last_error(), null
        assert _stats(lib, prec=prec, M=0) == -1
        for bad in (dict(N=192, K=192), dict(N=256, K=384), dict(N=512, K=512), dict(M=31), dict(x=ODD_PTR), dict(w=ODD_PTR), dict(r=ODD_PTR),
                    dict(y=ODD_PTR), dict(b=ODD_PTR), dict(ldx=260), dict(ldy=258), dict(st=68)):
            assert _stats(lib, prec=prec, **bad) == -2, (bad, lib.mi355_last_error())
            assert b"mi355_linear16_stats_r16_fwd" in lib.mi355_last_error()
        for null in ("x", "w1", "b1", "w2", "y"):
            assert _mlp(lib, prec=prec, **{null: None}) == -1 and b"invalid argument" in lib.mi355_last_error(), null
        assert _mlp(lib, prec=prec, M=0) == -1 and _mlp(lib, prec=prec, flags=4) == -1 and _mlp(lib, prec=prec, flags=-1) == -1
        for bad in (dict(C=96, hidden=384), dict(C=64, hidden=128), dict(C=128, hidden=256), dict(C=256, hidden=1024), dict(C=384, hidden=1536),
                    dict(x=ODD_PTR), dict(y=ODD_PTR), dict(w1=ODD_PTR), dict(w2=ODD_PTR)):
            assert _mlp(lib, prec=prec, **bad) == -2, (bad, lib.mi355_last_error())
            assert b"mi355_mlp_fused_o16_fwd" in lib.mi355_last_error()
    for prec in (0, 3, -1):
        assert _scale(lib, prec=prec) == -1 and _stats(lib, prec=prec) == -1 and _mlp(lib, prec=prec) == -1, "precision must be 1 (fp16) or 2 (bf16)"
    assert lib.mi355_version() == _ffi.ABI_VERSION


def test_arena_rows_are_registered_for_both_types():
    import arena_cases
    rows = [arena_cases.BY_ID[i] for i in xcit_io16_arena_rows.IDS]
    for name in NEW:
        mine = [r for r in rows if name in r["entries"]]
        assert {r["prec"] for r in mine} == {1, 2} and all(r["tol"] == TOL[r["prec"]] and r["bits"] for r in mine), name
        assert len(mine) >= 4, "a ragged and a model-sized shape per type"
        assert any("105" in r["id"] for r in mine) and any("6272" in r["id"] for r in mine), name
    assert any(r["opts"] == dict(mlp_tt4=1) for r in rows)
    assert all(r in arena_cases.ROWS for r in rows)


def test_cpu_16bit_tensor_raises_the_device_error_not_type_error():
    import mi355attn
    from mi355attn import _ffi
    from mi355attn import functional as F
    from mi355attn.modules import LPI, XCA, ClassAttention, ClassAttentionBlock, ConvPatchEmbed, XCABlock, XCiT, xcit_nano_12_p16
    from mi355attn.modules.xcit import Mlp
    ln, lin, lin4, lin1 = torch.nn.LayerNorm(64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 256), torch.nn.Linear(256, 64)
    for dt in XC.DTYPES:
        tok = torch.zeros(1, 16, 64, dtype=dt)
        for m, args in ((XCA(64, 2), (tok,)), (LPI(64), (tok, 4, 4)), (Mlp(64, 256), (tok,)), (XCABlock(64, 2, eta=1.0), (tok, 4, 4)),
                        (XCABlock(100, 4, eta=1.0), (torch.zeros(1, 16, 100, dtype=dt), 4, 4)), (ClassAttention(64, 2), (tok,)),
                        (ClassAttentionBlock(64, 2, eta=1.0), (tok, 4, 4)), (ConvPatchEmbed(64, 16, embed_dim=64), (torch.zeros(1, 3, 64, 64, dtype=dt),)),
                        (XC.model_module(), (torch.zeros(1, 3, 64, 64, dtype=dt),)),
                        (xcit_nano_12_p16(num_classes=10), (torch.zeros(1, 3, 64, 64, dtype=dt),))):
            with pytest.raises(mi355attn.Mi355Error, match="no CPU path"):
                m.eval()(*args)
        assert isinstance(XC.model_module(), XCiT)
        x16 = torch.zeros(16, 64, dtype=dt)
        for call in (lambda: F.linear16_res_scale(x16, x16, None, None, x16, precision=XC.IO[dt]),
                     lambda: F.linear16_stats_r16(torch.zeros(32, 256, dtype=dt), torch.zeros(256, 256, dtype=dt), None, torch.zeros(32, 256, dtype=dt),
                                                  1e-6, precision=XC.IO[dt]),
                     lambda: F.mlp_fused_o16(torch.zeros(16, 64), ln, lin4, lin1, precision=XC.IO[dt])):
            with pytest.raises((mi355attn.Mi355Error, TypeError), match="no CPU path|device tensor"):
                call()
    assert lin is not None
    text = "".join(re.findall(r'"([^"]*)"', inspect.getsource(_ffi.require_device_f32)))      # the refusal of every other module keeps its wording
    assert text.rstrip().endswith("PAM and CAM only)")
    for word in ("XCABlock", "XCA", "XCiT", "ClassAttentionBlock", "LPI", "ConvPatchEmbed", "CSWinBlock", "LePEAttention", "Merge_Block",
                 "CSWinTransformer", "TransformerEncoder", "MixerLayer", "DoubleAttention", "BAM"):
        assert word in text, word
    assert text.index("XCABlock") < text.index("BAM, PAM and CAM only)")


def test_new_kernel_instantiations_have_no_scratch_and_the_lds_of_their_siblings(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources                                            # needs msgpack: a missing package fails this test, it does not skip it
    by_name = {r["name"]: r for r in kernel_resources.kernels(built_lib)}

    def one(pattern):
        hits = [r for n, r in by_name.items() if pattern in n]
        assert len(hits) == 1, f"no single instantiation {pattern}: {[r['name'] for r in hits]}"
        return hits[0]
    pairs = []
    for t, prec in (("DF16_", 1), ("DF16b", 2)):
        for r16, o16 in ((1, 0), (0, 1), (1, 1)):
            for tile in ("Li256ELi4E", "Li128ELi2E"):
                k = f"gemm16_res%s_kernelI{t}Lb{r16}ELb{o16}E{tile}"
                pairs.append((one(k % "_scale"), one(k % ""), 128))
        for K, NT in ((256, 2), (384, 3)):
            pairs.append((one(f"gemm16_wreg_r16_kernelI{t}Li{K}ELi{NT}EEEv"), one(f"gemm16_wreg_kernelI{t}Li{K}ELi{NT}ELb1ELi1EEEv"), 256))
        for nwv, tt in ((16, 2), (8, 4)):
            pairs.append((one(f"mlp_fused_o16_kernelILi{prec}ELi64ELi256ELi{nwv}ELi{tt}EEEv"),
                          one(f"mlp_fused_kernelILi{prec}ELi64ELi256ELb0ELi{nwv}ELi{tt}ELb0EEEv"), 128 if tt == 2 else 256))
        pairs.append((one(f"mlp_fused_stream_o16_kernelILi{prec}ELi128ELi512EEEv"), one(f"mlp_fused_stream_kernelILi{prec}ELi128ELi512ELb0ELb0EEEv"), 256))
    assert len(pairs) == 22
    for new, old, regs in pairs:
        print(f"[xcit_io16 kernel] vgpr {new['vgpr']} (sibling {old['vgpr']}) agpr {new['agpr']} sgpr {new['sgpr']} lds {new['lds']} "
              f"scratch {new['scratch']}  {new['name']}")
        assert new["scratch"] == 0 and not new["spill_v"] and not new["spill_s"], (new["name"], new["scratch"], new["spill_v"], new["spill_s"])
        assert new["lds"] == old["lds"] <= 163840, (new["name"], new["lds"], old["lds"])
        assert new["vgpr"] + new["agpr"] <= regs, f"{new['name']}: {new['vgpr']} + {new['agpr']} registers break the launch bounds ({regs})"


# ---- the interface rounding alone, in fp64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", XC.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("cid", list(XC.BLOCKS))
def test_block_interface_rounding_stays_within_half_the_bar(cid, dtype):
    """The oracle on x rounded to the I/O type (the tensor a user hands over) with y rounded once, against the same oracle with y left
    wide: what the one rounding of the 16-bit store costs on assert_parity's two measures.  It is bounded by the unit roundoff of the
    type (2^-11 / 2^-8, below half of 1e-3 / 1.2e-2) whatever the seed, so at least half the bar of the GPU test is left to the kernels'
    own arithmetic."""
    plain, emu = XC.block_plain(cid, dtype), XC.block_emulated(cid, dtype)
    rf, ma = rel_fro(emu, plain), max_abs_ratio(emu, plain)
    half = TOL[XC.IO[dtype]] / 2
    print(f"[xcit_io16 emulation] {cid} {dtype}: rel_fro {rf:.3e} max_abs_ratio {ma:.3e} (half bar {half:.1e})")
    assert emu.dtype == dtype and tuple(emu.shape) == XC.block_shape(cid) and rf <= half and ma <= half, (cid, dtype, rf, ma)


@pytest.mark.parametrize("dtype", XC.DTYPES, ids=["fp16", "bf16"])
def test_model_interface_roundings_stay_within_half_the_bar(dtype):
    """The same for the model: the stream rounded behind the embedding and both blocks and the logits rounded once, against the oracle
    with nothing rounded inside."""
    plain, emu = XC.model_refs(dtype)
    rf, ma = rel_fro(emu, plain), max_abs_ratio(emu, plain)
    half = TOL[XC.IO[dtype]] / 2
    print(f"[xcit_io16 emulation] model {dtype}: rel_fro {rf:.3e} max_abs_ratio {ma:.3e} (half bar {half:.1e})")
    assert emu.dtype == dtype and rf <= half and ma <= half, (dtype, rf, ma)
