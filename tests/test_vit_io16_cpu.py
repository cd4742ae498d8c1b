"""CPU tests of the ViT encoder on fp16 / bf16 activations (no GPU): the two new C entries are declared, exported and bound with one
arity, they check their arguments before any launch, their arena rows are registered for both types, a CPU 16-bit tensor raises the
package's device error, the new kernel instantiations have no scratch, and the roundings of the 16-bit interface alone -- emulated in
fp64 on the shapes and seeds of tests/test_vit_io16_gpu.py -- stay within half the bar the GPU test holds the kernels to."""
import ctypes
import os
import re
import sys

import pytest
import torch

import vit_io16_arena_rows
import vit_io16_cases as VC
from arena_cases import TOL
from conftest import ROOT, max_abs_ratio, rel_fro
from test_abi import _declared_arity

P = ctypes.c_void_p
OK_PTR, ODD_PTR = 64, 72                  # no address of anything: never read.  64 is 16-byte aligned, 72 only 8-byte aligned
NEW = ("mi355_layernorm16_x16_fwd", "mi355_linear16_res_fwd")


def _res(lib, x=OK_PTR, w=OK_PTR, r=OK_PTR, y=OK_PTR, b=OK_PTR, rio=1, oio=0, M=394, N=256, K=256, prec=1, act=0):
    return lib.mi355_linear16_res_fwd(P(x), P(w), P(b), P(r), rio, P(y), oio, M, N, K, K, N, act, prec, P(None))


def test_entries_are_declared_exported_and_bound_with_one_arity(built_lib):
    from mi355attn import _ffi
    arity = _declared_arity()
    handle = ctypes.CDLL(built_lib)
    for name in NEW:
        assert name in arity and hasattr(handle, name), name
        assert len(_ffi.SIGNATURES[name][1]) == arity[name], (name, len(_ffi.SIGNATURES[name][1]), arity[name])
    assert arity["mi355_layernorm16_x16_fwd"] == 9 and arity["mi355_linear16_res_fwd"] == 15
    src = open(os.path.join(ROOT, "include", "mi355attn.h")).read()
    for name, words in (("mi355_layernorm16_x16_fwd", ("cols % 4 == 0", "2048", "16-byte aligned", "code 2")),
                        ("mi355_linear16_res_fwd", ("K % 64 == 0", "N % 8 == 0", "any M >= 1", "16-byte aligned", "rounded ONCE", "code 3",
                                                    "MI355_EUNSUPPORTED"))):
        at = src.index("int " + name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        for w in words:
            assert w in comment, f"the comment in front of {name} does not state {w!r}"


def test_new_entries_check_their_arguments_before_any_launch(built_lib):
    """No device in this process: an answer other than -1 / -2 would have needed a launch."""
    from mi355attn import _ffi
    lib = _ffi.lib()

    def ln(x=OK_PTR, w=OK_PTR, b=OK_PTR, y=OK_PTR, rows=5, cols=64, io=1):
        return lib.mi355_layernorm16_x16_fwd(P(x), P(w), P(b), P(y), rows, cols, 1e-5, io, P(None))
    for io in (1, 2):
        for null in ("x", "w", "b", "y"):
            assert ln(io=io, **{null: None}) == -1 and b"invalid argument" in lib.mi355_last_error(), null
        assert ln(io=io, rows=0) == -1 and ln(io=io, cols=0) == -1
        assert ln(io=io, x=65) == -2 and b"mi355_layernorm16_x16_fwd" in lib.mi355_last_error()      # an odd address is no 16-bit buffer
        assert ln(io=io, w=66) == -2
    for io in (0, 3, -1):
        assert ln(io=io) == -1, "io must be 1 (fp16) or 2 (bf16)"

    for prec in (1, 2):
        for rio, oio in ((prec, 0), (0, prec), (prec, prec)):
            kw = dict(rio=rio, oio=oio, prec=prec)
            for null in ("x", "w", "r", "y"):
                assert _res(lib, **kw, **{null: None}) == -1 and b"invalid argument" in lib.mi355_last_error(), null
            assert _res(lib, M=0, **kw) == -1
            assert _res(lib, act=2, **kw) == -1, "act is none or GELU"
            for bad in (dict(K=200), dict(N=100), dict(N=260), dict(x=ODD_PTR), dict(w=ODD_PTR), dict(r=ODD_PTR), dict(y=ODD_PTR), dict(b=ODD_PTR)):
                assert _res(lib, **kw, **bad) == -2, (bad, lib.mi355_last_error())
                assert b"mi355_linear16_res_fwd" in lib.mi355_last_error()
        assert _res(lib, rio=0, oio=0, prec=prec) == -2 and b"mi355_linear16_ws_fwd" in lib.mi355_last_error(), "the all-fp32 pair"
        other = 3 - prec
        assert _res(lib, rio=other, oio=0, prec=prec) == -1 and _res(lib, rio=0, oio=other, prec=prec) == -1, "16-bit means the type of `precision`"
    for prec in (0, 3):
        assert _res(lib, rio=1, oio=1, prec=prec) == -1
    assert lib.mi355_version() == _ffi.ABI_VERSION


def test_arena_rows_are_registered_for_both_types():
    import arena_cases
    rows = [arena_cases.BY_ID[i] for i in vit_io16_arena_rows.IDS]
    for name in NEW:
        mine = [r for r in rows if name in r["entries"]]
        assert {r["prec"] for r in mine} == {1, 2} and all(r["tol"] == TOL[r["prec"]] and r["bits"] for r in mine), name
    res = [r["id"] for r in rows if "mi355_linear16_res_fwd" in r["entries"]]
    for pair in ("r16_o32", "r32_o16", "r16_o16"):
        assert sum(pair in i for i in res) == 4, (pair, res)
    assert all(r in arena_cases.ROWS for r in rows)


def test_cpu_16bit_tensor_raises_the_device_error_not_type_error():
    import inspect

    import mi355attn
    from mi355attn import _ffi
    from mi355attn import functional as F
    from mi355attn.modules import PatchEmbedding, TransformerEncoder, VisionTransformer
    for dt in VC.DTYPES:
        for m, shape in ((TransformerEncoder(128, 4), (1, 17, 128)), (PatchEmbedding(32, 16, 3, 64), (1, 3, 32, 32)),
                         (VisionTransformer(image_size=32, patch_size=16, depths=1, embedding_dim=64, num_classes=4), (1, 3, 32, 32))):
            with pytest.raises(mi355attn.Mi355Error, match="no CPU path"):
                m.eval()(torch.zeros(*shape, dtype=dt))
        for call in (lambda: F.layernorm16_x16(torch.zeros(4, 64, dtype=dt), torch.ones(64), torch.zeros(64)),
                     lambda: F.token_mean16(torch.zeros(1, 4, 64, dtype=dt), skip_first=1)):
            with pytest.raises(mi355attn.Mi355Error, match="no CPU path"):
                call()
    text = "".join(re.findall(r'"([^"]*)"', inspect.getsource(_ffi.require_device_f32)))      # the refusal of every other module keeps its wording
    assert text.rstrip().endswith("PAM and CAM only)")
    for word in ("TransformerEncoder", "VisionTransformer (with its PatchEmbedding)", "MixerLayer", "MLP_Mixer (with its PatchEmbedding)",
                 "DoubleAttention", "SELayer", "CoordinateAttention", "BAM"):
        assert word in text, word


def test_new_kernel_instantiations_have_no_scratch_and_fit_lds(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources                                            # needs msgpack: a missing package fails this test, it does not skip it
    rows = kernel_resources.kernels(built_lib)
    # by mangled name: the demangler of the tool does not know the 16-bit float types (DF16_ = _Float16, DF16b = __bf16)
    gemm = [r for r in rows if re.search(r"\d+gemm16_res_kernelI", r["name"])]
    ln = [r for r in rows if re.search(r"\d+layernorm_x16_kernelI", r["name"])]
    gen = [r for r in rows if re.search(r"\d+layernorm_x16_generic_kernelI", r["name"])]
    names = [r["name"] for r in gemm]
    for t in ("DF16_", "DF16b"):
        for r16, o16 in ((1, 0), (0, 1), (1, 1)):
            for tile in ("Li256ELi4E", "Li128ELi2E"):
                k = f"gemm16_res_kernelI{t}Lb{r16}ELb{o16}E{tile}"
                assert sum(k in n for n in names) == 1, f"no single instantiation {k} in {names}"
        assert sum(t + "EEv" in r["name"] for r in ln) == 6 and sum(t + "EEv" in r["name"] for r in gen) == 1, [r["name"] for r in ln + gen]
    assert len(gemm) == 12 and len(ln) == 12 and len(gen) == 2, names
    for r in gemm + ln + gen:
        print(f"[vit_io16 kernel] vgpr {r['vgpr']} agpr {r['agpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']}  {r['demangled'][:80]}")
        assert r["scratch"] == 0 and not r["spill_v"] and not r["spill_s"], (r["demangled"], r["scratch"], r["spill_v"], r["spill_s"])
        assert r["lds"] <= 163840, (r["demangled"], r["lds"])
    for r in gemm:
        assert r["lds"] in (32768, 49152), (r["demangled"], r["lds"])     # one K-tile of X and W: (128 + BN) x 64 x 2 bytes


# ---- the interface roundings alone, in fp64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", VC.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("cid", list(VC.BLOCKS))
def test_block_interface_roundings_stay_within_half_the_bar(cid, dtype):
    """The oracle on x rounded to the I/O type (the tensor a user hands over) with y rounded once, against the same oracle with y left
    wide: what the one rounding of the 16-bit store costs on assert_parity's two measures.  It is bounded by the unit roundoff of the
    type (2^-11 / 2^-8, below half of 1e-3 / 1.2e-2) whatever the seed, so at least half the bar of the GPU test is left to the kernels'
    own arithmetic."""
    plain, emu = VC.block_plain(cid, dtype), VC.block_emulated(cid, dtype)
    rf, ma = rel_fro(emu, plain), max_abs_ratio(emu, plain)
    half = TOL[VC.IO[dtype]] / 2
    print(f"[vit_io16 emulation] {cid} {dtype}: rel_fro {rf:.3e} max_abs_ratio {ma:.3e} (half bar {half:.1e})")
    assert emu.dtype == dtype and rf <= half and ma <= half, (cid, dtype, rf, ma)


@pytest.mark.parametrize("dtype", VC.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("mid", list(VC.MODELS))
def test_model_interface_roundings_are_reported(mid, dtype):
    """VisionTransformer(dim 128, depths 2) on the image rounded to the I/O type: the stream rounded behind the embedding and behind each
    block and the logits rounded once, against the same oracle with nothing rounded inside.  Four roundings, each carried through the
    blocks behind it into ten logits that are small differences of larger terms: no multiple of the unit roundoff bounds this distance
    the way it bounds the one rounding of a block's y, so it is printed here as it is in the GPU test, not gated (fp16, seeds not
    selected: 4.0e-4 / 2.7e-4 / 6.5e-4 rel_fro for token_64 / avg_64 / token_96).  The GPU test gates the kernels against the EMULATED
    composition, which holds these roundings too."""
    plain, emu = VC.model_refs(mid, dtype)
    rf, ma = rel_fro(emu, plain), max_abs_ratio(emu, plain)
    print(f"[vit_io16 emulation] model {mid} {dtype}: rel_fro {rf:.3e} max_abs_ratio {ma:.3e} (bar of the GPU test against the emulation {TOL[VC.IO[dtype]]:g})")
    assert emu.dtype == dtype and tuple(emu.shape) == tuple(plain.shape) and bool(torch.isfinite(emu).all())
