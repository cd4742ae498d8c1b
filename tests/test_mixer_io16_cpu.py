"""CPU tests of the MLP-Mixer family on fp16 / bf16 activations (no GPU): the new C entries check their arguments before any launch, the
header states their envelopes, a CPU 16-bit tensor raises the package's device error, the new kernel instantiations have no scratch, and
the roundings of the 16-bit interface alone -- emulated in fp64 on the shapes and seeds of tests/test_mixer_io16_gpu.py -- stay within
half the bar the GPU test holds the kernels to."""
import ctypes
import os
import re
import sys

import pytest
import torch

import mixer_io16_arena_rows  # noqa: F401  (registers the arena rows of the new entries with tests/arena_cases.py)
import mixer_io16_cases as MC
from arena_cases import TOL
from conftest import ROOT, max_abs_ratio, rel_fro

P = ctypes.c_void_p
OK_PTR, ODD_PTR = 64, 72                  # no address of anything: never read.  64 is 16-byte aligned, 72 only 8-byte aligned


def _entries(lib):
    """name -> call(ptr, shape_ok, io): every pointer argument is `ptr` (None = null), the shape inside or outside the envelope."""
    def tok(p, ok, io):
        N, C, T = (196, 256, 128) if ok else (49, 256, 128)
        return lib.mi355_mixer_token_x16_fwd(P(p), P(p), P(p), 1e-5, P(p), P(p), P(p), P(p), P(p), 2, N, C, T, io, P(p), 1 << 20, P(None))

    def pe(p, ok, io):
        ps = 16 if ok else 4                                                 # ps % 8 != 0: outside
        return lib.mi355_patch_embed_x16_fwd(P(p), P(p), P(p), P(p), 2, 3, 224, 224, ps, 256, io, P(p), 1 << 30, P(None))

    def mean(p, ok, io):
        return lib.mi355_token_mean_x16_fwd(P(p), P(p), 2, 196, 256 if ok else 254, 196 * 256, io, P(None))

    def widen(p, ok, io):
        return lib.mi355_widen16_fwd(P(p if ok or p is None else ODD_PTR), P(p), 1000, io, P(None))

    def rnd(p, ok, io):
        return lib.mi355_round16_fwd(P(p), P(p if ok or p is None else ODD_PTR), 1000, io, P(None))
    return {"mi355_mixer_token_x16_fwd": tok, "mi355_patch_embed_x16_fwd": pe, "mi355_token_mean_x16_fwd": mean, "mi355_widen16_fwd": widen,
            "mi355_round16_fwd": rnd}


def test_new_entries_check_their_arguments_before_any_launch(built_lib):
    """No device in this process: an answer other than -1 / -2 would have needed a launch."""
    from mi355attn import _ffi
    lib = _ffi.lib()
    for name, call in _entries(lib).items():
        for io in (1, 2):
            assert call(None, True, io) == -1 and b"invalid argument" in lib.mi355_last_error(), (name, "null pointers")
            assert call(None, False, io) == -1, (name, "null pointers outside the envelope: the pointers are checked first")
            assert call(OK_PTR, False, io) == -2, (name, io, lib.mi355_last_error())
            assert name.encode() in lib.mi355_last_error(), (name, lib.mi355_last_error())
        for io in (0, 3):
            assert call(OK_PTR, True, io) == -1, (name, "io must be 1 (fp16) or 2 (bf16)")
    assert lib.mi355_mixer_token_x16_workspace_bytes(4, 196, 512) == lib.mi355_mixer_token_workspace_bytes(4, 196, 512) > 0
    assert lib.mi355_patch_embed_x16_workspace_bytes(2, 3, 224, 224, 16, 256) == 2 * 196 * 768 * 2
    assert lib.mi355_patch_embed_x16_workspace_bytes(2, 3, 224, 224, 4, 256) == 0
    # too small a workspace is an argument error, not a launch
    assert lib.mi355_mixer_token_x16_fwd(P(64), P(64), P(64), 1e-5, P(64), P(64), P(64), P(64), P(64), 2, 196, 256, 128, 1, P(64), 16, P(None)) == -1
    assert lib.mi355_patch_embed_x16_fwd(P(64), P(64), P(64), P(64), 2, 3, 224, 224, 16, 256, 1, P(64), 16, P(None)) == -1
    assert lib.mi355_version() == _ffi.ABI_VERSION


def test_header_states_envelope_and_ownership_of_every_new_entry():
    src = open(os.path.join(ROOT, "include", "mi355attn.h")).read()
    family = src[src.index("/* MLP-Mixer on fp16 / bf16 activations"):]
    family = family[:family.index("*/")]
    assert "The caller owns every buffer" in family and "MI355_EUNSUPPORTED" in family and "MI355_EINVAL" in family
    for name, words in (("mi355_mixer_token_x16_fwd", ("N = 196", "T % 32 == 0", "C % 256 == 0", "1024", "16-byte aligned")),
                        ("mi355_patch_embed_x16_fwd", ("% 64 == 0", "ps % 8 == 0", "W % 8 == 0", "E % 8 == 0", "16-byte aligned")),
                        ("mi355_token_mean_x16_fwd", ("C % 4 == 0", "aligned")),
                        ("mi355_widen16_fwd", ("16-byte aligned",)),
                        ("mi355_round16_fwd", ("16-byte aligned",))):
        at = src.index("int " + name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        for w in words:
            assert w in comment, f"the comment in front of {name} does not state {w!r}"
        assert re.search(r"\bint\s+io\b", src[at:src.index(";", at)]), f"{name} carries no `int io`"


def test_cpu_16bit_tensor_raises_the_device_error_not_type_error():
    import mi355attn
    from mi355attn.modules import MLP_Mixer, MixerLayer
    from mi355attn.modules.mixer import PatchEmbedding
    for dt in MC.DTYPES:
        for m, shape in ((MixerLayer(256, 196), (1, 196, 256)), (PatchEmbedding(32, 16, 3, 64), (1, 3, 32, 32)),
                         (MLP_Mixer(dim=64, depth=1, image_size=32, num_classes=4), (1, 3, 32, 32))):
            with pytest.raises(mi355attn.Mi355Error, match="no CPU path"):
                m.eval()(torch.zeros(*shape, dtype=dt))
    import inspect
    from mi355attn import _ffi
    text = "".join(re.findall(r'"([^"]*)"', inspect.getsource(_ffi.require_device_f32)))      # the refusal of every other module keeps its wording
    assert "PAM and CAM only" in text and "MixerLayer" in text and "MLP_Mixer" in text and "DoubleAttention" in text


def test_new_kernel_instantiations_have_no_scratch_and_fit_lds(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources                                            # needs msgpack: a missing package fails this test, it does not skip it
    rows = kernel_resources.kernels(built_lib)
    tok = [r for r in rows if re.search(r"\bmixer_token16_kernel<", r["demangled"])]
    names = [r["demangled"] for r in tok]
    for p in (1, 2):
        for early in ("false", "true"):
            for stats in (0, 2):
                k = f"mixer_token16_kernel<{p}, {early}, {stats}>"
                assert sum(k in n for n in names) == 1, f"no single instantiation {k} in {names}"
    assert len(tok) == 8, names
    others = [r for r in rows if any(s in r["demangled"] or s in r.get("name", "") for s in
                                     ("row_stats_x16_kernel", "im2col_gather16_kernel", "token_mean16_kernel", "widen16_kernel"))
              or re.search(r"(?<!da_)round16_kernel", r["demangled"])]
    assert len(others) == 6 + 1 + 2 + 2 + 2, [r["demangled"] for r in others]
    for r in tok + others:
        print(f"[mixer_io16 kernel] vgpr {r['vgpr']} agpr {r['agpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']}  {r['demangled'][:70]}")
        assert r["scratch"] == 0 and not r["spill_v"] and not r["spill_s"], (r["demangled"], r["scratch"], r["spill_v"], r["spill_s"])
        assert r["lds"] <= 163840, (r["demangled"], r["lds"])             # static part; the token kernel's dynamic 132 KB: MX_LDS below
    for r in tok:
        assert r["vgpr"] + r["agpr"] <= 256, (r["demangled"], r["vgpr"], r["agpr"])      # two waves per SIMD: 512 threads, launch bounds (512, 2)
    # the fp32-x instantiations are still there, one for one
    assert len([r for r in rows if re.search(r"\bmixer_token_kernel<", r["demangled"])]) == 8
    src = open(os.path.join(ROOT, "pytorch-attention_amd", "csrc", "mixer_fused.hip")).read()
    assert 'static_assert(MX_LDS <= 160 * 1024, "LDS budget")' in src


# ---- the interface roundings alone, in fp64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MC.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("cid", list(MC.LAYERS))
def test_layer_interface_roundings_stay_within_half_the_bar(cid, dtype):
    """The oracle on x rounded to the I/O type (the tensor a user hands over) with y rounded once, against the same oracle with y left
    wide: what the one rounding of the 16-bit store costs on assert_parity's two measures.  It is bounded by the unit roundoff of the
    type (2^-11 / 2^-8, below half of 1e-3 / 1.2e-2) whatever the seed, so at least half the bar of the GPU test is left to the
    kernels' own arithmetic.  (Measured against the oracle on the UNROUNDED fp32 x the figure would also hold the rounding of the input,
    which no 16-bit module can be charged with; the max-abs measure then lands between 5e-4 and 7e-4 in fp16 on these shapes, two
    half-ulps at the largest element, and passes or fails with the seed.  The seeds here were not selected.)"""
    plain, emu = MC.layer_plain(cid, dtype), MC.layer_emulated(cid, dtype)
    rf, ma = rel_fro(emu, plain), max_abs_ratio(emu, plain)
    half = TOL[MC.IO[dtype]] / 2
    print(f"[mixer_io16 emulation] {cid} {dtype}: rel_fro {rf:.3e} max_abs_ratio {ma:.3e} (half bar {half:.1e})")
    assert emu.dtype == dtype and rf <= half and ma <= half, (cid, dtype, rf, ma)


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=["fp16", "bf16"])
def test_model_interface_roundings_stay_within_half_the_bar(dtype):
    """MLP_Mixer(dim 256, depth 2) on the image rounded to the I/O type: the stream rounded behind the embedding and behind each layer and
    the logits rounded once, against the same oracle with nothing rounded inside."""
    plain, emu = MC.model_refs(dtype)
    rf, ma = rel_fro(emu, plain), max_abs_ratio(emu, plain)
    half = TOL[MC.IO[dtype]] / 2
    print(f"[mixer_io16 emulation] model {dtype}: rel_fro {rf:.3e} max_abs_ratio {ma:.3e} (half bar {half:.1e})")
    assert emu.dtype == dtype and rf <= half and ma <= half, (dtype, rf, ma)
