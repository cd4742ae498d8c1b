"""CPU tests of DoubleAttention on fp16 / bf16 activations (mi355_double_attn16_fwd, csrc/double_attn.hip and the 16-bit-I/O
instantiations of csrc/double_attn_small.hip / csrc/double_attn_fused.hip): the two C entries exist in the header, the built library and
the binding; they validate their arguments before any HIP call; a CPU 16-bit tensor raises the package's own error; the bars the GPU tests
use hold for the fp64 reference with the kernels' 16-bit rounding points alone; the 16-bit-I/O instantiations of the three fused kernels
exist for both types, use no scratch and fit a 512-thread workgroup."""
import ctypes
import os
import re
import sys

import pytest
import torch

import da_io16_arena_rows                                              # registers the entry's rows with tests/arena_cases.py
from conftest import ROOT, assert_parity

ENTRIES = ("mi355_double_attn16_fwd", "mi355_double_attn16_ws_bytes")
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
    proto = re.search(r"\bmi355_double_attn16_fwd\s*\(([^;]*?)\)\s*;", src, flags=re.S).group(1)
    assert re.search(r"\bint\s+io\b", proto) and not re.search(r"\bint\s+precision\b", proto)
    assert ffi.SIGNATURES["mi355_double_attn16_fwd"] == ffi.SIGNATURES["mi355_double_attn_fwd"]      # the same argument list, x / y as void*
    assert ffi.lib().mi355_version() == 1                              # additions only: the ABI version stays


def test_the_entry_has_arena_rows_in_both_types_and_forms():
    import arena_cases
    rows = [r for r in arena_cases.ROWS if "mi355_double_attn16_fwd" in r["entries"]]
    assert [r["id"] for r in rows] == da_io16_arena_rows.IDS and len(rows) == 12
    assert {r["prec"] for r in rows} == {1, 2} and {r["opts"]["da_fused"] for r in rows} == {0, 1}
    assert all(r["tol"] == arena_cases.TOL[r["prec"]] and arena_cases.BY_ID[r["id"]] is r for r in rows)


def _call(lib, io, p, B=2, C=64, cm=32, cn=32, H=8, W=8, ws=WS):
    return lib.mi355_double_attn16_fwd(p, p, p, p, p, p, p, p, p, p, B, C, cm, cn, H, W, io, p, ws, None)


def test_argument_validation_precedes_every_hip_call(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()
    for io in (1, 2):                                                  # null pointers
        assert _call(lib, io, None) == -1 and b"invalid argument" in lib.mi355_last_error(), (io, lib.mi355_last_error())
    for io in (0, 3, -1):                                              # io is checked before any pointer is looked at
        for ptr in (None, 64):
            assert _call(lib, io, ptr) == -1, (io, ptr)
            text = lib.mi355_last_error()
            assert b"invalid argument" in text and b"io" in text, text
        assert lib.mi355_double_attn16_ws_bytes(2, 64, 32, 32, 8, 8, io) == 0
    for kw in (dict(B=0), dict(C=0), dict(cm=0), dict(cn=-4), dict(H=0), dict(W=-1)):     # non-positive sizes
        assert _call(lib, 1, 64, **kw) == -1 and b"invalid argument" in lib.mi355_last_error(), kw
    # a workspace below mi355_double_attn16_ws_bytes: the one-kernel shape, and a general-route shape (fp32 result + widened x + the
    # fp32 entry's workspace)
    # (the one-kernel shape gets the general route's size, like mi355_double_attn_ws_bytes: unaligned parameters send it there)
    assert lib.mi355_double_attn16_ws_bytes(2, 64, 32, 32, 8, 8, 1) == 2 * 64 * 64 * 4 + lib.mi355_double_attn_workspace_bytes(2, 64, 32, 32, 8, 8)
    assert _call(lib, 1, 64, ws=8) == -1 and b"ws_bytes" in lib.mi355_last_error()
    need = lib.mi355_double_attn16_ws_bytes(2, 48, 12, 12, 6, 6, 2)
    assert need >= 2 * 2 * 48 * 36 * 4 + lib.mi355_double_attn_workspace_bytes(2, 48, 12, 12, 6, 6)
    assert _call(lib, 2, 64, C=48, cm=12, cn=12, H=6, W=6, ws=need - 16) == -1 and b"ws_bytes" in lib.mi355_last_error()


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_cpu_16bit_tensor_raises_the_package_error(built_lib, dtype):
    from mi355attn import Mi355Error
    from mi355attn.modules import DoubleAttention
    x = torch.randn(2, 64, 8, 8).to(getattr(torch, dtype))
    with pytest.raises(Mi355Error):
        DoubleAttention(64, 32, 32)(x)


def test_type_error_text_names_double_attention_and_keeps_the_other_names():
    src = open(os.path.join(ROOT, "pytorch-attention_amd", "mi355attn", "_ffi.py")).read()
    text = " ".join(re.findall(r'"([^"]*)"', src[src.index("def require_device_f32"):src.index("IO_CODES =")]))
    for name in ("SELayer", "ECALayer", "CBAM", "ChannelAttention", "SpatialAttention", "SELayerBias", "SELayerBias4", "SELayerHidden",
                 "SqueezeExcite", "simam_module", "SRM", "GaussianGCT", "LCT", "GCT", "DoubleAttention"):
        assert re.search(r"\b%s\b" % name, text), name


# ---- the bars, shown to hold for the reference with the kernels' roundings alone ------------------------------------------------------
def _emulate(x16, wA, bA, wB, bB, wV, bV, wP, bP, dt):
    """fp64 evaluation of DoubleAttention with a rounding to `dt` at every point where the fused kernels hold a 16-bit value: the
    weights, A, E = exp(b - max), the channel softmax of V, G, M' = WP G and the output.  Sums, maxima and biases stay fp64 (the
    kernels keep them in fp32, four orders below the 16-bit steps)."""
    r = lambda t: t.to(dt).double()
    B, C, H, W = x16.shape
    X = x16.double().reshape(B, C, H * W)
    pw = lambda w, b: torch.einsum("oc,bcn->bon", r(w.double().reshape(w.shape[0], -1)), X) + b.double()[None, :, None]
    A = r(pw(wA, bA))
    b = pw(wB, bB)
    e = torch.exp(b - b.amax(dim=2, keepdim=True))
    V = r(torch.softmax(pw(wV, bV), dim=1))
    G = r(torch.einsum("bmn,bkn->bmk", A, r(e)) / e.sum(dim=2)[:, None, :])
    M = r(torch.einsum("om,bmk->bok", r(wP.double().reshape(wP.shape[0], -1)), G))
    y = torch.einsum("bok,bkn->bon", M, V) + bP.double()[None, :, None]
    return r(y).reshape(B, wP.shape[0], H, W)


EMU = [((2, 64, 32, 32), 32), ((2, 64, 8, 8), 32), ((2, 256, 8, 8), 128), ((2, 128, 14, 14), 128), ((3, 72, 6, 6), 12)]


@pytest.mark.parametrize("dtype,tol", [("float16", 1e-3), ("bfloat16", 1.2e-2)])
def test_bars_hold_for_the_reference_with_16bit_roundings_alone(dtype, tol):
    import oracle.chan_attn as OC
    from mi355attn.modules import DoubleAttention
    dt = getattr(torch, dtype)
    worst = [0.0, 0.0]
    for shape, c in EMU:
        for seed in (0, 1):
            torch.manual_seed(seed)
            m = DoubleAttention(shape[1], c, c)                        # default Conv2d init
            p = [t.detach() for t in (m.convA.weight, m.convA.bias, m.convB.weight, m.convB.bias, m.convV.weight, m.convV.bias,
                                      m.proj.weight, m.proj.bias)]
            x16 = torch.randn(*shape).to(dt)
            ref = OC.double_attention_forward(x16.double(), *p, dtype=torch.float64)
            rf, ma = assert_parity(_emulate(x16, *p, dt), ref, tol, f"{shape} c {c} seed {seed} {dtype}")
            worst = [max(worst[0], rf), max(worst[1], ma)]
    print(f"[da16 emulation] {dtype}: rel_fro <= {worst[0]:.2e}, max-abs ratio <= {worst[1]:.2e} (bar {tol:g})")


# ---- kernel metadata ----------------------------------------------------------------------------------------------------------------
def test_io16_instantiations_exist_without_scratch_inside_a_512_thread_budget(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources                                            # needs msgpack: a missing package fails this test, it does not skip it
    rows = {r["demangled"]: r for r in kernel_resources.kernels(built_lib)}
    want = [f"da_small_kernel<{p}, 64, true>" for p in (1, 2)]
    want += [f"da_pass1_kernel<{p}, {ks}, true>" for p in (1, 2) for ks in (4, 8)]
    want += [f"da_pass2_kernel<{p}, {ct}, true>" for p in (1, 2) for ct in (1, 2)]
    for k in want:
        hit = [r for n, r in rows.items() if k in n]
        assert len(hit) == 1, f"no instantiation {k}: {sorted(n for n in rows if k.split('<')[0] in n)}"
        r = hit[0]
        print(f"[da16] {k}: vgpr {r['vgpr']} agpr {r['agpr']} sgpr {r['sgpr']} scratch {r['scratch']} lds {r['lds']}")
        assert not r["scratch"] and not r["spill_v"], (k, r)
        assert r["vgpr"] + r["agpr"] <= 256, (k, r["vgpr"], r["agpr"])  # two waves per SIMD: a 512-thread workgroup
        assert r["lds"] <= 160 * 1024, (k, r["lds"])
    # the fp32-I/O instantiations are still there, beside the new ones
    for k in ("da_small_kernel<1, 64, false>", "da_pass1_kernel<2, 8, false>", "da_pass2_kernel<1, 2, false>"):
        assert any(k in n for n in rows), k
