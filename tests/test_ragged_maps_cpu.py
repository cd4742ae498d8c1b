"""CPU tests (-m "not gpu") of DoubleAttention and CAM on maps whose H*W or channel counts are no multiples of 4 (the ragged routes of
csrc/double_attn.hip and csrc/sk_dual.hip on csrc/ragged_maps.hip): the new workspace query exists in the header, the library and the
binding; the workspace queries grow for ragged shapes only; the oracle the GPU tests compare with equals the real reference's modules on
every ragged shape (where a reference checkout is present); CAM's input scale keeps the oracle's own fp32 evaluation a factor ten inside the
precision-0 bar."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

import oracle.axis_attn as OA
import oracle.chan_attn as OC
import ragged_cases as R
from conftest import ROOT, max_abs_ratio, rel_fro

REFERENCE = os.environ.get("MI355_REFERENCE", "/root/reference")


def _up4(v):
    return (v + 3) & ~3


def test_cam_ws_bytes_declared_exported_and_bound(built_lib):
    import mi355attn._ffi as ffi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355attn.h")).read(), flags=re.S)
    proto = re.search(r"\bsize_t\s+mi355_cam_ws_bytes\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert proto, "mi355_cam_ws_bytes is not declared in mi355attn.h"
    assert [a.split()[0] for a in proto.group(1).split(",")] == ["int"] * 4
    assert hasattr(ctypes.CDLL(built_lib), "mi355_cam_ws_bytes"), "mi355_cam_ws_bytes is not exported by the library"
    assert ffi.SIGNATURES["mi355_cam_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    assert ffi.lib().mi355_version() == 1                              # additions only: the ABI version stays


def test_cam_workspace_query(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()
    for B, C, H, W in ((2, 64, 32, 32), (4, 256, 28, 28)):
        assert lib.mi355_cam_ws_bytes(B, C, H, W) == lib.mi355_cam_workspace_bytes(B, C) > 0
    for B, C, H, W in ((2, 64, 7, 7), (3, 30, 9, 7)):
        need = lib.mi355_cam_ws_bytes(B, C, H, W)
        assert need > lib.mi355_cam_workspace_bytes(B, C)
        assert need >= 4 * B * _up4(C) * (_up4(C) + _up4(H * W))       # the Gram matrices and the padded image
    for args in ((0, 64, 7, 7), (2, 0, 7, 7), (2, 64, 0, 7), (2, 64, 7, -1)):
        assert lib.mi355_cam_ws_bytes(*args) == 0
    assert lib.mi355_cam_workspace_bytes(0, 64) == 0 and lib.mi355_cam_workspace_bytes(2, -4) == 0
    # a ragged call with the aligned query's size is refused before anything is launched
    small = lib.mi355_cam_workspace_bytes(2, 64)
    assert lib.mi355_cam_fwd(64, 64, 64, 2, 64, 7, 7, 0, 64, small, None) == -1 and b"workspace_bytes" in lib.mi355_last_error()


def test_double_attention_workspace_queries(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()
    # aligned shapes: byte for byte what the entries returned before the ragged route (the expressions of tests/test_da_io16_cpu.py)
    gen = lib.mi355_double_attn_workspace_bytes
    for prec in (0, 1, 2):
        assert lib.mi355_double_attn_ws_bytes(2, 64, 32, 32, 8, 8, prec) == gen(2, 64, 32, 32, 8, 8)
        assert lib.mi355_double_attn_ws_bytes(2, 48, 12, 12, 6, 6, prec) == gen(2, 48, 12, 12, 6, 6)
    for io in (1, 2):
        assert lib.mi355_double_attn16_ws_bytes(2, 64, 32, 32, 8, 8, io) == 2 * 64 * 64 * 4 + gen(2, 64, 32, 32, 8, 8)
        assert lib.mi355_double_attn16_ws_bytes(2, 48, 12, 12, 6, 6, io) == 2 * 2 * 48 * 36 * 4 + gen(2, 48, 12, 12, 6, 6)
    # a ragged shape: at least the padded tensors
    B, C, cm, cn, H, W = 2, 30, 10, 6, 9, 7
    Cp, cmp_, cnp, HWp = _up4(C), _up4(cm), _up4(cn), _up4(H * W)
    M3p = cmp_ + 2 * cnp
    padded = 4 * (B * Cp * HWp + M3p * Cp + M3p + C * cmp_ + B * M3p * HWp + B * cmp_ * cnp + B * C * cnp)
    for prec in (0, 1, 2):
        assert lib.mi355_double_attn_ws_bytes(B, C, cm, cn, H, W, prec) >= padded
    for io in (1, 2):
        assert lib.mi355_double_attn16_ws_bytes(B, C, cm, cn, H, W, io) >= padded + 4 * B * C * H * W
    assert lib.mi355_double_attn16_ws_bytes(B, C, cm, cn, H, W, 0) == 0
    # ... and a workspace below the query is refused before anything is launched
    need = lib.mi355_double_attn_ws_bytes(B, C, cm, cn, H, W, 0)
    args = [64] * 10 + [B, C, cm, cn, H, W]
    assert lib.mi355_double_attn_fwd(*args, 0, 64, need - 16, None) == -1 and b"ws_bytes" in lib.mi355_last_error()
    need = lib.mi355_double_attn16_ws_bytes(B, C, cm, cn, H, W, 1)
    assert lib.mi355_double_attn16_fwd(*args, 1, 64, need - 16, None) == -1 and b"ws_bytes" in lib.mi355_last_error()


def _reference_module(name):
    path = os.path.join(REFERENCE, "attention_mechanisms", name + ".py")
    if not os.path.exists(path):
        pytest.skip("no reference checkout (MI355_REFERENCE)")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("case", R.DA, ids=R.da_id)
def test_oracle_equals_the_reference_double_attention(case):
    ref_cls = _reference_module("double_attention").DoubleAttention
    m = R.da_module(case, cls=ref_cls)
    x = R.da_input(case)
    with torch.no_grad():
        want = m(x)
    got = OC.double_attention_forward(x, *R.da_params(m))
    assert rel_fro(got, want) <= 1e-5 and max_abs_ratio(got, want) <= 1e-5, (rel_fro(got, want), max_abs_ratio(got, want))


@pytest.mark.parametrize("shape", R.CAM, ids=R.cam_id)
def test_oracle_equals_the_reference_cam(shape):
    m = _reference_module("dual_attention").CAM().eval()
    x = R.cam_input(shape)
    with torch.no_grad():
        m.beta.fill_(R.CAM_BETA)
        want = m(x)
    got = OA.cam_forward(x, {"beta": m.beta.detach()})
    assert rel_fro(got, want) <= 1e-5 and max_abs_ratio(got, want) <= 1e-5, (rel_fro(got, want), max_abs_ratio(got, want))


@pytest.mark.parametrize("shape", R.CAM, ids=R.cam_id)
def test_cam_input_scale_keeps_the_fp32_oracle_a_tenth_inside_the_strict_bar(shape):
    """The Gram logits are unscaled sums over HW; at the scale of ragged_cases.cam_input the softmax is well enough conditioned that an
    fp32 evaluation of the reference's own operator sequence stays within TOL[0] / 10 of the fp64 one, so a miss of the GPU tests at
    this scale is the kernels'."""
    r64, r32 = R.cam_ref(shape), R.cam_ref(shape, torch.float32)
    rf, ma = rel_fro(r32, r64), max_abs_ratio(r32, r64)
    print(f"[ragged] CAM {R.cam_id(shape)}: fp32 oracle vs fp64 rel_fro {rf:.2e} max-abs ratio {ma:.2e} (bar {R.TOL[0] / 10:g})")
    assert rf <= R.TOL[0] / 10 and ma <= R.TOL[0] / 10
    # the block is not the identity at this scale: the attention term is a visible part of the output
    x = R.cam_input(shape).double()
    assert rel_fro(r64, x) >= 0.05
