"""CPU tests (-m "not gpu") of CAM and PAM on fp16 / bf16 activations (csrc/dual_attn_io16.hip): the four entries are declared, exported
and bound with matching arity; the workspace query keeps its condition; every entry refuses a bad io, null pointers, a short workspace and
ld_tokens < C with MI355_EINVAL before any HIP call (fake pointers, as tests/test_ragged_maps_cpu.py uses them); the fp32 oracle rounded
once keeps the bounds the GPU tests use, for every shape and both types; the row table of tests/arena_cases.py covers the new entries."""
import ctypes
import os
import re

import pytest
import torch

import dual_io16_arena_rows
import dual_io16_cases as D
from conftest import ROOT
from io16_common import DTYPES

ENTRIES = {"mi355_cam16_ws_bytes": ("size_t", 5), "mi355_cam_x16_fwd": ("int", 11), "mi355_conv1x1_tokens16_fwd": ("int", 11),
           "mi355_tokens_to_nchw_axpy_x16_fwd": ("int", 10)}
EINVAL = -1


def _up32(v):
    return (v + 31) // 32 * 32


def test_entries_declared_exported_and_bound(built_lib):
    import mi355attn._ffi as ffi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355attn.h")).read(), flags=re.S)
    handle = ctypes.CDLL(built_lib)
    for name, (res, arity) in ENTRIES.items():
        proto = re.search(r"\b%s\s+%s\s*\(([^;]*?)\)\s*;" % (res, name), src, flags=re.S)
        assert proto, f"{name} is not declared in mi355attn.h"
        assert proto.group(1).count(",") + 1 == arity, name
        assert "precision" not in proto.group(1), f"{name}: the 16-bit entries have no precision parameter"
        assert hasattr(handle, name), f"{name} is not exported by the library"
        assert name in ffi.SIGNATURES and len(ffi.SIGNATURES[name][1]) == arity, name
        assert ffi.SIGNATURES[name][0] is (ffi.c_size if res == "size_t" else ffi.c_int), name
    assert ffi.lib().mi355_version() == 1                              # additions only: the ABI version stays


def test_workspace_query(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()
    for B, C, H, W in D.CAM_SHAPES + [(4, 512, 65, 65)]:
        Cp, HWp = _up32(C), _up32(H * W)
        for io in (1, 2):
            need = lib.mi355_cam16_ws_bytes(B, C, H, W, io)
            assert 4 * B * C * C <= need <= 4 * B * Cp * Cp + 2 * B * Cp * HWp + 4096, (B, C, H, W, io, need)
    for args in ((0, 64, 7, 7, 1), (2, 0, 7, 7, 1), (2, 64, 0, 7, 2), (2, 64, 7, -1, 2), (2, 64, 7, 7, 0), (2, 64, 7, 7, 3), (2, 64, 7, 7, -1)):
        assert lib.mi355_cam16_ws_bytes(*args) == 0, args


def test_entries_refuse_bad_arguments_before_any_launch(built_lib):
    from mi355attn import _ffi
    lib = _ffi.lib()
    P = 64                                                               # a fake, 16-byte aligned, non-null pointer: never dereferenced

    def refused(rc, *words):
        text = lib.mi355_last_error()
        assert rc == EINVAL and text and b"invalid argument" in text and all(w in text for w in words), (rc, text)

    need = lib.mi355_cam16_ws_bytes(2, 64, 7, 7, 1)
    cam = lambda x=P, beta=P, y=P, io=1, ws=P, n=need: lib.mi355_cam_x16_fwd(x, beta, y, 2, 64, 7, 7, io, ws, n, None)  # noqa: E731
    for io in (0, 3, -1):
        refused(cam(io=io), b"mi355_cam_x16_fwd", b"io")
    for kw in (dict(x=None), dict(beta=None), dict(y=None), dict(ws=None)):
        refused(cam(**kw), b"mi355_cam_x16_fwd")
    refused(cam(n=need - 16), b"workspace_bytes")
    refused(cam(ws=P + 4), b"workspace")                                 # a misaligned workspace
    refused(lib.mi355_cam_x16_fwd(P, P, P, 2, 0, 7, 7, 1, P, need, None), b"mi355_cam_x16_fwd")

    conv = lambda x=P, w=P, y=P, cin=30, ldw=32, io=2: lib.mi355_conv1x1_tokens16_fwd(x, w, None, y, 2, cin, 63, 90, ldw, io, None)  # noqa: E731
    for io in (0, 3):
        refused(conv(io=io), b"mi355_conv1x1_tokens16_fwd", b"io")
    for kw in (dict(x=None), dict(w=None), dict(y=None)):
        refused(conv(**kw), b"mi355_conv1x1_tokens16_fwd")
    refused(conv(ldw=28), b"ldw")                                        # ldw < Cin
    refused(conv(ldw=34), b"ldw")                                        # ldw % 4 != 0
    refused(conv(cin=0), b"mi355_conv1x1_tokens16_fwd")

    axpy = lambda tok=P, y=P, ld=30, io=1: lib.mi355_tokens_to_nchw_axpy_x16_fwd(tok, P, P, y, 2, 63, 30, ld, io, None)  # noqa: E731
    for io in (0, 3):
        refused(axpy(io=io), b"mi355_tokens_to_nchw_axpy_x16_fwd", b"io")
    for kw in (dict(tok=None), dict(y=None)):
        refused(axpy(**kw), b"mi355_tokens_to_nchw_axpy_x16_fwd")
    refused(axpy(ld=29), b"ld_tokens")                                   # ld_tokens < C


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", D.CAM_SHAPES, ids=D.sid)
def test_fp32_oracle_rounded_once_keeps_the_cam_bound(shape, dtype):
    x, ref = D.cam_case(shape, dtype)
    D.check(D.cam_ref(x, dtype=torch.float32).to(dtype), ref, dtype, D.T_CAM, f"fp32 oracle, CAM{shape} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", D.PAM_SHAPES, ids=D.sid)
def test_fp32_oracle_rounded_once_keeps_the_pam_bound(shape, dtype):
    x, m, ref = D.pam_case(shape, dtype)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    D.check(D.pam_ref(x, sd, dtype=torch.float32).to(dtype), ref, dtype, D.T_PAM, f"fp32 oracle, PAM{shape} {dtype}")


def test_subnormal_channel_input_and_what_a_flushed_gram_would_cost():
    """The input of the GPU test that decides the form of the fp16 Gram: channel 0 holds fp16 subnormals only, no other channel holds one;
    the fp32 evaluation rounded once keeps the bound, a Gram with the subnormals flushed misses it by two orders of magnitude."""
    x = D.subnormal_input()
    sub = (x != 0) & (x.abs().float() < 2.0 ** -14)
    assert bool(sub[0, 0].all()) and not bool(sub[0, 1:].any())
    ref = D.cam_ref(x)
    D.check(D.cam_ref(x, dtype=torch.float32).half(), ref, torch.float16, D.T_CAM, "fp32 oracle, subnormal channel")
    flushed = x.clone()
    flushed[0, 0] = 0
    xf, ff = x.double().flatten(2), flushed.double().flatten(2)
    attn = torch.softmax(ff @ ff.transpose(1, 2), dim=-1)               # only the Gram product sees the flushed operand
    y = (torch.tensor(D.R.CAM_BETA, dtype=torch.float64) * (attn @ xf)).reshape(x.shape) + x.double()
    with pytest.raises(AssertionError, match="x the bound"):
        D.check(y.half(), ref, torch.float16, D.T_CAM, "flushed Gram")


def test_arena_rows_cover_the_new_entries():
    import arena_cases
    covered = {s for r in arena_cases.ROWS for s in r["entries"]}
    assert {n for n in ENTRIES if n.endswith("_fwd")} <= covered
    rows = [arena_cases.BY_ID[i] for i in dual_io16_arena_rows.IDS]
    assert len(rows) == 12 and all(r["tol"] in (5e-5, 1e-3, 1.2e-2) for r in rows)
