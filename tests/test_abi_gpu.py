"""GPU side of the C-ABI checks (tests/test_abi.py compares header, exports and binding on the CPU): the SURVEY 8(b) spellings of three
entry points are exported and run the same code as the names the library uses."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_survey_8b_aliases_run_the_same_code():
    import mi355attn
    from mi355attn import _ffi
    L = mi355attn.lib()
    torch.manual_seed(3)
    qkv = torch.randn(2, 197, 3 * 768, device="cuda")
    a, b = torch.empty(2, 197, 768, device="cuda"), torch.empty(2, 197, 768, device="cuda")
    st = _ffi.stream_ptr(qkv.device)
    assert L.mi355_sdpa_fwd(_ffi.dptr(qkv), _ffi.dptr(a), 2, 197, 12, 64, ctypes.c_float(0.125), 1, st) == 0
    assert L.mi355_sdpa_core_fwd(_ffi.dptr(qkv), _ffi.dptr(b), 2, 197, 12, 64, ctypes.c_float(0.125), 1, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    x, w, bias = torch.randn(64, 256, device="cuda"), torch.randn(128, 256, device="cuda"), torch.randn(128, device="cuda")
    y0, y1 = torch.empty(64, 128, device="cuda"), torch.empty(64, 128, device="cuda")
    for fn, y in ((L.mi355_linear_fwd, y0), (L.mi355_gemm_bias_act_fwd, y1)):
        assert fn(_ffi.dptr(x), _ffi.dptr(w), _ffi.dptr(bias), None, None, _ffi.dptr(y), 64, 128, 256, 256, 128, 1, 1, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
    assert L.mi355_mixer_token_mlp_workspace_bytes(4, 196, 512) == L.mi355_mixer_token_workspace_bytes(4, 196, 512) > 0
    assert L.mi355_xca_workspace_bytes(2, 196, 8, 48) == 0 and L.mi355_layernorm_workspace_bytes(10, 64) == 0
    assert L.mi355_cswin_lepe_attn_workspace_bytes(2, 56, 64) == 0 and L.mi355_sdpa_core_workspace_bytes(2, 197, 12, 64) == 0
