"""MixerLayer token mixing in one kernel (csrc/mixer_fused.hip; option "mixer_fused"): against the three-launch path it replaces and the
oracle of the whole layer; the entry refuses other geometries; the "mixer_early" epilogue variant and the row statistics computed
inside the kernel (option "mixer_stats") are bit-identical to the default.  Its range report: tests/test_range_guard_gpu.py."""
import pytest
import torch

import oracle as O
from conftest import assert_parity

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prec,tol", [(1, 1e-3), (2, 8e-3)])
@pytest.mark.parametrize("B,C", [(1, 256), (5, 512), (3, 768)])
def test_mixer_token_mixing_in_one_kernel(B, C, prec, tol):
    """N = 196 tokens, T = C / 2 hidden token units (128 / 256 / 384): the fused half (row statistics + one kernel) against the three-launch path it replaces,
    against the oracle of the whole layer, run-to-run bit identity, and an image's independence of its batch."""
    import mi355attn
    from mi355attn.modules import MixerLayer
    torch.manual_seed(B * 1000 + C)
    m = MixerLayer(C, 196, precision=prec).eval()
    with torch.no_grad():
        for ln in (m.norm1, m.norm2):
            ln.weight.uniform_(0.5, 1.5)
            ln.bias.normal_(0, 0.2)
        m.token_mlp.fc1.bias.normal_(0, 0.3)
        m.token_mlp.fc2.bias.normal_(0, 0.3)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.randn(B, 196, C) * 1.3 + 0.2
    ref = O.mixer_layer_forward(x, sd)
    m = m.cuda()
    xd = x.cuda()
    with torch.no_grad():
        with mi355attn.options(mixer_fused=1):
            out = [None]

            def run():
                out[0] = m(xd)
            tags = [t for t, *_ in mi355attn.kernel_trace(run)]
            assert any("mixer_token_kernel" in t for t in tags), tags
            assert not any("layernorm16_t" in t for t in tags), tags
            y1 = out[0]
            y1b = m(xd)
            y_last = m(xd[B - 1:].contiguous())
        with mi355attn.options(mixer_fused=0):
            y0 = m(xd)
    torch.cuda.synchronize()
    assert torch.isfinite(y1).all()
    assert torch.equal(y1, y1b), "run-to-run difference"
    assert torch.equal(y1[B - 1:], y_last), "an image's bits depend on the batch"
    assert_parity(y1.cpu(), ref, tol, "fused token mixing vs oracle")
    assert_parity(y0.cpu(), ref, tol, "three-launch token mixing vs oracle")
    assert_parity(y1.cpu(), y0.cpu(), tol, "fused vs three launches")


def test_mixer_token_entry_refuses_other_geometries():
    import ctypes
    import mi355attn
    from mi355attn import _ffi
    L = _ffi.lib()
    x = torch.zeros(1, 49, 256, device="cuda")
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = lambda t_: ctypes.c_void_p(t_.data_ptr())
    rc = L.mi355_mixer_token_fwd(p(x), p(buf), p(buf), 1e-5, p(buf), p(buf), p(buf), p(buf), p(x), 1, 49, 256, 256, 1, p(buf), 1 << 16,
                                 _ffi.stream_ptr(None))
    assert rc == -2, rc          # MI355_EUNSUPPORTED (include/mi355attn.h)


@pytest.mark.parametrize("prec", [1, 2])
def test_mixer_early_residual_variant_is_bit_identical(prec):
    import mi355attn
    from mi355attn.modules import MixerLayer
    torch.manual_seed(11)
    m = MixerLayer(512, 196, precision=prec).eval().cuda()
    x = torch.randn(7, 196, 512, device="cuda")
    with torch.no_grad():
        with mi355attn.options(mixer_early=0):
            y0 = m(x)
        with mi355attn.options(mixer_early=1):
            seen = []
            def run():
                seen.append(m(x))
            tags = [t for t, *_ in mi355attn.kernel_trace(run)]
    assert any("mixer_token_kernel<early>" in t for t in tags), tags
    assert torch.equal(y0, seen[0])


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("B,C", [(8, 512), (5, 512), (16, 256), (3, 768)])
def test_mixer_statistics_inside_the_token_kernel_are_bit_identical(B, C, prec):
    """Option "mixer_stats": LayerNorm row statistics computed inside mixer_token_kernel (phase 0, every workgroup of an image reads the
    image's rows once more; the two workgroups of an image get block ids 8 apart when B % 8 == 0) against the row_stats_kernel pre-pass:
    same per-lane sums in the same order, hence the same bits -- for one / two / three workgroups per image and both id mappings."""
    import mi355attn
    from mi355attn.modules import MixerLayer
    torch.manual_seed(B * 100 + C)
    m = MixerLayer(C, 196, precision=prec).eval().cuda()
    with torch.no_grad():
        m.norm1.weight.uniform_(0.5, 1.5)
        m.norm1.bias.normal_(0, 0.2)
    x = torch.randn(B, 196, C, device="cuda") * 1.7 + 0.3
    with torch.no_grad():
        with mi355attn.options(mixer_stats=0):
            t0 = [t for t, *_ in mi355attn.kernel_trace(lambda: m(x))]
            y0 = m(x)
        with mi355attn.options(mixer_stats=1):
            seen = []
            t1 = [t for t, *_ in mi355attn.kernel_trace(lambda: seen.append(m(x)))]
    assert any("row_stats_kernel" in t for t in t0), t0
    if C == 512:                                                       # phase 0 is built for C = 512 (two float4 per lane and row)
        assert not any("row_stats_kernel" in t for t in t1) and any("mixer_token_kernel<stats>" in t for t in t1), t1
    assert torch.isfinite(y0).all() and torch.equal(y0, seen[0])
