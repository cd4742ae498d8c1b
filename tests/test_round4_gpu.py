"""Round-4 boundary items ("Next round" 7 and the advisor's findings):

  * a kernel whose dynamic LDS depends on the shape (DoubleAttention(64,32,32): HW * 64 + 43 KB) runs a small image first and a large
    one afterwards (the attribute used to stay at the first value);
  * PAM at DANet's own width (dim = 512 > the attention kernel's widest head) against the oracle;
  * XCiT(drop_rate > 0) is the reference's eval-mode identity, and refused in train mode;
  * left-over rows of the two-accumulator GEMM on the ring-pipelined small tiles; LPI on 2 x 2 patches per lane.

The GCT / LCT capture test is in tests/test_chan_attn_gpu.py, the guarded_forward and range-guard tests in tests/test_range_guard_gpu.py,
the Mixer token-mixing tests in tests/test_mixer_gpu.py.
"""
import pytest
import torch

import oracle as O
from conftest import assert_parity
from kernel_cases import TAIL_SHAPES

pytestmark = pytest.mark.gpu


def test_dynamic_lds_limit_follows_the_largest_request():
    """double_attn_small asks for HW * 64 + 43 008 bytes of dynamic LDS: 16 x 16 first (59 KB), then 32 x 32 (109 KB) in the same process."""
    from mi355attn.modules import DoubleAttention
    torch.manual_seed(1234)
    m = DoubleAttention(64, 32, 32).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    keys = ("convA.weight", "convA.bias", "convB.weight", "convB.bias", "convV.weight", "convV.bias", "proj.weight", "proj.bias")
    m = m.cuda()
    for hw in (16, 32, 24, 32):
        torch.manual_seed(hw)
        x = torch.randn(4, 64, hw, hw)
        with torch.no_grad():
            y = m(x.cuda())
        torch.cuda.synchronize()
        ref = O.double_attention_forward(x, *[sd[k] for k in keys])
        assert_parity(y.cpu(), ref, 1e-3, f"DoubleAttention(64,32,32) at {hw}x{hw}")


@pytest.mark.parametrize("dim,hw", [(512, 24), (384, 16), (320, 16)])
def test_pam_wider_than_the_attention_kernel(dim, hw):
    from mi355attn.modules import PAM
    torch.manual_seed(1234)
    m = PAM(dim).eval()
    with torch.no_grad():
        m.alpha.fill_(0.7)
        for c in (m.b, m.c, m.d):
            c.weight.mul_(0.5)                                  # keeps the unscaled logits (a sum over `dim` channels) in a sane range
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(4321)
    x = torch.randn(2, dim, hw, hw) * 0.5
    ref = O.pam_forward(x, sd, dtype=torch.float64).float()
    with torch.no_grad():
        y = m.cuda()(x.cuda())
    torch.cuda.synchronize()
    assert_parity(y.cpu(), ref, 1e-3, f"PAM({dim}) at {hw}x{hw}")


def test_xcit_dropout_rates_are_eval_identities():
    from torch import nn
    from mi355attn.modules.xcit import XCiT
    kw = dict(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=4, eta=1.0, cls_attn_layers=1, norm_layer=nn.LayerNorm, num_classes=10)
    torch.manual_seed(1234)
    plain = XCiT(**kw).eval().cuda()
    torch.manual_seed(1234)
    dropped = XCiT(drop_rate=0.1, attn_drop_rate=0.2, **kw).eval().cuda()
    assert list(plain.state_dict().keys()) == list(dropped.state_dict().keys())
    x = torch.randn(3, 3, 64, 64, device="cuda")
    with torch.no_grad():
        a, b = plain(x), dropped(x)
    assert torch.equal(a, b)
    dropped.train()
    with pytest.raises(RuntimeError, match="eval"):
        dropped(x)
    with pytest.raises(ValueError):
        XCiT(drop_rate=1.5, **kw)


# ---- left-over rows of the two-accumulator GEMM on ring-pipelined small tiles (option "gemm_pa_tail"; gemm16.hip) -------------------
@pytest.mark.parametrize("prec,dt", [(1, torch.float16), (2, torch.bfloat16)])
@pytest.mark.parametrize("M,N,K,which", TAIL_SHAPES)
def test_left_over_rows_on_the_ring_kernel_are_bit_identical(M, N, K, which, prec, dt):
    import mi355attn
    from mi355attn import functional as F
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("round arithmetic of the shapes above assumes 256 CUs")
    torch.manual_seed(M + N + K)
    x16 = torch.randn(M, K, device="cuda").to(dt)
    w16 = (torch.randn(N, K, device="cuda") / K ** 0.5).to(dt)
    b = torch.randn(N, device="cuda")
    resid = torch.randn(M, N, device="cuda")
    for kw in (dict(bias=b, resid=resid), dict(bias=None, resid=resid), dict(bias=b, resid=resid, act=F.ACT_GELU)):
        with mi355attn.options(gemm_pa_tail=0):
            y_off = F.linear16(x16, w16, precision=prec, **kw)
        with mi355attn.options(gemm_pa_tail=30):
            tags = []
            y_on = [None]

            def run():
                y_on[0] = F.linear16(x16, w16, precision=prec, **kw)
            tags = [t for t, *_ in mi355attn.kernel_trace(run)]
            assert any(f"tail {which}" in t for t in tags), f"the ring kernel did not run: {tags}"
            y_on2 = F.linear16(x16, w16, precision=prec, **kw)
            torch.cuda.synchronize()
        assert torch.equal(y_on[0], y_on2), "run-to-run difference"
        assert torch.equal(y_off, y_on[0]), f"split launch differs from the single launch with {sorted(kw)}"
    with mi355attn.options(gemm_pa_tail=30):
        with mi355attn.options(gemm_variant=7):
            y7 = F.linear16(x16, w16, b, resid=resid, precision=prec)
        assert torch.equal(y7, F.linear16(x16, w16, b, resid=resid, precision=prec)), "differs from the round-1 tile kernel"
        # the last rows (the ring kernel's) against an fp64 product of the same 16-bit operands
        rows = slice(M - 96, M)
        ref = (x16[rows].double() @ w16.double().t() + b.double() + resid[rows].double()).float()
        assert_parity(F.linear16(x16, w16, b, resid=resid, precision=prec)[rows], ref, 2e-5, "fp64 product, last rows")


def test_left_over_rows_split_is_recorded_under_graph_capture():
    """Two plain launches on one stream: nothing to step aside for under capture."""
    import mi355attn
    from mi355attn import functional as F
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("assumes 256 CUs")
    torch.manual_seed(1)
    M, N, K = 128 * 392, 512, 2048
    x16 = torch.randn(M, K, device="cuda").half()
    w16 = (torch.randn(N, K, device="cuda") / K ** 0.5).half()
    resid = torch.randn(M, N, device="cuda")
    y_eager = F.linear16(x16, w16, None, resid=resid, precision=1)
    y_graph = torch.empty_like(y_eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.linear16(x16, w16, None, resid=resid, precision=1)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        y_graph.copy_(F.linear16(x16, w16, None, resid=resid, precision=1))
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_eager, y_graph)


# ---- LPI on 2 x 2 patches per lane (xcit.hip lpi_patch_kernel; option "lpi_patch") ---------------------------------------------------
@pytest.mark.parametrize("C,with_ln,with_tail", [(384, True, True), (96, False, True), (32, True, False), (64, False, False)])
def test_lpi_patch_kernel_against_the_general_kernel_and_the_oracle(C, with_ln, with_tail):
    """14 x 14 tokens, C % 32 == 0: the patch kernel (fused multiply-adds, taps in scalar registers) against the general kernel
    (option off: separately rounded products) to 1e-6, against the oracle, run-to-run bit identity, and a row's independence of the
    batch around it."""
    import mi355attn
    from mi355attn.modules import LPI
    torch.manual_seed(C + 7)
    B, H, W = 5, 14, 14
    m = LPI(C).eval()
    with torch.no_grad():
        m.bn.running_mean.normal_(0, 0.2)
        m.bn.running_var.uniform_(0.5, 1.5)
        m.bn.weight.uniform_(0.5, 1.5)
        m.bn.bias.normal_(0, 0.2)
    ln = torch.nn.LayerNorm(C)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.normal_(0, 0.2)
    x = torch.randn(B, H * W, C) * 1.5 + 0.3
    gamma = torch.rand(C) + 0.5
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m, ln = m.cuda(), ln.cuda()
    xd, gd = x.cuda(), gamma.cuda()
    kw = dict(gamma=gd, resid=xd) if with_tail else {}
    if with_ln:
        kw["ln"] = ln
    with torch.no_grad():
        with mi355attn.options(lpi_patch=1):
            tags = []
            out = [None]

            def run():
                out[0] = m(xd, H, W, **kw)
            tags = [t for t, *_ in mi355attn.kernel_trace(run)]
            assert any("lpi_patch_kernel" in t for t in tags), tags
            y1 = out[0]
            y1b = m(xd, H, W, **kw)
            y_one = m(xd[3:4].contiguous(), H, W, **({**kw, "resid": xd[3:4].contiguous()} if with_tail else kw))
        with mi355attn.options(lpi_patch=0):
            y0 = m(xd, H, W, **kw)
    torch.cuda.synchronize()
    assert torch.equal(y1, y1b), "run-to-run difference"
    assert torch.equal(y1[3:4], y_one), "a row's bits depend on the batch"
    assert_parity(y1.cpu(), y0.cpu(), 1e-6, "patch kernel vs general kernel")
    u = torch.nn.functional.layer_norm(x, (C,), ln.weight.cpu(), ln.bias.cpu(), ln.eps) if with_ln else x
    ref = O.lpi_forward(u, sd, H, W)
    if with_tail:
        ref = x + gamma * ref
    assert_parity(y1.cpu(), ref, 2e-5, "patch kernel vs oracle")
