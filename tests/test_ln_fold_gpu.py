"""LayerNorm folded into the GEMMs around it (csrc/ln_fold.hip; round 4): op-level contracts and block-level parity.

  * producer  mi355_linear16_emit_fwd: Y bit-identical to mi355_linear16_fwd; the emitted operand is exactly T(Y - c); the group pairs
    reproduce the row statistics;
  * finalize  rowtau = {rstd, rstd (c - mean)}, c := mean; rows outside the band (mean moved by more than tol * std, std outside the
    fp16 band: 1e5- and 1e-6-scale streams) are rewritten as the plain LayerNorm operand and counted;
  * consumer  act(LayerNorm(Y) W^T + b) within the operand rounding of the unfolded path (LayerNorm -> 16 bit -> GEMM), checked against
    an fp64 reference and against the unfolded path's own error;
  * TransformerEncoder / VisionTransformer blocks (ViT.py:116-119) with the fold on and off against the oracle at a fold-eligible
    batch (rows % 128 == 0), run-to-run bit identity, and independence of a row from the batch around it among eligible batches.
"""
import pytest
import torch

import oracle as O
from conftest import assert_parity, rel_fro

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _ln_fold_enabled():
    """The fold is opt-in (option "ln_fold", default 0: DESIGN.md 6.2c): these tests switch it on for their duration."""
    import mi355attn
    with mi355attn.options(ln_fold=1):
        yield


def _ref_ln(y, gamma, beta, eps=1e-5):
    yd = y.double()
    mu = yd.mean(-1, keepdim=True)
    var = ((yd - mu) ** 2).mean(-1, keepdim=True)
    return (yd - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def _gelu(t):
    return torch.nn.functional.gelu(t)


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("act", [0, 1])
def test_emit_finalize_consume_against_fp64(prec, act):
    import mi355attn
    from mi355attn import functional as F
    torch.manual_seed(7)
    M, C, K = 128 * 5, 768, 768
    dt = F.dtype16(prec)
    x16 = (torch.randn(M, K, device="cuda") * 0.7).to(dt)
    w = (torch.randn(C, K, device="cuda") / K ** 0.5)
    w16 = w.to(dt)
    bias = torch.randn(C, device="cuda") * 0.1
    resid = torch.randn(M, C, device="cuda") * 1.5 + torch.randn(M, 1, device="cuda") * 3.0        # per-row means of a few std
    c_before = resid.mean(-1).contiguous()                                                          # the "previous LayerNorm's" means
    cvec = c_before.clone()
    slow = torch.zeros(1, dtype=torch.int32, device="cuda")
    y, st = F.linear16_emit(x16, w16, bias, resid, cvec, 1e-5, act=act, precision=prec, slow_rows=slow)
    y_plain = F.linear16(x16, w16, bias, act=act, resid=resid, precision=prec)
    torch.cuda.synchronize()
    assert torch.equal(y, y_plain), "the emitting epilogue changed Y"
    yd = y.double()
    mu, var = yd.mean(-1), yd.var(-1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    assert int(slow.item()) == 0, "well-conditioned rows took the slow path"
    assert torch.equal(st.a16, (y - c_before[:, None]).to(dt)), "emitted operand is not T(Y - c)"
    assert torch.allclose(st.cvec.double(), mu, rtol=0, atol=2e-6 * float(yd.abs().max()))
    assert torch.allclose(st.rowtau[:, 0].double(), rstd, rtol=2e-6, atol=0)
    assert torch.allclose(st.rowtau[:, 1].double(), rstd * (c_before.double() - mu), rtol=1e-4, atol=1e-5)
    # consumer against fp64 and against the unfolded path
    ln = torch.nn.LayerNorm(C).cuda()
    lin = torch.nn.Linear(C, 1024).cuda()
    with torch.no_grad():
        ln.weight.copy_(1.0 + 0.3 * torch.randn(C, device="cuda"))
        ln.bias.copy_(0.2 * torch.randn(C, device="cuda"))
    wf, cs, bf = F.lnfold_weights(ln, lin, prec)
    out = F.linear16_lnfold(st, wf, bf, cs, act=F.ACT_GELU, precision=prec).float()
    u16 = F.layernorm16(y, ln.weight, ln.bias, ln.eps, prec)
    out_unf = F.linear16(u16, F.weight16(lin.weight, prec), lin.bias, act=F.ACT_GELU, out16=True, precision=prec).float()
    ref = _gelu((_ref_ln(y, ln.weight.detach(), ln.bias.detach()) @ lin.weight.detach().double().t() + lin.bias.detach().double()).float())
    e_fold, e_unf = rel_fro(out, ref), rel_fro(out_unf, ref)
    tol = 1e-3 if prec == 1 else 8e-3
    assert e_fold <= tol, f"folded consumer off the fp64 reference: {e_fold:.3e}"
    assert e_fold <= 1.6 * e_unf + 1e-5, f"folded path lost accuracy against LayerNorm -> 16 bit -> GEMM: {e_fold:.3e} vs {e_unf:.3e}"
    mi355attn.range_status(wait=True)


@pytest.mark.parametrize("case", ["mean_jump", "scale_1e5", "scale_1e-6", "mixed"])
def test_rows_outside_the_band_are_rewritten(case):
    """The heuristic (c = previous mean) is never trusted: a row whose mean moved by more than tol * std, or whose std leaves the fp16
    band, is rewritten from the fp32 stream -- the consumer's result stays on the reference."""
    from mi355attn import functional as F
    torch.manual_seed(11)
    M, C, K, prec = 256, 768, 768, 1
    x16 = (torch.randn(M, K, device="cuda") * 0.5).half()
    w16 = (torch.randn(C, K, device="cuda") / K ** 0.5).half()
    resid = torch.randn(M, C, device="cuda")
    c_before = resid.mean(-1).contiguous()
    if case == "mean_jump":
        resid = resid + 5.0                                  # every row's mean moves by 5 std: c is useless
        expect_slow = M
    elif case == "scale_1e5":
        resid = resid * 1.0e5
        c_before = resid.mean(-1).contiguous()
        expect_slow = M
    elif case == "scale_1e-6":
        resid = resid * 1.0e-6
        x16 = x16 * 0
        c_before = resid.mean(-1).contiguous()
        expect_slow = M
    else:
        resid[::3] += 7.0                                    # a third of the rows jump
        expect_slow = len(range(0, M, 3))
    cvec = c_before.clone()
    slow = torch.zeros(1, dtype=torch.int32, device="cuda")
    y, st = F.linear16_emit(x16, w16, None, resid, cvec, 1e-5, precision=prec, slow_rows=slow)
    torch.cuda.synchronize()
    assert int(slow.item()) == expect_slow
    ln = torch.nn.LayerNorm(C).cuda()
    lin = torch.nn.Linear(C, 512).cuda()
    wf, cs, bf = F.lnfold_weights(ln, lin, prec)
    out = F.linear16_lnfold(st, wf, bf, cs, precision=prec).float()
    ref = (_ref_ln(y, ln.weight.detach(), ln.bias.detach()) @ lin.weight.detach().double().t() + lin.bias.detach().double()).float()
    assert torch.isfinite(out).all()
    assert rel_fro(out, ref) <= 1e-3, f"{case}: {rel_fro(out, ref):.3e}"


def test_center16_is_the_plain_operand():
    from mi355attn import functional as F
    torch.manual_seed(3)
    x = torch.randn(300, 768, device="cuda") * 4 + 2
    st = F.ln_center16(x, 1e-5, 1)
    one, zero = torch.ones(768, device="cuda"), torch.zeros(768, device="cuda")
    ref = F.layernorm16(x, one, zero, 1e-5, 1)
    torch.cuda.synchronize()
    assert torch.equal(st.a16, ref)
    assert torch.equal(st.rowtau, torch.tensor([1.0, 0.0], device="cuda").expand(300, 2))
    assert torch.allclose(st.cvec, x.mean(-1), atol=1e-5)


def _encoder(seed=1234):
    from mi355attn.modules import TransformerEncoder
    torch.manual_seed(seed)
    return TransformerEncoder(768, 12).eval()


@pytest.mark.parametrize("scale", [1.0, 1.0e5])
def test_transformer_encoder_folded_vs_oracle(scale):
    """B = 128 images of 197 tokens = 25 216 rows (% 128 == 0): the folded path; images 0 / 63 / 127 against the oracle.  At 1e5 the
    residual stream leaves the fp16 band and every row of LayerNorm 2 goes through the rewrite."""
    import mi355attn
    blk = _encoder()
    with torch.no_grad():                                    # away from the default initialisation: non-trivial gains and shifts
        for ln in (blk.layernorm1, blk.layernorm2):
            ln.weight.add_(0.2 * torch.randn(768))
            ln.bias.add_(0.1 * torch.randn(768))
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    g = torch.Generator().manual_seed(4321)
    x = torch.randn(128, 197, 768, generator=g) * scale
    pick = [0, 63, 127]
    ref = O.vit_encoder_forward(x[pick], sd, 12)
    blk = blk.cuda()
    xd = x.cuda()
    assert blk.fold_ok(xd)
    with torch.no_grad():
        y = blk(xd)
        y2 = blk(xd)
        with mi355attn.options(ln_fold=0):
            assert not blk.fold_ok(xd)
            y_unf = blk(xd)
    mi355attn.range_status(wait=True)
    assert torch.equal(y, y2), "run-to-run results differ"
    assert_parity(y[pick].cpu(), ref, 1e-3, f"folded TransformerEncoder at scale {scale:g}")
    assert_parity(y_unf[pick].cpu(), ref, 1e-3, f"unfolded TransformerEncoder at scale {scale:g}")
    d = rel_fro(y, y_unf)
    print(f"[ln_fold] scale {scale:g}: folded vs oracle {rel_fro(y[pick].cpu(), ref):.3e}, unfolded vs oracle {rel_fro(y_unf[pick].cpu(), ref):.3e}, "
          f"folded vs unfolded {d:.3e}")
    assert d <= 8e-4


def test_folded_rows_do_not_depend_on_the_batch():
    """Among fold-eligible batches a row's result is bit-identical whatever surrounds it (every piece of the fold is row-local)."""
    blk = _encoder().cuda()
    g = torch.Generator().manual_seed(99)
    x = torch.randn(256, 197, 768, generator=g).cuda()
    with torch.no_grad():
        y256 = blk(x)
        y128 = blk(x[128:].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(y256[128:], y128)


def test_vit_chain_state_travels_between_blocks():
    """Three encoder blocks driven like VisionTransformer.forward (the LnState of block i + 1 comes out of block i's fc2) against
    the same blocks called one by one (each starting from mi355_ln_center16_fwd): same rows up to the operand rounding, and the
    chain launches no LayerNorm kernel after the first."""
    from mi355attn.modules import TransformerEncoder
    torch.manual_seed(5)
    blocks = [TransformerEncoder(768, 12).eval().cuda() for _ in range(3)]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(128, 197, 768, generator=g).cuda()
    with torch.no_grad():
        t, state = x, None
        for i, b in enumerate(blocks):
            nxt = blocks[i + 1].layernorm1.eps if i + 1 < len(blocks) else None
            t, state = b.forward_folded(t, state, nxt)
        u = x
        for b in blocks:
            u = b(u)
    torch.cuda.synchronize()
    assert state is None
    assert rel_fro(t, u) <= 6e-4
    sd = [{k: v.detach().cpu() for k, v in b.state_dict().items()} for b in blocks]
    r = x[:2].cpu()
    for s in sd:
        r = O.vit_encoder_forward(r, s, 12)
    assert_parity(t[:2].cpu(), r, 1e-3, "three folded blocks")
