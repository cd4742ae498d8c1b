"""GPU tests (-m gpu): PAM on any channel count from 1 to 2048 (mi355attn/modules/axis.py PAM._route).

  * parity with the fp64 oracle at the 1e-3 bar the suite holds PAM to (tests/test_round4_gpu.py, the same protocol: alpha = 0.7, conv
    weights x 0.5, x = randn x 0.5, seeds 1234 / 4321) for channel counts that run zero-padded on the streaming kernel (48, 50, 96, 100,
    160) and on the wide-head kernel sdpa_wide_kernel (576, 600, 768, 1000, 2048), on maps with partial key tiles and query blocks;
    neither route materialises logits (no qk_logits launch);
  * the routes that existed before keep their kernels and are deterministic;
  * precisions 1 and 2 of the wide kernel against the stream kernel's own error at width 256;
  * batch independence, the refusals of the C entry (nothing launched), the fp16 range guard of the wide kernel.
"""
import ctypes
import re
import warnings

import pytest
import torch

import oracle as O
from conftest import assert_parity, rel_fro
from kernel_cases import _drain_range, _tags

pytestmark = pytest.mark.gpu

PADDED = [(48, 6, 5), (50, 7, 7), (96, 8, 8), (100, 5, 9), (160, 4, 4)]
WIDE = [(576, 5, 7), (600, 8, 16), (768, 9, 15), (1000, 6, 6), (2048, 6, 8)]


def _pam(dim):
    from mi355attn.modules import PAM
    torch.manual_seed(1234)
    m = PAM(dim).eval()
    with torch.no_grad():
        m.alpha.fill_(0.7)
        for c in (m.b, m.c, m.d):
            c.weight.mul_(0.5)
    return m, {k: v.detach().clone() for k, v in m.state_dict().items()}


def _x(B, dim, h, w):
    torch.manual_seed(4321)
    return torch.randn(B, dim, h, w) * 0.5


def _logits_launch(tags):
    """A materialised logit matrix: mi355_qk_logits_fwd has no tag of its own, it launches the batched NT product of csrc/gemm.hip, the
    only gemm_kernel of a PAM forward with the A operand as it lies (a0; the 1x1 convs gather theirs from NCHW: a2)."""
    return any("qk_logits" in t or re.search(r"gemm_kernel<prec \d,b0,a0>", t) for t in tags)


def _finish():
    import mi355attn
    torch.cuda.synchronize()
    mi355attn.sync_status(wait=True)
    mi355attn.range_status(wait=True)


def _run_traced(m, xd):
    out = {}

    def run():
        with torch.no_grad():
            out["y"] = m(xd)
    tags = _tags(run)
    torch.cuda.synchronize()
    return out["y"], tags


@pytest.mark.parametrize("dim,h,w", PADDED + WIDE)
def test_pam_any_width_matches_fp64(dim, h, w):
    from mi355attn import functional as F
    m, sd = _pam(dim)
    x = _x(2, dim, h, w)
    ref = O.pam_forward(x, sd, dtype=torch.float64).float()
    y, tags = _run_traced(m.cuda(), x.cuda())
    rf, ma = assert_parity(y.cpu(), ref, 1e-3, f"PAM({dim}) at {h}x{w}")
    print(f"[pam any width] PAM({dim}) {h}x{w} strict: rel_fro {rf:.3e} max_abs_ratio {ma:.3e}")
    if (dim, h, w) in WIDE:
        assert any(f"sdpa_wide_kernel<d={(dim + 63) // 64 * 64},prec 0>" in t for t in tags), tags
        assert not any("sdpa_stream_kernel" in t for t in tags), tags
    else:
        assert any(f"sdpa_stream_kernel<d={F.attn_head_width(dim)}," in t for t in tags), tags
        assert not any("sdpa_wide_kernel" in t for t in tags), tags
    assert not _logits_launch(tags), tags
    _finish()


@pytest.mark.parametrize("dim,pair", [(64, False), (256, False), (320, True), (512, True)])
def test_existing_routes_keep_their_kernels(dim, pair):
    m, sd = _pam(dim)
    x = _x(2, dim, 6, 6)
    ref = O.pam_forward(x, sd, dtype=torch.float64).float()
    md, xd = m.cuda(), x.cuda()
    y, tags = _run_traced(md, xd)
    y2, _ = _run_traced(md, xd)
    assert torch.equal(y, y2), "run-to-run difference"
    assert_parity(y.cpu(), ref, 1e-3, f"PAM({dim}) at 6x6")
    att = [t for t in tags if "sdpa_" in t]
    assert not any("sdpa_wide_kernel" in t for t in att), att
    assert any("sdpa_stream_kernel<d=" in t for t in att), att
    assert _logits_launch(tags) == pair, tags
    if not pair:
        assert all(f"sdpa_stream_kernel<d={dim},prec 0>" in t for t in att), att
    _finish()


def _compose(m, xd, p):
    """PAM's forward with the whole width as ONE head of a direct F.sdpa_general call (the module sends 320 down the pair route)."""
    from mi355attn import functional as F
    c = xd.shape[1]
    rows, bias = m._fused()
    bcd, _ = F.conv2d_tokens(xd, None, bias, 1, 1, 0, 0, precision=p, wrows=rows)
    y = F.sdpa_general(bcd[:, :, :c], bcd[:, :, c:2 * c], bcd[:, :, 2 * c:], 1, 1.0, precision=p)
    return F.tokens_to_nchw_axpy(y, xd, m.alpha)


@pytest.mark.parametrize("p", [1, 2])
def test_wide_kernel_in_16_bit_operand_modes(p):
    """The bar is the stream kernel's own error: PAM(256) on an 8 x 8 map in this precision, measured here.  PAM(320) as one head on the
    wide kernel must stay within 2 x that figure (the 16-bit operand error of unscaled logits grows about sqrt(C): 1.12 x from 256 to 320;
    the factor 2 covers seed spread)."""
    errs = {}
    for dim in (256, 320):
        m, sd = _pam(dim)
        x = _x(2, dim, 8, 8)
        ref = O.pam_forward(x, sd, dtype=torch.float64)
        md, xd = m.cuda(), x.cuda()
        out = {}

        def run():
            with torch.no_grad():
                out["y"] = _compose(md, xd, p)
        tags = _tags(run)
        torch.cuda.synchronize()
        want = f"sdpa_stream_kernel<d=256,prec {p}>" if dim == 256 else f"sdpa_wide_kernel<d=320,prec {p}>"
        assert any(want in t for t in tags) and not _logits_launch(tags), tags
        assert torch.isfinite(out["y"]).all()
        errs[dim] = rel_fro(out["y"].cpu(), ref)
    print(f"[pam any width] precision {p}: PAM(256) stream kernel rel_fro {errs[256]:.3e}, PAM(320) wide kernel rel_fro {errs[320]:.3e}")
    assert errs[320] <= 2.0 * errs[256], f"precision {p}: wide kernel {errs[320]:.3e} vs stream kernel {errs[256]:.3e}"
    _finish()


@pytest.mark.parametrize("dim,h,w", [(768, 9, 15), (2048, 6, 8)])
def test_wide_module_in_16_bit_operand_modes(dim, h, w):
    m, sd = _pam(dim)
    x = _x(2, dim, h, w)
    ref = O.pam_forward(x, sd, dtype=torch.float64)
    md, xd = m.cuda(), x.cuda()
    errs = {}
    for p in (1, 2):
        md.precision = p
        y, tags = _run_traced(md, xd)
        assert any(f"sdpa_wide_kernel<d={dim},prec {p}>" in t for t in tags), tags
        assert torch.isfinite(y).all(), f"PAM({dim}) precision {p}: non-finite output"
        errs[p] = rel_fro(y.cpu(), ref)
        print(f"[pam any width] PAM({dim}) {h}x{w} precision {p}: rel_fro {errs[p]:.3e}")
    assert errs[1] <= errs[2], f"PAM({dim}): fp16 operands {errs[1]:.3e} worse than bf16 operands {errs[2]:.3e}"
    _finish()


def test_an_image_does_not_depend_on_its_batch():
    m, _ = _pam(768)
    x = _x(3, 768, 9, 15)
    md, xd = m.cuda(), x.cuda()
    with torch.no_grad():
        y3, y3b, y1 = md(xd), md(xd), md(xd[:1].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(y3, y3b), "run-to-run difference"
    assert torch.equal(y3[:1], y1), "image 0 of a batch of three differs from the same image alone"
    _finish()


def test_c_entry_refusals_launch_nothing():
    import mi355attn
    from mi355attn.modules import PAM
    lib = mi355attn.lib()
    _drain_range()
    torch.cuda.synchronize()
    mi355attn.sync_status(wait=True)

    def call(width, io16=0, with_bias=False, prec=1):
        dt = torch.float32 if not io16 else torch.float16
        q, k, v, o = (torch.full((1, 8, width), 3.0, dtype=dt, device="cuda") for _ in range(4))
        b = torch.zeros(1, 8, 8, device="cuda") if with_bias else None
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        rc = lib.mi355_sdpa_general_fwd(ptr(q), ptr(k), ptr(v), ptr(b), ptr(o), 1, 1, 8, 8, width, width, width, width, width, 0, 1.0,
                                        io16, prec, None)
        text = lib.mi355_last_error().decode()
        torch.cuda.synchronize()
        assert rc == 0 or bool((o == 3.0).all()), "a refused call wrote its output"
        return rc, text

    for kw, words in ((dict(width=512, io16=1), ("io16", "bias")), (dict(width=512, with_bias=True), ("io16", "bias")),
                      (dict(width=2112), ("2112", "2048")), (dict(width=352), ("352", "multiple of 64"))):
        rc, text = call(**kw)
        assert rc == -2, (kw, rc, text)                                   # MI355_EUNSUPPORTED
        assert "mi355_sdpa_general_fwd" in text and all(s in text for s in words), (kw, text)
    assert call(512)[0] == 0 and call(2048, prec=0)[0] == 0               # the same calls without the refused feature run
    with pytest.raises(NotImplementedError, match="2048"):
        PAM(2049).cuda()(torch.zeros(1, 2049, 2, 2, device="cuda"))
    _finish()


def test_fp16_range_guard_of_the_wide_kernel():
    """Precision 1 stages fp32 q / k / v to fp16: a finite value that becomes an fp16 inf is reported (range code 7, as by the stream
    kernel), and module(x) then returns the strict result with one warning."""
    import mi355attn
    from mi355attn import functional as F
    _drain_range()
    torch.manual_seed(7)
    q, k, v = (torch.randn(1, 40, 576, device="cuda") * 0.1 for _ in range(3))
    F.sdpa_general(q, k, v, 1, 1.0, precision=1)
    mi355attn.range_status(wait=True)                                     # ordinary data: nothing to report
    for which in range(3):
        t = [q.clone(), k.clone(), v.clone()]
        t[which][0, 37, 401] = 7.0e4                                      # finite in fp32, inf in fp16
        F.sdpa_general(*t, 1, 1.0, precision=1)
        with pytest.raises(mi355attn.Mi355RangeError):
            mi355attn.range_status(wait=True)
        mi355attn.range_status(wait=True)                                 # reported once
        F.sdpa_general(*t, 1, 1.0, precision=2)                           # bf16 has the fp32 range
        mi355attn.range_status(wait=True)
    # the module: b's weights scaled so that q passes 65504 while x and every weight stay inside fp16
    m, _ = _pam(576)
    with torch.no_grad():
        m.b.weight.mul_(2000.0)
    x = _x(2, 576, 5, 7) * 100.0
    md, xd = m.cuda(), x.cuda()
    with torch.no_grad():
        strict = md(xd)
        bcd, _ = F.conv2d_tokens(xd, None, md._fused(576)[1], 1, 1, 0, 0, precision=0, wrows=md._fused(576)[0])
    assert float(bcd[:, :, :576].abs().max()) > 65520.0 and float(xd.abs().max()) < 6.0e4, "the construction no longer saturates q alone"
    assert torch.isfinite(strict).all()
    md.precision = 1
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            y, tags = _run_traced(md, xd)
    hits = [i for i in w if "re-running this forward in strict mode" in str(i.message)]
    assert len(hits) == 1, [str(i.message) for i in w]
    assert any("sdpa_wide_kernel<d=576,prec 1>" in t for t in tags) and any("sdpa_wide_kernel<d=576,prec 0>" in t for t in tags), tags
    assert torch.equal(y, strict), "the fallback did not return the strict result"
    _finish()
