"""Precision 3 ("logit-compensated") on the GPU: the two kernels alone against fp64, the gated margin case (C3 `Attention(768, 12)`,
ViT.py:79-89, at B = 16 over five seed pairs and weight scales 1-4; C5 `VisionTransformer(num_heads=12)`, ViT.py:180-192, gated at
scales 1-2 and recorded at 3), and the mode's boundaries: exactly precision 1 outside ViT attention, exactly precision 0 outside the
kernels' envelope, the range fallback, and a default that does not move.

Bars (not tuned to the results): 1e-3 on both criteria is the project's parity bar; 5e-5 is the bar the project already uses
for split-bf16 (strict) results (tests/test_parity_margin_gpu.py); 3e-3 is that file's outer bound for cells that are recorded.
Truth is the fp64 oracle.  The cells are written to $MI355_LOGIT_OUT (default: mi355_logit_mode_margin.md in the system's temporary
directory); profiles/logit_mode.md holds a committed copy.
"""
import os
import subprocess
import sys
import tempfile
import warnings

import pytest
import torch

import oracle as O
from conftest import PKG, assert_parity, max_abs_ratio, rel_fro

pytestmark = pytest.mark.gpu

SEEDS = [(1234, 4321), (1, 2), (7, 11), (2024, 930), (31337, 271828)]
B = 16
_rows = []


@pytest.fixture(autouse=True)
def _default_restored():
    import mi355attn
    yield
    mi355attn.set_default_precision(1)


# ---- the kernels alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("C", [384, 768])
@pytest.mark.parametrize("M", [197, 16 * 197, 1000])
def test_projection_kernel_vs_fp64(M, C, bias):
    from mi355attn import functional as F
    torch.manual_seed(C + M)
    w = torch.nn.init.trunc_normal_(torch.empty(3 * C, C), std=.02) * 3.0
    b = torch.randn(3 * C) * 0.5 if bias else None
    x = torch.randn(M, C)
    ref = x.double() @ w.double().t() + (b.double() if bias else 0.0)
    hi, lo, v16 = F.split_qkv_weight(w.cuda())
    y = F.qkv_split16(x.cuda(), hi, lo, v16, b.cuda() if bias else None)
    assert tuple(y.shape) == (M, 5 * C) and y.dtype == torch.int16
    qh, ql, kh, kl, v = (t.cpu() for t in F.qkv_split16_planes(y))
    assert qh.dtype == torch.bfloat16 and v.dtype == torch.float16
    q, k = qh.double() + ql.double(), kh.double() + kl.double()
    for name, got, want, tol in (("q", q, ref[:, :C], 5e-5), ("k", k, ref[:, C:2 * C], 5e-5), ("v", v, ref[:, 2 * C:], 1e-3)):
        rf, ma = rel_fro(got, want), max_abs_ratio(got, want)
        print("[logit-mode] projection M %d C %d %s %s: rel_fro %.2e max_abs %.2e" % (M, C, "bias" if bias else "nobias", name, rf, ma))
        assert_parity(got, want, tol, "projection %s (M %d, C %d)" % (name, M, C))
    F.range_status(wait=True)


@pytest.mark.parametrize("N", [49, 197, 224])
@pytest.mark.parametrize("d", [32, 64])
def test_core_kernel_vs_fp64(d, N):
    from mi355attn import functional as F
    heads, Bc = 6, 3
    C = heads * d
    torch.manual_seed(d * 1000 + N)
    a = 5.0 ** 0.5                                                      # q.k / sqrt(d) then has std ~ a^2 = 5
    q, k, v = torch.randn(Bc, N, C) * a, torch.randn(Bc, N, C) * a, torch.randn(Bc, N, C)
    qh = q.to(torch.bfloat16); ql = (q - qh.float()).to(torch.bfloat16)
    kh = k.to(torch.bfloat16); kl = (k - kh.float()).to(torch.bfloat16)
    v16 = v.half()
    qkv5 = torch.cat([t.view(torch.int16) for t in (qh, ql, kh, kl, v16)], dim=-1).contiguous()
    q64, k64, v64 = qh.double() + ql.double(), kh.double() + kl.double(), v16.double()     # the operands the kernel is given, exactly
    ref = torch.empty(Bc, N, C, dtype=torch.float64)
    for h in range(heads):
        sl = slice(h * d, (h + 1) * d)
        s = (q64[..., sl] @ k64[..., sl].transpose(-1, -2)) * d ** -0.5
        if h == 0:
            print("[logit-mode] core d %d N %d: logit std %.2f" % (d, N, float(s.std())))
        ref[..., sl] = torch.softmax(s, dim=-1) @ v64[..., sl]
    out = F.sdpa16_split(qkv5.cuda(), heads, d ** -0.5)
    assert out.dtype == torch.float16 and tuple(out.shape) == (Bc, N, C)
    rf, ma = assert_parity(out.cpu(), ref, 1e-3, "core (d %d, N %d)" % (d, N))
    print("[logit-mode] core d %d N %d: rel_fro %.2e max_abs %.2e" % (d, N, rf, ma))


def test_entries_reject_shapes_outside_the_envelope():
    """Unsupported-shape code, nothing launched, never an abort; the existing entries keep rejecting precision 3."""
    from mi355attn import _ffi
    lib = _ffi.lib()
    t = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    p, st = _ffi.dptr(t), _ffi.stream_ptr(t.device)
    assert lib.mi355_qkv_split16_fwd(p, p, p, p, None, p, 8, 96, 64, 64, st) == _ffi.MI355_EUNSUPPORTED       # C % 64
    assert lib.mi355_qkv_split16_fwd(p, p, p, p, None, p, 8, 64, 96, 96, st) == _ffi.MI355_EUNSUPPORTED       # K % 64
    assert lib.mi355_qkv_split16_fwd(None, p, p, p, None, p, 8, 64, 64, 64, st) == -1
    assert lib.mi355_sdpa16_split_fwd(p, p, 1, 16, 1, 48, 0.1, st) == _ffi.MI355_EUNSUPPORTED                  # head width
    assert lib.mi355_sdpa16_split_fwd(p, p, 1, 225, 1, 64, 0.1, st) == _ffi.MI355_EUNSUPPORTED                 # N > 224
    assert lib.mi355_sdpa16_fwd(p, p, 1, 16, 1, 64, 0.1, 3, st) == -1 and b"precision" in lib.mi355_last_error()
    assert lib.mi355_cast16_fwd(p, p, 16, 3, st) == -1


# ---- the margin case ---------------------------------------------------------------------------------------------------------------
def _scaled(ctor, seed, scale):
    torch.manual_seed(seed)
    m = ctor().eval()
    if scale != 1.0:
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() >= 2:
                    p.mul_(scale)
    return m


def _cell(name, ctor, shape, ref_fn, wseed, xseed, scale):
    import mi355attn
    m = _scaled(ctor, wseed, scale)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(xseed)
    x = torch.randn(*shape)
    ref = ref_fn(x, sd)
    md, xd = m.cuda(), x.cuda()
    rec = dict(block=name, wseed=wseed, xseed=xseed, scale=scale)
    for mode in (1, 3, 0):
        mi355attn.set_default_precision(mode)
        try:
            with torch.no_grad():
                y = md(xd).cpu()
        finally:
            mi355attn.set_default_precision(1)
        rec["fro%d" % mode], rec["max%d" % mode] = rel_fro(y, ref), max_abs_ratio(y, ref)
        rec["finite%d" % mode] = bool(torch.isfinite(y).all())
    _rows.append(rec)
    print("[logit-mode] %-3s wseed %-6d xseed %-6d scale %.0fx  mode 1 %.2e / %.2e | mode 3 %.2e / %.2e | mode 0 %.2e / %.2e"
          % (name, wseed, xseed, scale, rec["fro1"], rec["max1"], rec["fro3"], rec["max3"], rec["fro0"], rec["max0"]))
    return rec


@pytest.mark.parametrize("scale", [1.0, 2.0, 3.0, 4.0])
@pytest.mark.parametrize("seeds", SEEDS, ids=["w%d" % s[0] for s in SEEDS])
def test_c3_mode3_inside_bar_at_every_scale(seeds, scale):
    """The promise of the mode: the attention block inside 1e-3 on both criteria at any logit scale (the emulation of
    tests/test_logit_mode_cpu.py predicts <= 5.1e-4)."""
    from mi355attn.modules import Attention
    rec = _cell("C3", lambda: Attention(768, 12), (B, 197, 768),
                lambda x, sd: O.vit_attention_forward(x, sd, 12, dtype=torch.float64), seeds[0], seeds[1], scale)
    assert rec["finite3"] and rec["fro3"] <= 1e-3 and rec["max3"] <= 1e-3, rec


@pytest.mark.parametrize("scale", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("seeds", SEEDS, ids=["w%d" % s[0] for s in SEEDS])
def test_c5_mode3(seeds, scale):
    """Full ViT-Base: gated at 1e-3 at weight scales 1 and 2 (mode 1 itself passes there); at 3x the value path and the MLP GEMMs, which
    the mode leaves in fp16, compound over 12 layers -- the emulation puts mode 3 on the bar (0.95-1.03e-3), so that cell is recorded and
    only bounded by 3e-3."""
    from mi355attn.modules import VisionTransformer
    rec = _cell("C5", lambda: VisionTransformer(num_heads=12), (B, 3, 224, 224),
                lambda x, sd: O.vit_forward(x, sd, 12, 12, dtype=torch.float64), seeds[0], seeds[1], scale)
    bar = 1e-3 if scale <= 2.0 else 3e-3
    assert rec["finite3"] and rec["fro3"] <= bar and rec["max3"] <= bar, rec


def test_zz_write_cells():
    """Runs last in this file: every cell measured above, modes 1 / 3 / 0 side by side (also when some of them failed)."""
    if not _rows:
        pytest.skip("no cell ran")
    path = os.environ.get("MI355_LOGIT_OUT", os.path.join(tempfile.gettempdir(), "mi355_logit_mode_margin.md"))
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("Cells of tests/test_logit_mode_gpu.py: B = %d, truth = fp64 oracle, rel-Frobenius / max-abs ratio.\n\n" % B)
            f.write("| block | weight seed | input seed | weight scale | precision 1 | precision 3 | precision 0 | 3 inside 1e-3 |\n|---|---|---|---|---|---|---|---|\n")
            for r in _rows:
                f.write("| %s | %d | %d | %.0fx | %.2e / %.2e | %.2e / %.2e | %.2e / %.2e | %s |\n" % (
                    r["block"], r["wseed"], r["xseed"], r["scale"], r["fro1"], r["max1"], r["fro3"], r["max3"], r["fro0"], r["max0"],
                    "yes" if r["fro3"] <= 1e-3 and r["max3"] <= 1e-3 else "NO"))
            for blk in ("C3", "C5"):
                for s in sorted({r["scale"] for r in _rows if r["block"] == blk}):
                    sel = [r for r in _rows if r["block"] == blk and r["scale"] == s]
                    f.write("\n%s scale %.0fx: worst precision 1 %.2e / %.2e, worst precision 3 %.2e / %.2e, worst precision 0 %.2e / %.2e\n" % (
                        blk, s, max(r["fro1"] for r in sel), max(r["max1"] for r in sel), max(r["fro3"] for r in sel),
                        max(r["max3"] for r in sel), max(r["fro0"] for r in sel), max(r["max0"] for r in sel)))
    except OSError as e:
        pytest.skip("table not written: %s" % e)


# ---- boundaries of the mode ---------------------------------------------------------------------------------------------------------
def _both_defaults(m, x, *fwd_args):
    import mi355attn
    out = []
    for mode in (1, 3):
        mi355attn.set_default_precision(mode)
        try:
            with torch.no_grad():
                out.append(m(x, *fwd_args).clone())
        finally:
            mi355attn.set_default_precision(1)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", ["MixerLayer", "XCABlock", "CSWinBlock_s3", "SELayer"])
def test_mode3_is_mode1_outside_vit_attention(case):
    from mi355attn.modules import CSWinBlock, MixerLayer, SELayer, XCABlock
    torch.manual_seed(1234)
    if case == "MixerLayer":
        m, shape, args = MixerLayer(512, 196), (8, 196, 512), ()
    elif case == "XCABlock":
        m, shape, args = XCABlock(384, 8, qkv_bias=True, eta=1.0), (8, 196, 384), (14, 14)
    elif case == "CSWinBlock_s3":
        m, shape, args = CSWinBlock(256, 14, 8, split_size=7, qkv_bias=True), (8, 196, 256), ()
    else:
        m, shape, args = SELayer(64), (4, 64, 32, 32), ()
    torch.manual_seed(4321)
    x = torch.randn(*shape).cuda()
    y1, y3 = _both_defaults(m.eval().cuda(), x, *args)
    assert torch.isfinite(y1).all() and torch.equal(y1, y3), case


@pytest.mark.parametrize("case", ["d192", "N577"])
def test_outside_the_envelope_mode3_is_mode0(case):
    from mi355attn.modules import Attention
    heads, N = (4, 197) if case == "d192" else (12, 577)
    torch.manual_seed(1234)
    m3 = Attention(768, heads, precision=3).eval()
    m0 = Attention(768, heads, precision=0).eval()
    m0.load_state_dict(m3.state_dict())
    torch.manual_seed(4321)
    x = torch.randn(2, N, 768).cuda()
    with torch.no_grad():
        y3, y0 = m3.cuda()(x), m0.cuda()(x)
    assert torch.isfinite(y0).all() and torch.equal(y3, y0)
    ref = O.vit_attention_forward(x.cpu(), {k: v.cpu() for k, v in m0.state_dict().items()}, heads, dtype=torch.float64)
    assert_parity(y3.cpu(), ref, 5e-5, case)


@pytest.mark.parametrize("where", ["input", "v_weight"])
def test_value_path_saturation_warns_once_and_returns_the_strict_result(where):
    """Finite inputs whose VALUE path leaves fp16 -- x itself, as the operand of the v tiles (range code 1), or v rows of the qkv weight
    large enough that v saturates in the projection's epilogue (code 3; the weights themselves stay inside fp16): one warning, the strict result."""
    import mi355attn
    from mi355attn.modules import Attention
    torch.manual_seed(1234)
    m = Attention(768, 12, precision=3).eval()
    xscale = 1.0
    if where == "input":
        xscale = 1e5
    else:
        with torch.no_grad():
            m.qkv.weight[2 * 768:].mul_(1e6)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(4321)
    x = torch.randn(4, 197, 768) * xscale
    ref = O.vit_attention_forward(x, sd, 12, dtype=torch.float64)
    assert torch.isfinite(ref).all()
    md, xd = m.cuda(), x.cuda()
    assert mi355attn.get_option("range_fallback") == 1
    mi355attn.range_status(wait=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            y = md(xd)
        torch.cuda.synchronize()
    hits = [i for i in w if "re-running this forward in strict mode" in str(i.message)]
    assert len(hits) == 1, [str(i.message) for i in w]
    assert_parity(y.cpu(), ref, 2e-4, where + " [strict re-run]")
    mi355attn.range_status(wait=True)
    m0 = Attention(768, 12, precision=0).eval()
    m0.load_state_dict(sd)
    with torch.no_grad():
        assert torch.equal(y, m0.cuda()(xd))


def test_default_untouched():
    """A fresh process starts at precision 1, and a precision-1 forward of C3 is the same bits before and after a mode-3 forward."""
    import mi355attn
    from mi355attn.modules import Attention
    code = "import sys; sys.path.insert(0, %r); import mi355attn; print(mi355attn.default_precision())" % PKG
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "1", (r.stdout, r.stderr)
    assert mi355attn.default_precision() == 1
    torch.manual_seed(1234)
    m = Attention(768, 12).eval().cuda()
    torch.manual_seed(4321)
    x = torch.randn(4, 197, 768).cuda()
    with torch.no_grad():
        before = m(x).clone()
        mi355attn.set_default_precision(3)
        y3 = m(x).clone()
        mi355attn.set_default_precision(1)
        after = m(x).clone()
    assert torch.equal(before, after)
    assert not torch.equal(before, y3)                                   # the mode-3 forward did run other kernels
    m1 = Attention(768, 12, precision=1).eval().cuda()
    m1.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert torch.equal(m1(x), before)
