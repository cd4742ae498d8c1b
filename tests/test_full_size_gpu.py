"""Parity at the sizes bench.py TIMES (BASELINE.json configs[2..4], B = 256 per GPU): SURVEY.md 8(d) "big-shape checks compare
on-device against the oracle for a sampled subset of images (0, 127, 255)".

For every timed transformer configuration -- C3 ViT `Attention(768, 12)` on (256,197,768); C4 the four `CSWinBlock`s and
`XCABlock(384, 8)` / `XCA` at B = 256; C5 `VisionTransformer(num_heads=12)` on 256 images -- the input is built on the device in
slabs from the seed-4321 CPU stream (so that the sampled images exist on the host without holding the whole batch there) and the
test asserts:

  * images 0 / 127 / 255 of the B = 256 run match the oracle within 1e-3 (default fp16-operand mode) -- the M = 50 432-row GEMMs,
    the 3 072 ... 114 688-workgroup attention grids and the XCD-remapped block order are the ones bench.py reports;
  * the same three images in strict mode (split-bf16 operands) within 5e-5;
  * run-to-run bit identity of the full-size launch;
  * batch independence: a 3-image batch of the sampled images gives the same rows as the 256-image run bit-for-bit (every GEMM
    variant keeps a row's K order); the one exception is the split last round of the persistent GEMM ("gemm_splitk"), with which
    the rows agree to the operand format's rounding level and bit-for-bit again once it is switched off (DoubleAttention: the
    pixel ranges of pass 1 follow the batch size unless "da_ranges" pins them).
"""
import pytest
import torch

import oracle as O
from conftest import assert_parity

pytestmark = pytest.mark.gpu

PICK = [0, 127, 255]
B = 256


def _seeded(ctor):
    torch.manual_seed(1234)
    return ctor().eval()


def _device_batch(shape, slab=32):
    """randn(seed 4321) of `shape` (B first) on the device, filled slab by slab; returns (x_device, {b: host image})."""
    g = torch.Generator(device="cpu").manual_seed(4321)
    x = torch.empty(*shape, device="cuda")
    host = {}
    for b0 in range(0, shape[0], slab):
        n = min(slab, shape[0] - b0)
        blk = torch.randn(n, *shape[1:], generator=g)
        x[b0:b0 + n] = blk.cuda()
        for b in PICK:
            if b0 <= b < b0 + n:
                host[b] = blk[b - b0].clone()
    return x, host


def _check(name, module, shape, ref_fn, fwd_args=(), tol=1e-3, strict_tol=5e-5, pin=(("gemm_splitk", 0),), path_tol=5e-4):
    """`pin`: the options that make the kernel path independent of the batch size; `path_tol`: how far the default paths of the
    full batch and of the 3-image batch may be apart."""
    import mi355attn
    m = module.cuda()
    x, host = _device_batch(shape)
    xs = torch.stack([host[b] for b in PICK])
    with torch.no_grad():
        y = m(x, *fwd_args)
        y2 = m(x, *fwd_args)
        sub = m(x[PICK].contiguous(), *fwd_args)
    torch.cuda.synchronize()
    assert tuple(y.shape)[0] == B
    assert torch.isfinite(y).all(), name + ": non-finite output at full size"
    assert torch.equal(y, y2), name + ": run-to-run results differ at full size"
    ref = ref_fn(xs)
    assert_parity(y[PICK].cpu(), ref, tol, name + " [B=256, images 0/127/255]")
    if not torch.equal(y[PICK], sub):
        # The only launch-dependent arithmetic is the persistent GEMM's split last round (option "gemm_splitk", K >= 1536): the fp32
        # summation order of those tiles changes, and a 1e-7 difference in front of a 16-bit re-rounding of the next operand shows up
        # at the operand format's rounding level downstream -- inside the parity tolerance by a factor of two at least.  With the
        # split off every row must be bit-identical whatever the batch around it.
        assert_parity(sub.cpu(), y[PICK].cpu(), path_tol, name + " [batch independence, default options]")
        # DoubleAttention's analogue: the number of pixel ranges an image is cut into follows the batch size ("da_ranges" pins it).
        # ViT encoder chain (round 4): the LayerNorm fold needs rows % 128 == 0, so B = 256 folds and B = 3 does not ("ln_fold" pins it).
        with mi355attn.options(**dict(pin)):
            with torch.no_grad():
                y0 = m(x, *fwd_args)
                sub0 = m(x[PICK].contiguous(), *fwd_args)
            torch.cuda.synchronize()
        assert torch.equal(y0[PICK], sub0), name + f": output of an image depends on its batch neighbours ({pin})"
        assert_parity(y0[PICK].cpu(), ref, tol, name + f" [B=256, {pin}]")
        del y0, sub0
    assert_parity(sub.cpu(), ref, tol, name + " [3-image batch]")
    del y2, sub
    # strict (fp32-class) mode on the same full-size input
    old = mi355attn.default_precision()
    mi355attn.set_default_precision(0)
    try:
        with torch.no_grad():
            ys = m(x, *fwd_args)
        torch.cuda.synchronize()
    finally:
        mi355attn.set_default_precision(old)
    assert_parity(ys[PICK].cpu(), ref, strict_tol, name + " [B=256 strict]")
    # the fast result must sit inside the tolerance of the strict one everywhere, not only on the sampled images
    d = (y - ys).float()
    rel = float(d.norm() / ys.float().norm())
    assert rel <= tol, f"{name}: fast vs strict over the whole batch rel_fro={rel:.3e}"


def _sd(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


def test_c3_vit_attention_full_size():
    from mi355attn.modules import Attention
    m = _seeded(lambda: Attention(768, 12))
    sd = _sd(m)
    _check("ViT Attention(768,12)", m, (B, 197, 768), lambda xs: O.vit_attention_forward(xs, sd, 12))


CSWIN = [
    ("s1", (64, 56, 2), dict(split_size=1, qkv_bias=True), (3136, 64), (56, 2, 1, False)),
    ("s2", (128, 28, 4), dict(split_size=2, qkv_bias=True), (784, 128), (28, 4, 2, False)),
    ("s3", (256, 14, 8), dict(split_size=7, qkv_bias=True), (196, 256), (14, 8, 7, False)),
    ("s4", (512, 7, 16), dict(split_size=7, qkv_bias=True, last_stage=True), (49, 512), (7, 16, 7, True)),
]


@pytest.mark.parametrize("cfg", CSWIN, ids=[c[0] for c in CSWIN])
def test_c4_cswin_block_full_size(cfg):
    from mi355attn.modules import CSWinBlock
    name, args, kw, shp, oargs = cfg
    m = _seeded(lambda: CSWinBlock(*args, **kw))
    sd = _sd(m)
    _check("CSWinBlock " + name, m, (B,) + shp, lambda xs: O.cswin_block_forward(xs, sd, *oargs))


def test_c4_xca_block_full_size():
    from mi355attn.modules import XCABlock
    m = _seeded(lambda: XCABlock(384, 8, qkv_bias=True, eta=1.0))
    sd = _sd(m)
    _check("XCABlock(384,8)", m, (B, 196, 384), lambda xs: O.xca_block_forward(xs, sd, 8, 14, 14), fwd_args=(14, 14))


def test_c4_xca_full_size():
    from mi355attn.modules import XCA
    m = _seeded(lambda: XCA(384, 8, qkv_bias=True))
    sd = _sd(m)
    _check("XCA(384,8)", m, (B, 196, 384), lambda xs: O.xca_forward(xs, sd, 8))


def test_c5_vit_base_full_size():
    from mi355attn.modules import VisionTransformer
    m = _seeded(lambda: VisionTransformer(num_heads=12))
    sd = _sd(m)
    _check("VisionTransformer(ViT-Base/16)", m, (B, 3, 224, 224), lambda xs: O.vit_forward(xs, sd, 12, 12))


def test_c5_vit_base_full_size_with_the_layernorm_fold():
    """The same forward with the opt-in LayerNorm fold ("ln_fold" = 1): B = 256 folds (rows % 128 == 0), the 3-image batch cannot, so
    batch independence is checked with the fold pinned off."""
    import mi355attn
    from mi355attn.modules import VisionTransformer
    m = _seeded(lambda: VisionTransformer(num_heads=12))
    sd = _sd(m)
    with mi355attn.options(ln_fold=1):
        _check("VisionTransformer(ViT-Base/16) + ln_fold", m, (B, 3, 224, 224), lambda xs: O.vit_forward(xs, sd, 12, 12),
               pin=(("gemm_splitk", 0), ("ln_fold", 0)), path_tol=1e-3)


def test_mixer_layer_full_size():
    from mi355attn.modules import MixerLayer
    m = _seeded(lambda: MixerLayer(512, 196))
    sd = _sd(m)
    _check("MixerLayer(512,196)", m, (B, 196, 512), lambda xs: O.mixer_layer_forward(xs, sd))


def test_double_attention_full_size():
    from mi355attn.modules import DoubleAttention
    m = _seeded(lambda: DoubleAttention(256, 128, 128))
    sd = _sd(m)
    keys = ("convA.weight", "convA.bias", "convB.weight", "convB.bias", "convV.weight", "convV.bias", "proj.weight", "proj.bias")
    _check("DoubleAttention(256,128,128)@56x56", m, (B, 256, 56, 56),
           lambda xs: O.double_attention_forward(xs, *[sd[k] for k in keys]), pin=(("da_ranges", 1),))
