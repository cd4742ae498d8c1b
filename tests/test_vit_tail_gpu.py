"""The pooled-token tail of a ViT (csrc/vit_tail.hip, option "vit_tail"): with global_pool = "token" nothing but row 0 of the last
encoder block's output is read, so that block computes LayerNorm 1 and k / v for every token and everything else for one row per image.

Every kernel involved is row-independent and keeps the GEMM engine's K order, so the requirement is BIT IDENTITY with the full block
(option 0 vs 1, `gemm_splitk` pinned to 0: the split last round of the persistent GEMM is the one launch-dependent summation order of
the engine).  With default options the two paths may differ by that effect only: 5e-4, the figure tests/test_full_size_gpu.py uses
for it.
"""
import pytest
import torch

import oracle as O
from conftest import assert_parity, rel_fro

pytestmark = pytest.mark.gpu

LIMITED = "win_attn_kernel<d=64,io16,rows>"
FULL = "win_attn_kernel<d=64,io16>"


def _model(seed=1234, nontrivial=True, **kw):
    from mi355attn.modules import VisionTransformer
    from model_cases import prep_model
    from route_cases import prep_nontrivial
    torch.manual_seed(seed)
    m = VisionTransformer(**kw).eval()
    if nontrivial:
        prep_nontrivial(m)
        prep_model(m)
    return m.cuda()


def _input(shape, seed=4321):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.empty(*shape, device="cuda")
    for b0 in range(0, shape[0], 32):
        n = min(32, shape[0] - b0)
        x[b0:b0 + n] = torch.randn(n, *shape[1:], generator=g).cuda()
    return x


def _fwd(m, x, **opts):
    import mi355attn
    with mi355attn.options(**opts), torch.no_grad():
        y = m(x)
    torch.cuda.synchronize()
    return y


def _tags(m, x, **opts):
    import mi355attn
    with mi355attn.options(**opts), torch.no_grad():
        rows = mi355attn.kernel_trace(lambda: m(x))
    return {t.split(" ")[0]: c for t, c, *_ in rows}


def _assert_paths_equal(m, x, name):
    y0 = _fwd(m, x, vit_tail=0, gemm_splitk=0)
    y1 = _fwd(m, x, vit_tail=1, gemm_splitk=0)
    d0 = _fwd(m, x, vit_tail=0)
    d1 = _fwd(m, x, vit_tail=1)
    print(f"[vit_tail] {name}: full vs pruned max|diff| split off {float((y0 - y1).abs().max()):.3e}, "
          f"default options {float((d0 - d1).abs().max()):.3e} rel_fro {rel_fro(d1.cpu(), d0.cpu()):.3e}")
    assert torch.isfinite(y1).all()
    assert torch.equal(y0, y1), f"{name}: pruned last block differs from the full block (gemm_splitk = 0)"
    assert_parity(d1.cpu(), d0.cpu(), 5e-4, f"{name}: pruned vs full, default options")
    return y1


@pytest.mark.parametrize("prec", [1, 2])
def test_vit_base_b256_bit_identical_to_full_block(prec):
    """The benchmark's configuration: ViT-Base/16, num_heads = 12, B = 256, weights seed 1234, input seed 4321."""
    m = _model(nontrivial=False, num_heads=12, precision=prec)
    x = _input((256, 3, 224, 224))
    tags = _tags(m, x[:2].contiguous(), vit_tail=1)
    assert tags.get(LIMITED) == 1 and tags.get(FULL) == 11, tags
    y = _assert_paths_equal(m, x, f"ViT-Base/16 B=256 precision {prec}")
    # run-to-run bit identity and batch independence of the pruned forward (split off: every row's bits are its own)
    assert torch.equal(y, _fwd(m, x, vit_tail=1, gemm_splitk=0))
    for i in (0, 127, 255):
        yi = _fwd(m, x[i:i + 1].contiguous(), vit_tail=1, gemm_splitk=0)
        assert torch.equal(yi[0], y[i]), f"image {i} alone differs from image {i} inside the batch of 256"
    if prec == 1:           # the project's 1e-3 is the bound of the default fp16 operand mode (bf16 operands carry 8 mantissa bits)
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        pick = [0, 127, 255]
        assert_parity(y[pick].cpu(), O.vit_forward(x[pick].cpu(), sd, 12, 12), 1e-3, "pruned ViT-Base/16 vs fp64 oracle")


SMALL = [
    ("depth1", dict(depths=1, num_heads=12, qkv_bias=True, num_classes=10), (4, 3, 224, 224)),
    ("depth2", dict(depths=2, num_heads=12, qkv_bias=True, num_classes=10), (4, 3, 224, 224)),
    ("depth2_nobias", dict(depths=2, num_heads=12, qkv_bias=False, num_classes=10), (2, 3, 224, 224)),
    ("b1", dict(depths=2, num_heads=12, qkv_bias=True, num_classes=10), (1, 3, 224, 224)),
    ("b19", dict(depths=2, num_heads=12, qkv_bias=True, num_classes=10), (19, 3, 224, 224)),
    ("d32_c256", dict(depths=2, num_heads=8, embedding_dim=256, qkv_bias=True, num_classes=10), (5, 3, 224, 224)),
    ("d32_c128_17tok", dict(depths=1, num_heads=4, embedding_dim=128, image_size=64, qkv_bias=True, num_classes=10), (3, 3, 64, 64)),
    ("d64_5tok", dict(depths=2, num_heads=2, embedding_dim=128, image_size=32, qkv_bias=True, num_classes=10), (7, 3, 32, 32)),
]


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_small_models_bit_identical_to_full_block(case, prec):
    name, kw, shape = case
    m = _model(precision=prec, **kw)
    x = _input(shape)
    tags = _tags(m, x, vit_tail=1)
    assert sum(c for t, c in tags.items() if ",rows>" in t and t.startswith("win_attn_kernel")) == 1, tags
    y = _assert_paths_equal(m, x, f"{name} precision {prec}")
    if prec == 1:           # fp16 operand mode: the project's 1e-3 against the fp64 oracle
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        heads, depth = kw["num_heads"], kw["depths"]
        assert_parity(y.cpu(), O.vit_forward(x.cpu(), sd, heads, depth), 1e-3, f"{name}: pruned forward vs fp64 oracle")


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("N", [5, 16, 17, 197, 224])
def test_limited_core_row0_is_the_full_core_row0(N, d, prec):
    """mi355_sdpa16_rows_fwd with q_rows = 1: row 0 carries mi355_sdpa16_fwd's bits, in the full layout nothing else is written, and
    the dense (B, 1, C) layout holds the same row."""
    from mi355attn import functional as F
    heads, B = 3, 5
    C = heads * d
    g = torch.Generator().manual_seed(N * 131 + d)
    qkv = torch.randn(B, N, 3 * C, generator=g).cuda().to(F.dtype16(prec))
    full = F.sdpa16(qkv, heads, d ** -0.5, precision=prec)
    fill = torch.full((B, N, C), 7.0, device="cuda").to(qkv.dtype)
    out = F.sdpa16_rows(qkv, heads, d ** -0.5, 1, out=fill.clone(), precision=prec)
    dense = F.sdpa16_rows(qkv, heads, d ** -0.5, 1, precision=prec)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 0], full[:, 0])
    assert torch.equal(out[:, 1:], fill[:, 1:]), "the limited core wrote rows it does not own"
    assert tuple(dense.shape) == (B, 1, C) and torch.equal(dense[:, 0], full[:, 0])
    if N >= 17:                                    # more than one row, more than one tile's worth of buffer
        q3 = F.sdpa16_rows(qkv, heads, d ** -0.5, 3, out=fill.clone(), precision=prec)
        torch.cuda.synchronize()
        assert torch.equal(q3[:, :3], full[:, :3]) and torch.equal(q3[:, 3:], fill[:, 3:])


def test_entry_refuses_outside_the_envelope():
    from mi355attn import _ffi
    lib = _ffi.lib()
    p = _ffi.dptr(torch.zeros(1 << 16, device="cuda"))
    st = _ffi.stream_ptr(torch.device("cuda", torch.cuda.current_device()))

    def call(B, N, C, hidden, heads, prec):
        return lib.mi355_vit_tail_fwd(p, p, p, 1e-5, p, p, p, p, p, p, 1e-5, p, p, p, p, p, B, N, C, hidden, heads, 0.1, prec, p, 1 << 18, st)

    for args in ((1, 5, 192, 768, 2, 1), (1, 225, 128, 512, 2, 1), (1, 5, 96, 384, 3, 1), (1, 5, 128, 512, 2, 0), (1, 5, 128, 512, 2, 3)):
        assert call(*args) == _ffi.MI355_EUNSUPPORTED, args
        assert b"mi355_vit_tail_fwd" in lib.mi355_last_error()
    assert lib.mi355_sdpa16_rows_fwd(p, p, 1, 16, 1, 64, 0.1, 1, 1, 3, st) == -1
    assert lib.mi355_sdpa16_rows_fwd(p, p, 1, 16, 1, 96, 0.1, 1, 1, 1, st) == _ffi.MI355_EUNSUPPORTED
    assert lib.mi355_sdpa16_rows_fwd(p, p, 1, 225, 1, 64, 0.1, 1, 1, 1, st) == _ffi.MI355_EUNSUPPORTED
    torch.cuda.synchronize()


def _limited(tags):
    return sum(c for t, c in tags.items() if t.startswith("win_attn_kernel") and ",rows>" in t)


def test_routing_by_option_and_configuration():
    kw = dict(depths=2, num_heads=12, qkv_bias=True, num_classes=10)
    m = _model(**kw)
    x = _input((2, 3, 224, 224))
    on, off = _tags(m, x, vit_tail=1), _tags(m, x, vit_tail=0)
    assert on.get(FULL) == 1 and on.get(LIMITED) == 1, on
    assert off.get(FULL) == 2 and _limited(off) == 0, off
    assert _limited(_tags(m, x, vit_tail=1, ln_fold=1)) == 0
    for name, kw2, shape, prec in (("avg", dict(kw, global_pool="avg"), (2, 3, 224, 224), None),
                                   ("none", dict(kw, global_pool="none"), (2, 3, 224, 224), None),
                                   ("225 tokens", dict(kw, depths=1), (2, 3, 224, 256), None),
                                   ("heads8", dict(kw, num_heads=8), (2, 3, 224, 224), None),
                                   ("strict", dict(kw, precision=0), (2, 3, 224, 224), 0),
                                   ("logit", dict(kw, precision=3), (2, 3, 224, 224), 3)):
        tags = _tags(_model(**kw2), _input(shape), vit_tail=1)
        assert _limited(tags) == 0, (name, tags)


@pytest.mark.parametrize("where", ["block", "mlp", "pre_qkv"])
def test_hooks_keep_the_full_block(where):
    m = _model(depths=2, num_heads=12, qkv_bias=True, num_classes=10)
    x = _input((3, 3, 224, 224))
    ref = _fwd(m, x, vit_tail=1, gemm_splitk=0)
    seen = []
    last = m.blocks[-1]
    if where == "block":
        h = last.register_forward_hook(lambda mod, inp, out: seen.append(tuple(out.shape)))
    elif where == "mlp":
        h = last.mlp.register_forward_hook(lambda mod, inp, out: seen.append(tuple(out.shape)))
    else:
        h = last.attn.qkv.register_forward_pre_hook(lambda mod, inp: None)
    try:
        tags = _tags(m, x, vit_tail=1, gemm_splitk=0)
        assert _limited(tags) == 0 and tags.get(FULL) == 2, tags
        seen.clear()
        y = _fwd(m, x, vit_tail=1, gemm_splitk=0)
    finally:
        h.remove()
    if where != "pre_qkv":
        assert seen == [(3, 197, 768)], seen
    assert torch.equal(y, ref)
    assert _limited(_tags(m, x, vit_tail=1)) == 1                      # hook gone: pruned again


def test_in_place_weight_rescale_is_seen():
    from model_cases import rescale_cached
    m = _model(depths=2, num_heads=12, qkv_bias=True, num_classes=10)
    x = _input((3, 3, 224, 224))
    names = ("blocks.1.attn.qkv.weight", "blocks.1.attn.proj.weight", "blocks.1.mlp.fc1.weight", "blocks.1.mlp.fc2.weight",
             "blocks.1.layernorm2.weight", "blocks.1.attn.qkv.bias", "head.weight")
    before = _fwd(m, x, vit_tail=1, gemm_splitk=0)
    rescale_cached(m, names)
    after = _fwd(m, x, vit_tail=1, gemm_splitk=0)
    full = _fwd(m, x, vit_tail=0, gemm_splitk=0)
    assert not torch.equal(before, after)
    assert torch.equal(after, full)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert_parity(after.cpu(), O.vit_forward(x.cpu(), sd, 12, 2), 1e-3, "pruned forward after an in-place rescale vs fp64 oracle")


@pytest.mark.parametrize("prec", [1, 2])
def test_graph_capture_replays_equal_eager(prec):
    m = _model(depths=2, num_heads=12, qkv_bias=True, num_classes=10, precision=prec)
    import mi355attn
    x = _input((4, 3, 224, 224))
    eager = _fwd(m, x, vit_tail=1)
    assert _limited(_tags(m, x, vit_tail=1)) == 1
    xs = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with mi355attn.options(vit_tail=1), torch.no_grad(), torch.cuda.stream(s):
        m(xs)                                           # warm-up on the capture stream: caches and workspaces exist
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = m(xs)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_fp16_range_report_reaches_the_tail():
    """A LayerNorm 2 gain that saturates fp16 inside the pruned block is reported like in the full block (code 2): with the range
    fall-back the forward re-runs strict and stays finite."""
    import warnings
    import mi355attn
    m = _model(depths=1, num_heads=12, qkv_bias=True, num_classes=10, precision=1)
    x = _input((2, 3, 224, 224))
    with torch.no_grad():
        m.blocks[0].layernorm2.weight.mul_(1e6)
    with mi355attn.options(vit_tail=1), torch.no_grad(), warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        y = m(x)
    torch.cuda.synchronize()
    assert any("overflowed" in str(i.message) for i in w), [str(i.message) for i in w]
    assert torch.isfinite(y).all()
