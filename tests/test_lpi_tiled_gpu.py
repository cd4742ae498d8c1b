"""GPU tests (-m gpu): the LPI stencil block on token grids above 16 x 16 (lpi_tile_kernel, csrc/xcit.hip).

The tiled kernel serves one (image, tile, 32-channel group) per workgroup with a 2-cell halo of input; the grids below are the smallest
that exercise each seam of that scheme (first size past the old limit, the 384 px / patch 16 and 224 px / patch 8 grids, tall and wide
grids with ragged channel counts, single rows and columns, column tiles, bands with interior bands).  BatchNorm statistics, affine terms
and every bias are non-trivial, so a wrong halo of the intermediate shows: out-of-grid intermediate cells are conv2's zero padding,
in-grid ring cells are recomputed.

Bars: 5e-6 against the fp64 oracle for the plain block (tests/test_ops_gpu.py::test_lpi), 2e-5 with the LayerNorm in front
(tests/test_round3_kernels_gpu.py), bit identity wherever two routes evaluate the same expressions.
"""
import pytest
import torch

import oracle as O
from conftest import assert_parity

pytestmark = pytest.mark.gpu

GRIDS = [(2, 17, 17, 32),      # first size past the old limit
         (1, 24, 24, 64),      # 384 px / patch 16
         (1, 28, 28, 32),      # 224 px / patch 8
         (2, 33, 9, 36),       # tall, ragged C
         (1, 9, 40, 32),       # wide
         (1, 1, 300, 8),       # single row, wide
         (1, 300, 1, 8),       # single column, tall
         (1, 3, 100, 5),       # C < 4 lanes
         (1, 70, 70, 32)]      # several bands with interior bands
LN_GRIDS = [g for g in GRIDS if 300 not in g]
TILE = "lpi_tile_kernel"
_CASES = {}


def F():
    from mi355attn import functional
    return functional


def _params(C, seed):
    """O.lpi_forward's state-dict layout, as tests/test_ops_gpu.py::test_lpi builds it."""
    torch.manual_seed(seed)
    return {"conv1.weight": torch.randn(C, 1, 3, 3) / 3, "conv1.bias": torch.randn(C), "bn.weight": torch.rand(C) + 0.5,
            "bn.bias": torch.randn(C), "bn.running_mean": torch.randn(C) * 0.1, "bn.running_var": torch.rand(C) + 0.5,
            "conv2.weight": torch.randn(C, 1, 3, 3) / 3, "conv2.bias": torch.randn(C)}


def _case(B, H, W, C):
    """Inputs, parameters and the fp64 references of a grid: computed once, shared by the tests, never modified."""
    key = (B, H, W, C)
    if key not in _CASES:
        p = _params(C, H * W + C)
        x = torch.randn(B, H * W, C)
        gamma, resid = torch.rand(C) + 0.5, torch.randn(B, H * W, C)
        ln = torch.nn.LayerNorm(C)
        with torch.no_grad():
            ln.weight.uniform_(0.5, 1.5)
            ln.bias.normal_(0, 0.2)
        xl = x * 2 + 0.5
        u = torch.nn.functional.layer_norm(xl.double(), (C,), ln.weight.double(), ln.bias.double(), ln.eps)
        _CASES[key] = dict(p=p, x=x, gamma=gamma, resid=resid, ln=ln, xl=xl, ref=O.lpi_forward(x, p, H, W, torch.float64),
                           ref_ln=xl.double() + gamma.double() * O.lpi_forward(u, p, H, W, torch.float64))
    return _CASES[key]


def _lpi(x, d, H, W, **kw):
    return F().lpi(x, d["conv1.weight"], d["conv1.bias"], d["bn.weight"], d["bn.bias"], d["bn.running_mean"], d["bn.running_var"], 1e-5,
                   d["conv2.weight"], d["conv2.bias"], H, W, **kw)


def _traced(fn):
    """(result, kernel tags) of fn()."""
    import mi355attn
    out = []
    rows = mi355attn.kernel_trace(lambda: out.append(fn()))
    return out[0], [t for t, *_ in rows]


def _dev(p):
    return {k: v.cuda() for k, v in p.items()}


@pytest.mark.parametrize("B,H,W,C", GRIDS)
def test_tiled_lpi_matches_the_oracle(B, H, W, C):
    """Plain and with gamma + resid against the fp64 oracle at 5e-6; each run goes through the tiled kernel.  (2, 17, 17, 32) is the
    first grid the untiled kernel refused (Mi355Error: the token grid exceeds the LDS tile)."""
    c = _case(B, H, W, C)
    d, xd = _dev(c["p"]), c["x"].cuda()
    got, tags = _traced(lambda: _lpi(xd, d, H, W))
    assert any(TILE in t for t in tags), tags
    assert not any("<ln>" in t for t in tags), tags
    assert_parity(got.cpu(), c["ref"].float(), 5e-6, "lpi")
    got, tags = _traced(lambda: _lpi(xd, d, H, W, gamma=c["gamma"].cuda(), resid=c["resid"].cuda()))
    assert any(TILE in t for t in tags), tags
    assert_parity(got.cpu(), (c["resid"].double() + c["gamma"].double() * c["ref"]).float(), 5e-6, "lpi gamma+resid")


@pytest.mark.parametrize("B,H,W,C", [(1, 28, 28, 32), (1, 70, 70, 32), (1, 9, 40, 32), (1, 3, 100, 5), (2, 33, 9, 36)])
def test_bias_only_probe_is_a_function_of_position(B, H, W, C):
    """x = 0 with non-zero conv1 bias and BatchNorm shift: the intermediate is the constant bn(gelu(b1)) on the whole grid and zero
    outside it.  A kernel that fills out-of-grid intermediate cells with bn(gelu(b1)) is wrong on the grid's border; one that zeroes
    in-grid ring cells is wrong at the tile seams.  Every token at least one cell away from the border sees nine equal taps of the
    same constant: identical bits, whichever tile computed it."""
    c = _case(B, H, W, C)
    x0 = torch.zeros(B, H * W, C)
    ref = O.lpi_forward(x0, c["p"], H, W, torch.float64)
    got, tags = _traced(lambda: _lpi(x0.cuda(), _dev(c["p"]), H, W))
    assert any(TILE in t for t in tags), tags
    got = got.cpu()
    assert_parity(got, ref.float(), 5e-6, "bias-only probe")
    g = got.reshape(B, H, W, C)
    if H > 2 and W > 2:
        inner = g[:, 1:-1, 1:-1]
        assert torch.equal(inner, inner[:, :1, :1].expand_as(inner)), "interior tokens differ: a tile seam shows"


@pytest.mark.parametrize("B,H,W,C", LN_GRIDS)
def test_fused_layernorm_is_bit_identical_to_layernorm_then_lpi(B, H, W, C):
    """ln= (mi355_ln_lpi_fwd) against F.layernorm followed by F.lpi: the same bits; against the oracle at 2e-5; and the stats= form
    (mi355_ln_lpi_stats_fwd) fed the (mean, rstd) rows of mi355_ln_lpi_fwd's own statistics pass: the same bits again."""
    from mi355attn import _ffi
    c = _case(B, H, W, C)
    d, ln = _dev(c["p"]), c["ln"].cuda()
    xd, gd = c["xl"].cuda(), c["gamma"].cuda()
    with torch.no_grad():
        fused, tags = _traced(lambda: _lpi(xd, d, H, W, gamma=gd, resid=xd, ln=ln))
        assert any(TILE + "<ln>" in t for t in tags), tags
        n = _ffi.lib().mi355_lpi_workspace_bytes(B, H, W, C)
        stats = _ffi.workspace(n, xd.device)[:B * H * W * 8].clone().view(torch.float32).reshape(B * H * W, 2)
        unfused = _lpi(F().layernorm(xd, ln.weight, ln.bias, ln.eps), d, H, W, gamma=gd, resid=xd)
        given, tags = _traced(lambda: _lpi(xd, d, H, W, gamma=gd, resid=xd, ln=ln, stats=stats))
        assert any(TILE + "<ln>" in t for t in tags) and not any("ln_stats" in t for t in tags), tags
    assert torch.equal(fused, unfused), "fused LayerNorm differs from layernorm -> lpi"
    assert torch.equal(fused, given), "stats= differs from ln="
    assert_parity(fused.cpu(), c["ref_ln"].float(), 2e-5, "ln + lpi vs oracle")


@pytest.mark.parametrize("B,H,W,C,tag", [(2, 14, 14, 64, "lpi_patch_kernel"), (2, 16, 16, 32, "lpi_kernel"), (2, 7, 9, 36, "lpi_kernel")])
def test_small_grids_keep_their_kernels(B, H, W, C, tag):
    c = _case(B, H, W, C)
    got, tags = _traced(lambda: _lpi(c["x"].cuda(), _dev(c["p"]), H, W))
    assert any(t.startswith(tag) for t in tags), tags
    assert not any(TILE in t for t in tags), tags
    assert_parity(got.cpu(), c["ref"].float(), 5e-6, "lpi")


def test_deterministic_and_independent_of_the_batch():
    """Two runs give the same bits; image 0 of a B = 5 call equals the B = 1 call on that image (the tile shape depends on (H, W) only)."""
    H, W, C = 28, 28, 32
    c = _case(1, H, W, C)
    torch.manual_seed(5)
    x = torch.randn(5, H * W, C).cuda()
    d, ln, gd = _dev(c["p"]), c["ln"].cuda(), c["gamma"].cuda()
    with torch.no_grad():
        for kw in (dict(), dict(gamma=gd, ln=ln)):
            res = dict(resid=x) if kw else {}
            y, tags = _traced(lambda: _lpi(x, d, H, W, **kw, **res))
            assert any(TILE in t for t in tags), tags
            assert torch.equal(y, _lpi(x, d, H, W, **kw, **res))
            x0 = x[:1].contiguous()
            assert torch.equal(y[:1], _lpi(x0, d, H, W, **kw, **(dict(resid=x0) if kw else {}))), "image 0 depends on its batch"


def test_memory_contract_by_hand():
    """mi355_ln_lpi_fwd at (2, 17, 19, 36) with y and the workspace carved out of a 0xFF-filled buffer, the workspace exactly
    mi355_lpi_workspace_bytes long: 256 bytes on either side of each stay 0xFF, and y holds no NaN (0xFF.. is a NaN pattern: every
    element was written)."""
    from mi355attn import _ffi
    B, H, W, C = 2, 17, 19, 36
    c = _case(B, H, W, C)
    d, ln = _dev(c["p"]), c["ln"].cuda()
    xd, gd = c["xl"].cuda(), c["gamma"].cuda()
    lib = _ffi.lib()
    ny = B * H * W * C * 4
    nws = lib.mi355_lpi_workspace_bytes(B, H, W, C)
    assert nws == B * H * W * 8 + 16
    pad = 256
    y0 = pad
    w0 = (y0 + ny + pad + 255) // 256 * 256
    total = w0 + nws + pad
    buf = torch.full((total,), 0xFF, dtype=torch.uint8, device="cuda")
    y = buf[y0:y0 + ny].view(torch.float32)
    ws = buf[w0:w0 + nws]
    ptr = _ffi.dptr
    order = ("conv1.weight", "conv1.bias", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")
    rc = lib.mi355_ln_lpi_fwd(ptr(xd), ptr(ln.weight.detach()), ptr(ln.bias.detach()), float(ln.eps), *[ptr(d[k]) for k in order], 1e-5,
                              ptr(d["conv2.weight"]), ptr(d["conv2.bias"]), ptr(gd), ptr(xd), ptr(y), B, H, W, C, ptr(ws), nws,
                              _ffi.stream_ptr(xd.device))
    _ffi.check(rc, "mi355_ln_lpi_fwd")
    torch.cuda.synchronize()
    host = buf.cpu()
    for name, lo, n in (("y", y0, ny), ("workspace", w0, nws)):
        assert bool((host[lo - pad:lo] == 0xFF).all()), f"bytes in front of {name} were written"
        assert bool((host[lo + n:lo + n + pad] == 0xFF).all()), f"bytes behind {name} were written"
    got = host[y0:y0 + ny].view(torch.float32).reshape(B, H * W, C)
    assert not torch.isnan(got).any(), "y holds elements the kernel did not write"
    assert_parity(got, c["ref_ln"].float(), 2e-5, "ln + lpi by hand vs oracle")
