"""GPU tests (-m gpu): the XCiT path at token counts above 256 -- patch 8 at 224 px (28 x 28 = 784 tokens), patch 16 at 384 px
(24 x 24 = 576) and a rectangular input (14 x 20 = 280) -- against the fp64 oracle, with the non-trivial parameters of
tests/route_cases.py / tests/model_cases.py (LayerNorm, BatchNorm, biases, LayerScales, temperatures, cls token).

Bars: those tests/test_routes_gpu.py holds the xcab_c128 row to and tests/test_models_gpu.py the xcit_p8 row: 1e-3 at the default
precision (fp16 operands), 5e-5 strict.  Each forward must run the tiled LPI kernel, and the range fallback must stay silent.
"""
import pytest
import torch
import torch.nn as nn

import oracle as O
from conftest import assert_parity
from test_routes_gpu import TOL, _run

pytestmark = pytest.mark.gpu

_XCIT = "vision_transformers.xcit"
_KW = dict(embed_dim=128, depth=2, num_heads=4, mlp_ratio=4, qkv_bias=True, norm_layer=nn.LayerNorm, cls_attn_layers=2, eta=1.0,
           num_classes=10)
_MODEL = lambda x, sd, dt: O.xcit_forward(x, sd, 4, 2, 2, dt)      # noqa: E731

ROWS = {
    "xcab_c128_24x24": dict(cls="XCABlock", args=(128, 4), kwargs=dict(qkv_bias=True, eta=1.0), shape=(1, 576, 128), fwd_args=(24, 24),
                            oracle=lambda x, sd, dt: O.xca_block_forward(x, sd, 4, 24, 24, dt), block=True),
    "xcit_p8_224": dict(cls="XCiT", kwargs=dict(_KW, img_size=224, patch_size=8), shape=(2, 3, 224, 224), oracle=_MODEL),
    "xcit_p16_384": dict(cls="XCiT", kwargs=dict(_KW, img_size=384, patch_size=16), shape=(1, 3, 384, 384), oracle=_MODEL),
    "xcit_p16_224x320": dict(cls="XCiT", kwargs=dict(_KW, img_size=224, patch_size=16), shape=(1, 3, 224, 320), oracle=_MODEL),
}
_BUILT = {}


def _built(rid):
    """(state dict, input, fp64 reference) of a row: built once, shared by both precisions."""
    if rid not in _BUILT:
        import importlib
        import model_cases
        import route_cases
        row = ROWS[rid]
        cls = getattr(importlib.import_module(_XCIT), row["cls"])
        m, x = (route_cases if row.get("block") else model_cases).build_row(row, cls)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        _BUILT[rid] = (sd, x, row["oracle"](x, sd, torch.float64).float())
    return _BUILT[rid]


@pytest.mark.parametrize("prec", [1, 0])
@pytest.mark.parametrize("rid", list(ROWS))
def test_large_grid_matches_fp64(rid, prec):
    import importlib
    row = ROWS[rid]
    sd, x, ref = _built(rid)
    m = getattr(importlib.import_module(_XCIT), row["cls"])(*row.get("args", ()), **row["kwargs"]).eval()
    m.load_state_dict(sd)
    for sub in m.modules():
        if hasattr(sub, "precision"):
            sub.precision = prec
    y, tags, fired = _run(m.cuda(), x.cuda(), row.get("fwd_args", ()))
    assert not fired, f"{rid} p{prec}: range fallback fired: {fired}"
    assert any("lpi_tile_kernel<ln>" in t for t in tags), tags
    if prec == 1:
        assert any("gemm16" in t for t in tags), f"{rid}: no 16-bit GEMM on the default route: {tags}"
    assert_parity(y.cpu(), ref, TOL[prec], f"{rid} p{prec}")
