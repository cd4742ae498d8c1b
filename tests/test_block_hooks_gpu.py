"""Forward hooks on the sub-modules of the transformer blocks fire on fp32 input.

TransformerEncoder calls `attn` and `mlp`, and CSWinBlock calls `mlp` on every route but its fused ones, through nn.Module.__call__, so a
forward hook registered on them sees one call per forward (VisionTransformer._tail_ok is built on hooks being observable).  The same
fp32 bodies also serve a widened 16-bit x, where they call the sub-modules' `_run` instead; this file pins the fp32 side.  A hook that
returns nothing leaves the output bit-identical.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _encoder(precision):
    from mi355attn.modules import TransformerEncoder
    return TransformerEncoder(64, num_heads=2, precision=precision)


def _cswin_mlp2():
    from mi355attn.modules import CSWinBlock                   # route_cases cswin_c64_mlp2: stripe kernel + proj GEMM + layernorm16 + plain MLP
    return CSWinBlock(64, 8, 2, split_size=2, mlp_ratio=2., qkv_bias=True)


def _cswin_strict():
    from mi355attn.modules import CSWinBlock
    return CSWinBlock(64, 6, 2, split_size=2, qkv_bias=True, precision=0)


# id -> (constructor, input shape, sub-module -> calls per forward)
CASES = {
    "encoder_default": (lambda: _encoder(None), (2, 17, 64), {"attn": 1, "mlp": 1}),
    "encoder_strict": (lambda: _encoder(0), (2, 17, 64), {"attn": 1, "mlp": 1}),
    "cswin_c64_mlp2": (_cswin_mlp2, (3, 64, 64), {"mlp": 1}),
    "cswin_strict": (_cswin_strict, (3, 36, 64), {"mlp": 1}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_forward_hooks_fire_once_and_keep_the_bits(name):
    build, shape, want = CASES[name]
    torch.manual_seed(1234)
    m = build().eval().cuda()
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(4321)).cuda()
    with torch.no_grad():
        plain = m(x)
    fired = dict.fromkeys(want, 0)

    def counter(key):
        def hook(module, args, output):
            fired[key] += 1
        return hook

    handles = [getattr(m, key).register_forward_hook(counter(key)) for key in want]
    try:
        with torch.no_grad():
            hooked = m(x)
    finally:
        for h in handles:
            h.remove()
    torch.cuda.synchronize()
    assert fired == want, f"{name}: hook calls {fired}, expected {want}"
    assert torch.equal(hooked, plain), f"{name}: the hooked forward differs from the plain one"
