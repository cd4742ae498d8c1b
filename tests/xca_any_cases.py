"""Shapes of the tests of the run-time-width XCiT kernels (xca_any_kernel of csrc/xcit.hip, class_attn_any_kernel of csrc/cls_attn.hip):
one table, imported by tests/test_xca_any_gpu.py, tests/test_xca_any_cpu.py and tests/xca_any_arena_rows.py.  A plain module, nothing
here is collected.

Head widths 32 / 48 / 64 keep their template kernels; every other width from 1 to D_MAX runs the general kernels."""
from torch import nn

import oracle as O

D_MAX = 256
TEMPLATE_WIDTHS = (32, 48, 64)

# (B, N, heads, d) of the XCA core on the general kernel
CORE = [
    (2, 5, 3, 1),
    (2, 70, 3, 5),        # unaligned heads, two chunks with the last partial
    (1, 1, 2, 24),
    (2, 36, 4, 24),       # the live-fixture shape
    (2, 196, 8, 16),
    (3, 65, 2, 40),
    (2, 33, 2, 72),       # more than one row block
    (1, 196, 1, 96),
    (1, 17, 1, 129),      # odd, above 128
    (1, 64, 1, 256),
    (1, 300, 2, 20),
]
# softmax mask: k = -q at temperature 10 puts every diagonal logit at -10, so an unmasked padded column (logit 0) would take the row
MASK = [(2, 40, 2, 24), (2, 40, 3, 5)]
MASK_TEMPERATURE = 10.0
ZERO_CHANNEL = (2, 40, 2, 24)      # one all-zero q channel: the 1e-12 clamp of F.normalize
BATCH_INDEPENDENCE = [(3, 50, 2, 24), (3, 50, 2, 72)]
ROUTING_TEMPLATE, ROUTING_ANY, ROUTING_REFUSED = (32, 48, 64), (16, 24, 96), 257

# (B, N, heads, d) of the class-attention core on the general kernel
CLASS_ATTN = [(2, 1, 2, 24), (3, 65, 3, 5), (2, 197, 4, 24), (1, 50, 2, 72), (2, 33, 1, 256)]

# the arena rows (tests/xca_any_arena_rows.py)
ARENA_XCA = [(2, 70, 3, 5), (1, 33, 2, 72)]
ARENA_CLASS_ATTN = [(3, 65, 3, 5)]

# ---- module rows against the fp64 oracle (rows in the format of tests/route_cases.py / tests/model_cases.py) ------------------------
_XCIT = "vision_transformers.xcit"


def _xcab(heads, H, W):
    return lambda x, sd, dt: O.xca_block_forward(x, sd, heads, H, W, dt)


def _xcit_kw(dim, heads):
    return dict(img_size=64, patch_size=16, embed_dim=dim, depth=2, num_heads=heads, mlp_ratio=4, qkv_bias=True, norm_layer=nn.LayerNorm,
                cls_attn_layers=2, eta=1.0, num_classes=10)


MODULES = {
    "xca_c96_h4": dict(cls="XCA", args=(96, 4), kwargs=dict(qkv_bias=True), shape=(2, 36, 96), d=24, block=True,
                       oracle=lambda x, sd, dt: O.xca_forward(x, sd, 4, dt)),
    "xcab_c96_h4_fp32": dict(cls="XCABlock", args=(96, 4), kwargs=dict(qkv_bias=True, eta=1.0), shape=(3, 20, 96), fwd_args=(4, 5), d=24,
                             block=True, oracle=_xcab(4, 4, 5)),
    "xcab_c128_h8_fast": dict(cls="XCABlock", args=(128, 8), kwargs=dict(qkv_bias=True, eta=1.0), shape=(1, 196, 128), fwd_args=(14, 14), d=16,
                              block=True, oracle=_xcab(8, 14, 14), in16=True),
    "xcab_c320_h8": dict(cls="XCABlock", args=(320, 8), kwargs=dict(qkv_bias=True, eta=1.0), shape=(3, 49, 320), fwd_args=(7, 7), d=40,
                         block=True, oracle=_xcab(8, 7, 7)),
    "xcab_c256_h1": dict(cls="XCABlock", args=(256, 1), kwargs=dict(qkv_bias=True, eta=1.0), shape=(2, 16, 256), fwd_args=(4, 4), d=256,
                         block=True, oracle=_xcab(1, 4, 4)),
    "cab_c96_h4": dict(cls="ClassAttentionBlock", args=(96, 4), kwargs=dict(qkv_bias=True, eta=1.0), shape=(2, 17, 96), fwd_args=(4, 4), d=24,
                       oracle=lambda x, sd, dt: O.class_attention_block_forward(x, sd, 4, dt)),
    "xcit_c96_h4": dict(cls="XCiT", kwargs=_xcit_kw(96, 4), shape=(2, 3, 64, 64), d=24,
                        oracle=lambda x, sd, dt: O.xcit_forward(x, sd, 4, 2, 2, dt)),
    "xcit_c160_h2": dict(cls="XCiT", kwargs=_xcit_kw(160, 2), shape=(2, 3, 64, 64), d=80,
                         oracle=lambda x, sd, dt: O.xcit_forward(x, sd, 2, 2, 2, dt)),
}


def build(rid, namespace=None):
    """(module, x) of a module row: route_cases.build_row for blocks, model_cases.build_row for the rest.  `namespace`: the module
    that holds the classes (default: the drop-in vision_transformers.xcit)."""
    import importlib

    import model_cases
    import route_cases
    row = MODULES[rid]
    cls = getattr(namespace or importlib.import_module(_XCIT), row["cls"])
    return (route_cases if row.get("block") else model_cases).build_row(row, cls)

