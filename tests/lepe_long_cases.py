"""Shapes and builders shared by the long-window LePE tests (tests/test_lepe_long_gpu.py, tests/test_lepe_long_cpu.py) and by the
fixture writer tests/golden/make_lepe_long.py: stripe windows of 225 .. 512 tokens, the envelope win_attn_long_kernel of
csrc/attn.hip adds to the three LePE entries.

Every builder takes the classes to build from, so the same seed protocol runs on the drop-in modules (the tests) and on the reference's
(the fixture writer): same constructor arguments, same init stream, same perturbation of the LayerNorm / bias parameters.
"""
import torch

# (reso, idx, split, dim, heads): T = H_sp * W_sp tokens per stripe window, head width 32
WINDOWS = [(15, -1, 15, 32, 1),       # T = 225: one key and one query row past the short kernel, a last tile with one live slot
           (16, -1, 16, 64, 2),       # T = 256: a multiple of every tile and block size; the full-plane window of a last stage
           (24, 0, 12, 64, 2), (24, 1, 12, 64, 2),       # T = 288: the 384 px stage-3 stripes, two windows per image
           (30, 0, 10, 64, 2), (30, 1, 10, 64, 2),       # T = 300: no multiple of 16; W_sp = 10 borders for LePE
           (32, 0, 16, 32, 1), (32, 1, 16, 32, 1)]       # T = 512: the maximum (batch 1)
T288, T512 = (24, 0, 12, 64, 2), (32, 0, 16, 32, 1)
TOO_LONG = (23, -1, 23, 32, 1)        # T = 529
# T = 224, the short kernel's largest window.  (H_sp, W_sp) = (56, 4): both divide the 56 x 56 grid, as the entries require.
SHORT_MAX = (56, 0, 4, 32, 1)

# CSWinBlock rows: (id, constructor args, kwargs, input shape, (reso, heads, split) of the oracle)
BLOCKS = [("c256_reso24_split12", (256, 24, 8), dict(split_size=12, qkv_bias=True), (2, 576, 256), (24, 8, 12)),
          ("c64_reso16_split16", (64, 16, 2), dict(split_size=16, qkv_bias=True), (2, 256, 64), (16, 2, 16))]
MODEL_KW = dict(img_size=384, patch_size=4, embed_dim=64, depth=[1, 1, 1, 1], split_size=[1, 2, 12, 12], num_heads=[2, 4, 8, 16],
                num_classes=10)
MODEL_SHAPE = (1, 3, 384, 384)


def wid(case):
    return "r%d_i%d_s%d_c%d_h%d" % case


def batch(case):
    return 1 if case[0] * case[0] >= 1024 else 2


def stripe(case):
    reso, idx, split = case[:3]
    return (reso, reso) if idx < 0 else ((reso, split) if idx == 0 else (split, reso))


def tokens(case):
    h, w = stripe(case)
    return h * w


def lepe_inputs(cls, case):
    """(module, qkv) under the protocol of tests/test_ops_gpu.py::test_lepe_attention_vs_oracle: seed reso + dim, then randn."""
    reso, idx, split, dim, heads = case
    torch.manual_seed(reso + dim)
    m = cls(dim, reso, idx, split_size=split, num_heads=heads).eval()
    return m, torch.randn(3, batch(case), reso * reso, dim)


def block_inputs(cls, row):
    """(module, x) of a BLOCKS row: the seed protocol and the non-trivial LayerNorm / bias parameters of tests/route_cases.py."""
    from route_cases import build_row
    _, args, kwargs, shape, _ = row
    return build_row(dict(args=args, kwargs=kwargs, shape=shape), cls)


def model_inputs(cls):
    from model_cases import build_row
    return build_row(dict(kwargs=dict(MODEL_KW), shape=MODEL_SHAPE), cls)


def state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}
