"""Helpers and shape tables shared by the kernel-level GPU tests.

  _drain_range        swallow a pending fp16 range report, so that a test starts (or leaves) with none
  _tags               kernel_trace tags of one call
  _ref_linear         fp64 evaluation of a linear16 call on its 16-bit operands
  _xca_ref            fp64 evaluation of the XCA core on 16-bit q / k / v
  _seeded, _sd, _bn_randomise
                      a module from a fixed seed, its state dict on the CPU, non-trivial BatchNorm statistics and affine parts
  P8_SHAPES, PA_SHAPES, TAIL_SHAPES, W4_CASES
                      products for gemm16_p8 / gemm16_pa / the ring-kernel tail of gemm16_pa / gemm16_w4
  STRIPES, DA_SHAPES  CSWin stripe geometries, DoubleAttention inputs on the two-pass path
"""
import torch


def _drain_range():
    import mi355attn
    try:
        mi355attn.range_status(wait=True)
    except mi355attn.Mi355RangeError:
        pass


def _tags(fn):
    import mi355attn
    return [t for t, *_ in mi355attn.kernel_trace(fn)]


def _ref_linear(x16, w16, b, act, resid=None, gamma=None):
    """fp64 evaluation of a linear16 call on its 16-bit operands: gelu(x w^T + b) * gamma + resid."""
    y = x16.double() @ w16.double().t()
    if b is not None:
        y = y + b.double()
    if act:
        y = torch.nn.functional.gelu(y)
    if gamma is not None:
        y = y * gamma.double()
    if resid is not None:
        y = y + resid.double()
    return y


def _xca_ref(qkv16, temperature, heads):
    """fp64 evaluation of xcit.py:249-262 on the 16-bit inputs (what both kernels are given)."""
    B, N, C3 = qkv16.shape
    C = C3 // 3
    d = C // heads
    q, k, v = (qkv16.double().cpu().reshape(B, N, 3, heads, d).permute(2, 0, 3, 4, 1))      # (3, B, h, d, N)
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    k = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    a = ((q @ k.transpose(-2, -1)) * temperature.double().cpu().reshape(1, heads, 1, 1)).softmax(dim=-1)
    return (a @ v).permute(0, 3, 1, 2).reshape(B, N, C)


def _seeded(ctor, seed=1234):
    torch.manual_seed(seed)
    return ctor().eval()


def _sd(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _bn_randomise(mod):
    with torch.no_grad():
        for c in mod.modules():
            if isinstance(c, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                c.running_mean.normal_(0, 0.3)
                c.running_var.uniform_(0.5, 1.5)
                c.weight.uniform_(0.5, 1.5)
                c.bias.normal_(0, 0.2)


P8_SHAPES = [  # (M, N, K): all have >= one full round of 256x256 tiles on a 256-CU part unless forced through gemm_variant 15
    (50432, 2304, 768), (50432, 768, 768), (12544, 1536, 512), (50176, 1152, 384),
    (65536 + 40, 256 + 8, 256),          # ragged in both directions, 2 tile columns, the second almost empty
    (300, 264, 128), (256, 256, 64), (1, 8, 64), (4097, 520, 192),
]


PA_SHAPES = [  # (M, N, K): M % 128 == 0, N % 256 == 0, K >= 640
    (128, 256, 640),                 # one tile, one workgroup: serial drain only
    (128 * 5, 512, 768),             # 10 tiles on 256 CUs: one tile each
    (128 * 300, 256, 640),           # 300 tiles: one full round + a partial one; tiles_n = 1
    (128 * 394, 768, 768),           # ViT-Base proj: 4.6 rounds
    (128 * 200, 768, 3072),          # long reduction (ViT-Base fc2 geometry)
    (128 * 37, 1024, 1152),
    # round 4, swapped orientation (256 x 128 tiles): M % 256 == 0, N % 128 == 0 but not % 256
    (256, 128, 640),                 # one tile
    (256 * 3, 384, 768),             # 9 tiles, three column tiles per row panel
    (256 * 196, 384, 1536),          # XCiT-S fc2 at B = 256: 588 tiles = 2.3 rounds
    (256 * 70, 640, 1024),           # five column tiles
    # round 4, short reductions (16-bit epilogue packed two / three pieces per barrier interval; fp32 outputs refuse K < 640)
    (128 * 40, 512, 256),            # K = 256: four K-tiles, three pieces per interval
    (128 * 300, 768, 320),           # five K-tiles, two pieces per interval
    (256 * 20, 384, 384),            # swapped orientation + six K-tiles
    (128 * 64, 1024, 512),           # eight K-tiles
]


# left-over rows of the two-accumulator GEMM on ring-pipelined small tiles (option "gemm_pa_tail"; gemm16.hip)
TAIL_SHAPES = [  # (M, N, K, tail kernel expected)
    (128 * 392, 512, 2048, "32x64"),      # MixerLayer fc2 at B = 256: 784 tiles = 3.06 rounds -> 49 152 rows + 1 024 rows (the default's case)
    (256 * 196, 384, 1536, "32x64"),      # XCiT-S fc2: 588 swapped tiles = 2.30 rounds -> 43 520 rows + 6 656 rows (1 248 ring workgroups, five per CU in turn)
    (128 * 264, 256, 1024, "32x64"),      # one column tile, eight left-over tiles, the shortest reduction that splits
    (128 * 160, 512, 1088, "32x64"),      # 320 tiles: one round + 64 (4 096 rows); 17 K-tiles (more than the ring holds)
]


# gemm16_w4.hip: the one-wave-per-SIMD persistent kernel
W4_CASES = [  # M, N, K, gelu, bias
    (2048, 2304, 768, False, True),        # fewer tiles than CUs (72)
    (256 * 20, 768, 768, True, True),      # 60 tiles, GELU epilogue
    (256 * 90, 768, 320, False, False),    # 270 tiles = 1 round + 14, odd number of K-tiles (5), no bias
    (256 * 30, 512, 128, False, True),     # two K-tiles: the shortest stream the kernel takes
    (256 * 33, 1024, 1024, True, False),   # 132 tiles, GELU, no bias
    (256 * 131, 512, 576, False, True),    # 262 tiles = 1 round + 6
    (256 * 197, 2304, 768, False, True),   # the qkv product of ViT-Base at the timed size (B = 256): 1773 tiles = 6.93 rounds
    (256 * 197, 3072, 768, True, True),    # fc1 of ViT-Base at the timed size, GELU epilogue: 2364 tiles
]


STRIPES = [  # (C, reso, heads, split, B): tokens per stripe = reso * split <= 64
    (64, 56, 2, 1, 3), (128, 28, 4, 2, 3), (64, 28, 2, 2, 2), (64, 8, 2, 2, 5), (128, 16, 4, 4, 2), (64, 16, 2, 1, 1), (128, 8, 4, 8, 2), (64, 7, 2, 7, 3),
]


DA_SHAPES = [  # (B, C, H, W): c_m = c_n = 128 -- the two-pass path; pixel counts with and without a ragged last 32-pixel tile
    (3, 256, 56, 56), (1, 256, 56, 56), (2, 256, 14, 14), (5, 128, 28, 28), (2, 256, 10, 10), (1, 128, 2, 2), (2, 256, 6, 10), (37, 256, 8, 8), (2, 256, 9, 12), (300, 128, 6, 6),
]
