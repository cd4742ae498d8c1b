"""What tests/test_cswin_io16_cpu.py and tests/test_cswin_io16_gpu.py share: the CSWinBlock and CSWinTransformer shapes and seeds, the
module and input builders, and the fp64 emulation of the 16-bit interface (oracle.cswin.cswin_block_forward on x rounded to the I/O type
with y rounded once; for the model, the fp64 composition with the stream rounded behind the stem, every block and every merge).
References are computed once per (case, type) and never modified.  A plain module, not a test file: nothing here is collected.

The shapes are the smallest that reach each way the code can go: the four instantiations of the stripe kernel (split == 1 or not, fewer
than 48 tokens per stripe or not) at C = 64 and C = 128, a ragged last chunk of the proj + MLP kernels (M = 108 at 32 tokens per wave,
M = 36 on the streaming kernel), both forms of the C = 64 kernel (option mlp_tt4), the block without a fused MLP, the routes that reuse
the GEMMs (stripes above 64 tokens, C = 256 / 512, one branch, the last stage) and the widening route."""
import functools

import torch

import oracle as O
from route_cases import prep_nontrivial

DTYPES = [torch.float16, torch.bfloat16]
IO = {torch.float16: 1, torch.bfloat16: 2}

# id -> CSWinBlock(*args, **kw) on x (B, reso^2, C).  route: "A" stripe x16 + proj/MLP x16, "A2" stripe x16 without the fused MLP,
# "B" LayerNorm x16 + qkv GEMM + LePE core + proj/MLP x16, "B2" the same with the GEMM second half, "C" widen, fp32 body, round
BLOCKS = {
    "c64_r6_s2": dict(args=(64, 6, 2), kw=dict(split_size=2, qkv_bias=True), B=3, route="A"),            # split > 1, T = 12 < 48; M = 108 ragged
    "c64_r8_s1": dict(args=(64, 8, 2), kw=dict(split_size=1, qkv_bias=True), B=2, route="A"),            # split == 1, T = 8 < 48
    "c64_r56_s1": dict(args=(64, 56, 2), kw=dict(split_size=1, qkv_bias=True), B=1, route="A"),          # split == 1, T = 56: stage 1
    "c64_r28_s2": dict(args=(64, 28, 2), kw=dict(split_size=2, qkv_bias=True), B=1, route="A"),          # split > 1, T = 56
    "c128_r6_s3": dict(args=(128, 6, 4), kw=dict(split_size=3, qkv_bias=True), B=1, route="A"),          # stream kernel, M = 36 ragged
    "c128_r8_s1": dict(args=(128, 8, 4), kw=dict(split_size=1), B=2, route="A"),                         # no qkv bias
    "c128_r56_s1": dict(args=(128, 56, 4), kw=dict(split_size=1, qkv_bias=True), B=1, route="A"),
    "c128_r28_s2": dict(args=(128, 28, 4), kw=dict(split_size=2, qkv_bias=True), B=1, route="A"),        # stage 2
    "c64_r6_s2_tt4": dict(args=(64, 6, 2), kw=dict(split_size=2, qkv_bias=True), B=3, route="A", opts=dict(mlp_tt4=1)),
    "c64_r8_s2_mlp2": dict(args=(64, 8, 2), kw=dict(split_size=2, mlp_ratio=2., qkv_bias=True), B=3, route="A2"),
    "c64_r96_s1": dict(args=(64, 96, 2), kw=dict(split_size=1, qkv_bias=True), B=1, route="B"),          # T = 96 > 64: 384-px stripes
    "c256_r14_s7": dict(args=(256, 14, 8), kw=dict(split_size=7, qkv_bias=True), B=1, route="B2"),       # stage 3
    "c256_r7_s7": dict(args=(256, 7, 8), kw=dict(split_size=7, qkv_bias=True), B=3, route="B2"),         # reso == split: one branch
    "c512_r7_last": dict(args=(512, 7, 16), kw=dict(split_size=7, qkv_bias=True, last_stage=True), B=1, route="B2"),
    # K % 64 != 0.  One head of width 32 needs the one-branch form (reso == split): two branches would leave num_heads // 2 = 0 heads each
    "c32_r8_s8": dict(args=(32, 8, 1), kw=dict(split_size=8), B=2, route="C"),
    "c64_r6_s2_strict": dict(args=(64, 6, 2), kw=dict(split_size=2, qkv_bias=True), B=3, route="C", precision=0),
}
SEED = {cid: 9100 + 17 * i for i, cid in enumerate(BLOCKS)}

MODEL = dict(img_size=64, patch_size=4, embed_dim=64, depth=[1, 1, 1, 1], split_size=[1, 2, 2, 2], num_heads=[2, 4, 8, 16], num_classes=10)
MODEL_SHAPE, MODEL_SEED = (2, 3, 64, 64), 9501


def block_module(cid, precision="case"):
    """A fresh fp32 CSWinBlock of the case on the CPU, LayerNorm parameters and biases non-trivial (prep_nontrivial).
    precision: the constructor's (default: the case's own, None unless the case names one)."""
    from mi355attn.modules import CSWinBlock
    c = BLOCKS[cid]
    torch.manual_seed(SEED[cid])
    m = CSWinBlock(*c["args"], precision=c.get("precision") if precision == "case" else precision, **c["kw"]).eval()
    prep_nontrivial(m)
    return m.requires_grad_(False)


def block_shape(cid):
    c = BLOCKS[cid]
    return c["B"], c["args"][1] ** 2, c["args"][0]


def block_input(cid):
    """The fp32 input of the case (the tests round it to the I/O type)."""
    g = torch.Generator().manual_seed(SEED[cid] + 1)
    return torch.randn(*block_shape(cid), generator=g) * 1.3 + 0.2


def _sd(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _block64(x, sd, cid):
    c = BLOCKS[cid]
    _, reso, heads = c["args"]
    return O.cswin_block_forward(x, sd, reso, heads, c["kw"]["split_size"], last_stage=c["kw"].get("last_stage", False), dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def block_plain(cid, dtype):
    """The fp64 restatement on x rounded to dtype (the tensor the user hands over), y left wide."""
    return _block64(block_input(cid).to(dtype).double(), _sd(block_module(cid)), cid)


def block_emulated(cid, dtype):
    """... y rounded once to dtype: the 16-bit interface with exact arithmetic inside."""
    return block_plain(cid, dtype).to(dtype)


def model_module():
    from mi355attn.modules import CSWinTransformer
    torch.manual_seed(MODEL_SEED)
    m = CSWinTransformer(**MODEL).eval()
    prep_nontrivial(m)
    return m.requires_grad_(False)


def model_input():
    g = torch.Generator().manual_seed(MODEL_SEED + 1)
    return torch.randn(*MODEL_SHAPE, generator=g)


@functools.lru_cache(maxsize=None)
def model_refs(dtype):
    """(oracle on the image rounded to dtype with nothing rounded inside, fp64 emulation of the 16-bit composition: the stream rounded
    behind the stem, every block and every merge; the final LayerNorm, the pooled row and the head kept wide; the logits rounded once)."""
    import torch.nn.functional as TF

    import oracle.transformer as OT
    sd, img = _sd(model_module()), model_input().to(dtype).double()
    depth, split, heads = MODEL["depth"], MODEL["split_size"], MODEL["num_heads"]
    plain = O.cswin_forward(img, sd, MODEL["embed_dim"], tuple(depth), tuple(split), tuple(heads), torch.float64)

    def d(k):
        return sd[k].double()

    def sub(prefix):
        return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    B = img.shape[0]
    x = TF.conv2d(img, d("stage1_conv_embed.0.weight"), d("stage1_conv_embed.0.bias"), stride=4, padding=2)
    reso = x.shape[-1]
    x = OT.layernorm(x.flatten(2).transpose(1, 2), d("stage1_conv_embed.2.weight"), d("stage1_conv_embed.2.bias"))
    x = x.to(dtype).double()
    for si in range(4):
        if si > 0:
            grid = x.transpose(1, 2).reshape(B, x.shape[-1], reso, reso)
            grid = TF.conv2d(grid, d(f"merge{si}.conv.weight"), d(f"merge{si}.conv.bias"), stride=2, padding=1)
            reso = grid.shape[-1]
            x = OT.layernorm(grid.flatten(2).transpose(1, 2), d(f"merge{si}.norm.weight"), d(f"merge{si}.norm.bias")).to(dtype).double()
        for bi in range(depth[si]):
            x = O.cswin_block_forward(x, sub(f"stage{si + 1}.{bi}."), reso, heads[si], split[si], last_stage=(si == 3),
                                      dtype=torch.float64).to(dtype).double()
    pooled = OT.layernorm(x, d("norm.weight"), d("norm.bias")).mean(dim=1)
    logits = OT.linear(pooled, d("head.weight"), d("head.bias"))
    return plain, logits.to(dtype)
