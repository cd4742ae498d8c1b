"""What tests/test_xcit_io16_cpu.py and tests/test_xcit_io16_gpu.py share: the XCABlock and XCiT shapes and seeds, the module and input
builders, and the fp64 emulation of the 16-bit interface (oracle.xca_block_forward on x rounded to the I/O type with y rounded once; for
the model, the fp64 composition with the stream rounded behind the embedding and every XCABlock, the class-attention tail wide and the
logits rounded once).  References are computed once per (case, type) and never modified.  A plain module, not a test file: nothing here
is collected.

The shapes are the smallest that reach each way the code can go: three images of 5 x 7 tokens (M = 105: ragged for the 128-row GEMM
tiles, the 32-row tiles of the weight-stationary kernel, the 32 / 64-token chunks of the fused MLP and the 256-token steps of its
streaming form), both fused-MLP widths, a width between them on the tile GEMMs, both widths of the statistics-writing projection (the
C4 shape at a small batch), the LayerScale initialisation that fp16 cannot fold, a grid above 256 tokens (the tiled LPI kernel) and the
two ways onto the widening route."""
import functools

import torch

import oracle as O
from route_cases import prep_nontrivial

DTYPES = [torch.float16, torch.bfloat16]
IO = {torch.float16: 1, torch.bfloat16: 2}

# id -> XCABlock(dim, heads, eta=eta) on x (B, H * W, dim).  route: "G-fused" / "G" / "G-stats" the 16-bit dataflow (by its proj and MLP
# kernels), "W" widen, the fp32 body, round.  route16: the route per I/O type where the two differ.
BLOCKS = {
    "c64_h2": dict(dim=64, heads=2, eta=1.0, B=3, hw=(5, 7), route="G-fused"),          # mlp_fused_kernel o16, a ragged 32-token chunk
    "c64_h2_tt4": dict(dim=64, heads=2, eta=1.0, B=3, hw=(5, 7), route="G-fused", opts=dict(mlp_tt4=1)),
    "c128_h4": dict(dim=128, heads=4, eta=1.0, B=3, hw=(5, 7), route="G-fused"),        # mlp_fused_stream_kernel o16 (the nano model's width)
    "c192_h4": dict(dim=192, heads=4, eta=1.0, B=3, hw=(5, 7), route="G"),              # d = 48; gemm16_res r16 -> o32 and r32 -> o16, folded
    "c256_h8": dict(dim=256, heads=8, eta=1.0, B=3, hw=(5, 7), route="G-stats"),        # wreg resid16 + stats, last tile partial
    "c384_h8": dict(dim=384, heads=8, eta=1.0, B=2, hw=(14, 14), route="G-stats"),      # the C4 shape at a small batch
    # eta = 1e-5: in fp16 the fold returns None, gamma runs in both gemm16_res epilogues; bf16 folds and takes the statistics kernel
    "c256_eta": dict(dim=256, heads=8, eta=1e-5, B=3, hw=(5, 7), route="G", route16={torch.bfloat16: "G-stats"}),
    "c64_tile": dict(dim=64, heads=2, eta=1.0, B=1, hw=(18, 18), route="G-fused"),      # N = 324 > 256: lpi_tile_kernel inside the 16-bit block
    "c100_h4": dict(dim=100, heads=4, eta=1.0, B=3, hw=(5, 7), route="W"),              # dim % 64 != 0, d = 25 on the run-time-width XCA kernel
    "c256_p0": dict(dim=256, heads=8, eta=1.0, B=3, hw=(5, 7), route="W", precision=0),  # strict
}
SEED = {cid: 9700 + 17 * i for i, cid in enumerate(BLOCKS)}

MODEL = dict(img_size=64, patch_size=16, embed_dim=64, depth=2, num_heads=2, cls_attn_layers=2, num_classes=10, eta=1.0, qkv_bias=True)
MODEL_SHAPE, MODEL_SEED = (2, 3, 64, 64), 9901


def route(cid, dtype):
    c = BLOCKS[cid]
    return c.get("route16", {}).get(dtype, c["route"])


def block_module(cid, precision="case"):
    """A fresh fp32 XCABlock of the case on the CPU: LayerNorm, BatchNorm, bias, gamma and temperature parameters non-trivial
    (prep_nontrivial; eta sets the magnitude of the gammas).  precision: the constructor's (default: the case's own, None unless the
    case names one)."""
    from mi355attn.modules import XCABlock
    c = BLOCKS[cid]
    torch.manual_seed(SEED[cid])
    m = XCABlock(c["dim"], c["heads"], eta=c["eta"], precision=c.get("precision") if precision == "case" else precision).eval()
    prep_nontrivial(m)
    return m.requires_grad_(False)


def block_shape(cid):
    c = BLOCKS[cid]
    return c["B"], c["hw"][0] * c["hw"][1], c["dim"]


def block_input(cid):
    """The fp32 input of the case (the tests round it to the I/O type)."""
    g = torch.Generator().manual_seed(SEED[cid] + 1)
    return torch.randn(*block_shape(cid), generator=g) * 1.3 + 0.2


def _sd(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


@functools.lru_cache(maxsize=None)
def block_plain(cid, dtype):
    """The fp64 restatement on x rounded to dtype (the tensor the user hands over), y left wide."""
    c = BLOCKS[cid]
    return O.xca_block_forward(block_input(cid).to(dtype).double(), _sd(block_module(cid)), c["heads"], *c["hw"], dtype=torch.float64)


def block_emulated(cid, dtype):
    """... y rounded once to dtype: the 16-bit interface with exact arithmetic inside."""
    return block_plain(cid, dtype).to(dtype)


def model_module(**over):
    from mi355attn.modules import XCiT
    torch.manual_seed(MODEL_SEED)
    m = XCiT(norm_layer=torch.nn.LayerNorm, **dict(MODEL, **over)).eval()
    prep_nontrivial(m)
    with torch.no_grad():
        m.cls_token.copy_(0.2 * torch.randn(m.cls_token.shape, generator=torch.Generator().manual_seed(MODEL_SEED + 2)))
    return m.requires_grad_(False)


def model_input():
    g = torch.Generator().manual_seed(MODEL_SEED + 1)
    return torch.randn(*MODEL_SHAPE, generator=g)


@functools.lru_cache(maxsize=None)
def model_refs(dtype):
    """(oracle on the image rounded to dtype with nothing rounded inside, fp64 emulation of the 16-bit composition: the stream rounded
    behind the embedding and behind every XCABlock, the class-attention tail, the final LayerNorm and the head kept wide, the logits
    rounded once)."""
    import oracle.transformer as OT
    import oracle.xcit as OX
    sd, img = _sd(model_module()), model_input().to(dtype).double()
    heads, depth, cls_layers = MODEL["num_heads"], MODEL["depth"], MODEL["cls_attn_layers"]
    plain = O.xcit_forward(img, sd, heads, depth, cls_layers, torch.float64)

    def sub(prefix):
        return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    x, (Hp, Wp) = OX.conv_patch_embed_forward(img, sub("patch_embed."), torch.float64)
    x = x + OX.fourier_position_rows(Hp, Wp, sd["pos_embeder.token_projection.weight"], sd["pos_embeder.token_projection.bias"], dtype=torch.float64)
    x = x.to(dtype).double()
    for i in range(depth):
        x = OX.xca_block_forward(x, sub(f"blocks.{i}."), heads, Hp, Wp, torch.float64).to(dtype).double()
    x = torch.cat([sd["cls_token"].double().expand(x.shape[0], -1, -1), x], dim=1)
    for i in range(cls_layers):
        x = OX.class_attention_block_forward(x, sub(f"cls_attn_blocks.{i}."), heads, torch.float64)
    x = OT.layernorm(x, sd["norm.weight"].double(), sd["norm.bias"].double())[:, 0]
    logits = OT.linear(x, sd["head.weight"].double(), sd["head.bias"].double())
    return plain, logits.to(dtype)
