"""What tests/test_vit_io16_cpu.py and tests/test_vit_io16_gpu.py share: the TransformerEncoder and VisionTransformer shapes and seeds,
the module and input builders, and the fp64 emulation of the 16-bit interface (the oracle's ViT restatement on x rounded to the I/O type
with y rounded once; for the model, the token stream rounded behind the embedding and behind every block).  References are computed
once per (case, type) and never modified.  A plain module, not a test file: nothing here is collected."""
import functools

import torch

import oracle as O
from route_cases import prep_nontrivial

DTYPES = [torch.float16, torch.bfloat16]
IO = {torch.float16: 1, torch.bfloat16: 2}

# id -> TransformerEncoder(C, heads, qkv_bias[, precision]) at (B, N); fast: the 16-bit route without a widen / round launch
BLOCKS = {
    "c128_h4_n197": dict(C=128, heads=4, qkv_bias=False, B=2, N=197, fast=True),             # d = 32, short K
    "c256_h4_n50_b3": dict(C=256, heads=4, qkv_bias=True, B=3, N=50, fast=True),             # d = 64
    "c384_h6_n197": dict(C=384, heads=6, qkv_bias=True, B=1, N=197, fast=True),
    "c256_h2_n230": dict(C=256, heads=2, qkv_bias=False, B=1, N=230, fast=True),             # d = 128, streaming core
    "c768_h12_n197": dict(C=768, heads=12, qkv_bias=True, B=2, N=197, fast=True),            # ViT-Base width
    "c192_h4_n50": dict(C=192, heads=4, qkv_bias=False, B=2, N=50, fast=False),              # d = 48: widening route
    "c96_h3_n17": dict(C=96, heads=3, qkv_bias=False, B=2, N=17, fast=False),                # K % 64 != 0: widening route
    "c256_h4_n50_strict": dict(C=256, heads=4, qkv_bias=True, B=1, N=50, fast=False, precision=0),      # strict route
}
SEED = {cid: 8100 + 17 * i for i, cid in enumerate(BLOCKS)}

# id -> VisionTransformer(image 64, patch 16, dim 128, depths 2, heads 4, classes 10) on `shape`
MODEL = dict(image_size=64, patch_size=16, embedding_dim=128, depths=2, num_heads=4, num_classes=10, seed=8501)
MODELS = {
    "token_64": dict(global_pool="token", shape=(2, 3, 64, 64)),
    "avg_64": dict(global_pool="avg", shape=(2, 3, 64, 64)),
    "token_96": dict(global_pool="token", shape=(1, 3, 96, 96)),                             # resizes the position table
}


def block_module(cid, precision="case"):
    """A fresh fp32 TransformerEncoder of the case on the CPU, LayerNorm parameters and biases non-trivial (prep_nontrivial).
    precision: the constructor's (default: the case's own, None unless the case names one)."""
    from mi355attn.modules import TransformerEncoder
    c = BLOCKS[cid]
    torch.manual_seed(SEED[cid])
    m = TransformerEncoder(c["C"], c["heads"], qkv_bias=c["qkv_bias"], precision=c.get("precision") if precision == "case" else precision).eval()
    prep_nontrivial(m)
    return m.requires_grad_(False)


def block_input(cid):
    """The fp32 input of the case (the tests round it to the I/O type)."""
    c = BLOCKS[cid]
    g = torch.Generator().manual_seed(SEED[cid] + 1)
    return torch.randn(c["B"], c["N"], c["C"], generator=g) * 1.3 + 0.2


def _sd(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


@functools.lru_cache(maxsize=None)
def block_plain(cid, dtype):
    """The fp64 restatement on x rounded to dtype (the tensor the user hands over), y left wide."""
    return O.vit_encoder_forward(block_input(cid).to(dtype).double(), _sd(block_module(cid)), BLOCKS[cid]["heads"], torch.float64)


def block_emulated(cid, dtype):
    """... y rounded once to dtype: the 16-bit interface with exact arithmetic inside."""
    return block_plain(cid, dtype).to(dtype)


def model_module(mid):
    from mi355attn.modules import VisionTransformer
    torch.manual_seed(MODEL["seed"])
    m = VisionTransformer(image_size=MODEL["image_size"], patch_size=MODEL["patch_size"], depths=MODEL["depths"], num_heads=MODEL["num_heads"],
                          embedding_dim=MODEL["embedding_dim"], num_classes=MODEL["num_classes"], global_pool=MODELS[mid]["global_pool"]).eval()
    prep_nontrivial(m)
    return m.requires_grad_(False)


def model_input(mid):
    g = torch.Generator().manual_seed(MODEL["seed"] + 1)
    return torch.randn(*MODELS[mid]["shape"], generator=g)


@functools.lru_cache(maxsize=None)
def model_refs(mid, dtype):
    """(oracle on the image rounded to dtype with nothing rounded inside, fp64 emulation of the 16-bit composition): the token stream
    rounded behind the embedding and behind every block, the pooled row kept wide, the logits rounded once."""
    import oracle.transformer as OT
    sd, img = _sd(model_module(mid)), model_input(mid).to(dtype).double()
    pool, heads, depth = MODELS[mid]["global_pool"], MODEL["num_heads"], MODEL["depths"]
    plain = O.vit_forward(img, sd, heads, depth, torch.float64, pool)
    w = sd["patch_embedding.proj.weight"]
    x = OT.vit_patch_embed_forward(img, w, sd["patch_embedding.proj.bias"], torch.float64)
    cls = sd["cls_token"].double().expand(x.shape[0], -1, -1)
    x = torch.cat([x, cls], dim=1) + OT.vit_position_rows(sd["position_embedding"], w.shape[-1], img.shape[-2], img.shape[-1], torch.float64)
    x = x.to(dtype).double()
    for i in range(depth):
        sub = {k[len(f"blocks.{i}."):]: v for k, v in sd.items() if k.startswith(f"blocks.{i}.")}
        x = O.vit_encoder_forward(x, sub, heads, torch.float64).to(dtype).double()
    pooled = x[:, 0] if pool == "token" else x[:, 1:].mean(dim=1)
    logits = OT.linear(pooled, sd["head.weight"].double(), sd["head.bias"].double())
    return plain, logits.to(dtype)
