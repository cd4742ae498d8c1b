"""What tests/test_mixer_io16_cpu.py and tests/test_mixer_io16_gpu.py share: the MixerLayer shapes and seeds, the module and input
builders, and the fp64 emulation of the 16-bit interface (the oracle's Mixer restatement on x rounded to the I/O type with y rounded
once; for the model, the stream rounded behind the embedding and behind every layer).  References are computed once per (case, type)
and never modified.  A plain module, not a test file: nothing here is collected."""
import functools

import torch

import oracle as O
from route_cases import prep_nontrivial

DTYPES = [torch.float16, torch.bfloat16]
IO = {torch.float16: 1, torch.bfloat16: 2}

# id -> MixerLayer(C, N, mlp_ratio) at batch B; fused: inside the envelope of the token kernel (N = 196, T % 32 == 0 <= 512, C % 256 == 0 <= 1024)
LAYERS = {
    "c256_b1": dict(C=256, N=196, ratio=None, B=1, fused=True),              # one workgroup per image
    "c256_b3": dict(C=256, N=196, ratio=None, B=3, fused=True),
    "c512_b2": dict(C=512, N=196, ratio=None, B=2, fused=True),              # two halves, no XCD pairing
    "c512_b8": dict(C=512, N=196, ratio=None, B=8, fused=True),              # two halves, XCD pairing
    "c1024_b1": dict(C=1024, N=196, ratio=None, B=1, fused=True),            # widest, T = 512
    "c256_t32_b2": dict(C=256, N=196, ratio=[0.125, 4], B=2, fused=True),    # T = 32: one hidden block
    "c128_n49_b2": dict(C=128, N=49, ratio=None, B=2, fused=False),          # outside the envelope: widening route (channel-major GEMMs)
    "c1280_b1": dict(C=1280, N=196, ratio=None, B=1, fused=False),           # outside the envelope: widening route (fp32 token mixing)
}
SEED = {cid: 7000 + 13 * i for i, cid in enumerate(LAYERS)}
MODEL = dict(dim=256, depth=2, num_classes=10, shape=(2, 3, 224, 224), seed=7301)


def layer_module(cid):
    """A fresh fp32 MixerLayer of the case on the CPU, LayerNorm parameters and biases non-trivial (route_cases.prep_nontrivial)."""
    from mi355attn.modules import MixerLayer
    c = LAYERS[cid]
    torch.manual_seed(SEED[cid])
    m = MixerLayer(c["C"], c["N"], mlp_ratio=c["ratio"] or [0.5, 4]).eval()
    prep_nontrivial(m)
    return m.requires_grad_(False)


def layer_input(cid):
    """The fp32 input of the case (the tests round it to the I/O type)."""
    c = LAYERS[cid]
    g = torch.Generator().manual_seed(SEED[cid] + 1)
    return torch.randn(c["B"], c["N"], c["C"], generator=g) * 1.3 + 0.2


def _sd(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


@functools.lru_cache(maxsize=None)
def layer_plain(cid, dtype):
    """The fp64 restatement on x rounded to dtype (the tensor the user hands over), y left wide."""
    return O.mixer_layer_forward(layer_input(cid).to(dtype).double(), _sd(layer_module(cid)), torch.float64)


def layer_emulated(cid, dtype):
    """... y rounded once to dtype: the 16-bit interface with exact arithmetic inside."""
    return layer_plain(cid, dtype).to(dtype)


def model_module():
    from mi355attn.modules import MLP_Mixer
    torch.manual_seed(MODEL["seed"])
    m = MLP_Mixer(dim=MODEL["dim"], depth=MODEL["depth"], num_classes=MODEL["num_classes"]).eval()
    prep_nontrivial(m)
    return m.requires_grad_(False)


def model_input():
    g = torch.Generator().manual_seed(MODEL["seed"] + 1)
    return torch.randn(*MODEL["shape"], generator=g)


@functools.lru_cache(maxsize=None)
def model_refs(dtype):
    """(oracle on the image rounded to dtype with nothing rounded inside, fp64 emulation of the 16-bit composition): the token stream
    rounded behind the embedding and behind every layer, the pooled row kept wide, the logits rounded once."""
    import oracle.transformer as OT
    sd, img = _sd(model_module()), model_input().to(dtype).double()
    plain = O.mixer_forward(img, sd, MODEL["depth"], torch.float64)
    x = OT.vit_patch_embed_forward(img, sd["patch_embedding.proj.weight"], sd["patch_embedding.proj.bias"], torch.float64)
    x = x.to(dtype).double()
    for i in range(MODEL["depth"]):
        sub = {k[len(f"blocks.{i}."):]: v for k, v in sd.items() if k.startswith(f"blocks.{i}.")}
        x = O.mixer_layer_forward(x, sub, torch.float64).to(dtype).double()
    logits = OT.linear(x.mean(dim=1), sd["head.weight"].double(), sd["head.bias"].double())
    return plain, logits.to(dtype)
