"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for the entries that carry the MLP-Mixer family
on fp16 / bf16 activations: mi355_mixer_token_x16_fwd (csrc/mixer_fused.hip) and mi355_patch_embed_x16_fwd, mi355_token_mean_x16_fwd,
mi355_widen16_fwd, mi355_round16_fwd (csrc/gemm.hip, layernorm.hip, gemm16.hip), each in both I/O types.  The token kernel at one and at two workgroups per
image; the copies at a length with a ragged tail (n % 8 != 0); the token mean at a channel count off the 256-channel slab.

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_mixer_io16_cpu.py, tests/test_mixer_io16_arena_gpu.py); the latter runs them through the harness."""
import torch

import arena_cases
import oracle as O
from arena_cases import TOL, _gen, _rn, row

IDS = []


def _token_ref(d):
    m, x = d["m"], d["x"].double()
    u = O.layernorm(x, m.norm1.weight.double(), m.norm1.bias.double(), m.norm1.eps)
    t = m.token_mlp
    hid = O.gelu(torch.einsum("tn,bnc->btc", t.fc1.weight.double(), u) + t.fc1.bias.double()[None, :, None])
    return x + torch.einsum("nt,btc->bnc", t.fc2.weight.double(), hid) + t.fc2.bias.double()[None, :, None]


def _register():
    from mi355attn.modules import MixerLayer
    from route_cases import prep_nontrivial
    for dt, p in ((torch.float16, 1), (torch.bfloat16, 2)):
        for B, C in ((2, 256), (3, 512)):
            IDS.append(f"mixer_token16_{B}x196x{C}_p{p}")

            def make_tok(seed, B=B, C=C, dt=dt):
                torch.manual_seed(seed)
                m = MixerLayer(C, 196).eval()
                prep_nontrivial(m)
                return dict(m=m.requires_grad_(False), x=(_rn(_gen(seed), B, 196, C) * 1.3 + 0.2).to(dt))
            row(id=IDS[-1], entries=("mi355_mixer_token_x16_fwd",), prec=p, tol=TOL[p], make=make_tok, ref=_token_ref,
                run=lambda F, d: F.mixer_token_mlp16(d["x"], d["m"].norm1, d["m"].token_mlp.fc1, d["m"].token_mlp.fc2),
                tags=(f"mixer_token16_kernel<{'f16' if p == 1 else 'bf16'}>",))
        IDS.append(f"patch_embed16_2x32x8x64_p{p}")

        def make_pe(seed, dt=dt):
            g = _gen(seed)
            return dict(img=_rn(g, 2, 3, 32, 32).to(dt), w=_rn(g, 64, 3, 8, 8) / 192 ** 0.5, b=_rn(g, 64, s=0.1))
        row(id=IDS[-1], entries=("mi355_patch_embed_x16_fwd",), prec=p, tol=TOL[p], make=make_pe,
            run=lambda F, d: F.patch_embed16(d["img"], d["w"], d["b"], 8),
            ref=lambda d: O.vit_patch_embed_forward(d["img"].double(), d["w"], d["b"], torch.float64))
        IDS.append(f"token_mean16_3x49x132_p{p}")
        row(id=IDS[-1], entries=("mi355_token_mean_x16_fwd",), prec=p, tol=TOL[0], make=lambda seed, dt=dt: dict(x=_rn(_gen(seed), 3, 49, 132).to(dt)),
            run=lambda F, d: F.token_mean16(d["x"]), ref=lambda d: d["x"].double().mean(1))
        IDS.append(f"widen16_4099_p{p}")
        row(id=IDS[-1], entries=("mi355_widen16_fwd",), prec=p, tol=0.0, make=lambda seed, dt=dt: dict(x=_rn(_gen(seed), 4099, s=30.0).to(dt)),
            run=lambda F, d: F.widen16(d["x"]), ref=lambda d: d["x"].double())
        IDS.append(f"round16_4099_p{p}")
        row(id=IDS[-1], entries=("mi355_round16_fwd",), prec=p, tol=0.0, make=lambda seed: dict(x=_rn(_gen(seed), 4099, s=30.0)),
            run=lambda F, d, dt=dt: F.round16(d["x"], dt), ref=lambda d, dt=dt: d["x"].to(dt).double())
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
