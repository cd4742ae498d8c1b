"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for the two entries that carry a CSWinBlock of
the narrow stages on fp16 / bf16 activations: mi355_cswin_stripe_attn_x16_fwd (csrc/cswin_fused.hip) and mi355_proj_mlp_fused_x16_fwd
(csrc/mlp_fused.hip), each at precision 1 and 2 = in both I/O types.  The stripe entry at a ragged shape (three images of 6 x 6 tokens in
stripes of 12: the last token tile of a window and the last windows of the grid are partial) and at the two model shapes (56 x 56 x 64
in stripes of one column, 28 x 28 x 128 in stripes of two); the proj + MLP entry at M = 108 (a ragged 32-token chunk; also under
mlp_tt4 = 1, 64-token chunks) and M = 3136 at C = 64, M = 36 (a ragged step of the streaming kernel) and M = 784 at C = 128.

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_cswin_io16_cpu.py, tests/test_cswin_io16_arena_gpu.py); the latter runs them through the harness."""
import torch

import arena_cases
from arena_cases import TOL, _gen, _rn, gelu64, ln64, row

IDS = []
STRIPE_SHAPES = ((3, 6, 2, 64), (1, 56, 1, 64), (1, 28, 2, 128))                 # (B, reso, split, C)
MLP_SHAPES = ((108, 64, {}), (108, 64, dict(mlp_tt4=1)), (3136, 64, {}), (36, 128, {}), (784, 128, {}))     # (M, C, options)


def _ln(C, g):
    ln = torch.nn.LayerNorm(C)
    with torch.no_grad():
        ln.weight.copy_(0.5 + torch.rand(C, generator=g))
        ln.bias.copy_(_rn(g, C, s=0.2))
    return ln.requires_grad_(False)


def _linear(K, N, g):
    lin = torch.nn.Linear(K, N)
    with torch.no_grad():
        lin.weight.copy_(_rn(g, N, K) / K ** 0.5)
        lin.bias.copy_(_rn(g, N, s=0.1))
    return lin.requires_grad_(False)


def _getv(Cb, g):
    conv = torch.nn.Conv2d(Cb, Cb, 3, 1, 1, groups=Cb)
    with torch.no_grad():
        conv.weight.copy_(_rn(g, Cb, 1, 3, 3, s=0.3))
        conv.bias.copy_(_rn(g, Cb, s=0.1))
    return conv.requires_grad_(False)


def _register():
    from oracle.cswin import lepe_attention_forward
    for dt, p in ((torch.float16, 1), (torch.bfloat16, 2)):
        for (B, reso, split, C) in STRIPE_SHAPES:
            IDS.append(f"cswin_stripe_x16_b{B}_r{reso}_s{split}_c{C}_p{p}")

            def make_stripe(seed, B=B, reso=reso, C=C, dt=dt):
                g = _gen(seed)
                return dict(x=(_rn(g, B, reso * reso, C) * 1.3 + 0.2).to(dt), ln=_ln(C, g), qkv=_linear(C, 3 * C, g), gv0=_getv(C // 2, g),
                            gv1=_getv(C // 2, g))

            def ref_stripe(d, reso=reso, split=split, C=C):
                x = d["x"].double()
                B_, L = x.shape[:2]
                u = ln64(x, d["ln"].weight, d["ln"].bias, d["ln"].eps)
                qkv = (u @ d["qkv"].weight.double().t() + d["qkv"].bias.double()).reshape(B_, L, 3, C).permute(2, 0, 1, 3)
                h = C // 64
                a0 = lepe_attention_forward(qkv[..., :C // 2], d["gv0"].weight, d["gv0"].bias, reso, 0, split, h, torch.float64)
                a1 = lepe_attention_forward(qkv[..., C // 2:], d["gv1"].weight, d["gv1"].bias, reso, 1, split, h, torch.float64)
                return torch.cat([a0, a1], dim=2)
            row(id=IDS[-1], entries=("mi355_cswin_stripe_attn_x16_fwd",), prec=p, tol=TOL[p], make=make_stripe, ref=ref_stripe,
                run=lambda F, d, reso=reso, split=split, C=C: F.cswin_stripe_attention16(d["x"], d["ln"], d["qkv"], d["gv0"], d["gv1"], reso,
                                                                                        C // 32, split, 32 ** -0.5),
                tags=(f"cswin_stripe_kernel<C={C},x16>",))
        for (M, C, opts) in MLP_SHAPES:
            IDS.append(f"proj_mlp_fused_x16_{M}x{C}{'_tt4' if opts else ''}_p{p}")

            def make_mlp(seed, M=M, C=C, dt=dt):
                g = _gen(seed)
                return dict(x=(_rn(g, M, C) * 1.3 + 0.2).to(dt), ctx=_rn(g, M, C).to(dt), proj=_linear(C, C, g), ln=_ln(C, g),
                            fc1=_linear(C, 4 * C, g), fc2=_linear(4 * C, C, g))

            def ref_mlp(d):
                lin = lambda t, m: t @ m.weight.double().t() + m.bias.double()      # noqa: E731
                x1 = d["x"].double() + lin(d["ctx"].double(), d["proj"])
                u = ln64(x1, d["ln"].weight, d["ln"].bias, d["ln"].eps)
                return x1 + lin(gelu64(lin(u, d["fc1"])), d["fc2"])
            row(id=IDS[-1], entries=("mi355_proj_mlp_fused_x16_fwd",), prec=p, tol=TOL[p], opts=dict(opts), make=make_mlp, ref=ref_mlp,
                run=lambda F, d: F.proj_mlp_fused16(d["x"], d["ctx"], d["proj"], d["ln"], d["fc1"], d["fc2"]),
                tags=(f"mlp_fused_kernel<C={C},proj,x16>",))
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
