"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for the three LePE entries at stripe windows
above 224 tokens (win_attn_long_kernel of csrc/attn.hip): mi355_cswin_lepe_attn_fwd (fp32 I/O, precision 0 / 1 / 2),
mi355_cswin_lepe_attn16_fwd and mi355_cswin_lepe_attn16_pair_fwd (16-bit I/O, precision 1 / 2), each at T = 288 (24 x 12: the 384 px
stage-3 stripe) and T = 300 (30 x 10: no multiple of a key tile).  The single entries attend over the second channel half of a
(B, L, 3, 2 * dim) buffer and must leave the first half of `out` alone; the pair entry writes both halves.

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_lepe_long_cpu.py, tests/test_lepe_long_arena_gpu.py); the latter runs them through the harness."""
import torch

import arena_cases
import oracle as O
from arena_cases import TOL, _gen, _rn, dt16, row

IDS = []
GEOM = ((24, 12), (30, 10))            # (reso, split): T = 288 and T = 300
DIM, HEADS = 64, 2                     # per branch: two heads of width 32
LONG_TAG = "win_attn_long_kernel<d=32,lepe"
F64 = torch.float64


def _branch_ref(qkv, w, b, reso, idx, split, c0):
    """fp64 LePE attention of channels [c0, c0 + DIM) of a (B, L, 3 * Ctot) buffer -> (B, L, DIM)."""
    B, L, c3 = qkv.shape
    sl = qkv.double().reshape(B, L, 3, c3 // 3)[..., c0:c0 + DIM].permute(2, 0, 1, 3)
    return O.lepe_attention_forward(sl, w, b, reso, idx, split, HEADS, F64)


def _make(seed, reso, dt=None):
    g = _gen(seed)
    qkv = _rn(g, 2, reso * reso, 3 * 2 * DIM)
    d = dict(qkv=qkv if dt is None else qkv.to(dt))
    for i in (0, 1):
        d[f"w{i}"], d[f"b{i}"] = _rn(g, DIM, 1, 3, 3, s=0.3), _rn(g, DIM, s=0.1)
    return d


def _register():
    for reso, split in GEOM:
        gid = f"r{reso}_s{split}"
        scale = (DIM // HEADS) ** -0.5

        def single_ref(dd, reso=reso, split=split):
            B, L, c3 = dd["qkv"].shape
            out = torch.zeros(B, L, c3 // 3, dtype=F64)
            out[..., DIM:] = _branch_ref(dd["qkv"], dd["w1"], dd["b1"], reso, 1, split, DIM)
            return out

        def pair_ref(dd, reso=reso, split=split):
            return torch.cat([_branch_ref(dd["qkv"], dd[f"w{i}"], dd[f"b{i}"], reso, i, split, i * DIM) for i in (0, 1)], dim=-1)

        def run32(F, dd, p, reso=reso, split=split, scale=scale):
            B, L, c3 = dd["qkv"].shape
            out = F.torch.zeros(B, L, c3 // 3, dtype=torch.float32, device=dd["qkv"].device)
            return F.cswin_lepe_attention(dd["qkv"], dd["w1"], dd["b1"], out, reso, DIM, DIM, HEADS, split, reso, scale, precision=p)

        def run16(F, dd, p, reso=reso, split=split, scale=scale):
            B, L, c3 = dd["qkv"].shape
            out = F.torch.zeros(B, L, c3 // 3, dtype=dd["qkv"].dtype, device=dd["qkv"].device)
            return F.cswin_lepe_attention16(dd["qkv"], dd["w1"], dd["b1"], out, reso, DIM, DIM, HEADS, split, reso, scale, precision=p)

        def run_pair(F, dd, p, reso=reso, split=split, scale=scale):
            B, L, c3 = dd["qkv"].shape
            out = F.torch.zeros(B, L, c3 // 3, dtype=dd["qkv"].dtype, device=dd["qkv"].device)
            return F.cswin_lepe_attention16_pair(dd["qkv"], dd["w0"], dd["b0"], dd["w1"], dd["b1"], out, reso, HEADS, split, scale, precision=p)

        for p in (0, 1, 2):
            IDS.append(f"lepe_long_{gid}_p{p}")
            row(id=IDS[-1], entries=("mi355_cswin_lepe_attn_fwd",), prec=p, tol=TOL[p], tags=(LONG_TAG + ">",),
                make=lambda seed, reso=reso: _make(seed, reso), ref=single_ref, run=lambda F, dd, p=p, run=run32: run(F, dd, p))
        for p in (1, 2):
            make16 = lambda seed, reso=reso, p=p: _make(seed, reso, dt16(p))  # noqa: E731
            IDS.append(f"lepe16_long_{gid}_p{p}")
            row(id=IDS[-1], entries=("mi355_cswin_lepe_attn16_fwd",), prec=p, tol=TOL[p], tags=(LONG_TAG + ",io16>",), make=make16,
                ref=single_ref, run=lambda F, dd, p=p, run=run16: run(F, dd, p))
            IDS.append(f"lepe16_pair_long_{gid}_p{p}")
            row(id=IDS[-1], entries=("mi355_cswin_lepe_attn16_pair_fwd",), prec=p, tol=TOL[p], tags=(LONG_TAG + ",io16>",), make=make16,
                ref=pair_ref, run=lambda F, dd, p=p, run=run_pair: run(F, dd, p))
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
