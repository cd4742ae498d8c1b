"""GPU tests (-m gpu) of the streaming attention core, mi355_sdpa_general_fwd / sdpa_stream_kernel, through F.sdpa_general.

Inputs come from tests/sdpa_stream_cases.py (tests/test_sdpa_stream_cases_cpu.py proves on the CPU that each construction has the
property it is named for); the reference is the fp64 restatement there.  Tolerances are the suite's own (tests/test_ops_gpu.py):
strict 5e-5, fp16 operands 1e-3, bf16 operands 1.2e-2, relative Frobenius AND max-abs (conftest.assert_parity).

  a  test_index_bit_exact*      one-hot attention through a key map pi: out == v[pi] bit for bit in every operand mode, I/O type,
                                tensor layout and with out= a channel slice of a wider tensor
  b  test_parity_vs_fp64        every head width x N_kv x N_q of the table, without / with bias (shared, per image; vector and scalar
                                bias loads), fp32 and 16-bit tensors
  c  test_running_max_carry,    logits that climb / fall from key tile to key tile inside one wave; one spiked key in the first /
     test_spiked_key            the last tile
  d  test_masked_tiles,         -1e30 and -inf masks over whole key tiles (leading, middle, trailing), a fully masked row (NaN, as
     test_fully_masked_row,     torch.softmax gives it), k-NN attention with every neighbour in the last tile
     test_knn_last_tile
"""
import pytest
import torch

import sdpa_stream_cases as S
from conftest import assert_parity, max_abs_ratio, rel_fro

pytestmark = pytest.mark.gpu

TOL = {0: 5e-5, 1: 1e-3, 2: 1.2e-2}
F32 = torch.float32
MODES = [(0, F32), (1, F32), (1, torch.float16), (2, F32), (2, torch.bfloat16)]      # (precision, I/O type)
PAD = 8                                     # elements left and right of a channel slice: 16-byte aligned in fp32 and in 16 bit
SENTINEL = -7.0


def F():
    from mi355attn import functional
    return functional


def _check(out, ref, tol, what):
    out = out.float().cpu()
    if torch.isfinite(out).all():
        print(f"{what}: rel_fro={rel_fro(out, ref):.3e} max_abs_ratio={max_abs_ratio(out, ref):.3e} (tol {tol:g})")
    assert_parity(out, ref, tol, what)


# ------------------------------------------------------------------------------------------------ a. bit-exact indexing
def _place(q, k, v, layout, dt):
    """Device views of q / k / v in one of three layouts: separate dense tensors; "strided": q a channel slice of a wider tensor, k and
    v the halves of one (B, Nkv, 2C) tensor; "fused": the thirds of one (B, N, 3C) tensor (N_q == N_kv)."""
    q, k, v = (t.to(dt) for t in (q, k, v))
    C = q.shape[-1]
    if layout == "separate":
        return q.cuda(), k.cuda(), v.cuda()
    if layout == "fused":
        dev = torch.cat([q, k, v], dim=-1).cuda()
        return dev[..., :C], dev[..., C:2 * C], dev[..., 2 * C:]
    wide = torch.full((q.shape[0], q.shape[1], C + 2 * PAD), SENTINEL, dtype=dt)
    wide[..., PAD:PAD + C] = q
    kv = torch.cat([k, v], dim=-1).cuda()
    return wide.cuda()[..., PAD:PAD + C], kv[..., :C], kv[..., C:]


def _index_case(d, Nq, Nkv, layouts):
    q, k, pi = S.onehot_inputs(d, Nq, Nkv)
    C = S.HEADS * d
    for prec, dt in MODES:
        for name, v in S.value_patterns(Nkv, C, prec).items():
            want = S.expected_rows(v, pi)
            for layout in layouts:
                qd, kd, vd = _place(q, k, v, layout, dt)
                assert qd.stride(1) > C or layout == "separate"
                what = f"d={d} Nq={Nq} Nkv={Nkv} p{prec} {dt} {layout} v={name}"
                out = F().sdpa_general(qd, kd, vd, S.HEADS, S.ONEHOT_SCALE, precision=prec)
                assert out.dtype == dt
                assert torch.equal(out.float().cpu(), want), f"{what}: out != v[pi]"
                # out= a channel slice of a wider tensor (ldo > row width): the columns around it stay untouched
                wide = torch.full((S.BATCH, Nq, C + 2 * PAD), SENTINEL, dtype=dt).cuda()
                F().sdpa_general(qd, kd, vd, S.HEADS, S.ONEHOT_SCALE, precision=prec, out=wide[..., PAD:PAD + C])
                got = wide.float().cpu()
                assert torch.equal(got[..., PAD:PAD + C], want), f"{what}: out= slice != v[pi]"
                assert bool((got[..., :PAD] == SENTINEL).all()) and bool((got[..., PAD + C:] == SENTINEL).all()), \
                    f"{what}: wrote outside the out= slice"


@pytest.mark.parametrize("shape", S.SHAPES, ids=S.sid)
def test_index_bit_exact(shape):
    """Head offset head * hd, slice offset sl * DV, the row strides ldq / ldk / ldv / ldo, the key position inside a 64-key tile and
    the transposed V image are pure index math: with one-hot attention (query t of image b / head h attends key pi[b, h, t] only; the
    other probabilities underflow to exactly 0 and the row sum is exactly 1) and integer v exact in the operand type, out == v[pi]."""
    _index_case(*shape, layouts=("separate", "strided"))


@pytest.mark.parametrize("N", S.FUSED_N)
@pytest.mark.parametrize("d", S.WIDTHS)
def test_index_bit_exact_fused_qkv(d, N):
    """The same with q, k, v the three channel slices of one fused (B, N, 3C) projection and pi a permutation."""
    _index_case(d, N, N, layouts=("fused",))


# ------------------------------------------------------------------------------------------------ b. parity against fp64
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.sid)
def test_parity_vs_fp64(shape, prec):
    d, Nq, Nkv = shape
    for io in [F32] + ([S.DT16[prec]] if prec else []):
        c = S.parity_inputs(d, Nq, Nkv, io)
        qd, kd, vd = c["q"].cuda(), c["k"].cuda(), c["v"].cuda()
        for bias, ref in ((None, c["ref"]), (c["bias"].cuda(), c["ref_bias"])):
            out = F().sdpa_general(qd, kd, vd, S.HEADS, c["scale"], bias=bias, precision=prec)
            assert out.dtype == io
            _check(out, ref, TOL[prec], f"parity {S.sid(shape)} p{prec} {io} bias={'none' if bias is None else c['kind']}")


# ------------------------------------------------------------------------------------------------ c. running-max carry
def _run_all_precisions(c, what, bias=None):
    qd, kd, vd = c["q"].cuda(), c["k"].cuda(), c["v"].cuda()
    for prec in (0, 1, 2):
        out = F().sdpa_general(qd, kd, vd, S.HEADS, c["scale"], bias=None if bias is None else bias.cuda(), precision=prec)
        _check(out, c["ref"], TOL[prec], f"{what} p{prec}")


@pytest.mark.parametrize("Nq,Nkv", S.RAMP_SHAPES)
@pytest.mark.parametrize("d", S.WIDTHS)
def test_running_max_carry(d, Nq, Nkv):
    """Ramp logits: inside every 16-query wave some rows fix their max in tile 0 (alpha = 1 ever after) and others raise it at every
    tile (alpha = e^-2 .. e^-0.25), so a per-query factor applied to the wrong O row, or a stale running sum, is an O(1) error.
    A CPU model of the kernel's loop (64-key tiles, same update order, P and V rounded to the operand type) gives at most 4.3e-7 /
    4.4e-4 / 2.8e-3 for unrounded / fp16 / bf16 operands on such inputs -- a model, not a GPU measurement."""
    _run_all_precisions(S.ramp_inputs(d, Nq, Nkv), f"ramp d={d} Nq={Nq} Nkv={Nkv}")


@pytest.mark.parametrize("where", sorted(S.SPIKES))
def test_spiked_key(where):
    """One key dominates every row: in the first tile, or as the only key of the last tile (the running max jumps by ~8 at the end
    and everything accumulated so far is scaled by e^-8)."""
    _run_all_precisions(S.spike_inputs(64, 33, 321, where), f"spike {where}")


# ------------------------------------------------------------------------------------------------ d. masks
@pytest.mark.parametrize("value", sorted(S.MASK_VALUES))
@pytest.mark.parametrize("group", ["leading", "inner"])
@pytest.mark.parametrize("Nq,Nkv", S.MASK_SHAPES)
@pytest.mark.parametrize("d", S.MASK_WIDTHS)
def test_masked_tiles(d, Nq, Nkv, group, value):
    """Additive masks (-1e30 as mi355_topk_mask_fwd writes, -inf as masked_fill does) that cover whole key tiles of some rows --
    "leading": the first one, two or all-but-the-last tiles, so the running max is still -inf (or -1e30) when the first open key
    arrives; "inner": a middle tile, the ragged last tile, or both -- next to unmasked rows in the same wave."""
    c = S.mask_inputs(d, Nq, Nkv, group, value)
    _run_all_precisions(c, f"mask {group} {value} d={d} Nq={Nq} Nkv={Nkv}", bias=c["bias"])


@pytest.mark.parametrize("d", S.MASK_WIDTHS)
def test_fully_masked_row(d):
    """A row with no finite logit is NaN, as torch.softmax gives it; every other row of its wave and block still meets the tolerance."""
    Nq, Nkv = S.MASK_SHAPES[0]
    c = S.mask_inputs(d, Nq, Nkv, "inner", "minf", True)
    keep = torch.ones(S.HEADS, Nq, dtype=torch.bool)
    for h, t in S.FULL_ROWS:
        keep[h, t] = False
    per_head = lambda y: y.reshape(S.BATCH, Nq, S.HEADS, d).permute(0, 2, 1, 3)     # (B, heads, Nq, d)
    ref = per_head(c["ref"])
    assert bool(torch.isnan(ref[:, ~keep]).all()) and bool(torch.isfinite(ref[:, keep]).all())
    qd, kd, vd, bd = c["q"].cuda(), c["k"].cuda(), c["v"].cuda(), c["bias"].cuda()
    for prec in (0, 1, 2):
        out = per_head(F().sdpa_general(qd, kd, vd, S.HEADS, c["scale"], bias=bd, precision=prec).cpu())
        assert bool(torch.isnan(out[:, ~keep]).all()), f"p{prec}: a fully masked row must be NaN"
        _check(out[:, keep], ref[:, keep], TOL[prec], f"fully masked row d={d} p{prec}: the other rows")


def test_knn_last_tile():
    """k-NN attention as KNNAttention composes it (mi355_qk_logits_fwd -> mi355_topk_mask_fwd -> additive -1e30 bias) with every
    query's neighbours in the ragged last key tile: three tiles of p = 1 garbage are wiped by alpha = 0 when the last tile arrives."""
    c = S.knn_inputs()
    d, Nq, Nkv, topk = S.KNN_SHAPE
    qd, kd, vd = c["q"].cuda(), c["k"].cuda(), c["v"].cuda()
    bias = F().topk_mask_(F().qk_logits(qd, kd, S.HEADS), topk)
    assert tuple(bias.shape) == (S.BATCH, S.HEADS, Nq, Nkv)
    open_keys = (bias == 0).cpu()
    assert bool(open_keys[..., Nkv - topk:].all()) and not bool(open_keys[..., :Nkv - topk].any())
    for prec in (0, 1, 2):
        out = F().sdpa_general(qd, kd, vd, S.HEADS, c["scale"], bias=bias, precision=prec)
        _check(out, c["ref"], TOL[prec], f"knn last tile p{prec}")
