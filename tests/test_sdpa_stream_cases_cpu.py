"""CPU guard of tests/sdpa_stream_cases.py: each input construction of the streaming-attention GPU tests has the property it is named
for, shown with the fp64 reference alone.  A construction that quietly lost its property (a one-hot row that is not one-hot, a ramp
whose running max never moves, a "leading tile masked" row with a key left open) would make the GPU test pass for the wrong reason.
"""
import math

import pytest
import torch

import sdpa_stream_cases as S

ONEHOT_SHAPES = S.SHAPES + [(d, n, n) for d in S.WIDTHS for n in S.FUSED_N]


def test_shape_table_covers_the_axes():
    assert {(d, nkv) for d, _, nkv in S.SHAPES} == {(d, nkv) for d in S.WIDTHS for nkv in S.NKV}
    assert {(d, nq) for d, nq, _ in S.SHAPES} == {(d, nq) for d in S.WIDTHS for nq in S.NQ}
    for d in S.WIDTHS:                      # shared and per-image bias on the vector (N_kv % 4 == 0) and the scalar bias load path
        assert {(S.bias_kind(d, nkv), nkv % 4 == 0) for nkv in S.NKV} == {(k, vec) for k in S.BIAS_KINDS for vec in (True, False)}


@pytest.mark.parametrize("shape", ONEHOT_SHAPES, ids=S.sid)
def test_onehot_rows_are_one_hot(shape):
    d, Nq, Nkv = shape
    q, k, pi = S.onehot_inputs(d, Nq, Nkv)
    att = S.logits64(q, k, S.HEADS, S.ONEHOT_SCALE)                         # (B, heads, Nq, Nkv)
    top2 = att.topk(min(2, Nkv), dim=-1)
    assert torch.equal(top2.indices[..., 0], pi), "the designated key is not the argmax"
    if Nkv > 1:
        margin = float((top2.values[..., 0] - top2.values[..., 1]).min())
        assert margin >= S.onehot_margin(Nkv, d) >= 96.0                  # exp(-96) < 2^-138
    p = torch.softmax(att, dim=-1)
    onehot = torch.zeros_like(p).scatter_(-1, pi[..., None], 1.0)
    assert float((p - onehot).abs().max()) <= 2.0 ** -100
    for mode in (0, 1, 2):
        assert S.roundtrips(q, mode) and S.roundtrips(k, mode)
    for b in range(S.BATCH):                                                # every (image, head) selects differently
        for h in range(S.HEADS):
            others = [pi[bb, hh] for bb in range(S.BATCH) for hh in range(S.HEADS) if (bb, hh) != (b, h)]
            assert all(not torch.equal(pi[b, h], o) for o in others) or Nkv == 1
    ntiles = (Nkv + S.KTILE - 1) // S.KTILE
    assert int(pi[0, 0, 0]) == Nkv - 1                                      # the last key (a 1-key tile at N_kv = 65 / 321) is attended
    if Nq >= 17:                                                            # pi spreads over the key tiles: all of them are hit, and
        assert set((pi // S.KTILE).flatten().tolist()) == set(range(ntiles))                          # every (image, head) hits several
        assert all(len(set((pi[b, h] // S.KTILE).tolist())) >= min(ntiles - 1, 3) for b in range(S.BATCH) for h in range(S.HEADS))
    if Nq == Nkv:
        assert all(sorted(pi[b, h].tolist()) == list(range(Nkv)) and not torch.equal(pi[b, h], torch.arange(Nkv))
                   for b in range(S.BATCH) for h in range(S.HEADS)), "fused case: pi must be a non-trivial permutation"


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_value_patterns_are_exact_and_tell_everything_apart(mode):
    Nkv, C = max(S.NKV), S.HEADS * max(S.WIDTHS)
    pats = S.value_patterns(Nkv, C, mode)
    for name, v in pats.items():
        assert float(v.max()) < S.V_BOUND[mode] and float(v.min()) >= 0 and torch.equal(v, v.round())
        assert S.roundtrips(v, mode), f"{name}: not exact in the operand type of precision {mode}"
        if name != "mix":                                                   # the small patterns are exact in every type
            assert all(S.roundtrips(v, m) for m in (0, 1, 2))
    sig = torch.stack([pats[n] for n in ("mix", "key", "chan")], dim=-1)    # (B, Nkv, C, 3): the signature of one v element
    assert len(torch.unique(sig.reshape(-1, 3), dim=0)) == S.BATCH * Nkv * C, "two (image, key, channel) positions look alike"


@pytest.mark.parametrize("d", S.WIDTHS)
@pytest.mark.parametrize("Nq,Nkv", S.RAMP_SHAPES)
def test_ramp_moves_the_running_max(d, Nq, Nkv):
    c = S.ramp_inputs(d, Nq, Nkv)
    assert all(S.roundtrips(c[n], m) for n in ("q", "k") for m in (0, 1, 2))
    assert float(c["q"].abs().max()) * 8 < 256 and float(c["k"].abs().max()) * 8 < 256      # 8 significant bits on the 1/8 grid
    for t in (c["q"], c["k"]):
        assert torch.equal(t * 8, (t * 8).round())
    att = S.logits64(c["q"], c["k"], S.HEADS, c["scale"])
    tile = att.argmax(dim=-1) // S.KTILE                                    # (B, heads, Nq)
    last = (Nkv - 1) // S.KTILE
    assert Nkv > 128
    for b in range(S.BATCH):
        for h in range(S.HEADS):
            seen = set(tile[b, h].tolist())
            assert len(seen) >= 3 and 0 in seen and last in seen
            first16 = set(tile[b, h, :16].tolist())                         # inside ONE 16-query wave
            assert 0 in first16 and last in first16
    # the carry: some row's running max rises at every tile, another's never after tile 0
    tmax = torch.stack([att[..., j * S.KTILE:(j + 1) * S.KTILE].amax(dim=-1) for j in range(last + 1)], dim=-1)
    rising = (tmax[..., 1:] > tmax[..., :-1].cummax(dim=-1).values).all(dim=-1)
    pinned = (tmax[..., 1:] < tmax[..., :1]).all(dim=-1)
    assert bool(rising[..., :16].any(dim=-1).all()) and bool(pinned[..., :16].any(dim=-1).all())


@pytest.mark.parametrize("where", sorted(S.SPIKES))
def test_spike_dominates_its_row(where):
    c = S.spike_inputs(64, 33, 321, where)
    att = S.logits64(c["q"], c["k"], S.HEADS, c["scale"])
    top2 = att.topk(2, dim=-1)
    assert bool((top2.indices[..., 0] == c["key"]).all())
    assert float((top2.values[..., 0] - top2.values[..., 1]).min()) > 4.0
    assert c["key"] // S.KTILE == (0 if where == "first" else (321 - 1) // S.KTILE)


def _masked(bias):
    return bias <= -1e29


@pytest.mark.parametrize("value", sorted(S.MASK_VALUES))
@pytest.mark.parametrize("group", ["leading", "inner"])
@pytest.mark.parametrize("Nq,Nkv", S.MASK_SHAPES)
def test_mask_rows_have_their_property(Nq, Nkv, group, value):
    for full_rows in (False, True):
        if full_rows and (group, value, Nq) != ("inner", "minf", 70):
            continue
        c = S.mask_inputs(64, Nq, Nkv, group, value, full_rows)
        m = _masked(c["bias"])
        assert bool((c["bias"][m] == S.MASK_VALUES[value]).all()) and bool(torch.isfinite(c["bias"][~m]).all())
        tile = torch.arange(Nkv) // S.KTILE
        last = (Nkv - 1) // S.KTILE
        per_tile = torch.stack([m[..., tile == j].all(dim=-1) for j in range(last + 1)], dim=-1)      # (heads, Nq, tiles): tile fully masked
        want = {"none": [], "lead1": [0], "lead2": [0, 1], "leadall": list(range(last)), "mid": [1], "trail": [last],
                "midtrail": [1, last]}
        for kind, rows in c["rows"].items():
            for h, t in rows:
                if kind == "full":
                    assert bool(m[h, t].all())
                    continue
                assert not bool(m[h, t].all()), "a row outside FULL_ROWS lost every key"
                if kind == "rand":
                    assert 0 < int(m[h, t].sum()) < Nkv
                else:
                    assert per_tile[h, t].nonzero().flatten().tolist() == want[kind], (kind, h, t)
        assert set(c["rows"].get("full", [])) == (set(S.FULL_ROWS) if full_rows else set())
        kinds = set(c["rows"])
        assert kinds >= ({"none", "lead1", "lead2", "leadall", "rand"} if group == "leading" else {"none", "mid", "trail", "midtrail", "rand"})
        for h in range(S.HEADS):                                             # every 16-query wave mixes masked and unmasked rows
            for t0 in range(0, Nq - 15, 16):
                wave = {k for k, rows in c["rows"].items() for hh, t in rows if hh == h and t0 <= t < t0 + 16}
                assert "none" in wave and len(wave) >= 4
        ref = c["ref"]
        bad = torch.isnan(ref).any(dim=-1)                                  # (B, Nq): NaN exactly in the columns of a fully masked (head, row)
        assert bool(torch.isfinite(ref[~bad]).all())
        if full_rows:
            d = 64
            for h, t in S.FULL_ROWS:
                assert bool(torch.isnan(ref[:, t, h * d:(h + 1) * d]).all())
            keep = torch.ones(S.HEADS, Nq, dtype=torch.bool)
            for h, t in S.FULL_ROWS:
                keep[h, t] = False
            per_head = ref.reshape(S.BATCH, Nq, S.HEADS, d).permute(0, 2, 1, 3)
            assert bool(torch.isfinite(per_head[:, keep]).all())
        else:
            assert not bool(bad.any())


def test_knn_neighbours_all_sit_in_the_last_tile():
    c = S.knn_inputs()
    d, Nq, Nkv, topk = S.KNN_SHAPE
    att = c["logits"]
    assert bool((att[..., 1:] > att[..., :-1]).all()), "logits must grow strictly with the key index"
    idx = att.topk(topk, dim=-1).indices
    assert int(idx.min()) == Nkv - topk and (Nkv - topk) // S.KTILE == (Nkv - 1) // S.KTILE >= 2
    raw = S.logits64(c["q"], c["k"], S.HEADS, 1.0)                          # what mi355_qk_logits_fwd computes: exact in fp32
    assert torch.equal(raw.float().double(), raw)
    assert bool(torch.isfinite(c["ref"]).all())
    assert math.isclose(c["scale"], d ** -0.5)
