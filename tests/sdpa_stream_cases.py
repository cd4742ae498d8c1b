"""Inputs of the streaming attention core's op-level tests (tests/test_sdpa_stream_cases_cpu.py, tests/test_sdpa_stream_gpu.py).

mi355_sdpa_general_fwd (csrc/sdpa_general.hip, sdpa_stream_kernel) streams 64-key tiles through an online softmax; head widths above
64 cut the value / output columns into 64-wide slices.  Four constructions, each aimed at one way such a kernel goes wrong:

  one-hot   query t attends exactly key pi(t): the output is v[pi] BIT FOR BIT, so head / slice / stride / key-position arithmetic is
            checked exactly (onehot_inputs, value_patterns, expected_rows)
  parity    randn inputs, optional additive bias (shared / per image, N_kv % 4 == 0 -> vector loads, else scalar loads), fp32 and
            16-bit tensors (parity_inputs)
  ramp      logits that grow, shrink or stay level from key tile to key tile, per query: the running max / sum / O rescaling of the
            online softmax is exercised with alpha = 1 and alpha << 1 inside one wave (ramp_inputs, spike_inputs)
  masks     additive -1e30 / -inf masks covering whole key tiles of some rows (mask_inputs), k-NN attention whose neighbours all sit in
            the last tile (knn_inputs)

The CPU test proves, with the fp64 reference alone, that each construction has the property it is named for.  Everything is built on
the CPU from fixed seeds; builders are cached, the tests must not modify what they return.
"""
import functools
import math

import torch

BATCH, HEADS = 2, 2                         # heads = 2: the head offset head * hd is non-zero
KTILE = 64                                  # keys per streamed tile (csrc/sdpa_general.hip)
WIDTHS = (32, 64, 128, 192, 256)            # head widths the kernel is built for; above 64 the DV != D path (64-wide slices)
NQ = (1, 17, 70, 130)                       # partial wave, partial block, more than one block
NKV = (5, 20, 40, 64, 65, 200, 321)         # part of the first 16-key sub-tile, partial second sub-tile, half a P.V group, exactly one
                                            # tile, one key in the second tile, ragged last tile, six tiles with a 1-key last tile
# Covering subset of the product: every width meets every N_kv, and (7 N_kv values against a rotation of period 4) every N_q.
SHAPES = [(d, NQ[(i + j) % len(NQ)], nkv) for i, d in enumerate(WIDTHS) for j, nkv in enumerate(NKV)]
FUSED_N = (65, 200)                         # N_q == N_kv: q / k / v as slices of one fused (B, N, 3C) tensor
DT16 = {1: torch.float16, 2: torch.bfloat16}


def sid(shape):
    return "d%d_q%d_kv%d" % tuple(shape)


def heads_view(t, h):
    B, N, C = t.shape
    return t.reshape(B, N, h, C // h).permute(0, 2, 1, 3)


def sdpa64(q, k, v, h, scale, bias=None):
    """fp64 softmax(q k^T * scale + bias) v on (B, N, C) tensors; bias (h, Nq, Nkv) or (B, h, Nq, Nkv)."""
    att = heads_view(q.double(), h) @ heads_view(k.double(), h).transpose(-1, -2) * scale
    if bias is not None:
        att = att + bias.double()
    return (torch.softmax(att, dim=-1) @ heads_view(v.double(), h)).transpose(1, 2).reshape(q.shape)


def logits64(q, k, h, scale, bias=None):
    att = heads_view(q.double(), h) @ heads_view(k.double(), h).transpose(-1, -2) * scale
    return att if bias is None else att + bias.double()


def roundtrips(t, mode):
    """Whether every value of fp32 tensor t survives the operand format of a precision mode: 0 split-bf16 (hi + lo), 1 fp16, 2 bf16."""
    if mode == 0:
        hi = t.to(torch.bfloat16).float()
        lo = (t - hi).to(torch.bfloat16).float()
        return torch.equal(hi + lo, t)
    return torch.equal(t.to(DT16[mode]).float(), t)


# ------------------------------------------------------------------------------------------------------------------------ one-hot
ONEHOT_SCALE = 0.125                        # exact power of two: q = amp * code / scale stays exact in bf16
ONEHOT_AMP = 48.0


def onehot_bits(T):
    return max(1, (T - 1).bit_length())


def onehot_codes(T, d, amp=ONEHOT_AMP):
    """test_ops_gpu._onehot_codes spread over the whole head width: channel c carries bit c % bits of the +-1 code, so every
    32-channel k-step of the logit contraction takes part.  q_t = amp * code(t), k_s = code(s): q_t . k_s is maximal only at s == t,
    by at least onehot_margin (every differing bit occupies at least d // bits channels and costs 2 * amp on each)."""
    bits = onehot_bits(T)
    assert bits <= d
    ch = torch.arange(d) % bits
    code = ((torch.arange(T)[:, None] >> ch[None, :]) & 1).float() * 2 - 1
    return code * amp, code


def onehot_margin(T, d, amp=ONEHOT_AMP):
    return 2 * amp * (d // onehot_bits(T))


def spread_map(Nq, Nkv, b, h):
    """pi(t): a stride near the golden ratio of N_kv (coprime to it) walks over all key tiles within a few queries; t = 0 of
    image 0 / head 0 lands on the last key; every (image, head) has its own offset (a quarter of N_kv apart), so q / k rows of the
    wrong image or head select other keys."""
    stride = max(1, round(Nkv * 0.618))
    while math.gcd(stride, Nkv) != 1:
        stride += 1
    return (torch.arange(Nq) * stride + Nkv - 1 + (2 * b + h) * max(1, Nkv // 4)) % Nkv


@functools.lru_cache(maxsize=None)
def onehot_inputs(d, Nq, Nkv):
    """q (B, Nq, C), k (B, Nkv, C) fp32 and pi (B, heads, Nq): query t of (image b, head h) attends key pi[b, h, t] only."""
    qc, kc = onehot_codes(Nkv, d)
    C = HEADS * d
    q, k = torch.zeros(BATCH, Nq, C), torch.zeros(BATCH, Nkv, C)
    pi = torch.zeros(BATCH, HEADS, Nq, dtype=torch.long)
    for b in range(BATCH):
        for h in range(HEADS):
            pi[b, h] = spread_map(Nq, Nkv, b, h)
            q[b, :, h * d:(h + 1) * d] = qc[pi[b, h]] / ONEHOT_SCALE
            k[b, :, h * d:(h + 1) * d] = kc
    return q, k, pi


V_BOUND = {0: 65536, 1: 2048, 2: 256}       # integers below these are exact in split-bf16 (16 bits) / fp16 (11 bits) / bf16 (8 bits)
V_PRIME = {0: 65521, 1: 2039, 2: 251}       # largest prime below the bound


def value_patterns(Nkv, C, mode):
    """Integer v patterns (B, Nkv, C), exact in the operand type of precision `mode` (and, for modes 1 / 2, in the 16-bit I/O type).
    Together they tell apart every key, every channel (hence every slice and head) and every image:
      mix    (s * C + c + 7 b) mod p: neighbouring keys, neighbouring channels and the images differ; uses the type's full integer range
      key    s // 2 + b: keys at ANY distance differ (the pair s, s ^ 1 is told apart by `mix`)
      chan   c // 2: channels at any distance differ (the pair by `mix`)"""
    s = torch.arange(Nkv, dtype=torch.long)[None, :, None]
    c = torch.arange(C, dtype=torch.long)[None, None, :]
    b = torch.arange(BATCH, dtype=torch.long)[:, None, None]
    pats = {"mix": (s * C + c + 7 * b) % V_PRIME[mode], "key": s // 2 + b + 0 * c, "chan": c // 2 + 0 * b + 0 * s}
    out = {}
    for name, p in pats.items():
        assert int(p.max()) < V_BOUND[2] or name == "mix"
        out[name] = p.expand(BATCH, Nkv, C).float().contiguous()
    return out


def expected_rows(v, pi):
    """out[b, t, head h's columns] = v[b, pi[b, h, t], head h's columns]."""
    B, h, Nq = pi.shape
    d = v.shape[2] // h
    out = torch.empty(B, Nq, v.shape[2], dtype=v.dtype)
    for b in range(B):
        for hh in range(h):
            out[b, :, hh * d:(hh + 1) * d] = v[b, pi[b, hh], hh * d:(hh + 1) * d]
    return out


# ------------------------------------------------------------------------------------------------------------------------ parity
BIAS_KINDS = ("shared", "batched")


def bias_kind(d, Nkv):
    """Rotation under which every width meets shared and per-image bias on both load paths (N_kv % 4 == 0 and != 0)."""
    return BIAS_KINDS[(WIDTHS.index(d) + NKV.index(Nkv) // 2) % 2]


@functools.lru_cache(maxsize=None)
def parity_inputs(d, Nq, Nkv, io):
    """randn q / k / v rounded to the I/O type `io` (torch.float32 / float16 / bfloat16), an fp32 randn bias of this shape's kind,
    and the fp64 results without and with the bias (computed from the rounded tensors)."""
    g = torch.Generator().manual_seed(1000 * d + 10 * Nq + Nkv)
    C = HEADS * d
    q, k, v = (torch.randn(BATCH, n, C, generator=g).to(io) for n in (Nq, Nkv, Nkv))
    kind = bias_kind(d, Nkv)
    bias = torch.randn(*((BATCH,) if kind == "batched" else ()), HEADS, Nq, Nkv, generator=g)
    scale = d ** -0.5
    return dict(q=q, k=k, v=v, bias=bias, kind=kind, scale=scale,
                ref=sdpa64(q, k, v, HEADS, scale).float(), ref_bias=sdpa64(q, k, v, HEADS, scale, bias).float())


# ------------------------------------------------------------------------------------------------------------------------ ramp
SLOPES = (-4.0, -1.0, 0.0, 1.0, 4.0, 2.0, -2.0, 0.5)      # logit change per key tile is slope / 2
RAMP_SHAPES = ((70, 200), (33, 321))


def grid8(x):
    return torch.round(torch.as_tensor(x, dtype=torch.float32) * 8) / 8


def ramp_channel(d):
    return d - 3                              # inside the last 32-channel k-step of every width


def _grid_qkv(d, Nq, Nkv, g):
    C = HEADS * d
    q = torch.randint(-8, 9, (BATCH, Nq, C), generator=g).float() / 8
    k = torch.randint(-8, 9, (BATCH, Nkv, C), generator=g).float() / 8
    return q, k, torch.randn(BATCH, Nkv, C, generator=g)


@functools.lru_cache(maxsize=None)
def ramp_inputs(d, Nq, Nkv):
    """q, k on the 1/8 grid in [-1, 1] (exact in fp16 and bf16; their products and sums are exact in fp32, so the logits are the same
    in every operand mode), v randn.  In one channel per head k carries 2 * (key // 64) and query t carries SLOPES[(t + 3h + b) % 8] /
    (4 * scale) rounded to the grid: its logits move by slope / 2 per key tile.  Slope -4 pins the running max in tile 0 (alpha = 1
    from then on), slope +4 raises it by 2 at every tile (alpha = e^-2), and both kinds sit in every 16-query wave."""
    g = torch.Generator().manual_seed(77 * d + Nq + Nkv)
    q, k, v = _grid_qkv(d, Nq, Nkv, g)
    scale = d ** -0.5
    t = torch.arange(Nq)
    for b in range(BATCH):
        for h in range(HEADS):
            r = h * d + ramp_channel(d)
            k[b, :, r] = 2.0 * (torch.arange(Nkv) // KTILE)
            q[b, :, r] = grid8(torch.tensor(SLOPES)[(t + 3 * h + b) % len(SLOPES)] / (4 * scale))
    return dict(q=q, k=k, v=v, scale=scale, ref=sdpa64(q, k, v, HEADS, scale).float())


SPIKES = {"first": 3, "last": -1}             # key index of the spike


@functools.lru_cache(maxsize=None)
def spike_inputs(d, Nq, Nkv, where):
    """Grid q / k, v randn, and ONE key per (image, head) whose logit stands about 8 above all others for every query: in the first
    tile (the running max never moves again) or the very last key (it jumps at the last, 1-key tile)."""
    g = torch.Generator().manual_seed(91 * d + Nq + Nkv + len(where))
    q, k, v = _grid_qkv(d, Nq, Nkv, g)
    scale = d ** -0.5
    key = SPIKES[where] % Nkv
    for h in range(HEADS):
        r = h * d + ramp_channel(d)
        k[:, :, r] = 0.0
        k[:, key, r] = 8.0
        q[:, :, r] = grid8(1.0 / scale)
    return dict(q=q, k=k, v=v, scale=scale, key=key, ref=sdpa64(q, k, v, HEADS, scale).float())


# ------------------------------------------------------------------------------------------------------------------------ masks
MASK_SHAPES = ((70, 200), (17, 321))          # four tiles with a ragged 8-key tail; six tiles with a 1-key tail
MASK_WIDTHS = (64, 192)
MASK_VALUES = {"m1e30": -1e30, "minf": -math.inf}
# Row t of head h is of kind KINDS[(t + h) % len]: every 16-query wave holds every kind next to unmasked rows.
LEADING_KINDS = ("none", "lead1", "none", "lead2", "rand", "lead1", "leadall", "none")
INNER_KINDS = ("none", "mid", "none", "trail", "rand", "mid", "midtrail", "none")
FULL_ROWS = ((0, 5), (1, 37))                 # (head, query) rows with every key masked (-inf only)


def masked_keys(kind, Nkv, g):
    """Boolean (Nkv): the keys kind masks.  lead1 / lead2: the first one / two tiles; leadall: every tile but the last; mid: tile 1;
    trail: the last (ragged) tile; midtrail: both; rand: a random half that keeps key 0; full: all."""
    key = torch.arange(Nkv)
    tile, last = key // KTILE, (Nkv - 1) // KTILE
    assert last >= 2
    if kind == "none":
        return torch.zeros(Nkv, dtype=torch.bool)
    if kind == "rand":
        m = torch.rand(Nkv, generator=g) < 0.5
        m[0] = False
        return m
    return {"lead1": tile < 1, "lead2": tile < 2, "leadall": tile < last, "mid": tile == 1, "trail": tile == last,
            "midtrail": (tile == 1) | (tile == last), "full": key >= 0}[kind]


@functools.lru_cache(maxsize=None)
def mask_inputs(d, Nq, Nkv, group, value, full_rows=False):
    """randn q / k / v, a shared (heads, Nq, Nkv) bias = 0.5 * randn with MASK_VALUES[value] on the masked keys of every row, the
    rows of each kind as (head, query) pairs, and the fp64 result with the same bias.  group: "leading" / "inner"."""
    kinds = {"leading": LEADING_KINDS, "inner": INNER_KINDS}[group]
    g = torch.Generator().manual_seed(13 * d + Nq + Nkv + len(group))
    C = HEADS * d
    q, k, v = (torch.randn(BATCH, n, C, generator=g) for n in (Nq, Nkv, Nkv))
    bias = 0.5 * torch.randn(HEADS, Nq, Nkv, generator=g)
    rows = {}
    for h in range(HEADS):
        for t in range(Nq):
            kind = "full" if full_rows and (h, t) in FULL_ROWS else kinds[(t + h) % len(kinds)]
            bias[h, t, masked_keys(kind, Nkv, g)] = MASK_VALUES[value]
            rows.setdefault(kind, []).append((h, t))
    scale = d ** -0.5
    return dict(q=q, k=k, v=v, bias=bias, rows=rows, scale=scale, ref=sdpa64(q, k, v, HEADS, scale, bias).float())


KNN_SHAPE = (64, 70, 200, 5)                  # d, Nq, Nkv, top-k: all five neighbours in the ragged last tile (keys 192 .. 199)


@functools.lru_cache(maxsize=None)
def knn_inputs():
    """k-NN attention (kvt.py:83-89) whose logits grow with the key index: k carries key / 8 in one channel per head and 0 elsewhere,
    the query a positive factor there (1 .. 4 times round(1 / scale)), so the top 5 of every row are the last five keys and differ by
    scale * q / 8 from neighbour to neighbour.  ref: fp64 top-k attention (the others at -inf)."""
    d, Nq, Nkv, topk = KNN_SHAPE
    g = torch.Generator().manual_seed(5)
    q, k, v = _grid_qkv(d, Nq, Nkv, g)
    scale = d ** -0.5
    k.zero_()
    for h in range(HEADS):
        r = h * d + ramp_channel(d)
        k[:, :, r] = torch.arange(Nkv).float() / 8
        q[:, :, r] = grid8(1.0 / scale) * (1 + (torch.arange(Nq) + h) % 4).float()
    att = logits64(q, k, HEADS, scale)
    kth = att.topk(topk, dim=-1).values[..., -1:]
    mask = torch.where(att >= kth, 0.0, -math.inf)
    return dict(q=q, k=k, v=v, scale=scale, topk=topk, logits=att, ref=sdpa64(q, k, v, HEADS, scale, mask).float())
