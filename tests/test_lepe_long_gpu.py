"""GPU tests (-m gpu) of the long-window LePE core: stripe windows of 225 .. 512 tokens on win_attn_long_kernel (csrc/attn.hip), through
LePEAttention, the three C entries, CSWinBlock and the 384 px CSWinTransformer, against the fp64 oracle at the bars of
tests/test_ops_gpu.py (TOL, conftest.assert_parity: rel-Frobenius and max-abs).

The shapes (tests/lepe_long_cases.py) are the smallest at which the key-blocked softmax can go wrong: one key past the short kernel's
limit, an exact multiple of every tile and block, the 384 px stage-3 stripes in both orientations, a window that is no multiple of a key
tile, and the maximum.  Operand roundings alone (q * scale, k, v and P rounded, fp64 accumulation) stay at <= 2.1e-4 / 2.8e-4 (fp16) and
<= 1.7e-3 / 3.4e-3 (bf16) of the fp64 oracle at T = 225 .. 512, so the bars leave 3 - 4 x for the kernel's fp32 accumulation.
"""
import warnings

import pytest
import torch

import lepe_long_cases as LC
import oracle as O
from conftest import assert_parity

pytestmark = pytest.mark.gpu

TOL = {0: 5e-5, 1: 1e-3, 2: 1.2e-2}
LONG, LONG16, SHORT = "win_attn_long_kernel<d=32,lepe>", "win_attn_long_kernel<d=32,lepe,io16>", "win_attn_kernel<"
STRICT_FORBIDDEN = ("gemm16", "io16", "out16", "in16", "cast16", "mlp_fused", "mlp_wide", "cswin_stripe", "mixer_token", "layernorm16_t",
                    "ln_center16")                                       # tests/test_routes_gpu.py
F64 = torch.float64
_CACHE = {}


def F():
    from mi355attn import functional
    return functional


def dt16(p):
    return torch.float16 if p == 1 else torch.bfloat16


def _traced(fn):
    """(result of fn(), kernel tags, range-fallback warnings)."""
    import mi355attn
    out = []
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            rows = mi355attn.kernel_trace(lambda: out.append(fn()))
        torch.cuda.synchronize()
    return out[0], [t for t, *_ in rows], [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning)]


def _only_long(tags, want):
    assert any(want in t for t in tags), f"no {want!r} in {tags}"
    assert not [t for t in tags if SHORT in t], f"the short kernel ran: {tags}"


def _set_precision(m, p):
    for sub in m.modules():
        if hasattr(sub, "precision"):
            sub.precision = p
    return m


def _lepe(case):
    """(state of the seeded LePEAttention, qkv, fp64 oracle) of a window, computed once."""
    if case not in _CACHE:
        from mi355attn.modules import LePEAttention
        m, qkv = LC.lepe_inputs(LePEAttention, case)
        reso, idx, split, dim, heads = case
        ref = O.lepe_attention_forward(qkv, m.get_v.weight, m.get_v.bias, reso, idx, split, heads, F64).float()
        _CACHE[case] = (LC.state(m), qkv, ref)
    return _CACHE[case]


def _module(case, prec, sd=None):
    from mi355attn.modules import LePEAttention
    reso, idx, split, dim, heads = case
    m = LePEAttention(dim, reso, idx, split_size=split, num_heads=heads, precision=prec).eval()
    if sd is not None:
        m.load_state_dict(sd)
    return m.cuda()


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("case", LC.WINDOWS, ids=LC.wid)
def test_lepe_attention_vs_oracle(case, prec):
    sd, qkv, ref = _lepe(case)
    m = _module(case, prec, sd)
    out, tags, fired = _traced(lambda: m(qkv.cuda()))
    assert not fired, fired
    _only_long(tags, LONG)
    rf, ma = assert_parity(out.cpu(), ref, TOL[prec], f"lepe {LC.wid(case)} p{prec}")
    print(f"[lepe_long] {LC.wid(case)} T={LC.tokens(case)} p{prec}: rel_fro {rf:.2e} max_abs {ma:.2e}")


def _pair_inputs(reso, split, dim, heads, B, p):
    """qkv16 (B, L, 3 * 2 * dim) in the operand type, the two branches' get_v parameters, and the fp64 oracle of the concatenated branches
    on the rounded qkv."""
    key = ("pair", reso, split, dim, p)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(reso * 100 + split)
        qkv16 = torch.randn(B, reso * reso, 3 * 2 * dim, generator=g).to(dt16(p))
        wb = [(0.3 * torch.randn(dim, 1, 3, 3, generator=g), 0.1 * torch.randn(dim, generator=g)) for _ in (0, 1)]
        q4 = qkv16.double().reshape(B, reso * reso, 3, 2 * dim)
        ref = torch.cat([O.lepe_attention_forward(q4[..., i * dim:(i + 1) * dim].permute(2, 0, 1, 3), wb[i][0], wb[i][1], reso, i, split,
                                                  heads, F64) for i in (0, 1)], dim=-1).float()
        _CACHE[key] = (qkv16, wb, ref)
    return _CACHE[key]


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("reso,split,dim,heads,B", [(24, 12, 64, 2, 2), (32, 16, 32, 1, 1)], ids=["T288", "T512"])
def test_lepe16_single_and_pair_entries_vs_oracle(reso, split, dim, heads, B, prec):
    qkv16, wb, ref = _pair_inputs(reso, split, dim, heads, B, prec)
    qd = qkv16.cuda()
    (w0, b0), (w1, b1) = [(w.cuda(), b.cuda()) for w, b in wb]
    scale = (dim // heads) ** -0.5

    def singles():
        out = torch.zeros(B, reso * reso, 2 * dim, dtype=qd.dtype, device="cuda")
        F().cswin_lepe_attention16(qd, w0, b0, out, reso, 0, dim, heads, reso, split, scale, precision=prec)
        return F().cswin_lepe_attention16(qd, w1, b1, out, reso, dim, dim, heads, split, reso, scale, precision=prec)

    def pair():
        out = torch.zeros(B, reso * reso, 2 * dim, dtype=qd.dtype, device="cuda")
        return F().cswin_lepe_attention16_pair(qd, w0, b0, w1, b1, out, reso, heads, split, scale, precision=prec)
    outs = {}
    for what, fn in (("two single calls", singles), ("pair", pair)):
        out, tags, _ = _traced(fn)
        _only_long(tags, LONG16)
        rf, ma = assert_parity(out.float().cpu(), ref, TOL[prec], f"lepe16 {what} reso {reso} split {split} p{prec}")
        print(f"[lepe_long] 16-bit I/O {what} T={reso * split} p{prec}: rel_fro {rf:.2e} max_abs {ma:.2e}")
        outs[what] = out
    assert torch.equal(outs["pair"], outs["two single calls"]), "the pair launch is not two single launches"


# ---- 2. bit-exact window index math; one-hot logits put every query's maximum in another key block ------------------------------------------
def _onehot_codes(T, d, scale=48.0):
    """q_t = scale * code(t), k_s = code(s) with +-1 bit codes: q_t.k_s is maximal only at s == t, by >= 2*scale (tests/test_ops_gpu.py)."""
    bits = max(1, (T - 1).bit_length())
    assert bits <= d
    idx = torch.arange(T)
    code = torch.zeros(T, d)
    for b in range(bits):
        code[:, b] = ((idx >> b) & 1).float() * 2 - 1
    return code * scale, code


@pytest.mark.parametrize("case", LC.WINDOWS, ids=LC.wid)
def test_window_index_bit_exact(case):
    """The construction of tests/test_ops_gpu.py::test_window_index_bit_exact: one-hot attention, LePE switched off, integer V < 2^16:
    out must equal v BIT FOR BIT.  A query's own key lies in another key block for every block of queries, so the partial sums of the
    earlier blocks must be wiped by a factor of exactly 0 and the row maximum must map to exactly 2^0."""
    reso, idx, split, dim, heads = case
    m = _module(case, 0)
    torch.nn.init.zeros_(m.get_v.weight)
    torch.nn.init.zeros_(m.get_v.bias)
    B, L, d = LC.batch(case), reso * reso, dim // heads
    T = m.H_sp * m.W_sp
    tab = O.window_token_index(reso, m.H_sp, m.W_sp)                      # (nWin, T) token ids
    qc, kc = _onehot_codes(T, d)
    q = torch.zeros(B, L, dim)
    k = torch.zeros(B, L, dim)
    for w in range(tab.shape[0]):
        for hh in range(heads):
            q[:, tab[w], hh * d:(hh + 1) * d] = qc / m.scale               # kernel pre-scales q by m.scale
            k[:, tab[w], hh * d:(hh + 1) * d] = kc
    lidx, cidx, bidx = torch.arange(L).float()[None, :, None], torch.arange(dim).float()[None, None, :], \
        torch.arange(B).float()[:, None, None]
    patterns = [lidx * 16 + cidx % 16 + bidx * 7,                 # distinguishes every token
                cidx + (lidx % 64) * 512 + bidx * 0]              # distinguishes every channel (head split / merge)
    for v in patterns:
        v = v.expand(B, L, dim).contiguous()
        assert float(v.max()) < 65536
        qkv = torch.stack([q, k, v], dim=0)
        out, tags, _ = _traced(lambda: m(qkv.cuda()))
        _only_long(tags, LONG)
        assert torch.equal(out.cpu(), v), "window / head index math is not bit-exact"


# ---- 3. late and early maximum with large gaps -------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [1, 0])
def test_late_and_early_maximum_with_large_gaps(prec):
    """randn q / k / v at T = 288; the queries in even window slots get a bonus of +60 (in units of the scaled logit) on the LAST key of
    their window -- the running maximum arrives in the last key block and everything accumulated before is rescaled by ~e^-60 --, the
    queries in odd slots get it on the FIRST key (every later block is far below the running maximum).  The bonus rides on channel 0:
    q[.., 0] = +-a by slot parity, k[.., 0] = +a on the last key, -a on the first, 0 elsewhere, scale * a * a = 60."""
    case = LC.T288
    reso, idx, split, dim, heads = case
    sd, qkv, _ = _lepe(case)
    qkv = qkv.clone()
    d = dim // heads
    a = (60.0 / d ** -0.5) ** 0.5
    tab = O.window_token_index(reso, *LC.stripe(case))
    T = tab.shape[1]
    slot = torch.arange(T)
    for w in range(tab.shape[0]):
        for hh in range(heads):
            c = hh * d
            qkv[0][:, tab[w], c] = torch.where(slot % 2 == 0, a, -a)[None, :]
            qkv[1][:, tab[w], c] = 0.0
            qkv[1][:, tab[w][T - 1], c] = a
            qkv[1][:, tab[w][0], c] = -a
    ref = O.lepe_attention_forward(qkv, sd["get_v.weight"], sd["get_v.bias"], reso, idx, split, heads, F64).float()
    m = _module(case, prec, sd)
    out, tags, fired = _traced(lambda: m(qkv.cuda()))
    assert not fired, fired
    _only_long(tags, LONG)
    assert torch.isfinite(out).all()
    rf, ma = assert_parity(out.cpu(), ref, TOL[prec], f"late / early maximum p{prec}")
    print(f"[lepe_long] late / early maximum p{prec}: rel_fro {rf:.2e} max_abs {ma:.2e}")


# ---- 4. no over-read, no over-write ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io,prec", [(32, 0), (32, 1), (32, 2), (16, 1), (16, 2)])
@pytest.mark.parametrize("case", [LC.WINDOWS[0], LC.WINDOWS[3], LC.WINDOWS[4]], ids=LC.wid)
def test_branch_slice_reads_and_writes_only_its_channels(case, io, prec):
    """The single entries on the SECOND channel half of a (B, L, 3, 2 * Cb) buffer: every q / k / v channel of the first half is NaN, `out`
    is pre-filled with a sentinel.  The slice must match the oracle and every element outside it must keep the sentinel's bits."""
    reso, idx, split, Cb, heads = case
    sd, qkv, ref = _lepe(case)                                            # qkv (3, B, L, Cb)
    B, L = qkv.shape[1], qkv.shape[2]
    hsp, wsp = LC.stripe(case)
    dt = torch.float32 if io == 32 else dt16(prec)
    buf = torch.full((B, L, 3, 2 * Cb), float("nan"))
    buf[..., Cb:] = qkv.permute(1, 2, 0, 3)
    buf = buf.to(dt)
    if io == 16:                                                          # the oracle of the rounded operands
        ref = O.lepe_attention_forward(buf[..., Cb:].permute(2, 0, 1, 3).double(), sd["get_v.weight"], sd["get_v.bias"], reso, idx, split,
                                       heads, F64).float()
    sentinel = -1234.5
    out = torch.full((B, L, 2 * Cb), sentinel, dtype=dt, device="cuda")
    fn = F().cswin_lepe_attention if io == 32 else F().cswin_lepe_attention16
    _, tags, _ = _traced(lambda: fn(buf.reshape(B, L, 6 * Cb).cuda(), sd["get_v.weight"].cuda(), sd["get_v.bias"].cuda(), out, reso, Cb, Cb,
                                    heads, hsp, wsp, (Cb // heads) ** -0.5, precision=prec))
    _only_long(tags, LONG if io == 32 else LONG16)
    got = out.cpu()
    assert_parity(got[..., Cb:].float(), ref, TOL[prec], f"slice {LC.wid(case)} io{io} p{prec}")
    keep = torch.full((B, L, Cb), sentinel, dtype=dt)
    assert torch.equal(got[..., :Cb].contiguous().view(torch.uint8), keep.view(torch.uint8)), "channels outside [c0, c0 + Cb) were written"


# ---- 5. envelope -------------------------------------------------------------------------------------------------------------------
def test_windows_above_512_tokens_are_refused_by_all_three_entries():
    import mi355attn
    reso, idx, split, dim, heads = LC.TOO_LONG                            # T = 529
    L = reso * reso
    w, b = torch.zeros(dim, 1, 3, 3, device="cuda"), torch.zeros(dim, device="cuda")
    with pytest.raises(mi355attn.Mi355Error, match="512"):
        F().cswin_lepe_attention(torch.zeros(1, L, 3 * dim, device="cuda"), w, b, torch.zeros(1, L, dim, device="cuda"), reso, 0, dim, heads,
                                 reso, reso, 32 ** -0.5, precision=0)
    for p in (1, 2):
        q16 = torch.zeros(1, L, 3 * dim, dtype=dt16(p), device="cuda")
        with pytest.raises(mi355attn.Mi355Error, match="512"):
            F().cswin_lepe_attention16(q16, w, b, torch.zeros(1, L, dim, dtype=dt16(p), device="cuda"), reso, 0, dim, heads, reso, reso,
                                       32 ** -0.5, precision=p)
        q16 = torch.zeros(1, L, 3 * 2 * dim, dtype=dt16(p), device="cuda")
        with pytest.raises(mi355attn.Mi355Error, match="512"):
            F().cswin_lepe_attention16_pair(q16, w, b, w, b, torch.zeros(1, L, 2 * dim, dtype=dt16(p), device="cuda"), reso, heads, reso,
                                            32 ** -0.5, precision=p)
    m = _module(LC.TOO_LONG, 1)
    with pytest.raises(mi355attn.Mi355Error, match="512"), torch.no_grad():
        m(torch.zeros(3, 1, L, dim, device="cuda"))
    torch.cuda.synchronize()


def test_a_224_token_window_stays_on_the_short_kernel():
    """T = 224 (56 x 4 stripes: the largest window both dividing a grid and inside the old envelope) keeps its kernel and its tag."""
    case = LC.SHORT_MAX
    reso, idx, split, dim, heads = case
    sd, qkv, ref = _lepe(case)
    for prec in (0, 1):
        out, tags, _ = _traced(lambda: _module(case, prec, sd)(qkv.cuda()))
        assert any(t.startswith("win_attn_kernel<d=32,lepe") for t in tags) and not [t for t in tags if "win_attn_long" in t], tags
        assert_parity(out.cpu(), ref, TOL[prec], f"T = 224 p{prec}")


# ---- 6. blocks ---------------------------------------------------------------------------------------------------------------------
def _block(row):
    if row[0] not in _CACHE:
        from mi355attn.modules import CSWinBlock
        m, x = LC.block_inputs(CSWinBlock, row)
        reso, heads, split = row[4]
        _CACHE[row[0]] = (LC.state(m), x, O.cswin_block_forward(x, LC.state(m), reso, heads, split, False, F64).float())
    from mi355attn.modules import CSWinBlock
    m = CSWinBlock(*row[1], **row[2]).eval()
    m.load_state_dict(_CACHE[row[0]][0])
    return (m,) + _CACHE[row[0]][1:]


@pytest.mark.parametrize("prec", [1, 0])
@pytest.mark.parametrize("row", LC.BLOCKS, ids=lambda r: r[0])
def test_block_vs_oracle(row, prec):
    m, x, ref = _block(row)
    m = _set_precision(m, prec).cuda()
    y, tags, fired = _traced(lambda: m(x.cuda()))
    assert not fired, f"range fallback fired: {fired}"
    if prec == 0:
        bad = [t for t in tags if any(s in t for s in STRICT_FORBIDDEN)]
        assert not bad, f"16-bit kernels on the strict route: {bad}"
        _only_long(tags, LONG)
    else:
        _only_long(tags, LONG16)
        if row[0].startswith("c256"):                                    # layernorm16 + qkv GEMM + LePE pair + linear16_ln16 + MLP
            for s in ("layernorm_kernel<out16>", "resid+ln16"):
                assert any(s in t for t in tags), f"no {s!r} in {tags}"
            assert sum(1 for t in tags if LONG16 in t) == 1, f"the two branches did not run as one launch: {tags}"
    rf, ma = assert_parity(y.cpu(), ref, TOL[prec], f"CSWinBlock {row[0]} p{prec}")
    print(f"[lepe_long] CSWinBlock {row[0]} p{prec}: rel_fro {rf:.2e} max_abs {ma:.2e}")


# ---- 7. model ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [1, 0])
def test_model_384_vs_oracle(prec):
    from mi355attn.modules import CSWinTransformer
    if "model" not in _CACHE:
        m, x = LC.model_inputs(CSWinTransformer)
        kw = LC.MODEL_KW
        ref = O.cswin_forward(x, LC.state(m), kw["embed_dim"], tuple(kw["depth"]), tuple(kw["split_size"]), tuple(kw["num_heads"]), F64)
        _CACHE["model"] = (LC.state(m), x, ref.float())
    sd, x, ref = _CACHE["model"]
    m = CSWinTransformer(**LC.MODEL_KW).eval()
    m.load_state_dict(sd)
    m = _set_precision(m, prec).cuda()
    y, tags, fired = _traced(lambda: m(x.cuda()))
    assert not fired, f"range fallback fired: {fired}"
    assert any("win_attn_long_kernel<d=32,lepe" in t for t in tags), tags
    rf, ma = assert_parity(y.cpu(), ref, TOL[prec], f"CSWinTransformer 384 px p{prec}")
    print(f"[lepe_long] CSWinTransformer 384 px p{prec}: rel_fro {rf:.2e} max_abs {ma:.2e}")


# ---- 8. range fallback -------------------------------------------------------------------------------------------------------------
def test_range_fallback_reruns_the_long_window_in_strict_mode():
    """The v rows of qkv.weight x 1e5 (the recipe of cswin_s1_v_1e5 in tests/test_range_guard_gpu.py) on the C = 256 block: the fp16
    forward saturates, the strict re-run must take the same 288-token windows."""
    import mi355attn
    row = LC.BLOCKS[0]
    m, x, _ = _block(row)
    with torch.no_grad():
        m.qkv.weight[2 * 256:].mul_(1e5)
    reso, heads, split = row[4]
    ref = O.cswin_block_forward(x, LC.state(m), reso, heads, split, False, F64).float()
    assert torch.isfinite(ref).all()
    m = _set_precision(m, 1).cuda()
    assert mi355attn.get_option("range_fallback") == 1
    mi355attn.range_status(wait=True)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            y = m(x.cuda())
        torch.cuda.synchronize()
    hits = [w for w in rec if issubclass(w.category, RuntimeWarning)]
    assert len(hits) == 1 and "strict" in str(hits[0].message), [str(w.message) for w in rec]
    assert torch.isfinite(y).all()
    rf, ma = assert_parity(y.cpu(), ref, TOL[0], "strict re-run of the C = 256 block")
    print(f"[lepe_long] range fallback re-run: rel_fro {rf:.2e} max_abs {ma:.2e}")
    mi355attn.range_status(wait=True)                                    # clean: nothing left pending for the next caller


# ---- 9. graph capture --------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One fp16 forward of the C = 256 block captured on a single stream and replayed twice equals the eager result."""
    import mi355attn
    m, x, _ = _block(LC.BLOCKS[0])
    m = _set_precision(m, 1).cuda()
    static_x = x.cuda()
    with torch.no_grad():
        want = m(static_x).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        m(static_x)                                                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = m(static_x)
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), f"replay {rep} differs from the eager result"
        out.zero_()
    mi355attn.range_status(wait=True)
