"""GPU tests (-m gpu): SKLayer on every planes / groups -- the matrix-core branch kernel behind mi355_sk_fwd (csrc/sk_wide.hip).

Reference: the fp64 oracle (oracle.axis_attn.sk_forward) through conftest.assert_parity at 5e-5, the project's strict-mode bar
(TOL[0] of tests/arena_cases.py): the branches run in the fp32-class split-bf16 operand format.  A CPU emulation of the
hi.hi + hi.lo + lo.hi products on the rows of tests/sk_wide_cases.py gives 1.7e-6 .. 3.5e-6 rel-Frobenius and 2.1e-6 .. 5.8e-6
max-abs ratio; the reference's own fp32 evaluation about 2e-7.  Before the kernel existed every row of CASES raised Mi355Error
("planes / groups = ... not in {1,2,4,8,16}")."""
import ctypes
import re

import pytest
import torch

import sk_wide_cases as S
from conftest import assert_parity, max_abs_ratio, rel_fro
from io16_common import _status

pytestmark = pytest.mark.gpu


def _trace(fn):
    import mi355attn
    out = []
    with torch.no_grad():
        rows = mi355attn.kernel_trace(lambda: out.append(fn()))
    return out[0], [tag for tag, *_ in rows]


def _wide_tags(tags):
    return [t for t in tags if t.startswith(S.WIDE_TAG)]


def _field(tag, key):
    return int(re.search(r"\b%s=(\d+)" % key, tag).group(1))


def _forward(case, sk_wide=None):
    import mi355attn
    m, x = S.module(case).cuda(), S.input_of(case).cuda()
    with torch.no_grad():
        if sk_wide is None:
            return m(x)
        with mi355attn.options(sk_wide=sk_wide):
            return m(x)


# ---- parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", S.IDS)
def test_parity_against_fp64(cid):
    case = S.BY_ID[cid]
    m, x = S.module(case).cuda(), S.input_of(case).cuda()
    y, tags = _trace(lambda: m(x))                                     # Mi355Error without the kernel
    wide = _wide_tags(tags)
    assert len(wide) == 1, tags
    (Cin, planes), groups, (_, _, H, W) = case[1], case[2], case[3]
    assert (_field(wide[0], "cog"), _field(wide[0], "cin"), _field(wide[0], "H"), _field(wide[0], "W")) == (planes // groups, Cin // groups, H, W)
    if cid == "chunked_512":
        assert _field(wide[0], "chunks") >= 2, wide[0]
    if cid == "three_bands":
        bands = _field(wide[0], "bands")
        assert bands >= 3 and H % ((H + bands - 1) // bands) != 0, wide[0]
    if cid == "col_bands_chunk_tail":
        assert _field(wide[0], "bands") >= 2 and _field(wide[0], "chunks") >= 2, wide[0]
    ref = S.truth(case)
    print(f"[sk_wide] {cid}: rel_fro {rel_fro(y, ref):.2e} max-abs ratio {max_abs_ratio(y, ref):.2e} (bar {S.TOL:g})  {wide[0]}")
    assert y.dtype == torch.float32
    assert_parity(y.cpu(), ref, S.TOL, f"SKLayer {cid}")
    _status()


@pytest.mark.parametrize("cid", S.COVERED_IDS)
def test_new_kernel_on_old_shapes(cid):
    """options(sk_wide=1): the shapes the FMA kernels cover run on the matrix-core kernel and meet the same bar."""
    import mi355attn
    case = S.BY_ID[cid]
    m, x = S.module(case).cuda(), S.input_of(case).cuda()
    with mi355attn.options(sk_wide=1):
        y, tags = _trace(lambda: m(x))
    assert len(_wide_tags(tags)) == 1 and not [t for t in tags if t.startswith("sk_branch")], tags
    ref = S.truth(case)
    print(f"[sk_wide] {cid} sk_wide=1: rel_fro {rel_fro(y, ref):.2e} max-abs ratio {max_abs_ratio(y, ref):.2e} (bar {S.TOL:g})")
    assert_parity(y.cpu(), ref, S.TOL, f"SKLayer {cid} sk_wide=1")
    _status()


@pytest.mark.parametrize("cid", S.COVERED_IDS)
def test_old_path_untouched_by_default(cid):
    """Default option: the covered shapes launch no sk_wide kernel (neither the pack nor the main one) and keep their FMA kernel."""
    import mi355attn
    assert mi355attn.get_option("sk_wide") == 0
    case = S.BY_ID[cid]
    m, x = S.module(case).cuda(), S.input_of(case).cuda()
    y, tags = _trace(lambda: m(x))
    assert not [t for t in tags if "sk_wide" in t], tags
    assert len([t for t in tags if t.startswith("sk_branch")]) == 1, tags
    assert_parity(y.cpu(), S.truth(case), 3e-5, f"SKLayer {cid} default route")     # CHAIN of tests/arena_cases.py: the bar of its sk rows
    _status()


# ---- determinism and state ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["g32x32_tiles", "three_bands", "chunked_512"])
def test_two_forwards_give_the_same_bits(cid):
    case = S.BY_ID[cid]
    a, b = _forward(case), _forward(case)
    assert torch.equal(a, b)
    _status()


@pytest.mark.parametrize("cid", S.COVERED_IDS)
def test_a_wide_forward_between_two_default_forwards_leaves_their_bits(cid):
    case = S.BY_ID[cid]
    first = _forward(case)
    wide = _forward(case, sk_wide=1)
    second = _forward(case)
    assert torch.equal(first, second)
    assert torch.equal(wide, _forward(case, sk_wide=1))
    _status()


def test_graph_capture_and_replay():
    """One forward of the 32 x 32-group row captured on a single stream and replayed twice equals the eager result."""
    case = S.BY_ID["g32x32_tiles"]
    m, static_x = S.module(case).cuda(), S.input_of(case).cuda()
    with torch.no_grad():
        want = m(static_x).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        m(static_x)                                                    # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = m(static_x)
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), f"replay {rep} differs from the eager result"
        out.zero_()
    _status()


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------
def _raw_call(case, ws_bytes_delta=0, sk_wide=None, d=None):
    """mi355_sk_fwd through the raw library (no check()): returns (code, y, trace tags, bytes asked for)."""
    import mi355attn
    from mi355attn import _ffi
    from mi355attn import functional as F
    m, x = S.module(case).cuda(), S.input_of(case).cuda()
    b3 = F.bn_fold(m.split_3x3[1], m.split_3x3[0].bias)
    b5 = F.bn_fold(m.split_5x5[1], m.split_5x5[0].bias)
    bf = F.bn_fold(m.fc[1])
    ps = [t.detach().float().contiguous() for t in (m.split_3x3[0].weight, b3[0], b3[1], m.split_5x5[0].weight, b5[0], b5[1], m.fc[0].weight,
                                                    m.fc[0].bias, bf[0], bf[1], m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)]
    table = (ctypes.c_void_p * 14)(*[t.data_ptr() for t in ps])
    B, Cin, H, W = x.shape
    lib = _ffi.lib()
    need = lib.mi355_sk_ws_bytes(B, Cin, m.planes, m.groups, H, W)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    y = torch.full((B, m.planes, H, W), 7.0, device="cuda")
    out = []

    def call():
        out.append(lib.mi355_sk_fwd(_ffi.dptr(x), ctypes.cast(table, ctypes.c_void_p), _ffi.dptr(y), B, Cin, m.planes, m.groups,
                                    m.d if d is None else d, H, W, _ffi.dptr(ws), need + ws_bytes_delta, _ffi.stream_ptr(x.device)))
    with mi355attn.options(**({} if sk_wide is None else dict(sk_wide=sk_wide))):
        tags = [tag for tag, *_ in mi355attn.kernel_trace(call)]
    torch.cuda.synchronize()
    return out[0], y, tags, need


@pytest.mark.parametrize("cid", S.IDS + S.COVERED_IDS)
def test_ws_bytes_is_at_least_the_old_query(cid):
    from mi355attn import _ffi
    (Cin, planes), groups, (B, _, H, W) = S.BY_ID[cid][1], S.BY_ID[cid][2], S.BY_ID[cid][3]
    lib = _ffi.lib()
    assert lib.mi355_sk_ws_bytes(B, Cin, planes, groups, H, W) >= lib.mi355_sk_workspace_bytes(B, planes, H, W) > 0


@pytest.mark.parametrize("cid,sk_wide", [("g32x32_ragged", None), ("g3x5", None), ("covered_ragged", 1)])
def test_a_workspace_one_byte_short_is_refused_and_launches_nothing(cid, sk_wide):
    from mi355attn import _ffi
    case = S.BY_ID[cid]
    code, y, tags, _ = _raw_call(case, -1, sk_wide)
    assert code == -1 and b"workspace_bytes" in _ffi.lib().mi355_last_error(), (code, _ffi.lib().mi355_last_error())      # MI355_EINVAL
    assert not tags and bool((y == 7.0).all()), tags
    code, y, tags, _ = _raw_call(case, 0, sk_wide)                     # the exact size is accepted
    assert code == 0 and len(_wide_tags(tags)) == 1
    assert_parity(y.cpu(), S.truth(case), S.TOL, f"SKLayer {cid} raw call")
    _status()


def test_old_route_keeps_accepting_the_old_workspace_size():
    from mi355attn import _ffi
    case = S.BY_ID["covered_ragged"]
    (_, planes), (B, _, H, W) = case[1], case[3]
    code, y, tags, need = _raw_call(case, 0)
    old = _ffi.lib().mi355_sk_workspace_bytes(B, planes, H, W)
    assert old < need
    code, y, tags, _ = _raw_call(case, old - need)
    assert code == 0 and not _wide_tags(tags)
    assert_parity(y.cpu(), S.truth(case), 3e-5, "SKLayer covered_ragged, old workspace size")
    _status()


def test_select_kernel_limit_stays():
    """d + planes > 12288 is still MI355_EUNSUPPORTED (the select kernel's LDS), on the new route too; nothing is launched."""
    from mi355attn import _ffi
    code, y, tags, _ = _raw_call(S.BY_ID["g32x32_1x1"], 0, None, d=12288 - 64 + 1)
    assert code == -2 and b"12288" in _ffi.lib().mi355_last_error(), (code, _ffi.lib().mi355_last_error())
    assert not tags and bool((y == 7.0).all())
    _status()
