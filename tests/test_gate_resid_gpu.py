"""GPU tests (-m gpu) of the residual (+ ReLU) epilogue of SELayer / ECALayer / CBAM: m(x, resid=r, relu=b) = [relu](m(x) + r) in the gate
kernels' store epilogue (csrc/gate_res.h; mi355_se_res_fwd, mi355_eca_res_fwd, mi355_cbam_res_fwd).

  1  fp32: the bits of torch.relu(m(x) + r) / m(x) + r, every shape of tests/gate_resid_cases.py, both forms
  2  every I/O type against the fp64 composition of the oracle (fp32: conftest.assert_parity at 1e-5; 16-bit: io16_common._check_chan)
  3  one launch set: the residual call launches what the plain call launches, under tags of its own
  4  plain and residual calls mixed on one stream, and a replayed graph of a residual SE call, give the bits of isolated calls
  5  inf / NaN in x and in resid come out where the reference has them; an fp16 sum beyond 65504 is inf where the reference is
  6  channels_last and sliced resid give the bits of their contiguous copies
  7  argument errors are raised before any launch"""
import pytest
import torch

import gate_resid_cases as G
from conftest import assert_parity
from io16_common import _check_chan, _status

pytestmark = pytest.mark.gpu

IDS = [G.case_id(c) for c in G.CASES]


def _fused(m, x, r, relu):
    with torch.no_grad():
        return m(x, resid=r, relu=relu)


def _trace(fn):
    import mi355attn
    out = []
    with torch.no_grad():
        rows = mi355attn.kernel_trace(lambda: out.append(fn()))
    tags = []
    for tag, count, *_ in rows:
        tags += [tag] * count
    return out[0], sorted(tags)


# ---- 1: fp32 bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", G.CASES, ids=IDS)
@pytest.mark.parametrize("gate", G.GATES)
def test_fp32_result_has_the_bits_of_the_torch_composition(gate, case, relu):
    import mi355attn
    shape, opts = case
    m = G.build(gate, shape[1]).cuda()
    x, r = (t.cuda() for t in G.inputs(shape, torch.float32))
    with mi355attn.options(**opts), torch.no_grad():
        want = m(x) + r
        if relu:
            want = torch.relu(want)
        got = _fused(m, x, r, relu)
    assert got.dtype == torch.float32 and torch.equal(got, want), f"{gate}{shape}: {int((got != want).sum())} elements differ"
    _status(range_word=False)


# ---- 2: oracle -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("io", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("case", G.CASES, ids=IDS)
@pytest.mark.parametrize("gate", G.GATES)
def test_against_the_fp64_composition_of_the_oracle(gate, case, io, relu):
    import mi355attn
    shape, opts = case
    dt = G.DTYPES[io]
    m = G.build(gate, shape[1])
    x, r = G.inputs(shape, dt)
    ref = G.reference(gate, m, x, r, relu)
    m = m.cuda()
    with mi355attn.options(**opts):
        got = _fused(m, x.cuda(), r.cuda(), relu)
    what = f"{gate}{shape} {io} relu={relu}"
    if io == "fp32":
        assert got.dtype == torch.float32
        assert_parity(got.cpu().double(), ref, 1e-5, what)
    else:
        _check_chan(got, ref, dt, what)
    _status(range_word=False)


# ---- 3: one launch set -------------------------------------------------------------------------------------------------------------------
PLAIN_FINAL = {"se": "gate_scale", "eca": "gate_scale", "cbam": "cbam_apply_band"}      # fp32 multi-pass: the final pass carries no plain tag


@pytest.mark.parametrize("io", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("case", [(G.SINGLE, {}), (G.MULTI, G.SINGLE_OFF)], ids=["single", "multi"])
@pytest.mark.parametrize("gate", G.GATES)
def test_residual_call_is_one_launch_set_with_tags_of_its_own(gate, case, io):
    """The residual call launches the kernels of the plain call: its tags are the plain tags with `_res` in the kernel name and
    ` res=1 relu=b` at the end of the kernel that stores y.  (The fp32 multi-pass forms file none of their plain launches, so there the
    residual call shows its one tagged final pass and nothing else.)"""
    import mi355attn
    shape, opts = case
    dt = G.DTYPES[io]
    m = G.build(gate, shape[1]).cuda()
    x, r = (t.cuda() for t in G.inputs(shape, dt))
    with mi355attn.options(**opts):
        for relu in (False, True):
            _, plain = _trace(lambda: m(x))
            _, fused = _trace(lambda: m(x, resid=r, relu=relu))
            res = [t for t in fused if " res=1 relu=%d" % relu in t]
            assert len(res) == 1 and "_res_kernel " in res[0], (fused, plain)
            back = sorted(t.replace("_res_kernel ", "_kernel ").replace(" res=1 relu=%d" % relu, "") for t in fused)
            if io == "fp32" and opts:
                assert plain == [t for t in back if not t.startswith(PLAIN_FINAL[gate])] and len(fused) == len(plain) + 1, (plain, fused)
            else:
                # SE at three workgroups per CU runs its residual form at two: the occupancy and store-hint fields follow it
                strip = lambda ts: sorted(" ".join(f for f in t.split() if not f.startswith(("occ=", "nts="))) for t in ts)
                assert strip(back) == strip(plain) and len(fused) == len(plain), (plain, fused)
            twin = res[0].split()[0].replace("_res_kernel", "_kernel")
            assert not any(t.split()[0] == twin for t in fused), f"the residual call also shows the plain tag of {twin}: {fused}"
            _, again = _trace(lambda: m(x))
            assert again == plain, "a plain call after the residual call shows the plain tags"
    _status(range_word=False)


# Which instantiation a SLOTS shape reaches, read from the `NV=` field of the residual tag: fp32 rows hold H*W / 256 float4 per lane (SE /
# ECA ladder 1, 2, 4, 8, 13, 16), 16-bit rows H*W / 512 chunks (ladder 1, 2, 4, 7, 8); CBAM's NV is the channel slots per lane (4, 8, 16).
SLOT_NV = {32: [1, 2, 4, 8, 13, 16], 16: [1, 1, 2, 4, 7, 8]}
CBAM_NV = [4, 4, 4, 4, 4, 4]        # 16 / 32 channels over 16 or 32 channel groups: one slot, the 4-slot instantiation


@pytest.mark.parametrize("io", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("idx", range(len(G.SLOTS)))
@pytest.mark.parametrize("gate", G.GATES)
def test_slot_shapes_reach_the_instantiation_they_are_listed_for(gate, idx, io):
    shape = G.SLOTS[idx]
    dt = G.DTYPES[io]
    m = G.build(gate, shape[1]).cuda()
    x, r = (t.cuda() for t in G.inputs(shape, dt))
    _, fused = _trace(lambda: m(x, resid=r, relu=True))
    kernel = {"se": "se_single_res_kernel", "eca": "eca_halo_res_kernel", "cbam": "cbam_single_res_kernel"}[gate]
    if io != "fp32":
        kernel = kernel.replace("se_", "se16_").replace("eca_", "eca16_").replace("cbam_", "cbam16_")
    tags = [t for t in fused if t.startswith(kernel + " ")]
    assert len(tags) == 1 and len(fused) == 1, fused
    nv = int(dict(f.split("=") for f in tags[0].split()[1:])["NV"])
    want = CBAM_NV[idx] if gate == "cbam" else SLOT_NV[32 if io == "fp32" else 16][idx]
    assert nv == want, (tags[0], want)


CBAM_CLASS_SHAPES = [G.SINGLE, (1, 128, 8, 8), (1, 200, 8, 8), (1, 256, 8, 8), G.PARTIAL, (1, 512, 8, 8)]


def test_every_cbam_slot_class_is_reached_and_right():
    """The SLOTS shapes all land in CBAM's 4-slot instantiation, so its other classes get shapes of their own: NV = 4, 8 and 16, the last
    slot full and partly filled, fp32 and fp16 (16 partly filled slots have no 16-bit single-read form: that call takes the general
    form).  Each against the fp64 composition, with the class read from the tag."""
    seen = set()
    for shape in CBAM_CLASS_SHAPES:
        cpu = G.build("cbam", shape[1])
        m = G.build("cbam", shape[1]).cuda()
        for dt in (torch.float32, torch.float16):
            x, r = G.inputs(shape, dt)
            got, fused = _trace(lambda: m(x.cuda(), resid=r.cuda(), relu=True))
            single = [t for t in fused if "_single_res_kernel " in t]
            if single:
                assert len(fused) == 1, fused
                kv = dict(f.split("=") for f in single[0].split()[1:])
                seen.add((dt == torch.float32, int(kv["NV"]), int(kv["full"])))
            ref = G.reference("cbam", cpu, x, r, True)
            if dt == torch.float32:
                assert_parity(got.cpu().double(), ref, 1e-5, f"cbam{shape}")
            else:
                _check_chan(got, ref, dt, f"cbam{shape} fp16")
    want = {(f32, nv, full) for f32 in (True, False) for nv in (4, 8, 16) for full in (0, 1)} - {(False, 16, 0), (True, 4, 0), (False, 4, 0)}
    assert want <= seen, sorted(want - seen)
    _status(range_word=False)


def test_cbam_16_slot_form_beyond_one_workgroup_per_cu_takes_the_multi_pass_form():
    """The one documented exception to "the route of the plain call": single-read CBAM with 16 slots per lane runs one workgroup per CU in
    its residual form, so an image with more bands than the device has CUs takes the multi-pass residual form while the plain call stays
    single-read.  (1, 264, 257, 4): 257 one-row bands, 264 channels over 32 groups = 9 slots -> the 16-slot instantiation."""
    import mi355attn
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shape = (1, 264, 257, 4)
    m = G.build("cbam", shape[1]).cuda()
    x, r = (t.cuda() for t in G.inputs(shape, torch.float32))
    with torch.no_grad(), mi355attn.options(cbam_single=0):
        want = torch.relu(m(x) + r)                                    # the bits of the form that runs: the multi-pass composition
    _, plain = _trace(lambda: m(x))
    got, fused = _trace(lambda: m(x, resid=r, relu=True))
    assert_parity(got.cpu().double(), G.reference("cbam", G.build("cbam", shape[1]), x.cpu(), r.cpu(), True), 1e-5, "cbam reroute")
    assert len(plain) == 1 and plain[0].startswith("cbam_single_kernel ") and "NV=16" in plain[0], plain
    if 257 > cus:
        assert len(fused) == 1 and fused[0].startswith("cbam_apply_band_res_kernel "), fused
        assert torch.equal(got, want)
    else:
        assert len(fused) == 1 and fused[0].startswith("cbam_single_res_kernel "), fused
        with torch.no_grad():
            assert torch.equal(got, torch.relu(m(x) + r))
    mi355attn.sync_status(wait=True)


# ---- 4: mixing and replay ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("gate", G.GATES)
def test_plain_and_residual_calls_mixed_on_one_stream(gate, io):
    dt = G.DTYPES[io]
    shape = (6, 64, 28, 28)
    m = G.build(gate, 64).cuda()
    x, r = (t.cuda() for t in G.inputs(shape, dt))
    with torch.no_grad():
        want_p = m(x).clone()
        torch.cuda.synchronize()
        want_f = m(x, resid=r, relu=True).clone()
        torch.cuda.synchronize()
        a, b, c, d = m(x), m(x, resid=r, relu=True), m(x), m(x, resid=r, relu=True)
    torch.cuda.synchronize()
    assert torch.equal(a, want_p) and torch.equal(c, want_p) and torch.equal(b, want_f) and torch.equal(d, want_f)
    _status(range_word=False)


@pytest.mark.parametrize("io", ["fp32", "fp16", "bf16"])
def test_graph_replay_of_a_residual_se_call(io):
    """A captured and replayed graph of one residual SE call (a straight chain, no parallel branches) gives the bits of the eager call,
    with eager plain and residual calls on the same workspace in between."""
    dt = G.DTYPES[io]
    shape = (6, 64, 28, 28)
    se = G.build("se", 64).cuda()
    static_x, static_r = (t.cuda().clone() for t in G.inputs(shape, dt, seed=41))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        se(static_x, resid=static_r, relu=True)                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = se(static_x, resid=static_r, relu=True)
    for rep in range(3):
        x, r = (t.cuda() for t in G.inputs(shape, dt, seed=100 + rep))
        static_x.copy_(x)
        static_r.copy_(r)
        g.replay()
        if rep == 1:
            g.replay()
        torch.cuda.synchronize()
        got = out.clone()
        with torch.no_grad():
            se(x)                                                      # an eager plain call in between
            eager = se(x, resid=r, relu=True)
        assert torch.equal(got, eager), f"replay {rep}: replay and eager launch differ"
    _status(range_word=False)


# ---- 5: non-finite values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("case", [(G.SINGLE, {}), (G.RAGGED[1], {})], ids=["single", "ragged"])
@pytest.mark.parametrize("gate", G.GATES)
def test_inf_and_nan_come_out_where_the_reference_has_them(gate, case, io):
    shape, _ = case
    dt = G.DTYPES[io]
    m = G.build(gate, shape[1])
    x, r = (t.clone() for t in G.inputs(shape, dt))
    r[0, 1, 0, 0] = float("inf")
    r[0, 2, -1, -1] = float("-inf")                                    # relu(-inf) = 0
    r[1, 3, 0, 1] = float("nan")                                       # relu(NaN) = NaN
    x[1, 5, 2, 3] = float("nan")                                       # poisons the gates of image 1 (CBAM: the whole image)
    for relu in (False, True):
        ref = G.reference(gate, m, x, r, relu)
        got = _fused(m.cuda(), x.cuda(), r.cuda(), relu).cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{gate} {io} relu={relu}: NaN pattern"
        assert torch.equal(torch.isinf(got), torch.isinf(ref)) and torch.equal(got[torch.isinf(ref)].double(), ref[torch.isinf(ref)]), "inf pattern"
        assert torch.isnan(got[1, 3, 0, 1]) and float(got[0, 1, 0, 0]) == float("inf") and float(got[0, 2, -1, -1]) == (0.0 if relu else float("-inf"))
    _status(range_word=False)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("gate", G.GATES)
def test_fp16_overflow_is_inf_exactly_where_the_rounded_reference_is(gate, relu):
    """x = resid = 60000 in fp16: |y| reaches |x| + |resid|, the fp16 result is inf exactly where the fp64 reference rounded to fp16 is."""
    shape = G.SINGLE
    m = G.build(gate, shape[1])
    x = torch.full(shape, 60000.0, dtype=torch.float16)
    r = torch.full(shape, 60000.0, dtype=torch.float16)
    ref = G.reference(gate, m, x, r, relu)
    assert not ((ref.abs() > 6.5e4) & (ref.abs() < 6.6e4)).any(), "a reference element is borderline for fp16"
    ref16 = ref.to(torch.float16)
    assert torch.isinf(ref16).any()
    got = _fused(m.cuda(), x.cuda(), r.cuda(), relu).cpu()
    assert torch.equal(torch.isinf(got), torch.isinf(ref16))
    _check_chan(got, ref16.double().where(torch.isinf(ref16), ref), torch.float16, f"{gate} fp16 overflow relu={relu}")
    _status(range_word=False)


# ---- 6: layout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("gate", G.GATES)
def test_channels_last_and_sliced_resid_give_the_bits_of_their_contiguous_copies(gate, io):
    dt = G.DTYPES[io]
    shape = G.SINGLE
    m = G.build(gate, shape[1]).cuda()
    x, r = (t.cuda() for t in G.inputs(shape, dt))
    want = _fused(m, x, r, True)
    assert torch.equal(_fused(m, x, r.contiguous(memory_format=torch.channels_last), True), want)
    big = torch.zeros(shape[0], shape[1], shape[2] + 3, shape[3] + 5, dtype=dt, device="cuda")
    big[:, :, 1:1 + shape[2], 2:2 + shape[3]] = r
    sliced = big[:, :, 1:1 + shape[2], 2:2 + shape[3]]
    assert not sliced.is_contiguous() and torch.equal(_fused(m, x, sliced, True), want)
    _status(range_word=False)


# ---- 7: argument errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", G.GATES)
def test_argument_errors_are_raised_before_any_launch(gate):
    import mi355attn
    import mi355attn.functional as F
    shape = G.SINGLE
    m = G.build(gate, shape[1]).cuda()
    x, r = (t.cuda() for t in G.inputs(shape, torch.float32))

    def launches(fn, exc):
        out = []
        def run():
            with pytest.raises(exc):
                fn()
        rows = mi355attn.kernel_trace(run)
        assert not rows, rows

    launches(lambda: m(x, resid=r[:, :, :-1]), ValueError)
    launches(lambda: m(x, resid=r[:1]), ValueError)
    launches(lambda: m(x, resid=r.half()), TypeError)
    launches(lambda: m(x.half(), resid=r), TypeError)
    launches(lambda: m(x, resid=r.cpu()), mi355attn.Mi355Error)          # the package's own error for a CPU tensor, as for a CPU x
    launches(lambda: m(x, relu=True), ValueError)
    if gate == "cbam":
        w = (m.ca.fc[0].weight, m.ca.fc[2].weight, m.sa.conv.weight)
        launches(lambda: F.cbam_forward(x, *w, stage=1, resid=r), ValueError)
        launches(lambda: F.cbam_forward(x, *w, stage=2, resid=r, relu=True), ValueError)
    mi355attn.sync_status(wait=True)
