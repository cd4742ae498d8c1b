"""GPU tests (-m gpu): CoordinateAttention, TripletAttention (and AttentionGate on its own) and BAM on fp16 and bf16 activations
(csrc/axis_attn_io16.hip; entries mi355_coordatt16_fwd, mi355_triplet16_fwd, mi355_attention_gate16_fwd, mi355_bam16_fwd).

Reference: oracle.axis_attn.{coordatt,triplet,bam}_forward in fp64 on x16.double() and the modules' fp32 state_dict.  The kernels compute
in fp32 on the exactly widened input and round once, so for every element, none excluded,
    |y - ref64| <= u * |ref64| + 3e-5 * max|ref64| (+ 2^-25 for fp16 results below the normal range),
u = 2^-11 (fp16) / 2^-8 (bf16): half an ulp, relative; 3e-5 is what tests/test_gpu_parity.py allows these modules in fp32
(VECTOR_CHAINS).  _check below is io16_common._check_chan with that fp32 allowance in place of the channel gates' 1e-5; it prints
max err / bound before it asserts.  tests/test_axis_io16_cpu.py shows on the CPU that the fp32 oracle, rounded once, keeps the bound.

Modules are seeded (axis_io16_arena_rows.build): the default BatchNorm is the identity.  Each shape is the smallest that reaches one
code path; the expected kernel tags are asserted from mi355attn.kernel_trace."""
import functools

import pytest
import torch

from axis_io16_arena_rows import build, reference
from io16_common import DTYPES, IO, U, _input, _run, _status, _ulps

pytestmark = pytest.mark.gpu

T32 = 3e-5


def _check(got, ref, dtype, what, only=None):
    """The bound of the module docstring, every element (`only`: a mask, for the overflow test); prints the figures before it asserts."""
    assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape), what
    got, ref = got.detach().cpu().double(), ref.double()
    fin = torch.isfinite(ref) if only is None else only
    if only is None:
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaN pattern differs from the reference"
        assert torch.equal(torch.isinf(got), torch.isinf(ref)) and torch.equal(got[torch.isinf(ref)], ref[torch.isinf(ref)]), f"{what}: inf pattern"
    t32 = T32 * float(ref[fin].abs().max()) if fin.any() else 0.0
    bound = U[dtype] * ref.abs() + t32
    if dtype == torch.float16:
        bound = bound + (ref.abs() < 2.0 ** -14).double() * 2.0 ** -25
    err = (got - ref).abs()
    worst = float((err[fin] / bound[fin]).max()) if fin.any() else 0.0
    print(f"[axis16] {what}: max err / bound = {worst:.3f}, max abs err = {float(err[fin].max()) if fin.any() else 0.0:.3e}, t32 = {t32:.3e}")
    assert worst <= 1.0, f"{what}: error is {worst:.3f} x the bound"


@functools.lru_cache(maxsize=None)
def _case(kind, shape, dtype, ks=7):
    """(host x16, module on the device, fp64 reference): built once per case and shared, never modified."""
    m = build(kind, shape[1], ks)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = _input(shape, dtype)
    return x, m.cuda(), reference(kind, x, sd)


def _expected_tags(kind, shape, dtype, Cr=None):
    """The new kernels a forward of this shape must run, from the dispatch rules of csrc/axis_attn_io16.hip (a fresh device tensor is
    256-byte aligned): 16-byte lanes need H*W % 8 == 0 (channel reductions, plane sums) or W % 8 == 0 (pooling, apply); planes above
    64 KB as fp32 with the odd pitch take the pooling kernel without LDS."""
    B, C, H, W = shape
    io = IO[dtype]
    hw8, w8 = 8 if H * W % 8 == 0 else 1, 8 if W % 8 == 0 else 1
    pool = (f"plane_pool16_lds_kernel io={io} max=%d vec={w8} " if H * (W + 1) * 4 <= 65536 else f"plane_pool16_kernel io={io} max=%d ")
    mode = {"coord": 1, "triplet": 2, "bam": 3, "gate": 4}[kind]
    tags = [f"apply16_kernel io={io} mode={mode} vec={w8}"]
    if kind == "coord":
        tags.append(pool % 0)
    if kind == "triplet":
        tags.append(pool % 1)
    if kind in ("triplet", "gate"):
        tags.append(f"chan_reduce16_kernel io={io} mode=1 kmax=1 vec={hw8}")
    if kind == "bam":
        kmax = 4 if Cr <= 4 else (8 if Cr <= 8 else (16 if Cr <= 16 else 32))
        vec = 1 if hw8 == 1 else (4 if kmax >= 16 else 8)
        tags += [f"plane_dot16_kernel io={io} vec={hw8}", f"chan_reduce16_kernel io={io} mode=0 kmax={kmax} vec={vec}"]
    return tags


COMMON = [(2, 64, 32, 32),        # 16-byte lanes everywhere, LDS pooling
          (2, 48, 6, 10),         # H*W % 8 = 4: planes are only 8-byte aligned
          (3, 40, 13, 70),        # ragged in every dimension, W > 64
          (2, 16, 70, 6),         # tall: more than 64 rows
          (1, 16, 1, 1)]          # 1 x 1 map
CASES = ([("coord", s, 7) for s in COMMON] + [("coord", (1, 32, 130, 132), 7)]          # plane above 64 KB: pooling without LDS
         + [("triplet", s, 7) for s in COMMON] + [("triplet", (1, 8, 132, 130), 9)]     # the same pooling kernel, with the max
         + [("triplet", (2, 48, 6, 10), 3), ("triplet", (2, 48, 6, 10), 5)]             # the other gate-conv sizes
         + [("bam", s, 7) for s in COMMON]
         + [("bam", (3, 80, 9, 11), 7),                                                 # Cr = 5: the dilated conv without the quad form
            ("bam", (2, 512, 12, 12), 7)]                                               # Cr = 32: the widest channel reduction
         + [("gate", (2, 64, 32, 32), 7), ("gate", (3, 40, 13, 70), 7)])                # AttentionGate on its own


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,shape,ks", CASES, ids=[f"{k}-{'x'.join(map(str, s))}-k{ks}" for k, s, ks in CASES])
def test_modules_vs_fp64_oracle(kind, shape, ks, dtype):
    x, m, ref = _case(kind, shape, dtype, ks)
    y, tags = _run(m, x.cuda())
    Cr = m.spatial_attn.conv1.weight.shape[0] if kind == "bam" else None
    for want in _expected_tags(kind, shape, dtype, Cr):
        assert any(t.startswith(want) for t in tags), (want, tags)
    _check(y, ref, dtype, f"{kind}{shape} k{ks} {dtype}")
    _status()


SUBSET = [("coord", (2, 64, 32, 32)), ("coord", (3, 40, 13, 70)), ("triplet", (2, 64, 32, 32)), ("triplet", (3, 40, 13, 70)),
          ("bam", (2, 64, 32, 32)), ("bam", (3, 80, 9, 11)), ("gate", (2, 64, 32, 32)), ("gate", (3, 40, 13, 70))]


@pytest.mark.parametrize("dtype", DTYPES)
def test_16bit_path_vs_fp32_path_rounded(dtype):
    """m(x16) against m(x16.float()) rounded to the I/O type: the two paths differ by fp32 reassociation only, far below a 16-bit step,
    so they are at most one representable value apart, everywhere."""
    for kind, shape in SUBSET:
        x, m, _ = _case(kind, shape, dtype)
        xd = x.cuda()
        with torch.no_grad():
            y16, y32 = m(xd), m(xd.float())
        assert y16.dtype == dtype and y32.dtype == torch.float32
        d = _ulps(y16, y32.to(dtype))
        print(f"[axis16] {kind}{shape} {dtype}: {d} ulp from the fp32 path")
        assert d <= 1, f"{kind}{shape}: {d} ulps"
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_byte_aligned_input_gives_the_same_bits(dtype):
    """A contiguous x that starts one element into its storage takes the 2-byte lanes in every kernel: bit-identical to an aligned copy."""
    for kind, shape in SUBSET:
        x, m, _ = _case(kind, shape, dtype)
        n = x.numel()
        buf = torch.zeros(n + 1, dtype=dtype, device="cuda")
        off = buf[1:].view(shape)
        off.copy_(x)
        assert off.is_contiguous() and off.data_ptr() % 16 == 2
        y_off, tags = _run(m, off)
        assert tags and all("vec=1" in t or t.startswith("plane_pool16_kernel") for t in tags), tags
        with torch.no_grad():
            y = m(x.cuda())
        assert torch.equal(y_off, y), f"{kind}{shape} {dtype}: the result depends on the alignment of x"
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_16bit_parameters_and_in_place_update(dtype):
    for kind, shape in (("coord", (2, 64, 32, 32)), ("triplet", (3, 40, 13, 70)), ("bam", (2, 64, 32, 32)), ("gate", (2, 64, 32, 32))):
        m = build(kind, shape[1]).cuda()
        xd = _input(shape, dtype).cuda()
        cast = lambda: {torch.float16: m.half, torch.bfloat16: m.bfloat16}[dtype]()
        with torch.no_grad():
            m16 = cast()                                               # in place: parameters and BatchNorm statistics are 16-bit now
            assert all(p.dtype == dtype for p in m16.parameters()) and all(b.dtype == dtype for b in m16.buffers() if b.is_floating_point())
            y16 = m16(xd)
            y32 = m16.float()(xd)                                      # the same (rounded) values in fp32 parameters
            assert y16.dtype == dtype and torch.equal(y16, y32), f"{kind}: 16-bit parameters change the result"
            m16 = cast()
            assert torch.equal(m16(xd), y16)
            p = next(m16.parameters())
            p.mul_(-1.5)                                               # in-place update: no cached fp32 copy may survive it
            after = m16(xd)
            assert not torch.equal(after, y16), f"{kind}: stale fp32 copy of an updated 16-bit parameter"
            assert torch.equal(after, m16.float()(xd)), kind
    _status()


def test_bam_fp16_overflow_follows_the_rounded_reference():
    """BAM's y = x (1 + sigmoid(.)) reaches 2|x|: y may leave the fp16 range.  y is +-inf exactly where the fp64 reference rounded to fp16
    is, finite elsewhere and inside the bound; nothing is reported (outputs are not MFMA operands); the same input in bf16 stays finite."""
    shape = (2, 64, 32, 32)
    m = build("bam", 64)
    with torch.no_grad():
        m.spatial_attn.conv3.weight.zero_()                            # spatial gate = its folded bias: a planted value does not move it
        m.channel_attn.bn.bias.add_(4.0)                               # channel gates well above 0: 1 + sigmoid(.) near 2 ...
        m.channel_attn.bn.bias[17] = -8.0                              # ... and one channel near 1
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.cuda()
    x = _input(shape, torch.float16)
    # +-60000 in pairs per channel, so that the channel means (and with them every channel gate) stay where the random data put them
    big = [(0, 3, 4, 5, 60000.0), (0, 3, 31, 31, -60000.0), (1, 40, 0, 0, 60000.0), (1, 40, 9, 9, -60000.0), (0, 17, 9, 9, 60000.0),
           (0, 17, 20, 1, -60000.0)]
    for b, c, i, j, v in big:
        x[b, c, i, j] = v
    ref = reference("bam", x, sd)
    for b, c, i, j, v in big:
        gate = float(ref[b, c, i, j]) / v                              # 65520 / 60000 = 1.092 is where the fp16 rounding turns to inf
        assert (gate > 1.9) if c != 17 else (gate < 1.01), (b, c, gate)
    ref16 = ref.to(torch.float16)
    assert int(torch.isinf(ref16).sum()) == 4 and bool(torch.isfinite(ref16[0, 17, 9, 9]))
    with torch.no_grad():
        y = m(x.cuda()).cpu()
    assert y.dtype == torch.float16
    assert torch.equal(torch.isinf(y), torch.isinf(ref16)) and torch.equal(y[torch.isinf(ref16)], ref16[torch.isinf(ref16)]), "inf pattern"
    assert not torch.isnan(y).any()
    _check(y, ref, torch.float16, "bam fp16, x = +-60000, finite elements", only=~torch.isinf(ref16))
    _status()                                                          # sync and range words stay clean
    with torch.no_grad():
        yb = m(x.bfloat16().cuda())
    assert torch.isfinite(yb).all(), "bf16 has the fp32 range"
    _check(yb, reference("bam", x.bfloat16(), sd), torch.bfloat16, "bam bf16, x = +-60000")
    _status()


def test_fp32_input_keeps_its_path_and_the_other_entries_still_refuse():
    from mi355attn import functional as F
    shape = (2, 64, 32, 32)
    for kind in ("coord", "triplet", "bam", "gate"):
        x, m, _ = _case(kind, shape, torch.float16)
        xd = x.cuda().float()
        y_first, tags = _run(m, xd)
        assert y_first.dtype == torch.float32 and not any("16" in t for t in tags), (kind, tags)
        with torch.no_grad():
            m(xd.half()), m(xd.bfloat16())
            y_last = m(xd)
        assert torch.equal(y_first, y_last), f"{kind}: an fp32 result changed after 16-bit calls (shared workspace state)"
    xh = _input(shape, torch.float16).cuda()
    bam = _case("bam", shape, torch.float16)[1]
    gc = [torch.zeros(1, device="cuda")] * 8
    with pytest.raises(TypeError):
        F.gc_forward(xh, gc[0], gc[1], gc[2], gc[3], gc[4], gc[5], 1e-5, gc[6], gc[7])
    with pytest.raises(TypeError):
        F.bam_gates(xh, [torch.zeros(1, device="cuda")] * 16, 4, 4)
    with pytest.raises(TypeError):
        F.zpool(xh)
    with pytest.raises(TypeError):
        bam.channel_attn(xh)                                           # the parameter-container helpers return fp32 maps and keep refusing
    _status()


def test_graph_capture_and_replay():
    """One fp16 CoordinateAttention and one fp16 BAM forward captured on a single stream and replayed twice equal the eager result."""
    shape = (2, 64, 32, 32)
    coord, bam = _case("coord", shape, torch.float16)[1], _case("bam", shape, torch.float16)[1]
    static_x = _input(shape, torch.float16, seed=41).cuda()
    with torch.no_grad():
        want = (coord(static_x).clone(), bam(static_x).clone())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        coord(static_x), bam(static_x)                                 # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = (coord(static_x), bam(static_x))
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]), f"replay {rep} differs from the eager result"
        out[0].zero_(), out[1].zero_()
    _status()
