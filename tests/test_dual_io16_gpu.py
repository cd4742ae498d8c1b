"""GPU tests (-m gpu): CAM and PAM on fp16 and bf16 activations (csrc/dual_attn_io16.hip; entries mi355_cam_x16_fwd,
mi355_conv1x1_tokens16_fwd, mi355_tokens_to_nchw_axpy_x16_fwd).

Reference: oracle.axis_attn.cam_forward / pam_forward in fp64 on x16.double().  Shapes, inputs and the per-element bound
    |y - ref64| <= u |ref64| + T max|ref64|  (+ 2^-25 for fp16 results below the normal range),  T = 5e-5 (CAM) / 1e-3 (PAM)
are tests/dual_io16_cases.py; tests/test_dual_io16_cpu.py shows on the CPU that the fp32 oracle, rounded once, keeps them.  Each shape is
the smallest that reaches one code path; the kernel tags are asserted from mi355attn.kernel_trace."""
import re

import pytest
import torch

import dual_io16_cases as D
from io16_common import DTYPES, IO, _run, _status

pytestmark = pytest.mark.gpu


def _no_fp32_x_kernels(tags):
    """No staged fp32 copy of x, no fp32 Gram / apply product and no gathering fp32 projection (gemm_kernel<..,a2>)."""
    assert not any("ragged_stage_kernel" in t for t in tags), tags
    assert not any(re.search(r"gemm_kernel<prec \d,b\d,a2>", t) for t in tags), tags


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", D.CAM_SHAPES, ids=D.sid)
def test_cam_vs_fp64_oracle(shape, dtype):
    x, ref = D.cam_case(shape, dtype)
    y, tags = _run(D.cam_module().cuda(), x.cuda())
    assert y.dtype == dtype
    io, vec = IO[dtype], D.vec_of(shape)
    for want in (f"cam_gram16_kernel io={io} vec={vec} ", f"cam_apply16_kernel io={io} vec={vec} "):
        assert any(t.startswith(want) for t in tags), (want, tags)
    _no_fp32_x_kernels(tags)
    assert not any("gemm_kernel<" in t for t in tags), tags
    D.check(y, ref, dtype, D.T_CAM, f"CAM{shape} {dtype}")
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", D.PAM_SHAPES, ids=D.sid)
def test_pam_vs_fp64_oracle(shape, dtype):
    from mi355attn.modules import PAM
    x, m, ref = D.pam_case(shape, dtype)
    y, tags = _run(m.cuda(), x.cuda())
    assert y.dtype == dtype
    io, vec = IO[dtype], D.vec_of(shape)
    for want in (f"conv1x1_tokens16_kernel io={io} vec={vec} ", f"tokens_to_nchw_axpy16_kernel io={io} "):
        assert any(t.startswith(want) for t in tags), (want, tags)
    _no_fp32_x_kernels(tags)
    kind = PAM._route(shape[1])[0]
    assert any("sdpa_wide_kernel" in t for t in tags) == (kind == "wide"), (kind, tags)
    D.check(y, ref, dtype, D.T_PAM, f"PAM{shape} ({kind}) {dtype}")
    _status()


def test_cam_subnormal_channel():
    """Decides the form of the fp16 Gram: a product that flushes fp16 subnormal operands misses this bound 206 times over
    (tests/test_dual_io16_cpu.py)."""
    x = D.subnormal_input()
    y, tags = _run(D.cam_module().cuda(), x.cuda())
    assert any(t.startswith("cam_gram16_kernel io=1 vec=8 ") for t in tags), tags
    D.check(y, D.cam_ref(x), torch.float16, D.T_CAM, "CAM, fp16 subnormal channel")
    _status()


VS32 = ([("cam", s) for s in D.CAM_SHAPES if s[2:] != (65, 65)] + [("pam", s) for s in D.PAM_SHAPES if s[2:] != (65, 65)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,shape", VS32, ids=[f"{k}-{D.sid(s)}" for k, s in VS32])
def test_16bit_path_vs_fp32_path(kind, shape, dtype):
    """m(x16) against m(x16.float()) in its strict mode (precision 0; PAM's default, set here for CAM, whose default runs attn . X on
    fp16 operands and is no strict-class path), which runs on code this change does not touch: both are strict-class, so
    |float(y16) - y32| <= u |y32| + 5e-5 max|y32| per element; PAM at precision 1 as well (both paths then round the same fp32 q / k / v):
    there the allowance is 1e-3, the bar of that mode.  CAM.precision is not read for a 16-bit x."""
    if kind == "cam":
        m, xd = D.cam_module().cuda(), D.cam_case(shape, dtype)[0].cuda()
        with torch.no_grad():
            y_default = m(xd)
            m.precision = 0
            y16, y32 = m(xd), m(xd.float())
        assert y16.dtype == dtype and y32.dtype == torch.float32
        assert torch.equal(y16, y_default), "CAM.precision changed the result on a 16-bit x"
        D.check(y16, y32.cpu(), dtype, 5e-5, f"CAM{shape} {dtype} vs the strict fp32 path")
    else:
        x, m, _ = D.pam_case(shape, dtype)
        m, xd = m.cuda(), x.cuda()
        try:
            for prec, T in ((0, 5e-5), (1, 1e-3)):
                m.precision = prec
                with torch.no_grad():
                    y16, y32 = m(xd), m(xd.float())
                assert y16.dtype == dtype and y32.dtype == torch.float32
                D.check(y16, y32.cpu(), dtype, T, f"PAM{shape} {dtype} precision {prec} vs the fp32 path")
        finally:
            m.precision = 0
    _status()


def test_fp32_input_keeps_its_path_and_the_other_modules_still_refuse():
    from mi355attn.modules import GCModule, SKLayer
    shape = (2, 64, 8, 8)
    for name, m, x in (("CAM", D.cam_module().cuda(), D.cam_case(shape, torch.float16)[0]),
                       ("PAM", D.pam_case(shape, torch.float16)[1].cuda(), D.pam_case(shape, torch.float16)[0])):
        xd = x.cuda().float()
        y_first, tags = _run(m, xd)
        assert y_first.dtype == torch.float32 and tags and not any("16" in t for t in tags), (name, tags)
        with torch.no_grad():
            m(xd.half()), m(xd.bfloat16())
            y_last = m(xd)
        assert torch.equal(y_first, y_last), f"{name}: an fp32 result changed after 16-bit calls"
    xh = D.cam_case(shape, torch.float16)[0].cuda()
    for m in (GCModule(64), SKLayer(64, 64)):
        with pytest.raises(TypeError, match="PAM and CAM only"):
            m.eval().cuda()(xh)
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_16bit_parameters_and_in_place_update(dtype):
    """module.half() / .bfloat16() on x of the same type equals the fp32-parameter module built from the widened parameters, bit for bit;
    an in-place change of alpha / beta is seen by the next forward (no stale fp32 copy)."""
    for name, build, shape, scalar in (("PAM", lambda: D.pam_module(48)[0], (2, 48, 6, 10), "alpha"), ("CAM", D.cam_module, (2, 48, 6, 10), "beta")):
        m = build().cuda()
        xd = (D.pam_input(shape, dtype) if name == "PAM" else D.cam_input(shape, dtype)).cuda()
        cast = lambda: {torch.float16: m.half, torch.bfloat16: m.bfloat16}[dtype]()  # noqa: E731
        with torch.no_grad():
            m16 = cast()
            assert all(p.dtype == dtype for p in m16.parameters())
            y16 = m16(xd)
            y32 = m16.float()(xd)                                      # the same (rounded) values in fp32 parameters
            assert y16.dtype == dtype and torch.equal(y16, y32), f"{name}: 16-bit parameters change the result"
            m16 = cast()
            assert torch.equal(m16(xd), y16)
            getattr(m16, scalar).mul_(-1.5)
            after = m16(xd)
            assert not torch.equal(after, y16), f"{name}: stale fp32 copy of an updated 16-bit parameter"
            assert torch.equal(after, m16.float()(xd)), name
    _status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_pam_range_fallback_works_with_16bit_x(dtype):
    """PAM.precision = 1 on a 16-bit x: the projection stays strict-class, the core stages fp32 q / k / v to fp16 and reports a saturation
    (range code 7) as for an fp32 x; module(x) then returns the strict result with one warning (the construction of
    tests/test_pam_any_width_gpu.py::test_fp16_range_guard_of_the_wide_kernel: b's weights x 2000, x x 100)."""
    import warnings
    import mi355attn
    mi355attn.range_status(wait=True)
    m, _ = D.pam_module(64)
    with torch.no_grad():
        m.b.weight.mul_(2000.0)
    m = m.cuda()
    xd = (D.pam_input((2, 64, 8, 8), torch.float32) * 100.0).to(dtype).cuda()
    with torch.no_grad():
        strict = m(xd)
    assert strict.dtype == dtype and torch.isfinite(strict).all()
    m.precision = 1
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        y, tags = _run(m, xd)
    hits = [i for i in w if "re-running this forward in strict mode" in str(i.message)]
    assert len(hits) == 1, [str(i.message) for i in w]
    assert any("sdpa_stream_kernel<d=64,prec 1>" in t for t in tags) and any("sdpa_stream_kernel<d=64,prec 0>" in t for t in tags), tags
    assert torch.equal(y, strict), "the fallback did not return the strict result"
    _status()


def test_fp16_extremes_follow_the_rounded_fp32_result():
    """x = +-60000 at (1,16,4,8) with beta / alpha = 0.7: |y| reaches (1 + 0.7) max|x| and leaves the fp16 range.  y is inf exactly where
    m(x.float()).half() is; the finite elements keep the bound; nothing is reported (outputs are not MFMA operands)."""
    shape = (1, 16, 4, 8)
    g = torch.Generator(device="cpu").manual_seed(4321)
    x = torch.where(torch.randn(*shape, generator=g) >= 0, 60000.0, -60000.0).half()
    pam, sd = D.pam_module(16)
    for name, m, ref, T in (("CAM", D.cam_module(0.7), D.cam_ref(x, 0.7), D.T_CAM), ("PAM", pam, D.pam_ref(x, sd), D.T_PAM)):
        m = m.cuda()
        with torch.no_grad():
            y = m(x.cuda()).cpu()
            y32h = m(x.cuda().float()).half().cpu()
        assert y.dtype == torch.float16 and not torch.isnan(y).any(), name
        assert torch.equal(torch.isinf(y), torch.isinf(y32h)) and torch.equal(y[torch.isinf(y)], y32h[torch.isinf(y)]), f"{name}: inf pattern"
        print(f"[dual16] {name} at +-60000: {int(torch.isinf(y).sum())} of {y.numel()} elements are inf")
        fin = torch.isfinite(y) & (ref.abs() < 65504.0)
        D.check(y, ref, torch.float16, T, f"{name} fp16, x = +-60000, finite elements", only=fin)
        _status()                                                      # sync and range words stay clean


def test_graph_capture_and_replay():
    """One fp16 CAM and one fp16 PAM(64) forward captured on a single stream and replayed twice equal the eager result."""
    shape = (2, 64, 8, 8)
    cam, pam = D.cam_module().cuda(), D.pam_case(shape, torch.float16)[1].cuda()
    static_x = D.cam_input(shape, torch.float16).cuda()
    with torch.no_grad():
        want = (cam(static_x).clone(), pam(static_x).clone())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        cam(static_x), pam(static_x)                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = (cam(static_x), pam(static_x))
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]), f"replay {rep} differs from the eager result"
        out[0].zero_(), out[1].zero_()
    _status()
