"""What tests/test_dual_io16_cpu.py and tests/test_dual_io16_gpu.py share: the shapes, seeded inputs, modules, fp64 references and the
bound of CAM and PAM on fp16 / bf16 activations (csrc/dual_attn_io16.hip).  A plain module, not a test file: nothing here is collected.

Bound, per element, none excluded (the form of tests/test_axis_io16_gpu.py::_check):
    |y - ref64| <= u |ref64| + T max|ref64|  (+ 2^-25 for fp16 results below the normal range),  u = 2^-11 (fp16) / 2^-8 (bf16),
T = 5e-5 for CAM (the bar test_strict_precision_is_fp32_class holds the fp32 CAM to) and 1e-3 for PAM (the bar tests/test_gpu_parity.py
holds UNSCALED_LOGITS to in every mode).  Inputs are rounded to the I/O type before the oracle sees them.
CAM: ragged_cases.CAM_SCALE * randn / sqrt(HW), beta = ragged_cases.CAM_BETA.  PAM: the protocol of tests/test_pam_any_width_gpu.py
(alpha = 0.7, conv weights x 0.5, x = 0.5 randn, seeds 1234 / 4321)."""
import functools

import torch

import oracle.axis_attn as OA
import ragged_cases as R
from io16_common import U

T_CAM, T_PAM = 5e-5, 1e-3

CAM_SHAPES = [(2, 64, 8, 8),          # 16-byte rows
              (2, 48, 6, 10),         # H*W % 8 == 4: 8-byte pieces
              (2, 64, 7, 7),          # odd H*W
              (3, 30, 9, 7),          # C off every multiple, odd H*W, B = 3
              (1, 5, 3, 3),           # smaller than one MFMA tile in every dimension
              (1, 16, 1, 1),          # 1 x 1 map, K = 1
              (1, 144, 8, 16),        # more than one channel tile in both Gram dimensions and in the K of the apply
              (1, 32, 65, 65)]        # DANet's map: 133 K-steps of 32, unaligned rows
PAM_SHAPES = [(2, 64, 8, 8),          # route `one`
              (2, 48, 6, 10),         # `padded`, 8-byte rows
              (3, 30, 9, 7),          # `padded`, K tail, odd H*W
              (1, 320, 4, 8),         # `pair`, 10 K-steps, Cout = 960 over several N tiles
              (1, 328, 5, 7),         # `wide`, cp = 384
              (1, 32, 65, 65),        # DANet's map
              (1, 8, 1, 1)]           # one token


def sid(shape):
    return "x".join(map(str, shape))


def vec_of(shape):
    """Width of the x loads of a fresh (256-byte aligned) device tensor of this shape: the `vec=` of the kernel tags."""
    hw = shape[2] * shape[3]
    return 8 if hw % 8 == 0 else (4 if hw % 4 == 0 else 1)


def cam_input(shape, dtype):
    return R.cam_input(shape).to(dtype)


def cam_module(beta=R.CAM_BETA):
    from mi355attn.modules import CAM
    m = CAM().eval()
    with torch.no_grad():
        m.beta.fill_(beta)
    return m


def cam_ref(x16, beta=R.CAM_BETA, dtype=torch.float64):
    return OA.cam_forward(x16.to(dtype), {"beta": torch.tensor([beta])}, dtype=dtype)


def pam_module(dim):
    from mi355attn.modules import PAM
    torch.manual_seed(1234)
    m = PAM(dim).eval()
    with torch.no_grad():
        m.alpha.fill_(0.7)
        for c in (m.b, m.c, m.d):
            c.weight.mul_(0.5)
    return m, {k: v.detach().clone() for k, v in m.state_dict().items()}


def pam_input(shape, dtype):
    torch.manual_seed(4321)
    return (torch.randn(*shape) * 0.5).to(dtype)


def pam_ref(x16, sd, dtype=torch.float64):
    return OA.pam_forward(x16.to(dtype), sd, dtype=dtype)


def subnormal_input():
    """fp16 (1,8,4,8): all 32 elements of channel 0 are subnormals (randn x 2e-5), channels 1..7 (randn x 1000) hold none.  Row 0 of the
    Gram matrix is then made of products with subnormals: logits of -5e-3 .. -0.13 that a flushing product turns into 0."""
    g = torch.Generator(device="cpu").manual_seed(4321)
    x = torch.randn(1, 8, 4, 8, generator=g)
    x[:, 0] *= 2e-5
    x[:, 1:] *= 1000.0
    return x.half()


@functools.lru_cache(maxsize=None)
def cam_case(shape, dtype):
    """(host x16, fp64 reference): built once per case and shared, never modified."""
    x = cam_input(shape, dtype)
    return x, cam_ref(x)


@functools.lru_cache(maxsize=None)
def pam_case(shape, dtype):
    """(host x16, module on the host, fp64 reference): built once per case and shared, never modified."""
    m, sd = pam_module(shape[1])
    x = pam_input(shape, dtype)
    return x, m, pam_ref(x, sd)


def check(got, ref, dtype, T, what, only=None, u=None):
    """The bound of the module docstring, every element (`only`: a mask, for the overflow tests; u: another relative term); prints the
    figures before it asserts."""
    assert tuple(got.shape) == tuple(ref.shape), what
    got, ref = got.detach().cpu().double(), ref.double()
    fin = torch.isfinite(ref) if only is None else only
    if only is None:
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaN pattern differs from the reference"
        assert torch.equal(torch.isinf(got), torch.isinf(ref)) and torch.equal(got[torch.isinf(ref)], ref[torch.isinf(ref)]), f"{what}: inf pattern"
    t32 = T * float(ref[fin].abs().max()) if fin.any() else 0.0
    bound = (U[dtype] if u is None else u) * ref.abs() + t32
    if dtype == torch.float16:
        bound = bound + (ref.abs() < 2.0 ** -14).double() * 2.0 ** -25
    err = (got - ref).abs()
    worst = float((err[fin] / bound[fin]).max()) if fin.any() else 0.0
    print(f"[dual16] {what}: max err / bound = {worst:.3f}, max abs err = {float(err[fin].max()) if fin.any() else 0.0:.3e}, t32 = {t32:.3e}")
    assert worst <= 1.0, f"{what}: error is {worst:.3f} x the bound"
    return worst
