"""What tests/test_ragged_maps_cpu.py and tests/test_ragged_maps_gpu.py share: the feature maps whose H*W or channel counts are no
multiples of 4 (the ragged routes of mi355_double_attn_fwd, mi355_double_attn16_fwd and mi355_cam_fwd), the seeded inputs and modules,
and the fp64 references.  A plain module, not a test file: nothing here is collected.

DoubleAttention rows, the smallest at which each piece can go wrong:
  (2, 64, 7, 7) c 32/32      the README configuration on a 7 x 7 map: HW = 1 mod 4, channel counts aligned, not the one-kernel route
  (3, 128, 13, 13) c 128     the two-pass route's channel counts at HW = 169: must not enter it
  (1, 36, 5, 6) c 12/20      HW = 2 mod 4, C % 64 != 0
  (2, 30, 9, 7) c 10/6       HW = 3 mod 4; C, c_m and c_n = 2 mod 4: every pad at once
  (1, 5, 3, 3) c 3/1         c_n = 1 (the softmax over c_n is identically 1); three pad columns out of 12
  (2, 8, 1, 1) c 4/4         HW = 1
  (1, 64, 65, 65) c 32/32    HW = 4225 > 4096: a softmax row that no lane holds in registers
CAM rows: the same residues, C pads, the long row.

CAM's Gram logits are unscaled sums over HW, and large logits make the softmax ill-conditioned whatever evaluates it, so x is
CAM_SCALE * randn / sqrt(HW): diagonal logits near CAM_SCALE^2 at every shape.  tests/test_ragged_maps_cpu.py asserts that at this scale
the oracle's own fp32 evaluation stays within a tenth of the precision-0 bar of its fp64 evaluation."""
import torch

import oracle.axis_attn as OA
import oracle.chan_attn as OC

TOL = {0: 5e-5, 1: 1e-3, 2: 1.2e-2}            # tests/arena_cases.py

# (shape, c_m, c_n)
DA = [((2, 64, 7, 7), 32, 32),
      ((3, 128, 13, 13), 128, 128),
      ((1, 36, 5, 6), 12, 20),
      ((2, 30, 9, 7), 10, 6),
      ((1, 5, 3, 3), 3, 1),
      ((2, 8, 1, 1), 4, 4),
      ((1, 64, 65, 65), 32, 32)]
CAM = [(2, 64, 7, 7), (3, 30, 9, 7), (1, 5, 3, 3), (1, 32, 65, 65)]
CAM_SCALE = 3.0
CAM_BETA = 0.7                                  # at the default of 0 the block is the identity


def da_id(case):
    return "x".join(map(str, case[0])) + f"_c{case[1]}_{case[2]}"


def cam_id(shape):
    return "x".join(map(str, shape))


def da_module(case, precision=None, cls=None, seed=1234):
    """DoubleAttention with the default Conv2d init (non-zero biases); cls: another class with the same constructor (the reference's)."""
    if cls is None:
        from mi355attn.modules import DoubleAttention as cls
    shape, cm, cn = case
    torch.manual_seed(seed)
    m = cls(shape[1], cm, cn)
    if precision is not None:
        m.precision = precision
    return m.eval()


def da_params(m):
    return [t.detach().cpu().float() for t in (m.convA.weight, m.convA.bias, m.convB.weight, m.convB.bias, m.convV.weight, m.convV.bias,
                                               m.proj.weight, m.proj.bias)]


def da_input(case, seed=4321):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*case[0], generator=g) + 0.5


def cam_input(shape, seed=4321):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return CAM_SCALE * torch.randn(*shape, generator=g) / (shape[2] * shape[3]) ** 0.5


_refs = {}


def da_ref(case, x=None):
    """fp64 oracle on da_input(case) (cached) or on x."""
    if x is not None:
        return OC.double_attention_forward(x.double().cpu(), *da_params(da_module(case)), dtype=torch.float64)
    key = ("da", da_id(case))
    if key not in _refs:
        _refs[key] = OC.double_attention_forward(da_input(case).double(), *da_params(da_module(case)), dtype=torch.float64)
    return _refs[key]


def cam_ref(shape, dtype=torch.float64):
    key = ("cam", cam_id(shape), dtype)
    if key not in _refs:
        _refs[key] = OA.cam_forward(cam_input(shape), {"beta": torch.tensor([CAM_BETA])}, dtype=dtype)
    return _refs[key]
