"""Cases of the residual (+ ReLU) epilogue of SELayer / ECALayer / CBAM (tests/test_gate_resid_gpu.py, tests/test_gate_resid_cpu.py):
y = gate(x) + resid, with relu=True y = relu(gate(x) + resid).

The shapes are the smallest that reach each form of the kernels:
  SINGLE    the README shape, single-read form of all three gates and I/O types
  RAGGED    the ragged set of tests/test_io16_gpu.py: H*W no multiple of 4 / 8, C no multiple of 8 -- the multi-pass (general) forms
  PARTIAL   16 register slots per lane in single-read CBAM, the last one partly filled (FULL = false)
  SLOTS     one shape per NV instantiation of the single-read SE / ECA kernels (fp32: 1, 2, 4, 8, 13, 16 float4 per lane; 16-bit: 1, 2,
            4, 7, 8 chunks of 8 values), which also walk CBAM through NV = 4 / 8 / 16 at both segment widths
  MULTI     a shape every single-read form takes, run with the three *_single options at 0: the multi-pass forms on vector lanes
A plain module, not a test file.  The reference of every comparison is the composition of the fp64 oracle functions (reference())."""
import functools
import math

import torch

import oracle.chan_attn as OC

GATES = ("se", "eca", "cbam")
SINGLE = (2, 64, 32, 32)
RAGGED = [(3, 72, 7, 7), (2, 48, 13, 17), (1, 8, 1, 1), (2, 100, 5, 9)]
PARTIAL = (2, 400, 8, 8)
# H*W / 4 / 64 (fp32) -> 1, 2, 4, 8, 13, 16;  H*W / 8 / 64 (16-bit) -> 1, 1, 2, 4, 7, 8
SLOTS = [(2, 16, 16, 16), (2, 16, 16, 32), (1, 16, 32, 32), (1, 16, 32, 64), (2, 32, 56, 56), (1, 32, 64, 64)]
MULTI = (2, 512, 28, 28)
SINGLE_OFF = dict(se_single=0, eca_single=0, cbam_single=0)

# (shape, library options): every case of the table
CASES = [(SINGLE, {})] + [(s, {}) for s in RAGGED] + [(PARTIAL, {})] + [(s, {}) for s in SLOTS] + [(MULTI, SINGLE_OFF)]
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def case_id(case):
    shape, opts = case
    return "x".join(map(str, shape)) + ("_multi" if opts else "")


def build(gate, C):
    """The drop-in module of `gate` for C channels with seeded, non-trivial parameters (fp32, CPU)."""
    from mi355attn.modules import CBAM, ECALayer, SELayer
    torch.manual_seed(1234 + C)
    red = 16 if C >= 32 else 4
    m = {"se": lambda: SELayer(C, red), "eca": lambda: ECALayer(C), "cbam": lambda: CBAM(C, red)}[gate]().eval()
    g = torch.Generator().manual_seed(99 + C)
    with torch.no_grad():
        for p in m.parameters():
            fan = p[0].numel()
            p.copy_(torch.randn(p.shape, generator=g) * (1.5 / math.sqrt(max(fan, 1))))
    return m


@functools.lru_cache(maxsize=None)
def inputs(shape, dtype, seed=4321):
    """(x, resid) on the CPU in `dtype`; the tests must not modify what this returns."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g).to(dtype)
    r = (torch.randn(*shape, generator=g) * 0.7).to(dtype)              # about a third of x * gate + resid comes out negative
    return x, r


def gate64(gate, m, x, dtype=torch.float64):
    """gate(x) of module m by the oracle, evaluated in `dtype` (fp64: the reference; fp32: its restatement)."""
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    x = x.to(dtype)
    if gate == "se":
        return OC.se_forward(x, sd["fc.0.weight"], sd["fc.2.weight"], dtype)
    if gate == "eca":
        return OC.eca_forward(x, sd["conv.weight"], dtype)
    return OC.cbam_forward(x, sd["ca.fc.0.weight"], sd["ca.fc.2.weight"], sd["sa.conv.weight"], dtype)


def reference(gate, m, x, resid, relu, dtype=torch.float64):
    """relu(OC.<gate>_forward(x.double(), ...) + resid.double()): the composition of the existing oracle functions."""
    s = gate64(gate, m, x, dtype) + resid.to(dtype)
    return torch.relu(s) if relu else s
