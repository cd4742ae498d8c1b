"""Case table of SKLayer on the matrix-core branch kernel (csrc/sk_wide.hip): planes / groups outside {1, 2, 4, 8, 16}, which
mi355_sk_fwd refused before, on the smallest shapes that reach each way that kernel can go wrong.

Protocol: the module is built under seed 1234; then every parameter and BatchNorm buffer is perturbed (perturb) so that no folded term
is an identity: conv / fc weights by half their own spread, conv and fc biases, BatchNorm gains and shifts by 0.2 * randn, running
means 0.2 * randn, running variances 1 + rand.  x is randn under seed 4321.  Truth is oracle.sk_forward in fp64.  The scales keep the
outputs at |y| <= about 2.5, because tests/test_sk_wide_cpu.py holds the oracle to an ABSOLUTE 1e-6 of the reference module's own fp32
evaluation, whose rounding error is about 3e-7 of the largest output.

TOL is the project's strict-mode bar (TOL[0] of tests/arena_cases.py): the branches run in the fp32-class split-bf16 operand format."""
import importlib

import torch

import oracle as O

WEIGHT_SEED, INPUT_SEED = 1234, 4321
TOL = 5e-5
WIDE_TAG = "sk_wide_kernel"

# id, (inplanes, planes), groups, x shape, what the row reaches
CASES = [
    ("g32x32_tiles", (64, 64), 2, (2, 64, 9, 12), "32 x 32 groups, several row tiles; the SKNet stage-4 group in small"),
    ("g32x32_ragged", (64, 64), 2, (2, 64, 7, 7), "ragged row ends, W % 4 != 0"),
    ("g32x32_1x1", (64, 64), 2, (2, 64, 1, 1), "a map smaller than the dilation: eight of nine taps are padding"),
    ("g32x32_2x3", (64, 64), 2, (2, 64, 2, 3), "a map smaller than the dilation"),
    ("one_group_40", (24, 40), 1, (2, 24, 6, 8), "output channels padded 40 -> 48, one group"),
    ("g3x5", (36, 60), 12, (3, 36, 5, 7), "3 in / 5 out per group: channel octet and output tile mostly padding"),
    ("g2x32", (64, 1024), 32, (1, 64, 5, 6), "2 in / 32 out per group, d = 64"),
    ("chunked_512", (512, 64), 1, (1, 512, 6, 40), "input channels in at least two chunks"),
    ("three_bands", (96, 96), 3, (2, 96, 40, 8), "at least three bands, H no multiple of the band height"),
    ("sknet_last", (1024, 1024), 32, (2, 1024, 7, 7), "SKNet's last SK unit as the reference builds it"),
    ("col_bands_chunk_tail", (40, 24), 1, (1, 40, 5, 70), "W above 64: two column bands; 40 input channels in chunks of 24 + 16"),
]
IDS = [c[0] for c in CASES]
BY_ID = {c[0]: c for c in CASES}

# the golden shapes the FMA kernels cover (tests/golden/cases.py sk64, sk_ragged): run on the new kernel with options(sk_wide=1)
COVERED = [
    ("covered_sk64", (64, 64), 32, (2, 64, 32, 32), "planes / groups = 2, four bands"),
    ("covered_ragged", (48, 96), 12, (3, 48, 9, 11), "planes / groups = 8, W % 4 != 0"),
]
COVERED_IDS = [c[0] for c in COVERED]
BY_ID.update({c[0]: c for c in COVERED})


def perturb(module):
    g = torch.Generator().manual_seed(WEIGHT_SEED + 1)
    with torch.no_grad():
        for p in module.parameters():
            if p.dim() > 1:
                p.add_(0.5 * float(p.std()) * torch.randn(p.shape, generator=g))
            else:
                p.add_(0.2 * torch.randn(p.shape, generator=g))
        for m in module.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(1.0 + torch.rand(m.num_features, generator=g))
    return module


def module(case, cls=None):
    """The drop-in SKLayer of the case (or `cls`, e.g. the reference's class) on the CPU, eval mode, perturbed."""
    _, args, groups, _, _ = case
    if cls is None:
        cls = importlib.import_module("attention_mechanisms.sk_module").SKLayer
    with torch.random.fork_rng():
        torch.manual_seed(WEIGHT_SEED)
        m = cls(*args, groups=groups).eval()
    return perturb(m)


def input_of(case):
    return torch.randn(*case[3], generator=torch.Generator().manual_seed(INPUT_SEED))


_TRUTH = {}


def truth(case):
    """fp64 oracle of the case, computed once per process and shared (callers must not modify it)."""
    if case[0] not in _TRUTH:
        _TRUTH[case[0]] = O.sk_forward(input_of(case), module(case).state_dict(), case[2], torch.float64)
    return _TRUTH[case[0]]
