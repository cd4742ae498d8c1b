"""Rows of the ABI memory-contract harness (tests/arena.py, tests/test_abi_memory_gpu.py) for the four 16-bit entries of the axis gates:
mi355_coordatt16_fwd, mi355_triplet16_fwd, mi355_attention_gate16_fwd and mi355_bam16_fwd (csrc/axis_attn.hip on the kernels of
csrc/axis_attn_io16.hip).  A wide shape (16-byte lanes everywhere) and one that is ragged in every dimension, both I/O types; the
drop-in modules run with their parameters, BatchNorm statistics and input in the arena.

Importing this module appends the rows to the table of tests/arena_cases.py through its own row() helper, once, so that the table's
coverage checks (tests/test_abi_memory_cpu.py) see them in any run that collects the test files that import it
(tests/test_axis_io16_cpu.py, tests/test_axis_io16_arena_gpu.py); the latter runs them through the harness."""
import torch

import arena_cases
import oracle.axis_attn as OA
from arena_cases import TOL, row

IDS = []
SHAPES = ((2, 64, 32, 32), (3, 40, 13, 70))
F64 = torch.float64


def seeded(m, seed):
    """Parameters and BatchNorm statistics moved off their defaults by O(1) amounts (the defaults make every BatchNorm the identity)."""
    g = torch.Generator().manual_seed(seed)
    m = m.eval()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=g))
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                mod.running_mean.copy_(0.2 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
    return m


def build(kind, C, ks=7):
    """A seeded drop-in module of one of the four kinds: "coord", "triplet", "gate" (AttentionGate on its own), "bam"."""
    from mi355attn.modules import BAM, CoordinateAttention, TripletAttention
    from mi355attn.modules.axis import AttentionGate
    torch.manual_seed(1234)
    m = {"coord": lambda: CoordinateAttention(C, C), "triplet": lambda: TripletAttention(ks), "gate": lambda: AttentionGate(ks),
         "bam": lambda: BAM(C)}[kind]()
    return seeded(m, 77)


def reference(kind, x16, sd):
    """fp64 oracle of a host 16-bit x and the module's state_dict."""
    if kind == "coord":
        return OA.coordatt_forward(x16.double(), sd, dtype=F64)
    if kind == "triplet":
        return OA.triplet_forward(x16.double(), sd, dtype=F64)
    if kind == "bam":
        return OA.bam_forward(x16.double(), sd, 4, dtype=F64)
    return OA._attention_gate(x16.double(), {"g." + k: v for k, v in sd.items()}, "g", F64)      # triplet_attention.py:45-49


ENTRY = {"coord": "mi355_coordatt16_fwd", "triplet": "mi355_triplet16_fwd", "gate": "mi355_attention_gate16_fwd", "bam": "mi355_bam16_fwd"}


def _register():
    for shape in SHAPES:
        sid = "x".join(map(str, shape))
        for dt, p in ((torch.float16, 1), (torch.bfloat16, 2)):
            for kind, sym in ENTRY.items():
                def make(seed, kind=kind, shape=shape, dt=dt):
                    g = torch.Generator().manual_seed(seed)
                    return dict(m=build(kind, shape[1]), x=torch.randn(*shape, generator=g).to(dt))

                def run(F, d):
                    with torch.no_grad():
                        return d["m"](d["x"])

                def ref(d, kind=kind):
                    return reference(kind, d["x"], d["m"].state_dict())
                IDS.append(f"{kind}16_{sid}_p{p}")
                row(id=IDS[-1], entries=(sym,), prec=p, tol=TOL[p], make=make, run=run, ref=ref, module=True)
    arena_cases.BY_ID.update({r["id"]: r for r in arena_cases.ROWS if r["id"] in IDS})


_register()
