"""Kernel metadata of the software-pipelined weight-stationary GEMM (gemm16_wst.hip): 256 AGPRs of weights + a full VGPR file leave no room
for a spill -- a scratch access inside the hand-ordered instruction stream would also join the kernel's counted vmcnt waits."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_wst1_instantiation_runs_without_scratch(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources                                            # needs msgpack: a missing package fails this test, it does not skip it
    rows = [r for r in kernel_resources.kernels(built_lib) if "gemm16_wst1_kernel" in r["name"]]
    assert len(rows) == 4, [r["name"] for r in rows]                   # fp16 / bf16 x plain / GELU
    for r in rows:
        assert r["scratch"] == 0 and not r["spill_v"] and not r["spill_s"], (r["name"], r["scratch"], r["spill_v"], r["spill_s"])
        assert r["agpr"] == 256 and r["lds"] <= 160 * 1024, (r["name"], r["agpr"], r["lds"])
