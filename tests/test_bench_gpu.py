"""bench.py and the measuring tools around it, end to end with the real kernels:

  * a plain run times exactly --steps steps and --dump-outputs is reproducible;
  * `--gpus 2 --dist-backend gloo`: the whole N > 1 path (self-launch, barrier-bracketed windows, ranks_seen, host-staged gather) with
    two ranks sharing the one visible GPU;
  * bench.make_comm: the C-ABI communicator self-test passes, and a construction that never returns times out without hanging;
  * a ragged batch gathered over a gloo group from device tensors;
  * the in-process kernel tally (mi355_trace_begin / mi355_trace_end): a refused launch leaves no phantom tag, a report longer than the
    caller's buffer is handed out whole;
  * the MFMA yardstick of the bench line.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_plain_run_times_its_steps_and_dumps_outputs(tmp_path):
    """A plain bench.py run (no --full): the headline keys only, exactly --steps timed steps, and --dump-outputs writes the last timed
    step's outputs, the same values on a second run with the same arguments."""
    import numpy as np
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    lines = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c2", "--batch", "4", "--steps", "3",
               "--warmup", "1", "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert "roofline" not in line and "cpu_baseline" not in line
    assert sorted(os.listdir(tmp_path / "a")) == ["CBAM.npy", "ECA.npy", "SE.npy"]
    for n in ("SE", "CBAM", "ECA"):
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype == np.float32 and a.size == min(4 * 256 * 56 * 56, bench.DUMP_ELEMS) and np.isfinite(a).all()
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6), n


@pytest.mark.parametrize("workload,first_key", [("c5", "ViTBase"), ("c2", "SE")])
def test_bench_two_ranks_share_one_gpu_on_gloo(workload, first_key):
    """c5: the end-of-forward gather path; c2 (round 6): the single-read SE / CBAM exchange kernels of two processes share the GPU -- each
    launch polls for peer workgroups of its own grid while the other rank's grid occupies CUs."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "4"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--workload", workload, "--batch", "16",
           "--steps", "2", "--warmup", "1", "--full", "--no-cpu", "--no-strict", "--no-calib"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    # two ranks on ONE GPU: a launch-path run, reported as such -- n_gpus counts distinct devices
    assert line["n_gpus"] == 1 and line["scaling"].startswith("none") and line["config"]["distinct_gpus"] == 1
    assert line["config"]["ranks_seen"] == 2 and len(line["ms_per_step_by_rank"]) == 2
    assert line["config"]["dist_backend"] == "gloo" and "gloo" in line["config"]["gather"]
    assert len(line["ms_windows"]) == 3 and line["value"] > 0
    assert line["blocks"][0]["key"] == first_key


def test_bench_comm_selftest_passes_and_times_out_without_hanging(monkeypatch):
    """bench.make_comm: the C-ABI communicator self-test runs on a helper thread with a deadline; the verdict is an all-reduce over the
    torch.distributed group.  One rank, nccl backend: the real communicator passes; a construction that never returns is reported as a
    time-out and the caller falls back (on an 8-GPU node a stuck RCCL bootstrap must not hang the scaling run)."""
    import socket
    import time
    import torch.distributed as dist
    import bench
    import mi355attn.dist as mdist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        dev = torch.device("cuda", 0)
        comm, why = bench.make_comm(dist, dev, 0, 1, timeout_s=60.0)
        assert comm is not None and why is None, why
        got = comm.all_gather(torch.ones(2, 3, device=dev))
        assert got.shape == (2, 3)
        comm.close()

        class Stuck:
            def __init__(self, *a, **k):
                time.sleep(30)
        monkeypatch.setattr(mdist, "RcclComm", Stuck)
        t0 = time.time()
        comm, why = bench.make_comm(dist, dev, 0, 1, timeout_s=1.0)
        assert comm is None and "timed out" in why and time.time() - t0 < 10
    finally:
        dist.destroy_process_group()


# ---- ragged gather over gloo from device tensors ------------------------------------------------------------------------------------
_RAGGED = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.path.join({root!r}, "pytorch-attention_amd"))
from mi355attn.dist import forward_sharded
from mi355attn.modules import SELayer
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
torch.manual_seed(1234)
m = SELayer(64).eval().cuda()
torch.manual_seed(4321)
x = torch.randn(5, 64, 16, 16, device="cuda")                # 5 images over 2 ranks: 3 + 2
with torch.no_grad():
    y = forward_sharded(m, x)
    full = m(x)
assert y.is_cuda and tuple(y.shape) == tuple(full.shape) and torch.equal(y, full), (y.shape, full.shape)
dist.barrier()
dist.destroy_process_group()
print("RAGGED_OK", rank)
"""


def test_ragged_gather_over_gloo_with_device_tensors(tmp_path):
    script = tmp_path / "ragged.py"
    script.write_text(_RAGGED.format(root=ROOT))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29733", str(script)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.count("RAGGED_OK") == 2, (r.stdout[-1500:], r.stderr[-3000:])


# ---- the kernel tally and the MFMA yardstick ----------------------------------------------------------------------------------------
def test_trace_has_no_phantom_tags_and_long_reports_survive():
    """A launch the two-accumulator kernel refuses (K too short for its fp32 epilogue) must not leave a tag; a report longer than the
    caller's buffer is kept by the library and handed out whole on the second call."""
    import mi355attn
    from mi355attn import _ffi
    from mi355attn import functional as F
    x16 = torch.randn(512, 384, device="cuda").half()
    w16 = torch.randn(256, 384, device="cuda").half()
    res = torch.randn(512, 256, device="cuda")

    def run():
        F.linear16(x16, w16, None, resid=res, precision=1)            # fp32 out + residual, K = 384 < 640: not gemm16_pa's shape
    rows = mi355attn.kernel_trace(run)
    assert len(rows) == 1 and rows[0][1] == 1, rows                   # exactly one kernel ran, exactly one tag with one launch
    assert all(mn > 0.5 for _, _, _, mn, _ in rows), rows             # no near-zero phantom interval
    # long report: many distinct tags through a 64-byte buffer
    L = _ffi.lib()
    assert L.mi355_trace_begin() == 0
    for k in (64, 128, 192, 256, 320):
        F.linear16(torch.randn(256, k, device="cuda").half(), torch.randn(64, k, device="cuda").half(), None, out16=True, precision=1)
    torch.cuda.synchronize()
    small = ctypes.create_string_buffer(64)
    need = L.mi355_trace_end(small, 64)
    assert need > 64
    big = ctypes.create_string_buffer(need + 1)
    assert L.mi355_trace_end(big, need + 1) == need
    lines = big.value.decode().splitlines()
    assert len(lines) == 5 and all(len(l.split("\t", 4)) == 5 for l in lines), lines
    assert big.value.decode().startswith(small.value.decode())
    assert L.mi355_trace_end(big, need + 1) == 0                      # handed out whole: dropped


def test_mfma_yardstick_reads_a_sane_rate_and_clock():
    from mi355attn import functional as F
    dev = torch.device("cuda", 0)
    y0 = F.mfma_yardstick(dev, 0, target_ms=10.0)
    y1 = F.mfma_yardstick(dev, 1, target_ms=10.0)
    for y in (y0, y1):
        assert 300.0 < y["TFLOPs"] < 2600.0, y                        # between a badly throttled part and the 2.5 PF nameplate
    assert 500.0 < y1["sclk_MHz_issue"] < 2500.0, y1
    if y1["sclk_MHz_counter"]:
        assert 50.0 < y1["sclk_MHz_counter"] < 3000.0, y1
