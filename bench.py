#!/usr/bin/env python
"""bench.py -- forward throughput of the MI355X hot path, one JSON line on rank 0.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload all|c2|c3|c4|c5|mixer|da|...] [--dump-outputs DIR] [--full [--no-cpu]]

A plain run sets up, warms up, times exactly K steps, writes the last timed step's outputs when --dump-outputs is given, and prints
the line: `metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, plus the run's `config` (workload, precision,
ranks).  Everything else described below -- box calibration, the two drift windows, per-block timing and the roofline, the strict
passes, the model passes, the dominant-kernel tally and the CPU baseline -- runs only with `--full`.

`--gpus N` with N > 1 and no WORLD_SIZE in the environment re-executes itself under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...`
(one rank per GPU over RCCL); launched that way by somebody else it just reads RANK / LOCAL_RANK / WORLD_SIZE.

Default workload "all" = every north-star target in ONE step (BASELINE.json configs[1..4] at B = 256 images per GPU):
  C2  SELayer(256), CBAM(256), ECALayer(256)        x = (256,256,56,56) fp32                      HBM-bound
  C3  ViT Attention(768, heads 12)                  x = (256,197,768)                              MFMA-bound
  C4  CSWinBlock s1..s4, XCABlock(384,8), XCA       x = (256,3136,64) ... (256,49,512), (256,196,384)
  +   DoubleAttention(64,32,32) @ (256,64,32,32), DoubleAttention(256,128,128) @ (256,256,56,56), MixerLayer(512,196) @ (256,196,512):
      the remaining class-surface rows of north_star (no BASELINE config of their own; round 3)
  C5  VisionTransformer ViT-Base/16                 x = (256,3,224,224); logits all-gathered over RCCL when N > 1
One "step" = one forward of each block over the per-GPU batch (inputs resident in HBM, H2D excluded).  `value` = images/s through
the whole step, aggregated over all ranks (weak scaling: per-GPU batch fixed, batch-sharded, no data-path collective except the
end-of-forward all-gather of the ViT logits).  Every block gets its own roofline entry in `config.blocks` (achieved = algorithmic
bytes or FLOPs of the block / its average duration measured with HIP events on the launch stream); the top-level
`roofline` is the one of the slowest block of the step.  `cpu_baseline` = the oracle (torch-CPU restatement of the reference
forward; /root/reference does not exist on the GPU box) timed on this host's cores on a bounded sample of the same step
(rank 0, N = 1 only).

Shape of the line (round 5; the driver's record keeps scalar leaves and a ~9 KB tail, so everything that must survive is a SCALAR and the
line stays under 8 KB): `config.ms_<key>` / `config.frac_<key>` / `config.strict_ms_<key>` for every block (keys SE, CBAM, ECA, ViTAttn,
CSWin_s1..s4, XCABlock, XCA, DA64, DA256, Mixer, ViTBase); `config.ms_window_1..3` = THREE consecutive windows of --steps steps, each
between barrier + synchronize pairs (`ms_per_step` / `value` are window 1, the contract's timed region; 2 and 3 show drift of a cold or
power-managed box); box calibration before and after the timed region: `config.stream_copy_GBps_{before,after}`,
`config.mfma_{16x16x32,32x32x16}_TFLOPs_{before,after}` (register-operand MFMA loops: what THIS box's matrix pipes sustain),
`config.sclk_MHz_{counter,issue}_*` (shader clock under that load, two independent readings) and `config.smi_{idle,load}_*` (clock /
power / temperature from sysfs or amd-smi, idle and while windows 2-3 run).  The per-block list is the LAST key; `--detail FILE` writes
the verbose records (per-kernel tally table, CPU probe times, calibration) next to the line.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "pytorch-attention_amd"))
sys.path.insert(0, ROOT)

T_START = time.perf_counter()
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8.0 TB/s spec
MFMA_PEAK_TFLOPS = 2500.0    # dense bf16/fp16 MFMA


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="all")
    ap.add_argument("--batch", type=int, default=256, help="images per GPU")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: box calibration, drift windows, per-block timing + roofline, strict "
                         "and model passes, dominant-kernel tally, CPU baseline (the --no-* switches below apply to these)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write each block's output of the last timed step to DIR/<key>.npy (float32; outputs above "
                         "the size cap as a fixed, seeded sample of their elements)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline leg")
    ap.add_argument("--no-strict", action="store_true", help="skip the per-block strict-mode (fp32-class) timing passes")
    ap.add_argument("--cpu-sample", type=int, default=None, help="override the per-block CPU-baseline sample size (images)")
    ap.add_argument("--chunk-images", type=int, default=None, help="override the Infinity-Cache chunk size")
    ap.add_argument("--nt", type=int, default=None, help="channel-attention final pass: bit0 NT loads, bit1 NT stores")
    ap.add_argument("--reverse", type=int, default=None, help="channel-attention final pass walks the batch backwards")
    ap.add_argument("--precision", type=int, default=None, help="MFMA operand precision 0 strict / 1 fp16 / 2 bf16")
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE", help="mi355_set_option override (tuning experiments)")
    ap.add_argument("--only", default=None, help="keep only the blocks of the workload whose name contains this text (profiling aid)")
    ap.add_argument("--gather", default="auto", choices=("auto", "capi", "torch"),
                    help="end-of-forward all-gather of the ViT logits: 'capi' = mi355_allgather_f32 (RCCL behind the C ABI), 'torch' = "
                         "torch.distributed all_gather_into_tensor, 'auto' (default) = capi when its start-up self-test passes on every "
                         "rank, else torch -- the choice is reported in config.gather")
    ap.add_argument("--dist-backend", default="nccl", choices=("nccl", "gloo"),
                    help="process-group backend for N > 1: 'nccl' (= RCCL over xGMI, one GPU per rank: the default and what a multi-GPU node "
                         "runs) or 'gloo' (host-side barrier / max-reduce / gather; ranks may SHARE a GPU, rank r uses GPU r mod visible: lets "
                         "the whole N > 1 path -- self-launch, barrier-bracketed timing, ranks_seen, end-of-forward gather -- run end to end "
                         "with the real kernels on a one-GPU box)")
    ap.add_argument("--no-calib", action="store_true", help="skip the box calibration (MFMA / copy yardsticks, telemetry)")
    ap.add_argument("--no-models", action="store_true",
                    help="skip the model-level passes of the default workload (CSWin-T, XCiT-nano, MLP-Mixer full forwards, un-timed: roofline.model_ms)")
    ap.add_argument("--detail", default=None, help="also write the line + the verbose per-block / per-kernel / CPU-leg records to this JSON file")
    ap.add_argument("--launch-check", action="store_true",
                    help="rendezvous + barrier + max-reduce of an empty step on the gloo backend, no GPU work: what the CPU tests "
                         "use to check that --gpus N really runs N ranks")
    return ap.parse_args(argv)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args, argv):
    """--gpus N > 1 outside a torchrun environment: become the launcher (one rank per GPU) instead of measuring one GPU."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


def host_cpu_info():
    """(physical cores, hardware threads, model name) of this host."""
    threads = os.cpu_count() or 1
    cores, model = set(), None
    try:
        phys = core = None
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name") and model is None:
                    model = line.split(":", 1)[1].strip()
                elif line.startswith("physical id"):
                    phys = line.split(":", 1)[1].strip()
                elif line.startswith("core id"):
                    core = line.split(":", 1)[1].strip()
                elif not line.strip():
                    if phys is not None and core is not None:
                        cores.add((phys, core))
                    phys = core = None
    except OSError:
        pass
    return (len(cores) or threads), threads, model


def _seeded(ctor, seed=1234):
    import torch
    torch.manual_seed(seed)
    return ctor().eval()


def csrc_fingerprint():
    """sha256 over the kernel sources (csrc/*.hip, *.h, the public header), first 16 hex digits: what a PMC traffic table was measured
    against.  (The GPU box gets the tree without .git, so a commit id is not available there; the source hash is.)"""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "pytorch-attention_amd", "csrc", "*.hip")) +
                   glob.glob(os.path.join(ROOT, "pytorch-attention_amd", "csrc", "*.h")) + [os.path.join(ROOT, "include", "mi355attn.h")])
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def load_pmc_traffic():
    """(block name -> bytes below L2 per forward, note).  profiles/pmc_traffic.json is produced by separate rocprofv3 --pmc passes
    (tools/gpu_round3.sh) and stamped with csrc_fingerprint(); a table measured against other kernel sources is NOT relayed."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(path):
        return {}, "no profiles/pmc_traffic.json"
    try:
        tab = json.load(open(path))
    except Exception as e:                                   # noqa: BLE001
        return {}, "unreadable profiles/pmc_traffic.json: %s" % e
    have, want = tab.get("_csrc_sha16"), csrc_fingerprint()
    if have != want:
        return {}, "stale: profiles/pmc_traffic.json was measured at csrc %s, this tree is %s -- traffic not reported" % (have, want)
    return dict(tab.get("all", {})), "PMC FETCH_SIZE x 2 + WRITE_SIZE per block forward (separate rocprofv3 passes, tools/gpu_round5_final.sh) at csrc %s" % want


# ------------------------------------------------------------------------------------------------------------
# workloads: each returns dict(name, blocks, dtype); a block = dict(name, module, x, fwd_args, bound "hbm"|"mfma",
#            work = algorithmic bytes or FLOPs per call, cpu(callable on a host sample), cpu_n, gather)
# ------------------------------------------------------------------------------------------------------------
def workload_c2(B, dev):
    import torch
    from mi355attn.modules import CBAM, ECALayer, SELayer
    from oracle import aten_seq as A
    C, H, W = 256, 56, 56
    torch.manual_seed(4321)
    x = torch.randn(B, C, H, W, device=dev)
    nbytes = 2 * B * C * H * W * 4                      # read x once + write y once
    se, cb, ec = _seeded(lambda: SELayer(C)), _seeded(lambda: CBAM(C)), _seeded(lambda: ECALayer(C))

    sds = [{k: v.detach().cpu() for k, v in m.state_dict().items()} for m in (se, cb, ec)]
    note = "ATen-operator-sequence restatement of the reference forward (oracle/aten_seq.py)"
    blocks = [
        dict(name="SELayer(256)", key="SE", module=se.to(dev), x=x, bound="hbm", work=nbytes, cpu=lambda xs: A.se_aten(xs, sds[0]), cpu_n=64, cpu_note=note),
        dict(name="CBAM(256)", key="CBAM", module=cb.to(dev), x=x, bound="hbm", work=nbytes, cpu=lambda xs: A.cbam_aten(xs, sds[1]), cpu_n=64, cpu_note=note),
        dict(name="ECALayer(256)", key="ECA", module=ec.to(dev), x=x, bound="hbm", work=nbytes, cpu=lambda xs: A.eca_aten(xs, sds[2]), cpu_n=64, cpu_note=note),
    ]
    return dict(name="SELayer+CBAM+ECALayer fwd, x=(%d,256,56,56) fp32 per GPU (BASELINE configs[1])" % B,
                blocks=blocks, dtype="f32")


def workload_all(B, dev):
    """BASELINE.json configs[1..4] in one step: C2 + C3 + C4 + C5 (module docstring)."""
    import bench_workloads as W
    parts = [workload_c2(B, dev), W.workload_c3(B, dev), W.workload_c4(B, dev), W.workload_da(B, dev), W.workload_mixer(B, dev),
             W.workload_c5(B, dev)]
    blocks = [b for p in parts for b in p["blocks"]]
    return dict(name="north-star step: C2 SE+CBAM+ECA, C3 ViT-Attn, C4 CSWin s1-4 + XCABlock + XCA, DA x2, Mixer, C5 ViT-Base fwd; B=%d/GPU" % B,
                blocks=blocks, dtype="f32/f16")


WORKLOADS = {"c2": workload_c2, "all": workload_all}


def _extra_workloads():
    import bench_workloads
    for k, v in bench_workloads.WORKLOADS.items():
        WORKLOADS.setdefault(k, v)


def launch_check(args, rank, world):
    """No GPU work: prove the launch path (N ranks, barrier-bracketed timing, max over ranks) on the gloo backend."""
    import torch
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pass
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        ranks = [None] * world
        dist.all_gather_object(ranks, rank)
    else:
        ranks = [0]
    if rank == 0:
        print(json.dumps({"metric": "launch check (no GPU work)", "value": 0.0, "unit": "images/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / max(args.steps, 1) * 1e3, 6),
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "ranks_seen": sorted(ranks),
                          "config": {"workload": "launch-check"}}))
    if world > 1:
        dist.destroy_process_group()


def yardsticks(dev, src):
    """Box calibration: float4 streaming copy of the C2 footprint + the register-operand MFMA loops (both instruction shapes),
    each ~40 ms.  Flat scalars."""
    import torch
    from mi355attn import StreamTimer
    from mi355attn import functional as F
    out = {}
    if src is not None and src.numel() * 4 % 16 == 0 and src.numel() * 4 >= (1 << 26):
        dst = torch.empty_like(src)
        F.stream_copy(src, dst)
        torch.cuda.synchronize()
        tm = StreamTimer(dev)
        tm.start()
        for _ in range(10):
            F.stream_copy(src, dst)
        cms = tm.stop_ms() / 10
        out["stream_copy_GBps"] = round(2 * src.numel() * 4 / (cms * 1e-3) / 1e9, 1)
        del dst
    y0 = F.mfma_yardstick(dev, 0)
    y1 = F.mfma_yardstick(dev, 1)
    out.update({"mfma_16x16x32_TFLOPs": y0["TFLOPs"], "mfma_32x32x16_TFLOPs": y1["TFLOPs"], "sclk_MHz_counter": y1["sclk_MHz_counter"],
                "sclk_MHz_issue": y1.get("sclk_MHz_issue")})
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args, argv))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.launch_check:
        return launch_check(args, rank, world)

    import torch
    import bench_telemetry as tele
    _extra_workloads()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: torch.cuda.is_available() is False (no CPU fallback exists)")
    ndev = torch.cuda.device_count()
    shared_gpu = args.dist_backend == "gloo"                 # ranks may share a GPU (host-side collectives): N > visible GPUs is allowed
    if ndev < world and not shared_gpu:
        raise SystemExit(f"--gpus {world} but only {ndev} GPU(s) visible (use --dist-backend gloo to let ranks share a GPU)")
    dev_index = local_rank % ndev
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if shared_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    import mi355attn
    from mi355attn import StreamTimer
    if args.chunk_images is not None:
        mi355attn.set_option("chunk_images", args.chunk_images)
    if args.nt is not None:
        mi355attn.set_option("nt", args.nt)
    if args.reverse is not None:
        mi355attn.set_option("reverse", args.reverse)
    for kv in args.opt:
        key, _, val = kv.partition("=")
        mi355attn.set_option(key, int(val))
    if args.precision is not None:
        mi355attn.set_default_precision(args.precision)

    comm, gather_kind, comm_ok = None, "none (single rank)", False
    if dist is not None and shared_gpu:
        gather_kind = "gloo all_gather staged through the host (--dist-backend gloo)"
    elif dist is not None:
        gather_kind = "torch.distributed all_gather_into_tensor (RCCL)"
        if args.gather in ("auto", "capi"):
            comm, why = make_comm(dist, dev, rank, world)
            if comm is not None:
                comm_ok = True
                gather_kind = "mi355_allgather_f32 (RCCL behind the C ABI)"
            elif args.gather == "capi":
                raise SystemExit("--gather capi: " + why)
            else:
                gather_kind += " [C-ABI communicator self-test failed: %s]" % why[:60]

    wl = WORKLOADS[args.workload](args.batch, dev)
    wname, blocks = wl["name"], wl["blocks"]
    if wl.get("gather") is not None:                      # whole-workload gather (full-model workloads): applies to every block
        for b in blocks:
            b.setdefault("gather", True)
    if args.only:
        blocks = [b for b in blocks if args.only in b["name"]]
        wname += " [only: %s]" % args.only
        if not blocks:
            raise SystemExit("--only matched no block")
    for b in blocks:
        b.setdefault("key", "".join(c for c in b["name"].split("(")[0] if c.isalnum()))

    def run_block(b):
        y = b["module"](b["x"], *b.get("fwd_args", ()))
        if b.get("gather") and dist is not None:
            from mi355attn.dist import gather_batch
            y = gather_batch(y, comm=comm)                 # one RCCL all-gather over xGMI (1 MB per rank for ViT logits)
        return y

    def step():
        with torch.no_grad():
            return [run_block(b) for b in blocks]

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    last = {}

    def window(keep=False):
        """K steps bracketed by barrier + synchronize on both sides; seconds on this rank.  keep: hold on to the LAST step's outputs
        (only that step's: the steps before it free theirs as they always did)."""
        barrier()
        t0 = time.perf_counter()
        for i in range(args.steps):
            if keep and i == args.steps - 1:
                last["outs"] = step()
            else:
                step()
        barrier()
        return time.perf_counter() - t0

    # ---- box calibration BEFORE the timed region (rank 0 measures, every rank waits): yardsticks + telemetry -------------------------
    calib = {}
    want_calib = args.full and rank == 0 and not args.only and not args.no_calib
    if want_calib:
        card = tele.find_card(tele.pci_address(dev_index))   # the sysfs directory of THIS GPU (a host may list eight cards)
        calib["idle"] = tele.snapshot(card)
        src = blocks[0]["x"].reshape(-1) if blocks[0]["x"].dtype == torch.float32 else None
        calib["before"] = yardsticks(dev, src)

    for _ in range(args.warmup):
        step()
    # THE timed region of the contract: W warm-up steps, then exactly K steps between barrier + synchronize pairs, max over ranks
    elapsed = local_elapsed = window(keep=True)
    if args.dump_outputs and rank == 0:
        dump_outputs(blocks, last.get("outs", []), args.dump_outputs)
    last.clear()
    # two more windows of K steps right behind it (same bracket): drift of a cold / power-managed box shows as a trend across the three
    sampler = tele.LoadSampler(card) if want_calib else None
    if sampler is not None:
        sampler.start()
    extra = [window() for _ in range(2 if args.full and not args.only else 0)]
    if sampler is not None:
        calib["load"] = sampler.stop()

    def max_over_ranks(v):
        if dist is None:
            return v
        t = torch.tensor([v], dtype=torch.float64, device="cpu" if shared_gpu else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    elapsed = max_over_ranks(elapsed)
    extra = [max_over_ranks(e) for e in extra]
    if not args.full:
        return plain_line(args, rank, world, dist, shared_gpu, dev_index, local_elapsed, elapsed, wl, wname, gather_kind, comm, comm_ok)

    # per-block durations with HIP events on the launch stream (un-timed extra passes)
    pmc, pmc_note = load_pmc_traffic()

    def time_block(b, reps):
        with torch.no_grad():
            run_block(b)
        torch.cuda.synchronize()
        tm = StreamTimer(dev)
        tm.start()
        with torch.no_grad():
            for _ in range(reps):
                run_block(b)
        return tm.stop_ms() / reps

    per_block = []
    for b in blocks:
        ms = time_block(b, args.steps)
        if b["bound"] == "hbm":
            ach, peak, unit = b["work"] / (ms * 1e-3) / 1e9, HBM_PEAK_GBS, "GB/s"
        else:
            ach, peak, unit = b["work"] / (ms * 1e-3) / 1e12, MFMA_PEAK_TFLOPS, "TFLOP/s"
        rec = dict(block=b["name"], key=b["key"], ms=round(ms, 4), bound=b["bound"], achieved=round(ach, 1), unit=unit,
                   frac=round(ach / peak, 4), traffic=pmc.get(b["name"]))
        if b.get("alt_work"):                                 # mixed blocks: the FLOP rate next to the HBM figure
            rec["alt_TFLOPs"] = round(b["alt_work"] / (ms * 1e-3) / 1e12, 1)
        # both roofs (VERDICT round 5 missing #5): the HBM side of a block graded on the MFMA roof = its algorithmic
        # activation bytes (x in + y out; `alt_bytes`) and its counter bytes (PMC traffic) over the same duration, as fractions of 8 TB/s
        alg_bytes = b["work"] if b["bound"] == "hbm" else b.get("alt_bytes")
        if alg_bytes:
            rec["alg_bytes"] = int(alg_bytes)
            rec["hbm_frac_alg"] = round(alg_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            if rec["traffic"]:
                rec["hbm_frac_pmc"] = round(rec["traffic"] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                rec["traffic_x"] = round(rec["traffic"] / alg_bytes, 2)
        per_block.append(rec)
    # the fp32-class cost of the MFMA blocks (precision 0: bf16 hi/lo split, three MFMAs per product): a few un-timed passes per block
    if mi355attn.default_precision() != 0 and not args.no_strict and not args.only:
        try:
            mi355attn.set_default_precision(0)
            for b, rec in zip(blocks, per_block):
                if b["bound"] == "mfma" or b.get("alt_work"):
                    rec["strict_ms"] = round(time_block(b, max(3, args.steps // 4)), 4)
        finally:
            mi355attn.set_default_precision(1 if args.precision is None else args.precision)
    dominant = None
    # model-level numbers of the next rows, OUTSIDE the timed step like the strict passes: full forwards
    # of CSWin-T/224, XCiT-nano-12/16 and MLP-Mixer(512, depth 12) at the same batch, rank 0 only, no gather (a collective entered by one rank
    # alone would never return)
    model_ms = {}
    if args.workload == "all" and rank == 0 and not args.only and not args.no_models:
        import bench_workloads as BW
        for key, build in (("CSWinT", BW.workload_cswin), ("XCiTnano", BW.workload_xcit), ("Mixer12", BW.workload_mixer_full)):
            try:
                mb = build(args.batch, dev)["blocks"][0]
                with torch.no_grad():
                    mb["module"](mb["x"])
                torch.cuda.synchronize()
                tm = StreamTimer(dev)
                tm.start()
                reps = max(3, args.steps // 4)
                with torch.no_grad():
                    for _ in range(reps):
                        mb["module"](mb["x"])
                model_ms[key] = round(tm.stop_ms() / reps, 4)
                del mb
                torch.cuda.empty_cache()
            except Exception as e:                                  # noqa: BLE001  (reported, never fatal for the contract's line)
                sys.stderr.write("[bench] model pass %s failed: %s\n" % (key, str(e)[:200]))

    rank_ms, ranks_seen, rank_devs = [round(local_elapsed / args.steps * 1e3, 4)], [rank], [dev_index]
    if dist is not None:
        ms_all = [None] * world
        dist.all_gather_object(ms_all, (rank, round(local_elapsed / args.steps * 1e3, 4), torch.cuda.current_device()))
        ranks_seen = sorted(r for r, _, _ in ms_all)
        rank_ms = [m for _, m, _ in sorted(ms_all)]
        rank_devs = [d for _, _, d in sorted(ms_all)]
    if comm is not None:
        comm.close()
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    ms_per_step = elapsed / args.steps * 1e3
    value = world * args.batch * args.steps / elapsed
    dom = max(per_block, key=lambda r: r["ms"])
    if not args.only:                                          # --only runs feed the PMC passes: block kernels only
        dominant = dominant_kernel_tally(blocks[per_block.index(dom)], run_block, args, dom["ms"])
    if want_calib:
        calib["after"] = yardsticks(dev, blocks[0]["x"].reshape(-1) if blocks[0]["x"].dtype == torch.float32 else None)

    # ---- the line (round 6): the driver's record keeps the FIRST 24 keys of each dict, scalar leaves only -> assemble_line() orders
    #      every dict so that what must survive comes first (tests/test_bench_units_cpu.py checks the cap on a synthetic record)
    out = assemble_line(dict(
        batch=args.batch, steps=args.steps, warmup=args.warmup, world=world, value=value, ms_per_step=ms_per_step,
        extra_ms=[e / args.steps * 1e3 for e in extra], workload=wname, dtype=wl.get("dtype", "f32"),
        precision=mi355attn.default_precision(), dist_backend="none" if world == 1 else args.dist_backend, gather=gather_kind,
        rccl_self_test=("passed on every rank" if comm_ok else ("not run (single rank)" if world == 1 else
                        ("not run (gloo backend)" if shared_gpu else "FAILED or skipped: see gather"))),
        ranks_seen=len(ranks_seen), distinct_gpus=len(set(rank_devs)) if shared_gpu else world, per_block=per_block, calib=calib,
        pmc_note=pmc_note, dominant=dominant, dom=dom, blocks=blocks, model_ms=model_ms))
    detail = {"ms_per_step_by_rank": rank_ms, "ranks": ranks_seen, "rank_devices": rank_devs, "ms_windows": [round(ms_per_step, 4)] +
              [round(e / args.steps * 1e3, 4) for e in extra], "calibration": calib, "dominant_kernel": dominant, "blocks": per_block}

    sys.stderr.write("[bench] GPU part done %.1f s after start\n" % (time.perf_counter() - T_START))
    if world == 1 and not args.no_cpu:
        cpu, cpu_detail = cpu_baseline(blocks, args)
        out["cpu_baseline"] = cpu
        detail["cpu_blocks"] = cpu_detail
    out["ms_per_step_by_rank"] = rank_ms
    out["ms_windows"] = detail["ms_windows"]
    # the per-block list stays LAST and short (the scalar / string series above carry the same figures; --detail has every field): the line
    # must stay under ~8 KB for readers that keep a bounded tail
    keep = ("block", "key", "ms", "achieved", "unit", "frac", "traffic", "strict_ms", "alt_TFLOPs")
    out["blocks"] = [{k: r[k] for k in keep if k in r} for r in per_block]
    line = json.dumps(out, separators=(",", ":"))
    if args.detail:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(args.detail)), exist_ok=True)
            with open(args.detail, "w") as f:
                json.dump({"line": out, "detail": detail}, f, indent=1)
        except OSError as e:
            sys.stderr.write("[bench] --detail %s not written: %s\n" % (args.detail, e))
    sys.stderr.write("[bench] JSON line: %d bytes%s\n" % (len(line), "" if len(line) < 8192 else "  (WARNING: above 8 KB)"))
    print(line)
    if dist is not None:
        dist.destroy_process_group()


DUMP_BYTES = 60 << 20           # --dump-outputs: all arrays together stay under 64 MB
DUMP_ELEMS = 1 << 20            # per output: a larger one is written as a seeded sample of this many elements (fewer when outputs are many)
DUMP_SEED = 4321


def dump_outputs(blocks, outs, dirname):
    """Write every block's output of the last timed step to DIR/<key>.npy (float32, float64 stays float64).  An output with more
    elements than the per-output cap is written as the elements at a fixed, seeded, sorted set of flat indices (torch.Generator seeded
    with DUMP_SEED, drawn on the CPU: the same indices on every run and every build for the same shape)."""
    import re
    import numpy as np
    import torch
    arrays = []
    for b, y in zip(blocks, outs):
        ys = list(y) if isinstance(y, (list, tuple)) else [y]
        for i, t in enumerate(ys):
            if torch.is_tensor(t):
                arrays.append((b["key"] if len(ys) == 1 else "%s_%d" % (b["key"], i), t))
    cap = max(1, min(DUMP_ELEMS, DUMP_BYTES // 8 // max(1, len(arrays))))
    os.makedirs(dirname, exist_ok=True)
    seen = set()
    for key, t in arrays:
        name = re.sub(r"[^A-Za-z0-9_.-]", "_", key)
        while name in seen:
            name += "_"
        seen.add(name)
        flat = t.detach().reshape(-1)
        if flat.numel() > cap:
            g = torch.Generator().manual_seed(DUMP_SEED)
            idx = torch.randint(0, flat.numel(), (cap,), generator=g).sort().values
            flat = flat[idx.to(flat.device)]
        a = flat.cpu().numpy()
        np.save(os.path.join(dirname, name + ".npy"), a if a.dtype == np.float64 else a.astype(np.float32))


def plain_line(args, rank, world, dist, shared_gpu, dev_index, local_elapsed, elapsed, wl, wname, gather_kind, comm, comm_ok):
    """The line of a plain run (no --full): the headline keys, meaning what they mean in the --full line, plus the run's config."""
    import torch
    import mi355attn
    rank_ms = [round(local_elapsed / args.steps * 1e3, 4)]
    ranks_seen, rank_devs = [rank], [dev_index]
    if dist is not None:
        ms_all = [None] * world
        dist.all_gather_object(ms_all, (rank, rank_ms[0], torch.cuda.current_device()))
        ranks_seen = sorted(r for r, _, _ in ms_all)
        rank_ms = [m for _, m, _ in sorted(ms_all)]
        rank_devs = [d for _, _, d in sorted(ms_all)]
    if comm is not None:
        comm.close()
    if rank == 0:
        distinct = len(set(rank_devs)) if shared_gpu else world
        out = headline(dict(batch=args.batch, steps=args.steps, warmup=args.warmup, world=world, distinct_gpus=distinct,
                            value=world * args.batch * args.steps / elapsed, ms_per_step=elapsed / args.steps * 1e3,
                            dtype=wl.get("dtype", "f32"), precision=mi355attn.default_precision()))
        out["config"] = {"workload": wname, "precision": PRECISION_NAMES[mi355attn.default_precision()], "ranks_seen": len(ranks_seen),
                         "gather": gather_kind, "batch_per_gpu": args.batch, "parallelism": "batch-shard x%d" % world,
                         "dist_backend": "none" if world == 1 else args.dist_backend,
                         "rccl_self_test": ("passed on every rank" if comm_ok else ("not run (single rank)" if world == 1 else
                                            ("not run (gloo backend)" if shared_gpu else "FAILED or skipped: see gather"))),
                         "distinct_gpus": distinct, "full": "off: --full adds calibration, roofline, per-block and CPU-baseline figures"}
        out["ms_per_step_by_rank"] = rank_ms
        line = json.dumps(out, separators=(",", ":"))
        if args.detail:
            try:
                os.makedirs(os.path.dirname(os.path.abspath(args.detail)), exist_ok=True)
                with open(args.detail, "w") as f:
                    json.dump({"line": out, "detail": {"ms_per_step_by_rank": rank_ms, "ranks": ranks_seen, "rank_devices": rank_devs}}, f,
                              indent=1)
            except OSError as e:
                sys.stderr.write("[bench] --detail %s not written: %s\n" % (args.detail, e))
        print(line)
    if dist is not None:
        dist.destroy_process_group()


PRECISION_NAMES = {0: "strict(bf16x3)", 1: "fp16-mfma", 2: "bf16-mfma"}


def headline(m):
    """The top-level keys of the line, shared by the plain and the --full run."""
    shared = m["distinct_gpus"] != m["world"]
    return {
        "metric": "forward images/sec through one step (+ ms/block), B=%d per GPU, 224x224-derived shapes" % m["batch"],
        "value": round(m["value"], 1), "unit": "images/s",
        # ranks that SHARE a GPU (--dist-backend gloo on a one-GPU box) are not an N-GPU result: n_gpus counts distinct devices then
        "n_gpus": m["distinct_gpus"] if shared else m["world"], "steps": m["steps"], "warmup": m["warmup"],
        "ms_per_step": round(m["ms_per_step"], 4), "higher_is_better": True,
        "scaling": "none (%d ranks share %d GPU: launch-path run, not a scaling point)" % (m["world"], m["distinct_gpus"]) if shared else "weak",
        "vs_baseline": None,
        "dtype": m["dtype"] if m["dtype"] in ("f32", "f32/f16") else {0: "bf16x3", 1: "f16", 2: "bf16"}[m["precision"]],
        "data": "synthetic (torch.randn seed 4321; module-default init seed 1234)",
    }


DRIVER_KEYS_PER_DICT = 24       # the driver's BENCH record keeps the first 24 keys of every dict of the line (scalar leaves only)


def _pairs(recs, field, fmt="%.4g"):
    """'SE=0.593,CBAM=0.43,...' of the records that carry `field`: ONE string leaf instead of one key per block."""
    return ",".join("%s=%s" % (r["key"], fmt % r[field]) for r in recs if r.get(field) is not None)


def assemble_line(m):
    """The JSON line from the measured pieces (pure: no GPU, unit-tested).  Order is the contract with the driver's 24-key cap:

      config    workload, precision, ranks_seen, gather | the box yardstick: copy GB/s, two MFMA TFLOP/s, shader clock and power under
                load | ms_<key> of every block (14 in the default step) | ms_windows -- 24 keys; everything after that is for readers of
                the builder-run line (`profiles/r06_bench_all.json`) and may be cut by the driver;
      roofline  the contract's keys for the slowest block + its dominant kernel, then ONE string per per-block series: `fracs` (every
                block on the roof it is graded on), `hbm_fracs` (mixed / MFMA blocks on the HBM roof: algorithmic bytes / counter bytes),
                `traffic_x` (counter bytes over algorithmic bytes), `strict_ms`, `strict_over_fast`, `model_ms` (full forwards of CSWin-T / XCiT-nano /
                MLP-Mixer at the same batch, measured outside the timed step);
      cpu_baseline is ordered by cpu_baseline() itself."""
    per_block, calib = m["per_block"], m["calib"]
    bef, aft, load, idle = calib.get("before", {}), calib.get("after", {}), calib.get("load", {}), calib.get("idle", {})
    cfg = {"workload": m["workload"],
           "precision": PRECISION_NAMES[m["precision"]],
           "ranks_seen": m["ranks_seen"], "gather": m["gather"],
           "stream_copy_GBps": bef.get("stream_copy_GBps"), "mfma_16x16x32_TFLOPs": bef.get("mfma_16x16x32_TFLOPs"),
           "mfma_32x32x16_TFLOPs": bef.get("mfma_32x32x16_TFLOPs"),
           "sclk_MHz_load": load.get("sclk_MHz_mean", bef.get("sclk_MHz_counter")), "power_W_load": load.get("power_W_mean")}
    for rec in per_block:
        cfg["ms_" + rec["key"]] = rec["ms"]
    cfg["ms_windows"] = "/".join("%.4f" % v for v in [m["ms_per_step"]] + list(m["extra_ms"]))
    # ---- beyond the cap for the default step (14 blocks): kept in builder-run lines -------------------------------------------------
    cfg.update({"batch_per_gpu": m["batch"], "parallelism": "batch-shard x%d" % m["world"], "dist_backend": m["dist_backend"],
                "rccl_self_test": m["rccl_self_test"], "distinct_gpus": m["distinct_gpus"]})
    for k, v in aft.items():
        cfg[k + "_after"] = v
    for k in ("sclk_MHz_counter", "sclk_MHz_issue"):
        if k in bef:
            cfg[k + "_before"] = bef[k]
    for phase, d in (("idle", idle), ("load", load)):
        for k, v in d.items():
            cfg["smi_%s_%s" % (phase, k)] = v
    cfg["traffic_source"] = m["pmc_note"][:110]

    dom, dominant = m["dom"], m["dominant"]
    roof = {"bound": dom["bound"], "achieved": dom["achieved"], "peak": HBM_PEAK_GBS if dom["bound"] == "hbm" else MFMA_PEAK_TFLOPS,
            "unit": dom["unit"], "frac": dom["frac"], "traffic": dom["traffic"], "block": dom["block"],
            "kernel": dominant["name"] if dominant else dom["block"], "ms": dom["ms"]}
    for k in ("avg_us", "achieved", "frac", "share_of_block"):          # the dominant kernel's own figures (in-process HIP-event tally)
        roof["kernel_" + k] = dominant.get(k) if dominant else None
    roof["fracs"] = _pairs(per_block, "frac")
    roof["hbm_fracs"] = ",".join("%s=%.3g/%s" % (r["key"], r["hbm_frac_alg"], ("%.3g" % r["hbm_frac_pmc"]) if r.get("hbm_frac_pmc") else "-")
                                 for r in per_block if r.get("hbm_frac_alg") is not None and r["bound"] != "hbm")
    roof["traffic_x"] = _pairs(per_block, "traffic_x")
    roof["strict_ms"] = _pairs(per_block, "strict_ms")
    roof["strict_over_fast"] = ",".join("%s=%.2f" % (r["key"], r["strict_ms"] / r["ms"]) for r in per_block if r.get("strict_ms"))
    if m.get("model_ms"):                                           # full forwards of the next-row models at the same batch (ms), un-timed passes
        roof["model_ms"] = ",".join("%s=%.4g" % kv for kv in m["model_ms"].items())
    for k in ("launches_per_forward", "us_per_forward", "traced_us_per_forward"):
        if dominant and k in dominant:
            roof["kernel_" + k] = dominant[k]
    roof["legend"] = ("fracs: block time on its graded roof (2.5 PFLOP/s or 8 TB/s); hbm_fracs: algorithmic activation bytes / PMC counter "
                      "bytes over the block time, of 8 TB/s; traffic_x: counter bytes over algorithmic bytes")
    out = headline(m)
    out["config"] = cfg
    # `roofline` grades the slowest BLOCK of the step (a block is many launches: `block` names it, achieved / frac are the block's);
    # `kernel` names the one kernel that takes the largest share of that block, its own figures are the kernel_* keys
    out["roofline"] = roof
    return out


def dominant_kernel_tally(block, run_block, args, ms_block):
    """The kernel that takes the largest share of the slowest block, from an IN-PROCESS tally of that block's OWN launches: the library
    brackets every instrumented launch with HIP events on the launch stream (include/mi355attn.h mi355_trace_begin / _end) while the
    block's forward runs `reps` times; a tag = kernel name + the shape parameters that tell its launches apart.  Returns the per-tag
    table and the dominant KERNEL (tags of one kernel summed), with its own roofline figure when its work is known (GEMM: 2 M N K)."""
    import re
    import torch
    import mi355attn
    reps = max(2, min(5, args.steps))

    def body():                                               # the block's forward WITHOUT the end-of-forward gather: only rank 0 runs this
        with torch.no_grad():                                 # tally, and a collective entered by one rank alone would never return
            for _ in range(reps):
                block["module"](block["x"], *block.get("fwd_args", ()))
        torch.cuda.synchronize()

    rows = mi355attn.kernel_trace(body)
    if not rows:
        return None
    table, by_kernel = [], {}
    for tag, cnt, tot, mn, mx in rows:
        rec = {"tag": tag, "launches_per_forward": round(cnt / reps, 2), "avg_us": round(tot / cnt, 1), "min_us": round(mn, 1),
               "us_per_forward": round(tot / reps, 1)}
        m = re.search(r"M=(\d+) N=(\d+) K=(\d+)", tag)
        if m and tag.startswith("gemm"):
            flop = 2.0 * int(m.group(1)) * int(m.group(2)) * int(m.group(3))
            rec["TFLOPs"] = round(flop / (tot / cnt * 1e-6) / 1e12, 1)
            rec["flop"] = flop
        table.append(rec)
        k = tag.split(" ")[0]
        d = by_kernel.setdefault(k, {"us": 0.0, "launches": 0, "flop": 0.0, "all_flop": True})
        d["us"] += tot / reps
        d["launches"] += cnt / reps
        if "flop" in rec:
            d["flop"] += rec["flop"] * cnt / reps
        else:
            d["all_flop"] = False
    name, d = max(by_kernel.items(), key=lambda kv: kv[1]["us"])
    out = {"name": name, "block": block["name"], "launches_per_forward": round(d["launches"], 2),
           "avg_us": round(d["us"] / d["launches"], 1), "us_per_forward": round(d["us"], 1),
           "share_of_block": round(d["us"] / (ms_block * 1e3), 3),
           "traced_us_per_forward": round(sum(r["us_per_forward"] for r in table), 1),
           "source": "in-process HIP-event tally of the block's own launches (mi355_trace_begin / mi355_trace_end), %d forwards" % reps}
    if d["all_flop"] and d["flop"] > 0:
        ach = d["flop"] / (d["us"] * 1e-6) / 1e12
        out.update({"achieved": round(ach, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_PEAK_TFLOPS, 4)})
    for r in table:
        r.pop("flop", None)
    out["kernels"] = table[:16]
    return out


def make_comm(dist, dev, rank, world, timeout_s=120.0):
    """C-ABI communicator + a self-test all-gather checked on every rank (outside the timed region).  Returns (comm, None) when every
    rank passed, else (None, reason) -- bench.py then gathers through torch.distributed and says so in its JSON line.
    The construction (a host-blocking ncclCommInitRank inside mi355_comm_init) and the self-test run on a helper thread that is given
    `timeout_s`: a rank whose RCCL bootstrap never returns reports "timed out" and every rank falls back together (the verdict is an
    all-reduce over the torch.distributed group, which does not depend on the communicator under test) instead of the job hanging."""
    import threading
    import torch
    state = {"comm": None, "why": "", "abandon": False}

    def build():
        try:
            torch.cuda.set_device(dev)
            from mi355attn.dist import RcclComm
            comm = RcclComm(device=dev, check="never")   # no torch.distributed collective on this thread behind the id broadcast: a rank that
            if state["abandon"]:                          # timed out must not find its peers inside one when it enters the verdict all-reduce
                return
            got = comm.all_gather(torch.full((3, 5), float(rank + 1), device=dev))
            torch.cuda.synchronize()
            want = torch.arange(1, world + 1, dtype=torch.float32, device=dev).repeat_interleave(3)[:, None].expand(-1, 5)
            if not torch.equal(got, want):
                state["why"] = "self-test all-gather returned wrong data on rank %d" % rank
            state["comm"] = comm
        except Exception as e:                               # noqa: BLE001  (reported, not swallowed: see config.gather)
            state["why"] = "%s: %s" % (type(e).__name__, str(e)[:200])

    th = threading.Thread(target=build, name="mi355-comm-selftest", daemon=True)
    th.start()
    th.join(timeout_s)
    if th.is_alive():
        state["abandon"] = True
        state["why"] = "C-ABI communicator self-test timed out after %.0f s on rank %d" % (timeout_s, rank)
    comm, why = state["comm"], state["why"]
    flag = torch.tensor([1.0 if why else 0.0], device=dev)
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    if float(flag.item()) > 0:
        if comm is not None and not why:
            why = "another rank failed"
        return None, why or "failed"
    comm.fix_shape()          # the step gathers one fixed shape: verified on its first (warm-up) call, no host collective in the timed loop
    return comm, None


def cpu_budget():
    """(cpus this process may run on, cgroup quota in cpus or None, source text): `os.cpu_count()` / /proc/cpuinfo describe the HOST; what a
    container may use is its affinity mask and its cgroup cpu.max."""
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = os.cpu_count() or 1
    quota, src = None, "no cgroup cpu limit found"
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                txt = f.read().split()
        except OSError:
            continue
        try:
            if path.endswith("cpu.max"):
                if txt and txt[0] != "max":
                    quota = float(txt[0]) / float(txt[1] if len(txt) > 1 else 100000)
                src = "cgroup v2 cpu.max = %s" % " ".join(txt)
            else:
                q = float(txt[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                        quota = q / float(f.read().split()[0])
                src = "cgroup v1 cfs_quota_us = %s" % txt[0]
        except (ValueError, IndexError, OSError):
            pass
        break
    return aff, quota, src


def cpu_baseline(blocks, args):
    """The reference's CPU path beside the GPU numbers: per block, the ATen-operator-sequence restatement of the reference forward
    (oracle/aten_seq.py, oracle/cswin.py *_aten: /root/reference does not exist on the GPU box, hence kind "port") on this host's cores,
    on the first n images of the same batch (n = 64 for C2 and for ViT-Base -- BASELINE.md 3 -- 32 for the others).

    Round 6: the host is described by what this process may USE (affinity mask, cgroup cpu.max) next to
    /proc/cpuinfo; the (threads x sub-batch) pair is probed jointly -- thread counts {16, 32, 64, 128} capped at the usable cpus, sub-batch 8
    and the whole sample -- one pass per pair inside the block's budget (cheap pairs twice), then the best pair is timed with >= 3 passes and
    the MEDIAN counts (>= 5 passes for blocks under 5 ms, where one pass is timer noise).
    value = images/s through the same step = 1 / sum_b (t_b / n_b).
    Returns (flat record for the line, ordered for the driver's 24-key cap; verbose per-block list for --detail)."""
    import statistics
    import torch
    cores, threads, model = host_cpu_info()
    aff, quota, qsrc = cpu_budget()
    usable = max(1, min(aff, int(quota) if quota and quota >= 1 else aff))
    cands = sorted({min(usable, n) for n in (16, 32, 64, 128)})
    budget_s = float(os.environ.get("MI355_CPU_BLOCK_BUDGET_S", "3"))
    per_image, detail, used = 0.0, [], 0
    with torch.no_grad():
        for b in blocks:
            t_blk = time.perf_counter()
            blk_budget = budget_s * b.get("cpu_budget_x", 1.0)   # full models get a larger share of the leg's time
            ns = min(args.cpu_sample or b.get("cpu_n", 32), b["x"].shape[0])
            xs = b["x"][:ns].cpu()
            torch.set_num_threads(cands[min(1, len(cands) - 1)])
            b["cpu"](xs[:max(1, ns // 8)])                     # first touch of the weights / code paths, small
            subs = [8, ns] if ns >= 16 else [ns]

            def one_pass(sub):
                t1 = time.perf_counter()
                for c0 in range(0, ns, sub):
                    b["cpu"](xs[c0:c0 + sub])
                return time.perf_counter() - t1

            probe = {}
            for sub in subs:                                   # sub-batch 8 first (cache-resident intermediates), then the whole sample
                for nthr in cands:
                    if probe and time.perf_counter() - t_blk > blk_budget:
                        break                                  # budget used: the remaining pairs are not tried, visible in `probe`
                    torch.set_num_threads(nthr)
                    t = one_pass(sub)
                    if t < blk_budget / 20:                    # cheap: a second pass, the faster one counts (thread-pool start-up)
                        t = min(t, one_pass(sub))
                    probe[(nthr, sub)] = t
            best_n, best_sub = min(probe, key=probe.get)
            torch.set_num_threads(best_n)
            used = max(used, best_n)
            passes = [probe[(best_n, best_sub)]]
            want = 5 if passes[0] < 5e-3 else 3
            while len(passes) < want or (len(passes) < 9 and passes[0] < 5e-3 and time.perf_counter() - t_blk < blk_budget):
                passes.append(one_pass(best_sub))
                if len(passes) >= 3 and time.perf_counter() - t_blk > 2.5 * blk_budget:
                    break
            t = statistics.median(passes)
            per_image += t / ns
            flop = b.get("alt_work") or (b["work"] if b["bound"] == "mfma" else None)
            rec = {"block": b["name"], "key": b["key"], "images": ns, "sub_batch": best_sub, "threads": best_n, "images_per_s": round(ns / t, 1),
                   "passes_s": [round(v, 4) for v in passes],
                   "probe_s": {"%dx%d" % k: round(v, 4) for k, v in probe.items()},
                   "note": b.get("cpu_note", "oracle restatement (same math as the reference forward, not its exact operator sequence)")}
            if flop:                                            # achieved host rate, so that a reader can see the baseline is sane
                rec["GFLOPs"] = round(flop / b["x"].shape[0] * ns / t / 1e9, 1)
            else:
                rec["GBps"] = round(b["work"] / b["x"].shape[0] * ns / t / 1e9, 1)
            detail.append(rec)
            sys.stderr.write("[bench] cpu leg %-42s %.1f s (threads %d x sub-batch %d of %d pairs; median of %d passes)\n" % (
                b["name"], time.perf_counter() - t_blk, best_n, best_sub, len(probe), len(passes)))
    out = {"value": round(1.0 / per_image, 2), "unit": "images/s", "cores": used, "kind": "port",
           "sample": "first n images of the same batch per block (n = cpu images per block: %s); (threads x sub-batch) probed jointly over "
                     "{16,32,64,128} x {8, n}, best pair timed >= 3 passes, median" % ",".join("%s=%d" % (d["key"], d["images"]) for d in detail),
           "host": "%s: %d cores / %d threads; usable by this process: affinity %d, %s" % (model, cores, threads, aff, qsrc)}
    for d in detail:                                            # 14 blocks -> keys 7..20 of the 24 the driver keeps
        out["img_s_" + d["key"]] = d["images_per_s"]
    out["threads_x_sub"] = ",".join("%s=%dx%d" % (d["key"], d["threads"], d["sub_batch"]) for d in detail)
    out["GFLOPs"] = ",".join("%s=%.0f" % (d["key"], d["GFLOPs"]) for d in detail if "GFLOPs" in d)
    out["GBps"] = ",".join("%s=%.0f" % (d["key"], d["GBps"]) for d in detail if "GBps" in d)
    out["legend"] = ("img_s_* per block key; threads_x_sub = the (torch threads x sub-batch) pair used; GFLOPs / GBps = achieved host rate; "
                     "ATen-operator-sequence restatements of the reference forward (oracle/aten_seq.py); cores = largest thread count used")
    out.update({"host_cores": cores, "host_threads": threads, "affinity_cpus": aff, "cgroup_cpus": quota, "host_cpu": model})
    return out, detail


if __name__ == "__main__":
    main()
