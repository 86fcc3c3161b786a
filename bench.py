#!/usr/bin/env python3
"""bench.py — candidate renders scored per second on MI355X (BASELINE.json metric).

A "step" is one pass of the hot path over one batch of candidate poses: pose batch in
(resident in HBM) -> virtual cameras -> hash-grid NeRF ray march -> composite over the fixed
background -> rot90 + CLIP preprocess -> ViT forward -> logits against the cached text
embeddings, then (N>1) ONE all-gather of logits, ratio, smoothing, argmax.

python bench.py [--gpus N] [--steps K] [--warmup W] [--config C] [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps and prints the JSON line (value, ms_per_step and the roofline figures
read from the timed steps' own device timers).  --full adds what takes work of its own after the timed steps: the CPU
baseline with its parity check against the oracle (--cpu-sample), the per-product ViT event times (--product-steps)
and the rocm-smi power line (--power-seconds).  --dump-outputs DIR writes what the last timed step computed (gathered
logits, smoothed scores, the best pose) as DIR/<name>.npy; the inputs are seeded, so two builds compare output for output.

Default workload (no --config): BASELINE.json configs[1] — synthetic "shopping" scene (seeded,
SURVEY.md §8(d)), 4 096 candidate poses per GPU, 640x360 renders, ViT-B/16, bf16 MFMA with fp32
accumulation; N>1 = weak scaling, pose grid [64,64,N], every rank renders+scores its own contiguous
block, no data-path collective except ONE all-gather of the logits (d2r_allgather_scores: RCCL over
xGMI behind the C ABI).  This is the line a 1/2/4/8-GPU scaling sweep reads (`--gpus N`, nothing else).

--config C runs BASELINE.json configs[C] as a named workload (pose grids of SURVEY.md §8(d),
reference vision_3d/obj_pose_opt.py:16-36):
  0  shopping, grid [8,4,1,1,1,1] = 32 (type 3), 160x90, ViT-B/16 — the reference's CPU-runnable case; the CPU
     baseline covers all 32 candidates
  1  shopping, [64,64,1,1,1,1] = 4 096 per GPU (type 3), 640x360, ViT-B/16 (the default; weak over N)
  2  pool_triangle, [128,128,1,1,1,1] = 16 384 per GPU (type 0), 640x360, ViT-B/16 (weak over N)
  3  shopping, [128,128,8,1,1,1] = 131 072 in total (type 3), 640x360, ViT-B/16: STRONG scaling, the grid is
     split over the N GPUs (on one GPU the whole grid runs)
  4  shelf (aabb_scale 2), 6-DoF grid [16,16,16,4,4,4] = 262 144 in total (type 1, eulers linspace(-pi, pi/2, 4)),
     640x360, ViT-L/14: STRONG scaling; with fewer than 8 GPUs each rank takes shard `rank` of the 8-GPU partition
     (one GPU: a 1/8 slice, 32 768 candidates; --slice-of 1 runs the whole grid).  BASELINE.json words this
     config "fp16 render + fp8 MFMA ViT"; this build computes it in bf16 (an MX-fp8 tower
     misses the 1e-3 parity bar) and says so in the line.
Individual flags (--scene, --sample-res, --clip, --width, --height, --scaling, ...) override the table.

With --gpus N > 1 and no launcher environment (WORLD_SIZE unset) the script runs itself as a child process under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1` and exits with its status.
"""
import argparse
import json
import os
import sys
import time


def effective_cpus() -> int:
    """CPUs this process may actually use: the scheduler affinity, capped by the container's CPU quota (cgroup v2 cpu.max,
    v1 cpu.cfs_quota_us) — a 256-core host that grants the container 16 CPUs' worth of time runs 128 threads SLOWER than 16."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // p))
        except (OSError, ValueError):
            pass
    return n


_ENV_AT_START = set(os.environ)       # thread-count variables the CALLER set are respected, the defaults below are not inherited by child ranks


def rank_cpu_share() -> int:
    """This rank's share of those CPUs when several ranks run on the node (one process per GPU): quota // LOCAL_WORLD_SIZE.  The
    library's PNG / text workers size themselves the same way (csrc/pngio.cpp d2r_default_io_threads reads LOCAL_WORLD_SIZE)."""
    lws = int(os.environ.get("D2R_LOCAL_WORLD_SIZE") or os.environ.get("LOCAL_WORLD_SIZE") or 1)
    return max(1, effective_cpus() // max(1, lws))


# the CPU-baseline leg (oracle: OpenMP render + BLAS ViT) gets the CPUs the box really grants — a rank of an N-GPU run its share of
# them — unless the caller chose
for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_k, str(rank_cpu_share()))

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

ALGO_BYTES_PER_SAMPLE = 512          # L*8*F*2 B = 16*8*2*2
HBM_PEAK_GBPS = 8000.0               # MI355X_MICROARCH.md: 8.0 TB/s spec
MFMA_BF16_PEAK_TFLOPS = 2500.0       # dense bf16
MFMA_FP8_PEAK_TFLOPS = 5000.0        # dense fp8 (MX-scaled v_mfma_scale_f32_32x32x64_f8f6f4)
MLP_FLOP_PER_SAMPLE = 20480


def vit_gflop(cfg, executed: bool = False, l0_touched: float = 1.0) -> float:
    """Forward FLOPs per image of the vision tower (35.1 GFLOP for ViT-B/16).
    executed=True: what the library actually issues — its last block computes k/v for every token but q,
    attention output, out-projection and MLP for the class token only (the head reads nothing else;
    the other rows of the last block are dead code), 2.4 GFLOP less for ViT-B/16."""
    P, d, mlp, L = cfg["patch_size"], cfg["hidden_size"], cfg["mlp"], cfg["num_layers"]
    npatch = (cfg["image_size"] // P) ** 2
    T = npatch + 1
    per_layer = 2 * T * (4 * d * d + 2 * d * mlp) + 4 * T * T * d
    total = 2 * npatch * d * 3 * P * P + L * per_layer + 2 * d * cfg["proj"]
    if executed:
        last = 2 * T * 2 * d * d + 2 * d * d + 4 * T * d + 2 * (d * d + 2 * d * mlp)
        total += last - per_layer
        # layer-0 reuse: patch embedding and the first block's QKV product run on the touched patch tokens only
        total -= (1.0 - l0_touched) * npatch * (2 * d * 3 * P * P + 2 * d * 3 * d)
    return total / 1e9


def vit_fp8_gflop(cfg, l0_reuse: bool) -> float:
    """FLOPs per image the library issues on the fp8 MFMA with option vit_fp8 (the four Linear products of every block but the
    first — when its rows are reused — and the class-token-only last one)."""
    d, mlp, L = cfg["hidden_size"], cfg["mlp"], cfg["num_layers"]
    T = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    blocks = max(0, L - 1 - (1 if l0_reuse else 0))
    return blocks * 2 * T * (4 * d * d + 2 * d * mlp) / 1e9


def vit_product_table(t, cfg, per_launch, peak_tflops):
    """roofline.products: per full-size product launch of the vision tower (default schedule), the average event time, the flops of
    one launch over `per_launch` images, and flops / time / the dense bf16 MFMA peak."""
    d, mlp = cfg["hidden_size"], cfg["mlp"]
    T = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    rows = per_launch * T
    flops = {"qkv": 2.0 * rows * 3 * d * d, "attn": 4.0 * per_launch * T * T * d, "out": 2.0 * rows * d * d,
             "fc1": 2.0 * rows * d * mlp, "fc2": 2.0 * rows * d * mlp}
    out = {}
    for k, f in flops.items():
        ms, n = t.get(f"vit_{k}_ms", 0.0), t.get(f"vit_{k}_launches", 0)
        if not n or ms <= 0:
            continue
        avg_ms = ms / n
        tf = f / (avg_ms * 1e-3) / 1e12
        out[k] = {"avg_launch_ms": round(avg_ms, 4), "launches": int(n), "gflop_per_launch": round(f / 1e9, 1),
                  "achieved": round(tf, 1), "frac": round(tf / peak_tflops, 5)}
    if out:
        covered = sum(t.get(f"vit_{k}_ms", 0.0) for k in flops)
        out["other_ms_per_forward"] = round((t["clip_ms"] - covered) / max(1, t["clip_launches"]), 3)
        out["images_per_launch"] = int(per_launch)
        out["note"] = ("full-size launches only (layer 0's compact QKV under l0_reuse and the class-token-only last block are in other_ms_per_forward, with row "
                       "statistics, patch embedding and head); a ragged last chunk lowers a product's average")
    return out or None


def recorded_pmc(scene_name, W, H, per_launch, clip_name):
    """PMC figures bench.py cannot collect itself (it does not run under rocprofv3 --pmc): read from the committed summary of the
    same workload (profiles/r06_pmc.json, separate --pmc passes as MI355X_MICROARCH.md prescribes), else null."""
    for name in ("r06_pmc.json",):
        try:
            t = json.load(open(os.path.join(REPO, "profiles", name)))
        except (OSError, ValueError):
            continue
        wl = t.get("workload", {})
        if (wl.get("scene"), wl.get("width"), wl.get("height"), wl.get("chunk"), wl.get("clip")) != (scene_name, W, H, per_launch, clip_name):
            continue
        src = f"profiles/{name}"
        return t.get("vit_traffic_bytes_per_forward"), src, dict(t.get("march", {}), source=src)
    return None, None, None


def power_probe(step_fn, device_index: int, seconds: float):
    """Socket power and shader clock (rocm-smi) sampled over EXTRA, untimed steps after the timed region: the step
    runs against the package power limit, which is what prices the ViT's MFMA fraction.
    Returns None when rocm-smi is not there."""
    import re
    import shutil
    import subprocess
    import threading
    smi = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    if not os.path.exists(smi) or seconds <= 0:
        return None
    samples, stop = [], threading.Event()
    cmd = [smi, "-d", str(device_index), "--showpower", "--showclocks"]
    try:
        # the first rocm-smi of a fresh box takes many seconds (the image pages in): pay that before the sampled steps, not during them
        subprocess.run(cmd, capture_output=True, text=True, timeout=60)
    except Exception:
        return None
    step_fn()                                    # the device is under load when the first sample is taken

    def work():
        while not stop.is_set():
            try:
                txt = subprocess.run(cmd, capture_output=True, text=True, timeout=10).stdout
            except Exception:
                continue
            w = re.search(r"Power \(W\):\s*([\d.]+)", txt)
            c = re.search(r"sclk clock level:\s*\S+\s*\((\d+)Mhz\)", txt)
            if w and c:
                samples.append((float(w.group(1)), int(c.group(1))))

    th = threading.Thread(target=work, daemon=True)
    th.start()
    t0 = time.perf_counter()
    # `seconds` of steps, extended (to at most three times that) until there are enough samples to call it an average
    while time.perf_counter() - t0 < seconds or (len(samples) < 8 and time.perf_counter() - t0 < 3 * seconds):
        step_fn()
    stop.set()
    th.join(timeout=6)
    cap = None
    try:
        m = re.search(r"Max Graphics Package Power \(W\):\s*([\d.]+)", subprocess.run([smi, "-d", str(device_index), "--showmaxpower"],
                                                                                  capture_output=True, text=True, timeout=5).stdout)
        cap = float(m.group(1)) if m else None
    except Exception:
        pass
    if not samples:
        return None
    return {"avg_w": round(sum(s[0] for s in samples) / len(samples), 1), "max_w": max(s[0] for s in samples), "cap_w": cap,
            "sclk_mhz_avg": round(sum(s[1] for s in samples) / len(samples)), "samples": len(samples),
            "note": "rocm-smi over extra untimed steps after the timed region"}


def cpu_baseline(scene, W, H, cfg, sd, text, poses_world, n_sample):
    """The oracle (CPU restatement) timed on the host cores on a bounded sample of the same
    workload.  Checker code used here ONLY as the reported CPU baseline."""
    from oracle import render_ref
    from oracle.pipeline import OraclePipeline, oracle_logits
    pipe = OraclePipeline(scene, W, H)
    bg = pipe.background()                       # setup, not timed (once per view)
    n_sample = min(n_sample, len(poses_world))
    idx = np.unique(np.linspace(0, len(poses_world) - 1, n_sample).astype(int))
    t0 = time.time()
    frames = pipe.frames(poses_world[idx].reshape(-1, 4, 4), bg=bg)
    t_render = time.time() - t0
    t1 = time.time()
    lg, _ = oracle_logits(frames, cfg, sd, text)
    t_clip = time.time() - t1
    dt = time.time() - t0
    blas = None
    try:
        from threadpoolctl import threadpool_info
        blas = max([int(i.get("num_threads", 0)) for i in threadpool_info() if i.get("user_api") == "blas"] or [0]) or None
    except Exception:
        pass
    return {"value": round(len(idx) / dt, 4), "unit": "candidates/s", "cores": max(render_ref.num_threads(), blas or 1),
            "host_cpus": os.cpu_count(), "cpu_quota": effective_cpus(),
            "threads": {"render_openmp": render_ref.num_threads(), "vit_blas": blas},
            "kind": "port",
            "sample": f"{len(idx)} of the {len(poses_world)} candidates at {W}x{H}: oracle C render+composite "
                      f"(OpenMP, {render_ref.num_threads()} threads, {t_render:.1f}s) + numpy fp32 ViT "
                      f"(BLAS, {blas} threads, {t_clip:.1f}s); `cores` = threads used = the CPUs the container's quota grants "
                      f"({effective_cpus()} of the host's {os.cpu_count()})"}, frames, lg, idx


def self_launch(n: int):
    """`python bench.py --gpus N` outside a launcher: run `torch.distributed.run` with N ranks as a fresh child process (not
    an exec: torch.cuda.device_count() below may already have opened the GPU in this one) and exit with its status."""
    import socket
    import subprocess
    import torch
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    # dmabuf IPC: the host driver of these boxes has no legacy IPC mode; without it RCCL's (and torch's) cross-process
    # buffer registration fails with `hipIpcGetMemHandle: invalid argument`.  The image exports it already — this only
    # fills it in for an environment that was built without it, and never overrides a value the caller set.
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):       # each rank: its share of the CPU quota (set at import for n = 1)
        env[k] = str(max(1, effective_cpus() // n)) if k not in _ENV_AT_START else env[k]
    if torch.cuda.device_count() < n:
        # fewer GPUs than ranks (a 1-GPU box): ranks share GPUs, which RCCL refuses -> gloo process group and
        # the torch fallback of the gather; the JSON line says so ("collective")
        env.setdefault("D2R_DIST_BACKEND", "gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    rc = subprocess.run(cmd, env=env).returncode
    sys.exit(rc if rc >= 0 else 128 - rc)


# BASELINE.json configs[0..4] as named workloads (pose-grid bounds per scene type:
# reference vision_3d/obj_pose_opt.py:16-36).  "per_gpu": weak scaling, the grid's z axis grows with the GPU count;
# "total": strong scaling, the grid is fixed and split over the GPUs.
BASELINE_CONFIGS = {
    0: dict(scene="shopping", sample_res=[8, 4, 1, 1, 1, 1], width=160, height=90, clip="vit_b16", scaling="strong",
            name="shopping_demo.json, 32 candidate poses, 160x90 render (the reference's CPU-runnable case)"),
    1: dict(scene="shopping", sample_res=[64, 64, 1, 1, 1, 1], width=640, height=360, clip="vit_b16", scaling="weak",
            name="shopping scene, 4096 candidate poses per GPU, 640x360, bf16 MLP + ViT-B/16"),
    2: dict(scene="pool_triangle", sample_res=[128, 128, 1, 1, 1, 1], width=640, height=360, clip="vit_b16", scaling="weak",
            name="pool_triangle scene, 16384 candidate poses per GPU, 640x360 (hash-grid HBM-bound stress)"),
    3: dict(scene="shopping", sample_res=[128, 128, 8, 1, 1, 1], width=640, height=360, clip="vit_b16", scaling="strong",
            name="shopping scene, pose-shard over the GPUs, 131072 candidates, all-gather of scores"),
    4: dict(scene="shelf", sample_res=[16, 16, 16, 4, 4, 4], width=640, height=360, clip="vit_l14", scaling="strong", partition=8,
            name="shelf_demo 6-DoF, 262144 candidates, ViT-L/14 encoder, fp16 render as BASELINE words it (NeRF MLPs on the fp16 MFMA: the library's default); "
                 "BASELINE's fp8 ViT is --vit-fp8 — outside the 1e-3 parity bar, so the tower runs in bf16 by default"),
}


def shard_plan(sample_res, world: int, partition: int) -> dict:
    """Which candidates each rank renders and in which order the gathered logits come back.
    `order`: the pose-batch indices in sharding order — 3-DoF grids (orientations 1, nz > 1) are walked z-major so
    that a rank owns whole (x, y) sheets (pose order has z fastest); 6-DoF grids keep the pose order (orientations
    fastest: contiguous blocks are x slabs with every orientation).  The order is cut into `partition` contiguous
    shards (dist.shard_range); rank r takes shard r.  partition == world except for a strong-scaling grid run on
    fewer GPUs than the partition its config names: then only shards 0..world-1 run (`n_run` candidates per step) and
    the rest of the grid keeps score 0.  `run_idx`: pose indices of the gathered rows, rank-major."""
    from dream2real_amd.dist import shard_range
    N = int(np.prod(sample_res))
    nx, ny, nz = sample_res[:3]
    n_ori = sample_res[3] * sample_res[4] * sample_res[5]
    if n_ori == 1 and nz > 1:
        order = np.arange(N).reshape(nx, ny, nz).transpose(2, 0, 1).reshape(-1)
    else:
        order = np.arange(N)
    shards = [order[slice(*shard_range(N, r, partition))] for r in range(world)]
    run_idx = np.concatenate(shards)
    return {"order": order, "shards": shards, "run_idx": run_idx, "n_run": int(len(run_idx))}


class Watchdog:
    """An N > 1 run happens on a node the builder never sees: nothing may hang.  Every stage that can block on another
    rank (rendezvous, communicator init, a step with its collective, the barriers) runs under a deadline; when one passes,
    this rank prints ONE JSON line naming the stage, itself, its GPU and its HSA_* / NCCL_* environment, and exits
    non-zero — the launcher then stops the other ranks instead of leaving them in a barrier."""

    def __init__(self):
        import threading
        self.stage_name, self.deadline, self.device = None, None, None
        self.scale = float(os.environ.get("D2R_WATCHDOG_SCALE", "1"))
        self._lock = threading.Lock()
        threading.Thread(target=self._run, name="d2r-watchdog", daemon=True).start()

    def stage(self, name, seconds):
        with self._lock:
            self.stage_name, self.deadline = name, time.monotonic() + seconds * self.scale

    def done(self):
        with self._lock:
            self.stage_name, self.deadline = None, None

    def _run(self):
        while True:
            time.sleep(0.5)
            with self._lock:
                name, dl = self.stage_name, self.deadline
            if dl is not None and time.monotonic() > dl:
                report_failure(name, f"no progress within the stage's deadline ({self.scale}x scale): a rank is stuck or gone", self.device, code=3)


def report_failure(stage, err, device_index, code=1):
    """One JSON line on stdout (and stderr) describing a failed multi-rank run, then exit non-zero NOW (os._exit: the
    interpreter may be blocked inside a collective)."""
    from dream2real_amd import dist as d2r_dist
    line = {"collective_error": str(err), "stage": stage}
    try:
        line.update(d2r_dist.describe_environment(device_index))
        line["comm_report"] = dict(d2r_dist.LAST_COMM_REPORT)
    except Exception as e:                    # the report must come out whatever else is broken
        line["describe_environment_failed"] = repr(e)
    txt = json.dumps(line)
    print(txt, flush=True)
    print(txt, file=sys.stderr, flush=True)
    os._exit(code)


def resolve_workload(args, world: int) -> dict:
    """The workload `--config` / the individual flags name at `world` GPUs: scene, encoder, frame size, pose grid, scaling, partition."""
    base = dict(BASELINE_CONFIGS[1 if args.config is None else args.config])
    scaling = args.scaling or base["scaling"]
    sample_res = list(base["sample_res"])
    if args.sample_res:
        sample_res = [int(x) for x in args.sample_res.split(",")]
        assert len(sample_res) == 6, "--sample-res takes six numbers"
    elif args.poses_total is not None or (args.scaling == "strong" and args.config is None):
        total = args.poses_total or 131072
        side = int(round(np.sqrt(total / 8)))
        assert side * side * 8 == total, "--poses-total must be x*x*8"
        sample_res, scaling = [side, side, 8, 1, 1, 1], "strong"
    elif args.poses_per_gpu is not None:
        side = int(round(np.sqrt(args.poses_per_gpu)))
        assert side * side == args.poses_per_gpu, "--poses-per-gpu must be a square"
        sample_res = [side, side, 1, 1, 1, 1]
    if scaling == "weak":
        assert sample_res[2] == 1, "weak scaling stacks one [x,y] sheet per GPU along z"
        sample_res[2] = world
    partition = max(world, args.slice_of if args.slice_of is not None else base.get("partition", 1)) if scaling == "strong" else world
    assert partition % world == 0 or partition == world, "--slice-of must be a multiple of --gpus"
    return dict(base=base, scene=args.scene or base["scene"], clip=args.clip or base["clip"], width=args.width or base["width"],
                height=args.height or base["height"], scaling=scaling, sample_res=sample_res, partition=partition)


def device_workspace_estimate(chunk: int, W: int, H: int, cfg: dict, ray_sort: bool = True) -> dict:
    """HBM a rank's passes take beyond models and weights, from the sizes the library reserves (api.hip render_score_core, nerf.hip
    d2r_reserve_render, clip.hip): worst-case ray queue(s), frames, patches, and the vision tower's activations.  An ESTIMATE for
    planning (the measured figure of a real run is `hbm_footprint` in its line); everything scales with the pass size, nothing
    with the number of ranks — a rank of an 8-GPU run holds exactly what the 1-GPU run holds."""
    px, P, d, mlp = W * H, cfg["patch_size"], cfg["hidden_size"], cfg["mlp"]
    T = (cfg["image_size"] // P) ** 2 + 1
    rows = -(-chunk * T // 256) * 256
    rays = chunk * px
    queue = rays * 8
    out = {"ray_queue": queue, "ray_queue_sorted": queue if ray_sort else 0,
           "sort_counts": ((-(-rays // 16384)) + 2) * 4096 * 4 if ray_sort else 0,
           "frames_u8": chunk * px * 3, "patches_bf16": chunk * (T - 1) * (-(-3 * P * P // 64) * 64) * 2,
           # residual hi + lo byte + operand copy, q / k / v, attention output, the MLP's hidden activations, fp32 patch embedding, row statistics
           "vit_activations": rows * (d * 2 + d + d * 2 + 3 * d * 2 + d * 2 + mlp * 2 + d * 4 + 64)}
    out["total"] = int(sum(out.values()))
    return out


def run_plan(args, wd):
    """--plan: what every rank of this run WOULD do, worked out without touching a GPU (runs on a CPU box under gloo): the device
    it would take (LOCAL_RANK, as run_kernel_bench does), its contiguous pose shard, passes per step, device workspaces, CPU threads.
    Rank 0 prints the gathered plan as one JSON line."""
    import torch
    from dream2real_amd import dist as d2r_dist
    from dream2real_amd.clip_model import CLIP_CONFIGS
    wd.stage("rendezvous (torch.distributed.init_process_group)", 300)
    rank, world, local = d2r_dist.init_from_env("gloo" if int(os.environ.get("WORLD_SIZE", "1")) > 1 else None)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    wl = resolve_workload(args, world)
    plan = shard_plan(wl["sample_res"], world, wl["partition"])
    mine = plan["shards"][rank]
    n_dev = torch.cuda.device_count()
    chunk = min(args.chunk, max(1, len(mine)))
    cfg = CLIP_CONFIGS[wl["clip"]]
    ws = device_workspace_estimate(chunk, wl["width"], wl["height"], cfg)
    entry = {"rank": rank, "local_rank": local, "device": local % n_dev if n_dev else local, "devices_visible": n_dev,
             "poses": int(len(mine)), "first_pose": int(mine[0]) if len(mine) else None, "last_pose": int(mine[-1]) if len(mine) else None,
             "passes_per_step": -(-len(mine) // chunk), "chunk": chunk, "workspace_bytes": ws,
             "cpu_threads": {"omp": int(os.environ.get("OMP_NUM_THREADS", "0")), "share_of_quota": rank_cpu_share(), "quota": effective_cpus(),
                             "local_world": int(os.environ.get("LOCAL_WORLD_SIZE", "1"))},
             "collective": "none" if world == 1 else f"one all-gather of {plan['n_run']} x 2 fp32 logits = {plan['n_run'] * 8} bytes per step (d2r_allgather_scores)"}
    entries = [entry]
    if world > 1:
        entries = [None] * world
        torch.distributed.all_gather_object(entries, entry)
    wd.done()
    if rank == 0:
        print(json.dumps({"plan": entries, "n_gpus": world, "scaling": wl["scaling"], "sample_res": wl["sample_res"], "poses_total": int(np.prod(wl["sample_res"])),
                          "poses_per_step": plan["n_run"], "scene": wl["scene"], "clip": wl["clip"], "width": wl["width"], "height": wl["height"],
                          "partition": wl["partition"]}), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def run_dry_collective(args, wd):
    """--dry-collective: ONLY what N > 1 adds to the path — rendezvous, the C-ABI communicator (d2r_comm_init: RCCL over
    xGMI), one 1 MiB all-gather through d2r_allgather_scores, and agreement of every rank on the argmax of the gathered
    buffer.  Separates "the collective is broken on this node" from "the path is broken" when a scaling run fails."""
    import torch
    from dream2real_amd import dist as d2r_dist
    from dream2real_amd import engine
    wd.stage("rendezvous (torch.distributed.init_process_group)", 300)
    rank, world, local = d2r_dist.init_from_env()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    wd.device = local
    dev = torch.device("cuda", local)
    ctx = engine.Context(local)
    wd.stage("d2r_comm_init (ncclCommInitRank)", 300)
    use_c_abi = d2r_dist.init_comm(ctx, rank, world)
    n_total = 131072                                       # x 2 captions x 4 B = 1 MiB gathered
    g = d2r_dist.ShardGather(ctx, n_total, 2, rank, world, dev, use_c_abi)
    lo, hi = g.lo, g.hi
    vals = torch.arange(lo, hi, dtype=torch.float32, device=dev)
    g.local[: hi - lo, 0] = torch.sin(vals * 0.001)
    g.local[: hi - lo, 1] = vals
    torch.cuda.synchronize(dev)
    wd.stage("all-gather of 1 MiB (d2r_allgather_scores)", 120)
    times = []
    for _ in range(5):
        torch.cuda.synchronize(dev)
        if world > 1:
            torch.distributed.barrier()
        t0 = time.perf_counter()
        full = g.gather()
        times.append(time.perf_counter() - t0)
    want = np.stack([np.sin(np.arange(n_total, dtype=np.float32) * np.float32(0.001)), np.arange(n_total, dtype=np.float32)], 1)
    exact = bool(np.allclose(full[:, 0], want[:, 0], atol=1e-6) and (full[:, 1] == want[:, 1]).all())
    best = int(np.argmax(full[:, 0]))
    wd.stage("argmax agreement (all_reduce)", 120)
    agree = True
    if world > 1:
        t = torch.tensor([best, -best], dtype=torch.int64, device=dev if torch.distributed.get_backend() == "nccl" else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        agree = int(t[0].item()) == best and int(-t[1].item()) == best
    wd.done()
    if not (exact and agree):
        report_failure("dry collective check", f"gathered buffer exact={exact}, argmax agreement={agree}", local)
    if rank == 0:
        print(json.dumps({"dry_collective": "ok", "n_gpus": world, "bytes_gathered": n_total * 8,
                          "collective": "d2r_allgather_scores (ncclAllGather, RCCL)" if use_c_abi and world > 1 else
                                        ("device copy (one rank)" if world == 1 else f"torch.distributed all_gather ({torch.distributed.get_backend()})"),
                          "gather_ms": [round(t * 1e3, 3) for t in times], "argmax": best,
                          "comm_report": dict(d2r_dist.LAST_COMM_REPORT), **d2r_dist.describe_environment(local)}), flush=True)
    if world > 1:
        torch.distributed.barrier()
        ctx.comm_destroy()
        torch.distributed.destroy_process_group()


# The reference's own workload (configs/shopping_demo.json:28, combined_rendering.py:86, clip_scoring.py:150-151): pose grid
# [100,100,7,1,1,1] = 70 000 poses, 336x336 renders, openai/clip-vit-large-patch14-336, physics pre-filter on.
REFERENCE_WORKLOAD = dict(scene="shopping", sample_res=[100, 100, 7, 1, 1, 1], width=336, height=336, clip="vit_l14_336",
                          name="the reference's own configuration: shopping_demo.json grid [100,100,7,1,1,1] = 70000 poses, "
                               "336x336, ViT-L/14-336, physics pre-filter on")


def run_api(args, wd):
    """--api: the number a caller of the drop-in API gets.  One step = one `ImaginationEngine.dream_best_pose` call
    (reference dream2real.py:286-358): physics pre-filter on the objects' mesh files -> renderer -> optimise_pose_grid (the
    fused, chunked d2r_render_score_host call; pose-sharded with ONE all-gather under a launcher) -> smoothing -> argmax ->
    goal_pose / pose_batch / pose_scores.txt (+ cb_render/*.png with --api-save 1, as the reference does).  Host arrays in,
    host arrays out: pose upload, logits download, text files and PNG encoding are all inside the timed region."""
    import resource
    import shutil
    import tempfile

    import torch
    from dream2real_amd import dist as d2r_dist
    from dream2real_amd import dream2real, engine
    from dream2real_amd.accio2ngp import converter
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    from synthetic_scenes import make_scene, make_task, scene_text_embeds, write_phys_meshes

    wd.stage("rendezvous (torch.distributed.init_process_group)", 300)
    rank, world, local = d2r_dist.init_from_env()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    wd.device = local
    wd.stage("setup + dream_best_pose calls (the API brings the communicator up itself)", 3600)
    base = dict(REFERENCE_WORKLOAD if args.config is None else BASELINE_CONFIGS[args.config])
    scene_name, clip_name = args.scene or base["scene"], args.clip or base["clip"]
    W, H = args.width or base["width"], args.height or base["height"]
    sample_res = [int(x) for x in args.sample_res.split(",")] if args.sample_res else list(base["sample_res"])
    from dream2real_amd.scene import DEMO_LENS
    scene = make_scene(scene_name, lens=DEMO_LENS if args.lens == "demo" else None)
    cfg = CLIP_CONFIGS[clip_name]
    sd = random_clip_state_dict(cfg, seed=6)
    ctx = engine.Context(local)
    ctx.set_option("chunk", args.chunk)
    for k, v in base.get("opts", {}).items():
        ctx.set_option(k, int(v))
    for kv in args.opt:
        k, v = kv.split("=")
        ctx.set_option(k, int(v))
    fg, bg = scene.testbeds(ctx)       # set_camera_to_training_view(0) on both: the view's intrinsics AND its lens
    scorer = engine.ClipScorer(ctx, cfg, sd)
    task = make_task(scene, fg, bg)
    cam_ngp = converter(np.asarray(scene.cam_poses, np.float32))[0]
    T1 = converter(np.asarray(scene.obj_pose, np.float32)[None])[0]
    bg_rgba, bg_depth = bg.render_batch(cam_ngp[None, :3], W, H)
    view = fg.view(W, H)
    ctx.set_background(view, bg_rgba[0], bg_depth[0])
    text_encoder = tokenizer = None
    if args.api_text == "tower":
        # the captions of the task through the library's own BPE tokenizer and text tower (random weights of the same
        # checkpoint, the byte-level BPE vocabulary committed under tests/golden/ as data): the whole caption -> score path
        # inside the timed call.  Random-weight towers have no language prior, so the scores mean nothing; the work is real.
        from dream2real_amd.tokenizer import ClipBpeTokenizer
        g = os.path.join(REPO, "tests", "golden")
        tokenizer = ClipBpeTokenizer.from_files(os.path.join(g, "bpe_vocab.json"), os.path.join(g, "bpe_merges.txt"), context_length=32)
        tcfg = dict(cfg, vocab=len(tokenizer.vocab), ctx=32)
        text_encoder = engine.TextEncoder(ctx, tcfg, random_clip_state_dict(tcfg, seed=6))
    else:
        _, e0 = scorer.score_frames(fg.render_composite(view, T1, cam_ngp, T1[None]), np.zeros((1, cfg["proj"]), np.float32), return_embeds=True)
        task.text_embeds = scene_text_embeds(e0[0])
    root = args.api_dir or tempfile.mkdtemp(prefix="d2r_api_")
    data_dir = os.path.join(root, "run")
    if rank == 0:
        os.makedirs(data_dir, exist_ok=True)
    use_phys = bool(args.api_phys) and scene_name in ("shopping", "pool_triangle")
    if use_phys:
        if rank == 0:
            write_phys_meshes(scene, root)
        task.movable_obj.phys_model, task.task_bground_obj.phys_model = os.path.join(root, "movable.obj"), os.path.join(root, "bground.obj")
    if world > 1:
        torch.distributed.barrier()
    pcfg = dream2real.PathConfig(data_dir=data_dir, sample_res=sample_res, scene_type=scene.scene_type, resolution=(W, H),
                                 use_phys=use_phys, save_renders=bool(args.api_save))
    eng = dream2real.ImaginationEngine(pcfg, ctx, scorer, text_encoder=text_encoder, tokenizer=tokenizer)
    stages = {}

    from dream2real_amd import clip_scoring

    def one():
        t0 = time.perf_counter()
        best, pose_batch, scores = eng.dream_best_pose(task)
        total = time.perf_counter() - t0
        stages.clear()
        stages.update({k: round(v * 1e3, 2) for k, v in clip_scoring.LAST_TIMINGS.items()})
        stages["physics_setup_renderer_and_txt_files"] = round((total - sum(clip_scoring.LAST_TIMINGS.values())) * 1e3, 2)
        return best, pose_batch, scores

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        one()
    ctx.set_option("timing", 1)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        best, pose_batch, scores = one()
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if torch.distributed.get_backend() == "nccl" else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    timing = ctx.timing()
    ctx.set_option("timing", 0)
    if rank == 0:
        sc = scores.numpy()
        n_valid, N = int((sc != 0).sum()), int(sc.shape[0])
        n_png = len(os.listdir(os.path.join(data_dir, "cb_render"))) if args.api_save else 0
        label = (f"BASELINE.json configs[{args.config}]: {base['name']}" if args.config is not None else base["name"])
        out = {
            "metric": f"candidate renders scored/sec ({W}x{H}) through the drop-in API (ImaginationEngine.dream_best_pose)",
            "value": round(n_valid * args.steps / elapsed, 2), "unit": "candidates/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None,
            "dtype": "fp8 e4m3 Linear products (fp32 accumulate) in the ViT, bf16 elsewhere" if "vit_fp8=1" in args.opt else "bf16", "data": "synthetic",
            "config": {"workload": f"{label} — ran: {scene_name} scene, pose grid {sample_res} = {N} poses sampled, {n_valid} valid after the "
                                   f"physics pre-filter ({'GPU GJK on the mesh files' if use_phys else 'off: every pose valid'}), {W}x{H}, bf16 MLP + {clip_name}, "
                                   f"{'pose-shard x' + str(world) if world > 1 else 'one GPU'}; host arrays in / out, "
                                   f"save_renders={bool(args.api_save)} ({n_png} PNG files written per step)",
                       "api": "dream2real_amd.dream2real.ImaginationEngine.dream_best_pose", "scene": scene_name, "clip": clip_name,
                       "width": W, "height": H, "poses_sampled": N, "poses_valid": n_valid, "sample_res": sample_res,
                       "save_renders": bool(args.api_save), "physics": use_phys,
                       "text_embeds": ("captions -> ClipBpeTokenizer -> d2r_text_encode (random-weight text tower) inside the timed call" if args.api_text == "tower"
                                       else "2 seeded unit vectors correlated with the scene's image embedding, cached on the task"),
                       "parallelism": f"pose-shard x{world}" if world > 1 else "single GPU"},
            "poses_sampled_per_s": round(N * args.steps / elapsed, 2),
            "device_ms_per_step": {k.replace("_ms", ""): round(v / args.steps, 3) for k, v in timing.items() if k.endswith("_ms")},
            "note_device_ms": "with the two-stream pipeline the render half (march / raygen / prep) overlaps the ViT of the previous chunk: the parts do not add up to the step",
            "host_ms_last_step": dict(stages),
            "peak_host_rss_gb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1048576, 2),
            "argmax_pose": int(np.argmax(sc)),
            "roofline": None, "cpu_baseline": None,
            "note": "API-level line (bench.py --api): the kernel-level line with roofline is the default `python bench.py`, cpu_baseline is `python bench.py --full`",
        }
        print(json.dumps(out), flush=True)
        if not args.api_dir:
            shutil.rmtree(root, ignore_errors=True)
    wd.done()
    if world > 1:
        torch.distributed.barrier()
        ctx.comm_destroy()
        torch.distributed.destroy_process_group()


def load_real_inputs(args) -> dict:
    """--api --data-dir: everything the reference's `dream_best_pose` consumes, from the files a reference run leaves in
    method_out/<scene>/ (install.sh:38-50 downloads them; dream2real.py:146-151,356-358, train_ngp.py:145-151 write them) and a Hugging Face
    checkpoint directory (clip_scoring.py:150-151) — loaded and validated on the HOST only.  Every missing input is named."""
    from dream2real_amd import _lib, clip_model
    from dream2real_amd.tokenizer import ClipBpeTokenizer
    d = args.data_dir
    found, missing, problems = {}, [], []

    def need(name, path):
        if os.path.exists(path):
            found[name] = path
            return True
        missing.append(f"{name}: {path}")
        return False

    for k in ("fg", "bg"):
        if need(f"{k}_base.ingp", os.path.join(d, f"{k}_base.ingp")):
            try:
                info = _lib.ingp_validate(open(found[f"{k}_base.ingp"], "rb").read())        # the loader's own checks, no GPU
                found[f"{k}_snapshot"] = {"n_levels": info.n_levels, "n_features": info.n_features, "aabb_scale": info.aabb_scale,
                                          "training_views": info.n_views, "unknown_keys": info.n_unknown_keys}
            except _lib.D2RError as e:
                problems.append(f"{k}_base.ingp: {e}")
    cams = None
    if need("opt_cam_poses.npy", os.path.join(d, "opt_cam_poses.npy")):
        cams = np.load(found["opt_cam_poses.npy"]).reshape(-1, 4, 4)
    obj_path = args.obj_pose or os.path.join(d, "obj_pose.txt")
    obj_pose = np.loadtxt(obj_path).reshape(4, 4) if need("obj_pose.txt (the movable object's world pose, ObjectModel.pose: scene_model.py; the reference "
                                                          "recomputes it instead of caching it — np.savetxt it from a reference session)", obj_path) else None
    ref = {}
    for name in ("pose_scores.txt", "pose_batch.txt", "goal_pose.txt"):
        pth = os.path.join(d, name)
        if os.path.exists(pth):
            ref[name] = np.loadtxt(pth)
    caps = {}
    if args.goal_caption:
        caps = {"goal_caption": args.goal_caption, "norm_captions": args.norm_caption}
    elif os.path.exists(args.captions_json):
        c = json.load(open(args.captions_json))[args.caption_index]
        caps = {"goal_caption": c["goal_caption"], "norm_captions": [c["norm_caption"]], "instruction": c["instruction"]}
    else:
        missing.append(f"captions: --goal-caption / --norm-caption or {args.captions_json}")
    clip = None
    if not args.clip_dir:
        missing.append("--clip-dir (openai/clip-vit-large-patch14-336: model.safetensors, vocab.json, merges.txt)")
    else:
        ok = all(need(f"clip/{f}", os.path.join(args.clip_dir, f)) for f in ("model.safetensors", "vocab.json", "merges.txt"))
        if ok:
            try:
                cfg, sd = clip_model.load_clip_safetensors(os.path.join(args.clip_dir, "model.safetensors"))
                tok = ClipBpeTokenizer.from_files(os.path.join(args.clip_dir, "vocab.json"), os.path.join(args.clip_dir, "merges.txt"), context_length=cfg["ctx"])
                clip = (cfg, sd, tok)
                found["clip"] = {k: cfg[k] for k in ("image_size", "patch_size", "hidden_size", "num_layers", "proj", "vocab", "ctx")}
            except Exception as e:      # noqa: BLE001
                problems.append(f"CLIP checkpoint: {type(e).__name__}: {e}")
    return {"found": found, "missing": missing, "problems": problems, "cams": cams, "obj_pose": obj_pose, "reference_outputs": ref, "captions": caps, "clip": clip}


def run_api_real(args, wd):
    """`python bench.py --api --data-dir method_out/<scene> --clip-dir <checkpoint>`: the drop-in API on the reference's REAL
    artefacts, the day they exist — snapshots through `get_vis_ngps` (reconstruction/ngp_visual_model.py:20-29), the checkpoint through
    `load_clip_safetensors` + the BPE tokenizer + the text tower, captions from the cached LLM pairs, `dream_best_pose` timed as in --api, and then
    the two numbers north_star names: the arg-max pose against the reference run's goal_pose.txt and max |score - pose_scores.txt|.  With the
    reference's pose_scores.txt present, ITS validity mask stands in for the PyBullet pre-filter (zero = invalid, clip_scoring.py:92-94) so that the
    same poses are rendered.  Not reproduced: the sensor-depth background (depths_gt and the movable masks are recomputed from the raw dataset by
    the reference, not cached) — the background depth is the background NeRF's own render (combined_rendering.py:111-113)."""
    import tempfile
    import types
    wd.stage("host-side loading of the real artefacts", 900)
    inp = load_real_inputs(args)
    report = {"data_dir": args.data_dir, "found": inp["found"], "missing": inp["missing"], "problems": inp["problems"],
              "reference_outputs_present": sorted(inp["reference_outputs"]), "captions": inp["captions"]}
    runnable = not inp["problems"] and inp["cams"] is not None and inp["obj_pose"] is not None and inp["clip"] is not None and \
        all(f"{k}_base.ingp" in inp["found"] for k in ("fg", "bg")) and inp["captions"]
    if args.check_only or not runnable:
        report["runnable"] = bool(runnable)
        print(json.dumps({"metric": "bench.py --api --data-dir (host-side check)", "value": None, "real_artifacts": report}), flush=True)
        wd.done()
        return 0 if runnable else 2
    import torch
    from dream2real_amd import dream2real, engine, ngp_visual_model
    from dream2real_amd.geometry_utils import spatially_smooth_heatmap
    cfg, sd, tok = inp["clip"]
    W, H = args.width or 336, args.height or 336                      # the reference hard-wires 336 x 336 (combined_rendering.py:86,121)
    sample_res = [int(x) for x in args.sample_res.split(",")] if args.sample_res else [100, 100, 7, 1, 1, 1]
    torch.cuda.set_device(0)
    wd.device = 0
    wd.stage("models + dream_best_pose", 3600)
    ctx = engine.Context(0)
    ctx.set_option("chunk", args.chunk)
    for kv in args.opt:
        k, v = kv.split("=")
        ctx.set_option(k, int(v))
    fg = ngp_visual_model.get_vis_ngps(None, None, args.scene_type, use_cache=True, data_dir=args.data_dir, fg=True, ctx=ctx)
    bg = ngp_visual_model.get_vis_ngps(None, None, args.scene_type, use_cache=True, data_dir=args.data_dir, fg=False, ctx=ctx)
    scorer, enc = engine.ClipScorer(ctx, cfg, sd), engine.TextEncoder(ctx, cfg, sd)
    centre = [float(x) for x in args.scene_centre.split(",")]
    task = types.SimpleNamespace(
        scene_model=types.SimpleNamespace(scene_centre=torch.tensor(centre, dtype=torch.float32),
                                          opt_cam_poses=[torch.tensor(p, dtype=torch.float32) for p in inp["cams"]], device="cpu"),
        movable_obj=types.SimpleNamespace(vis_model=fg, pose=torch.tensor(inp["obj_pose"], dtype=torch.float32)),
        task_bground_obj=types.SimpleNamespace(vis_model=bg), goal_caption=inp["captions"]["goal_caption"],
        norm_captions=inp["captions"].get("norm_captions"), movable_masks=None)
    ref = inp["reference_outputs"]
    old_scores = ref.get("pose_scores.txt")
    out_dir = args.api_dir or tempfile.mkdtemp(prefix="d2r_real_")
    os.makedirs(out_dir, exist_ok=True)
    pcfg = dream2real.PathConfig(data_dir=out_dir, sample_res=sample_res, scene_type=args.scene_type, render_cam_pose_idx=(args.render_view,),
                                 resolution=(W, H), use_phys=False, save_renders=bool(args.api_save))
    eng = dream2real.ImaginationEngine(pcfg, ctx, scorer, text_encoder=enc, tokenizer=tok)
    if old_scores is not None and old_scores.shape[0] == int(np.prod(sample_res)):
        mask = torch.from_numpy(old_scores != 0)
        # dream_best_pose builds its own pre-filter from mesh files; with use_phys False every pose is valid — the reference run's mask goes in through
        # the same seam (`phys_check`) by wrapping optimise_pose_grid's callable
        from dream2real_amd import clip_scoring
        inner = clip_scoring.optimise_pose_grid

        def with_mask(*a, **k):
            k["phys_check"] = lambda pose_batch, task_model, valid: valid & mask
            return inner(*a, **k)
        clip_scoring.optimise_pose_grid = with_mask
    t0 = time.perf_counter()
    try:
        best, pose_batch, scores = eng.dream_best_pose(task)
    finally:
        if old_scores is not None and old_scores.shape[0] == int(np.prod(sample_res)):
            clip_scoring.optimise_pose_grid = inner          # the wrapper that carried the reference run's validity mask
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    sc = scores.numpy()
    n_valid = int((sc != 0).sum())
    cmp = {}
    if "pose_batch.txt" in ref and ref["pose_batch.txt"].shape == tuple(pose_batch.shape):
        cmp["pose_batch_max_abs_diff"] = float(np.abs(ref["pose_batch.txt"] - pose_batch.numpy()).max())
    if old_scores is not None and old_scores.shape == sc.shape:
        valid = old_scores != 0
        rel = np.abs(sc[valid] - old_scores[valid]) / np.maximum(np.abs(old_scores[valid]), 1e-12)
        cmp.update(max_abs_dscore=float(np.abs(sc - old_scores).max()), max_rel_dscore=float(rel.max()), valid_poses_reference=int(valid.sum()),
                   argmax_ours=int(np.argmax(sc)), argmax_reference=int(np.argmax(old_scores)), argmax_identical=bool(int(np.argmax(sc)) == int(np.argmax(old_scores))))
    if "goal_pose.txt" in ref:
        cmp["goal_pose_max_abs_diff"] = float(np.abs(ref["goal_pose.txt"].reshape(4, 4) - best.numpy()).max())
        cmp["goal_pose_identical"] = bool(cmp["goal_pose_max_abs_diff"] < 1e-5)
    report.update(runnable=True, comparison=cmp or "no reference outputs in the directory (pose_scores.txt / pose_batch.txt / goal_pose.txt)",
                  note="background depth = the background NeRF's render (the sensor-depth background needs depths_gt + movable masks, which the reference recomputes from the raw dataset)")
    print(json.dumps({"metric": f"candidate renders scored/sec ({W}x{H}) through the drop-in API on REAL artefacts", "value": round(n_valid / elapsed, 2),
                      "unit": "candidates/s", "n_gpus": 1, "steps": 1, "warmup": 0, "ms_per_step": round(elapsed * 1e3, 3), "higher_is_better": True,
                      "dtype": "bf16", "data": "real artefacts (first call: includes one-time set-up)",
                      "config": {"workload": f"{args.data_dir}: pose grid {sample_res}, {n_valid} valid poses, {W}x{H}, CLIP {inp['found'].get('clip')}"},
                      "real_artifacts": report}), flush=True)
    wd.done()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", type=int, choices=sorted(BASELINE_CONFIGS), default=None,
                    help="run BASELINE.json configs[C] (default: configs[1], weak over --gpus)")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--poses-per-gpu", type=int, default=None, help="weak scaling: candidates per GPU (a square) -> grid [s,s,N,1,1,1]")
    ap.add_argument("--scaling", choices=("weak", "strong"), default=None)
    ap.add_argument("--poses-total", type=int, default=None,
                    help="strong scaling: total candidates = x*x*8 (131072 = BASELINE.json configs[3])")
    ap.add_argument("--sample-res", default=None, help="six comma-separated grid resolutions x,y,z,rx,ry,rz (overrides the config's)")
    ap.add_argument("--slice-of", type=int, default=None,
                    help="strong scaling on fewer GPUs than the partition: every rank takes shard `rank` of this many (config 4 "
                         "defaults to 8: one GPU = a 1/8 slice; 1 = the whole grid)")
    ap.add_argument("--clip", default=None)
    ap.add_argument("--product-steps", type=int, default=2,
                    help="--full: extra untimed steps after the timed region with an event pair around every product of the vision tower "
                         "(roofline.products: QKV / attention / out-proj / fc1 / fc2); 0 = skip")
    ap.add_argument("--scene", default=None)
    ap.add_argument("--lens", choices=("demo", "none"), default="demo",
                    help="lens of the scene's training views: demo (default) = the OpenCV coefficients the reference's configs carry "
                         "(configs/shopping_demo.json:51-56) — every frame is rendered through set_camera_to_training_view's lens, as in the reference "
                         "(reconstruction/combined_rendering.py:98,116); none = pinhole")
    ap.add_argument("--chunk", type=int, default=4096, help="candidates per pass (the library caps it per model/view)")
    ap.add_argument("--opt", action="append", default=[], help="library tunable key=value (repeatable)")
    ap.add_argument("--vit-fp8", action="store_true",
                    help="the ViT's Linear products on the fp8 MFMA (library option vit_fp8; configs[4] is worded \"fp8 MFMA ViT\"); NOT within "
                         "north_star's 1e-3 of the fp32 oracle, hence not the default")
    ap.add_argument("--cpu-sample", type=int, default=32, help="--full: candidates in the CPU-baseline sample (0 = skip)")
    ap.add_argument("--dump", default=None, help="rank 0: write the last step's gathered logits, scores, pose order and grid to this .npz (tests)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0: write what the last TIMED step computed as DIR/<name>.npy (float32): logits (gathered, [poses per step, 2]), "
                         "scores (smoothed, [poses in the grid]), best_pose (the arg-max pose, [16], world frame)")
    ap.add_argument("--power-seconds", type=float, default=2.5, help="--full: extra untimed seconds sampled with rocm-smi for the power line (0 = skip)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure what the headline figure does not need: the CPU baseline and the parity of its "
                         "sample against the GPU's logits (--cpu-sample), roofline.products (--product-steps) and the power line (--power-seconds)")
    ap.add_argument("--api", action="store_true",
                    help="time the drop-in API (ImaginationEngine.dream_best_pose) instead of the kernel-level step; without --config: "
                         "the reference's own workload (70 000 poses, 336x336, ViT-L/14-336, physics on)")
    ap.add_argument("--api-save", type=int, default=0, help="--api: 1 = write cb_render/*.png for every valid pose, as the reference does")
    ap.add_argument("--api-phys", type=int, default=1, help="--api: 0 = skip the physics pre-filter (every pose valid)")
    ap.add_argument("--text", choices=("synthetic", "tower"), default="synthetic",
                    help="kernel bench: where the C = 2 text embeddings come from.  synthetic (default): seeded unit vectors correlated with the scene's image "
                         "embedding (a well-conditioned goal / norm ratio).  tower: the task's goal / normalising captions (tests/golden/captions.json) -> the "
                         "library's BPE tokenizer -> its text tower (random weights of the same checkpoint) — the reference's caption -> score path end to end; "
                         "random towers have no language prior, so these scores are numerically real and semantically meaningless")
    ap.add_argument("--api-text", choices=("cached", "tower"), default="cached",
                    help="--api: 'tower' = tokenise the task's captions and run the library's text tower inside the timed call")
    ap.add_argument("--api-dir", default=None, help="--api: data_dir root (default: a temporary directory, removed afterwards)")
    ap.add_argument("--data-dir", default=None,
                    help="--api on the reference's REAL artefacts: method_out/<scene>/ with fg_base.ingp, bg_base.ingp, opt_cam_poses.npy (+ the reference "
                         "run's pose_scores.txt / pose_batch.txt / goal_pose.txt to compare against, obj_pose.txt = the movable object's 4x4 world pose)")
    ap.add_argument("--clip-dir", default=None, help="--data-dir: Hugging Face CLIP checkpoint directory (model.safetensors, vocab.json, merges.txt)")
    ap.add_argument("--captions-json", default=os.path.join(REPO, "tests", "golden", "captions.json"), help="--data-dir: goal / normalising captions (lang/cache.json's pairs)")
    ap.add_argument("--caption-index", type=int, default=1, help="--data-dir: entry of --captions-json (1 = the shopping scene's apple / bowl pair)")
    ap.add_argument("--goal-caption", default=None)
    ap.add_argument("--norm-caption", action="append", default=None)
    ap.add_argument("--scene-centre", default="0.5,0.0,0.035", help="--data-dir: scene_centre of the config (configs/shopping_demo.json:29)")
    ap.add_argument("--scene-type", type=int, default=3, help="--data-dir: scene type of sample_poses_grid (shopping 3, pool 0, shelf 1)")
    ap.add_argument("--render-view", type=int, default=0, help="--data-dir: render_cam_pose_idx[0]")
    ap.add_argument("--obj-pose", default=None, help="--data-dir: 4x4 txt of the movable object's pose (default <data-dir>/obj_pose.txt)")
    ap.add_argument("--check-only", action="store_true", help="--data-dir: load and validate every input on the host, print what was found, touch no GPU")
    ap.add_argument("--plan", action="store_true",
                    help="NO GPU NEEDED: every rank works out what it would do in this run (device it would take, its pose shard, launches per step, "
                         "device workspaces, CPU threads) and rank 0 prints the gathered plan as one JSON line — the N-GPU run checked on a CPU box")
    ap.add_argument("--dry-collective", action="store_true",
                    help="only rendezvous + communicator init + one 1 MiB all-gather + argmax agreement (diagnoses a failed --gpus N run)")
    args = ap.parse_args()
    if args.vit_fp8 and "vit_fp8=1" not in args.opt:
        args.opt.append("vit_fp8=1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)
    wd = Watchdog()
    try:
        if args.plan:
            return run_plan(args, wd)
        if args.dry_collective:
            return run_dry_collective(args, wd)
        if args.api and args.data_dir:
            return run_api_real(args, wd)
        if args.api:
            return run_api(args, wd)
        return run_kernel_bench(args, wd)
    except SystemExit:
        raise
    except BaseException as e:              # N > 1: say what broke, on which rank and GPU, and leave at once so that no rank waits in a barrier
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            import traceback
            traceback.print_exc()
            report_failure(wd.stage_name or "setup", f"{type(e).__name__}: {e}", wd.device)
        raise


def run_kernel_bench(args, wd):

    import torch
    from dream2real_amd import dist as d2r_dist
    from dream2real_amd import engine, obj_pose_opt
    from dream2real_amd.accio2ngp import converter
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    from dream2real_amd.clip_scoring import reduce_logits
    from dream2real_amd.geometry_utils import spatially_smooth_heatmap
    from synthetic_scenes import make_scene, make_task, scene_text_embeds

    wd.stage("rendezvous (torch.distributed.init_process_group)", 300)
    rank, world, local = d2r_dist.init_from_env()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    local = local % torch.cuda.device_count()      # several ranks may share a GPU in smoke runs (gloo)
    torch.cuda.set_device(local)
    wd.device = local
    wd.stage("setup (scene, models, background)", 900)
    dev = torch.device("cuda", local)

    # ---------------- which workload
    wl = resolve_workload(args, world)
    base, scene_name, clip_name, W, H = wl["base"], wl["scene"], wl["clip"], wl["width"], wl["height"]
    scaling, sample_res, partition = wl["scaling"], wl["sample_res"], wl["partition"]

    # ---------------- setup (untimed): scene, models, background, poses in HBM
    from dream2real_amd.scene import DEMO_LENS
    scene = make_scene(scene_name, lens=DEMO_LENS if args.lens == "demo" else None)
    cfg = CLIP_CONFIGS[clip_name]
    sd = random_clip_state_dict(cfg, seed=6)
    hbm_free0, hbm_total = torch.cuda.mem_get_info(dev)      # before the library allocates anything: the run's HBM footprint is the difference
    ctx = engine.Context(local)
    ctx.set_option("chunk", args.chunk)
    for k, v in base.get("opts", {}).items():          # what the configuration itself names (configs[4]: fp16 render)
        ctx.set_option(k, int(v))
    for kv in args.opt:
        k, v = kv.split("=")
        ctx.set_option(k, int(v))
    mlp_f16 = bool(ctx.get_option("mlp_f16"))
    fg, bg = scene.testbeds(ctx)       # set_camera_to_training_view(0) on both: the view's intrinsics AND its lens
    scorer = engine.ClipScorer(ctx, cfg, sd)
    task = make_task(scene)
    pose_batch = obj_pose_opt.sample_poses_grid(task, sample_res, scene.scene_type)       # [N,16] world
    N = pose_batch.shape[0]
    plan = shard_plan(sample_res, world, partition)
    order, run_idx, N_run = plan["order"], plan["run_idx"], plan["n_run"]
    my_idx = plan["shards"][rank]
    poses_ngp = converter(pose_batch[my_idx].reshape(-1, 4, 4)).reshape(-1, 16).astype(np.float32)
    poses_dev = torch.from_numpy(poses_ngp).to(dev)
    K_local = poses_dev.shape[0]
    cam_ngp = converter(np.asarray(scene.cam_poses, np.float32))[0]
    bg_rgba, bg_depth = bg.render_batch(cam_ngp[None, :3], W, H)
    view = fg.view(W, H)
    ctx.set_background(view, bg_rgba[0], bg_depth[0])
    T1 = converter(np.asarray(scene.obj_pose, np.float32)[None])[0]
    # cached text embeddings (goal, normalising): seeded unit vectors correlated with the embedding
    # of the un-moved scene, standing in for the text tower output of a real caption pair
    text_info = ("2 seeded unit vectors correlated with the scene's image embedding (random-weight "
                 "towers give uncorrelated text: the goal/norm ratio needs positive logits); "
                 "throughput does not depend on their values")
    if args.text == "tower":
        # captions -> byte-level BPE (the vocabulary committed as data under tests/golden/) -> text tower -> L2-normalised embeddings, once per task
        # (reference clip_scoring.py:153-163,177-181 redoes this per batch)
        from dream2real_amd.clip_scoring import build_captions
        from dream2real_amd.tokenizer import ClipBpeTokenizer
        g = os.path.join(REPO, "tests", "golden")
        tok = ClipBpeTokenizer.from_files(os.path.join(g, "bpe_vocab.json"), os.path.join(g, "bpe_merges.txt"), context_length=32)
        tcfg = dict(cfg, vocab=len(tok.vocab), ctx=32)
        enc = engine.TextEncoder(ctx, tcfg, random_clip_state_dict(tcfg, seed=6))
        captions, _ = build_captions(task.goal_caption, task.norm_captions, False)
        t_tok = time.perf_counter()
        ids = tok(captions)
        text = enc.encode(np.asarray(ids[0] if isinstance(ids, tuple) else ids, np.int32))
        text_info = (f"captions {captions} -> ClipBpeTokenizer -> d2r_text_encode (random-weight text tower, vocabulary of tests/golden/): "
                     f"{(time.perf_counter() - t_tok) * 1e3:.1f} ms once per task, outside the timed steps as in a real run (cached per task)")
    else:
        frame0 = fg.render_composite(view, T1, cam_ngp, T1[None])
        _, e0 = scorer.score_frames(frame0, np.zeros((1, cfg["proj"]), np.float32), return_embeds=True)
        text = scene_text_embeds(e0[0])
    # run the library on a torch-owned (non-null) stream so torch copies order after it
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    # the one collective: the C-ABI communicator (RCCL over xGMI); torch.distributed only bootstraps it
    # (id blob) and provides the timing barrier
    wd.stage("d2r_comm_init (ncclCommInitRank)", 300)
    c_abi_comm = d2r_dist.init_comm(ctx, rank, world)
    wd.stage("warmup steps (render + score + all-gather)", 900)
    # gathered layout: `world` shards of the partition in rank order (padded to the largest inside the exchange)
    N_gather = N_run
    gather = d2r_dist.ShardGather(ctx, N_gather, text.shape[0], rank, world, dev, c_abi_comm)
    logits_dev = gather.local

    def step():
        engine.render_score_device(ctx, fg, scorer, view, T1, cam_ngp, poses_dev.data_ptr(), K_local, text,
                                   logits_dev.data_ptr())
        lg = gather.gather()                                               # [N_gather, C], shard order (ONE all-gather at N>1)
        step.logits = lg
        scores = np.zeros(N, np.float32)
        scores[run_idx] = reduce_logits(lg, 1, True)                       # poses outside a slice stay 0 = "invalid" (clip_scoring.py:205-209)
        scores = spatially_smooth_heatmap(scores, sample_res)
        return int(np.argmax(scores)), scores

    def barrier():
        torch.cuda.synchronize(dev)
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        step()
    ctx.set_option("timing", 1)
    barrier()
    wd.stage("timed steps (render + score + all-gather)", 600 + 120 * args.steps)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        best, scores = step()
    barrier()
    elapsed = time.perf_counter() - t0
    if rank == 0 and args.dump_outputs:
        # before any untimed step of --full can overwrite them: what a caller of the timed path receives from its last step
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in (("logits", step.logits), ("scores", scores), ("best_pose", pose_batch[best])):
            np.save(os.path.join(args.dump_outputs, f"{name}.npy"), np.asarray(a, np.float32))
    wd.stage("result reduction (all_reduce) and report", 1200)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=dev if torch.distributed.get_backend() == "nccl" else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    ranks_seen = 1
    if world > 1:
        t = torch.ones(1, dtype=torch.int32, device=dev if torch.distributed.get_backend() == "nccl" else "cpu")
        torch.distributed.all_reduce(t)
        ranks_seen = int(t.item())
    timing = ctx.timing()
    ctx.set_option("timing", 0)
    stats = ctx.render_stats(collect_K=K_local)          # counters of the last step
    # per-product device time of the vision tower ("timing" 2: an event pair around every product launch) over EXTRA, untimed
    # steps after the timed region — the events cost a few tenths of a per cent of a step, so they stay out of `value`
    vit_products = None
    if rank == 0 and world == 1 and args.full and args.product_steps > 0:
        ctx.set_option("timing", 2)
        for _ in range(args.product_steps):
            step()
        torch.cuda.synchronize(dev)
        vit_products = ctx.timing()
        ctx.set_option("timing", 0)
    brick_config = {"lds_slots": ctx.get_option("march_lds_slots"), "hbm_brick_slots": ctx.get_option("march_hbm_brick_slots")}

    launches_per_step = max(1, round(timing["march_launches"] / max(1, args.steps)))
    per_launch = -(-K_local // launches_per_step)          # candidates per k_march launch actually used

    def recorded_traffic():
        """HBM-side bytes per k_march launch from the committed PMC passes (bench.py cannot run
        under --pmc itself); only reported when it was measured on this exact workload."""
        for name in ("r06_march_traffic.json", "r05_march_traffic.json", "r04_march_traffic.json", "r03_march_traffic.json", "r01_march_traffic.json"):
            try:
                t = json.load(open(os.path.join(REPO, "profiles", name)))
            except OSError:
                continue
            wl = t["workload"]
            if (wl["scene"], wl["width"], wl["height"], wl["chunk"], wl["clip"]) != (scene_name, W, H, per_launch, clip_name):
                continue
            return t["traffic_bytes_per_launch"], f"profiles/{name} ({t.get('how', 'FETCH_SIZE+WRITE_SIZE')})"
        return None, None

    if rank == 0:
        total = N_run * args.steps
        traffic, traffic_src = recorded_traffic()
        value = total / elapsed
        samples_per_launch = stats["samples"] / launches_per_step
        march_avg_s = timing["march_ms"] / max(1, timing["march_launches"]) * 1e-3
        achieved = samples_per_launch * ALGO_BYTES_PER_SAMPLE / march_avg_s / 1e9 if march_avg_s > 0 else 0.0
        n_img = K_local * args.steps
        # MFMA utilisation is priced on the flops the library issues (class-token-only last block), not on the
        # textbook count of the architecture
        cls_last = "cls_last=0" not in args.opt
        l0_frac = stats["l0_touched"] / stats["l0_tokens"] if stats.get("l0_tokens") else 1.0       # of the last step (every step touches the same tokens)
        gflop_exec = vit_gflop(cfg, executed=cls_last, l0_touched=l0_frac) if cls_last else vit_gflop(cfg) - (vit_gflop(cfg, True) - vit_gflop(cfg, True, l0_frac))
        clip_tflops = gflop_exec * 1e9 * n_img / (timing["clip_ms"] * 1e-3) / 1e12 if timing["clip_ms"] > 0 else None
        # option vit_fp8: part of those flops are issued on the fp8 MFMA (twice the bf16 rate): the ViT's peak is the harmonic blend
        # (the library runs the fp8 blocks for hidden / MLP sizes that are multiples of 256 with the hi + lo-byte residual, ln_fold 4 — its default)
        vit_fp8 = ("vit_fp8=1" in args.opt and cfg["hidden_size"] % 256 == 0 and cfg["mlp"] % 256 == 0 and cfg["mlp"] >= 2 * cfg["hidden_size"]
                   and not any(o.startswith("ln_fold=") and o != "ln_fold=4" for o in args.opt))
        f8_share = min(1.0, vit_fp8_gflop(cfg, bool(stats.get("l0_tokens"))) / gflop_exec) if vit_fp8 else 0.0
        vit_peak = 1.0 / (f8_share / MFMA_FP8_PEAK_TFLOPS + (1.0 - f8_share) / MFMA_BF16_PEAK_TFLOPS)
        mlp_tflops = samples_per_launch * MLP_FLOP_PER_SAMPLE / march_avg_s / 1e12 if march_avg_s > 0 else None
        sort_avg_s = timing.get("sort_ms", 0.0) / max(1, timing.get("sort_launches", 0) or 1) * 1e-3
        products = vit_product_table(vit_products, cfg, per_launch, vit_peak) if vit_products else None
        vit_traffic, vit_traffic_src, march_pmc = recorded_pmc(scene_name, W, H, per_launch, clip_name)
        # name the workload from what actually ran: the BASELINE.json config whose scene / grid / size / encoder it is
        per_gpu_res = sample_res[:2] + [1] + sample_res[3:] if scaling == "weak" else sample_res
        match = [k for k, c in BASELINE_CONFIGS.items()
                 if (c["scene"], c["sample_res"], c["width"], c["height"], c["clip"], c["scaling"]) == (scene_name, per_gpu_res, W, H, clip_name, scaling)]
        label = f"BASELINE.json configs[{match[0]}]: {BASELINE_CONFIGS[match[0]]['name']}" if match else "custom (not a BASELINE.json config)"
        what = (f"{scene_name} scene, pose grid {sample_res} = {N} candidates (scene type {scene.scene_type}), {W}x{H}, {'fp16' if mlp_f16 else 'bf16'} MLP + {clip_name}, "
                + (f"{scaling} scaling over {world} GPU(s)" if world > 1 else "one GPU"))
        if N_run != N:
            what += f"; SLICE: shards 0..{world - 1} of a {partition}-way partition = {N_run} of the {N} candidates per step (the rest of the grid scores 0)"
        rccl = None
        try:
            rccl = ".".join(str(x) for x in torch.cuda.nccl.version())
        except Exception:
            pass
        out = {
            "metric": f"candidate renders scored/sec ({W}x{H})", "value": round(value, 2), "unit": "candidates/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": scaling,
            "vs_baseline": None,
            "dtype": ("fp8 e4m3 Linear products (fp32 accumulate) in the ViT, bf16 elsewhere" if vit_fp8 else "bf16")
                     + (" + fp16 NeRF MLP operands (fp32 accumulate; the library's default: the reference's tiny-cuda-nn operand type, same MFMA rate; --opt mlp_f16=0 = bf16 operands)" if mlp_f16 else " (NeRF MLPs too: --opt mlp_f16=0)"),
            "data": "synthetic", "ranks_seen": ranks_seen,
            "config": {"workload": f"{label} — ran: {what}",
                       "baseline_config": match[0] if match else None,
                       "scene": scene_name, "clip": clip_name, "width": W, "height": H,
                       "poses_total": N, "poses_per_step": N_run, "sample_res": sample_res, "chunk": per_launch,
                       "parallelism": f"pose-shard x{world}" if world > 1 else "single GPU",
                       "collective": ("none (single GPU)" if world == 1 else
                                      "d2r_allgather_scores: one ncclAllGather (RCCL) of fp32 logits per step" if c_abi_comm else
                                      f"torch.distributed all_gather ({torch.distributed.get_backend()}): ranks share a GPU, RCCL unavailable"),
                       "rccl_version": rccl,
                       "lens": (f"OpenCV k1, k2, p1, p2 = {list(scene.lens)} (configs/shopping_demo.json:51-56) on every ray, as set_camera_to_training_view leaves it"
                                if scene.lens else "none (pinhole)"),
                       "text_embeds": text_info},
            # The step's dominant kernel family by time (86 % of the device time at configs[1]) is the vision tower: MFMA-bound by shape
            # (dense contractions), priced on the flops the library ISSUES against the dense bf16 MFMA peak.  `products` = the same figure
            # per product, from HIP events around every launch (extra untimed steps).  No field named `frac` here can exceed 1.
            "roofline": {"bound": "mfma", "kernel": "vision tower (k_gemm8<EPI> QKV / out-proj / fc1 / fc2 + k_attention_s + small kernels)",
                         "achieved": round(clip_tflops, 2) if clip_tflops else None, "peak": round(vit_peak, 1), "unit": "TFLOP/s",
                         "frac": round(clip_tflops / vit_peak, 5) if clip_tflops else None,
                         "traffic": vit_traffic, "traffic_source": vit_traffic_src,
                         "share_of_device_time": round(timing["clip_ms"] / max(1e-9, sum(timing.get(k, 0.0) for k in ("march_ms", "raygen_ms", "sort_ms", "prep_ms", "clip_ms"))), 4),
                         "gflop_per_image": round(gflop_exec, 2), "gflop_per_image_architecture": round(vit_gflop(cfg), 2),
                         "l0_touched_fraction": round(l0_frac, 4), "fp8_share_of_flops": round(f8_share, 4),
                         "products": products,
                         "note": "flops the library issues: last block's q, attention output, out-proj and MLP on the class token only (the head reads nothing else); "
                                 "patch embedding and layer-0 QKV on the patch tokens a candidate can have touched only (the others take the background's rows) — both exact.  "
                                 "products: per full-size launch of the default schedule, flops / event time / peak"},
            # k_march is NOT HBM-bound once the ray sort makes its lookups L2-resident (fabric traffic = 0.5 % of the HBM peak): it is bound by
            # VALU issue and dependent chains.  north_star's "hash-grid fetch" figure (algorithmic bytes / launch time / 8 TB/s, target >= 0.40)
            # counts the levels served from LDS bricks too and can exceed 1: it is reported under its own name, not as a roofline fraction.
            "march": {"bound": "valu-issue", "kernel": "k_march (hash-grid fetch + fused MLP + compositing)",
                      "avg_launch_ms": round(march_avg_s * 1e3, 4),
                      "sort_ms_per_launch": round(sort_avg_s * 1e3, 4),
                      "samples_per_launch": int(samples_per_launch),
                      "lane_utilisation": round(stats["samples"] / max(1, 64 * stats["wave_iters"]), 4),
                      "brick_config": brick_config,
                      "mlp_tflops": round(mlp_tflops, 3) if mlp_tflops else None,
                      "mlp_frac_of_mfma_peak": round(mlp_tflops / MFMA_BF16_PEAK_TFLOPS, 5) if mlp_tflops else None,
                      "hash_fetch_algorithmic_GBps": round(achieved, 2),
                      "hash_fetch_algorithmic_bytes_per_launch": int(samples_per_launch * ALGO_BYTES_PER_SAMPLE),
                      "hash_fetch_algorithmic_ratio": round(achieved / HBM_PEAK_GBPS, 5),
                      "hash_fetch_algorithmic_ratio_with_sort": round(samples_per_launch * ALGO_BYTES_PER_SAMPLE / (march_avg_s + sort_avg_s) / 1e9 / HBM_PEAK_GBPS, 5) if march_avg_s > 0 else None,
                      "hash_fetch_target": 0.40,
                      "levels_beyond_lds": 16 - 2 * int((brick_config or {}).get("lds_slots", 0)),
                      "hash_fetch_beyond_lds_ratio": round(achieved * (16 - 2 * int((brick_config or {}).get("lds_slots", 0))) / 16 / HBM_PEAK_GBPS, 5),
                      "fabric_traffic_bytes_per_launch": traffic, "fabric_traffic_source": traffic_src,
                      "fabric_frac": round(traffic / march_avg_s / 1e9 / HBM_PEAK_GBPS, 5) if (traffic and march_avg_s > 0) else None,
                      "pmc": march_pmc,
                      "note": "hash_fetch_algorithmic_ratio = samples x 512 B (16 levels x 8 corners x 4 B, SURVEY.md 8(d)) / k_march launch time / 8 TB/s — north_star's formula, "
                              "NOT a roofline fraction: 10 of 16 levels come from LDS bricks and the rest hit L2 at 0.99, so it can exceed 1 (the ..._with_sort variant "
                              "charges the ray sort's passes, timed separately, to the launch).  What bounds the kernel: VALU issue (pmc.valu_busy) with the MLPs at "
                              "mlp_frac_of_mfma_peak of the bf16 MFMA peak; fabric_frac is what HBM / Infinity Fabric actually carries"},
            "device_ms_per_step": {k.replace("_ms", ""): round(v / args.steps, 3) for k, v in timing.items() if k.endswith("_ms") and not k.startswith("vit_")},
            "render_stats_per_step": stats,
            "argmax_pose": best,
            # what this rank holds in HBM after the timed steps (models, weights, every workspace; torch's own context included): the same on
            # every rank of an N-GPU run, whose per-GPU work is this run's (`bench.py --plan` lists the terms)
            "hbm_footprint": {"bytes": int(hbm_free0 - torch.cuda.mem_get_info(dev)[0]), "of": int(hbm_total),
                              "workspace_estimate": device_workspace_estimate(per_launch, W, H, cfg, bool(ctx.get_option("ray_sort")))},
        }
        out["roofline_vit"] = out["roofline"]          # the name older readers look for: the same object
        if world == 1:
            out["power"] = power_probe(step, dev.index or 0, args.power_seconds) if args.full else None
        if world == 1 and args.full and args.cpu_sample > 0:
            cb, frames_o, lg_o, idx = cpu_baseline(scene, W, H, cfg, sd, text, pose_batch[my_idx], args.cpu_sample)
            out["cpu_baseline"] = cb
            # same candidates through the GPU path: parity of the benchmark itself
            lg_gpu = logits_dev[:K_local].cpu().numpy()[idx]
            out["parity_vs_oracle"] = {"max_cosine_err": float(np.abs(lg_gpu - lg_o).max() / scorer.logit_scale),
                                       "n": int(len(idx))}
            if vit_fp8:
                out["parity_vs_oracle"]["note"] = ("option vit_fp8 (BASELINE.json configs[4]'s \"fp8 MFMA ViT\"): e4m3 operands are outside north_star's "
                                                   "1e-3 cosine of the fp32 oracle by construction (tests/test_fp8.py holds the kernels to the format's restatement)")
        elif world > 1:
            out["cpu_baseline"] = {"value": None, "unit": "candidates/s", "cores": effective_cpus(), "kind": "port",
                                   "sample": "timed on rank 0 at n_gpus = 1 only: see the n_gpus = 1 line of the same --config"}
        else:
            out["cpu_baseline"] = None
        if args.dump:
            np.savez(args.dump, logits=step.logits, scores=scores, run_idx=run_idx, sample_res=np.asarray(sample_res), best=best,
                     pose_batch=pose_batch)
        print(json.dumps(out), flush=True)
    wd.done()
    if world > 1:
        torch.distributed.barrier()
        ctx.comm_destroy()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main() or 0)
