#!/usr/bin/env python
"""Times the two batch mask calls on one GPU: 100 frames of 1280x720 with a realistic label image (a table, six objects, speckle).
Per call: ms per frame with the transfers (wall clock) and from device events alone, the bytes moved by design (DESIGN.md section
4) and the fraction of the HBM bound the kernels reach.  With --profile a child process first runs the same calls under
`rocprofv3 --kernel-trace`; its trace gives each kernel's time, their sum per call and the span from the call's first kernel to its
last, so that the event time can be held against the sum of the kernels (a call that waited on the host between frames would show a
span, and an event time, far above the sum).  Writes profiles/masks_bench.json."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BYTES_PER_S = 8e12
# bytes per pixel each kernel must move; the prune figures are for a labelled pixel, duplicate mode, with oob
KERNEL_BYTES_PER_PX = {
    "scene_bound_masks": {"k_scene_bounds": 2.125, "k_morph<false>": 0.25, "k_morph<true>": 0.25, "k_unpack": 1.125},
    "masks_prune": {"k_label_tiles": 5.0, "k_label_seams": 1.0, "k_label_flatten": 9.0, "k_comp_stats": 7.0, "k_select<0>": 5.0,
                    "k_select<1>": 5.0, "k_prune_write": 7.0},
}
BYTES_PER_PX = {name: sum(k.values()) for name, k in KERNEL_BYTES_PER_PX.items()}
FIRST_KERNEL = {"scene_bound_masks": "k_scene_bounds", "masks_prune": "k_select_init"}
KERNELS_OF = {"scene_bound_masks": ("k_scene_bounds", "k_morph", "k_unpack"),
              "masks_prune": ("k_select_init", "k_label_tiles", "k_label_seams", "k_label_flatten", "k_comp_stats", "k_select", "k_prune_write")}


def short_name(full):
    """'(anonymous namespace)::k_morph<true>(...)' or the mangled '..7k_morphILb1EE..' -> 'k_morph<true>'; None for a kernel of
    another module."""
    for names in KERNELS_OF.values():
        for k in sorted(names, key=len, reverse=True):
            if k not in full:
                continue
            if k not in ("k_morph", "k_select"):
                return k
            m = re.match(r"<(\w+)>|IL[bi](\d)E", full[full.index(k) + len(k):])
            arg = (m.group(1) or m.group(2)) if m else "?"
            if k == "k_morph":
                arg = {"0": "false", "1": "true"}.get(arg, arg)
            return "%s<%s>" % (k, arg)
    return None


def read_trace(folder):
    """rocprofv3's kernel trace -> [(short name, start ns, end ns)] in start order."""
    files = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise RuntimeError("rocprofv3 wrote no kernel trace under " + folder)
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = short_name(r["Kernel_Name"])
                if name:
                    rows.append((name, int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    return sorted(rows, key=lambda r: r[1])


def calls_of(rows, name):
    """The trace split into this call's invocations: [[(kernel, start, end), ...], ...]."""
    mine = [r for r in rows if r[0].split("<")[0] in KERNELS_OF[name]]
    calls = []
    for r in mine:
        if r[0] == FIRST_KERNEL[name]:
            calls.append([])
        if calls:
            calls[-1].append(r)
    return calls


def profile(a):
    """Runs this tool's calls in a child under rocprofv3 --kernel-trace -> {call: per-kernel ms, their sum, the span} of the last
    (warm) invocation, all per call of a.frames frames."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    folder = tempfile.mkdtemp(prefix="masks_trace_")
    try:
        cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", folder, "--", sys.executable, os.path.abspath(__file__), "--frames",
               str(a.frames), "--width", str(a.width), "--height", str(a.height), "--repeat", "1", "--out", os.path.join(folder, "child.json")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
        rows = read_trace(folder)
        child = json.load(open(os.path.join(folder, "child.json")))
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    out = {}
    for name in KERNELS_OF:
        calls = calls_of(rows, name)
        if len(calls) < 2:
            raise RuntimeError("the trace holds %d invocations of %s, expected 2" % (len(calls), name))
        last = calls[-1]
        per = {}
        for k, s, e in last:
            per[k] = per.get(k, 0.0) + (e - s) * 1e-6
        out[name] = dict(kernel_ms=per, kernel_sum_ms=sum(per.values()), first_to_last_kernel_span_ms=(last[-1][2] - last[0][1]) * 1e-6,
                         launches=len(last), device_events_ms_under_trace=child[name]["ms_per_frame_device_events"] * a.frames)
    return out


def scene(n, w, h, seed=0):
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    label = np.zeros((h, w), np.uint8)
    label[h // 3:, w // 8: w - w // 8] = 1                                   # the table
    for k in range(6):                                                       # six objects on it
        ci, cj, r = rng.integers(h // 2, h - 60), rng.integers(w // 5, w - w // 5), rng.integers(30, 70)
        label[(ii - ci) ** 2 + (jj - cj) ** 2 < r * r] = 2 + k
    masks = np.repeat(label[None], n, 0)
    speck = rng.random((n, h, w)) < 0.002                                    # speckle: small wrong components of the objects' labels
    masks[speck] = rng.integers(2, 8, int(speck.sum())).astype(np.uint8)
    depth = (900 + 0.5 * ii[None] + rng.integers(-5, 6, (n, h, w))).astype(np.uint16)
    depth[rng.random((n, h, w)) < 0.03] = 0
    poses = np.repeat(np.eye(4, dtype=np.float32)[None], n, 0)
    poses[:, 0, 3] = np.linspace(-0.1, 0.1, n)
    K = np.array([[900.0, 0, (w - 1) / 2], [0, 900.0, (h - 1) / 2], [0, 0, 1]])
    return masks, depth, poses, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "masks_bench.json"))
    ap.add_argument("--profile", action="store_true", help="first trace the kernels in a child process under rocprofv3")
    a = ap.parse_args()
    traced = profile(a) if a.profile else None               # before this process opens the GPU
    from dream2real_amd import _lib, engine
    ctx = engine.Context(0)
    masks, depth, poses, K = scene(a.frames, a.width, a.height)
    bounds = np.array([[-0.4, -0.3, -0.1], [0.4, 0.3, 1.2]])
    centre = np.array([0.0, 0.1, 1.0])
    px = a.width * a.height
    res = dict(frames=a.frames, width=a.width, height=a.height, hbm_bytes_per_s=HBM_BYTES_PER_S)
    oob = None
    for name in ("scene_bound_masks", "masks_prune"):
        wall, dev, xfer = [], [], []
        for _ in range(a.repeat + 1):                                        # the first round grows the workspaces
            t0 = time.perf_counter()
            if name == "scene_bound_masks":
                oob = _lib.scene_bound_masks(ctx, depth, poses, K, bounds, 50)
            else:
                _lib.masks_prune(ctx, 0, masks, depth, oob, poses, K, centre)
            wall.append((time.perf_counter() - t0) * 1e3)
            up, k, down = _lib.masks_timing(ctx)
            dev.append(k)
            xfer.append(up + down)
        w_ms, k_ms, x_ms = min(wall[1:]) / a.frames, min(dev[1:]) / a.frames, min(xfer[1:]) / a.frames
        bound_ms = BYTES_PER_PX[name] * px / HBM_BYTES_PER_S * 1e3
        res[name] = dict(ms_per_frame_with_transfers=w_ms, ms_per_frame_device_events=k_ms, ms_per_frame_transfer_events=x_ms,
                         design_bytes_per_frame=BYTES_PER_PX[name] * px, hbm_bound_ms_per_frame=bound_ms, fraction_of_hbm_bound=bound_ms / k_ms)
        if traced:
            t = traced[name]
            t["kernel_fraction_of_hbm_bound"] = {k: KERNEL_BYTES_PER_PX[name][k] * px * a.frames / HBM_BYTES_PER_S * 1e3 / ms
                                                 for k, ms in t["kernel_ms"].items() if k in KERNEL_BYTES_PER_PX[name]}
            t["device_events_over_kernel_sum"] = k_ms * a.frames / t["kernel_sum_ms"]
            res[name].update(t)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
