#!/usr/bin/env python
"""Times the building of the point-cloud ablation's visual clouds on one GPU: 20 frames of 1280x720 with a realistic label image
(a table, six objects), every label's cloud over every view, voxel-downsampled at 0.002 (get_vis_pcds with pcds_type 1).  Per call
of d2r_pcd_build: the wall time with the transfers and the read-back of the clouds, the device-event times of the upload and of
the kernels; and, in the same process on the same inputs, the time of the host path (pcd_visual_model.get_vis_pcds without a
context), whose clouds the device's are checked against.  Writes profiles/pcd_build_bench.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def scene(n, w, h, seed=0):
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    label = np.zeros((h, w), np.uint8)
    label[h // 3:, w // 8: w - w // 8] = 1                                   # the table
    for k in range(6):                                                       # six objects on it
        ci, cj, r = rng.integers(h // 2, h - 60), rng.integers(w // 5, w - w // 5), rng.integers(30, 70)
        label[(ii - ci) ** 2 + (jj - cj) ** 2 < r * r] = 2 + k
    masks = np.repeat(label[None], n, 0)
    depth = ((900 + 0.5 * ii[None] + rng.integers(-5, 6, (n, h, w)) + 0.25) / 1000.0).astype(np.float32)
    depth[rng.random((n, h, w)) < 0.03] = 0
    rgbs = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    poses = np.repeat(np.eye(4)[None], n, 0)
    poses[:, 0, 3] = np.linspace(-0.1, 0.1, n)
    K = np.array([[900.0, 0, (w - 1) / 2], [0, 900.0, (h - 1) / 2], [0, 0, 1]])
    return rgbs, depth, masks, poses, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host-views", type=int, default=0, help="time the host path on this many views only and scale (0: all of them)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pcd_build_bench.json"))
    a = ap.parse_args()
    from dream2real_amd import _lib, engine
    from dream2real_amd import pcd_visual_model as pvm
    ctx = engine.Context(0)
    rgbs, depth, masks, poses, K = scene(a.frames, a.width, a.height)
    bounds = np.array([[-0.45, -0.3, 0.5], [0.45, 0.3, 1.2]])
    num_objs = 8
    args = (list(rgbs), list(depth), list(poses), K, list(masks), num_objs, bounds)
    wall, up, dev = [], [], []
    for _ in range(a.repeat + 1):                                            # the first call loads the kernels
        t0 = time.perf_counter()
        clouds = pvm.get_vis_pcds(*args, use_cache=False, pcds_type=1, ctx=ctx)
        wall.append((time.perf_counter() - t0) * 1e3)
        u, k = _lib.pcd_build_timing(ctx)
        up.append(u)
        dev.append(k)
    hv = a.host_views or a.frames
    hargs = tuple(x[:hv] if isinstance(x, list) else x for x in args)
    t0 = time.perf_counter()
    host = pvm.get_vis_pcds(*hargs, use_cache=False, pcds_type=1)
    host_ms = (time.perf_counter() - t0) * 1e3 * a.frames / hv
    same = True
    if hv == a.frames:
        same = all(np.array_equal(c.xyz, h.xyz) and np.array_equal(c.rgb, h.rgb) for c, h in zip(clouds, host))
    res = dict(frames=a.frames, width=a.width, height=a.height, objects=num_objs, voxel=pvm.FRAME_VOXEL_SIZE,
               points_out=[len(c) for c in clouds], call_ms_wall_with_transfers_and_read_back=min(wall[1:]),
               upload_ms_device_events=min(up[1:]), kernels_ms_device_events=min(dev[1:]), host_path_ms=host_ms,
               host_views_timed=hv, host_over_device_wall=host_ms / min(wall[1:]), equal_to_host_path=bool(same))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    if not same:
        sys.exit("the device clouds differ from the host path's")


if __name__ == "__main__":
    main()
