#!/usr/bin/env python
"""Time the TSDF physics backend at the reference's workload: 70 000 poses (100 x 100 x 7 positions, one
orientation) against the touch field of a synthetic table-top scene of 1 m x 1 m x 0.5 m at 2 mm — a table slab with a few boxes
of clutter, each a shell 16 mm deep as a TSDF leaves it — and a 10 cm box as the movable object (its shell's voxels as points).

Prints one JSON line and writes it to profiles/sdfphys_bench.json: point count, milliseconds per call with transfers (host wall
clock around the synchronous call, and the three device-event segments) and without (the kernel's device events), point-probe
lookups per second counted as poses x points x 6 (an upper count: waves leave early and skip decided probes), and the share of
point-probe pairs the coarse mask rejected, estimated with numpy on a sample of poses.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
VOXEL, SHELL = np.float32(0.002), 8          # voxels of shell = trunc / voxel


def shell(touch, lo, hi):
    """Set the SHELL-deep shell of the box [lo, hi) (voxel indices x, y, z), as seen from above and the sides."""
    box = np.zeros_like(touch)
    box[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    inner = np.zeros_like(touch)
    inner[:max(lo[2], hi[2] - SHELL), lo[1] + SHELL:hi[1] - SHELL, lo[0] + SHELL:hi[0] - SHELL] = True
    touch |= box & ~inner


def scene():
    nv = np.array([512, 512, 256], np.uint32)                    # 1.024 m x 1.024 m x 0.512 m in whole blocks
    b0 = np.array([-16, -16, -4], np.int32)
    touch = np.zeros((256, 512, 512), bool)
    shell(touch, (6, 6, 0), (506, 506, 64))                      # the table: top at voxel 63 (z = 0 at voxel 64 - 4 * 16 = 0)
    rng = np.random.default_rng(3)
    for _ in range(6):                                           # clutter on it
        x, y = rng.integers(60, 400, 2)
        w, d, h = rng.integers(30, 80, 3)
        shell(touch, (x, y, 64), (x + w, y + d, 64 + h))
    k = np.arange(50)                                            # the movable box: 10 cm, its SHELL-deep shell as points
    zz, yy, xx = np.meshgrid(k, k, k, indexing="ij")
    edge = (np.minimum(xx, 49 - xx) < SHELL) | (np.minimum(yy, 49 - yy) < SHELL) | (np.minimum(zz, 49 - zz) < SHELL)
    corner = np.array([231, 231, 66])
    g = np.stack([xx[edge], yy[edge], zz[edge]], 1) + corner + b0.astype(np.int64) * 16
    pts = g.astype(np.float32) * VOXEL
    init = np.eye(4)
    init[:3, 3] = (corner + 25 + b0.astype(np.int64) * 16) * 0.002
    return b0, nv, touch, pts, init


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=24, help="poses the coarse-mask share is estimated on")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sdfphys_bench.json"))
    a = ap.parse_args()
    from dream2real_amd import engine
    from dream2real_amd.physics_utils import SdfPhysicsShapes
    from tests import sdfphys_ref
    b0, nv, touch, pts, init = scene()
    words = sdfphys_ref.pack_bits(touch)
    res = (100, 100, 7, 1, 1, 1)
    xs, ys, zs = np.linspace(-0.4, 0.4, 100), np.linspace(-0.4, 0.4, 100), np.linspace(-0.02, 0.22, 7)
    poses = np.tile(init, (70000, 1, 1))
    poses[:, :3, 3] += np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3)
    ctx = engine.Context(0)
    shapes = SdfPhysicsShapes(ctx, b0, nv, VOXEL, words, pts)
    ones = np.ones(len(poses), bool)
    table_z = float(init[2, 3]) - 0.2
    valid = shapes.check(poses, ones, res, init, table_z)           # warm-up
    wall, seg = [], []
    for _ in range(a.reps):
        t = time.perf_counter()
        valid = shapes.check(poses, ones, res, init, table_z)
        wall.append((time.perf_counter() - t) * 1e3)
        seg.append(shapes.timing())
    shapes.close()
    ctx.close()
    seg = np.array(seg)
    kernel_ms = float(np.median(seg[:, 1]))
    # the coarse mask's share, on a sample: point-probe pairs whose voxel lies outside the grid or in a 16^3 block without a bit
    idx = np.random.default_rng(0).choice(len(poses), a.sample, replace=False)
    T = sdfphys_ref.transforms(poses[idx], init)
    tq = sdfphys_ref.probe_translations(T, 0.02, sdfphys_ref.GRAVITY, 0.04)
    coarse = touch.reshape(16, 16, 32, 16, 32, 16).any((1, 3, 5))
    lo = b0.astype(np.int64) * 16
    rejected = total = 0
    for n in range(len(idx)):
        r = [(T[n, k, 0] * pts[:, 0] + T[n, k, 1] * pts[:, 1]) + T[n, k, 2] * pts[:, 2] for k in range(3)]
        for q in range(6):
            f = [np.floor((r[k] + tq[n, q, k]) / VOXEL + np.float32(0.5)).astype(np.int64) - lo[k] for k in range(3)]
            inside = np.ones(len(pts), bool)
            for k in range(3):
                inside &= (f[k] >= 0) & (f[k] < int(nv[k]))
            c = [np.where(inside, f[k], 0) >> 4 for k in range(3)]
            rejected += int((~inside | ~coarse[c[2], c[1], c[0]]).sum())
            total += len(pts)
    out = dict(workload="70 000 poses (100 x 100 x 7, one orientation), table-top field 512 x 512 x 256 voxels of 2 mm, 10 cm box",
               poses=len(poses), points=int(len(pts)), valid=int(valid.sum()), field_mib=round(words.nbytes / 2 ** 20, 2),
               ms_per_call_with_transfers_wall=round(float(np.median(wall)), 4),
               ms_upload_kernel_download_events=[round(float(x), 4) for x in np.median(seg, 0)],
               ms_per_call_without_transfers=round(kernel_ms, 4),
               point_probe_lookups_per_s_upper_count=float(len(poses) * len(pts) * 6 / (kernel_ms * 1e-3)),
               coarse_mask_rejected_share_sampled=round(rejected / total, 4), sample_poses=int(a.sample), reps=int(a.reps))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
