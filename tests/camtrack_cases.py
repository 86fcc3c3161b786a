"""The scenes of tests/test_camtrack_*.py: analytic 320 x 240 depth frames of a slab carrying two spheres of different radii and a
box (all six degrees of freedom of a camera are constrained), the poses they are seen from, the perturbed poses to refine, and the
hand-made frames of the edge cases.  tests/tsdf_scene.py's sphere on a slab is the DEGENERATE case: symmetric about the sphere's axis,
its system is singular in yaw."""
from __future__ import annotations

import numpy as np

from tests import tsdf_scene

W, H = tsdf_scene.W, tsdf_scene.H
INTRINSICS = tsdf_scene.INTRINSICS
BOUNDS = tsdf_scene.BOUNDS                     # 0.18 x 0.18 x 0.11 m: 90 x 90 x 55 voxels of 2 mm before the padding
SLAB_LO, SLAB_HI = tsdf_scene.SLAB_LO, tsdf_scene.SLAB_HI
SPHERES = ((np.array([-0.035, -0.03, 0.03]), 0.03), (np.array([0.045, -0.035, 0.018]), 0.018))
BOX_LO, BOX_HI = np.array([-0.01, 0.025, 0.0]), np.array([0.05, 0.065, 0.035])
N_FUSED = 3                                    # frames 0 .. 2 are fused at their true poses, frame TRACKED is refined
TRACKED = 3
THR = 1.0                                      # the scan's weight threshold while it is being fused


def _slab(o, d, lo, hi):
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    tn, tf = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
    return np.where((tn <= tf) & (tn > 0), tn, np.inf)


def raycast(T, w=W, h=H, K=INTRINSICS):
    """-> uint16 [h,w] millimetres (rounded to nearest; 0 = nothing hit) of the scene seen from the camera-to-world pose T."""
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    d = np.stack([(jj - K[0, 2]) / K[0, 0], (ii - K[1, 2]) / K[1, 1], np.ones((h, w))], -1) @ T[:3, :3].T
    o = T[:3, 3]
    ts = [_slab(o, d, SLAB_LO, SLAB_HI), _slab(o, d, BOX_LO, BOX_HI)]
    for c, rad in SPHERES:
        oc = o - c
        a, b, cc = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - rad ** 2
        disc = b * b - 4 * a * cc
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        ts.append(np.where(t > 0, t, np.inf))
    t = np.min(ts, axis=0)
    return np.round(np.where(np.isfinite(t), t, 0.0) * 1000).astype(np.uint16)


def poses(n=TRACKED + 1):
    return np.stack(tsdf_scene.cameras(24)[:n])          # 15 degrees apart: see DESIGN.md section 2j on what wider baselines cost


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def perturbed(T, dt, axis, angle):
    """The camera moved by dt (metres) and turned about its own centre by `angle` (radians) about `axis` -> float32 [4,4]."""
    P = np.array(T, np.float64)
    P[:3, :3] = rotation(axis, angle) @ P[:3, :3]
    P[:3, 3] += np.asarray(dt, np.float64)
    return P.astype(np.float32)


# name -> (translation in metres, rotation axis, rotation in radians): a few millimetres and a few tenths of a degree, the scale of
# kinematic error; chosen on the CPU so that the restatement converges (tests/test_camtrack_host.py holds that)
TRACKING = {
    "a": ((0.003, -0.002, 0.0025), (1.0, 2.0, -1.0), np.deg2rad(0.3)),
    "b": ((-0.002, 0.003, -0.0015), (-1.0, 0.5, 2.0), np.deg2rad(0.4)),
}


def tracking_frames():
    """-> (depth uint16 [4,H,W], true poses float32 [4,4,4], mask uint8 [H,W] all set)"""
    T = poses()
    return np.stack([raycast(t) for t in T]), T.astype(np.float32), np.ones((H, W), np.uint8)


def tracking_start(name):
    dt, axis, angle = TRACKING[name]
    return perturbed(poses()[TRACKED], dt, axis, angle), float(np.linalg.norm(dt)), float(angle)


def fuse(vol, depths, true_poses, mask, n=N_FUSED):
    """Frames 0 .. n - 1 at their true poses into `vol`: a tests/tsdf_ref.Volume or a physics_utils.TsdfVolume (same call)."""
    for k in range(n):
        vol.integrate(depths[k], mask, INTRINSICS, true_poses[k], 1)
    return vol


def degenerate_field():
    """The exact truncated signed distance of tests/tsdf_scene.py's sphere on a slab, min(sphere, slab) / trunc clamped to +-1, sampled
    on the grid a volume over BOUNDS has, every weight 1 -> (tsdf, weight float32 [nz][ny][nx], lo int [3], voxel, trunc).  Symmetric
    about the sphere's axis, which is the world's z axis."""
    from tests import tsdf_ref
    v = tsdf_ref.Volume(BOUNDS)
    lo = v.b0 * 16
    axes = [((np.arange(int(v.nv[a])) + lo[a]).astype(np.float32) * v.voxel).astype(np.float64) for a in range(3)]
    zz, yy, xx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    P = np.stack([xx, yy, zz], -1)
    sphere = np.linalg.norm(P - tsdf_scene.SPHERE_C, axis=-1) - tsdf_scene.SPHERE_R
    q = np.abs(P - (SLAB_LO + SLAB_HI) / 2) - (SLAB_HI - SLAB_LO) / 2
    slab = np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)
    t = np.clip(np.minimum(sphere, slab) / float(v.trunc), -1, 1).astype(np.float32)
    return t, np.ones_like(t), lo, v.voxel, v.trunc


def degenerate_frames():
    """tests/tsdf_scene.py's sphere on a slab, millimetres rounded -> (depth uint16 [4,H,W], poses float32, mask)"""
    T = np.stack(tsdf_scene.cameras(24)[:TRACKED + 1])
    d = np.stack([np.round(tsdf_scene.raycast(t)[0] * 1000).astype(np.uint16) for t in T])
    return d, T.astype(np.float32), np.ones((H, W), np.uint8)
