"""The scene of tests/test_labeltrack_*.py: tests/camtrack_cases.py's slab with two spheres and a box at 320 x 240, seen from
tests/tsdf_scene.cameras(24), with a ray caster that also says which primitive a pixel shows -- the ground truth a tracked label image
is compared with -- and the small frames of the edge cases.  Everything is computed once per process and handed out read-only."""
from __future__ import annotations

import functools

import numpy as np

from tests import camtrack_cases as cases
from tests import labeltrack_ref as ref
from tests import tsdf_scene

W, H = cases.W, cases.H
K4 = np.array([cases.INTRINSICS[0, 0], cases.INTRINSICS[1, 1], cases.INTRINSICS[0, 2], cases.INTRINSICS[1, 2]], np.float64)     # fx fy cx cy
BOUNDS = cases.BOUNDS
SLAB, BOX, SPHERE_A, SPHERE_B = 0, 1, 2, 3           # the primitive a pixel shows = its true label (the slab is the background)
N_ARC = 8                                            # the first 8 cameras: a 105 degree arc
DEFAULTS = dict(voxel=0.004, band_voxels=2, tau_mm=10, grow=64)


def raycast(T, w=W, h=H, K=cases.INTRINSICS):
    """-> (uint16 [h,w] millimetres exactly as camtrack_cases.raycast gives them, uint8 [h,w] the primitive hit; 0 where nothing is)."""
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    d = np.stack([(jj - K[0, 2]) / K[0, 0], (ii - K[1, 2]) / K[1, 1], np.ones((h, w))], -1) @ T[:3, :3].T
    o = T[:3, 3]
    ts = [cases._slab(o, d, cases.SLAB_LO, cases.SLAB_HI), cases._slab(o, d, cases.BOX_LO, cases.BOX_HI)]
    for c, rad in cases.SPHERES:
        oc = o - c
        a, b, cc = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - rad ** 2
        disc = b * b - 4 * a * cc
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        ts.append(np.where(t > 0, t, np.inf))
    t = np.min(ts, axis=0)
    which = np.where(np.isfinite(t), np.argmin(ts, axis=0), 0).astype(np.uint8)
    return np.round(np.where(np.isfinite(t), t, 0.0) * 1000).astype(np.uint16), which


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def frames(n=24):
    """-> (d16 uint16 [n,H,W], truth uint8 [n,H,W], poses float32 [n,4,4]) of the first n cameras of the orbit, read-only."""
    T = np.stack(tsdf_scene.cameras(24)[:n])
    both = [raycast(t) for t in T]
    return _frozen(np.stack([b[0] for b in both]), np.stack([b[1] for b in both]), T.astype(np.float32))


@functools.lru_cache(maxsize=None)
def reference(n, voxel=0.004, band_voxels=2, tau_mm=10, grow=64):
    """The restatement over the first n frames of the scene, labels0 = frame 0's truth -> (labels, stats, vol, dims, lo), read-only."""
    d16, truth, poses = frames(n)
    return _frozen(*ref.scan(d16, poses, K4, truth[0], BOUNDS, voxel, band_voxels, tau_mm, grow))


def crop(n=3, rows=17, cols=65, i0=96, j0=120):
    """A cols x rows window cut from the scene's first n frames, with the intrinsics of the window: tails in every tiling.  The
    window lies on the box's silhouette in frame 0.  -> (d16, truth, poses, K4)"""
    d16, truth, poses = frames(n)
    k = K4.copy()
    k[2] -= j0
    k[3] -= i0
    return (np.ascontiguousarray(d16[:, i0:i0 + rows, j0:j0 + cols]), np.ascontiguousarray(truth[:, i0:i0 + rows, j0:j0 + cols]),
            poses, k)


def accuracy(labels, truth):
    """-> (share of pixels equal to the truth per frame [N], IoU per object and frame [N,3]: box, sphere a, sphere b; nan where
    neither image holds the object)."""
    acc = (labels == truth).reshape(len(labels), -1).mean(axis=1)
    iou = np.full((len(labels), 3), np.nan)
    for f in range(len(labels)):
        for k, obj in enumerate((BOX, SPHERE_A, SPHERE_B)):
            a, b = labels[f] == obj, truth[f] == obj
            if (a | b).any():
                iou[f, k] = (a & b).sum() / (a | b).sum()
    return acc, iou
