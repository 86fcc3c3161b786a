"""Frames for the cloud-building tests (test_pcd_build_gpu.py, test_pcd_build_host.py) and the host rule they are held to: the
functions of pcd_visual_model composed exactly as get_vis_pcds composes them, with the voxel size left open."""
from __future__ import annotations

import functools

import numpy as np

from dream2real_amd import pcd_visual_model as pvm

SORT_TILE = 256          # entries per tile of the radix sort (pcdbuild.hip, PB_THREADS)
SHAPES = ((40, 30), (130, 70), (200, 150))
VOXELS = (0.0, 0.002, 0.02)
VIEWS = (2, 0)           # frame 1 is a decoy no view names; the close view comes first
OBJ_IDS = (1, 0, 2)      # not in label order


def _pose(axis, angle, t):
    """A rigid pose with no zero entry in its rotation, fp64."""
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)
    T[:3, 3] = t
    return T


def label_image(w, h):
    """Three labels: 2 in the top-left block, 1 in the bottom-right block, 0 everywhere else, which touches all four borders.
    Each block is wider and taller than the 15 x 15 window by a few pixels, so every label keeps an eroded core at 40 x 30."""
    m = np.zeros((h, w), np.int64)
    m[:h // 2, :int(0.45 * w)] = 2
    m[h // 2:, int(0.55 * w):] = 1
    return m


@functools.lru_cache(maxsize=None)
def case(w, h):
    """-> dict: rgbs [3] uint8, depths [3] float32 metres, d16 [3,h,w], labels [3,h,w], poses [3,4,4] fp64, K, bounds.
    Frame 0: a steep plane, 0.3 .. 3 m across the columns (voxel indices beyond 255 at 0.002).  Frame 2: a plane at 0.25 m seen
    through a long lens, pixels 0.5 mm apart (far more than 64 points in a 0.02 voxel).  Some depths are 0."""
    rng = np.random.default_rng(w * 1000 + h)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    mm = [300 + 2700.0 * jj / w + 200.0 * ii / h + rng.integers(0, 3, (h, w)),
          rng.integers(250, 2600, (h, w)).astype(np.float64),
          250.0 + rng.integers(0, 2, (h, w))]
    depths = []
    for d in mm:
        d = ((d + 0.25) / 1000.0).astype(np.float32)
        d[rng.random((h, w)) < 0.05] = 0.0
        depths.append(d)
    d16 = np.stack([(d * 1000).astype(np.uint16) for d in depths])
    labels = np.stack([label_image(w, h), rng.integers(0, 3, (h, w)), label_image(w, h)[::-1, ::-1].copy()])
    rgbs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
    poses = np.stack([_pose([1, 2, 3], 0.7, [0.1, -0.2, 0.05]), _pose([3, 1, 1], 2.1, [5, 5, 5]), _pose([-2, 1, 0.5], -0.4, [0.3, 0.1, -0.2])])
    K = np.array([[500.0, 0.0, (w - 1) / 2 + 0.25], [0.0, 497.0, (h - 1) / 2 - 0.125], [0.0, 0.0, 1.0]])
    # the close view looks at the middle of what the steep view sees, so the crop below trims the steep view's ends only
    mid = pvm.backproject(rgbs[0], depths[0], poses[0], K)[0].mean(0)
    poses[2, :3, 3] = mid - poses[2, :3, :3] @ np.array([0.0, 0.0, 0.25])
    # the crop: 3 % off each side of the box around every point the two views see
    pts = np.concatenate([pvm.backproject(rgbs[f], depths[f], poses[f], K)[0] for f in VIEWS])
    lo, hi = pts.min(0), pts.max(0)
    bounds = np.stack([lo + 0.03 * (hi - lo), hi - 0.03 * (hi - lo)])
    return dict(rgbs=rgbs, depths=depths, d16=d16, labels=labels, poses=poses, K=K, bounds=bounds, rgb=np.stack(rgbs))


def host_segments(c, voxel, views=VIEWS, obj_ids=OBJ_IDS, bounds=None):
    """get_vis_pcds' loop with the voxel size as a parameter (0: none) -> per object a list of per-view (xyz fp64, rgb, n_cropped,
    voxel index image or None)."""
    bounds = c["bounds"] if bounds is None else bounds
    out = []
    for obj in obj_ids:
        segs = []
        for v in views:
            depth = c["depths"][v].copy()
            rgb = c["rgbs"][v].copy()
            mask = pvm.erode_rect(c["labels"][v] == obj)
            depth[~mask] = 0
            rgb[~mask] = 0
            xyz, col = pvm.crop(*pvm.backproject(rgb, depth, c["poses"][v], c["K"]), bounds)
            n, idx = xyz.shape[0], None
            if voxel and n:
                idx = np.floor((xyz - (xyz.min(0) - voxel * 0.5)) / voxel).astype(np.int64)
            if voxel:
                xyz, col = pvm.voxel_down_sample(xyz, col, voxel)
            segs.append((xyz, col, n, idx))
        out.append(segs)
    return out


def host_clouds(segments):
    return [(np.concatenate([s[0] for s in segs]).astype(np.float32).reshape(-1, 3), np.concatenate([s[1] for s in segs]).reshape(-1, 3))
            for segs in segments]


@functools.lru_cache(maxsize=None)
def expected(w, h, voxel):
    """-> (clouds [(xyz float32, rgb uint8)] per object of OBJ_IDS, facts): the host rule's result for case(w, h), and what the
    tests assert about it before they trust a comparison."""
    segs = host_segments(case(w, h), voxel)
    facts = dict(points=sum(s[2] for o in segs for s in o),
                 max_index=max((int(s[3].max()) for o in segs for s in o if s[3] is not None), default=0),
                 fullest=max((int(np.unique(s[3], axis=0, return_counts=True)[1].max()) for o in segs for s in o if s[3] is not None), default=0),
                 sizes=[sum(s[0].shape[0] for s in o) for o in segs])
    return host_clouds(segs), facts
