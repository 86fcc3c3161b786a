"""The synthetic RGB-D scene of tests/test_tsdf_*.py: a sphere resting on a slab, ray-cast analytically into fp16 depth
frames from posed pinhole cameras, with a label mask that mislabels a small patch of the slab as the sphere in a few views."""
from __future__ import annotations

import numpy as np

W, H = 320, 240
INTRINSICS = np.array([[380.0, 0.0, 159.5], [0.0, 380.0, 119.5], [0.0, 0.0, 1.0]])
SLAB_LO, SLAB_HI = np.array([-0.3, -0.3, -0.02]), np.array([0.3, 0.3, 0.0])      # wider than every view: a table top, no silhouette in the volume
SPHERE_R = 0.03              # the default sphere; make_scene(sphere_r=...) builds others, always resting on the slab
SPHERE_C = np.array([0.0, 0.0, SPHERE_R])
BOUNDS = np.array([[-0.09, -0.09, -0.03], [0.09, 0.09, 0.08]])
SPECKLE_C, SPECKLE_R, SPECKLE_VIEWS = np.array([0.05, 0.045, 0.0]), 0.010, 5


def look_at(eye, target):
    """Camera-to-world pose in the OpenCV convention (x right, y down, z forward)."""
    z = target - eye
    z = z / np.linalg.norm(z)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T


def cameras(n=12, dist=0.35):
    out = []
    for k in range(n):
        az, el = 2 * np.pi * k / n + 0.1, np.deg2rad(35.0 if k % 2 == 0 else 60.0)
        eye = np.array([0.0, 0.0, 0.02]) + dist * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
        out.append(look_at(eye, np.array([0.0, 0.0, 0.02])))
    return out


def raycast(T, sphere_r=SPHERE_R):
    """-> (depth float64 [H,W] camera z in metres, 0 = nothing hit; label uint8 [H,W] 0 slab / nothing, 1 sphere; hit points)."""
    K = INTRINSICS
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    d_cam = np.stack([(jj - K[0, 2]) / K[0, 0], (ii - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)      # z = 1: ray parameter = depth
    d = d_cam @ T[:3, :3].T
    o = T[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (SLAB_LO - o) / d, (SLAB_HI - o) / d
    tn, tf = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
    t_slab = np.where((tn <= tf) & (tn > 0), tn, np.inf)
    oc = o - np.array([0.0, 0.0, sphere_r])
    a, b, c = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - sphere_r ** 2
    disc = b * b - 4 * a * c
    t_sph = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    t_sph = np.where(t_sph > 0, t_sph, np.inf)
    t = np.minimum(t_slab, t_sph)
    hit = np.isfinite(t)
    depth = np.where(hit, t, 0.0)
    label = (hit & (t_sph < t_slab)).astype(np.uint8)
    pts = o + d * np.where(hit, t, 0.0)[..., None]
    return depth, label, pts


def make_scene(n_views=12, sphere_r=SPHERE_R, speckle_r=SPECKLE_R):
    """-> dict(depths fp16 [n,H,W], masks uint8 [n,H,W], cam_poses float64 [n,4,4], intrinsics, bounds)."""
    poses = cameras(n_views)
    depths, masks = [], []
    for k, T in enumerate(poses):
        depth, label, pts = raycast(T, sphere_r)
        if k < SPECKLE_VIEWS:                              # the mask error: a patch of the slab's top labelled as the sphere
            on_top = (label == 0) & (depth > 0) & (np.abs(pts[..., 2]) < 1e-6)
            label[on_top & (np.linalg.norm(pts[..., :2] - SPECKLE_C[:2], axis=-1) < speckle_r)] = 1
        depths.append(depth.astype(np.float16))
        masks.append(label)
    return dict(depths=np.stack(depths), masks=np.stack(masks), cam_poses=np.stack(poses), intrinsics=INTRINSICS.copy(), bounds=BOUNDS.copy())


def sphere_distance(p):
    return np.abs(np.linalg.norm(np.asarray(p, np.float64) - SPHERE_C, axis=-1) - SPHERE_R)


def slab_distance(p):
    """Distance to the surface of the slab (a box)."""
    p = np.asarray(p, np.float64)
    c, h = (SLAB_LO + SLAB_HI) / 2, (SLAB_HI - SLAB_LO) / 2
    q = np.abs(p - c) - h
    outside = np.linalg.norm(np.maximum(q, 0), axis=-1)
    inside = np.minimum(q.max(-1), 0)
    return np.abs(outside + inside)
