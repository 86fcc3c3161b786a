"""The synthetic scene the colour-TSDF tests share (tests/test_tsdfvis_host.py, tests/test_tsdfvis_gpu.py): a sphere in front of a
plane, seen by three cameras side by side, with analytic depth.  Small on purpose: 64 x 48 frames, volumes of about 0.1 m, the
background on a 4 mm grid and the sphere on a 3 mm grid (two different grids), truncation four voxels."""
from __future__ import annotations

import functools

import numpy as np

from tests import tsdfvis_ref as ref

W, H = 64, 48
K = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]])
PLANE_Z, SPHERE_C, SPHERE_R = 0.30, np.array([0.0, 0.0, 0.22]), 0.03
BG_BOUNDS = np.array([[-0.07, -0.05, 0.26], [0.07, 0.05, 0.32]])
MV_BOUNDS = np.array([[-0.04, -0.04, 0.18], [0.04, 0.04, 0.26]])
BG_VOXEL, MV_VOXEL = 0.004, 0.003
CAM_X = (-0.012, 0.0, 0.012)
ERODE = 3
THR = 3.0
O_NOW = np.eye(4, dtype=np.float32)
O_NOW[:3, 3] = SPHERE_C


def cam_pose(x):
    T = np.eye(4)
    T[0, 3] = x
    return T


def frame(x, tint=0):
    """The camera at (x, 0, 0) looking along +z -> (depth float32 [H,W] metres, labels uint8 [H,W] (1 the sphere), rgb uint8 [H,W,3])."""
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dx, dy = (jj - K[0, 2]) / K[0, 0], (ii - K[1, 2]) / K[1, 1]
    c = SPHERE_C - np.array([x, 0.0, 0.0])
    a = dx * dx + dy * dy + 1.0
    b = dx * c[0] + dy * c[1] + c[2]
    disc = b * b - a * (c @ c - SPHERE_R ** 2)
    on = disc > 0
    z = np.where(on, (b - np.sqrt(np.where(on, disc, 0.0))) / a, PLANE_Z)
    wx, wy = dx * z + x, dy * z
    rgb = np.zeros((H, W, 3), np.uint8)
    rgb[..., 0] = np.where(on, 200, 40 + 150 * ((np.floor(wx / 0.02) + np.floor(wy / 0.02)) % 2))
    rgb[..., 1] = np.clip(128 + 900 * wx, 0, 255)
    rgb[..., 2] = np.clip(128 + 900 * wy + tint, 0, 255)
    return z.astype(np.float32), on.astype(np.uint8), rgb


@functools.lru_cache(maxsize=None)
def frames():
    return [frame(x) for x in CAM_X]


def fuse(vol, obj, *, tint=0, skip_band=None, n=3):
    """Fuses the three frames' pixels of object `obj` (0 the plane, 1 the sphere) into `vol`: a tsdfvis_ref.ColourVolume or a
    physics_utils.TsdfVolume.  skip_band = (frame, j0, j1): that frame leaves columns j0 .. j1 - 1 out, so their voxels stay below
    three observations."""
    for f, x in enumerate(CAM_X[:n]):
        z, lab, rgb = frame(x, tint)
        mask = lab == obj
        if skip_band is not None and skip_band[0] == f:
            mask = mask.copy()
            mask[:, skip_band[1]:skip_band[2]] = False
        vol.integrate_rgb((z * 1000).astype(np.uint16), mask, rgb, K, cam_pose(x), ERODE)
    return vol


@functools.lru_cache(maxsize=None)
def ref_volumes(kind="plain"):
    """-> (background, movable) restatement volumes.  kind: "plain"; "band": the background misses columns 20 .. 27 in one frame;
    "gap": it misses columns 30 .. 32 in one frame, a thin slab of two observations standing in depth for the oblique camera;
    "twins": the sphere twice, same geometry, the second with other colours; "padded": the movable's bounds padded by four empty
    blocks (of 16 voxels) on every side."""
    if kind == "twins":
        return (fuse(ref.ColourVolume(MV_BOUNDS, MV_VOXEL, 4 * MV_VOXEL), 1), fuse(ref.ColourVolume(MV_BOUNDS, MV_VOXEL, 4 * MV_VOXEL), 1, tint=90))
    return (fuse(ref.ColourVolume(*bg_args()), 0, skip_band=SKIP_BANDS.get(kind)), fuse(ref.ColourVolume(*mv_args(kind)), 1))


SKIP_BANDS = {"band": (1, 20, 28), "gap": (1, 30, 33)}


def bg_args():
    return BG_BOUNDS, BG_VOXEL, 4 * BG_VOXEL


def mv_args(kind="plain"):
    pad = 4 * 16 * MV_VOXEL if kind == "padded" else 0.0
    return MV_BOUNDS + np.array([[-pad], [pad]]), MV_VOXEL, 4 * MV_VOXEL


VIEWS = {"48x40": ref.View(48, 40, 45.0, 45.0, 23.5, 19.5), "45x37": ref.View(45, 37, 45.0, 45.0, 22.0, 18.0)}
CAM = np.eye(4, dtype=np.float32)


def moved(dx=0.0, dy=0.0, dz=0.0, axis=None, angle=0.0):
    """The sphere's pose O moved by (dx, dy, dz) and turned by `angle` about `axis` through its centre."""
    P = O_NOW.astype(np.float64).copy()
    if axis is not None:
        k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        P[:3, :3] = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx
    P[:3, 3] += (dx, dy, dz)
    return P.astype(np.float32)


# name -> candidate pose.  "front": where it was fused, in front of the plane; "behind": behind the plane (shows through the hole
# the sphere's own shadow left in it); "near": a box corner behind the near plane (the whole-frame path); "off": off screen;
# "left" .. "bottom": the rectangle clipped by one frame border; "rot*": turned, rays cross several blocks and leave the box
# through faces, edges and corners.
CANDIDATES = {
    "front": moved(), "behind": moved(dz=0.14), "near": moved(dz=-0.17), "off": moved(dx=5.0),
    "left": moved(dx=-0.10), "right": moved(dx=0.10), "top": moved(dy=-0.08), "bottom": moved(dy=0.08),
    "rot_x": moved(dx=0.03, axis=(1, 0, 0), angle=0.6), "rot_xyz": moved(dy=-0.02, dz=-0.05, axis=(1, 1, 1), angle=2.0),
    "rot_z": moved(dx=-0.05, dz=0.03, axis=(0.2, 0.1, 1), angle=0.785),
}
SMALL_VIEW_CANDIDATES = ("front", "near", "left", "bottom", "rot_xyz")


def poses(names):
    return np.stack([CANDIDATES[n] for n in names]) if len(names) else np.zeros((0, 4, 4), np.float32)


@functools.lru_cache(maxsize=None)
def _rendered(view_name, kind, names, cam):
    bg, mv = ref_volumes("plain" if kind == "padded" else kind)
    out = ref.render(bg, mv, VIEWS[view_name], CAM if cam is None else np.array(cam, np.float32).reshape(4, 4), O_NOW, poses(names), THR)
    for a in out[:2]:
        a.setflags(write=False)
    return out


def expected(view_name, kind="plain", names=tuple(CANDIDATES), cam=None):
    """The restatement's (frames, depth, background) for the named candidates: computed once per (view, volumes, camera) for every
    candidate of the table, shared, never changed."""
    if kind in ("plain", "padded") and cam is None:
        frames, depth, bg = _rendered(view_name, "plain", tuple(CANDIDATES), None)
        idx = [list(CANDIDATES).index(n) for n in names]
        return frames[idx], depth[idx], bg
    return _rendered(view_name, kind, tuple(names), cam)


BEHIND_CAM = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0.6], [0, 0, 0, 1]], np.float32)      # at z = 0.6, looking back along -z


def _look(eye, target):
    """OpenCV camera-to-world pose at `eye` looking at `target`, image-down along world +y."""
    fwd = (np.asarray(target, np.float64) - eye) / np.linalg.norm(np.asarray(target, np.float64) - eye)
    right = np.cross([0.0, 1.0, 0.0], fwd)
    right /= np.linalg.norm(right)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = right, np.cross(fwd, right), fwd, eye
    return T.astype(np.float32)


# 50 degrees off the plane's normal: a ray is in front of the plane left of the "gap" slab, crosses the plane inside it, and comes out
# behind the plane right of it within the truncation distance: observed > 0, unobserved, observed <= 0 along one ray
OBLIQUE_CAM = _look(np.array([-0.26, 0.0, 0.08]), [0.0, 0.0, 0.30])
