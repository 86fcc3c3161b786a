"""The colour-TSDF visual model restated in numpy: colour fusion on top of tests/tsdf_ref.py's volume, and
the ray caster.  The GPU (tsdf.hip's k_fuse_rgb, tsdfvis.hip) is held to this byte for byte.  Every step is one fp32 operation in
the rule's order; the ray caster evaluates EVERY sample index s = 0 .. S - 1 of every ray (it never skips), vectorised over rays.

Rule, ray caster: pixel (i, j) casts d_c = ((j - cx) / fx, (i - cy) / fy, 1); M [3,4] fp32 takes the camera frame to the volume's
frame (ray_matrix: composed in fp64, rounded once); o = M[:, 3], d_a = (M[a,0] x + M[a,1] y) + M[a,2]; t_s = near + (float)s voxel,
S = ceil((3 - near) / voxel) in fp64 of the fp32 values; p = o + t d; g = p / voxel, cell = floor(g), fraction g - floor(g); a
sample is observed when its cell's eight corners lie in the grid with weight >= thr; its value is the trilinear tsdf (x, then y,
then z, each a + f (b - a)).  Hit: the first s with sample s - 1 observed > 0 and sample s observed <= 0; t_hit = t_{s-1} +
(voxel v0) / (v0 - v1); colour = trilinear colour at p(t_hit) when that cell is observed, else at sample s; floor(c + 0.5)
clamped to 0 .. 255.  Composite: the movable hit wins where t_mov < t_bg; no hit: (0, 0, 0), depth +inf."""
from __future__ import annotations

import numpy as np

from tests import tsdf_ref

f32 = np.float32
BLOCK = tsdf_ref.BLOCK
DEPTH_MAX = 3.0


class ColourVolume(tsdf_ref.Volume):
    """tsdf_ref.Volume plus col float32 [nz][ny][nx][3]: at exactly the voxels a frame updates, c = (w c + rgb[v][u]) / (w + 1)
    with w the weight before the increment and (u, v) the pixel the voxel projected to."""

    def __init__(self, bounds, voxel=0.002, trunc=None):
        super().__init__(bounds, voxel, trunc)
        self.col = np.zeros(self.tsdf.shape + (3,), np.float32)

    def integrate_rgb(self, depth_u16, mask, rgb, intrinsics, cam_pose, erode_k):
        w0 = self.w.copy()
        if not self.integrate(depth_u16, mask, intrinsics, cam_pose, erode_k):
            return False
        iz, iy, ix = np.nonzero(self.w != w0)                      # the voxels whose (tsdf, weight) this frame updated
        K = np.asarray(intrinsics, np.float64).reshape(3, 3).astype(np.float32)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        Mi = tsdf_ref.rigid_inverse34(np.asarray(cam_pose, np.float64).reshape(4, 4).astype(np.float32))
        px = (ix + self.b0[0] * BLOCK).astype(np.float32) * self.voxel
        py = (iy + self.b0[1] * BLOCK).astype(np.float32) * self.voxel
        pz = (iz + self.b0[2] * BLOCK).astype(np.float32) * self.voxel
        xc, yc, zc = (((Mi[r, 0] * px + Mi[r, 1] * py) + Mi[r, 2] * pz) + Mi[r, 3] for r in range(3))
        u = np.floor(((fx * xc) / zc + cx) + f32(0.5)).astype(np.int64)      # section 2c's projection: these voxels passed its tests
        v = np.floor(((fy * yc) / zc + cy) + f32(0.5)).astype(np.int64)
        c = np.asarray(rgb, np.uint8)[v, u].astype(np.float32)
        w = w0[iz, iy, ix][:, None]
        self.col[iz, iy, ix] = (w * self.col[iz, iy, ix] + c) / (w + f32(1))
        return True

    def block_colours(self):
        """-> float32 [n,16,16,16,3] of the active blocks in active_blocks() order, indexed [z][y][x][channel]."""
        bz, by, bx = np.nonzero(self.ever)
        if not len(bz):
            return np.zeros((0, 16, 16, 16, 3), np.float32)
        return np.stack([self.col[z * 16:z * 16 + 16, y * 16:y * 16 + 16, x * 16:x * 16 + 16] for z, y, x in zip(bz, by, bx)])


# ---------------------------------------------------------------------------------------------------- matrices

def _mul4(A, B):
    C = np.zeros((4, 4), np.float64)
    for i in range(4):
        for j in range(4):
            C[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return C


def _rigid_inverse4(T):
    T = np.asarray(T, np.float32).astype(np.float64).reshape(4, 4)
    out = np.zeros((4, 4), np.float64)
    for i in range(3):
        for j in range(3):
            out[i, j] = T[j, i]
        out[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    out[3, 3] = 1.0
    return out


def ray_matrix(cam_pose, obj_pose_now=None, obj_pose=None):
    """-> float32 [3,4]: cam_pose for the background; (O inv(P)) cam_pose for the movable volume at candidate pose P."""
    C = np.asarray(cam_pose, np.float32).astype(np.float64).reshape(4, 4)
    if obj_pose is None:
        return C[:3].astype(np.float32)
    O = np.asarray(obj_pose_now, np.float32).astype(np.float64).reshape(4, 4)
    return _mul4(_mul4(O, _rigid_inverse4(obj_pose)), C)[:3].astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the ray caster

class View:
    def __init__(self, width, height, fx, fy, cx, cy, near=0.01):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy, self.near = f32(fx), f32(fy), f32(cx), f32(cy), f32(near)


def _sample(vol, p, thr):
    """p float32 [n,3] -> (observed bool [n], trilinear tsdf float32 [n], cell (z, y, x) local int64 [n] each, fractions [n,3])."""
    lo = (vol.b0 * BLOCK).astype(np.float64)
    hi = lo + vol.nv
    with np.errstate(all="ignore"):
        g = p / vol.voxel
        c = np.floor(g)
        fr = (g - c).astype(np.float32)
        inside = np.ones(len(p), bool)
        for a in range(3):
            inside &= (c[:, a] >= lo[a]) & (c[:, a] + 1 <= hi[a] - 1)       # both corners along the axis lie in the grid
    q = [np.where(inside, c[:, a], lo[a]).astype(np.int64) - int(lo[a]) for a in range(3)]
    t = [vol.tsdf[q[2] + (k >> 2), q[1] + ((k >> 1) & 1), q[0] + (k & 1)] for k in range(8)]
    ok = inside.copy()
    for k in range(8):
        ok &= vol.w[q[2] + (k >> 2), q[1] + ((k >> 1) & 1), q[0] + (k & 1)] >= f32(thr)
    return ok, _lerp3(t, fr), q, fr


def _lerp3(t, fr):
    f0, f1, f2 = (fr[:, a] if t[0].ndim == 1 else fr[:, a:a + 1] for a in range(3))
    with np.errstate(all="ignore"):
        x00, x10 = t[0] + f0 * (t[1] - t[0]), t[2] + f0 * (t[3] - t[2])
        x01, x11 = t[4] + f0 * (t[5] - t[4]), t[6] + f0 * (t[7] - t[6])
        y0, y1 = x00 + f1 * (x10 - x00), x01 + f1 * (x11 - x01)
        return y0 + f2 * (y1 - y0)


def _colour(vol, q, fr):
    t = [vol.col[q[2] + (k >> 2), q[1] + ((k >> 1) & 1), q[0] + (k & 1)] for k in range(8)]          # [n,3] each
    c = np.floor(_lerp3(t, fr) + f32(0.5))
    return np.clip(c, 0, 255).astype(np.uint8)


def cast(vol, M, view, thr=3.0, carry_gaps=False):
    """One volume under the ray matrices M float32 [m,3,4], every pixel of `view` -> (hit bool [m,H,W], t float32 [m,H,W] (+inf: no
    hit), rgb uint8 [m,H,W,3]).  carry_gaps restates a WRONG rule: an unobserved sample between two observed ones does not break the
    pair (the last observed value is carried across the gap)."""
    M = np.asarray(M, np.float32).reshape(-1, 3, 4)
    m, H, W = M.shape[0], view.height, view.width
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = ((jj.astype(np.float32) - view.cx) / view.fx).reshape(1, -1)
    y = ((ii.astype(np.float32) - view.cy) / view.fy).reshape(1, -1)
    o = np.stack([np.broadcast_to(M[:, a, 3:4], (m, H * W)).reshape(-1) for a in range(3)], 1)
    d = np.stack([((M[:, a, 0:1] * x + M[:, a, 1:2] * y) + M[:, a, 2:3]).reshape(-1) for a in range(3)], 1).astype(np.float32)
    n = m * H * W
    step = vol.voxel
    S = int(max(0.0, np.ceil((DEPTH_MAX - float(view.near)) / float(step))))
    hit = np.zeros(n, bool)
    t_hit = np.full(n, np.inf, np.float32)
    rgb = np.zeros((n, 3), np.uint8)
    prev_ok = np.zeros(n, bool)
    prev_v = np.zeros(n, np.float32)
    for s in range(S):
        t = view.near + f32(s) * step
        with np.errstate(all="ignore"):
            p = o + t * d
        ok, v, q, fr = _sample(vol, p, thr)
        new = ok & prev_ok & (prev_v > 0) & (v <= 0) & ~hit
        if new.any():
            idx = np.nonzero(new)[0]
            tp = view.near + f32(s - 1) * step
            v0, v1 = prev_v[idx], v[idx]
            th = (tp + (step * v0) / (v0 - v1)).astype(np.float32)
            ph = o[idx] + th[:, None] * d[idx]
            okh, _, qh, frh = _sample(vol, ph, thr)
            at_s = _colour(vol, [a[idx] for a in q], fr[idx])
            at_hit = _colour(vol, qh, frh)
            rgb[idx] = np.where(okh[:, None], at_hit, at_s)
            t_hit[idx] = th
            hit |= new
        if carry_gaps:
            prev_ok, prev_v = prev_ok | ok, np.where(ok, v, prev_v).astype(np.float32)
        else:
            prev_ok, prev_v = ok, np.where(ok, v, f32(0)).astype(np.float32)
    return hit.reshape(m, H, W), t_hit.reshape(m, H, W), rgb.reshape(m, H, W, 3)


def render(bg_vol, mv_vol, view, cam_pose, obj_pose_now, obj_poses, thr=3.0):
    """-> (frames uint8 [K,H,W,3], depth float32 [K,H,W], the background's own (hit, t, rgb))."""
    poses = np.asarray(obj_poses, np.float32).reshape(-1, 4, 4)
    bh, bt, bc = cast(bg_vol, ray_matrix(cam_pose)[None], view, thr)
    K = poses.shape[0]
    frames = np.broadcast_to(bc, (K,) + bc.shape[1:]).copy()
    depth = np.broadcast_to(bt, (K,) + bt.shape[1:]).copy()
    if K:
        mh, mt, mc = cast(mv_vol, np.stack([ray_matrix(cam_pose, obj_pose_now, P) for P in poses]), view, thr)
        win = mh & (mt < depth)                                    # a tie goes to the background
        frames[win] = mc[win]
        depth[win] = mt[win]
    return frames, depth, (bh[0], bt[0], bc[0])
