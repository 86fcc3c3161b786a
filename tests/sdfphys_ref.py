"""numpy restatement of the point-against-field physics rule — the oracle of tests/test_sdfphys_*.py.

The product does not import this module and this module imports nothing from the product.  Every step is fp32 in the written
order (numpy does not contract), fp64 only where the rule says so, so the GPU's bits, points and verdicts can be compared
bit for bit.
  grid      b0 (first block per axis), nv (voxels per axis, x y z), voxel, trunc; voxel g sits at g * voxel, local index g - 16 b0
  field     touch[g] = w[g] >= weight_threshold and tsdf[g] * trunc <= contact; bit x & 31 of word x >> 5, words [nz][ny][ceil(nx / 32)];
            several static grids are ORed
  points    (float)g * voxel of the voxels with w >= weight_threshold and tsdf <= 0, in (z, y, x) order
  pose      T = pose @ inv(init_pose), rows 0..2, fp64 (inv = the rigid inverse [R^T | -R^T t]; each entry summed over l = 0 .. 3 in
            order), rounded once to fp32
  probes    t0 = T[:, 3]; t1 = t0 + unsup_thresh * gravity; t2, t3 = t1 + (+-perturb, 0, 0); t4, t5 = t1 + (0, +-perturb, 0)
  point     c = ((T0 x + T1 y) + T2 z) + tq per row; voxel floor(c / voxel + 0.5) per axis, minus 16 b0; touches when inside the grid
            and its bit is set (outside or not finite: never)
  verdict   orientation mask and valid_so_far as d2r_phys_check; invalid if hit[0]; else valid if pose[2][3] < table_z; else invalid
            unless hit[1]; else, with stability_check, invalid unless hit[2..5] all hold
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
WEIGHT_THRESHOLD = 3.0
CONTACT = 0.002
GRAVITY = (0.0, 0.0, -1.0)


# ------------------------------------------------------------------------------------------------ field and points
def pack_bits(touch):
    """bool [nz, ny, nx] -> uint32 [nz, ny, ceil(nx / 32)]."""
    touch = np.asarray(touch, bool)
    nz, ny, nx = touch.shape
    wpr = (nx + 31) // 32
    pad = np.zeros((nz, ny, wpr * 32), bool)
    pad[:, :, :nx] = touch
    b = pad.reshape(nz, ny, wpr, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)
    return np.bitwise_or.reduce(b, axis=-1).astype(np.uint32)


def unpack_bits(words, nx):
    words = np.asarray(words, np.uint32)
    b = (words[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return b.reshape(words.shape[0], words.shape[1], -1)[:, :, :nx].astype(bool)


def grid_of(vol):
    """(b0 int32 [3], nv uint32 [3], voxel, trunc) of a tsdf_ref.Volume."""
    return np.asarray(vol.b0, np.int32), np.asarray(vol.nv, np.uint32), f32(vol.voxel), f32(vol.trunc)


def touch_words(vol, weight_threshold=WEIGHT_THRESHOLD, contact=CONTACT):
    touch = (vol.w >= f32(weight_threshold)) & (vol.tsdf * f32(vol.trunc) <= f32(contact))
    return pack_bits(touch)


def solid_points(vol, weight_threshold=WEIGHT_THRESHOLD):
    z, y, x = np.nonzero((vol.w >= f32(weight_threshold)) & (vol.tsdf <= f32(0)))         # C order = (z, y, x) order
    g = [x + int(vol.b0[0]) * 16, y + int(vol.b0[1]) * 16, z + int(vol.b0[2]) * 16]
    return np.stack([g[a].astype(np.float32) * f32(vol.voxel) for a in range(3)], 1).astype(np.float32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ per pose
def rigid_inverse(init_pose):
    I = np.asarray(init_pose, np.float32).astype(np.float64).reshape(4, 4)
    out = np.zeros((4, 4))
    for i in range(3):
        for j in range(3):
            out[i, j] = I[j, i]
        out[i, 3] = -((I[0, i] * I[0, 3] + I[1, i] * I[1, 3]) + I[2, i] * I[2, 3])
    out[3, 3] = 1.0
    return out


def transforms(poses, init_pose):
    """-> float32 [N, 3, 4]: rows 0..2 of pose @ inv(init_pose)."""
    M = np.asarray(poses, np.float32).astype(np.float64).reshape(-1, 4, 4)
    inv = rigid_inverse(init_pose)
    T = np.zeros((len(M), 3, 4))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):
            for j in range(4):
                T[:, i, j] = ((M[:, i, 0] * inv[0, j] + M[:, i, 1] * inv[1, j]) + M[:, i, 2] * inv[2, j]) + M[:, i, 3] * inv[3, j]
        return T.astype(np.float32)


def probe_translations(T, unsup_thresh, gravity, perturb):
    """-> float32 [N, 6, 3]."""
    t0 = T[:, :, 3]
    drop = f32(unsup_thresh) * np.asarray(gravity, np.float32)
    p = f32(perturb)
    with np.errstate(invalid="ignore", over="ignore"):
        t1 = t0 + drop
        offs = np.array([[p, 0, 0], [-p, 0, 0], [0, p, 0], [0, -p, 0]], np.float32)
        return np.stack([t0, t1] + [t1 + o for o in offs], 1).astype(np.float32)


def orientation_mask(poses, valid_so_far, oris, disallow_regrasp):
    M = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    mask = np.ones(oris, bool)
    kept = []
    for i in range(oris):
        a = M[i, :3, :3]
        seen = any(bool(np.all(np.abs(a - M[k, :3, :3]) <= f32(0.01) + f32(1e-5) * np.abs(M[k, :3, :3]))) for k in kept)
        if seen:
            mask[i] = False
        else:
            kept.append(i)
    if disallow_regrasp:
        for i in range(oris):
            if not mask[i] or not valid_so_far[i]:
                mask[i] = False
                continue
            if not (M[i, 2, 2] > f32(0.9) or -M[i, 1, 2] > f32(0.9)):
                mask[i] = False
    return mask


def hits(b0, nv, voxel, touch, points, T, tq):
    """touch bool [nz, ny, nx]; points float32 [P, 3]; T float32 [N, 3, 4]; tq float32 [N, 6, 3] -> bool [N, 6]."""
    nx, ny, nz = (int(v) for v in nv)
    lo = [f32(int(b0[a]) * 16) for a in range(3)]
    hi = [f32(int(b0[a]) * 16 + int(nv[a])) for a in range(3)]
    x, y, z = (np.asarray(points, np.float32)[:, a] for a in range(3))
    out = np.zeros((len(T), 6), bool)
    v = f32(voxel)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for n in range(len(T)):
            r = [(T[n, a, 0] * x + T[n, a, 1] * y) + T[n, a, 2] * z for a in range(3)]
            for q in range(6):
                f = [np.floor((r[a] + tq[n, q, a]) / v + f32(0.5)) for a in range(3)]
                inside = np.ones(len(x), bool)
                for a in range(3):
                    inside &= (f[a] >= lo[a]) & (f[a] < hi[a])
                idx = [np.where(inside, f[a], lo[a]).astype(np.int64) - int(b0[a]) * 16 for a in range(3)]
                out[n, q] = bool((inside & touch[idx[2], idx[1], idx[0]]).any())
    return out


def check(b0, nv, voxel, words, points, poses, valid_so_far, sample_res, init_pose, table_z, unsup_thresh=0.02, gravity=GRAVITY,
          perturb=0.04, stability_check=True, disallow_regrasp=False, detail=False):
    """words uint32 [nz, ny, wpr] or [n_grids, nz, ny, wpr] (ORed) -> valid bool [N]; with detail also a dict of the intermediate
    arrays (orientation mask tiled over the positions, hit [N, 6], below_table [N])."""
    words = np.asarray(words, np.uint32)
    if words.ndim == 4:
        words = np.bitwise_or.reduce(words, axis=0)
    touch = unpack_bits(words, int(nv[0]))
    M = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    N = len(M)
    oris = int(sample_res[3]) * int(sample_res[4]) * int(sample_res[5])
    assert N == int(np.prod([int(s) for s in sample_res]))
    valid_in = np.asarray(valid_so_far).astype(bool).reshape(-1)
    omask = np.tile(orientation_mask(M, valid_in, oris, disallow_regrasp), N // oris)
    T = transforms(M, init_pose)
    tq = probe_translations(T, unsup_thresh, gravity, perturb)
    hit = hits(b0, nv, voxel, touch, points, T, tq)
    with np.errstate(invalid="ignore"):
        below = M[:, 2, 3] < f32(table_z)
    ok = ~hit[:, 0]
    ok &= below | hit[:, 1]
    if stability_check:
        ok &= below | hit[:, 2:6].all(1)
    valid = valid_in & omask & ok
    if detail:
        return valid, dict(ori_mask=omask, hit=hit, below=below, T=T, tq=tq)
    return valid
