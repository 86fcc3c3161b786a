"""DESIGN.md section 2k restated in numpy: first-frame labels carried through a scan by geometry.  Global Jacobi sweeps (no tiles),
one pass over all voxels per vote, fp32 one operation at a time in the written order.  csrc/labeltrack.hip is held to this by equality
of every byte of the label images, the statistics and the volume."""
from __future__ import annotations

import numpy as np

UNKNOWN = 255
SWEEPS_PER_LAUNCH = 8
DEPTH_MAX = np.float32(3.0)
f32 = np.float32


def grid(bounds, voxel=0.004, band_voxels=2):
    """-> (lo int64 [3], n int64 [3], voxel fp32, band fp32): lo = floor((lo_b - band) / voxel), hi = ceil((hi_b + band) / voxel) in
    fp64 of the fp32 values, n = hi - lo + 1."""
    voxel = f32(voxel)
    band = f32(f32(band_voxels) * voxel)
    b = np.asarray(bounds, np.float64).reshape(2, 3).astype(np.float32).astype(np.float64)
    lo = np.floor((b[0] - np.float64(band)) / np.float64(voxel)).astype(np.int64)
    hi = np.ceil((b[1] + np.float64(band)) / np.float64(voxel)).astype(np.int64)
    return lo, hi - lo + 1, voxel, band


def rigid_inverse(T):
    """csrc/d2r_shared.h's d2r_rigid_inverse: rows 0..2 of [R^T | -R^T t] in fp64, the three products summed left to right -> fp32."""
    T = np.asarray(T, np.float32).reshape(4, 4).astype(np.float64)
    out = np.zeros((3, 4))
    for i in range(3):
        out[i, :3] = T[:3, i]
        out[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    return out.astype(np.float32)


def _z(d16):
    with np.errstate(invalid="ignore"):
        z = d16.astype(np.float32) / f32(1000.0)
    return z, (z > 0) & (z <= DEPTH_MAX)


def predict(vol, lo, n, voxel, d16, pose, K4):
    """-> W_0 uint8 [H,W]: the label of the voxel each valid pixel back-projects to, 255 elsewhere."""
    fx, fy, cx, cy = (f32(k) for k in K4)
    m = np.asarray(pose, np.float32).reshape(4, 4)
    H, W = d16.shape
    z, ok = _z(d16)
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    with np.errstate(all="ignore"):
        xc = ((jj - cx) / fx) * z
        yc = ((ii - cy) / fy) * z
        idx = []
        for a in range(3):
            pw = ((m[a, 0] * xc + m[a, 1] * yc) + m[a, 2] * z) + m[a, 3]
            g = np.floor(pw / voxel + f32(0.5))
            ok = ok & (g >= f32(lo[a])) & (g <= f32(lo[a] + n[a] - 1))                     # the test is made on the floats; NaN fails
            idx.append(np.where(ok, g, f32(lo[a])).astype(np.int64) - lo[a])
    s = vol[idx[2], idx[1], idx[0]]
    known = ok & ((s >> 8) != 0)
    return np.where(known, s & 255, UNKNOWN).astype(np.uint8)


def sweep(Wk, d16, valid, tau_mm):
    """One Jacobi sweep: every read sees Wk."""
    H, W = Wk.shape
    d = d16.astype(np.int64)
    out = Wk.copy()
    best = np.full((H, W), np.iinfo(np.int64).max)
    unknown = Wk == UNKNOWN
    for di, dj in ((-1, 0), (0, -1), (0, 1), (1, 0)):                                       # N, W, E, S
        q_lab = np.full((H, W), UNKNOWN, np.uint8)
        q_d = np.zeros((H, W), np.int64)
        q_valid = np.zeros((H, W), bool)
        dst = (slice(max(0, -di), H - max(0, di)), slice(max(0, -dj), W - max(0, dj)))
        src = (slice(max(0, di), H - max(0, -di)), slice(max(0, dj), W - max(0, -dj)))
        q_lab[dst], q_d[dst], q_valid[dst] = Wk[src], d[src], valid[src]
        diff = np.where(valid, np.abs(d - q_d), 0)
        gives = (q_lab != UNKNOWN) & (~valid | (q_valid & (diff <= tau_mm)))
        take = unknown & gives & (diff < best)                                              # strictly: a tie goes to the earlier neighbour
        out[take] = q_lab[take]
        best[take] = diff[take]
    return out


def fill(W0, d16, tau_mm, grow):
    """-> (W_grow, launches of SWEEPS_PER_LAUNCH sweeps in which a pixel changed)."""
    _, valid = _z(d16)
    Wk, changed_launches = W0, 0
    for start in range(0, grow, SWEEPS_PER_LAUNCH):
        before = Wk
        for _ in range(min(SWEEPS_PER_LAUNCH, grow - start)):
            Wk = sweep(Wk, d16, valid, tau_mm)
        if np.array_equal(Wk, before):
            break                                       # a fixed point: every later sweep is the identity
        changed_launches += 1
    return Wk, changed_launches


def vote(vol, lo, n, voxel, band, d16, pose, K4, Wf):
    """Every voxel once: Boyer-Moore on (label, count).  vol uint16 [nz,ny,nx] is updated in place."""
    fx, fy, cx, cy = (f32(k) for k in K4)
    inv = rigid_inverse(pose)
    H, W = d16.shape
    ax = [(np.arange(n[a], dtype=np.int64) + lo[a]).astype(np.float32) * voxel for a in range(3)]
    pz, py, px = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    cam = [((inv[r, 0] * px + inv[r, 1] * py) + inv[r, 2] * pz) + inv[r, 3] for r in range(3)]
    with np.errstate(all="ignore"):
        ok = cam[2] > 0
        u = np.floor(((fx * cam[0]) / cam[2] + cx) + f32(0.5))
        v = np.floor(((fy * cam[1]) / cam[2] + cy) + f32(0.5))
        ok &= (u >= 0) & (u < f32(W)) & (v >= 0) & (v < f32(H))
        ui, vi = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
        z, valid = _z(d16)
        ok &= valid[vi, ui]
        ok &= np.abs(z[vi, ui] - cam[2]) <= band
    lab_new = Wf[vi, ui].astype(np.uint16)
    ok &= lab_new != UNKNOWN
    lab, cnt = vol & 255, vol >> 8
    empty, same = ok & (cnt == 0), ok & (cnt != 0) & (lab == lab_new)
    other = ok & (cnt != 0) & (lab != lab_new)
    lab = np.where(empty, lab_new, lab)
    cnt = np.where(empty, 1, np.where(same, np.minimum(cnt + 1, 255), np.where(other, cnt - 1, cnt)))
    vol[...] = (lab | (cnt << 8)).astype(np.uint16)


def scan(d16, cam_poses, K4, labels0, bounds, voxel=0.004, band_voxels=2, tau_mm=10, grow=64):
    """-> (labels uint8 [N,H,W], stats uint32 [N,4], vol uint16 [nz,ny,nx], dims [3] (x, y, z), lo [3])."""
    d16 = np.asarray(d16, np.uint16)
    labels0 = np.asarray(labels0, np.uint8)
    assert not (labels0 == UNKNOWN).any()
    N, H, W = d16.shape
    lo, n, voxel, band = grid(bounds, voxel, band_voxels)
    vol = np.zeros((n[2], n[1], n[0]), np.uint16)
    out = np.zeros((N, H, W), np.uint8)
    stats = np.zeros((N, 4), np.uint32)
    for f in range(N):
        if f == 0:
            Wf = labels0
            out[0] = labels0
            stats[0] = (H * W, 0, 0, 0)
        else:
            W0 = predict(vol, lo, n, voxel, d16[f], cam_poses[f], K4)
            Wf, launches = fill(W0, d16[f], tau_mm, grow)
            out[f] = np.where(Wf == UNKNOWN, 0, Wf)
            known0, known = int((W0 != UNKNOWN).sum()), int((Wf != UNKNOWN).sum())
            stats[f] = (known0, known - known0, H * W - known, launches)
        vote(vol, lo, n, voxel, band, d16[f], cam_poses[f], K4, Wf)
    return out, stats, vol, n.astype(np.uint32), lo.astype(np.int32)


def boyer_moore(state, label):
    """One vote on a (label, count) word, as a scalar: for the hand vectors."""
    lab, cnt = state & 255, state >> 8
    if cnt == 0:
        lab, cnt = label, 1
    elif lab == label:
        cnt = min(cnt + 1, 255)
    else:
        cnt -= 1
    return lab | (cnt << 8)
