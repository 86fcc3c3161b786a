"""numpy restatement of the camera-pose refinement -- the oracle of tests/test_camtrack_*.py.

The product does not import this module and this module imports nothing from the product.  How a point meets the volume (cell,
fractions, the trilinear value and its gradient) is tests/tsdf_ref.py's cell and lerp3_grad, which tests/tsdfvis_ref.py builds on
too.  The linearisation is fp32, one IEEE operation at a time in the rule's order (numpy does not contract); each of the 29 sums
adds rint(fp64(a) * fp64(b) * 2^29) as integers, so the GPU's sums can be compared by integer equality.  The step (LDL^T, exp, the pose update) is Python floats (fp64) in
csrc/camtrack_solve.h's order, with math.sin / math.sqrt (the C library's, as the host code uses).

  pixel      (u, v) with u % stride == 0, v % stride == 0, mask set, 0 < z = u16 / 1000 <= 3
  point      p_c = (((u - cx) / fx) z, ((v - cy) / fy) z, z);  p_w[a] = ((m_a0 x + m_a1 y) + m_a2 z) + m_a3
  cell       g = p_w / voxel, c = floor(g), f = g - c; observed: c and c + 1 in the grid on every axis, eight weights >= thr
  value      e_yz = t(1,y,z) - t(0,y,z);  x_yz = t(0,y,z) + f0 e_yz;  d_z = x_1z - x_0z;  y_z = x_0z + f1 d_z;  gz = y_1 - y_0;
             phi = y_0 + f2 gz;  gy = d_0 + f2 (d_1 - d_0);  ey_z = e_0z + f1 (e_1z - e_0z);  gx = ey_0 + f2 (ey_1 - ey_0)
  row        r = phi trunc;  n_a = (g_a trunc) / voxel;  J = [n, p_w x n], (p x n)_0 = p1 n2 - p2 n1 and cyclic
  gates      |phi| < 1, |r| <= 1, |n_a| <= 4, |p_w a| <= 8
  sums       21: J_i J_j (i <= j, row by row); 6: J_i r; r r; the count
"""
from __future__ import annotations

import math

import numpy as np

from tests import tsdf_ref

f32 = np.float32
SUMS = 29
SCALE_LOG2 = 29
SCALE = float(2 ** SCALE_LOG2)
DEPTH_MAX = f32(3.0)
N_MAX, P_MAX, R_MAX = f32(4.0), f32(8.0), f32(1.0)
PIVOT_REL = 1e-6
CONVERGED = 1e-5
STATUS = ("converged", "max_iters", "degenerate", "too_few")


class Grid:
    """A dense volume: tsdf, w float32 [nz][ny][nx]; lo int [3] (x, y, z) the global coordinate of voxel 0; voxel, trunc float32."""

    def __init__(self, tsdf, w, lo, voxel, trunc):
        self.tsdf, self.w = np.asarray(tsdf, np.float32), np.asarray(w, np.float32)
        self.lo = np.asarray(lo, np.int64)
        self.nv = np.array(self.tsdf.shape[::-1], np.int64)
        self.voxel, self.trunc = f32(voxel), f32(trunc)


def grid_from_blocks(coords, tsdf, weight, b0, nv, voxel, trunc):
    """d2r_tsdf_read_voxels' blocks + d2r_tsdf_grid -> Grid (untouched blocks are zeros, as on the device)."""
    nx, ny, nz = (int(v) for v in nv)
    T, W = np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32)
    for (bx, by, bz), t, w in zip(np.asarray(coords, np.int64) - np.asarray(b0, np.int64), tsdf, weight):
        T[bz * 16:bz * 16 + 16, by * 16:by * 16 + 16, bx * 16:bx * 16 + 16] = t
        W[bz * 16:bz * 16 + 16, by * 16:by * 16 + 16, bx * 16:bx * 16 + 16] = w
    return Grid(T, W, np.asarray(b0, np.int64) * 16, voxel, trunc)


def grid_from_volume(vol):
    """tests/tsdf_ref.Volume -> Grid"""
    return Grid(vol.tsdf, vol.w, vol.b0 * 16, vol.voxel, vol.trunc)


def rows(grid, depth_u16, mask, intrinsics, pose, thr=1.0, stride=1, facts=None, full=False):
    """-> (J float32 [n,6], r float32 [n]) of the contributing pixels, in (v, u) order.  facts: a dict that gains counts of what the
    pixels met (selected, valid, in_grid, observed, phi_pm1, gated, frac0, negative, last_cell per axis, outside per axis)."""
    K = np.asarray(intrinsics, np.float64).reshape(3, 3).astype(np.float32)
    M = np.asarray(pose, np.float32).reshape(4, 4)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    d = np.asarray(depth_u16, np.uint16)
    m = np.asarray(mask)
    h, w = d.shape
    vv, uu = np.meshgrid(np.arange(0, h, stride), np.arange(0, w, stride), indexing="ij")
    vv, uu = vv.reshape(-1), uu.reshape(-1)
    z = d[vv, uu].astype(np.float32) / f32(1000)
    ok = (m[vv, uu] != 0) & (z > 0) & (z <= DEPTH_MAX)
    valid = ok.copy()
    xc = ((uu.astype(np.float32) - cx) / fx) * z
    yc = ((vv.astype(np.float32) - cy) / fy) * z
    with np.errstate(all="ignore"):
        p = np.stack([((M[a, 0] * xc + M[a, 1] * yc) + M[a, 2] * z) + M[a, 3] for a in range(3)], 1).astype(np.float32)
    last = grid.lo + grid.nv - 2                                     # c and c + 1 lie in the grid on every axis
    inside, c, f = tsdf_ref.cell(p, grid.voxel, grid.lo, last)
    if facts is not None:
        for a in range(3):
            facts.setdefault("outside", np.zeros(3, np.int64))[a] += int((valid & ~inside[:, a]).sum())
            facts.setdefault("last_cell", np.zeros(3, np.int64))[a] += int((valid & (c[:, a] == f32(last[a]))).sum())
            facts.setdefault("frac0", np.zeros(3, np.int64))[a] += int((valid & inside[:, a] & (f[:, a] == 0)).sum())
            facts.setdefault("negative", np.zeros(3, np.int64))[a] += int((valid & inside[:, a] & (c[:, a] < 0)).sum())
    ok &= inside.all(axis=1) & (np.abs(p) <= P_MAX).all(axis=1)
    in_grid = ok.copy()
    q = [np.where(ok, c[:, a], f32(grid.lo[a])).astype(np.int64) - int(grid.lo[a]) for a in range(3)]
    t = [grid.tsdf[q[2] + (k >> 2), q[1] + ((k >> 1) & 1), q[0] + (k & 1)] for k in range(8)]
    for k in range(8):
        ok &= grid.w[q[2] + (k >> 2), q[1] + ((k >> 1) & 1), q[0] + (k & 1)] >= f32(thr)
    observed = ok.copy()
    phi, (gx, gy, gz) = tsdf_ref.lerp3_grad(t, f)
    p = [p[:, a] for a in range(3)]
    with np.errstate(all="ignore"):
        r = phi * grid.trunc
        n = [(ga * grid.trunc) / grid.voxel for ga in (gx, gy, gz)]
        ok &= np.abs(phi) < f32(1)
        keep = ok & (np.abs(r) <= R_MAX) & (np.abs(n[0]) <= N_MAX) & (np.abs(n[1]) <= N_MAX) & (np.abs(n[2]) <= N_MAX)
        J = [n[0], n[1], n[2], p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0]]
    if facts is not None:
        for key, val in (("selected", len(z)), ("valid", valid.sum()), ("in_grid", in_grid.sum()), ("observed", observed.sum()),
                         ("phi_pm1", (observed & (np.abs(phi) == f32(1))).sum()), ("gated", (ok & ~keep).sum()), ("contributing", keep.sum())):
            facts[key] = facts.get(key, 0) + int(val)
    if full:           # every selected pixel: (contributes bool [n], J [n,6], r [n], fractions [n,3]); rows that do not contribute hold garbage
        return keep, np.stack(J, 1).astype(np.float32), r.astype(np.float32), f
    return np.stack([j[keep] for j in J], 1).astype(np.float32), r[keep].astype(np.float32)


def _term(a, b):
    return int(np.rint((a.astype(np.float64) * b.astype(np.float64)) * SCALE).astype(np.int64).sum(dtype=np.int64))


def sums_of(J, r):
    out = [_term(J[:, i], J[:, j]) for i in range(6) for j in range(i, 6)]
    out += [_term(J[:, i], r) for i in range(6)]
    return out + [_term(r, r), int(len(r))]


def system(grid, depth_u16, mask, intrinsics, pose, thr=1.0, stride=1, facts=None):
    """-> the 29 sums as Python integers."""
    return sums_of(*rows(grid, depth_u16, mask, intrinsics, pose, thr, stride, facts))


# ---------------------------------------------------------------------------------------------------- the step (fp64)

def solve(sums, pivots=None):
    """-> xi = -A^-1 b (list of 6 floats), or None: degenerate.  csrc/camtrack_solve.h's ct_solve line by line.  pivots: a list
    that gains (d_j, PIVOT_REL * max diag) per pivot reached."""
    A = [[0.0] * 6 for _ in range(6)]
    q = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = float(sums[q]) / SCALE
            q += 1
    b = [float(sums[21 + i]) / SCALE for i in range(6)]
    dmax = 0.0
    for i in range(6):
        dmax = max(dmax, A[i][i])
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s -= (L[j][k] * L[j][k]) * d[k]
        if pivots is not None:
            pivots.append((s, PIVOT_REL * dmax))
        if not s > PIVOT_REL * dmax:
            return None
        d[j] = s
        for i in range(j + 1, 6):
            t = A[i][j]
            for k in range(j):
                t -= (L[i][k] * L[j][k]) * d[k]
            L[i][j] = t / s
    y = [0.0] * 6
    for i in range(6):
        t = -b[i]
        for k in range(i):
            t -= L[i][k] * y[k]
        y[i] = t
    for i in range(6):
        y[i] = y[i] / d[i]
    xi = [0.0] * 6
    for i in range(5, -1, -1):
        t = y[i]
        for k in range(i + 1, 6):
            t -= L[k][i] * xi[k]
        xi[i] = t
    return xi


def exp_twist(xi):
    """-> E [3][4] (lists of floats) = rows 0..2 of exp(xi^): ct_exp line by line."""
    wx, wy, wz = xi[3], xi[4], xi[5]
    th2 = (wx * wx + wy * wy) + wz * wz
    th = math.sqrt(th2)
    if th < 1e-4:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        s, h = math.sin(th), math.sin(0.5 * th)
        a, b, c = s / th, (2.0 * (h * h)) / th2, (th - s) / (th2 * th)
    W = [[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]]
    W2 = [[(W[i][0] * W[0][j] + W[i][1] * W[1][j]) + W[i][2] * W[2][j] for j in range(3)] for i in range(3)]
    E = []
    for i in range(3):
        V = []
        row = []
        for j in range(3):
            one = 1.0 if i == j else 0.0
            row.append((one + a * W[i][j]) + b * W2[i][j])
            V.append((one + b * W[i][j]) + c * W2[i][j])
        row.append((V[0] * xi[0] + V[1] * xi[1]) + V[2] * xi[2])
        E.append(row)
    return E


def apply(E, T):
    """T <- exp(xi^) T on rows 0..2 ([3][4] lists): ct_apply line by line."""
    out = [[(E[i][0] * T[0][j] + E[i][1] * T[1][j]) + E[i][2] * T[2][j] for j in range(4)] for i in range(3)]
    for i in range(3):
        out[i][3] += E[i][3]
    return out


def rms(sums):
    return math.sqrt((float(sums[27]) / SCALE) / float(sums[28])) if sums[28] > 0 else 0.0


def _round(T):
    return np.array(T + [[0.0, 0.0, 0.0, 1.0]], np.float64).astype(np.float32)


def step(pose32, sums):
    """One iteration from the fp32 pose a linearisation used and its sums -> the next fp32 pose [4,4], or None: degenerate.  (The
    loop carries fp64 across iterations; from the rounded pose the result can differ from the loop's by one rounding.)"""
    xi = solve(sums)
    if xi is None:
        return None
    T = [[float(x) for x in row] for row in np.asarray(pose32, np.float32).reshape(4, 4)[:3]]
    return _round(apply(exp_twist(xi), T))


def refine(grid, depth_u16, mask, intrinsics, pose, thr=1.0, stride=1, max_iters=20, min_pixels=500):
    """The loop -> (pose float32 [4,4], report dict: status, iters, pixels_first / _last, rms_first / _last, poses [iters,4,4], sums
    (list of lists of Python integers))."""
    pose_in = np.asarray(pose, np.float32).reshape(4, 4)
    T = [[float(x) for x in row] for row in pose_in[:3]]
    rep = dict(status="max_iters", iters=0, poses=[], sums=[])
    keep_input = False
    for it in range(max_iters):
        P = _round(T)
        s = system(grid, depth_u16, mask, intrinsics, P, thr, stride)
        rep["poses"].append(P)
        rep["sums"].append(s)
        rep["iters"] = it + 1
        rep["pixels_last"], rep["rms_last"] = s[28], rms(s)
        if it == 0:
            rep["pixels_first"], rep["rms_first"] = s[28], rms(s)
        if s[28] < min_pixels:
            rep["status"], keep_input = "too_few", True
            break
        xi = solve(s)
        if xi is None:
            rep["status"] = "degenerate"
            break
        T = apply(exp_twist(xi), T)
        nv = math.sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2])
        nw = math.sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5])
        rep["last_step"] = (nv, nw)
        if nv < CONVERGED and nw < CONVERGED:
            rep["status"] = "converged"
            break
    rep["poses"] = np.stack(rep["poses"])
    return (pose_in.copy() if keep_input else _round(T)), rep


def pose_error(T, T_true):
    """-> (translation error in metres, rotation error in radians)"""
    A, B = np.asarray(T, np.float64).reshape(4, 4), np.asarray(T_true, np.float64).reshape(4, 4)
    R = A[:3, :3] @ B[:3, :3].T
    sk = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])           # sin(angle) axis: exact for small angles
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3])), float(math.atan2(np.linalg.norm(sk), (np.trace(R) - 1.0) / 2.0))
