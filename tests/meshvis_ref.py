"""numpy restatement of the mesh-picture rule — the oracle of tests/test_meshvis_*.py.

The product does not import this module.  Every step is integer arithmetic or one IEEE operation in the written order, so the
frames and the ids images are bit-identical to d2r_mesh_render's:
  matrices   inv(cam_pose) item_mat in fp64 (rigid inverse, entries summed over l = 0..3 in order), rounded to fp32; the cubes
             use inv(cam_pose) alone
  vertices   section 2b's fp32 projection (tests/pcd_ref.project_uv); X = rint(16 u), Y = rint(16 v), half to even
  drops      a vertex with z' <= near, a non-finite u or v, |u| or |v| >= 2^17; a doubled area of 0
  coverage   pixel (i, j) sampled at (16 j + 8, 16 i + 8); int64 edge functions of the triangle wound so that A > 0; a centre
             on an edge belongs to it when the edge is a top edge (dy == 0, dx > 0) or a left edge (dy < 0)
  depth      q_k = 1 / (double) z'_k; q = ((w0 q0 + w1 q1) + w2 q2) / A in fp64, rounded to fp32; the maximum key
             (bits(q) << 32) | (0xFFFFFFFF - triangle)
  cubes      12 triangles a cube (CUBE_TRIS over corners c +- h in fp32), a sample counts where its q > the mesh buffer's (0
             where empty); the maximum key (score << 32) | (0xFFFFFFFF - cube); score 0 is skipped
  resolve    (item colour * shade + 127) // 255 with shade = floor(255 (0.35 + 0.65 |n_z| / |n|) + 0.5) in fp64; then
             (under (65535 - s) + viridis5(s) s + 32767) // 65535; background elsewhere
"""
from __future__ import annotations

import numpy as np

from tests import pcd_ref
from tests.pcd_ref import PcdView  # noqa: F401  (the view of a case)

U64 = np.uint64
LOW = U64(0xFFFFFFFF)
INT32_MIN = np.int32(-2 ** 31)
UV_LIMIT = np.float32(131072.0)
LARGE_PX = 1024            # MV_LARGE_PX of meshvis.hip: a clipped box of more pixels goes to the workgroup launch
CUBE_TRIS = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1],
                      [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
VIRIDIS5 = np.array([[68, 1, 84], [59, 82, 139], [33, 145, 140], [94, 201, 98], [253, 231, 37]], np.int64)

# One departure from the rule at a time (tests/test_meshvis_host.py proves the cases can tell them from the rule)
WRONG_RULES = ("ge_all_edges",      # a centre on any edge is covered
               "ties_high",         # equal depths go to the higher triangle index
               "keep_z_eq_near",    # a vertex with z' == near is kept
               "linear_z")          # screen-linear z in place of 1 / z


def item_matrices(cam_pose, item_mats):
    """-> (camera [3,4] fp32, items [n,3,4] fp32)"""
    f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    Ci = pcd_ref.rigid_inverse(f64(cam_pose).reshape(4, 4))
    P = f64(item_mats).reshape(-1, 4, 4)
    M = pcd_ref.mul4(np.broadcast_to(Ci, P.shape), P)
    return Ci[:3].astype(np.float32), M[:, :3].astype(np.float32)


def setup(mats, tri_mat, P, view, wrong=None):
    """mats [n,3,4] fp32, tri_mat [nt] index into them, P [nt,3,3] fp32 world vertices -> dict of per-triangle arrays: X, Y int64
    [nt,3] (wound), q fp64 [nt,3], A int64, keep bool, box (bx0, by0, bx1, by1) clipped, cam fp32 [nt,3,3]"""
    nt = P.shape[0]
    X, Y = np.zeros((nt, 3), np.int64), np.zeros((nt, 3), np.int64)
    q, cam = np.zeros((nt, 3)), np.zeros((nt, 3, 3), np.float32)
    keep = np.ones(nt, bool)
    f = np.float32
    with np.errstate(all="ignore"):
        for k in range(3):
            p = P[:, k]
            M = mats[tri_mat]                                             # [nt,3,4]
            x, y, z = (((M[:, r, 0] * p[:, 0] + M[:, r, 1] * p[:, 1]) + M[:, r, 2] * p[:, 2]) + M[:, r, 3] for r in range(3))
            u = (f(view.fx) * x) / z + f(view.cx)
            v = (f(view.fy) * y) / z + f(view.cy)
            cam[:, k] = np.stack([x, y, z], 1)
            front = z >= f(view.near) if wrong == "keep_z_eq_near" else z > f(view.near)
            ok = front & (np.abs(u) < UV_LIMIT) & (np.abs(v) < UV_LIMIT)
            keep &= ok
            X[:, k] = np.where(ok, np.rint(f(16) * u), 0).astype(np.int64)
            Y[:, k] = np.where(ok, np.rint(f(16) * v), 0).astype(np.int64)
            q[:, k] = np.where(ok, 1.0 / z.astype(np.float64), 0.0)
    A = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    keep &= A != 0
    swap = A < 0
    for a in (X, Y, q):
        a[swap, 1], a[swap, 2] = a[swap, 2].copy(), a[swap, 1].copy()
    A = np.abs(A)
    bx0 = np.maximum((X.min(1) + 7) >> 4, 0)
    bx1 = np.minimum((X.max(1) - 8) >> 4, view.width - 1)
    by0 = np.maximum((Y.min(1) + 7) >> 4, 0)
    by1 = np.minimum((Y.max(1) - 8) >> 4, view.height - 1)
    keep &= (bx1 >= bx0) & (by1 >= by0)
    return dict(X=X, Y=Y, q=q, A=A, keep=keep, box=(bx0, by0, bx1, by1), cam=cam)


def shade_bytes(cam):
    """cam fp32 [nt,3,3] camera-space vertices -> uint8 [nt]"""
    c = cam.astype(np.float64)
    with np.errstate(all="ignore"):
        a, b = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        good = (ln > 0) & (ln < np.inf)
        r = np.where(good, np.abs(nz) / np.where(good, ln, 1.0), 0.0)
        s = 0.35 + 0.65 * r
    return np.floor(s * 255.0 + 0.5).astype(np.uint8)


def _samples(S, idx, ii, jj, wrong):
    """triangles idx [m] sampled at pixels (ii, jj) [m] -> (covered bool [m], q fp32 [m], on_edge bool [m]: the centre lies on an
    edge of the closed triangle)"""
    X, Y, qv, A = S["X"][idx], S["Y"][idx], S["q"][idx], S["A"][idx]
    Px, Py = 16 * jj + 8, 16 * ii + 8
    w, cov, on_edge, closed = [], np.ones(idx.shape[0], bool), np.zeros(idx.shape[0], bool), np.ones(idx.shape[0], bool)
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        dx, dy = X[:, b] - X[:, a], Y[:, b] - Y[:, a]
        E = dx * (Py - Y[:, a]) - dy * (Px - X[:, a])
        owns = (dy < 0) | ((dy == 0) & (dx > 0))
        if wrong == "ge_all_edges":
            owns = np.ones_like(owns)
        cov &= (E > 0) | ((E == 0) & owns)
        on_edge |= E == 0
        closed &= E >= 0
        w.append(E)
    Ad = A.astype(np.float64)
    with np.errstate(all="ignore"):
        if wrong == "linear_z":
            z = ((w[0].astype(np.float64) * (1.0 / qv[:, 0]) + w[1].astype(np.float64) * (1.0 / qv[:, 1])) + w[2].astype(np.float64) * (1.0 / qv[:, 2])) / Ad
            q = (1.0 / z).astype(np.float32)
        else:
            q = (((w[0].astype(np.float64) * qv[:, 0] + w[1].astype(np.float64) * qv[:, 1]) + w[2].astype(np.float64) * qv[:, 2]) / Ad).astype(np.float32)
    return cov, q, on_edge & closed


def _walk(S, view):
    """every (triangle, pixel) pair of the kept triangles' clipped boxes, in chunks -> (idx, ii, jj)"""
    bx0, by0, bx1, by1 = S["box"]
    kept = np.nonzero(S["keep"])[0]
    bw, bh = (bx1 - bx0 + 1)[kept], (by1 - by0 + 1)[kept]
    small = (bw <= 8) & (bh <= 8)
    ks = kept[small]
    for di in range(int(bh[small].max()) if ks.size else 0):
        for dj in range(int(bw[small].max()) if ks.size else 0):
            m = (di < (by1 - by0 + 1)[ks]) & (dj < (bx1 - bx0 + 1)[ks])
            if m.any():
                yield ks[m], by0[ks[m]] + di, bx0[ks[m]] + dj
    for t in kept[~small]:
        ii, jj = np.mgrid[by0[t]:by1[t] + 1, bx0[t]:bx1[t] + 1]
        yield np.full(ii.size, t), ii.ravel(), jj.ravel()


def raster(S, view, low, keys, wrong=None, cube_scores=None, mesh_keys=None, stats=None):
    """keys [H*W] uint64 <- maximum with the triangles' samples (in place).  low [nt]: the low word's owner index per triangle.
    cube_scores given: cube mode against mesh_keys.  stats (optional): (on_edge [H*W], cover [H*W]) += the triangles that have the
    centre on an edge, the triangles that cover it."""
    for idx, ii, jj in _walk(S, view):
        cov, q, on_edge = _samples(S, idx, ii, jj, wrong)
        pix = ii * view.width + jj
        owner = low[idx].astype(U64)
        lo = owner if wrong == "ties_high" and cube_scores is None else LOW - owner
        if cube_scores is None:
            key = (q.view(np.uint32).astype(U64) << U64(32)) | lo
        else:
            mq = (mesh_keys[pix] >> U64(32)).astype(np.uint32).view(np.float32)
            cov &= q > mq
            key = (cube_scores[low[idx]].astype(U64) << U64(32)) | lo
        np.maximum.at(keys, pix[cov], key[cov])
        if stats is not None:
            np.add.at(stats[0], pix[on_edge], 1)
            np.add.at(stats[1], pix[cov], 1)
    return keys


def viridis5(score):
    """int scores 0 .. 65535 [n] -> int64 [n,3]"""
    t = np.asarray(score, np.int64) * 4
    seg = np.minimum(t // 65535, 3)
    f = (t - seg * 65535)[:, None]
    return (VIRIDIS5[seg] * (65535 - f) + VIRIDIS5[seg + 1] * f + 32767) // 65535


def cube_triangles(centres, half):
    """-> fp32 [K*12,3,3]"""
    c = np.asarray(centres, np.float32).reshape(-1, 3)
    h = np.asarray(half, np.float32).reshape(-1)
    corners = np.stack([np.stack([np.where(b >> a & 1, c[:, a] + h, c[:, a] - h) for a in range(3)], 1) for b in range(8)], 1)   # [K,8,3]
    return corners[:, CUBE_TRIS].reshape(-1, 3, 3).astype(np.float32)


def render(view, cam_pose, verts, tris, tri_item, item_mats, item_rgb, cube_centres=None, cube_half=None, cube_scores=None,
           background=(255, 255, 255), wrong=None, details=False):
    """-> (rgb uint8 [H,W,3], ids int32 [H,W]): what d2r_mesh_render must return, bit for bit (with `wrong`: one of WRONG_RULES in
    its place).  details: also a dict with the mesh set-up, the shade bytes, the key buffers and, per pixel, how many mesh triangles have
    the centre on an edge and how many cover it."""
    assert wrong is None or wrong in WRONG_RULES, wrong
    H, W = view.height, view.width
    verts = np.asarray(verts if verts is not None else [], np.float32).reshape(-1, 3)
    tris = np.asarray(tris if tris is not None else [], np.int64).reshape(-1, 3)
    tri_item = np.asarray(tri_item if tri_item is not None else [], np.int64).reshape(-1)
    item_rgb = np.asarray(item_rgb if item_rgb is not None else [], np.int64).reshape(-1, 3)
    Mc, Mi = item_matrices(cam_pose, item_mats if item_mats is not None and len(item_mats) else np.zeros((0, 4, 4)))
    mesh_keys, cube_keys = np.zeros(H * W, U64), np.zeros(H * W, U64)
    stats = (np.zeros(H * W, np.int64), np.zeros(H * W, np.int64))
    S, shade = None, np.zeros(0, np.uint8)
    nt = tris.shape[0]
    if nt:
        S = setup(Mi, tri_item, verts[tris], view, wrong)
        shade = shade_bytes(S["cam"])
        raster(S, view, np.arange(nt), mesh_keys, wrong, stats=stats)
    SC = None
    K = 0 if cube_scores is None else len(cube_scores)
    if K:
        scores = np.asarray(cube_scores, np.int64).reshape(-1)
        SC = setup(Mc[None], np.zeros(K * 12, np.int64), cube_triangles(cube_centres, cube_half), view, wrong)
        SC["keep"] &= np.repeat(scores != 0, 12)
        raster(SC, view, np.repeat(np.arange(K), 12), cube_keys, wrong, cube_scores=scores, mesh_keys=mesh_keys)
    rgb = np.empty((H * W, 3), np.int64)
    rgb[:] = np.asarray(background, np.int64).reshape(3)
    ids = np.full(H * W, INT32_MIN, np.int32)
    hit = mesh_keys != 0
    t = (mesh_keys[hit] & LOW).astype(np.int64)
    t = t if wrong == "ties_high" else 0xFFFFFFFF - t
    rgb[hit] = (item_rgb[tri_item[t]] * shade[t].astype(np.int64)[:, None] + 127) // 255
    ids[hit] = t
    chit = cube_keys != 0
    s = (cube_keys[chit] >> U64(32)).astype(np.int64)
    rgb[chit] = (rgb[chit] * (65535 - s)[:, None] + viridis5(s) * s[:, None] + 32767) // 65535
    ids[chit] = -1 - (0xFFFFFFFF - (cube_keys[chit] & LOW).astype(np.int64))
    out = rgb.astype(np.uint8).reshape(H, W, 3), ids.reshape(H, W)
    if details:
        return out + (dict(mesh=S, cubes=SC, shade=shade, mesh_keys=mesh_keys, cube_keys=cube_keys, on_edge=stats[0].reshape(H, W), cover=stats[1].reshape(H, W)),)
    return out
