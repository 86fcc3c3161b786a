"""numpy restatement of the point-cloud render rule — the oracle of tests/test_pcd_*.py.

The product does not import this module.  Every step follows the written order so that frames are bit-identical:
  matrices   inv(cam_pose) P_k inv(O) in fp64 (rigid inverses [R^T | -R^T t], entries summed over l = 0..3 in order),
             rounded to fp32; the background uses inv(cam_pose) alone
  points     x' = ((m0 x + m1 y) + m2 z) + m3 per row in fp32, culled when z' <= near;
             u = (fx x') / z' + cx, v = (fy y') / z' + cy (fp32, correctly rounded divide)
  sprite     columns ceil(u - ps / 2) .. + ps - 1, rows likewise, clipped to the frame
  visibility the minimum key (float_bits(z') << 32) | global index (background first, then the movable cloud)
  colour     the winner's rgb; white where no point lands; all three channels > 220 -> (0, 0, 0)
"""
from __future__ import annotations

import dataclasses

import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


@dataclasses.dataclass
class PcdView:
    width: int = 336
    height: int = 336
    fx: float = 436.01158022
    fy: float = 435.90814372
    cx: float = 168.0
    cy: float = 168.0
    point_size: float = 3.0
    near: float = 0.01


def rigid_inverse(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    out = np.zeros((4, 4))
    for i in range(3):
        for j in range(3):
            out[i, j] = T[j, i]
        out[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    out[3, 3] = 1.0
    return out


def mul4(A, B):
    """[..., 4, 4] @ [..., 4, 4] with each entry summed over l = 0..3 in order (no BLAS reordering)."""
    return ((A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :])
            + A[..., :, 2, None] * B[..., None, 2, :]) + A[..., :, 3, None] * B[..., None, 3, :]


def matrices(cam_pose, obj_pose_now, obj_poses):
    """-> (background [3,4] fp32, candidates [K,3,4] fp32).  Poses arrive as fp32 (the ABI's type)."""
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    Ci = rigid_inverse(f32(cam_pose).reshape(4, 4))
    Oi = rigid_inverse(f32(obj_pose_now).reshape(4, 4))
    P = f32(obj_poses).reshape(-1, 4, 4)
    M = mul4(mul4(np.broadcast_to(Ci, P.shape), P), np.broadcast_to(Oi, P.shape))
    return Ci[:3].astype(np.float32), M[:, :3].astype(np.float32)


# One departure from the rule at a time, for tests that prove their cases can tell the rule from its near misses
# (tests/test_pcd_edges_host.py).  `wrong=None`, the default everywhere, is the rule.
WRONG_RULES = (
    "floor_plus_one",     # sprite starts at floor(u - ps / 2) + 1 instead of ceil(u - ps / 2)
    "keep_z_eq_near",     # a point with z' == near is kept
    "ties_high",          # equal depths go to the higher global index
    "z24",                # keys compare z' truncated to the upper 24 bits of its pattern
    "ge_220",             # all three channels >= 220 -> black
    "white_stays",        # a pixel no point reaches stays white
    "cull_ge_minus_ps",   # kept when a >= -ps (and b >= -ps)
    "cull_le_size",       # kept when a <= W (and b <= H)
)


def project_uv(M, xyz, view: PcdView):
    """-> (u, v, z) fp32 [N]: the image coordinates and the camera-space depth before any cull (inf / NaN where they overflow)."""
    M = np.asarray(M, np.float32)
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x, y, z = (((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3] for r in range(3))
        f = np.float32
        u = (f(view.fx) * x) / z + f(view.cx)
        v = (f(view.fy) * y) / z + f(view.cy)
    return u, v, z


def project(M, xyz, view: PcdView, wrong=None):
    """-> (z fp32 [N], j0 int64 [N], i0 int64 [N], ok bool [N])."""
    u, v, z = project_uv(M, xyz, view)
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        half = f(view.point_size) * f(0.5)
        if wrong == "floor_plus_one":
            a, b = np.floor(u - half) + f(1), np.floor(v - half) + f(1)
        else:
            a, b = np.ceil(u - half), np.ceil(v - half)
        ps = f(view.point_size)
        W, H = f(view.width), f(view.height)
        front = z >= f(view.near) if wrong == "keep_z_eq_near" else z > f(view.near)
        lo = (a >= -ps) & (b >= -ps) if wrong == "cull_ge_minus_ps" else (a > -ps) & (b > -ps)
        hi = (a <= W) & (b <= H) if wrong == "cull_le_size" else (a < W) & (b < H)
        ok = front & lo & hi
    j0 = np.where(ok, a, 0).astype(np.int64)
    i0 = np.where(ok, b, 0).astype(np.int64)
    return z, j0, i0, ok


def splat(keys, M, xyz, first_index, view: PcdView, wrong=None):
    """keys [H*W] uint64 <- minimum with the cloud's sprites (in place)."""
    z, j0, i0, ok = project(M, xyz, view, wrong)
    idx = np.nonzero(ok)[0]
    zbits = z[idx].view(np.uint32).astype(np.uint64)
    if wrong == "z24":
        zbits &= np.uint64(0xFFFFFF00)
    low = (idx + first_index).astype(np.uint64)
    if wrong == "ties_high":
        low = np.uint64(0xFFFFFFFF) - low            # resolve() undoes it
    key = (zbits << np.uint64(32)) | low
    ps = int(view.point_size)
    for dr in range(ps):
        for dc in range(ps):
            r, c = i0[idx] + dr, j0[idx] + dc
            m = (r >= 0) & (r < view.height) & (c >= 0) & (c < view.width)
            np.minimum.at(keys, r[m] * view.width + c[m], key[m])
    return keys


def resolve(keys, colours, view: PcdView, wrong=None):
    """keys [H*W] -> uint8 [H,W,3] through the colour table (background then movable)."""
    out = np.full((keys.shape[0], 3), 255, np.uint8)
    hit = keys != EMPTY
    low = keys[hit] & np.uint64(0xFFFFFFFF)
    if wrong == "ties_high":
        low = np.uint64(0xFFFFFFFF) - low
    out[hit] = colours[low.astype(np.int64)]
    black = np.all(out >= 220, axis=-1) if wrong == "ge_220" else np.all(out > 220, axis=-1)
    if wrong == "white_stays":
        black &= hit
    out[black] = 0
    return out.reshape(view.height, view.width, 3)


def render(bg_xyz, bg_rgb, mv_xyz, mv_rgb, view: PcdView, cam_pose, obj_pose_now, obj_poses, wrong=None):
    """-> uint8 [K,H,W,3]: what d2r_pcd_render must return, bit for bit (with `wrong`: one of WRONG_RULES in its place)."""
    assert wrong is None or wrong in WRONG_RULES, wrong
    Mb, Mk = matrices(cam_pose, obj_pose_now, obj_poses)
    nb = np.asarray(bg_xyz).reshape(-1, 3).shape[0]
    colours = np.concatenate([np.asarray(bg_rgb, np.uint8).reshape(-1, 3), np.asarray(mv_rgb, np.uint8).reshape(-1, 3)], 0)
    bg_keys = splat(np.full(view.width * view.height, EMPTY, np.uint64), Mb, bg_xyz, 0, view, wrong)
    return np.stack([resolve(splat(bg_keys.copy(), M, mv_xyz, nb, view, wrong), colours, view, wrong) for M in Mk]) if len(Mk) else \
        np.zeros((0, view.height, view.width, 3), np.uint8)
