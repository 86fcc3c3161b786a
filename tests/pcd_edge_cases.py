"""Seeded scenes for the point-cloud renderer's edges (test_pcd_edges_host.py, test_pcd_edges_gpu.py): sprite sizes and rounding
edges, the LDS tile grid of k_pcd_candidates, depth edges, empty inputs and the colour threshold.

Every builder returns (bg_xyz, bg_rgb, mv_xyz, mv_rgb, PcdView, cam_pose, obj_pose_now, obj_poses, what); `what` is a dict that says
what the case is meant to reach, in terms the host test checks from tests/pcd_ref.py alone.  `args(case)` is the first eight, the
arguments of pcd_ref.render.

The lattice scenes use an identity camera and object pose, power-of-two fx and fy and coordinates with few mantissa bits, so that
u = (fx x) / z + cx is exact in fp32 and the side of a rounding edge a point sits on can be read off its construction; `lattice`
asserts that exactness."""
from __future__ import annotations

import functools

import numpy as np

from tests import pcd_ref
from tests.pcd_ref import PcdView

TILE_PX = 4096           # PCD_TILE_PX in pcd.hip: LDS keys per tile
F32 = np.float32
EYE34 = np.eye(4, dtype=np.float32)[:3]


def args(case):
    return case[:8]


def up(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


def down(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


def shift(x=0.0, y=0.0, z=0.0):
    P = np.eye(4, dtype=np.float32)
    P[:3, 3] = [x, y, z]
    return P


def px_shift(view, du, dv):
    """The pose that moves a point at depth 1 by (du, dv) pixels under an identity camera."""
    return shift(du / view.fx, dv / view.fy)


def pose(axis, angle, t):
    """A rigid pose with no zero entry in its rotation, fp32."""
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)
    T[:3, 3] = t
    return T.astype(np.float32)


def look_at(eye, target):
    """OpenCV camera-to-world pose: x right, y down, z forward."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.1, 0.05, 1.0])                      # a slightly rolled camera: no zero entry in its rotation
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T.astype(np.float32)


def lattice(view, u, v, z=1.0):
    """World points that an identity camera sees at exactly (u, v) in fp32, at depth z.  u and v are fp32 values held in float64."""
    u, v = np.atleast_1d(np.asarray(u, np.float64)), np.atleast_1d(np.asarray(v, np.float64))
    z = np.broadcast_to(np.asarray(z, np.float64), u.shape)
    p = np.stack([(u - view.cx) * z / view.fx, (v - view.cy) * z / view.fy, z], 1)
    p32 = p.astype(np.float32)
    assert (p32 == p).all(), "a lattice coordinate is not an fp32 number"
    uu, vv, zz = pcd_ref.project_uv(EYE34, p32, view)
    assert (uu.astype(np.float64) == u).all() and (vv.astype(np.float64) == v).all() and (zz == z).all(), "the lattice is not exact"
    return p32


def at(view, a, b, z=1.0):
    """World points whose sprites start at column a, row b: u - half = a - 0.25, a quarter pixel inside the rounding interval, so the
    fp32 rounding of x and u (about 1e-3 pixel at column 8000) cannot move it."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    z = np.broadcast_to(np.asarray(z, np.float64), a.shape)
    half = view.point_size * 0.5
    return np.stack([(a - 0.25 + half - view.cx) * z / view.fx, (b - 0.25 + half - view.cy) * z / view.fy, z], 1).astype(np.float32)


def _rgb(rng, n, lo=0, hi=200):
    return rng.integers(lo, hi, (n, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- A: sprites

SPRITE_SIZES = (1, 2, 4, 5, 16)


def sprite_view(ps):
    return PcdView(97, 61, 64.0, 32.0, 48.25, 29.75, float(ps), 0.01)


def _edge_kinds(w, half):
    """u (or v) with u - half whole, whole + 0.5, and one fp32 ulp either side of whole."""
    t = w + half
    return [t, t + 0.5, up(t), down(t)]


def _sprite_lattice(view, nu, nv, z):
    half = view.point_size * 0.5
    us = [u for n in nu for u in _edge_kinds(n, half)]
    vs = [v for n in nv for v in _edge_kinds(n, half)]
    uu, vv = np.meshgrid(us, vs, indexing="ij")
    return lattice(view, uu.ravel(), vv.ravel(), np.resize(np.asarray(z, np.float64), uu.size))


def _frame_edge_points(view, z):
    """Sprites that show exactly one column (row) at each frame edge, and sprites that miss each edge by one."""
    W, H, ps, half = view.width, view.height, int(view.point_size), view.point_size * 0.5
    pts, shows = [], []
    # (start column or row, does one line show): whole starts and starts that ceil rounds up onto the same whole
    cols = [(-ps + 1, True), (-ps + 0.5, True), (-ps, False), (-ps - 0.5, False), (W - 1, True), (W - 1.5, True), (W, False), (W - 0.5, False)]
    rows = [(-ps + 1, True), (-ps + 0.5, True), (-ps, False), (-ps - 0.5, False), (H - 1, True), (H - 1.5, True), (H, False), (H - 0.5, False)]
    for k, (a, s) in enumerate(cols):
        pts.append(lattice(view, a + half, 4.0 + 6 * k + half, z))
        shows.append(s)
    for k, (b, s) in enumerate(rows):
        pts.append(lattice(view, 6.0 + 10 * k + half, b + half, z))
        shows.append(s)
    return np.concatenate(pts), np.array(shows)


@functools.lru_cache(maxsize=None)
def sprites(ps):
    """Identity camera, every rounding edge of ceil(u - ps / 2) and every frame edge, in both clouds."""
    view = sprite_view(ps)
    rng = np.random.default_rng(100 + ps)
    mv_lat = _sprite_lattice(view, (20, 40, 70), (18, 35, 50), 1.0)
    bg_lat = _sprite_lattice(view, (23, 44, 66), (20, 33, 47), (2.0, 0.5))          # farther and nearer than the movable lattice
    mv_edge, mv_shows = _frame_edge_points(view, 1.0)
    bg_edge, bg_shows = _frame_edge_points(view, 2.0)
    # candidate 1 moves the cloud 8 m (512 pixels) to the right: the lattice leaves the frame, and three points placed 8 m to the left
    # arrive: one shows pixel (0, 0) alone, one misses the corner by one, one is a whole sprite mid-frame, larger than the rectangle
    # of the others
    half = view.point_size * 0.5
    late = lattice(view, [-ps + 1 + half, -ps + half, 30 + half], [-ps + 1 + half, -ps + 1 + half, 20 + half], 1.0)
    late[:, 0] -= 8.0
    mv_xyz = np.concatenate([mv_lat, mv_edge, late])
    bg_xyz = np.concatenate([bg_lat, bg_edge])
    poses = np.stack([shift(), shift(8.0), px_shift(view, 1, 0), px_shift(view, -0.5, 0.5), px_shift(view, 3, -2), shift(z=1.0),
                      shift(-64.0), px_shift(view, -1, -1)])
    what = dict(n_lattice=mv_lat.shape[0], mv_edge=slice(mv_lat.shape[0], mv_lat.shape[0] + mv_edge.shape[0]), mv_edge_shows=mv_shows,
                bg_edge=slice(bg_lat.shape[0], bg_xyz.shape[0]), bg_edge_shows=bg_shows, late=slice(mv_xyz.shape[0] - 3, mv_xyz.shape[0]))
    return (bg_xyz, _rgb(rng, bg_xyz.shape[0]), mv_xyz, _rgb(rng, mv_xyz.shape[0]), view, np.eye(4, dtype=np.float32),
            np.eye(4, dtype=np.float32), poses, what)


@functools.lru_cache(maxsize=None)
def sprites_posed(ps):
    """A rotated, translated camera and a non-identity obj_pose_now: the candidate matrices are products that round."""
    view = sprite_view(ps)
    rng = np.random.default_rng(200 + ps)
    bg_xyz = rng.uniform([-0.7, -0.7, 0.0], [0.7, 0.7, 0.2], (1500, 3)).astype(np.float32)
    d = rng.normal(size=(600, 3))
    body = (0.12 * d / np.linalg.norm(d, axis=1, keepdims=True) + [0.0, 0.0, 0.15])            # the object where it stands in the world
    now = pose([1, 2, 3], 0.7, [0.1, -0.05, 0.02])
    Oi = pcd_ref.rigid_inverse(now)
    mv_xyz = (body @ Oi[:3, :3].T + Oi[:3, 3]).astype(np.float32)                              # ... in the object's own frame
    cam = look_at([0.3, -0.9, 0.6], [0.0, 0.0, 0.05])
    moves = [pose([0, 0, 1], 0.0, [0, 0, 0]), pose([1, 1, 5], 0.9, [0.3, 0.1, 0.0]), pose([2, -1, 4], -1.3, [-0.5, 0.2, 0.05]),
             pose([1, 0, 0.2], 0.4, [0.25, -0.75, 0.4]), pose([0, 1, 1], 2.0, [2.0, 0.0, 0.0]), pose([3, 1, 2], 0.2, [-0.1, -0.3, 0.0])]
    poses = np.stack([(m.astype(np.float64) @ now.astype(np.float64)).astype(np.float32) for m in moves])
    return (bg_xyz, _rgb(rng, 1500, 0, 256), mv_xyz, _rgb(rng, 600, 0, 256), view, cam, now, poses, dict())


# ---------------------------------------------------------------------------------------------------- B: tiles

TILE_FRAMES = ("8229x5", "3x5000", "336x336")
TILE_SIZES = (16, 2)


def movable_rect(M, xyz, view):
    """The clipped pixel rectangle the movable sprites cover, as k_pcd_candidates reduces it -> (x0, y0, x1, y1) or None."""
    _, j0, i0, ok = pcd_ref.project(M, xyz, view)
    if not ok.any():
        return None
    ps = int(view.point_size)
    j0, i0 = j0[ok], i0[ok]
    return (int(np.maximum(j0, 0).min()), int(np.maximum(i0, 0).min()),
            int(np.minimum(j0 + ps - 1, view.width - 1).max()), int(np.minimum(i0 + ps - 1, view.height - 1).max()))


def tile_grid(rect):
    """The kernel's formulas -> dict(rw, rh, tw, th, col_edges, row_edges, ...): edges are the first column / row of every tile
    after the first."""
    x0, y0, x1, y1 = rect
    rw, rh = x1 - x0 + 1, y1 - y0 + 1
    tw = min(rw, TILE_PX)
    th = min(rh, TILE_PX // tw)
    cols, rows = list(range(x0, x1 + 1, tw)), list(range(y0, y1 + 1, th))
    return dict(rw=rw, rh=rh, tw=tw, th=th, n_col=len(cols), n_row=len(rows), last_col=x1 - cols[-1] + 1, last_row=y1 - rows[-1] + 1,
                col_edges=cols[1:], row_edges=rows[1:])


def _steps(n, ps, extra=()):
    """Sprite starts 0, 7, 15, 23 ... n - ps: every 4096-aligned edge has a start one before it."""
    return sorted({0, n - ps} | {k for k in range(7, n - ps + 1, 8)} | {e for e in extra if e <= n - ps})


@functools.lru_cache(maxsize=None)
def tiles(frame, ps):
    """A rigid grid of movable points at depth 1 that pixel shifts push off the frame's left / top, so that the rectangle left on the
    frame takes the sizes the tile loops branch on; background points nearer (0.5) and farther (2) under every tile edge."""
    rng = np.random.default_rng(300 + ps + len(frame))
    if frame == "8229x5":
        view = PcdView(8229, 5, 64.0, 64.0, 4114.25, 2.25, float(ps), 0.01)
        A, B = _steps(8229, ps), [0, 1, 2, 3]
        shifts = [(0, 0), (-5200, 0), (-6400, 0), (-(A[-1] + ps - 1), -(B[-1] + ps - 1))]
    elif frame == "3x5000":
        view = PcdView(3, 5000, 64.0, 64.0, 1.25, 2500.25, float(ps), 0.01)
        A, B = [2 - ps, 3 - ps], _steps(5000, ps, (1364, 2729, 4094))
        shifts = [(0, 0), (-1, 0), (-2, 0)]
    elif frame == "336x336":
        view = PcdView(336, 336, 64.0, 64.0, 168.25, 167.75, float(ps), 0.01)
        A, B = _steps(336, ps), sorted({12 - ps, min(-1, 12 - ps)})
        shifts = [(0, 0), (0, 1)]
    else:
        raise KeyError(frame)
    W, H = view.width, view.height
    aa, bb = np.meshgrid(A, B, indexing="ij")
    mv_xyz = at(view, aa.ravel(), bb.ravel(), 1.0)
    poses = np.stack([px_shift(view, du, dv) for du, dv in shifts])
    # background: a scatter over the whole frame, and a block of points around every tile edge of every candidate
    n = min(1500, 3 * W * H // (2 * ps * ps))              # about one and a half sprites per pixel at most
    sa, sb = rng.integers(-ps + 1, W, n), rng.integers(-ps + 1, H, n)
    for M in pcd_ref.matrices(np.eye(4), np.eye(4), poses)[1]:
        rect = movable_rect(M, mv_xyz, view)
        g = tile_grid(rect)
        for e in g["col_edges"]:
            ea, eb = np.meshgrid([e - ps, e - 2, e - 1, e, e + 1], np.arange(-ps + 1, H, max(1, ps // 2))[:40], indexing="ij")
            sa, sb = np.concatenate([sa, ea.ravel()]), np.concatenate([sb, eb.ravel()])
        for e in g["row_edges"]:
            ea, eb = np.meshgrid(np.arange(rect[0] - ps + 1, rect[2] + 1, max(1, ps // 2))[:40], [e - ps, e - 2, e - 1, e, e + 1], indexing="ij")
            sa, sb = np.concatenate([sa, ea.ravel()]), np.concatenate([sb, eb.ravel()])
    bz = np.where(rng.random(sa.size) < 1.0 / ps, 0.5, 2.0)      # large sprites overlap: fewer near ones, or they would hide every far one
    bg_xyz = at(view, sa, sb, bz)
    return (bg_xyz, _rgb(rng, bg_xyz.shape[0], 0, 256), mv_xyz, _rgb(rng, mv_xyz.shape[0], 0, 256), view, np.eye(4, dtype=np.float32),
            np.eye(4, dtype=np.float32), poses, dict())


# ---------------------------------------------------------------------------------------------------- C: depth

DEPTH_KINDS = ("near", "near0")
NEAR = float(F32(0.01))


def odd_points():
    """Coordinates pcd_project documents as culled before an index is formed: NaN, infinities and overflow in each coordinate, a u
    that overflows to inf, and sprite starts that are finite but far beyond the int range.  One of them is not culled and must not
    be: z = 3e38 with finite x and y is a point very far away on the optical axis (ODD_KEPT)."""
    out = []
    for k in range(3):
        for val in (np.nan, np.inf, -np.inf, 3e38, -3e38):
            p = [0.1, 0.1, 1.0]
            p[k] = val
            out.append(p)
    out += [[3e37, 0.0, 1.0], [0.0, -3e37, 1.0], [1e12, 0.0, 1.0], [-1e12, 0.0, 1.0], [0.0, 1e12, 1.0], [0.0, -1e12, 1.0]]
    return np.array(out, np.float32)


ODD_KEPT = 13            # odd_points()[13] = (0.1, 0.1, 3e38)


@functools.lru_cache(maxsize=None)
def depth(kind):
    """Pairs of points in 8 x 8 pixel slots, the second two columns right of and one row below the first: 4 x 4 sprites that overlap in
    2 x 3 pixels and each show alone elsewhere.  Each pair is (cloud, z, cloud, z) with "b" the background and "m" the movable cloud;
    within one cloud the first of a pair has the lower index."""
    near = NEAR if kind == "near" else 0.0
    view = PcdView(64, 48, 32.0, 32.0, 31.75, 24.25, 4.0, near)
    rng = np.random.default_rng(400 + len(kind))
    z1, z2 = 1.0, up(1.0)
    sub = float(np.ldexp(1.0, -130))
    if kind == "near":
        pairs = [(c, z, d, 1.0) for z in (NEAR, up(NEAR), down(NEAR)) for c, d in (("b", "b"), ("m", "m"), ("m", "b"), ("b", "m"))]
        pairs += [("b", z1, "b", z2), ("b", z2, "b", z1), ("m", z1, "m", z2), ("m", z2, "m", z1), ("b", z1, "m", z2), ("b", z2, "m", z1),
                  ("m", z1, "b", z2), ("m", z2, "b", z1)]
        pairs += [("b", 1.5, "b", 1.5), ("m", 1.5, "m", 1.5), ("b", 1.5, "m", 1.5), ("m", 1.5, "b", 1.5)]
    else:
        pairs = [(c, z, d, 1.0) for z in (sub, -0.0, 0.0, -1.0, -sub) for c, d in (("b", "b"), ("m", "m"), ("m", "b"), ("b", "m"))]
        pairs += [("b", sub, "b", up(sub)), ("b", up(sub), "b", sub), ("m", up(sub), "m", sub), ("b", up(sub), "m", sub)]
    clouds = {"b": [], "m": []}
    for s, (c, zc, d, zd) in enumerate(pairs):
        sx, sy = 8 * (s % 8), 8 * (s // 8)
        clouds[c].append(at(view, sx + 1, sy + 1, zc))
        clouds[d].append(at(view, sx + 3, sy + 2, zd))
    assert len(pairs) <= 48
    if kind == "near0":      # the smallest subnormal depth, on the optical axis (x = y = 0 is the only lattice point it has)
        clouds["m"].append(np.array([[0.0, 0.0, np.ldexp(1.0, -149)]], np.float32))
        clouds["b"].append(at(view, 31, 23, 1.0))
    bg_xyz = np.concatenate(clouds["b"] + [odd_points()])
    mv_xyz = np.concatenate(clouds["m"] + [odd_points()])
    poses = np.stack([shift(), shift(1.0 / 32), shift(z=2.0 ** -10)])
    return (bg_xyz, _rgb(rng, bg_xyz.shape[0]), mv_xyz, _rgb(rng, mv_xyz.shape[0]), view, np.eye(4, dtype=np.float32),
            np.eye(4, dtype=np.float32), poses, dict(pairs=pairs, n_odd=odd_points().shape[0]))


# ---------------------------------------------------------------------------------------------------- D: empty

EMPTY_KINDS = ("bg0", "mv0", "both0", "K0", "K1", "mv_behind", "bg_culled")


@functools.lru_cache(maxsize=None)
def empty(kind):
    view = PcdView(40, 30, 32.0, 32.0, 20.25, 14.75, 3.0, 0.01)
    rng = np.random.default_rng(500)
    bg_xyz = rng.uniform([-1.0, -0.8, 1.0], [1.0, 0.8, 3.0], (400, 3)).astype(np.float32)
    mv_xyz = rng.uniform([-0.2, -0.2, 0.8], [0.2, 0.2, 1.2], (150, 3)).astype(np.float32)
    bg_rgb, mv_rgb = _rgb(rng, 400, 0, 256), _rgb(rng, 150, 0, 256)
    poses = np.stack([shift(), shift(0.1, -0.05), shift(-0.3, 0.1, 0.5)])
    if kind in ("bg0", "both0"):
        bg_xyz, bg_rgb = bg_xyz[:0], bg_rgb[:0]
    if kind in ("mv0", "both0"):
        mv_xyz, mv_rgb = mv_xyz[:0], mv_rgb[:0]
    if kind == "K0":
        poses = poses[:0]
    if kind == "K1":
        poses = poses[1:2]
    if kind == "mv_behind":
        poses = poses + shift(z=-5.0) - shift()
    if kind == "bg_culled":
        bg_xyz = bg_xyz * np.array([1, 1, -1], np.float32)
    return (bg_xyz, bg_rgb, mv_xyz, mv_rgb, view, np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), poses, dict(kind=kind))


# ---------------------------------------------------------------------------------------------------- E: colour

@functools.lru_cache(maxsize=None)
def colour():
    """27 background and 27 movable points, one per combination of {220, 221, 255} in the three channels, sprites 2 x 2 and 4 pixels
    apart: each is the winner of its own pixels, and most of the frame is reached by no point."""
    view = PcdView(40, 30, 32.0, 32.0, 20.25, 14.75, 2.0, 0.01)
    combos = np.array([[r, g, b] for r in (220, 221, 255) for g in (220, 221, 255) for b in (220, 221, 255)], np.uint8)
    i = np.arange(27)
    bg_xyz = at(view, 1 + 4 * (i % 9), 1 + 4 * (i // 9), 2.0)
    mv_xyz = at(view, 1 + 4 * (i % 9), 15 + 4 * (i // 9), 1.0)
    poses = np.stack([shift(), px_shift(view, 1, 0)])
    return (bg_xyz, combos, mv_xyz, combos[::-1].copy(), view, np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), poses, dict())


# ---------------------------------------------------------------------------------------------------- the list

CASES = {}
CASES.update({f"sprites-{ps}": (sprites, ps) for ps in SPRITE_SIZES})
CASES.update({f"sprites_posed-{ps}": (sprites_posed, ps) for ps in (2, 5)})
CASES.update({f"tiles-{fr}-{ps}": (tiles, fr, ps) for fr in TILE_FRAMES for ps in TILE_SIZES})
CASES.update({f"depth-{k}": (depth, k) for k in DEPTH_KINDS})
CASES.update({f"empty-{k}": (empty, k) for k in EMPTY_KINDS})
CASES["colour"] = (colour,)


def build(name):
    fn, *a = CASES[name]
    return fn(*a)


@functools.lru_cache(maxsize=None)
def expected(name):
    """pcd_ref.render of the case, computed once and shared (read-only)."""
    out = pcd_ref.render(*args(build(name)))
    out.setflags(write=False)
    return out
