"""Seeded scenes for the mesh-picture renderer (test_meshvis_host.py, test_meshvis_gpu.py): the fill rule, clipping, depth,
items, cubes and sizes.  `case(name)` builds the arguments of meshvis_ref.render / _lib.mesh_render as a dict; `rule(name)`
renders the rule once per process and keeps (rgb, ids, details).

The fill-rule scene uses an identity camera, power-of-two fx and fy and coordinates with few mantissa bits, so u and v are exact in
fp32 (pcd_edge_cases.lattice asserts it) and the snapped vertex of every triangle can be read off its construction."""
from __future__ import annotations

import functools

import numpy as np

from tests import meshvis_ref
from tests.pcd_edge_cases import lattice, look_at, pose, up
from tests.pcd_ref import PcdView

EYE = np.eye(4, dtype=np.float32)
NAMES = ("A", "B", "C", "D", "E", "E_k0", "E_nt0", "E_empty", "F_many", "F_wide", "F_small")


def _view(w, h, f, near=0.01):
    return PcdView(width=w, height=h, fx=float(f), fy=float(f), cx=float(w // 2), cy=float(h // 2), point_size=1.0, near=near)


def _soup(tri_list, items=None):
    """a list of [3,3] world triangles -> verts, tris, tri_item (every triangle owns its vertices)"""
    P = np.asarray(tri_list, np.float32).reshape(-1, 3, 3)
    n = P.shape[0]
    return P.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3), np.zeros(n, np.uint32) if items is None else np.asarray(items, np.uint32)


def _world(view, uvz):
    """general (u, v, z) -> world points under an identity camera (not exact: for cases that do not sit on a rounding edge)"""
    uvz = np.asarray(uvz, np.float64).reshape(-1, 3)
    return np.stack([(uvz[:, 0] - view.cx) * uvz[:, 2] / view.fx, (uvz[:, 1] - view.cy) * uvz[:, 2] / view.fy, uvz[:, 2]], 1).astype(np.float32)


def _pack(view, verts, tris, item, mats=None, cols=None, cam=EYE, cubes=None, background=(255, 255, 255), what=None):
    n_items = int(item.max()) + 1 if item.size else 1
    mats = np.tile(EYE, (n_items, 1, 1)) if mats is None else np.asarray(mats, np.float32)
    cols = np.array([[200, 120, 40], [40, 200, 120], [120, 40, 200], [220, 220, 60]], np.uint8)[:n_items] if cols is None else np.asarray(cols, np.uint8)
    cc, ch, cs = cubes if cubes is not None else (None, None, None)
    return dict(view=view, cam_pose=np.asarray(cam, np.float32), verts=verts, tris=tris, tri_item=item, item_mats=mats, item_rgb=cols,
                cube_centres=None if cc is None else np.asarray(cc, np.float32), cube_half=None if ch is None else np.asarray(ch, np.float32),
                cube_scores=None if cs is None else np.asarray(cs, np.uint16), background=background, what=what or {})


def _case_A():
    """fill rule, 33 x 17"""
    view = _view(33, 17, 16)
    s = 1.0 / 16
    tri = []

    def add(uv, z=1.0):
        uv = np.asarray(uv, np.float64) + 0.5        # pixel (i, j) is sampled at (16 j + 8, 16 i + 8): its centre is u = j + 0.5
        tri.append(lattice(view, uv[:, 0], uv[:, 1], z))
    c = (8, 8)                                      # a fan of 8 around a vertex on a pixel centre, windings alternating
    ring = [(12, 8), (11, 11), (8, 12), (5, 11), (4, 8), (5, 5), (8, 4), (11, 5)]
    for i in range(8):
        a, b = ring[i], ring[(i + 1) % 8]
        add([c, a, b] if i % 2 == 0 else [c, b, a])
    add([(16, 2), (28, 2), (28, 14)])               # a quad: edges through centres horizontally, vertically and along the diagonal
    add([(16, 2), (16, 14), (28, 14)])              # (the other winding)
    add([(1, 1), (2, 2), (3, 3)])                   # zero area
    add([(2 - s, 13), (4 + s, 13 + s), (2, 16 - s)], z=0.5)     # a sixteenth either side of centres
    h = 1.0 / 32                                    # 16 u = 16.5 and 49.5: the half-way points of rint (-> 16 and 50)
    add([(0.5 + h, 0.5 + h), (2.5 + 3 * h, 0.5 + h), (0.5 + h, 2.5 + 3 * h)], z=2.0)
    verts, tris, item = _soup(tri)
    return _pack(view, verts, tris, item, what=dict(zero_area=10, n_fan=8))


def _case_B():
    """clipping, 97 x 61"""
    view = _view(97, 61, 64, near=0.25)
    lim = 131072.0
    tri, what = [], {}

    def add(name, P):
        what[name] = len(tri)
        tri.append(np.asarray(P, np.float32))
    add("quad0", _world(view, [(-40, -30, 3), (140, -30, 6), (140, 90, 6)]))          # overflows the frame on all sides, tilted
    add("quad1", _world(view, [(-40, -30, 3), (140, 90, 6), (-40, 90, 3)]))
    add("whole", _world(view, [(-300, -200, 4), (500, -200, 4), (100, 600, 4)]))       # covers every pixel; the quad passes through it
    add("below_limit", np.concatenate([lattice(view, [10, 10], [5, 25], 1.0), lattice(view, lim - 1 / 64, 15, 1.0)]))
    add("at_limit", np.concatenate([lattice(view, [10, 10], [35, 55], 1.0), lattice(view, lim, 45, 1.0)]))
    add("z_eq_near", [(-0.1, -0.1, 0.25), (0.0, -0.1, 0.25), (-0.1, 0.0, 0.25)])
    zu = up(0.25)
    add("z_above_near", [(0.02, -0.1, zu), (0.12, -0.1, zu), (0.02, 0.0, zu)])
    add("nan", [(np.nan, 0, 1), (0.1, 0, 1), (0, 0.1, 1)])
    add("inf", [(np.inf, 0, 1), (0.1, 0, 1), (0, 0.1, 1)])
    add("z_inf", [(0, 0, np.inf), (0.1, 0, 1), (0, 0.1, 1)])
    add("off_frame", _world(view, [(200, 10, 1), (260, 10, 1), (200, 50, 1)]))
    add("small", _world(view, [(60, 40, 0.5), (66, 41, 0.5), (61, 47, 0.5)]))          # the thread path beside the workgroup path
    add("behind", [(0, 0, -1), (0.1, 0, -1), (0, 0.1, -1)])
    verts, tris, item = _soup(tri)
    return _pack(view, verts, tris, item, what=what)


def _case_C():
    """depth, 64 x 48"""
    view = _view(64, 48, 64)
    tri, what = [], {}

    def add(name, P):
        what[name] = len(tri)
        tri.append(np.asarray(P, np.float32))
    # coplanar (z = 2: every q is exactly 0.5) overlapping pairs, the lower index first in one and second in the other
    add("co_a0", lattice(view, [2, 14, 2], [2, 2, 14], 2.0))
    add("co_a1", lattice(view, [4, 16, 16], [2, 2, 14], 2.0))
    add("co_b0", lattice(view, [24, 36, 36], [2, 2, 14], 2.0))
    add("co_b1", lattice(view, [22, 34, 22], [2, 2, 14], 2.0))
    # two triangles that pass through each other: z runs 1 -> 4 one way and 3 -> 1 the other
    add("cross0", _world(view, [(4, 18, 1), (60, 32, 4), (4, 46, 1)]))
    add("cross1", _world(view, [(60, 18, 1), (4, 32, 3), (60, 46, 1)]))
    # one fp32 ulp apart in depth, the nearer one at the higher index
    add("ulp_far", lattice(view, [44, 60, 44], [2, 2, 14], 1.0) * np.float32(up(2.0)))
    add("ulp_near", lattice(view, [44, 60, 44], [2, 2, 14], 2.0))
    verts, tris, item = _soup(tri, items=[0, 1, 0, 1, 2, 3, 0, 1])
    return _pack(view, verts, tris, item, what=what)


def _sphere(n_lat, n_lon, radius):
    th = np.linspace(0, np.pi, n_lat + 1)
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    V = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones_like(ph))], -1) * radius
    T = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b, c, d = i * n_lon + j, i * n_lon + (j + 1) % n_lon, (i + 1) * n_lon + j, (i + 1) * n_lon + (j + 1) % n_lon
            T += [(a, c, b), (b, c, d)]
    return V.reshape(-1, 3).astype(np.float32), np.array(T, np.uint32)


def _case_D():
    """items, 97 x 61: three spheres of 1 000 triangles under rotations without a zero entry, a rolled camera looking down"""
    view = PcdView(width=97, height=61, fx=90.3, fy=89.7, cx=47.6, cy=30.2, point_size=1.0, near=0.01)
    V, T = _sphere(20, 25, 0.07)
    verts = np.concatenate([V, V, V])
    tris = np.concatenate([T, T + np.uint32(len(V)), T + np.uint32(2 * len(V))])
    item = np.repeat(np.arange(3, dtype=np.uint32), len(T))
    mats = np.stack([pose((1, 2, 3), 0.7, (-0.09, 0.02, 0.07)), pose((-2, 1, 0.5), 1.9, (0.07, -0.05, 0.07)), pose((0.3, -1, 2), -2.6, (0.02, 0.11, 0.07))])
    cam = look_at((0.32, -0.27, 0.42), (0.0, 0.02, 0.04))
    return _pack(view, verts, tris, item, mats=mats, cols=[[230, 60, 50], [60, 200, 90], [70, 90, 240]], cam=cam, background=(12, 20, 28))


def _cubes_E():
    # in front of the mesh, behind it, cut by it; two equal scores overlapping; scores 0, 1 and 65535
    cc = [(-0.25, -0.15, 1.2), (0.0, -0.15, 2.6), (0.25, -0.15, 2.115), (-0.2, 0.18, 1.5), (-0.12, 0.2, 1.5), (0.1, 0.2, 1.4), (0.22, 0.2, 1.4),
          (0.34, 0.2, 1.4)]
    ch = [0.08, 0.2, 0.09, 0.07, 0.07, 0.05, 0.05, 0.05]
    cs = [40000, 50000, 30000, 20000, 20000, 0, 1, 65535]
    return cc, ch, cs


def _case_E(mesh=True, cubes=True):
    """cubes, 64 x 48: a tilted wall at z about 2 and eight cubes"""
    view = _view(64, 48, 64)
    wall = [[(-1.0, -0.6, 1.9), (1.0, -0.6, 2.1), (1.0, 0.6, 2.1)], [(-1.0, -0.6, 1.9), (1.0, 0.6, 2.1), (-1.0, 0.6, 1.9)]]
    verts, tris, item = _soup(wall if mesh else [])
    return _pack(view, verts, tris, item, cubes=_cubes_E() if cubes else None, background=(250, 250, 250))


def _case_F_many():
    """70 000 tiny triangles (more than 65 535) at 128 x 96"""
    r = np.random.default_rng(19)
    view = _view(128, 96, 128)
    n = 70000
    c = np.stack([r.uniform(-2, 130, n), r.uniform(-2, 98, n), r.uniform(1.0, 3.0, n)], 1)
    d = r.uniform(-1.5, 1.5, (n, 3, 3)) * np.array([1, 1, 0.02])
    P = _world(view, (c[:, None, :] + d).reshape(-1, 3)).reshape(n, 3, 3)
    verts, tris, item = _soup(P, items=r.integers(0, 4, n))
    return _pack(view, verts, tris, item)


def _case_F_wide(w=4100, h=3):
    view = PcdView(width=w, height=h, fx=64.0, fy=64.0, cx=w / 2.0, cy=h / 2.0, point_size=1.0, near=0.01)
    r = np.random.default_rng(23)
    n = 60
    c = np.stack([r.uniform(0, w, n), r.uniform(0, h, n), r.uniform(1.0, 3.0, n)], 1)
    d = r.uniform(-1, 1, (n, 3, 3)) * np.array([0.03 * w, 4.0, 0.05])
    P = _world(view, (c[:, None, :] + d).reshape(-1, 3)).reshape(n, 3, 3)
    verts, tris, item = _soup(P, items=r.integers(0, 3, n))
    cc = _world(view, np.stack([r.uniform(0, w, 6), r.uniform(0, h, 6), r.uniform(1.0, 2.5, 6)], 1))
    return _pack(view, verts, tris, item, cubes=(cc, np.full(6, max(0.02 * w / 64, 0.06), np.float32), [9000, 22000, 35000, 48000, 61000, 65535]))


@functools.lru_cache(maxsize=None)
def case(name):
    return {"A": _case_A, "B": _case_B, "C": _case_C, "D": _case_D, "E": _case_E, "E_k0": lambda: _case_E(cubes=False),
            "E_nt0": lambda: _case_E(mesh=False), "E_empty": lambda: _case_E(mesh=False, cubes=False), "F_many": _case_F_many,
            "F_wide": _case_F_wide, "F_small": lambda: _case_F_wide(40, 30)}[name]()


def args(c):
    return {k: v for k, v in c.items() if k != "what"}


@functools.lru_cache(maxsize=None)
def rule(name, wrong=None):
    """-> (rgb, ids, details) of the rule (or of one of meshvis_ref.WRONG_RULES) on a case; the arrays are read-only"""
    rgb, ids, det = meshvis_ref.render(**args(case(name)), wrong=wrong, details=True)
    rgb.setflags(write=False)
    ids.setflags(write=False)
    return rgb, ids, det
