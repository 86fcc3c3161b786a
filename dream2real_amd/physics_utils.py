"""Batched physics pre-filter of candidate poses on the GPU: the counterpart of the reference's
`create_unsupcol_check` / `unsupcol_check` (vision_3d/physics_utils.py:232-375), which walks the N sampled
poses in a Python loop with four to six PyBullet collision queries each.

Same contract: `create_unsupcol_check(ctx, task_model, sample_res, embodied, unsup_thresh, lazy_phys_mods,
stability_check)` returns `(unsupcol_check, static_obj_handles, movable_handles)` with
`unsupcol_check(pose_batch, task_model, valid_so_far, disallow_regrasp=embodied) -> bool tensor [N]`, the closure
`optimise_pose_grid` takes as `phys_check` (reference dream2real.py:304-326, clip_scoring.py:108-113).  `ctx` (an
engine.Context) stands where the reference passes `pyb_planner`.

Shapes come from where the reference takes them: every object's `phys_model` is the path of a Wavefront .obj mesh in
world coordinates (reference :238 `createCollisionShape(GEOM_MESH, fileName=obj.phys_model)`; written by
get_phys_models :25-229; its TSDF branch is `get_phys_models` below, Poisson and VHACD stay outside the path).  PyBullet turns each shape of the file (an `o` /
`g` group: VHACD writes one per convex part) into the convex hull of its vertices, so an object is a compound of
convex parts: `hulls_from_obj` reads exactly that.  Objects may instead carry vertex arrays (`phys_hull` /
`phys_hulls`), which take precedence — tests and callers without mesh files use them.

A second backend needs no convex parts: `get_phys_models(..., phys_backend="tsdf")` writes
`sdf_{id}.npz` — the TSDF volume's "touch" bits and its observed solid voxels — and when every object's `phys_model` is such
a file, `create_unsupcol_check` answers the same three questions point against field (`SdfPhysicsShapes`).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

GRAVITY_DIRECTION = np.array([0, 0, -1])          # reference vision_3d/physics_utils.py:18
# Collision margin PyBullet gives a convex hull it loads from a mesh file (believed: its default collision margin for
# file-loaded convex shapes is 0.001 m, and getClosestPoints at distance 0 — what pairwise_collision asks — reports
# two bodies whose hulls are closer than the sum of their margins).  PyBullet is not available offline: UNPINNED.
PYBULLET_MESH_MARGIN = 0.001


def hulls_from_obj(path: str) -> list:
    """Vertex sets of the convex parts of a Wavefront .obj, one per shape as PyBullet's GEOM_MESH loader (tinyobj)
    splits the file: a new shape starts at every `o` or `g` line, and a shape's vertices are the ones its faces
    reference (indices are global, 1-based, negative = relative to the vertices read so far; `v/vt/vn` forms
    accepted).  A file without groups is one shape; a shape without faces is skipped; a file with vertices but no
    faces at all is one shape of all its vertices (a point cloud's hull)."""
    verts, shapes, cur = [], [], set()

    def close():
        if cur:
            shapes.append(sorted(cur))
        cur.clear()

    with open(path, "r", errors="replace") as f:
        for line in f:
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            if t[0] == "v" and len(t) >= 4:
                verts.append((float(t[1]), float(t[2]), float(t[3])))
            elif t[0] in ("o", "g"):
                close()
            elif t[0] == "f":
                for tok in t[1:]:
                    i = int(tok.split("/")[0])
                    i = i - 1 if i > 0 else len(verts) + i
                    if not 0 <= i < len(verts):
                        raise ValueError(f"{path}: face references vertex {tok} of {len(verts)}")
                    cur.add(i)
    close()
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    if not shapes:
        if len(v) == 0:
            raise ValueError(f"{path}: no vertices")
        return [v]
    return [v[idx] for idx in shapes]


def object_hulls(obj) -> list:
    """Convex parts of a scene object: `phys_hulls` (list of [V,3]) or `phys_hull` ([V,3]) when the object carries
    vertex arrays, else the shapes of its `phys_model` mesh file (reference scene_model.py:14-17)."""
    if getattr(obj, "phys_hulls", None) is not None:
        return [np.asarray(h, np.float64).reshape(-1, 3) for h in obj.phys_hulls]
    if getattr(obj, "phys_hull", None) is not None:
        return [np.asarray(obj.phys_hull, np.float64).reshape(-1, 3)]
    model = getattr(obj, "phys_model", None)
    if model is None:
        raise ValueError("object has neither hull vertex arrays nor a phys_model mesh path")
    return hulls_from_obj(model)


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _as_parts(hulls, what):
    """One hull ([V,3] array, nested list or tensor) or a sequence of hulls -> list of [V,3] float64 arrays.  A bare
    [V,3] list-of-lists is ONE hull (iterating it would give V one-point 'hulls' that pass validation and collide wrongly)."""
    if hasattr(hulls, "detach") or isinstance(hulls, np.ndarray):
        hulls = _np(hulls)
    else:
        try:
            arr = np.asarray([_np(h) for h in hulls], np.float64)
        except (ValueError, TypeError):
            arr = None                                   # ragged: a real sequence of hulls
        if arr is not None and arr.ndim == 2 and arr.shape[1] == 3:
            hulls = arr
    if isinstance(hulls, np.ndarray):
        if hulls.ndim == 2 and hulls.shape[1] == 3:
            hulls = [hulls]
        elif hulls.ndim == 3 and hulls.shape[2] == 3:
            hulls = list(hulls)
        else:
            raise ValueError(f"{what}: expected [V,3] vertices or a sequence of such arrays, got shape {hulls.shape}")
    parts = []
    for k, h in enumerate(hulls):
        a = np.asarray(_np(h), np.float64)
        if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1:
            raise ValueError(f"{what}: part {k} must be a [V,3] array with at least one vertex, got shape {a.shape}")
        parts.append(a)
    return parts


def _pack(hulls):
    hs = [np.asarray(h, np.float64).reshape(-1, 3) for h in hulls]
    off = np.zeros(len(hs) + 1, np.uint32)
    off[1:] = np.cumsum([len(h) for h in hs])
    v = np.ascontiguousarray(np.concatenate(hs) if hs else np.zeros((0, 3)), np.float32)
    return v, off


class PhysicsShapes:
    """d2r_phys: the movable object's convex part(s) and the static parts on the GPU."""

    def __init__(self, ctx, movable_hulls, static_hulls):
        self.ctx = ctx
        movable_hulls = _as_parts(movable_hulls, "movable_hulls")      # a single hull in any array-like form, or parts
        static_hulls = _as_parts(static_hulls, "static_hulls") if len(static_hulls) else []
        mv, moff = _pack(movable_hulls)
        sv, soff = _pack(static_hulls)
        h = C.c_void_p()
        ctx.check(ctx.lib.d2r_phys_create(ctx.h, _lib.ptr(mv), _lib.ptr(moff), len(moff) - 1,
                                          _lib.ptr(sv) if len(sv) else None, _lib.ptr(soff), len(soff) - 1, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.d2r_phys_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, pose_batch, valid_so_far, sample_res, init_pose, table_z, unsup_thresh=0.02,
              stability_check=True, disallow_regrasp=False, perturb=0.04, margin=0.0) -> np.ndarray:
        poses = np.ascontiguousarray(np.asarray(pose_batch, np.float64).reshape(-1, 16), np.float32)
        valid = np.ascontiguousarray(np.asarray(valid_so_far).astype(np.uint8).reshape(-1))
        assert valid.shape[0] == poses.shape[0]
        prm = _phys_params(sample_res, init_pose, table_z, unsup_thresh, perturb, stability_check, disallow_regrasp, margin)
        self.ctx.check(self.ctx.lib.d2r_phys_check(self.ctx.h, self.h, C.byref(prm), _lib.ptr(poses), poses.shape[0], _lib.ptr(valid)))
        return valid.astype(bool)


SDF_CONTACT = 2 * PYBULLET_MESH_MARGIN      # the distance at which the hull backend calls two parts "in contact"
_SDF_GRID_KEYS = ("b0", "nv", "voxel", "trunc")


def _phys_params(sample_res, init_pose, table_z, unsup_thresh, perturb, stability_check, disallow_regrasp, margin):
    return _lib.PhysParams((C.c_uint32 * 6)(*[int(x) for x in sample_res]),
                           (C.c_float * 16)(*np.asarray(init_pose, np.float64).reshape(16)),
                           float(table_z), float(unsup_thresh), (C.c_float * 3)(*[float(x) for x in GRAVITY_DIRECTION]),
                           float(perturb), int(bool(stability_check)), int(bool(disallow_regrasp)), float(margin))


def save_sdf_model(path, grid, weight_threshold, contact, words, points):
    """sdf_{id}.npz: the grid header (b0, nv, voxel, trunc), the two constants the field was cut with, the touch words
    uint32 [nz, ny, ceil(nx / 32)] and the solid points float32 [n, 3]."""
    b0, nv, voxel, trunc = grid
    np.savez_compressed(path, b0=np.asarray(b0, np.int32), nv=np.asarray(nv, np.uint32), voxel=np.float32(voxel), trunc=np.float32(trunc),
                        weight_threshold=np.float32(weight_threshold), contact=np.float32(contact),
                        words=np.ascontiguousarray(words, np.uint32), points=np.ascontiguousarray(points, np.float32).reshape(-1, 3))


def load_sdf_model(path) -> dict:
    with np.load(path) as z:
        m = {k: z[k] for k in z.files}
    nx, ny, nz = (int(v) for v in m["nv"])
    if m["words"].shape != (nz, ny, (nx + 31) // 32):
        raise ValueError(f"{path}: touch words of shape {m['words'].shape} do not fit the grid {nx} x {ny} x {nz}")
    return m


class SdfPhysicsShapes:
    """d2r_sdfphys: the static scene as one touch bit per voxel (`words`: one grid or a stack of grids, ORed) and the movable
    object's solid points, on the GPU."""

    def __init__(self, ctx, b0, nv, voxel, words, points):
        self.ctx = ctx
        b0 = np.ascontiguousarray(b0, np.int32).reshape(3)
        nv = np.ascontiguousarray(nv, np.uint32).reshape(3)
        nx, ny, nz = (int(v) for v in nv)
        w = np.ascontiguousarray(words, np.uint32)
        if w.ndim == 3:
            w = w[None]
        if w.ndim != 4 or w.shape[1:] != (nz, ny, (nx + 31) // 32):
            raise ValueError(f"touch words of shape {w.shape} do not fit the grid {nx} x {ny} x {nz}")
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        h = C.c_void_p()
        ctx.check(ctx.lib.d2r_sdfphys_create(ctx.h, _lib.ptr(b0), _lib.ptr(nv), voxel, _lib.ptr(w), w.shape[0],
                                             _lib.ptr(pts), pts.shape[0], C.byref(h)))
        self.h = h
        self.n_points = pts.shape[0]

    @classmethod
    def from_files(cls, ctx, static_paths, movable_path):
        """The static objects' sdf_{id}.npz files (their grids must be one grid) and the movable object's."""
        mov = load_sdf_model(movable_path)
        stat = [load_sdf_model(p) for p in static_paths]
        if not stat:
            raise ValueError("no static object to check against")
        for p, m in zip(list(static_paths) + [movable_path], stat + [mov]):
            for k in _SDF_GRID_KEYS:
                if not np.array_equal(m[k], stat[0][k]):
                    raise ValueError(f"{p}: grid differs from {static_paths[0]} in {k} ({m[k]} against {stat[0][k]}); the volumes of a "
                                     "scene must be built over the same scene_bounds")
        if len(mov["points"]) == 0:
            raise ValueError(f"{movable_path}: the movable object has no solid points (seen in no frame)")
        return cls(ctx, stat[0]["b0"], stat[0]["nv"], float(stat[0]["voxel"]), np.stack([m["words"] for m in stat]), mov["points"])

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.d2r_sdfphys_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, pose_batch, valid_so_far, sample_res, init_pose, table_z, unsup_thresh=0.02,
              stability_check=True, disallow_regrasp=False, perturb=0.04, margin=0.0) -> np.ndarray:
        """PhysicsShapes.check's arguments; `margin` is ignored (the contact distance is in the bits)."""
        poses = np.ascontiguousarray(np.asarray(pose_batch, np.float64).reshape(-1, 16), np.float32)
        valid = np.ascontiguousarray(np.asarray(valid_so_far).astype(np.uint8).reshape(-1))
        assert valid.shape[0] == poses.shape[0]
        prm = _phys_params(sample_res, init_pose, table_z, unsup_thresh, perturb, stability_check, disallow_regrasp, 0.0)
        self.ctx.check(self.ctx.lib.d2r_sdfphys_check(self.ctx.h, self.h, C.byref(prm), _lib.ptr(poses), poses.shape[0], _lib.ptr(valid)))
        return valid.astype(bool)

    def timing(self):
        """(upload, kernel, download) of the last check, device-event milliseconds."""
        ms = np.zeros(3, np.float64)
        self.ctx.check(self.ctx.lib.d2r_sdfphys_get_timing(self.ctx.h, self.h, _lib.ptr(ms)))
        return tuple(float(x) for x in ms)


def _is_sdf_model(obj) -> bool:
    if getattr(obj, "phys_hulls", None) is not None or getattr(obj, "phys_hull", None) is not None:
        return False
    model = getattr(obj, "phys_model", None)
    return isinstance(model, (str, os.PathLike)) and os.fspath(model).endswith(".npz")


def create_unsupcol_check(ctx, task_model, sample_res, embodied, unsup_thresh=0.02, lazy_phys_mods=True, stability_check=True,
                          margin=PYBULLET_MESH_MARGIN, movable_hull=None, static_hulls=None):
    """-> (unsupcol_check, static_obj_handles, movable_handles), the reference's triple (vision_3d/physics_utils.py:232,377).

    Objects checked, as the reference chooses them (:235): with `lazy_phys_mods` the merged background object and the
    movable object, otherwise every object of the scene model — all but the movable one static.  The handles are what
    stands for PyBullet's body ids here: per static object the list of its convex parts' vertex arrays, and for the
    movable object a one-element list holding its parts; `unsupcol_check.shapes` is the GPU-side object (close() frees it).
    `movable_hull` / `static_hulls` override the lookup with explicit vertex arrays.

    When every object's `phys_model` is an sdf_{id}.npz (get_phys_models(phys_backend="tsdf")) the check runs point against
    field (SdfPhysicsShapes; `margin` does not apply, the contact distance is in the bits) and the handles are the files'
    paths; a mix of .npz and mesh files is a ValueError."""
    if movable_hull is None and static_hulls is None:
        objs = [task_model.task_bground_obj, task_model.movable_obj] if lazy_phys_mods else list(task_model.scene_model.objs)
        sdf = [o for o in objs if _is_sdf_model(o)]
        if sdf and len(sdf) != len(objs):
            other = next(o for o in objs if not _is_sdf_model(o))
            raise ValueError(f"create_unsupcol_check: the objects mix physics backends: {sdf[0].phys_model} is a TSDF field "
                             f"(phys_backend='tsdf') and {getattr(other, 'phys_model', None)} is not; build all of them with one backend")
        if sdf:
            if not any(o is task_model.movable_obj for o in objs):
                raise ValueError("the movable object is not among the objects to check")
            static_paths = [os.fspath(o.phys_model) for o in objs if o is not task_model.movable_obj]
            movable_path = os.fspath(task_model.movable_obj.phys_model)
            field = SdfPhysicsShapes.from_files(ctx, static_paths, movable_path)

            def sdf_unsupcol_check(pose_batch, task_model, valid_so_far, disallow_regrasp=embodied):
                import torch
                valid = field.check(_np(pose_batch), _np(valid_so_far), sample_res, _np(task_model.movable_obj.pose),
                                    float(_np(task_model.scene_model.scene_centre)[2]), unsup_thresh, stability_check, disallow_regrasp)
                return torch.from_numpy(valid)

            sdf_unsupcol_check.shapes = field
            return sdf_unsupcol_check, static_paths, [movable_path]      # the handles: the objects' field files
    if movable_hull is not None or static_hulls is not None:
        mov = [np.asarray(movable_hull, np.float64).reshape(-1, 3)] if movable_hull is not None else object_hulls(task_model.movable_obj)
        static_objs = [[np.asarray(h, np.float64).reshape(-1, 3)] for h in static_hulls] if static_hulls is not None else \
            [object_hulls(task_model.task_bground_obj)]
    else:
        phys_obj_list = [task_model.task_bground_obj, task_model.movable_obj] if lazy_phys_mods else list(task_model.scene_model.objs)
        mov, static_objs = None, []
        for obj in phys_obj_list:
            if obj is task_model.movable_obj:
                mov = object_hulls(obj)
            else:
                static_objs.append(object_hulls(obj))
        if mov is None:
            raise ValueError("the movable object is not among the objects to check")
    shapes = PhysicsShapes(ctx, mov, [h for parts in static_objs for h in parts])

    def unsupcol_check(pose_batch, task_model, valid_so_far, disallow_regrasp=embodied):
        import torch
        valid = shapes.check(_np(pose_batch), _np(valid_so_far), sample_res, _np(task_model.movable_obj.pose),
                             float(_np(task_model.scene_model.scene_centre)[2]), unsup_thresh, stability_check,
                             disallow_regrasp, margin=margin)
        return torch.from_numpy(valid)

    unsupcol_check.shapes = shapes
    return unsupcol_check, static_objs, [mov]


# ------------------------------------------------------------------------------------- physics meshes from RGB-D (TSDF)

TSDF_VOXEL = 0.002                # reference vision_3d/physics_utils.py:62
TSDF_TRUNC_MULTIPLIER = 8         # Open3D's trunc_voxel_multiplier default (believed)
TSDF_WEIGHT_THRESHOLD = 3.0       # Open3D's extract_triangle_mesh default (believed)
TSDF_CLUSTER_KEEP = 0.02          # :107
ERODE_BACKGROUND, ERODE_OBJECT = 20, 8      # :77-80


class TsdfVolume:
    """d2r_tsdf: a dense (tsdf, weight) grid over `bounds` ([2][3] min, max) on the GPU; frames are integrated in call
    order, `extract` runs the marching cubes and the clean-up of DESIGN.md section 2c."""

    def __init__(self, ctx, bounds, voxel: float = TSDF_VOXEL, trunc: float | None = None):
        self.ctx = ctx
        self.voxel = np.float32(voxel)
        self.trunc = np.float32(TSDF_TRUNC_MULTIPLIER) * self.voxel if trunc is None else np.float32(trunc)
        b = np.ascontiguousarray(np.asarray(_np(bounds), np.float64).reshape(6), np.float32)
        h = C.c_void_p()
        ctx.check(ctx.lib.d2r_tsdf_create(ctx.h, _lib.ptr(b), self.voxel, self.trunc, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.d2r_tsdf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def integrate(self, depth_u16, mask, intrinsics, cam_pose, erode_k: int):
        d = np.ascontiguousarray(depth_u16, np.uint16)
        m = np.ascontiguousarray(mask, np.uint8)
        assert d.ndim == 2 and m.shape == d.shape
        K = np.ascontiguousarray(np.asarray(_np(intrinsics), np.float64).reshape(9), np.float32)
        T = np.ascontiguousarray(np.asarray(_np(cam_pose), np.float64).reshape(16), np.float32)
        self.ctx.check(self.ctx.lib.d2r_tsdf_integrate(self.h, _lib.ptr(d), _lib.ptr(m), d.shape[1], d.shape[0],
                                                       _lib.ptr(K), _lib.ptr(T), int(erode_k)))

    def integrate_rgb(self, depth_u16, mask, rgb, intrinsics, cam_pose, erode_k: int):
        """d2r_tsdf_integrate_rgb: `integrate` plus the frame's colours uint8 [h,w,3].  A volume takes its
        frames through one of the two calls only."""
        d = np.ascontiguousarray(depth_u16, np.uint16)
        m = np.ascontiguousarray(mask, np.uint8)
        c = np.ascontiguousarray(rgb, np.uint8)
        assert d.ndim == 2 and m.shape == d.shape and c.shape == d.shape + (3,)
        K = np.ascontiguousarray(np.asarray(_np(intrinsics), np.float64).reshape(9), np.float32)
        T = np.ascontiguousarray(np.asarray(_np(cam_pose), np.float64).reshape(16), np.float32)
        self.ctx.check(self.ctx.lib.d2r_tsdf_integrate_rgb(self.h, _lib.ptr(d), _lib.ptr(m), _lib.ptr(c), d.shape[1], d.shape[0],
                                                           _lib.ptr(K), _lib.ptr(T), int(erode_k)))

    def read_colours(self):
        """-> float32 [n,16,16,16,3] indexed [z][y][x][channel]: the colours of read_voxels' blocks, in its order."""
        n = C.c_uint32(0)
        self.ctx.check(self.ctx.lib.d2r_tsdf_read_colours(self.h, C.byref(n), None))
        cols = np.zeros((n.value, 16, 16, 16, 3), np.float32)
        if n.value:
            self.ctx.check(self.ctx.lib.d2r_tsdf_read_colours(self.h, C.byref(n), _lib.ptr(cols)))
        return cols

    def read_voxels(self):
        """-> (block coordinates int32 [n,3] (x, y, z), tsdf float32 [n,16,16,16] indexed [z][y][x], weight likewise), the
        blocks any frame touched in (z, y, x) order."""
        n = C.c_uint32(0)
        self.ctx.check(self.ctx.lib.d2r_tsdf_read_voxels(self.h, C.byref(n), None, None, None))
        coords = np.zeros((n.value, 3), np.int32)
        tsdf = np.zeros((n.value, 16, 16, 16), np.float32)
        weight = np.zeros((n.value, 16, 16, 16), np.float32)
        if n.value:
            self.ctx.check(self.ctx.lib.d2r_tsdf_read_voxels(self.h, C.byref(n), _lib.ptr(coords), _lib.ptr(tsdf), _lib.ptr(weight)))
        return coords, tsdf, weight

    def extract(self, weight_threshold: float = TSDF_WEIGHT_THRESHOLD, crop=None, cluster_keep: float = TSDF_CLUSTER_KEEP) -> dict:
        """-> vertices float32 [nv,3], triangles uint32 [nt,3] (all that survive the crop), clusters int32 [nt], keep bool
        [nt] (False: in a cluster below cluster_keep of the largest), centre float64 [3]."""
        c = None if crop is None else np.ascontiguousarray(np.asarray(_np(crop), np.float64).reshape(6), np.float32)
        nv, nt = C.c_uint32(0), C.c_uint32(0)
        args = (self.h, weight_threshold, _lib.ptr(c), cluster_keep, C.byref(nv), C.byref(nt))
        self.ctx.check(self.ctx.lib.d2r_tsdf_extract(*args, None, None, None, None, None))
        v = np.zeros((nv.value, 3), np.float32)
        t = np.zeros((nt.value, 3), np.uint32)
        lab = np.zeros(nt.value, np.int32)
        keep = np.zeros(nt.value, np.uint8)
        centre = np.zeros(3, np.float64)
        self.ctx.check(self.ctx.lib.d2r_tsdf_extract(*args, _lib.ptr(v), _lib.ptr(t), _lib.ptr(lab), _lib.ptr(keep), _lib.ptr(centre)))
        return dict(vertices=v, triangles=t, clusters=lab, keep=keep.astype(bool), centre=centre)


    def grid(self):
        """-> (b0 int32 [3] first block per axis, nv uint32 [3] voxels per axis (x, y, z), voxel, trunc)."""
        b0, nv = np.zeros(3, np.int32), np.zeros(3, np.uint32)
        voxel, trunc = C.c_float(0), C.c_float(0)
        self.ctx.check(self.ctx.lib.d2r_tsdf_grid(self.h, _lib.ptr(b0), _lib.ptr(nv), C.byref(voxel), C.byref(trunc)))
        return b0, nv, np.float32(voxel.value), np.float32(trunc.value)

    def touch_bits(self, weight_threshold: float = TSDF_WEIGHT_THRESHOLD, contact: float = SDF_CONTACT) -> np.ndarray:
        """-> uint32 [nz, ny, ceil(nx / 32)]: bit x & 31 of word x >> 5 = the voxel is observed and within `contact` of the
        surface or behind it."""
        nx, ny, nz = (int(v) for v in self.grid()[1])
        words = np.zeros((nz, ny, (nx + 31) // 32), np.uint32)
        self.ctx.check(self.ctx.lib.d2r_tsdf_touch_bits(self.h, weight_threshold, contact, _lib.ptr(words)))
        return words

    def solid_points(self, weight_threshold: float = TSDF_WEIGHT_THRESHOLD) -> np.ndarray:
        """-> float32 [n, 3]: the centres of the observed solid voxels (weight >= threshold, tsdf <= 0) in (z, y, x) order."""
        n = C.c_uint32(0)
        self.ctx.check(self.ctx.lib.d2r_tsdf_solid_points(self.h, weight_threshold, C.byref(n), None))
        xyz = np.zeros((n.value, 3), np.float32)
        self.ctx.check(self.ctx.lib.d2r_tsdf_solid_points(self.h, weight_threshold, C.byref(n), _lib.ptr(xyz)))
        return xyz


PHYS_BACKENDS = ("hulls", "tsdf")


def vhacd_convexify(concave_path: str, convex_path: str, obj_id: int):
    """The reference's VHACD call (:185-193) through PyBullet, when PyBullet is installed.  Nothing is downloaded."""
    try:
        import pybullet as p
    except ImportError as e:
        raise RuntimeError("get_phys_models: mesh_{id}.obj comes from VHACD, which needs PyBullet (pybullet.vhacd), and PyBullet is "
                           "not importable here; install it, or pass convexify=callable(concave_path, convex_path, obj_id)") from e
    log = os.path.join(os.path.dirname(convex_path), f"mesh_vhacd_{obj_id}.log")
    p.vhacd(concave_path, convex_path, log, resolution=1000000 if obj_id == 0 else 10000, depth=80, concavity=0.00002, gamma=0.00002,
            minVolumePerCH=0.00002, maxNumVerticesPerCH=64)


def get_phys_models(depths, cam_poses, intrinsics, masks, num_objs, scene_bounds, embodied=False, save_dir=None, vis=False,
                    use_cache=True, use_phys_tsdf=False, use_vis_pcds=False, single_view_idx=0, *, ctx=None, convexify=None,
                    phys_backend="hulls"):
    """reference vision_3d/physics_utils.py:25-229 -> (mesh_paths, init_poses): per object id the path of mesh_{id}.obj and
    its initial pose (float32 4x4 tensor: identity with the mesh centre as translation).

    use_cache: read <save_dir>/mesh_{id}.obj and init_pose_{id}.txt (:28-50).  Otherwise, with use_phys_tsdf, fuse the masked
    frames on the GPU, write mesh_concave_{id}.obj and init_pose_{id}.txt, and hand the concave mesh
    to `convexify(concave_path, convex_path, obj_id)` (default: PyBullet's VHACD with the reference's arguments).  The
    Poisson branch (use_phys_tsdf=False) is not built.  `vis` (an Open3D window) and `embodied` (PyBullet's connection)
    are accepted and ignored.  `ctx`: an engine.Context (default: a fresh one on device 0).

    phys_backend="tsdf" (DESIGN.md section 2e): fuse and write mesh_concave_{id}.obj and init_pose_{id}.txt as above, skip
    `convexify`, write sdf_{id}.npz (save_sdf_model) from the same volume and return those paths; with use_cache the
    sdf_{id}.npz paths are returned."""
    import torch
    if phys_backend not in PHYS_BACKENDS:
        raise ValueError(f"get_phys_models: phys_backend must be one of {PHYS_BACKENDS}, got {phys_backend!r}")
    model_name = "sdf_{}.npz" if phys_backend == "tsdf" else "mesh_{}.obj"
    if use_cache:
        mesh_paths, init_poses = [], []
        for obj_id in range(num_objs):
            mesh_paths.append(os.path.join(save_dir, model_name.format(obj_id)))
            init_poses.append(torch.tensor(np.loadtxt(f"{save_dir}/init_pose_{obj_id}.txt")).float())
        return mesh_paths, init_poses
    if not use_phys_tsdf:
        raise NotImplementedError("get_phys_models: the Poisson branch (use_phys_tsdf=False: per-frame point clouds, statistical outlier "
                                  "removal, Poisson reconstruction) is not implemented; set use_phys_tsdf=True")
    if save_dir is None:
        raise ValueError("get_phys_models: save_dir is needed, the result is the paths of the mesh files")
    os.makedirs(save_dir, exist_ok=True)
    convexify = convexify or vhacd_convexify
    own_ctx = ctx is None
    if own_ctx:
        from . import engine
        ctx = engine.Context(0)
    bounds = np.asarray(_np(scene_bounds), np.float64).reshape(2, 3)
    frame_range = [single_view_idx] * 4 if use_vis_pcds else range(len(depths))
    mesh_paths, init_poses = [], []
    try:
        for obj_id in range(num_objs):
            vol = TsdfVolume(ctx, bounds)
            try:
                for f in frame_range:
                    depth = _np(depths[f])
                    u16 = (depth * 1000).astype(np.uint16)                      # the reference's expression, in the array's own type (:88)
                    vol.integrate(u16, _np(masks[f]) == obj_id, intrinsics, cam_poses[f], ERODE_BACKGROUND if obj_id == 0 else ERODE_OBJECT)
                try:
                    mesh = vol.extract(TSDF_WEIGHT_THRESHOLD, bounds, TSDF_CLUSTER_KEEP)
                except _lib.D2RError as e:
                    raise ValueError(f"get_phys_models: object {obj_id} has no TSDF surface inside scene_bounds ({e})") from e
                if phys_backend == "tsdf":
                    field = (vol.grid(), TSDF_WEIGHT_THRESHOLD, SDF_CONTACT, vol.touch_bits(TSDF_WEIGHT_THRESHOLD, SDF_CONTACT),
                             vol.solid_points(TSDF_WEIGHT_THRESHOLD))
            finally:
                vol.close()
            init_pose = torch.eye(4)
            init_pose[:3, 3] = torch.tensor(mesh["centre"])
            init_poses.append(init_pose)
            _lib.savetxt(os.path.join(save_dir, f"init_pose_{obj_id}.txt"), init_pose.numpy())
            concave = os.path.join(save_dir, f"mesh_concave_{obj_id}.obj")
            _lib.obj_write(concave, mesh["vertices"], mesh["triangles"], mesh["keep"])
            if phys_backend == "tsdf":
                model = os.path.join(save_dir, model_name.format(obj_id))
                save_sdf_model(model, *field)
            else:
                model = os.path.join(save_dir, f"mesh_{obj_id}.obj")
                convexify(concave, model, obj_id)
            mesh_paths.append(model)
    finally:
        if own_ctx:
            ctx.close()
    return mesh_paths, init_poses


def create_lazy_phys_mods(scene_model, movable_obj, scene_bounds, save_dir, embodied=False, vis=False, use_cache=False, use_phys_tsdf=True,
                          use_vis_pcds=False, single_view_idx=0, *, ctx=None, convexify=None, phys_backend="hulls"):
    """reference scene_model.py:116-125 (TaskModel.create_lazy_phys_mods): two physics models, the movable object (mask 1)
    and everything else (mask 0) -> ([bground_phys, movable_phys], [bground_init_pose, movable_init_pose])."""
    fg_bg_masks = [(_np(m) == movable_obj.mask_idx).astype(np.uint8) for m in scene_model.masks]
    return get_phys_models(scene_model.depths, scene_model.opt_cam_poses, scene_model.intrinsics, fg_bg_masks, num_objs=2,
                           scene_bounds=scene_bounds, embodied=embodied, save_dir=save_dir, vis=vis, use_cache=use_cache,
                           use_phys_tsdf=use_phys_tsdf, use_vis_pcds=use_vis_pcds, single_view_idx=single_view_idx, ctx=ctx, convexify=convexify,
                           phys_backend=phys_backend)
