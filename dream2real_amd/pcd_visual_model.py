"""The point-cloud ablation (`use_vis_pcds`, configs/*/pcd.json): reference vision_3d/pcd_visual_model.py.

`get_vis_pcds` builds the coloured clouds from the masked RGB-D frames (host numpy, once per task) and reads / writes
their `obj_vis_{id}.pcd` cache; `PointCloudRenderer` renders one frame per candidate pose of the movable object on the
GPU (pcd.hip) — the render rule is DESIGN.md section 2, a written restatement of what the reference asks Open3D's
Filament renderer for — and `render_score` feeds the frames straight into the vision tower (d2r_pcd_render_score_host).

PCD files are read and written here on the host: DATA ascii, binary and binary_compressed (LZF) with any FIELDS /
SIZE / TYPE / COUNT layout that carries x y z and a packed rgb / rgba float or r g b uchar fields.  The writer writes
what open3d.io.write_point_cloud writes by default as far as it is known here: DATA binary, FIELDS x y z rgb, F 4 each
(believed: not checked against a file Open3D wrote).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

import numpy as np

from . import _lib
from .combined_rendering import INTRINSICS_CLIP_VIEW

POINT_SIZE = 3.0            # reference pcd_visual_model.py:107 (MaterialRecord.point_size)
NEAR = 0.01                 # believed: points nearer than this (camera z, metres) are culled
FRAME_VOXEL_SIZE = 0.002    # reference :47 (multi-view clouds)
ERODE_SIZE = 15             # reference :64 (15 x 15 rectangle)


@dataclasses.dataclass(eq=False)
class PointCloud:
    """A coloured point cloud on the host: xyz float32 [N,3], rgb uint8 [N,3].  The renderer uploads it on first use,
    keyed by identity: a cloud is not expected to change after it has been rendered."""
    xyz: np.ndarray
    rgb: np.ndarray

    def __post_init__(self):
        self.xyz = np.ascontiguousarray(np.asarray(self.xyz, np.float32).reshape(-1, 3))
        self.rgb = np.ascontiguousarray(np.asarray(self.rgb, np.uint8).reshape(-1, 3))
        if self.xyz.shape[0] != self.rgb.shape[0]:
            raise ValueError(f"{self.xyz.shape[0]} points but {self.rgb.shape[0]} colours")

    def __len__(self):
        return self.xyz.shape[0]


# ---------------------------------------------------------------------------------------------------- PCD files

_NP_TYPES = {("F", 4): np.float32, ("F", 8): np.float64, ("U", 1): np.uint8, ("U", 2): np.uint16, ("U", 4): np.uint32,
             ("U", 8): np.uint64, ("I", 1): np.int8, ("I", 2): np.int16, ("I", 4): np.int32, ("I", 8): np.int64}


def lzf_decompress(src: bytes, out_len: int) -> bytes:
    """LZF (liblzf lzf_decompress), the codec of DATA binary_compressed."""
    out = bytearray(out_len)
    i = o = 0
    n = len(src)
    while i < n:
        ctrl = src[i]
        i += 1
        if ctrl < 32:                                  # literal run of ctrl + 1 bytes
            ln = ctrl + 1
            if i + ln > n or o + ln > out_len:
                raise ValueError("corrupt LZF data (literal run past the end)")
            out[o:o + ln] = src[i:i + ln]
            i += ln
            o += ln
            continue
        ln = ctrl >> 5                                 # back reference
        if ln == 7:
            if i >= n:
                raise ValueError("corrupt LZF data (truncated length)")
            ln += src[i]
            i += 1
        if i >= n:
            raise ValueError("corrupt LZF data (truncated offset)")
        ref = o - ((ctrl & 0x1F) << 8) - src[i] - 1
        i += 1
        ln += 2
        if ref < 0 or o + ln > out_len:
            raise ValueError("corrupt LZF data (reference out of range)")
        if ref + ln <= o:
            out[o:o + ln] = out[ref:ref + ln]
        else:                                          # overlapping copy: byte by byte
            for k in range(ln):
                out[o + k] = out[ref + k]
        o += ln
    if o != out_len:
        raise ValueError(f"corrupt LZF data ({o} bytes decoded, {out_len} expected)")
    return bytes(out)


def lzf_compress(src: bytes) -> bytes:
    """A valid LZF stream for `src` (greedy matches of 3+ bytes through a hash of the last position of each 3-byte
    sequence; liblzf's encoder may choose other matches — any valid stream decodes to the same bytes)."""
    out = bytearray()
    lit = bytearray()
    last = {}
    i, n = 0, len(src)

    def flush():
        for k in range(0, len(lit), 32):
            chunk = lit[k:k + 32]
            out.append(len(chunk) - 1)
            out.extend(chunk)
        lit.clear()

    while i < n:
        ref = last.get(src[i:i + 3]) if i + 3 <= n else None
        if i + 3 <= n:
            last[src[i:i + 3]] = i
        if ref is not None and i - ref - 1 < 8192:
            ln = 3
            while i + ln < n and ln < 264 and src[ref + ln] == src[i + ln]:
                ln += 1
            flush()
            off = i - ref - 1
            if ln - 2 < 7:
                out.append(((ln - 2) << 5) | (off >> 8))
            else:
                out.append((7 << 5) | (off >> 8))
                out.append(ln - 2 - 7)
            out.append(off & 0xFF)
            for k in range(i + 1, min(i + ln, n - 2)):
                last[src[k:k + 3]] = k
            i += ln
        else:
            lit.append(src[i])
            i += 1
    flush()
    return bytes(out)


def _parse_header(f, path):
    hdr = {}
    while True:
        line = f.readline()
        if not line:
            raise ValueError(f"{path}: PCD header ends before DATA")
        s = line.decode("ascii", "replace").strip()
        if not s or s.startswith("#"):
            continue
        key, _, rest = s.partition(" ")
        hdr[key.upper()] = rest.split()
        if key.upper() == "DATA":
            return hdr


def read_point_cloud(path: str) -> PointCloud:
    """A .pcd file -> PointCloud (o3d.io.read_point_cloud for the files this path reads)."""
    with open(path, "rb") as f:
        hdr = _parse_header(f, path)
        body = f.read()
    for key in ("FIELDS", "SIZE", "TYPE"):
        if key not in hdr:
            raise ValueError(f"{path}: PCD header has no {key}")
    fields = hdr["FIELDS"]
    sizes = [int(x) for x in hdr["SIZE"]]
    types = [t.upper() for t in hdr["TYPE"]]
    counts = [int(x) for x in hdr.get("COUNT", ["1"] * len(fields))]
    if not (len(fields) == len(sizes) == len(types) == len(counts)):
        raise ValueError(f"{path}: FIELDS, SIZE, TYPE and COUNT differ in length")
    for f_, s_, t_ in zip(fields, sizes, types):
        if (t_, s_) not in _NP_TYPES:
            raise ValueError(f"{path}: field {f_!r} has an unsupported TYPE {t_} / SIZE {s_}")
    if "POINTS" in hdr:
        n = int(hdr["POINTS"][0])
    elif "WIDTH" in hdr:
        n = int(hdr["WIDTH"][0]) * int(hdr.get("HEIGHT", ["1"])[0])
    else:
        raise ValueError(f"{path}: PCD header has no POINTS")
    data = hdr["DATA"][0].lower() if hdr["DATA"] else ""
    names = [f_ if c == 1 else f"{f_}__{k}" for f_, c in zip(fields, counts) for k in range(c)]
    dts = [np.dtype(_NP_TYPES[(t_, s_)]).newbyteorder("<") for t_, s_, c in zip(types, sizes, counts) for _ in range(c)]
    cols = {}
    if data == "ascii":
        text = body.decode("ascii", "replace").split()
        vals = np.array(text[:n * len(names)], dtype=object).reshape(n, len(names)) if n else np.empty((0, len(names)), object)
        if len(text) < n * len(names):
            raise ValueError(f"{path}: DATA ascii holds fewer than {n} points")
        for k, (nm, dt) in enumerate(zip(names, dts)):
            cols[nm] = np.array([float(v) for v in vals[:, k]], np.float64).astype(dt) if dt.kind == "f" else \
                np.array([int(float(v)) for v in vals[:, k]], np.int64).astype(dt)
    elif data == "binary":
        rec = np.dtype([(nm, dt) for nm, dt in zip(names, dts)])
        if len(body) < n * rec.itemsize:
            raise ValueError(f"{path}: DATA binary holds fewer than {n} points")
        arr = np.frombuffer(body, rec, count=n)
        cols = {nm: arr[nm] for nm in names}
    elif data == "binary_compressed":
        if len(body) < 8:
            raise ValueError(f"{path}: DATA binary_compressed has no size words")
        csize, usize = np.frombuffer(body[:8], "<u4")
        raw = lzf_decompress(body[8:8 + int(csize)], int(usize))
        off = 0
        for nm, dt in zip(names, dts):                 # field-major: all points of one field, then the next
            nb = n * dt.itemsize
            if off + nb > len(raw):
                raise ValueError(f"{path}: DATA binary_compressed holds fewer than {n} points")
            cols[nm] = np.frombuffer(raw[off:off + nb], dt)
            off += nb
    else:
        raise ValueError(f"{path}: unsupported PCD DATA {data!r} (ascii, binary or binary_compressed)")
    for k in ("x", "y", "z"):
        if k not in cols:
            raise ValueError(f"{path}: PCD file has no field {k!r}")
    xyz = np.stack([cols["x"], cols["y"], cols["z"]], 1).astype(np.float32)
    packed = next((k for k in ("rgb", "rgba") if k in cols), None)
    if packed is not None:
        v = np.ascontiguousarray(cols[packed])
        if v.dtype.itemsize != 4:
            raise ValueError(f"{path}: field {packed!r} must be 4 bytes wide")
        u = v.view(np.uint32)
        rgb = np.stack([(u >> 16) & 255, (u >> 8) & 255, u & 255], 1).astype(np.uint8)
    elif all(k in cols for k in ("r", "g", "b")):
        rgb = np.stack([cols["r"], cols["g"], cols["b"]], 1).astype(np.uint8)
    else:
        raise ValueError(f"{path}: PCD file has no colour (a field 'rgb', 'rgba' or 'r' 'g' 'b'): the point-cloud "
                         "renderer needs coloured clouds")
    return PointCloud(xyz, rgb)


def write_point_cloud(path: str, pcd: PointCloud, data: str = "binary"):
    """PointCloud -> .pcd file: FIELDS x y z rgb, F 4 each, rgb packed as (r << 16 | g << 8 | b) in a float's bits —
    believed to be o3d.io.write_point_cloud's default layout (DATA binary).  data = ascii / binary / binary_compressed."""
    n = len(pcd)
    rgb = pcd.rgb.astype(np.uint32)
    packed = ((rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]).astype("<u4").view("<f4")
    hdr = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\n"
           f"COUNT 1 1 1 1\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA {data}\n").encode()
    xyz = pcd.xyz.astype("<f4")
    if data == "ascii":
        u = packed.view("<u4")
        body = "".join(f"{x!r} {y!r} {z!r} {int(c)}\n" for (x, y, z), c in zip(xyz.tolist(), u.tolist())).encode()
        # the packed colour as its integer bits: a reader interprets rgb through its 4 bytes (F or U)
        hdr = hdr.replace(b"TYPE F F F F", b"TYPE F F F U")
    elif data == "binary":
        rec = np.empty(n, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgb", "<f4")]))
        rec["x"], rec["y"], rec["z"], rec["rgb"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], packed
        body = rec.tobytes()
    elif data == "binary_compressed":
        raw = b"".join(np.ascontiguousarray(a).tobytes() for a in (xyz[:, 0], xyz[:, 1], xyz[:, 2], packed))
        comp = lzf_compress(raw)
        body = np.array([len(comp), len(raw)], "<u4").tobytes() + comp
    else:
        raise ValueError(f"unsupported PCD DATA {data!r}")
    with open(path, "wb") as f:
        f.write(hdr + body)


# ---------------------------------------------------------------------------------------------------- cloud building

def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def erode_rect(mask: np.ndarray, size: int = ERODE_SIZE) -> np.ndarray:
    """cv2.erode(mask, np.ones((size, size)), iterations=1) of a 0/1 mask: the minimum over a size x size window
    anchored at its centre; outside the frame counts as 1 (cv2's default border value for erosion), so the frame
    border itself does not erode."""
    m = np.asarray(mask).astype(bool)
    r = size // 2
    p = np.pad(m, ((r, size - 1 - r), (0, 0)), constant_values=True)
    rows = np.lib.stride_tricks.sliding_window_view(p, size, axis=0).all(axis=-1)
    p = np.pad(rows, ((0, 0), (r, size - 1 - r)), constant_values=True)
    return np.lib.stride_tricks.sliding_window_view(p, size, axis=1).all(axis=-1)


def backproject(rgb, depth, cam_pose, intrinsics):
    """Open3D's create_from_rgbd_image (depth_scale 1000, depth_trunc 1000) for one masked frame: depth goes through
    (depth * 1000).astype(uint16), z = u16 / 1000; pixels with z > 0 in row-major order; x = (j - cx) z / fx,
    y = (i - cy) z / fy; world = cam_pose (x, y, z, 1), fp64.  -> (xyz float64 [M,3], rgb uint8 [M,3])."""
    d16 = (np.asarray(depth, np.float32) * 1000).astype(np.uint16)
    z_img = (d16 / np.float32(1000)).astype(np.float32)
    K = np.asarray(intrinsics, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ii, jj = np.nonzero(z_img > 0)                     # row-major order
    z = z_img[ii, jj].astype(np.float64)
    x = (jj - cx) * z / fx
    y = (ii - cy) * z / fy
    T = np.asarray(cam_pose, np.float64)
    pts = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)
    return pts, np.asarray(rgb)[ii, jj].astype(np.uint8)


def crop(xyz, rgb, bounds):
    """AxisAlignedBoundingBox(min_bound, max_bound) crop: inclusive on both ends."""
    lo, hi = np.asarray(bounds[0], np.float64), np.asarray(bounds[1], np.float64)
    keep = np.all((xyz >= lo) & (xyz <= hi), axis=1)
    return xyz[keep], rgb[keep]


def voxel_down_sample(xyz, rgb, voxel: float):
    """voxel_down_sample: voxel index floor((p - (min(p) - voxel / 2)) / voxel); each occupied voxel becomes the mean of
    its points and of their colours (rounded half up).  Voxels are emitted in sorted (ix, iy, iz) order — Open3D emits
    them in its hash map's order, which is not specified."""
    if xyz.shape[0] == 0:
        return xyz, rgb
    origin = xyz.min(axis=0) - voxel * 0.5
    idx = np.floor((xyz - origin) / voxel).astype(np.int64)
    keys, inv = np.unique(idx, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv, minlength=keys.shape[0]).astype(np.float64)
    mean = np.stack([np.bincount(inv, xyz[:, k], keys.shape[0]) for k in range(3)], 1) / cnt[:, None]
    col = np.stack([np.bincount(inv, rgb[:, k].astype(np.float64), keys.shape[0]) for k in range(3)], 1) / cnt[:, None]
    return mean, np.floor(col + 0.5).astype(np.uint8)


def _get_vis_pcds_device(ctx, rgbs, depths, cam_poses, intrinsics, masks, num_objs, scene_bounds, views, voxel):
    """The clouds of get_vis_pcds from one d2r_pcd_build call (pcdbuild.hip): the frames stacked once, every object at once."""
    labels = np.stack([_np(m) for m in masks])
    if labels.size and (labels.min() < 0 or labels.max() > 255):
        raise ValueError(f"the device path takes labels 0 .. 255, the masks hold {int(labels.min())} .. {int(labels.max())}")
    if num_objs > 256:
        raise ValueError(f"the device path takes object ids 0 .. 255, num_objs is {num_objs}")
    d16 = np.stack([(_np(d).astype(np.float32) * 1000).astype(np.uint16) for d in depths])
    rgb = np.stack([_np(c).astype(np.uint8) for c in rgbs])
    poses = np.stack([np.asarray(_np(T), np.float64) for T in cam_poses])
    handles = _lib.pcd_build(ctx, rgb, d16, labels.astype(np.uint8), poses, intrinsics, scene_bounds, voxel, list(views),
                             list(range(num_objs)))
    try:
        return [PointCloud(*_lib.pcd_read(ctx, h)) for h in handles]
    finally:
        for h in handles:
            _lib.load().d2r_pcd_destroy(h)


def get_vis_pcds(rgbs, depths, cam_poses, intrinsics, masks, num_objs, scene_bounds, save_dir=None, vis=False,
                 use_cache=True, pcds_type=1, single_view_idx=0, *, ctx=None):
    """reference vision_3d/pcd_visual_model.py:18-95: one PointCloud per object id (0 .. num_objs - 1) from the masked
    RGB-D frames, or read from <save_dir>/obj_vis_{id}.pcd with use_cache.  pcds_type 0: the view single_view_idx alone;
    1: every view, each voxel-downsampled at 0.002 before they are concatenated.  `vis` (an Open3D window) is ignored.
    With `ctx` (an engine.Context or a d2r_ctx pointer) the clouds are built on the GPU by one d2r_pcd_build call, bit for bit
    the ones the host path below gives; without it they are built here in numpy."""
    if use_cache:
        return [read_point_cloud(os.path.join(save_dir, f"obj_vis_{obj_id}.pcd")) for obj_id in range(num_objs)]
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
    views = range(len(depths)) if pcds_type == 1 else [single_view_idx]
    if ctx is not None:
        out = _get_vis_pcds_device(ctx, rgbs, depths, cam_poses, intrinsics, masks, num_objs, scene_bounds, views,
                                   FRAME_VOXEL_SIZE if pcds_type == 1 else 0.0)
        if save_dir is not None:
            for obj_id, pcd in enumerate(out):
                write_point_cloud(os.path.join(save_dir, f"obj_vis_{obj_id}.pcd"), pcd)
        return out
    out = []
    for obj_id in range(num_objs):
        parts_xyz, parts_rgb = [], []
        for v in views:
            depth = _np(depths[v]).astype(np.float32).copy()
            rgb = _np(rgbs[v]).copy()
            mask = erode_rect(_np(masks[v]) == obj_id)
            depth[~mask] = 0
            rgb[~mask] = 0
            xyz, col = backproject(rgb.astype(np.uint8), depth, _np(cam_poses[v]), intrinsics)
            xyz, col = crop(xyz, col, scene_bounds)
            if pcds_type == 1:
                xyz, col = voxel_down_sample(xyz, col, FRAME_VOXEL_SIZE)
            parts_xyz.append(xyz)
            parts_rgb.append(col)
        pcd = PointCloud(np.concatenate(parts_xyz, 0) if parts_xyz else np.zeros((0, 3)),
                         np.concatenate(parts_rgb, 0) if parts_rgb else np.zeros((0, 3), np.uint8))
        out.append(pcd)
        if save_dir is not None:
            write_point_cloud(os.path.join(save_dir, f"obj_vis_{obj_id}.pcd"), pcd)
    return out


# ---------------------------------------------------------------------------------------------------- renderer

def _poses16(poses) -> np.ndarray:
    return np.ascontiguousarray(_np(poses).reshape(-1, 16), np.float32)


class PointCloudRenderer:
    """reference vision_3d/pcd_visual_model.py:98-155 on the MI355X: renders the task's background cloud plus the
    movable cloud at each candidate pose, 336 x 336 through INTRINSICS_CLIP_VIEW by default."""

    point_cloud = True          # optimise_pose_grid takes its use_vis_pcds branch with this renderer

    def __init__(self, ctx, width: int = 336, height: int = 336, intrinsics=INTRINSICS_CLIP_VIEW,
                 point_size: float = POINT_SIZE, near: float = NEAR):
        K = np.asarray(intrinsics, np.float64)
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.view = _lib.PcdView(self.width, self.height, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]),
                                 float(point_size), float(near))
        self._uploads = {}      # id(PointCloud) -> (the cloud, device handle)

    def _handle(self, pcd: PointCloud):
        if not isinstance(pcd, PointCloud):
            raise TypeError(f"the point-cloud renderer needs pcd_visual_model.PointCloud visual models, got {type(pcd).__name__}")
        hit = self._uploads.get(id(pcd))
        if hit is not None and hit[0] is pcd:
            return hit[1]
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.d2r_pcd_create(self.ctx.h, _lib.ptr(pcd.xyz), _lib.ptr(pcd.rgb), len(pcd), C.byref(h)))
        self._uploads[id(pcd)] = (pcd, h)
        return h

    def _args(self, render_pose, pose_batch, task_model):
        bg = self._handle(task_model.task_bground_obj.vis_model)
        mv = self._handle(task_model.movable_obj.vis_model)
        cam = np.ascontiguousarray(_np(render_pose).reshape(16), np.float32)
        now = np.ascontiguousarray(_np(task_model.movable_obj.pose).reshape(16), np.float32)
        return bg, mv, cam, now, _poses16(pose_batch)

    def render(self, render_pose, pose_batch, task_model, hide_movable=False):
        """-> list of uint8 [H,W,3], one per pose of pose_batch ([K,16] or [K,4,4]); render_pose is the OpenCV
        camera-to-world pose (not converted to NGP)."""
        if hide_movable:
            raise NotImplementedError("hide_movable=True is not implemented (nor is it in the reference)")
        bg, mv, cam, now, poses = self._args(render_pose, pose_batch, task_model)
        K = poses.shape[0]
        frames = np.empty((K, self.height, self.width, 3), np.uint8)
        self.ctx.check(self.ctx.lib.d2r_pcd_render(self.ctx.h, bg, mv, C.byref(self.view), _lib.ptr(cam), _lib.ptr(now),
                                                   _lib.ptr(poses), K, _lib.ptr(frames)))
        return list(frames)

    def render_score(self, render_pose, pose_batch, task_model, scorer, text_embeds, return_frames: bool = False):
        """The fused call (d2r_pcd_render_score_host): frames rendered and scored on the GPU -> logits [K,C] (and the
        frames uint8 [K,H,W,3] with return_frames).  Equal to scorer.score_frames(render(...), rot90=True)."""
        bg, mv, cam, now, poses = self._args(render_pose, pose_batch, task_model)
        K = poses.shape[0]
        t = np.ascontiguousarray(text_embeds, np.float32)
        logits = np.empty((K, t.shape[0]), np.float32)
        frames = np.empty((K, self.height, self.width, 3), np.uint8) if return_frames else None
        if K:
            self.ctx.check(self.ctx.lib.d2r_pcd_render_score_host(
                self.ctx.h, bg, mv, scorer.h, C.byref(self.view), _lib.ptr(cam), _lib.ptr(now), _lib.ptr(poses), K,
                _lib.ptr(t), t.shape[0], scorer.logit_scale, _lib.ptr(logits), _lib.ptr(frames)))
        return (logits, frames) if return_frames else logits

    def close(self):
        for _, h in self._uploads.values():
            self.ctx.lib.d2r_pcd_destroy(h)
        self._uploads = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
