"""The geometric half of the reference's segmentation stage (segmentation/XMem_infer.py:213-236, 264-351) on the GPU: connected
components of a raw label image, the area rule, the component nearest the scene centre (duplicate_prune) or the largest
(disconnected_prune), the out-of-scene overwrite, and the XMem_masks/rgb_%04d.png files everything downstream reads.  The rule
is DESIGN.md section 2d.

Running SAM or XMem is out of scope: `proposals_to_labels` turns the mask generator's proposals into the first frame's label
image (sam_seg.py:80-115 and integrate_masks); whatever produced the raw label images of all frames (XMem in
the reference), `refine_masks` is the body of the `segment_associate` loop from there on and `load_cached_masks` its cache branch.
`track_labels` is this package's own way from the first label image to all of them: by geometry, on the GPU,
and `propose_masks` its own way to the proposals on a table-top scene: what stands above the support plane in the first frame's
depth."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

MIN_COMPONENT_AREA = 200          # XMem_infer.py:289, :340
PROPOSAL_RECORD = np.dtype([(k, np.uint32) for k in ("area", "ncomp", "stage", "label", "boundary", "ew", "eh", "dd")])


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def depth_to_u16(depth):
    """The reference's (depth * 1000).astype(np.uint16) on its fp16-metre depth, the product in float16; uint16 input is
    taken as millimetres already."""
    d = _np(depth)
    if d.dtype == np.uint16:
        return np.ascontiguousarray(d)
    with np.errstate(over="ignore"):
        return (d.astype(np.float16) * np.float16(1000)).astype(np.uint16)


def duplicate_prune(mask, depth, T_WC, intrinsics, scene_centre, *, ctx):
    """reference XMem_infer.py:264-316: per label keep the component (area >= 200 when there are several) whose mean 3-D point is
    nearest the scene centre.  mask uint8 [H,W], depth fp16 metres [H,W] -> uint8 [H,W]."""
    m = _np(mask).astype(np.uint8)
    return _lib.masks_prune(ctx, 0, m[None], depth_to_u16(depth)[None], None, _np(T_WC).reshape(1, 16), _np(intrinsics), _np(scene_centre),
                            MIN_COMPONENT_AREA)[0]


def disconnected_prune(mask, *, ctx):
    """reference XMem_infer.py:318-351: per label keep the largest component (area >= 200 when there are several)."""
    return _lib.masks_prune(ctx, 1, _np(mask).astype(np.uint8)[None], min_area=MIN_COMPONENT_AREA)[0]


def refine_masks(raw_masks, depths, T_WC, intrinsics, out_scene_bound_masks, scene_centre, out_dir, *, ctx):
    """The batched body of segment_associate's loop (:213-236) for the associated frames: duplicate_prune of every raw label image,
    255 where the scene-bound mask is 255, written to <out_dir>/XMem_masks/rgb_%04d.png.  One GPU call for all frames.
    -> uint8 [N,H,W]."""
    m = _np(raw_masks).astype(np.uint8)
    oob = None if out_scene_bound_masks is None else _np(out_scene_bound_masks).astype(np.uint8)
    refined = _lib.masks_prune(ctx, 0, m, depth_to_u16(depths), oob, _np(T_WC).reshape(-1, 16), _np(intrinsics), _np(scene_centre),
                               MIN_COMPONENT_AREA)
    if out_dir is not None:
        mask_dir = os.path.join(out_dir, "XMem_masks")
        os.makedirs(mask_dir, exist_ok=True)
        for k in range(refined.shape[0]):
            _lib.png_write_channels(refined[k], os.path.join(mask_dir, "rgb_%04d.png" % k))
    return refined


def proposals_to_labels(proposals, inside=None, *, ctx, return_records=False):
    """The reference's Segmentor.segment after the mask generator (segmentation/sam_seg.py:80-115) and integrate_masks
    (XMem_infer.py:256-261) in one GPU call: proposals bool [M,H,W] in the proposer's order, inside bool [H,W] (True inside the
    scene bounds) or None -> the label image uint8 [H,W], survivors numbered 1, 2, ... in proposal order, the highest label on top.
    The rule is DESIGN.md section 2h.  With return_records also one record per proposal: area, ncomp, stage (0 kept, 1 disconnected,
    2 large, 3 subpart, 4 small), label, boundary, ew, eh, dd."""
    p = _np(proposals)
    if p.ndim != 3:
        raise ValueError(f"proposals must be [M, H, W], got shape {p.shape}")
    if p.shape[0] > _lib.PROP_MAX:
        raise ValueError(f"at most {_lib.PROP_MAX} proposals per call, got {p.shape[0]}")
    if p.shape[1] == 0 or p.shape[2] == 0:
        raise ValueError(f"proposals must have a height and a width, got shape {p.shape}")
    s = None
    if inside is not None:
        s = _np(inside)
        if s.shape != p.shape[1:]:
            raise ValueError(f"inside must be [H, W] = {tuple(p.shape[1:])}, got shape {s.shape}")
        s = (s != 0).astype(np.uint8)
    out = _lib.proposals_labels(ctx, (p != 0).astype(np.uint8), s, records=return_records)
    if not return_records:
        return out
    labels, recs = out
    return labels, np.ascontiguousarray(recs).view(PROPOSAL_RECORD).reshape(-1)


# the mirror of include/d2r.h's d2r_labeltrack_params (tests/test_labeltrack_host.py holds its layout to a C compiler's)
class LabeltrackParams(C.Structure):
    _fields_ = [("voxel", C.c_float), ("band_voxels", C.c_uint32), ("tau_mm", C.c_uint32), ("grow", C.c_uint32)]


def _labeltrack_bounds(scene_bounds):
    b = np.ascontiguousarray(np.asarray(_np(scene_bounds), np.float64).reshape(-1))
    if b.size != 6:
        raise ValueError(f"scene_bounds must be [[min xyz], [max xyz]], got {b.size} numbers")
    return b


def labeltrack_grid(scene_bounds, voxel=0.004, band_voxels=2):
    """d2r_labeltrack_grid (host only): the grid track_labels lays over scene_bounds -> (dims uint32 [3] along x, y, z, lo int32 [3])."""
    params = LabeltrackParams(float(voxel), int(band_voxels), 0, 0)
    dims, lo = np.zeros(3, np.uint32), np.zeros(3, np.int32)
    _lib.check(_lib.load().d2r_labeltrack_grid(_lib.ptr(_labeltrack_bounds(scene_bounds)), C.byref(params), _lib.ptr(dims), _lib.ptr(lo)))
    return dims, lo


def track_labels(depths, cam_poses, intrinsics, labels0, scene_bounds, *, ctx, voxel=0.004, band_voxels=2, tau_mm=10, grow=64,
                 return_stats=False, return_volume=False):
    """The first frame's label image carried to every frame of a scan by geometry (d2r_labeltrack_scan): a
    voxel grid over scene_bounds holds a (label, count) pair per voxel; frame 0 votes labels0 into it; every later frame, in order,
    reads its labels from the grid, grows them along depth-continuous image paths (`grow` sweeps, a step of more than tau_mm
    millimetres is not crossed) and votes in turn.  depths [N,H,W] metres (or uint16 millimetres), cam_poses [N,4,4] camera to
    world, intrinsics [3,3], labels0 uint8 [H,W] without 255 -> uint8 [N,H,W], frame 0's being labels0; pixels the labels did not
    reach are 0.  return_stats: also uint32 [N,4] (known after the prediction, labelled by the fill, left unknown, fill launches that
    changed a pixel); return_volume: also (uint16 [nz,ny,nx] label | count << 8, dims, lo)."""
    d = depth_to_u16(np.stack([_np(x) for x in depths]) if isinstance(depths, (list, tuple)) else depths)
    if d.ndim != 3:
        raise ValueError(f"depths must be [N, H, W], got shape {d.shape}")
    n, h, w = d.shape
    T = np.ascontiguousarray(np.array([np.asarray(_np(p), np.float64).reshape(16) for p in cam_poses]), np.float32)
    if T.shape != (n, 16):
        raise ValueError(f"{T.shape[0]} poses for {n} frames")
    K = np.asarray(_np(intrinsics), np.float64).reshape(3, 3)
    K4 = np.ascontiguousarray([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float64)
    l0 = np.ascontiguousarray(_np(labels0), np.uint8)
    if l0.shape != (h, w):
        raise ValueError(f"labels0 must be [H, W] = {(h, w)}, got shape {l0.shape}")
    b = _labeltrack_bounds(scene_bounds)
    params = LabeltrackParams(float(voxel), int(band_voxels), int(tau_mm), int(grow))
    out = np.zeros((n, h, w), np.uint8)
    stats = np.zeros((n, 4), np.uint32) if return_stats else None
    vol = dims = lo = None
    if return_volume:
        dims, lo = labeltrack_grid(b, voxel, band_voxels)
        vol = np.zeros((int(dims[2]), int(dims[1]), int(dims[0])), np.uint16)
    ctx.check(ctx.lib.d2r_labeltrack_scan(ctx.h, _lib.ptr(b), C.byref(params), n, w, h, _lib.ptr(K4), _lib.ptr(d), _lib.ptr(T), _lib.ptr(l0),
                                          _lib.ptr(out), _lib.ptr(stats), _lib.ptr(vol), _lib.ptr(dims), _lib.ptr(lo)))
    res = (out,) + ((stats,) if return_stats else ()) + (((vol, dims, lo),) if return_volume else ())
    return res if len(res) > 1 else out


def labeltrack_timing(ctx):
    """d2r_labeltrack_get_timing -> (upload, kernels, download) of the context's last track_labels, device-event milliseconds."""
    ms = np.zeros(3, np.float64)
    ctx.check(ctx.lib.d2r_labeltrack_get_timing(ctx.h, _lib.ptr(ms)))
    return tuple(float(x) for x in ms)


# the mirror of include/d2r.h's d2r_geoprop_params (tests/test_geoprop_host.py holds its layout to a C compiler's)
class GeopropParams(C.Structure):
    _fields_ = [("window_mm", C.c_uint32), ("h_min_mm", C.c_uint32), ("tau_mm", C.c_uint32), ("min_area", C.c_uint32), ("max_props", C.c_uint32)]


GEOPROP_RECORD = np.dtype([(k, np.uint32) for k in ("root", "area", "i0", "j0", "i1", "j1")])
GEOPROP_PLANE = np.dtype([(k, np.int32) for k in ("bin", "count", "inside", "above", "components")])


def propose_masks(depth0, cam_pose, intrinsics, scene_bounds, *, ctx, up=(0.0, 0.0, 1.0), window_mm=5, h_min_mm=6, tau_mm=10,
                  min_area=MIN_COMPONENT_AREA, max_props=255, return_labels=False):
    """Mask proposals for a table-top scene from one depth frame, without a network (d2r_geoprop_masks): the
    support plane is the fullest window of window_mm height bins along `up` among the pixels whose points lie in scene_bounds; what
    stands h_min_mm or more above it, cut along depth steps of more than tau_mm millimetres into 4-connected pieces of at least
    min_area pixels, is the proposals, the max_props largest at the most, numbered by their first pixel in raster order.  depth0
    [H,W] metres (or uint16 millimetres) in sensor orientation, cam_pose [4,4] camera to world, intrinsics [3,3].
    -> (bool [M,H,W], records [M] of root, area, i0, j0, i1, j1, plane record of bin, count, inside, above, components);
    return_labels: also the uint16 [H,W] image of the proposals' numbers.  A frame without a pixel inside the bounds gives M = 0."""
    d = depth_to_u16(depth0)
    if d.ndim != 2:
        raise ValueError(f"depth0 must be [H, W], got shape {d.shape}")
    h, w = d.shape
    T = np.ascontiguousarray(np.asarray(_np(cam_pose), np.float64).reshape(-1), np.float32)
    if T.size != 16:
        raise ValueError(f"cam_pose must be [4, 4], got {T.size} numbers")
    K = np.asarray(_np(intrinsics), np.float64).reshape(3, 3)
    K4 = np.ascontiguousarray([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float64)
    b = _labeltrack_bounds(scene_bounds)
    u = np.ascontiguousarray(np.asarray(_np(up), np.float64).reshape(-1))
    if u.size != 3:
        raise ValueError(f"up must be a vector of 3, got {u.size} numbers")
    params = GeopropParams(int(window_mm), int(h_min_mm), int(tau_mm), int(min_area), int(max_props))
    labels = np.zeros((h, w), np.uint16)
    recs = np.zeros((max(int(max_props), 1), len(GEOPROP_RECORD.names)), np.uint32)
    m, plane = C.c_uint32(0), np.zeros(len(GEOPROP_PLANE.names), np.int32)
    ctx.check(ctx.lib.d2r_geoprop_masks(ctx.h, _lib.ptr(b), _lib.ptr(u), C.byref(params), w, h, _lib.ptr(K4), _lib.ptr(d), _lib.ptr(T),
                                        _lib.ptr(labels), _lib.ptr(recs), C.byref(m), _lib.ptr(plane)))
    masks = labels[None] == np.arange(1, m.value + 1, dtype=np.uint16)[:, None, None]
    out = (masks, np.ascontiguousarray(recs[:m.value]).view(GEOPROP_RECORD).reshape(-1), plane.view(GEOPROP_PLANE)[0])
    return out + (labels,) if return_labels else out


def geoprop_timing(ctx):
    """d2r_geoprop_get_timing -> (upload, heights and histogram, components, selection and label image, download) of the context's
    last propose_masks, device-event milliseconds."""
    ms = np.zeros(5, np.float64)
    ctx.check(ctx.lib.d2r_geoprop_get_timing(ctx.h, _lib.ptr(ms)))
    return tuple(float(x) for x in ms)


def labels_from_census(counts):
    """The object count of build_scene_model (reference dream2real.py:139-144) from per-frame label counts [N,256] (or totals
    [256]): labels = the labels some pixel carries, num_objs = their number without 255 (out of scene).  ObjectModel.mask_idx =
    obj_idx assumes the labels below 255 are exactly 0 .. num_objs - 1; anything else is a ValueError naming the first missing
    label.  -> (labels int array, num_objs)."""
    totals = np.asarray(counts, np.uint64).reshape(-1, 256).sum(axis=0)
    labels = np.nonzero(totals)[0]
    num_objs = len(labels) - int(255 in labels)
    objs = labels[labels != 255]
    if not np.array_equal(objs, np.arange(num_objs)):
        missing = int(np.setdiff1d(np.arange(int(objs.max()) + 1), objs)[0])
        raise ValueError(f"label census: the masks carry the labels {objs.tolist()} but not {missing}; object k must carry label k "
                         f"(labels 0 .. {num_objs - 1} for {num_objs} objects, 255 outside the scene)")
    return labels, num_objs


def label_census(masks, *, ctx):
    """uint8 label images [N,H,W] -> (labels, num_objs, counts uint32 [N,256]): one d2r_masks_census call in place of
    torch.unique over all frames; counts[f, k] > 0 says frame f sees object k."""
    counts = _lib.masks_census(ctx, _np(masks).astype(np.uint8))
    labels, num_objs = labels_from_census(counts)
    return labels, num_objs, counts


def load_cached_masks(out_dir, n):
    """segment_associate's cache branch: <out_dir>/XMem_masks/rgb_%04d.png for n frames -> uint8 [n,H,W]."""
    mask_dir = os.path.join(out_dir, "XMem_masks")
    return np.stack([_lib.png_read_grey(os.path.join(mask_dir, "rgb_%04d.png" % k), 8) for k in range(n)])


def mask_touches_edge(mask) -> bool:
    """reference segmentation/sam_seg.py:286-297: a boolean mask [h,w] with at least one set pixel has one on the frame's border"""
    m = _np(mask).astype(bool)
    rows, cols = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
    return bool(rows[0] == 0 or rows[-1] == m.shape[0] - 1 or cols[0] == 0 or cols[-1] == m.shape[1] - 1)


def get_thumbnail(img, obj_mask, padding=5, use_mask=True):
    """reference segmentation/sam_seg.py:250-271: img [h,w,3] white outside obj_mask (with use_mask), cropped to the mask's bounding
    box widened by `padding` and clamped to the frame.  Host numpy; the engine's thumbnails come from caption.object_thumbnails."""
    img, m = _np(img), _np(obj_mask).astype(bool)
    if use_mask:
        img = img.copy()
        img[~m] = 255
    rows, cols = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
    first_row, last_row = max(0, rows[0] - padding), min(img.shape[0] - 1, rows[-1] + padding)
    first_col, last_col = max(0, cols[0] - padding), min(img.shape[1] - 1, cols[-1] + padding)
    return img[first_row:last_row + 1, first_col:last_col + 1]
