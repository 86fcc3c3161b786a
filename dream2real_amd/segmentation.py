"""The geometric half of the reference's segmentation stage (segmentation/XMem_infer.py:213-236, 264-351) on the GPU: connected
components of a raw label image, the area rule, the component nearest the scene centre (duplicate_prune) or the largest
(disconnected_prune), the out-of-scene overwrite, and the XMem_masks/rgb_%04d.png files everything downstream reads.  The rule
is DESIGN.md section 2d.

Running SAM or XMem is out of scope: `proposals_to_labels` turns the mask generator's proposals into the first frame's label
image (sam_seg.py:80-115 and integrate_masks); whatever produced the raw label images of all frames (XMem in
the reference), `refine_masks` is the body of the `segment_associate` loop from there on and `load_cached_masks` its cache branch."""
from __future__ import annotations

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
