"""Object thumbnails for captioning and the captioner as a callable (reference caption.py:55-169).

The reference's Captioner builds, per object and frame, a masked crop (for containers a frame with noise poured over a blurred,
dilated mask) on the CPU with cv2 and hands the images to BLIP-2.  Here the image work runs on the GPU (d2r_thumbs_plan /
d2r_thumbs_fill) and the captioning model enters as `captioner(list_of_images) -> list of strings`."""
from __future__ import annotations

import json

import numpy as np

from . import _lib


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _frames(rgbs, masks, scene_masks):
    rgbs = np.ascontiguousarray(np.stack([_np(a) for a in rgbs]), np.uint8)
    masks = np.ascontiguousarray(np.stack([_np(a) for a in masks]), np.uint8)
    oob = np.ascontiguousarray(np.stack([_np(a) != 0 for a in scene_masks]), np.uint8)
    return rgbs, masks, oob


def object_thumbnails(num_objs, rgbs, masks, scene_masks, topdown, multi_view=True, single_view_idx=0, *, ctx, noise=None,
                      min_area=200, hole_area=400, pad=5, dilate_k=60):
    """-> a list per object 1 .. num_objs - 1 of uint8 [h,w,3] thumbnails, frames in increasing order.
    rgbs uint8 [N,H,W,3]; masks label images [N,H,W]; scene_masks [N,H,W], non-zero = outside the scene.  noise: the image poured
    over a container's blurred background, default a seeded one (the reference's is unseeded).  An object without an accepted
    frame is a ValueError naming it (the reference dies with an IndexError)."""
    rgbs, masks, oob = _frames(rgbs, masks, scene_masks)
    if noise is None:
        noise = np.random.default_rng(0).integers(0, 256, rgbs[0].shape, np.uint8)
    noise = np.ascontiguousarray(_np(noise), np.uint8)
    if noise.shape != rgbs[0].shape:
        raise ValueError(f"noise {noise.shape} is not a frame {rgbs[0].shape}")
    recs, total = _lib.thumbs_plan(ctx, rgbs, masks, oob, num_objs, topdown, multi_view, single_view_idx, min_area, hole_area, pad, dilate_k)
    thumbs = [[] for _ in range(1, num_objs)]
    accepted = [r for r in recs if r[2] & _lib.THUMB_ACCEPTED]
    for o, mine in enumerate(thumbs, start=1):
        if not any(int(r[0]) == o for r in accepted):
            raise ValueError(f"object {o} has no frame to caption: in every visited frame it covers fewer than {min_area} pixels "
                             "inside the scene bounds")
    packed = _lib.thumbs_fill(ctx, noise, total)
    for r in accepted:
        off, rows, cols = int(r[8]) | int(r[9]) << 32, int(r[6]), int(r[7])
        thumbs[int(r[0]) - 1].append(packed[off:off + rows * cols * 3].reshape(rows, cols, 3).copy())
    return thumbs


def caption_objs(num_objs, rgbs, masks, lang_model, scene_masks, topdown, multi_view=True, single_view_idx=0, *, ctx, captioner,
                 noise=None, cache_path=None, read_cache=False):
    """reference Captioner.caption_objs -> (captions, debug_thumbnails): one caption per object with "__background__" first, and the
    first thumbnail per object behind rgbs[0].  captioner(list of uint8 [h,w,3] images) -> list of strings is called ONCE with all
    thumbnails in object-major order.  Single view: an object's first caption.  Multi view:
    lang_model.aggregate_captions_for_obj(obj_captions, silent=True).  The result is written to cache_path when given; with
    read_cache it is read from there and no image is built."""
    if read_cache:
        with open(cache_path) as f:
            agg_captions = json.load(f)
        return agg_captions, [None] * len(agg_captions)
    if multi_view and not hasattr(lang_model, "aggregate_captions_for_obj"):
        raise ValueError("caption_objs: multi-view captions need lang_model.aggregate_captions_for_obj(obj_captions, silent=True)")
    all_thumbnails = object_thumbnails(num_objs, rgbs, masks, scene_masks, topdown, multi_view, single_view_idx, ctx=ctx, noise=noise)
    batched = [t for obj_thumbnails in all_thumbnails for t in obj_thumbnails]
    batched_captions = [str(c).strip() for c in captioner(batched)] if batched else []
    if len(batched_captions) != len(batched):
        raise ValueError(f"caption_objs: the captioner returned {len(batched_captions)} captions for {len(batched)} images")
    all_captions, at = [], 0
    for obj_thumbnails in all_thumbnails:
        all_captions.append(batched_captions[at:at + len(obj_thumbnails)])
        at += len(obj_thumbnails)
    debug_thumbnails = [_np(rgbs[0])] + [obj_thumbnails[0] for obj_thumbnails in all_thumbnails]
    if multi_view:
        agg_captions = [lang_model.aggregate_captions_for_obj(obj_captions, silent=True) for obj_captions in all_captions]
    else:
        agg_captions = [obj_captions[0] for obj_captions in all_captions]
    agg_captions.insert(0, "__background__")
    if cache_path is not None:
        with open(cache_path, "w") as f:
            json.dump(agg_captions, f)
    return agg_captions, debug_thumbnails
