"""Object thumbnails for captioning and the captioner as a callable (reference caption.py:55-169).

The reference's Captioner builds, per object and frame, a masked crop (for containers a frame with noise poured over a blurred,
dilated mask) on the CPU with cv2 and hands the images to BLIP-2.  Here the image work runs on the GPU (d2r_thumbs_plan /
d2r_thumbs_fill) and the captioning model enters as `captioner(list_of_images) -> list of strings`, or is
this package's own: a ClipCaptioner names every object from a closed vocabulary with the CLIP towers the engine already holds, the
thumbnails never leaving the device (d2r_caption_names)."""
from __future__ import annotations

import json
import os

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
    accepted, packed = _plan_and_fill(num_objs, rgbs, masks, scene_masks, topdown, multi_view, single_view_idx, ctx, noise, min_area, hole_area,
                                      pad, dilate_k)
    thumbs = [[] for _ in range(1, num_objs)]
    for r in accepted:
        off, rows, cols = int(r[8]) | int(r[9]) << 32, int(r[6]), int(r[7])
        thumbs[int(r[0]) - 1].append(packed[off:off + rows * cols * 3].reshape(rows, cols, 3).copy())
    return thumbs


def _plan_and_fill(num_objs, rgbs, masks, scene_masks, topdown, multi_view, single_view_idx, ctx, noise, min_area, hole_area, pad, dilate_k):
    """thumbs_plan + thumbs_fill -> (the accepted records in record order, the packed thumbnails); they stay on the context's device"""
    rgbs, masks, oob = _frames(rgbs, masks, scene_masks)
    if noise is None:
        noise = np.random.default_rng(0).integers(0, 256, rgbs[0].shape, np.uint8)
    noise = np.ascontiguousarray(_np(noise), np.uint8)
    if noise.shape != rgbs[0].shape:
        raise ValueError(f"noise {noise.shape} is not a frame {rgbs[0].shape}")
    recs, total = _lib.thumbs_plan(ctx, rgbs, masks, oob, num_objs, topdown, multi_view, single_view_idx, min_area, hole_area, pad, dilate_k)
    accepted = [r for r in recs if r[2] & _lib.THUMB_ACCEPTED]
    for o in range(1, num_objs):
        if not any(int(r[0]) == o for r in accepted):
            raise ValueError(f"object {o} has no frame to caption: in every visited frame it covers fewer than {min_area} pixels "
                             "inside the scene bounds")
    return accepted, _lib.thumbs_fill(ctx, noise, total)


VOCABULARY_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "object_names.txt")


def load_vocabulary(path=VOCABULARY_PATH):
    """the names of a vocabulary file, one per line; blank lines and lines that start with # are skipped"""
    with open(path, encoding="utf-8") as f:
        return [line.strip() for line in f if line.strip() and not line.startswith("#")]


def class_embeddings(text_embeds):
    """e [V,P,D], the L2-normalised text embeddings of V names under P prompt templates -> c [V,D] float32, c_v = normalise(mean_p e[v][p])
    in float64, rounded once"""
    e = np.asarray(text_embeds, np.float64)
    if e.ndim != 3:
        raise ValueError(f"class_embeddings takes [V, P, D], got shape {e.shape}")
    m = e.mean(axis=1)
    return (m / np.sqrt((m * m).sum(axis=1, keepdims=True))).astype(np.float32)


class ClipCaptioner:
    """Zero-shot object names from a closed vocabulary.  scorer: an engine.ClipScorer, text_encoder: an
    engine.TextEncoder of the same checkpoint, tokenizer: callable(captions) -> ids [C,T] or (ids, attention_mask).  The vocabulary
    (default: dream2real_amd/data/object_names.txt) under every template (default: clip_scoring.CLIP_TEMPLATES) is tokenised and
    encoded once; class_embeds [V,D] is kept.  k: the names reported per object, 1 .. min(8, V); the caption is the first."""

    ENCODE_CHUNK = 2048          # captions per d2r_text_encode call

    def __init__(self, ctx, scorer, text_encoder, tokenizer, vocabulary=None, templates=None, k=3):
        missing = [n for n, v in (("scorer", scorer), ("text_encoder", text_encoder), ("tokenizer", tokenizer)) if v is None]
        if missing:
            raise ValueError("ClipCaptioner needs " + " and ".join(f"{n}=" for n in missing) + ": the names are matched against the "
                             "thumbnails by the CLIP towers")
        names = load_vocabulary() if vocabulary is None else [str(n) for n in vocabulary]
        if not names:
            raise ValueError("ClipCaptioner: the vocabulary is empty")
        if len(names) > _lib.CAPTION_MAX_V:
            raise ValueError(f"ClipCaptioner: {len(names)} names, at most {_lib.CAPTION_MAX_V}")
        if len(set(names)) != len(names):
            raise ValueError("ClipCaptioner: a name stands in the vocabulary twice")
        if not isinstance(k, int) or not 1 <= k <= min(_lib.CAPTION_MAX_K, len(names)):
            raise ValueError(f"ClipCaptioner: k must be 1 .. min({_lib.CAPTION_MAX_K}, the {len(names)} names), got {k!r}")
        if templates is None:
            from .clip_scoring import CLIP_TEMPLATES
            templates = CLIP_TEMPLATES
        templates = tuple(templates)
        if not templates or not all("{}" in t for t in templates):
            raise ValueError("ClipCaptioner: every template must hold {} for the name, and there must be one")
        if scorer.cfg["proj"] != text_encoder.cfg["proj"]:
            raise ValueError(f"ClipCaptioner: the scorer embeds into {scorer.cfg['proj']} dimensions, the text encoder into "
                             f"{text_encoder.cfg['proj']}: they are not towers of one checkpoint")
        self.ctx, self.scorer, self.names, self.templates, self.k = ctx, scorer, names, templates, k
        ids = tokenizer([t.format(n) for n in names for t in templates])
        ids = np.asarray(ids[0] if isinstance(ids, tuple) else ids, np.int32)
        e = np.concatenate([text_encoder.encode(ids[c0:c0 + self.ENCODE_CHUNK]) for c0 in range(0, len(ids), self.ENCODE_CHUNK)])
        self.class_embeds = class_embeddings(e.reshape(len(names), len(templates), -1))
        self.last_timing = None

    def _name(self, num_objs, rgbs, masks, scene_masks, topdown, multi_view, single_view_idx, noise, min_area=200, hole_area=400, pad=5,
              dilate_k=60):
        accepted, packed = _plan_and_fill(num_objs, rgbs, masks, scene_masks, topdown, multi_view, single_view_idx, self.ctx, noise, min_area,
                                          hole_area, pad, dilate_k)
        first = {}
        for r in accepted:
            if int(r[0]) not in first:
                off, rows, cols = int(r[8]) | int(r[9]) << 32, int(r[6]), int(r[7])
                first[int(r[0])] = packed[off:off + rows * cols * 3].reshape(rows, cols, 3).copy()
        if num_objs <= 1:
            return ["__background__"], [], []
        idx, score = _lib.caption_names(self.ctx, self.scorer, self.class_embeds, num_objs - 1, self.k)
        self.last_timing = _lib.caption_timing(self.ctx)
        top = [[(self.names[int(i)], float(s)) for i, s in zip(idx[o], score[o])] for o in range(num_objs - 1)]
        return ["__background__"] + [t[0][0] for t in top], top, [first[o] for o in range(1, num_objs)]

    def name_objects(self, num_objs, rgbs, masks, scene_masks, topdown, multi_view=True, single_view_idx=0, noise=None, **thumb_params):
        """-> (captions, top): one name per object with "__background__" first, and per object 1 .. num_objs - 1 its k best
        (name, score) pairs, score the sum over the object's accepted thumbnails of the cosine between thumbnail and name.  Two
        objects may take the same name.  thumb_params: min_area, hole_area, pad, dilate_k of object_thumbnails."""
        captions, top, _ = self._name(num_objs, rgbs, masks, scene_masks, topdown, multi_view, single_view_idx, noise, **thumb_params)
        return captions, top


def caption_objs(num_objs, rgbs, masks, lang_model, scene_masks, topdown, multi_view=True, single_view_idx=0, *, ctx, captioner,
                 noise=None, cache_path=None, read_cache=False):
    """reference Captioner.caption_objs -> (captions, debug_thumbnails): one caption per object with "__background__" first, and the
    first thumbnail per object behind rgbs[0].  captioner(list of uint8 [h,w,3] images) -> list of strings is called ONCE with all
    thumbnails in object-major order.  Single view: an object's first caption.  Multi view:
    lang_model.aggregate_captions_for_obj(obj_captions, silent=True).  The result is written to cache_path when given; with
    read_cache it is read from there and no image is built.  A ClipCaptioner as the captioner takes the device route instead
    (DESIGN.md section 2m): the summed evidence over an object's views stands where the language model's merging stands, so
    lang_model is not asked, and the k best names per object are written to caption_scores.json beside cache_path."""
    if read_cache:
        with open(cache_path) as f:
            agg_captions = json.load(f)
        return agg_captions, [None] * len(agg_captions)
    if isinstance(captioner, ClipCaptioner):
        agg_captions, top, first = captioner._name(num_objs, rgbs, masks, scene_masks, topdown, multi_view, single_view_idx, noise)
        if cache_path is not None:
            with open(cache_path, "w") as f:
                json.dump(agg_captions, f)
            with open(os.path.join(os.path.dirname(cache_path), "caption_scores.json"), "w") as f:
                json.dump([[[n, s] for n, s in t] for t in top], f)
        return agg_captions, [_np(rgbs[0])] + first
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
