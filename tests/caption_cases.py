"""Inputs shared by tests/test_caption_host.py, tests/test_caption_gpu.py and tests/test_caption_engine_gpu.py:
thumbnails of chosen sizes, seeded unit vectors, and the oracle's side of a comparison, computed once per process."""
import functools

import numpy as np

from tests import caption_ref as R

S = 224
# (h, w) the resize rule was checked on against HF's CLIPImageProcessor; the first four upscale
SHAPES = ((11, 40), (40, 11), (17, 17), (15, 600), (224, 224), (223, 225), (300, 1000), (720, 1280))
# one batch of the GPU test: the shapes above but the whole frame, one pass only either way, and at the end of the packed buffer three
# thumbnails whose cols * 3 (and, the rows being odd, whose byte count) is 1, 2 and 3 mod 4
BATCH = ((11, 40), (40, 11), (17, 17), (S, S), (S, S + 1), (S + 1, S), (223, 225), (300, 1000), (15, 600), (5, 3), (5, 2), (5, 1))
# sizes that fill a batch up to 33 thumbnails, past the tower's 32-row tiles
FILLER = tuple((20 + 7 * i, 31 + 5 * ((3 * i) % 11)) for i in range(33 - len(BATCH) - 1))


@functools.lru_cache(maxsize=None)
def thumbnail(h, w, seed=0):
    """smooth structure plus noise: a resize of pure noise would hide a shifted tap behind the grey it averages to"""
    rng = np.random.default_rng(1000 * h + w + seed)
    i, j = np.mgrid[0:h, 0:w]
    base = 127 + 90 * np.sin(i / 3.0 + seed)[..., None] * np.cos(j[..., None] / 5.0 + np.arange(3))
    img = np.clip(base + rng.integers(-37, 38, (h, w, 3)), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def oracle_preprocess(h, w, seed=0):
    """(pixel_values [3,S,S] f32, crop [S,S,3] u8) of oracle.render_ref.clip_preprocess on thumbnail(h, w, seed)"""
    from oracle import render_ref
    return render_ref.clip_preprocess(thumbnail(h, w, seed), S, rot90=False)


def unit_vectors(n, D, seed):
    v = np.random.default_rng(seed).standard_normal((n, D))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def vote_case(D, V, per_obj, seed, duplicates=True):
    """embeddings of n_objs = len(per_obj) objects with per_obj[o] thumbnails each, V classes; with duplicates class V - 1 repeats class
    0 and (V >= 4) class 2 repeats class 1, so that equal scores must order by index"""
    obj_of = np.repeat(np.arange(len(per_obj)), per_obj).astype(np.uint32)
    emb = unit_vectors(len(obj_of), D, seed)
    cls = unit_vectors(V, D, seed + 1)
    if duplicates and V >= 2:
        cls[V - 1] = cls[0]
    if duplicates and V >= 4:
        cls[2] = cls[1]
    return emb, obj_of, cls


NAMES_SEED = 21          # of the V = 8 class embeddings of names_case


@functools.lru_cache(maxsize=None)
def towers():
    """(cfg, state dict) of the random-weight ViT-B/16 the GPU parity tests use; no text tower"""
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    cfg = CLIP_CONFIGS["vit_b16"]
    return cfg, random_clip_state_dict(cfg, seed=6, text=False)


@functools.lru_cache(maxsize=None)
def names_case():
    """The scene of thumbs_cases.scan5, multi view, named by the oracle alone: its thumbnails by tests/thumbs_ref.py, its preprocess and
    its vision tower on its own pixel values, the rule's sums in fp64.  -> dict(cls [8,512], scores fp64 [3,8], order [3,8], margin [3]
    top-1 minus top-2, views [3] thumbnails per object)"""
    from oracle import clip_ref, render_ref
    from tests import thumbs_cases
    cfg, sd = towers()
    _, thumbs = thumbs_cases.reference("scan5", False, True, 0)
    pv = np.stack([render_ref.clip_preprocess(t, S, rot90=False)[0] for mine in thumbs for t in mine])
    emb = clip_ref.vision_embeds(pv, sd, cfg).astype(np.float64)
    cls = unit_vectors(8, cfg["proj"], NAMES_SEED)
    cos = emb @ cls.astype(np.float64).T
    views = [len(mine) for mine in thumbs]
    ends = np.cumsum(views)
    scores = np.stack([cos[e - n:e].sum(axis=0) for e, n in zip(ends, views)])
    order = np.argsort(-scores, axis=1, kind="stable")
    top = np.take_along_axis(scores, order, 1)
    return dict(cls=cls, scores=scores, order=order, margin=top[:, 0] - top[:, 1], views=views)
