"""ImaginationEngine(captioner="clip", proposer="geometric", tracker="geometric") on the scan folder of tests/test_engine_gpu.py:
build_scene_model names the objects with the engine's own CLIP towers and needs no callable from outside;
a callable captioner still takes the old path; use_cache_captions reads the file and builds no image."""
import json
import os
import zlib

import numpy as np
import pytest

from dream2real_amd import caption, engine
from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
from dream2real_amd.dream2real import ImaginationEngine
from tests import test_engine_gpu as scan

pytestmark = pytest.mark.gpu
CFG = CLIP_CONFIGS["vit_tiny"]


def word_tokenizer(captions):
    """one id per word (its CRC into the tiny model's vocabulary), framed by the start id and the end id, the largest, which also pads"""
    bos, eos = CFG["vocab"] - 2, CFG["vocab"] - 1
    rows = [[bos] + [2 + zlib.crc32(w.encode()) % (CFG["vocab"] - 4) for w in c.split()][:CFG["ctx"] - 2] + [eos] for c in captions]
    T = max(len(r) for r in rows)
    return np.array([r + [eos] * (T - len(r)) for r in rows], np.int32)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def towers(ctx):
    sd = random_clip_state_dict(CFG, seed=6)
    return engine.ClipScorer(ctx, CFG, sd), engine.TextEncoder(ctx, CFG, sd)


def test_build_scene_model_with_no_callable_from_outside(ctx, towers, tmp_path, monkeypatch):
    scorer, text_encoder = towers
    rgbs, mm, raw_labels, poses = scan._frames()
    d = str(tmp_path / "scan")
    scan._write_scan(d, rgbs, mm, poses)
    cfg = scan._engine_cfg(tmp_path, d, use_cache_segs=False, multi_view_captions=True)
    eng = ImaginationEngine(cfg, ctx, scorer, intrinsics=scan.K, proposer="geometric", tracker="geometric", captioner="clip",
                            text_encoder=text_encoder, tokenizer=word_tokenizer)
    assert eng.lang_model is None and eng.segmentor is None
    eng.build_scene_model()
    sm = eng.scene_model
    names = caption.load_vocabulary()
    assert len(sm.objs) == 3 and sm.objs[0].name == "__background__" and all(o.name in names for o in sm.objs[1:])
    captions, top = eng.captioner.name_objects(3, sm.rgbs, sm.masks, eng.out_scene_bound_masks, eng.topdown, multi_view=True, single_view_idx=0)
    assert json.load(open(os.path.join(d, "captions.json"))) == captions == [o.name for o in sm.objs]
    assert json.load(open(os.path.join(d, "caption_scores.json"))) == [[[n, s] for n, s in t] for t in top]
    assert len(top) == 2 and all(len(t) == 3 and t[0][1] >= t[1][1] >= t[2][1] for t in top) and [t[0][0] for t in top] == captions[1:]
    thumbs = caption.object_thumbnails(3, sm.rgbs, sm.masks, eng.out_scene_bound_masks, eng.topdown, True, 0, ctx=ctx)
    assert np.array_equal(sm.objs[0].thumbnail, caption._np(sm.rgbs[0])) and all(np.array_equal(sm.objs[k + 1].thumbnail, thumbs[k][0]) for k in range(2))
    print("names:", captions, "scores:", top, "timing (upload, preprocess, tower, scoring, download) ms:", eng.captioner.last_timing)

    # a callable captioner on the same scan: the old path, once, with every thumbnail in object-major order
    calls = []

    def captioner(images):
        calls.append([np.array(i) for i in images])
        return ["cap %d" % k for k in range(len(images))]

    single = scan._engine_cfg(tmp_path, d, use_cache_segs=False)
    old = ImaginationEngine(single, ctx, None, intrinsics=scan.K, proposer="geometric", tracker="geometric", captioner=captioner)
    old.build_scene_model()
    first = caption.object_thumbnails(3, sm.rgbs, sm.masks, eng.out_scene_bound_masks, eng.topdown, False, 0, ctx=ctx)
    assert len(calls) == 1 and len(calls[0]) == 2 and all(np.array_equal(a, b[0]) for a, b in zip(calls[0], first))
    assert [o.name for o in old.scene_model.objs] == ["__background__", "cap 0", "cap 1"] == json.load(open(os.path.join(d, "captions.json")))

    # use_cache_captions: the file is read, no image is built
    def no_images(*a, **k):
        raise AssertionError("use_cache_captions built thumbnails")

    monkeypatch.setattr(caption, "_plan_and_fill", no_images)
    cached = scan._engine_cfg(tmp_path, d, use_cache_segs=False, multi_view_captions=True, use_cache_captions=True)
    again = ImaginationEngine(cached, ctx, scorer, intrinsics=scan.K, proposer="geometric", tracker="geometric", captioner=eng.captioner)
    again.build_scene_model()
    assert [o.name for o in again.scene_model.objs] == ["__background__", "cap 0", "cap 1"]
