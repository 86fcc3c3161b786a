"""The object thumbnails on the GPU (d2r_thumbs_plan / d2r_thumbs_fill / d2r_thumbs_blur_bits): records and
bytes EQUAL tests/thumbs_ref.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from dream2real_amd import _lib, caption, engine
from tests import thumbs_cases as cases
from tests import thumbs_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("h,w", cases.BLUR_SIZES)
def test_blur_bits_equal_the_rule(ctx, h, w):
    """random blobs, the ring and a half-plane at every size; widths that are no multiple of 64 use the packed tail, 40 x 30 and the
    one-pixel-wide frames reflect more than once; every dilation size of the issue"""
    for kind in ("blobs", "ring", "half"):
        img = cases.blur_image(kind, h, w)
        bit = cases.blur_bit_ref(kind, h, w)
        for k in cases.BLUR_KS:
            got = _lib.thumbs_blur_bits(ctx, img, k)
            want = R.dilate(bit, k).astype(np.uint8)
            assert got.shape == want.shape and np.array_equal(got, want), (kind, h, w, k, int((got != want).sum()))


def _run(ctx, s, topdown, multi_view, single_view_idx):
    recs, total = _lib.thumbs_plan(ctx, s["rgbs"], s["masks"], s["oob"], s["num_objs"], topdown, multi_view, single_view_idx,
                                   s["min_area"], s["hole_area"], s["pad"], s["dilate_k"])
    return recs, total, _lib.thumbs_fill(ctx, s["noise"], total)


def _check(name, s, topdown, multi_view, single_view_idx, recs, total, packed):
    want_recs, want_thumbs = cases.reference(name, topdown, multi_view, single_view_idx)
    assert np.array_equal(recs[:, :8], cases.records_array(want_recs)), (name, topdown, multi_view, single_view_idx)
    flat = [t for mine in want_thumbs for t in mine]
    acc = [r for r in recs if r[2] & _lib.THUMB_ACCEPTED]
    assert len(acc) == len(flat)
    end = 0
    for r, t in zip(acc, flat):
        off = int(r[8]) | int(r[9]) << 32
        assert off % 4 == 0 and off >= end
        end = off + t.size
        got = packed[off:end].reshape(t.shape)
        assert np.array_equal(got, t), (name, int(r[0]), int(r[1]), int((got != t).sum()))
    assert total == (end + 3) // 4 * 4


@pytest.mark.parametrize("topdown", (False, True))
@pytest.mark.parametrize("multi_view,single_view_idx", ((True, 0), (False, 0), (False, 2)))
def test_plan_and_fill_equal_the_rule(ctx, topdown, multi_view, single_view_idx):
    s = cases.scan5()
    recs, total, packed = _run(ctx, s, topdown, multi_view, single_view_idx)
    _check("scan5", s, topdown, multi_view, single_view_idx, recs, total, packed)
    flags = {(int(r[0]), int(r[1])): int(r[2]) for r in recs}
    if multi_view:                                   # the scene holds what the rule branches on
        assert flags[(1, 0)] & R.CONTAINER and flags[(1, 3)] & R.CONTAINER and not flags[(2, 0)] & R.CONTAINER
        assert flags[(2, 3)] & R.SMALL and flags[(2, 4)] & R.SMALL and recs[[int(r[0]) == 2 and int(r[1]) == 4 for r in recs]][0][3] == 0
        assert all(flags[(3, f)] & R.EDGE for f in range(5))
        assert bool(flags[(3, 3)] & R.ACCEPTED) == topdown and bool(flags[(3, 4)] & R.ACCEPTED) == topdown


def test_frame_filling_container_at_the_reference_constants(ctx):
    s = cases.big_container()
    recs, total, packed = _run(ctx, s, False, True, 0)
    _check("big", s, False, True, 0, recs, total, packed)
    assert recs[0][2] & R.CONTAINER and recs[0][2] & R.ROTATED and tuple(recs[0][6:8]) == (1280, 720)


def test_254_objects(ctx):
    s = cases.many_objects()
    recs, total, packed = _run(ctx, s, True, True, 0)
    _check("many", s, True, True, 0, recs, total, packed)
    assert len(recs) == 254 * 2 and all(r[2] & R.ACCEPTED for r in recs)


def test_same_call_twice_same_bytes(ctx):
    s = cases.scan5()
    a = _run(ctx, s, False, True, 0)
    b = _run(ctx, s, False, True, 0)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    ms = _lib.thumbs_timing(ctx)
    assert len(ms) == 3 and all(np.isfinite(ms)) and ms[1] > 0


def test_refusals_carry_a_message():
    c = engine.Context(0)
    lib = _lib.load()
    s = cases.scan5()
    rgb, m, o, noise = s["rgbs"], s["masks"], s["oob"], s["noise"]
    n, h, w = m.shape
    n_recs, total = C.c_uint32(0), C.c_uint64(0)
    out = np.zeros(16, np.uint8)

    def plan(num_objs=4, dilate_k=60, single=0, multi=1, recs=None, cap=0):
        p = np.array([0, multi, single, 20, 40, 5, dilate_k], np.uint32)
        n_recs.value = cap
        return lib.d2r_thumbs_plan(c.h, _lib.ptr(rgb), _lib.ptr(m), _lib.ptr(o), n, w, h, num_objs, _lib.ptr(p), _lib.ptr(recs),
                                   C.byref(n_recs), C.byref(total))

    msg = lambda: lib.d2r_last_error(c.h).decode()
    assert lib.d2r_thumbs_fill(c.h, _lib.ptr(noise), _lib.ptr(out), 16) == -1 and "d2r_thumbs_plan" in msg()      # fill without a plan
    ms = np.zeros(3)
    assert lib.d2r_thumbs_get_timing(c.h, _lib.ptr(ms)) == -1 and "timing" in msg()
    assert plan(num_objs=0) == -1 and "num_objs" in msg()
    assert plan(num_objs=256) == -1 and "num_objs" in msg()
    assert plan(dilate_k=0) == -1 and "dilate_k" in msg()
    assert plan(dilate_k=65) == -1 and "dilate_k" in msg()
    assert plan(single=n, multi=0) == -1 and "single_view_idx" in msg()
    assert plan(recs=np.zeros((2, 10), np.uint32), cap=2) == -1 and "recs_out" in msg()
    assert lib.d2r_thumbs_fill(c.h, _lib.ptr(noise), _lib.ptr(out), 16) == -1                                    # a refused plan is no plan
    assert plan() == 0 and n_recs.value == 15 and total.value > 16                                               # count only
    assert lib.d2r_thumbs_fill(c.h, _lib.ptr(noise), _lib.ptr(out), 16) == -1 and "total_bytes" in msg()
    assert lib.d2r_thumbs_fill(c.h, None, _lib.ptr(out), total.value) == -1
    img = np.zeros((4, 4), np.uint8)
    assert lib.d2r_thumbs_blur_bits(c.h, _lib.ptr(img), 4, 4, 0, _lib.ptr(img)) == -1 and "dilate_k" in msg()
    assert lib.d2r_thumbs_blur_bits(c.h, None, 4, 4, 3, _lib.ptr(img)) == -1
    c.close()


def test_engine_builds_the_scene_with_a_captioner(ctx, tmp_path):
    """ImaginationEngine(captioner=...) on a scan folder of the five-frame scene: captions.json and ObjectModel.thumbnail are the
    rule's; with use_cache_captions the file is read and the captioner is not called"""
    from dream2real_amd.dream2real import ImaginationEngine
    from tests.test_engine_host import _cfg, _scan_folder
    s = cases.scan5()
    d = _scan_folder(tmp_path, s["masks"])
    for k in range(5):
        _lib.png_write(s["rgbs"][k], os.path.join(d, "images", "rgb_%04d.png" % k))
        _lib.png_write_channels(s["oob"][k], os.path.join(d, "images", "dynamic_mask_rgb_%04d.png" % k))
    calls = []

    def captioner(images):
        calls.append(len(images))
        return ["cap %d" % k for k in range(len(images))]

    eng = ImaginationEngine(_cfg(d, width=200, height=150), ctx, None, captioner=captioner)
    eng.build_scene_model()
    noise = np.random.default_rng(0).integers(0, 256, s["rgbs"][0].shape, np.uint8)
    _, want = R.plan_and_thumbs(4, s["rgbs"], s["masks"], s["oob"], noise, eng.topdown, False, 0)
    assert calls == [3] and json.load(open(os.path.join(d, "captions.json"))) == ["__background__", "cap 0", "cap 1", "cap 2"]
    objs = eng.scene_model.objs
    assert [o.name for o in objs] == ["__background__", "cap 0", "cap 1", "cap 2"]
    assert np.array_equal(objs[0].thumbnail, s["rgbs"][0]) and all(np.array_equal(objs[k + 1].thumbnail, want[k][0]) for k in range(3))
    assert want[0][0].shape == ((150, 200, 3) if eng.topdown else (200, 150, 3))            # the ring is a container: the whole frame
    again = ImaginationEngine(_cfg(d, width=200, height=150, use_cache_captions=True), ctx, None, captioner=captioner)
    again.build_scene_model()
    assert calls == [3] and [o.name for o in again.scene_model.objs] == [o.name for o in objs]


def test_caption_objs_from_gpu_thumbnails(ctx, tmp_path):
    """caption_objs through the engine's own path with a stub captioner: the captioner sees the rule's thumbnails once, in
    object-major order; captions.json and the thumbnails are as the rule says"""
    s = cases.scan5()
    want_recs, want_thumbs = cases.reference("scan5", False, False, 0)
    seen = []

    def captioner(images):
        seen.append([np.array(i) for i in images])
        return [f" thing {k} " for k in range(len(images))]

    path = str(tmp_path / "captions.json")
    default_noise = np.random.default_rng(0).integers(0, 256, s["rgbs"][0].shape, np.uint8)
    _, want_default = R.plan_and_thumbs(s["num_objs"], s["rgbs"], s["masks"], s["oob"], default_noise, False, False, 0, 200, 400, 5, 60)
    caps, thumbs = caption.caption_objs(s["num_objs"], s["rgbs"], s["masks"], None, s["oob"], False, multi_view=False, single_view_idx=0,
                                        ctx=ctx, captioner=captioner, cache_path=path)
    assert len(seen) == 1 and caps == ["__background__", "thing 0", "thing 1", "thing 2"] and json.load(open(path)) == caps
    flat = [t for mine in want_default for t in mine]
    assert len(seen[0]) == len(flat) and all(np.array_equal(a, b) for a, b in zip(seen[0], flat))
    assert np.array_equal(thumbs[0], s["rgbs"][0]) and all(np.array_equal(thumbs[k + 1], want_default[k][0]) for k in range(3))
    got = caption.object_thumbnails(s["num_objs"], s["rgbs"], s["masks"], s["oob"], False, False, 0, ctx=ctx, noise=s["noise"],
                                    min_area=20, hole_area=40)
    assert [len(g) for g in got] == [len(t) for t in want_thumbs]
    assert all(np.array_equal(a, b) for g, t in zip(got, want_thumbs) for a, b in zip(g, t))
    empty = np.zeros_like(s["masks"])
    empty[:, 10:40, 10:40] = 1
    with pytest.raises(ValueError, match="object 2"):
        caption.object_thumbnails(3, s["rgbs"], empty, s["oob"], False, ctx=ctx)
    assert os.path.exists(path)
