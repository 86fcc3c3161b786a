"""The object-thumbnail rule on the CPU: the tap table, the integer blur against scipy, hand vectors for
every branch of the rule as tests/thumbs_ref.py states it, and the Python layer (caption.caption_objs, the engine) with stubs."""
import json
import os

import numpy as np
import pytest

from dream2real_amd import _lib, caption, segmentation
from tests import thumbs_cases as cases
from tests import thumbs_ref as R


def test_tap_table_is_the_formula():
    q = R.derive_taps()
    assert np.array_equal(q, R.full_taps()) and len(R.TAPS) == 101 and np.array_equal(q, q[::-1])
    assert int(q.sum()) == 32767 and int(q.sum()) ** 2 < 2 ** 30 and int(q.sum()) < 2 ** 16


# images whose 0.5 contour crosses the frame (the cap on the band holds for them); 40 x 30 and 1 x 300 are smaller than the kernel:
# they exercise the repeated reflection, and the blur flattens them so far that a fifth of their pixels sits in the band
THRESHOLD_IMAGES = (("ring", 150, 200, True), ("half", 150, 200, True), ("blobs", 150, 200, True), ("half", 70, 130, True),
                    ("half", 30, 40, False), ("half", 300, 1, False))


@pytest.mark.parametrize("kind,h,w,capped", THRESHOLD_IMAGES)
def test_integer_blur_against_scipy(kind, h, w, capped):
    """bits agree with scipy's fp64 Gaussian wherever it is further than 0.008 from 0.5 (2 passes x 201 taps x 2^-16 of tap
    rounding = 0.0062); at most 5 % of the pixels may sit inside that band, or the image says nothing about the threshold"""
    from scipy import ndimage
    img = cases.blur_image(kind, h, w)
    ref = ndimage.gaussian_filter(img.astype(np.float64), sigma=30.5, mode="mirror", truncate=100 / 30.5)
    v = R.blur_values(img)
    band = np.abs(ref - 0.5) <= 0.008
    err = np.abs(v / 2.0 ** 30 - ref).max()
    print(kind, h, w, "in band %.4f" % band.mean(), "set %.4f" % (v >= R.BLUR_THRESHOLD).mean(), "max |v / 2^30 - scipy| %.2e" % err)
    assert np.array_equal((v >= R.BLUR_THRESHOLD)[~band], (ref >= 0.5)[~band])
    assert err < 0.0062
    assert band.mean() <= 0.05 or not capped
    if (h, w) == (150, 200):
        assert 0.02 < (v >= R.BLUR_THRESHOLD).mean() < 0.98         # the contour is inside the frame


def _scan(labels, oob=None, seed=0):
    labels = np.asarray(labels, np.uint8)
    rng = np.random.default_rng(seed)
    rgbs = rng.integers(0, 255, labels.shape + (3,), dtype=np.uint8)
    noise = rng.integers(0, 256, labels.shape[1:] + (3,), dtype=np.uint8)
    return rgbs, labels, (np.zeros_like(labels) if oob is None else np.asarray(oob, np.uint8)), noise


def _flags(recs):
    return {(r["obj"], r["frame"]): r["flags"] for r in recs}


def test_rotation_of_a_2x3_frame():
    a = np.arange(6).reshape(2, 3)
    assert np.array_equal(R.rot90ccw(a), [[2, 5], [1, 4], [0, 3]]) and np.array_equal(R.rot90ccw(a), np.rot90(a))
    lab = np.zeros((3, 2, 3), np.uint8)
    lab[:, 0, 2] = 1                                                  # one pixel at the top right: top left after the rotation
    rgbs, lab, oob, noise = _scan(lab)
    recs, thumbs = R.plan_and_thumbs(2, rgbs, lab, oob, noise, False, min_area=1, pad=0)
    assert [r["flags"] & R.ROTATED for r in recs] == [R.ROTATED, R.ROTATED, 0]
    assert [(r["row0"], r["col0"]) for r in recs] == [(0, 0), (0, 0), (0, 2)]
    assert all(np.array_equal(t[0, 0], rgbs[f][0, 2]) for f, t in enumerate(thumbs[0]))
    recs, _ = R.plan_and_thumbs(2, rgbs, lab, oob, noise, True, min_area=1, pad=0)
    assert not any(r["flags"] & R.ROTATED for r in recs)
    recs, _ = R.plan_and_thumbs(2, rgbs, lab, oob, noise, True, multi_view=False, single_view_idx=1, min_area=1, pad=0)
    assert len(recs) == 1 and recs[0]["frame"] == 1 and recs[0]["flags"] & R.ROTATED


def test_min_area_boundary_and_out_of_scene_pixels():
    lab = np.zeros((1, 20, 20), np.uint8)
    lab[0, 5:9, 5:10] = 1                                             # 20 pixels
    lab[0, 12:16, 5:10] = 2
    oob = np.zeros_like(lab)
    oob[0, 12, 5] = 7                                                 # any non-zero value is outside: object 2 keeps 19
    recs, thumbs = R.plan_and_thumbs(3, *_scan(lab, oob)[:3], _scan(lab)[3], True, min_area=20)
    f = _flags(recs)
    assert f[(1, 0)] == R.ACCEPTED and f[(2, 0)] == R.SMALL and [r["area"] for r in recs] == [20, 19]
    assert len(thumbs[0]) == 1 and thumbs[1] == []


def test_fourth_edge_touching_frame_is_skipped_unless_topdown():
    lab = np.zeros((5, 12, 12), np.uint8)
    lab[:, 0:3, 4:8] = 1
    lab[3, :, :] = 0
    lab[3, 4:7, 4:8] = 1                                              # frame 3 is clear of the border
    args = _scan(lab)
    recs, thumbs = R.plan_and_thumbs(2, *args, False, min_area=5)
    assert [bool(r["flags"] & R.ACCEPTED) for r in recs] == [True, True, True, True, False] and len(thumbs[0]) == 4
    assert [bool(r["flags"] & R.EDGE) for r in recs] == [True, True, True, False, True]
    recs, thumbs = R.plan_and_thumbs(2, *args, True, min_area=5)
    assert all(r["flags"] & R.ACCEPTED for r in recs) and len(thumbs[0]) == 5


def _ring_scan(n=1, size=40, hole=(14, 26), inner_label0=0, inner_total=None):
    """label 1 = a square ring whose hole is rows / columns hole[0] .. hole[1] - 1; inside the hole the first inner_label0 pixels (raster order) keep
    label 0 and the rest carry label 2"""
    lab = np.zeros((n, size, size), np.uint8)
    lab[:, 8:32, 8:32] = 1
    a, b = hole
    lab[:, a:b, a:b] = 2
    idx = np.argwhere(lab[0] == 2)[:inner_label0]
    lab[:, idx[:, 0], idx[:, 1]] = 0
    return lab


def test_container_test_branches():
    kw = dict(min_area=10, hole_area=100, dilate_k=3)
    lab = _ring_scan(inner_label0=20)                                 # hole 12 x 12 = 144, 20 of them label 0
    f = _flags(R.plan_and_thumbs(3, *_scan(lab), True, **kw)[0])
    assert f[(1, 0)] & R.CONTAINER and not f[(2, 0)] & R.CONTAINER
    lab = _ring_scan(hole=(14, 24), inner_label0=70)                  # hole 100, 70 label 0: 10 i == 7 a exactly, still a container
    assert _flags(R.plan_and_thumbs(3, *_scan(lab), True, **kw)[0])[(1, 0)] & R.CONTAINER
    lab = _ring_scan(hole=(14, 24), inner_label0=71)                  # one more: the hole is mostly background
    assert not _flags(R.plan_and_thumbs(3, *_scan(lab), True, **kw)[0])[(1, 0)] & R.CONTAINER
    lab = _ring_scan(hole=(14, 24), inner_label0=0)
    assert not _flags(R.plan_and_thumbs(3, *_scan(lab), True, min_area=10, hole_area=101, dilate_k=3)[0])[(1, 0)] & R.CONTAINER      # hole_area - 1
    assert _flags(R.plan_and_thumbs(3, *_scan(lab), True, min_area=10, hole_area=100, dilate_k=3)[0])[(1, 0)] & R.CONTAINER
    c_shape = _ring_scan(inner_label0=0)
    c_shape[:, 14:26, 26:] = 2                                        # the "hole" runs out to the border
    assert not _flags(R.plan_and_thumbs(3, *_scan(c_shape), True, **kw)[0])[(1, 0)] & R.CONTAINER
    for comp in R.components8(np.array([[1, 0], [0, 1]], bool)):      # diagonal neighbours are one component
        assert comp.sum() == 2


def test_container_flag_is_decided_on_frame_0_only():
    kw = dict(min_area=10, hole_area=100, dilate_k=3)
    lab = _ring_scan(n=4)
    lab[1:] = 0
    lab[1:, 8:32, 8:32] = 1                                           # frames 1 .. 3: a solid square, no hole
    recs, thumbs = R.plan_and_thumbs(2, *_scan(lab), True, **kw)
    assert all(r["flags"] & R.CONTAINER for r in recs) and thumbs[0][3].shape == (40, 40, 3)      # carried to frame 3: the whole frame
    small0 = lab.copy()
    small0[0] = 0
    small0[0, 0:3, 0:3] = 1                                           # frame 0 below min_area: never a container
    small0[1] = _ring_scan()[0]
    recs, _ = R.plan_and_thumbs(2, *_scan(small0), True, **kw)
    assert recs[0]["flags"] & R.SMALL and not any(r["flags"] & R.CONTAINER for r in recs)
    ring2 = np.repeat(_ring_scan(), 3, axis=0)
    recs, thumbs = R.plan_and_thumbs(2, *_scan(ring2), True, multi_view=False, single_view_idx=2, **kw)
    assert recs[0]["flags"] & R.ROTATED and not recs[0]["flags"] & R.CONTAINER and thumbs[0][0].shape == (34, 34, 3)
    recs, _ = R.plan_and_thumbs(2, *_scan(ring2), True, multi_view=False, single_view_idx=0, **kw)
    assert recs[0]["flags"] & R.CONTAINER


def test_pad_is_clamped_at_all_four_borders():
    lab = np.zeros((1, 30, 40), np.uint8)
    lab[0, 2:28, 3:38] = 1
    rgbs, lab, oob, noise = _scan(lab)
    recs, thumbs = R.plan_and_thumbs(2, rgbs, lab, oob, noise, True, min_area=1, pad=5)
    assert (recs[0]["row0"], recs[0]["col0"], recs[0]["rows"], recs[0]["cols"]) == (0, 0, 30, 40)
    want = segmentation.get_thumbnail(rgbs[0], lab[0] == 1)
    assert np.array_equal(thumbs[0][0], want) and not segmentation.mask_touches_edge(lab[0] == 1)
    lab2 = np.zeros((1, 30, 40), np.uint8)
    lab2[0, 10:12, 20:23] = 1
    rgbs, lab2, oob, noise = _scan(lab2)
    recs, thumbs = R.plan_and_thumbs(2, rgbs, lab2, oob, noise, True, min_area=1, pad=5)
    assert (recs[0]["row0"], recs[0]["col0"], recs[0]["rows"], recs[0]["cols"]) == (5, 15, 12, 13)
    assert np.array_equal(thumbs[0][0], segmentation.get_thumbnail(rgbs[0], lab2[0] == 1)) and (thumbs[0][0][0, 0] == 255).all()
    edge = np.zeros((4, 4), bool)
    edge[3, 1] = True
    assert segmentation.mask_touches_edge(edge)


def test_even_k_dilation_runs_in_the_rotated_frame():
    """an isolated bit dilated by an even k moves by (+1, +1)... in the frame the dilation runs in: dilating first and rotating
    after gives another answer, which is why blur and dilation are defined in the rotated frame"""
    b = np.zeros((9, 11), bool)
    b[4, 6] = True
    d = R.dilate(b, 2)
    assert d.sum() == 4 and d[4:6, 6:8].all()                        # offsets [-1, 0]: the block below and right of the bit
    assert np.array_equal(R.dilate(b, 1), b) and R.dilate(b, 3)[3:6, 5:8].all() and R.dilate(b, 3).sum() == 9
    corner = np.zeros((5, 5), bool)
    corner[0, 0] = True
    assert R.dilate(corner, 2).sum() == 4 and R.dilate(corner, 4).sum() == 9      # outside is ignored
    rot_then_dilate, dilate_then_rot = R.dilate(R.rot90ccw(b), 2), R.rot90ccw(R.dilate(b, 2))
    assert not np.array_equal(rot_then_dilate, dilate_then_rot)
    for img in (cases.blur_image("half", 30, 40), cases.blur_image("blobs", 70, 130)):       # the blur itself commutes with the rotation
        assert np.array_equal(R.blur_values(R.rot90ccw(img)), R.rot90ccw(R.blur_values(img)))
    assert np.array_equal(R.reflect101(np.array([-7, -1, 0, 2, 3, 4, 9]), 3), [1, 1, 0, 2, 1, 0, 1]) and R.reflect101(np.array([5]), 1)[0] == 0


# ------------------------------------------------------------------------------------------------ the Python layer, no GPU

@pytest.fixture
def fake_lib(monkeypatch):
    """_lib.thumbs_plan / thumbs_fill answered by the rule in numpy, packed as the library packs them"""
    state = {}

    def plan(ctx, rgbs, masks, oob, num_objs, topdown, multi_view=True, single_view_idx=0, min_area=200, hole_area=400, pad=5, dilate_k=60):
        state["args"] = (num_objs, rgbs, masks, oob), (topdown, multi_view, single_view_idx, min_area, hole_area, pad, dilate_k)
        recs, _ = R.plan_and_thumbs(num_objs, rgbs, masks, oob, np.zeros(rgbs[0].shape, np.uint8), *state["args"][1])
        out, off = np.zeros((len(recs), 10), np.uint32), 0
        for row, r in zip(out, recs):
            row[:8] = [r["obj"], r["frame"], r["flags"], r["area"], r["row0"], r["col0"], r["rows"], r["cols"]]
            if r["flags"] & R.ACCEPTED:
                row[8] = off
                off = (off + r["rows"] * r["cols"] * 3 + 3) // 4 * 4
        state["recs"] = out
        return out, off

    def fill(ctx, noise, total):
        (num_objs, rgbs, masks, oob), rest = state["args"]
        _, thumbs = R.plan_and_thumbs(num_objs, rgbs, masks, oob, noise, *rest)
        packed = np.zeros(total, np.uint8)
        flat = [t for mine in thumbs for t in mine]
        for row, t in zip([r for r in state["recs"] if r[2] & R.ACCEPTED], flat):
            packed[row[8]:row[8] + t.size] = t.reshape(-1)
        return packed

    monkeypatch.setattr(_lib, "thumbs_plan", plan)
    monkeypatch.setattr(_lib, "thumbs_fill", fill)
    return state


class _Aggregator:
    def aggregate_captions_for_obj(self, obj_captions, silent=False):
        assert silent is True
        return " + ".join(obj_captions)


def test_caption_objs_with_stub_callables(fake_lib, tmp_path):
    lab = np.zeros((3, 40, 40), np.uint8)
    lab[:, 4:20, 4:20] = 1
    lab[0:2, 20:36, 14:30] = 2                                        # object 2 is absent from frame 2
    rgbs, lab, oob, noise = _scan(lab)
    seen = []

    def captioner(images):
        seen.append(images)
        return [" %dx%d " % i.shape[:2] for i in images]

    path = str(tmp_path / "captions.json")
    caps, thumbs = caption.caption_objs(3, rgbs, lab, _Aggregator(), oob, True, ctx=None, captioner=captioner, noise=noise, cache_path=path)
    assert len(seen) == 1 and [i.shape[:2] for i in seen[0]] == [(25, 25)] * 3 + [(25, 26)] * 2         # once, object-major
    assert caps == ["__background__", "25x25 + 25x25 + 25x25", "25x26 + 25x26"] and json.load(open(path)) == caps
    assert np.array_equal(thumbs[0], rgbs[0]) and thumbs[1].shape == (25, 25, 3) and thumbs[2].shape == (25, 26, 3)
    assert np.array_equal(thumbs[1], segmentation.get_thumbnail(rgbs[0], lab[0] == 1))
    caps1, _ = caption.caption_objs(3, rgbs, lab, None, oob, True, multi_view=False, single_view_idx=1, ctx=None, captioner=captioner)
    assert caps1 == ["__background__", "25x25", "26x25"] and len(seen[1]) == 2                      # single view: rotated, first caption
    cached, none = caption.caption_objs(3, rgbs, lab, None, oob, True, ctx=None, captioner=None, cache_path=path, read_cache=True)
    assert cached == caps and none == [None] * 3
    with pytest.raises(ValueError, match="aggregate_captions_for_obj"):
        caption.caption_objs(3, rgbs, lab, object(), oob, True, ctx=None, captioner=captioner)
    assert len(seen) == 2                                             # refused before any image was built
    with pytest.raises(ValueError, match="object 2 has no frame"):
        caption.caption_objs(3, rgbs, lab, None, oob, True, multi_view=False, single_view_idx=2, ctx=None, captioner=captioner)
    default = caption.object_thumbnails(3, rgbs[:2], lab[:2], oob[:2], True, ctx=None)
    assert [len(t) for t in default] == [2, 2]
    with pytest.raises(ValueError, match="noise"):
        caption.object_thumbnails(3, rgbs, lab, oob, True, ctx=None, noise=np.zeros((4, 4, 3), np.uint8))


def test_engine_without_a_captioner_behaves_as_before(tmp_path, monkeypatch):
    from dream2real_amd.dream2real import CachedLangModel, ImaginationEngine
    from tests.test_engine_host import _cfg, _counts, _scan_folder
    labels = np.zeros((2, 6, 8), np.uint8)
    labels[0, :2] = 1
    d = _scan_folder(tmp_path, labels)
    monkeypatch.setattr(_lib, "masks_census", lambda ctx, m: _counts(*np.asarray(m)))
    eng = ImaginationEngine(_cfg(d), None, None)
    assert eng.captioner is None
    with pytest.raises(RuntimeError, match="captioning models are out of scope") as e:
        eng.build_scene_model()
    assert "captioner=" in str(e.value) and "captions.json" in str(e.value)
    eng.build_scene_model(captions=["__background__", "box"])
    assert all(o.thumbnail is None for o in eng.scene_model.objs) and len(CachedLangModel.METHODS) == 3


def test_engine_with_a_captioner_names_the_objects(fake_lib, tmp_path, monkeypatch):
    from dream2real_amd.dream2real import ImaginationEngine
    from tests.test_engine_host import _cfg, _counts, _scan_folder
    labels = np.zeros((2, 30, 40), np.uint8)
    labels[:, 5:25, 5:30] = 1
    d = _scan_folder(tmp_path, labels)
    monkeypatch.setattr(_lib, "masks_census", lambda ctx, m: _counts(*np.asarray(m)))
    eng = ImaginationEngine(_cfg(d, width=40, height=30), None, None, captioner=lambda images: ["a box"] * len(images))
    eng.build_scene_model()
    objs = eng.scene_model.objs
    assert [o.name for o in objs] == ["__background__", "a box"] and json.load(open(os.path.join(d, "captions.json"))) == ["__background__", "a box"]
    rot = not eng.topdown
    assert objs[1].thumbnail.shape == ((35, 30, 3) if rot else (30, 35, 3)) and objs[0].thumbnail.shape == (30, 40, 3)
