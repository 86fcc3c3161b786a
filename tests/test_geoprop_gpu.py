"""d2r_geoprop_masks against the numpy restatement of DESIGN.md section 2l (tests/geoprop_ref.py): the label image, the records and the
plane record are compared by equality of every byte, on the cases of tests/geoprop_cases.py."""
import ctypes as C

import numpy as np
import pytest

from dream2real_amd import _lib, segmentation
from tests import geoprop_cases as gc
from tests import geoprop_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _K(k4):
    return np.array([[k4[0], 0, k4[2]], [0, k4[1], k4[3]], [0, 0, 1]], np.float64)


def _raw(ctx, d16, pose, k4, bounds, up=(0.0, 0.0, 1.0), **params):
    """The C entry point with every output poisoned first -> (labels, records [max_props,6], M, plane record)."""
    p = dict(ref.DEFAULTS, **params)
    h, w = d16.shape
    labels = np.full((h, w), 0xA5A5, np.uint16)
    recs = np.full((p["max_props"], ref.REC_WORDS), 0xA5A5A5A5, np.uint32)
    plane, m = np.full(5, -7, np.int32), C.c_uint32(0xA5A5A5A5)
    rc = ctx.lib.d2r_geoprop_masks(ctx.h, _lib.ptr(np.ascontiguousarray(bounds, np.float64).reshape(6)), _lib.ptr(np.array(up, np.float64)),
                                   C.byref(segmentation.GeopropParams(p["window_mm"], p["h_min_mm"], p["tau_mm"], p["min_area"], p["max_props"])),
                                   w, h, _lib.ptr(np.ascontiguousarray(k4, np.float64)), _lib.ptr(np.ascontiguousarray(d16)),
                                   _lib.ptr(np.ascontiguousarray(pose, np.float32).reshape(16)), _lib.ptr(labels), _lib.ptr(recs), C.byref(m),
                                   _lib.ptr(plane))
    assert rc == 0, ctx.lib.d2r_last_error(ctx.h)
    return labels, recs, m.value, plane


def _same(got, want, what=""):
    for name, g, w in zip(("labels", "records", "M", "plane"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        diff = np.argwhere(g != w)
        assert len(diff) == 0, f"{what} {name}: {len(diff)} entries differ, the first at {diff[0].tolist()}: {g[tuple(diff[0])]} for {w[tuple(diff[0])]}"
    assert got[0].dtype == np.uint16 and got[1].dtype == np.uint32 and got[3].dtype == np.int32


@pytest.mark.parametrize("name", list(gc.CASES))
def test_every_byte_equals_the_restatement(ctx, name):
    d16, pose, k4, bounds, params = gc.case(name)
    _same(_raw(ctx, d16, pose, k4, bounds, **params), gc.reference(name), name)


def test_the_python_layer_hands_out_masks_records_and_the_plane(ctx):
    d16, pose, k4, bounds, params = gc.case("scene frame 0")
    labels, recs, m, plane = gc.reference("scene frame 0")
    masks, got_recs, got_plane, got_labels = segmentation.propose_masks(d16, pose, _K(k4), bounds, ctx=ctx, return_labels=True, **params)
    assert masks.dtype == bool and masks.shape == (m,) + d16.shape and np.array_equal(masks, ref.masks(labels, m)) and np.array_equal(got_labels, labels)
    assert [got_recs[k].tolist() for k in got_recs.dtype.names] == recs[:m].T.tolist()
    assert [int(got_plane[k]) for k in got_plane.dtype.names] == plane.tolist()
    metres = d16.astype(np.float16) / np.float16(1000)                # the loader's fp16 metres come back as the same millimetres here
    if np.array_equal(segmentation.depth_to_u16(metres), d16):
        assert np.array_equal(segmentation.propose_masks(metres, pose, _K(k4), bounds, ctx=ctx)[0], masks)
    empty = segmentation.propose_masks(np.zeros_like(d16), pose, _K(k4), bounds, ctx=ctx)
    assert empty[0].shape == (0,) + d16.shape and len(empty[1]) == 0 and int(empty[2]["inside"]) == 0


def test_a_tilted_up_and_other_parameters(ctx):
    d16, pose, k4, bounds, params = gc.case("scene frame 0")
    a = np.deg2rad(20.0)
    up = np.array([0.0, -np.sin(a), np.cos(a)])
    for over in (dict(up=up), dict(window_mm=1, h_min_mm=0, tau_mm=0), dict(window_mm=41, h_min_mm=30, tau_mm=65535, min_area=0, max_props=2),
                 dict(min_area=1, max_props=1024, tau_mm=1)):
        kw = dict(params, **{k: v for k, v in over.items() if k != "up"})
        want = ref.propose(d16, pose, k4, bounds, up=over.get("up", (0.0, 0.0, 1.0)), **kw)
        _same(_raw(ctx, d16, pose, k4, bounds, up=over.get("up", (0.0, 0.0, 1.0)), **kw), want, str(over))


def test_two_calls_give_the_same_bytes(ctx):
    d16, pose, k4, bounds, params = gc.case("crop 129 x 70")
    a = _raw(ctx, d16, pose, k4, bounds, **params)
    b = _raw(ctx, d16, pose, k4, bounds, **params)
    _same(a, b)
    ms = segmentation.geoprop_timing(ctx)
    assert len(ms) == 5 and all(np.isfinite(x) and x >= 0 for x in ms)


def test_every_refusal_leaves_the_outputs_untouched_and_the_context_usable(ctx):
    d16, pose, k4, bounds, params = gc.case("crop 65 x 17")
    h, w = d16.shape
    lib = ctx.lib
    P = segmentation.GeopropParams
    labels = np.full((h, w), 0xA5A5, np.uint16)
    recs = np.full((255, ref.REC_WORDS), 0xA5A5A5A5, np.uint32)
    plane, m = np.full(5, -7, np.int32), np.full(1, 0xA5A5A5A5, np.uint32)

    def call(**over):
        a = dict(ctx=ctx.h, bounds=np.array(bounds, np.float64).reshape(6), up=np.array([0.0, 0.0, 1.0]), params=P(5, 6, 10, 20, 255), w=w, h=h,
                 K=np.array(k4, np.float64), d16=np.array(d16), pose=np.array(pose, np.float32).reshape(16), labels=labels, recs=recs, m=m, plane=plane)
        a.update(over)
        p = a["params"]
        keep = [np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x for x in (a["bounds"], a["up"], a["K"], a["d16"], a["pose"])]
        ptr = lambda x: _lib.ptr(x) if x is not None else None
        return lib.d2r_geoprop_masks(a["ctx"], ptr(keep[0]), ptr(keep[1]), C.byref(p) if p is not None else None, a["w"], a["h"], ptr(keep[2]), ptr(keep[3]),
                                     ptr(keep[4]), ptr(a["labels"]), ptr(a["recs"]), ptr(a["m"]), ptr(a["plane"]))

    def bad_pose(k, v):
        p = np.array(pose, np.float32).reshape(16)
        p[k] = v
        return p

    def bad_bounds(k, v):
        b = np.array(bounds, np.float64).reshape(6)
        b[k] = v
        return b

    refusals = {
        "no context": dict(ctx=None), "no bounds": dict(bounds=None), "no up": dict(up=None), "no params": dict(params=None), "no K": dict(K=None),
        "no depth": dict(d16=None), "no pose": dict(pose=None), "no label image": dict(labels=None), "no records": dict(recs=None),
        "no count": dict(m=None), "no plane record": dict(plane=None),
        "w = 0": dict(w=0), "h = 0": dict(h=0), "too many pixels": dict(w=2048, h=1025),
        "a pose that is not rigid": dict(pose=bad_pose(0, 1.5)), "a pose with NaN": dict(pose=bad_pose(3, np.nan)),
        "a pose with a last row": dict(pose=bad_pose(12, 0.1)),
        "fx = 0": dict(K=np.array([0.0, 380, 1, 1])), "fx < 0": dict(K=np.array([-380.0, 380, 1, 1])), "fy = inf": dict(K=np.array([380.0, np.inf, 1, 1])),
        "fy = NaN": dict(K=np.array([380.0, np.nan, 1, 1])), "cx = NaN": dict(K=np.array([380.0, 380, np.nan, 1])),
        "bounds with NaN": dict(bounds=bad_bounds(1, np.nan)), "lo = hi": dict(bounds=bad_bounds(3, bounds.reshape(6)[0])),
        "lo > hi": dict(bounds=bad_bounds(5, -1.0)), "more than 2^16 height bins": dict(bounds=bad_bounds(5, 66.0)),
        "up too long": dict(up=np.array([0.0, 0.0, 1.00001])), "up of length 0": dict(up=np.zeros(3)), "up with NaN": dict(up=np.array([0.0, np.nan, 1.0])),
        "window 0": dict(params=P(0, 6, 10, 20, 255)), "window even": dict(params=P(4, 6, 10, 20, 255)), "window 65537": dict(params=P(65537, 6, 10, 20, 255)),
        "h_min 65536": dict(params=P(5, 65536, 10, 20, 255)), "tau 65536": dict(params=P(5, 6, 65536, 20, 255)),
        "max_props 0": dict(params=P(5, 6, 10, 20, 0)), "max_props 1025": dict(params=P(5, 6, 10, 20, 1025)),
    }
    for name, over in refusals.items():
        rc = call(**over)
        assert rc == -1, (name, rc)
        assert (labels == 0xA5A5).all() and (recs == 0xA5A5A5A5).all() and (plane == -7).all() and m[0] == 0xA5A5A5A5, name
        if over.get("ctx", 1) is not None:
            assert lib.d2r_last_error(ctx.h), name
    assert lib.d2r_geoprop_get_timing(ctx.h, None) == -1 and lib.d2r_geoprop_get_timing(None, _lib.ptr(np.zeros(5))) == -1
    # the context still works, and the very same buffers are filled now
    assert call() == 0
    _same((labels, recs, int(m[0]), plane), gc.reference("crop 65 x 17"))


def test_the_8_connected_labellers_still_give_their_results(ctx):
    """The labeller the new source shares with masks.hip (bytes) and proposals.hip (bits) keeps its diagonals there: the two squares
    that touch at a corner are one component to disconnected_prune and one component of the dilation to proposals_to_labels, as in
    tests/test_masks_gpu.py and tests/test_proposals_gpu.py; and 8-connected keys of a label image equal tests/masks_ref.py's."""
    from tests import masks_ref
    labels, recs, m, plane = gc.reference("diagonal")
    assert m == 2
    both = (labels > 0).astype(np.uint8)
    kept = segmentation.disconnected_prune(both, ctx=ctx)
    assert np.array_equal(kept, both)                                     # one component of 450 pixels: nothing is pruned
    keys = masks_ref.components(both)
    assert len(np.unique(keys[both > 0])) == 1
    two = both.copy()
    two[16:31, 64:79] = 0
    two[18:28, 66:76] = 1                                                 # a smaller square off the corner: two components, the larger stays
    kept = segmentation.disconnected_prune(two, ctx=ctx)
    assert kept[1:16, 49:64].all() and not kept[18:28, 66:76].any()
    out, rec = segmentation.proposals_to_labels(both[None].astype(bool), ctx=ctx, return_records=True)
    assert int(rec["ncomp"][0]) == 1 and int(rec["boundary"][0]) == 2 * 56      # both squares' outlines: one 8-connected component of the bits
