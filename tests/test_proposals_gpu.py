"""d2r_proposals_labels (proposals.hip) against tests/proposals_ref.py, the numpy statement of DESIGN.md section 2h: the label
image, every record and the pair-intersection matrix are EQUAL for every case of tests/proposals_cases.py; the refusals return
D2R_ERR_INVALID and leave the caller's label image alone."""
import ctypes as C

import numpy as np
import pytest

from dream2real_amd import _lib, segmentation
from tests import proposals_cases as pc
from tests import proposals_ref as ref

pytestmark = pytest.mark.gpu

CASES = pc.all_cases()


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """The reference's answer per case, computed once and never written to."""
    out = {}
    for name, (P, inside) in CASES.items():
        out[name] = ref.proposals_to_labels(P, inside)
        for a in out[name]:
            a.setflags(write=False)
    return out


def _check(got, want, name):
    for g, w, what in zip(got, want, ("labels", "records", "inter")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{name}: {what} differ at {bad[:5].tolist()}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"
        assert np.array_equal(g, w)


@pytest.mark.parametrize("name", sorted(CASES))
def test_equal_to_the_reference(ctx, expected, name):
    P, inside = CASES[name]
    _check(_lib.proposals_labels(ctx, P, inside, records=True, inter=True), expected[name], name)


@pytest.mark.parametrize("name", ["pairs_9_65x33", "blob_gaps", "pairs_17_130x50"])
def test_several_passes_of_the_labelling_workspace_give_the_same(ctx, expected, name, monkeypatch):
    """A workspace budget of three masks' worth drives the batch through several passes, as a large M at 1280 x 720 goes."""
    P, inside = CASES[name]
    m, h, w = P.shape
    per_mask = w * h * 8 + h * ((w + 63) // 64) * 8 + (5 * h + 2) * 4
    monkeypatch.setenv("D2R_PROPOSALS_WS_BYTES", str(3 * per_mask))
    assert m > 3
    _check(_lib.proposals_labels(ctx, P, inside, records=True, inter=True), expected[name], name)


def test_python_entry_point_returns_labels_and_structured_records(ctx, expected):
    P, inside = CASES["scene_bound_and"]
    labels, recs = segmentation.proposals_to_labels(P, inside, ctx=ctx, return_records=True)
    want_labels, want_recs, _ = expected["scene_bound_and"]
    assert np.array_equal(labels, want_labels) and labels.dtype == np.uint8
    assert recs.dtype.names == ("area", "ncomp", "stage", "label", "boundary", "ew", "eh", "dd") and recs.shape == (3,)
    for k, field in enumerate(recs.dtype.names):
        assert np.array_equal(recs[field], want_recs[:, k]), field
    assert np.array_equal(segmentation.proposals_to_labels(P, inside, ctx=ctx), want_labels)


def test_empty_input_is_an_all_zero_image(ctx):
    labels = _lib.proposals_labels(ctx, np.zeros((0, 33, 65), np.uint8))
    assert labels.shape == (33, 65) and not labels.any()
    lib = _lib.load()
    out = np.full((33, 65), 7, np.uint8)
    assert lib.d2r_proposals_labels(ctx.h, None, None, 0, 65, 33, _lib.ptr(out), None, None) == 0 and not out.any()


def test_255_survivors_fit_and_256_are_refused_with_the_outputs_untouched(ctx):
    P, _ = pc.square_grid(256)
    m, h, w = P.shape
    p8 = np.ascontiguousarray(P, np.uint8)
    labels = _lib.proposals_labels(ctx, p8[:255])
    want = np.zeros((h, w), np.uint8)
    for k in range(255):
        want[P[k]] = k + 1
    assert np.array_equal(labels, want)
    lib = _lib.load()
    out, recs, inter = np.full((h, w), 7, np.uint8), np.full((m, 8), 7, np.uint32), np.full((m, m), 7, np.uint32)
    assert lib.d2r_proposals_labels(ctx.h, _lib.ptr(p8), None, m, w, h, _lib.ptr(out), _lib.ptr(recs), _lib.ptr(inter)) == -1
    assert "256 proposals survive" in lib.d2r_last_error(ctx.h).decode()
    assert (out == 7).all() and (recs == 7).all() and (inter == 7).all()
    with pytest.raises(_lib.D2RError, match="survive"):
        segmentation.proposals_to_labels(P, ctx=ctx)


def test_refusals_return_invalid_and_leave_the_label_image_alone(ctx):
    lib = _lib.load()
    p = np.ones((2, 4, 4), np.uint8)
    out = np.full((4, 4), 7, np.uint8)
    call = lambda props, m, w, h, labels: lib.d2r_proposals_labels(ctx.h, props, None, m, w, h, labels, None, None)
    assert call(_lib.ptr(p), 1025, 4, 4, _lib.ptr(out)) == -1 and "1024" in lib.d2r_last_error(ctx.h).decode()
    assert call(_lib.ptr(p), 2, 0, 4, _lib.ptr(out)) == -1 and "width" in lib.d2r_last_error(ctx.h).decode()
    assert call(_lib.ptr(p), 2, 4, 0, _lib.ptr(out)) == -1
    assert call(_lib.ptr(p), 2, 8193, 4, _lib.ptr(out)) == -1
    assert call(None, 2, 4, 4, _lib.ptr(out)) == -1
    assert call(_lib.ptr(p), 2, 4, 4, None) == -1
    assert lib.d2r_proposals_labels(C.c_void_p(0), _lib.ptr(p), None, 2, 4, 4, _lib.ptr(out), None, None) == -1
    assert (out == 7).all()
    ms = np.zeros(3)
    assert lib.d2r_proposals_get_timing(ctx.h, None) == -1
    assert np.array_equal(_lib.proposals_labels(ctx, p), np.zeros((4, 4), np.uint8))          # two full masks: both large; the context still works
    assert lib.d2r_proposals_get_timing(ctx.h, _lib.ptr(ms)) == 0 and (ms >= 0).all()


@pytest.mark.parametrize("w,h", pc.LABELLER_SIZES)
def test_both_sources_of_the_labeller_count_the_same_components(ctx, w, h):
    """One image through both instantiations of k_label_*: the bit-plane source counts the components of the 5 x 5 dilation inside
    d2r_proposals_labels (record word 1), the byte source labels the same dilation through d2r_masks_components, where a root is a
    pixel whose key is its own raster index.  Both equal the flood fill's count."""
    from tests import masks_ref
    for name, B in pc.labeller_images(w, h).items():
        D = masks_ref.dilate(B, 5, fast=True)
        want = int((masks_ref.components(D).ravel() == np.arange(h * w)).sum())
        _, recs = _lib.proposals_labels(ctx, B[None], records=True)
        keys, _, _ = _lib.masks_components(ctx, D, np.zeros((h, w), np.uint16))
        roots = int((keys.ravel() == np.arange(h * w)).sum())
        print(name, w, h, "bits", int(recs[0, 1]), "bytes", roots, "flood fill", want)
        assert int(recs[0, 1]) == roots == want, (name, w, h)
