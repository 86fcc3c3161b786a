"""Object names from the package's own CLIP towers on the GPU (d2r_caption_embed / _vote / _names): the ragged
preprocess EQUALS the oracle's bytes, the vote hook EQUALS tests/caption_ref.py's bits, the fused call equals the hooks composed, and
the names equal the oracle's forward where the oracle's own margin is wide."""
import ctypes as C

import numpy as np
import pytest

from dream2real_amd import _lib, engine
from tests import caption_cases as cases
from tests import caption_ref as R
from tests import thumbs_cases
from tests.parity_utils import cosine, logit_bar

pytestmark = pytest.mark.gpu
S = cases.S


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scorer(ctx):
    cfg, sd = cases.towers()
    s = engine.ClipScorer(ctx, cfg, sd)
    yield s
    s.close()


def _plan_fill(ctx, s, topdown, multi_view):
    recs, total = _lib.thumbs_plan(ctx, s["rgbs"], s["masks"], s["oob"], s["num_objs"], topdown, multi_view, 0, s["min_area"], s["hole_area"],
                                   s["pad"], s["dilate_k"])
    packed = _lib.thumbs_fill(ctx, s["noise"], total)
    acc = [r for r in recs if r[2] & _lib.THUMB_ACCEPTED]
    thumbs = [packed[(int(r[8]) | int(r[9]) << 32):][:int(r[6]) * int(r[7]) * 3].reshape(int(r[6]), int(r[7]), 3) for r in acc]
    return acc, thumbs


def _oracle(img):
    from oracle import render_ref
    return render_ref.clip_preprocess(img, S, rot90=False)


def _check_preprocess(images, crops, pv):
    for i, img in enumerate(images):
        want_pv, want_u8 = _oracle(img)
        assert np.array_equal(crops[i], want_u8), (i, img.shape, int((crops[i] != want_u8).sum()))
        assert np.array_equal(pv[i].view(np.uint32), want_pv.view(np.uint32)), (i, img.shape)


@pytest.fixture(scope="module")
def container(ctx, scorer):
    """thumbs_cases.big_container through the real plan and fill: (thumbnails, embeddings, crops, pixel values) read where the fill
    left the packed buffer on the device"""
    acc, thumbs = _plan_fill(ctx, thumbs_cases.big_container(), False, True)
    thumbs = [t.copy() for t in thumbs]
    return (thumbs,) + _lib.caption_embed(ctx, scorer, len(thumbs), crops=True, pixel_values=True)


def test_whole_frame_container_from_the_fills_own_buffer(container):
    thumbs, emb, crops, pv = container
    assert thumbs[0].shape == (1280, 720, 3) and len(thumbs) == 2        # the rotated frame: 720 columns, a 1280-row support
    _check_preprocess(thumbs, crops, pv)
    assert np.abs(np.linalg.norm(emb.astype(np.float64), axis=1) - 1).max() < 1e-5


def test_ragged_batch_of_33_is_byte_exact_and_embeds_like_embed_pixels(ctx, scorer, container):
    """every size of the issue in ONE launch: x20 upscales elongated both ways, 17 x 17, S x S (no pass), one pass only either way,
    223 x 225, 300 x 1000, the 15 x 600 sliver of an 8960-column resize, a whole 1280 x 720 frame, and at the buffer's end thumbnails
    of 1, 2 and 3 bytes mod 4; 33 thumbnails run past the tower's 32-row tiles"""
    sizes = cases.BATCH[:9] + cases.FILLER
    images = [cases.thumbnail(h, w) for h, w in sizes] + [container[0][0]] + [cases.thumbnail(h, w) for h, w in cases.BATCH[9:]]
    assert len(images) == 33 and [im.shape[1] * 3 % 4 for im in images[-3:]] == [1, 2, 3]
    _lib.caption_load_packed(ctx, images, [0] * 33, 1)
    emb, crops, pv = _lib.caption_embed(ctx, scorer, 33, crops=True, pixel_values=True)
    _check_preprocess(images, crops, pv)
    again = _lib.caption_embed(ctx, scorer, 33, crops=True, pixel_values=True)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((emb, crops, pv), again))
    ms = _lib.caption_timing(ctx)
    assert len(ms) == 5 and all(np.isfinite(ms)) and ms[1] > 0 and ms[2] > 0 and ms[3] == 0
    # the same batch in passes of 16, 16 and 1 (the tower's pass size is the context's "chunk"): the later passes read their
    # descriptors at an offset and write pass-relative patches, crops and pixel values
    ctx.set_option("chunk", 16)
    try:
        emb3, crops3, pv3 = _lib.caption_embed(ctx, scorer, 33, crops=True, pixel_values=True)
    finally:
        ctx.set_option("chunk", 4096)
    assert np.array_equal(crops3, crops) and np.array_equal(pv3.view(np.uint32), pv.view(np.uint32))
    assert float((1.0 - cosine(emb3, emb)).max()) <= logit_bar(scorer.cfg) and np.abs(emb3 - emb).max() <= logit_bar(scorer.cfg)
    print(f"[caption] three passes vs one: max |d embedding| = {np.abs(emb3 - emb).max():.3e}")
    # the embeddings against the tower on the ORACLE's pixel values: both paths round the same fp32 values to bf16 patches
    want = scorer.embed_pixels(np.stack([_oracle(im)[0] for im in images]))
    worst = float((1.0 - cosine(emb, want)).max())
    same = np.array_equal(emb.view(np.uint32), want.view(np.uint32))
    bar = logit_bar(scorer.cfg, worst, "caption_embed vs embed_pixels on the oracle's pixel values, 1 - cosine")
    print(f"[caption] max |d embedding| = {np.abs(emb - want).max():.3e}, same bits: {same}")
    assert worst <= bar and np.abs(emb - want).max() <= bar


def test_batch_of_one(ctx, scorer):
    img = cases.thumbnail(40, 11)
    _lib.caption_load_packed(ctx, [img], [0], 1)
    emb, crops, pv = _lib.caption_embed(ctx, scorer, 1, crops=True, pixel_values=True)
    _check_preprocess([img], crops, pv)
    want = scorer.embed_pixels(_oracle(img)[0][None])
    assert float((1.0 - cosine(emb, want)).max()) <= logit_bar(scorer.cfg)


@pytest.mark.parametrize("D", (512, 768))
@pytest.mark.parametrize("V", (1, 3, 64, 65, 1000))
def test_vote_hook_equals_the_rule_bit_for_bit(ctx, D, V):
    """objects of 1 and 5 thumbnails and one without any; the last object's thumbnails are the last records; duplicated class rows"""
    per_obj = (1, 5, 0, 1, 5)
    emb, obj_of, cls = cases.vote_case(D, V, per_obj, 100 + V)
    for k in sorted({1, min(8, V)}):
        idx, sc = _lib.caption_vote(ctx, emb, obj_of, cls, len(per_obj), k)
        want_idx, want_sc = R.vote(emb, obj_of, cls, len(per_obj), k)
        assert np.array_equal(idx, want_idx), (D, V, k, idx.tolist(), want_idx.tolist())
        assert np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32)), (D, V, k)
        if V >= 2 and k >= 2:                      # class V - 1 repeats class 0: where it is named, 0 stands before it with the same bits
            for row, s in zip(idx.tolist(), sc.view(np.uint32).tolist()):
                assert V - 1 not in row or (0 in row and row.index(0) < row.index(V - 1) and s[row.index(0)] == s[row.index(V - 1)])


def test_a_score_that_is_no_number_ranks_as_minus_infinity(ctx):
    """a NaN in one thumbnail's embedding makes every score of its object NaN: the answer is then the first k classes at -inf, never
    an index outside the vocabulary; the other object is untouched"""
    emb, obj_of, cls = cases.vote_case(512, 5, (2, 2), 9, duplicates=False)
    emb = emb.copy()
    emb[1, 7] = np.nan
    idx, sc = _lib.caption_vote(ctx, emb, obj_of, cls, 2, 3)
    want_idx, want_sc = R.vote(emb, obj_of, cls, 2, 3)
    assert idx[0].tolist() == [0, 1, 2] and np.isneginf(sc[0]).all() and np.isfinite(sc[1]).all()
    assert np.array_equal(idx, want_idx) and np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))


@pytest.fixture(scope="module")
def scan5_names(ctx, scorer):
    """the five-frame scene, multi view, through plan, fill and the fused call with the oracle case's class embeddings; then the same
    thumbnails through the hooks"""
    case = cases.names_case()
    acc, _ = _plan_fill(ctx, thumbs_cases.scan5(), False, True)
    fused = _lib.caption_names(ctx, scorer, case["cls"], 3, 3)
    ms = _lib.caption_timing(ctx)
    emb = _lib.caption_embed(ctx, scorer, len(acc))
    obj_of = [int(r[0]) - 1 for r in acc]
    return case, fused, emb, obj_of, ms


def test_fused_call_equals_the_hooks_composed(ctx, scan5_names):
    case, (idx, sc), emb, obj_of, ms = scan5_names
    assert [obj_of.count(o) for o in range(3)] == case["views"]
    want_idx, want_sc = _lib.caption_vote(ctx, emb, obj_of, case["cls"], 3, 3)
    assert np.array_equal(idx, want_idx) and np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))
    rule_idx, rule_sc = R.vote(emb, np.array(obj_of), case["cls"], 3, 3)
    assert np.array_equal(idx, rule_idx) and np.array_equal(sc.view(np.uint32), rule_sc.view(np.uint32))
    assert all(m > 0 for m in ms[1:4])


def test_names_equal_the_oracles_forward(scorer, scan5_names):
    """first a condition on the INPUTS, on the oracle alone: every object's top-1 / top-2 margin exceeds four times the bar (a
    cosine's, times the views summed).  Seed 21 of the class embeddings, the first tried, gives margins of 0.15 .. 0.26."""
    case, (idx, sc), _, _, _ = scan5_names
    bar = logit_bar(scorer.cfg)
    for o in range(3):
        assert case["margin"][o] > 4 * bar * case["views"][o], (o, case["margin"][o])
    assert idx[:, 0].tolist() == case["order"][:, 0].tolist()
    worst = float(np.abs(sc.astype(np.float64) - np.take_along_axis(case["scores"], idx.astype(np.int64), 1)).max())
    print(f"[caption] max |score - oracle's| = {worst:.2e} over sums of {case['views']} cosines")
    assert worst <= bar * max(case["views"])


def test_refusals_carry_a_message_and_leave_outputs_untouched(scorer):
    c = engine.Context(0)
    lib = _lib.load()
    msg = lambda: lib.d2r_last_error(c.h).decode()
    D = scorer.cfg["proj"]
    cls = cases.unit_vectors(4, D, 1)
    emb = cases.unit_vectors(3, D, 2)
    idx, sc = np.full((2, 2), 77, np.uint32), np.full((2, 2), 7.0, np.float32)
    out = np.full((4, D), 7.0, np.float32)
    ms = np.zeros(5)
    clean = lambda: (idx == 77).all() and (sc == 7.0).all() and (out == 7.0).all()
    # a scorer of another context's device pointer is not used before the checks: no plan or fill on this context
    assert lib.d2r_caption_embed(c.h, scorer.h, _lib.ptr(out), None, None) == -1 and "d2r_thumbs_fill" in msg() and clean()
    assert lib.d2r_caption_names(c.h, scorer.h, _lib.ptr(cls), 4, D, 1, 2, _lib.ptr(idx), _lib.ptr(sc)) == -1 and "d2r_thumbs_fill" in msg() and clean()
    assert lib.d2r_caption_get_timing(c.h, _lib.ptr(ms)) == -1 and "timing" in msg()
    s = thumbs_cases.scan5()
    recs, total = _lib.thumbs_plan(c, s["rgbs"], s["masks"], s["oob"], s["num_objs"], False, False, 0, 20, 40, 5, 60)
    assert lib.d2r_caption_embed(c.h, scorer.h, _lib.ptr(out), None, None) == -1 and "d2r_thumbs_fill" in msg() and clean()      # a plan alone
    _lib.caption_load_packed(c, [cases.thumbnail(17, 17)], [0], 1)

    def vote(obj_of=(0, 0, 1), V=4, Dv=D, n_objs=2, k=2, classes=cls):
        o = np.array(obj_of, np.uint32)
        return lib.d2r_caption_vote(c.h, _lib.ptr(emb), _lib.ptr(o), 3, _lib.ptr(classes), V, Dv, n_objs, k, _lib.ptr(idx), _lib.ptr(sc))

    def names(V=4, Dn=D, k=2, classes=cls, n_objs=1):
        return lib.d2r_caption_names(c.h, scorer.h, _lib.ptr(classes), V, Dn, n_objs, k, _lib.ptr(idx), _lib.ptr(sc))

    bad = cls.copy()
    bad[3, 5] = np.inf
    for call in (vote, names):
        assert call(V=0) == -1 and "V = 0" in msg() and clean()
        assert call(k=0) == -1 and "k must be" in msg() and clean()
        assert call(k=5) == -1 and "k must be" in msg() and clean()                    # above V
        assert call(V=4, k=9) == -1 and "k must be" in msg() and clean()
        assert call(classes=bad) == -1 and "not finite" in msg() and clean()
    assert names(Dn=256) == -1 and "proj_dim" in msg() and clean()
    assert names(n_objs=2) == -1 and "n_objs is 2" in msg() and "1 objects" in msg() and clean()      # the outputs are sized by the caller
    assert vote(Dv=100) == -1 and "multiple of 64" in msg() and clean()
    assert vote(obj_of=(0, 1, 0)) == -1 and "non-decreasing" in msg() and clean()
    assert vote(obj_of=(0, 1, 2)) == -1 and "below n_objs" in msg() and clean()
    assert vote(n_objs=0) == -1 and "n_objs" in msg() and clean()
    assert lib.d2r_caption_embed(c.h, None, _lib.ptr(out), None, None) == -1 and lib.d2r_caption_embed(c.h, scorer.h, None, None, None) == -1
    r = np.array([[0, 4, 4, 0, 0]], np.uint32)
    img = np.zeros(48, np.uint8)
    assert lib.d2r_caption_load_packed(c.h, _lib.ptr(img), 40, _lib.ptr(r), 1, 1) == -1 and "inside the packed buffer" in msg()
    assert lib.d2r_caption_load_packed(c.h, _lib.ptr(img), 48, _lib.ptr(r), 0, 1) == -1
    assert vote() == 0 and not clean() and lib.d2r_caption_get_timing(c.h, _lib.ptr(ms)) == 0
    c.close()
