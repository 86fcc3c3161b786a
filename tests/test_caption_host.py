"""The rule of DESIGN.md section 2m without a GPU: the numpy restatement against Pillow and the oracle, the committed vocabulary, the
class embeddings, the cosine's order, the tie rule, and the argument errors of ClipCaptioner and the engine."""
import os

import numpy as np
import pytest

from dream2real_amd import caption
from tests import caption_cases as cases
from tests import caption_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _pillow(img, S):
    """Pillow's antialiased bicubic to the processor's size, then the floor centre crop"""
    from PIL import Image
    h, w, _ = img.shape
    nh, nw = R.resized_size(h, w, S)
    big = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BICUBIC))
    top, left = (nh - S) // 2, (nw - S) // 2
    return big[top:top + S, left:left + S]


@pytest.mark.parametrize("h,w", cases.SHAPES)
def test_resize_and_crop_equal_pillow_and_the_oracle(h, w):
    img = cases.thumbnail(h, w)
    got = R.resize_crop(img, cases.S)
    assert np.array_equal(got, _pillow(img, cases.S)), (h, w)
    pv, u8 = cases.oracle_preprocess(h, w)
    assert np.array_equal(got, u8), (h, w, int((got != u8).sum()))
    assert np.array_equal(R.pixel_values(got).view(np.uint32), pv.view(np.uint32)), (h, w)


def test_resized_size_truncates_and_squares_stay_square():
    assert R.resized_size(17, 17, 224) == (224, 224) and R.resized_size(223, 225, 224) == (224, 226)
    assert R.resized_size(15, 600, 224) == (224, 8960) and R.resized_size(40, 11, 224) == (814, 224)
    assert R.resized_size(720, 1280, 224) == (224, 398)             # 398.2 truncates


def test_default_vocabulary_is_usable():
    from dream2real_amd.tokenizer import ClipBpeTokenizer
    names = caption.load_vocabulary()
    assert 200 <= len(names) <= 1000 and len(set(names)) == len(names)
    assert all(n and n == n.lower() == n.strip() and all(c.isalpha() or c == " " for c in n) for n in names), [n for n in names if n != n.lower()]
    tok = ClipBpeTokenizer.from_files(os.path.join(GOLDEN, "bpe_vocab.json"), os.path.join(GOLDEN, "bpe_merges.txt"))
    # the small trained vocabulary of the tokenizer goldens splits words into more pieces than CLIP's does: an upper bound on the length
    longest = max(len(tok.encode(t.format(n))) for n in names for t in ("a low resolution photo of {}",))
    assert longest <= 77, longest
    assert os.path.getsize(caption.VOCABULARY_PATH) < 1 << 20


def test_class_embeddings_against_fp64():
    rng = np.random.default_rng(3)
    e = rng.standard_normal((7, 9, 64))
    e = (e / np.linalg.norm(e, axis=2, keepdims=True)).astype(np.float32)
    want = e.astype(np.float64).mean(axis=1)
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    for got in (caption.class_embeddings(e), R.class_embeddings(e)):
        assert got.dtype == np.float32 and got.shape == (7, 64)
        assert np.abs(got - want).max() <= 2.0 ** -24                  # one rounding of values below 1
        assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6
    with pytest.raises(ValueError, match=r"\[V, P, D\]"):
        caption.class_embeddings(e[0])


@pytest.mark.parametrize("D", (512, 768))
def test_cosine_is_close_to_fp64_and_is_its_written_order(D):
    img, cls = cases.unit_vectors(6, D, 1), cases.unit_vectors(40, D, 2)
    got = R.cosines(img, cls)
    brute = img.astype(np.float64) @ cls.astype(np.float64).T
    assert got.dtype == np.float32 and np.abs(got - brute).max() <= 1e-6
    # another order of the same sums is as close but not the same bits: the rule fixes the order, not only the value
    perm = np.random.default_rng(5).permutation(D)
    other = R.cosines(img[:, perm], cls[:, perm])
    assert np.abs(other - brute).max() <= 1e-6 and (other.view(np.uint32) != got.view(np.uint32)).any()
    flat = (img[:, None, :] * cls[None, :, :]).sum(axis=2, dtype=np.float32)
    assert (flat.view(np.uint32) != got.view(np.uint32)).any()
    assert np.array_equal(R.cosines(img, cls).view(np.uint32), got.view(np.uint32))


def test_scores_sum_in_record_order_and_ties_go_to_the_lower_index():
    emb, obj_of, cls = cases.vote_case(64, 9, (1, 5, 0, 2), 7)
    cos = R.cosines(emb, cls)
    s = R.object_scores(cos, obj_of, 4)
    assert np.array_equal(s[0], cos[0]) and not s[2].any()
    run = np.float32(0)
    for t in range(1, 6):
        run = np.float32(run + cos[t, 3])
    assert s[1, 3].view(np.uint32) == run.view(np.uint32)
    idx, sc = R.topk(s, 8)
    assert np.array_equal(s[:, 0], s[:, 8]) and np.array_equal(s[:, 1], s[:, 2])          # the duplicated rows
    for o in range(4):
        order = idx[o].tolist()
        assert len(set(order)) == 8 and all(sc[o, r] >= sc[o, r + 1] for r in range(7))
        assert 0 in order and (8 not in order or order.index(0) + 1 == order.index(8))
        if 1 in order and 2 in order:
            assert order.index(1) + 1 == order.index(2)
    assert idx[2].tolist() == list(range(8))                            # no thumbnail: every score 0, the first k classes
    one = np.array([[0.5, 0.75, 0.75, -1.0]], np.float32)
    assert R.topk(one, 3)[0].tolist() == [[1, 2, 0]]


class _Towers:
    """stand-ins that record what they are asked: a text encoder whose embedding depends on the ids alone, a tokenizer of characters"""

    def __init__(self, proj=64):
        self.cfg = {"proj": proj, "image_size": 64}
        self.calls = []

    def encode(self, ids):
        self.calls.append(ids.shape)
        e = np.stack([np.random.default_rng(int(np.abs(r).sum())).standard_normal(self.cfg["proj"]) for r in ids])
        return (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)

    @staticmethod
    def tokenizer(captions):
        T = max(len(c) for c in captions)
        return np.array([[ord(ch) for ch in c] + [0] * (T - len(c)) for c in captions], np.int32)


def test_clip_captioner_builds_class_embeddings_once_and_refuses_by_name():
    t = _Towers()
    cap = caption.ClipCaptioner(None, t, t, t.tokenizer, vocabulary=["mug", "red ball", "box"], templates=("{}", "a photo of {}"), k=2)
    assert t.calls == [(6, len("a photo of red ball"))] and cap.class_embeds.shape == (3, 64) and cap.names == ["mug", "red ball", "box"]
    want = R.class_embeddings(t.encode(t.tokenizer(["mug", "a photo of mug", "red ball", "a photo of red ball", "box", "a photo of box"])).reshape(3, 2, 64))
    assert np.array_equal(cap.class_embeds, want)
    full = caption.ClipCaptioner(None, t, t, lambda c: (t.tokenizer(c), None))          # (ids, mask) tokenizers; the committed defaults
    assert full.class_embeds.shape == (len(caption.load_vocabulary()), 64) and full.k == 3 and len(full.templates) == 9
    with pytest.raises(ValueError, match="text_encoder= and tokenizer="):
        caption.ClipCaptioner(None, t, None, None)
    with pytest.raises(ValueError, match="empty"):
        caption.ClipCaptioner(None, t, t, t.tokenizer, vocabulary=[])
    with pytest.raises(ValueError, match="twice"):
        caption.ClipCaptioner(None, t, t, t.tokenizer, vocabulary=["a", "b", "a"])
    for k in (0, 3, 9, 1.5):
        with pytest.raises(ValueError, match="k must be"):
            caption.ClipCaptioner(None, t, t, t.tokenizer, vocabulary=["a", "b"], k=k)
    with pytest.raises(ValueError, match="template"):
        caption.ClipCaptioner(None, t, t, t.tokenizer, vocabulary=["a"], templates=("a photo",), k=1)
    with pytest.raises(ValueError, match="one checkpoint"):
        caption.ClipCaptioner(None, t, _Towers(32), t.tokenizer, vocabulary=["a"], k=1)


def test_engine_refuses_captioner_strings_by_name(tmp_path):
    from dream2real_amd.dream2real import ImaginationEngine
    from tests.test_engine_host import _cfg
    cfg = _cfg(str(tmp_path))
    t = _Towers()
    with pytest.raises(ValueError, match="blip"):
        ImaginationEngine(cfg, None, t, captioner="blip")
    with pytest.raises(ValueError, match=r"text_encoder= and tokenizer= are missing"):
        ImaginationEngine(cfg, None, t, captioner="clip")
    with pytest.raises(ValueError, match=r"tokenizer= is missing"):
        ImaginationEngine(cfg, None, t, captioner="clip", text_encoder=t)
    with pytest.raises(ValueError, match="scorer"):
        ImaginationEngine(cfg, None, None, captioner="clip", text_encoder=t, tokenizer=t.tokenizer)
    eng = ImaginationEngine(cfg, None, t, captioner="clip", text_encoder=t, tokenizer=t.tokenizer)
    assert isinstance(eng.captioner, caption.ClipCaptioner) and eng.captioner.scorer is t
    assert ImaginationEngine(cfg, None, None, captioner=len).captioner is len and ImaginationEngine(cfg, None, None).captioner is None
