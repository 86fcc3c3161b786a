"""The text tower (d2r_text_create / d2r_text_encode: k_text_embed, k_attention<true>, the GEMMs, k_head with a pool_row) past one
attention tile, against the float64 reference of tests/text_ref.py.

The bar of every parity case: per caption |got - want|_2 <= BAR_FACTOR x floor, where `want` is the float64 forward and `floor` the
largest per-caption distance of the ideal bf16-operand tower from it on the same ids and weights (text_ref.floor_and_want).  The CPU
test tests/test_text_ref_host.py shows that the wrong causal masks that act only past the first 32-row tile land at >= 15 x floor
on the sweep's inputs.  Every case prints `HIP / floor`; docs/history/r17.md keeps the measured figures."""
import functools

import numpy as np
import pytest

from dream2real_amd import _lib
from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
from tests import text_ref

pytestmark = pytest.mark.gpu

D2R_ERR_INVALID = -1          # include/d2r.h

SWEEP_CFG = dict(CLIP_CONFIGS["vit_tiny"], **text_ref.SWEEP_OVERRIDE)
LONG_CFG = dict(SWEEP_CFG, ctx=512)
WIDE = {   # the text geometries of ViT-B/16 and ViT-L/14 at two layers (vision side: the tiny one, unused)
    "b16_text": dict(CLIP_CONFIGS["vit_tiny"], text_hidden=512, text_heads=8, text_mlp=2048, proj=512, vocab=49408, ctx=77, text_layers=2),
    "l14_text": dict(CLIP_CONFIGS["vit_tiny"], text_hidden=768, text_heads=12, text_mlp=3072, proj=768, vocab=49408, ctx=77, text_layers=2),
}
WIDE_EOS = [0, 1, 31, 32, 33, 63, 64, 65, 76]      # nine captions: two full k_head blocks and a remainder of one


@functools.lru_cache(maxsize=None)
def weights(name):
    cfg = {"sweep": SWEEP_CFG, "long": LONG_CFG, **WIDE}[name]
    return cfg, random_clip_state_dict(cfg, seed=6)


@pytest.fixture(scope="module")
def engine():
    from dream2real_amd import engine as e
    return e


@pytest.fixture(scope="module")
def ctx(engine):
    c = engine.Context(0)
    yield c
    c.close()


def encoder_fixture(name):
    @pytest.fixture(scope="module")
    def fx(engine, ctx):
        cfg, sd = weights(name)
        enc = engine.TextEncoder(ctx, cfg, sd)
        yield enc
        enc.close()
    return fx


sweep_enc = encoder_fixture("sweep")
long_enc = encoder_fixture("long")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_REFS = {}


def reference(ids, name):
    """(want, floor) of text_ref.floor_and_want, computed once per (weights, ids)."""
    key = (name, ids.shape, ids.tobytes())
    if key not in _REFS:
        cfg, sd = weights(name)
        _REFS[key] = text_ref.floor_and_want(ids, sd, cfg)
    return _REFS[key]


def check_parity(tag, got, ids, name):
    """The bar: per caption |got - want|_2 <= BAR_FACTOR x floor, unit norms; prints HIP / floor."""
    cfg, _ = weights(name)
    want, floor = reference(ids, name)
    assert got.shape == want.shape and np.isfinite(got).all()
    dist = np.linalg.norm(got.astype(np.float64) - want, axis=1)
    worst = int(dist.argmax())
    print(f"[text] {tag}: T {ids.shape[1]} Cn {ids.shape[0]} width {cfg['text_hidden']}: floor {floor:.3e}, HIP max {dist.max():.3e} "
          f"(caption {worst}, end token at {int(ids[worst].argmax())}), HIP / floor = {dist.max() / floor:.2f}")
    np.testing.assert_allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, rtol=0, atol=1e-5)
    over = np.nonzero(dist > text_ref.BAR_FACTOR * floor)[0]
    assert over.size == 0, f"captions {over.tolist()} beyond {text_ref.BAR_FACTOR:g} x floor: {(dist[over] / floor).round(2).tolist()}"
    return want


# ---- a. every query row at every tile-boundary length

@pytest.mark.parametrize("T", [1, 31, 32, 33, 64, 65, 76, 77])
def test_every_query_row_at_tile_boundary_lengths(sweep_enc, T):
    """Cn = T captions, caption c with its end token at position c: pooling reads every row of the causal attention, sequences start at
    rows c * T (unaligned to the 32-row tiles and the 256-row GEMM padding); T = 77 is 20 k_head blocks, the last with one item."""
    ids = text_ref.sweep_ids(T, SWEEP_CFG["vocab"])
    check_parity(f"a sweep T={T}", sweep_enc.encode(ids), ids, "sweep")


# ---- b. the real widths

@pytest.mark.parametrize("name", ["b16_text", "l14_text"])
def test_real_text_widths_at_context_77(engine, ctx, name):
    """Width 512 / 8 heads / MLP 2048 and width 768 / 12 heads / MLP 3072 (the product's own text geometry), vocabulary 49408, T = 77,
    end tokens on both sides of every tile boundary; the 768 model's QKV and fc1 run on the persistent 256x256 kernel."""
    cfg, sd = weights(name)
    enc = engine.TextEncoder(ctx, cfg, sd)
    try:
        ids = text_ref.eos_ids(WIDE_EOS, 77, cfg["vocab"])
        check_parity(f"b {name}", enc.encode(ids), ids, name)
    finally:
        enc.close()


# ---- c. long contexts: more query tiles than waves, more than 64 KiB of LDS

def long_positions(T, n=12):
    fixed = [p for p in (0, 255, 256, 287, 288, T - 1) if p < T]
    r = np.random.Generator(np.random.PCG64(1000 + T))
    rest = [int(p) for p in r.permutation(T) if p not in fixed][:n - len(set(fixed))]
    return sorted(set(fixed)) + rest


@pytest.mark.parametrize("T", [257, 289, 512])
def test_long_contexts(long_enc, T):
    """T = 257 / 289: 9 / 10 query tiles for the 8 waves (the query reload) and a last key tile with one valid key; 289 needs ~82 KiB of
    LDS and 512 ~131 KiB (the opt-in past 64 KiB)."""
    ids = text_ref.eos_ids(long_positions(T), T, LONG_CFG["vocab"])
    assert ids.shape[0] == 12
    check_parity(f"c long T={T}", long_enc.encode(ids), ids, "long")


# ---- d. causality is exact

def test_tokens_after_the_end_token_and_caption_order_change_no_bit(sweep_enc):
    """Masked scores are -inf and P exactly 0, every other kernel is row-independent at fixed shapes: replacing every token after each
    caption's end token leaves the embeddings bit-identical, and permuting the captions permutes the output rows bit for bit."""
    T, V = 77, SWEEP_CFG["vocab"]
    ids = text_ref.sweep_ids(T, V)
    first = sweep_enc.encode(ids)
    r = np.random.Generator(np.random.PCG64(5))
    other = ids.copy()
    tail = np.arange(T)[None, :] > np.arange(T)[:, None]
    other[tail] = (ids[tail] + r.integers(1, V - 1, size=int(tail.sum()))) % (V - 1)      # another id, still below the end token
    assert (other[tail] != ids[tail]).all() and (other.argmax(1) == np.arange(T)).all()
    second = sweep_enc.encode(other)
    diff = np.nonzero((bits(first) != bits(second)).any(1))[0]
    print(f"[text] d causality: {diff.size} of {T} captions changed bits after their tails were replaced")
    assert diff.size == 0, diff.tolist()
    perm = r.permutation(T)
    moved = sweep_enc.encode(ids[perm])
    diff = np.nonzero((bits(moved) != bits(first[perm])).any(1))[0]
    print(f"[text] d permutation: {diff.size} of {T} captions changed bits after the batch was permuted")
    assert diff.size == 0, diff.tolist()


# ---- e. ids

def test_two_end_tokens_negative_and_oversized_ids(sweep_enc):
    """Pooling is at the first maximum of the raw ids; the lookup uses the id clipped to [0, vocab - 1]."""
    T, V = 77, SWEEP_CFG["vocab"]
    ids = text_ref.eos_ids([10, 40, 20, 60], T, V)
    ids[0, 50] = V - 1                       # a second end token: pooled at 10
    ids[1, 3] = -7                           # encodes like id 0
    ids[2, 45] = V + 40                      # encodes like V - 1 and is the maximum: pooled at 45, past the end token at 20
    ids[3, 61] = -1
    assert ids.argmax(1).tolist() == [10, 40, 45, 60]
    got = sweep_enc.encode(ids)
    check_parity("e ids", got, ids, "sweep")
    clipped = ids.copy()
    clipped[1, 3] = 0
    assert np.array_equal(bits(sweep_enc.encode(clipped)[1]), bits(got[1]))


# ---- error codes: the bad-shape returns, and the encoder afterwards

def test_bad_caption_batch_shapes_are_invalid_and_leave_the_encoder_working(ctx, sweep_enc):
    T = 77
    ids = text_ref.sweep_ids(T, SWEEP_CFG["vocab"])[:5]
    before = sweep_enc.encode(ids)
    big = np.zeros((5, 80), np.int32)
    out = np.full((5, SWEEP_CFG["proj"]), 7.0, np.float32)
    for Cn, Tn in ((0, T), (5, 0), (5, T + 1)):
        rc = ctx.lib.d2r_text_encode(ctx.h, sweep_enc.h, _lib.ptr(big), Cn, Tn, _lib.ptr(out))
        assert rc == D2R_ERR_INVALID, (Cn, Tn, rc)
        assert (out == 7.0).all()
    with pytest.raises(_lib.D2RError):
        sweep_enc.encode(big[:, :78])
    after = sweep_enc.encode(ids)
    assert np.array_equal(bits(after), bits(before))
    check_parity("error codes, then encode", after, ids, "sweep")


# ---- f. shared workspaces

def test_text_and_vision_towers_share_workspaces_without_a_trace(engine):
    """The text tower runs in the context's clipws[1..5], pix and logits buffers, which the vision tower also uses.  On a fresh context
    (so that the wide text run is the one that grows the workspaces): score_frames, encode, score_frames -> the same scores and image
    embeddings bit for bit; encode, score_frames, encode -> the same text embeddings bit for bit."""
    vcfg = CLIP_CONFIGS["vit_tiny"]
    vsd = random_clip_state_dict(vcfg, seed=6)
    tcfg, tsd = weights("l14_text")
    r = np.random.Generator(np.random.PCG64(31))
    frames = r.integers(0, 256, size=(3, 54, 96, 3), dtype=np.uint8)
    text = r.standard_normal((2, vcfg["proj"])).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    ids = text_ref.eos_ids(WIDE_EOS, 77, tcfg["vocab"])
    c = engine.Context(0)
    try:
        sc, enc = engine.ClipScorer(c, vcfg, vsd), engine.TextEncoder(c, tcfg, tsd)
        lg0, em0 = sc.score_frames(frames, text, return_embeds=True)
        e0 = enc.encode(ids)
        lg1, em1 = sc.score_frames(frames, text, return_embeds=True)
        e1 = enc.encode(ids)
        sc.close()
        enc.close()
    finally:
        c.close()
    assert np.isfinite(lg0).all() and np.isfinite(e0).all()
    vision_same = np.array_equal(bits(lg0), bits(lg1)) and np.array_equal(bits(em0), bits(em1))
    text_same = np.array_equal(bits(e0), bits(e1))
    print(f"[text] f shared workspaces: vision bitwise {vision_same}, text bitwise {text_same}")
    assert vision_same and text_same
    check_parity("f l14_text between two vision runs", e1, ids, "l14_text")
