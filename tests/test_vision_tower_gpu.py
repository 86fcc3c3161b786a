"""The vision tower (d2r_clip_embed_pixels: k_patchify, k_gemm / k_gemm8 and the LayerNorm-fold epilogues, k_embed_ln, k_attention_s<1|2|4|8>,
k_attention_cls, k_head) against the float64 reference of tests/vision_ref.py.

The bar of every parity case: per image |got - want|_2 <= BAR_FACTOR x floor, norms within 1e-5 of 1, everything finite; `want` is the
float64 forward and `floor` the largest per-image distance of the ideal bf16-operand forward (rounding where clip.hip rounds, in the
ln_fold / cls_last mode under test) from it on the same pixels and weights.  tests/test_vision_ref_host.py shows that the mutants of the
streamed attention land at more than 2 x BAR_FACTOR x floor on the sweep's inputs.  Every case prints `HIP / floor`;
docs/history/r30.md keeps the measured figures."""
import functools

import numpy as np
import pytest

from dream2real_amd import _lib
from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
from tests import vision_ref

pytestmark = pytest.mark.gpu

D2R_OK, D2R_ERR_INVALID = 0, -1          # include/d2r.h
DEFAULTS = dict(ln_fold=4, cls_last=1, attn_rem=1)      # d2r_internal.h
# ln_fold -> (the residual model it implements, LayerNorm folded into the products)
LN_FOLD = {0: ("exact", False), 1: ("hi_lo", True), 2: ("bf16", True), 3: ("exact", True), 4: ("hi_lo", True)}
WIDE = {
    "b16_x2": dict(CLIP_CONFIGS["vit_b16"], num_layers=2),      # 768 / 12 / 3072, T = 197
    "vit_l14_x2": CLIP_CONFIGS["vit_l14_x2"],                   # 1024 / 16 / 4096, patch 14 (padded patch product), T = 257
    "vit_l14_336_x1": CLIP_CONFIGS["vit_l14_336_x1"],           # T = 577, one block
}


@functools.lru_cache(maxsize=None)
def model(name):
    """(cfg, weights): an image size of the sweep (an int) or a name of WIDE."""
    if isinstance(name, int):
        return vision_ref.sweep_weights(name)
    return WIDE[name], random_clip_state_dict(WIDE[name], seed=6, text=False)


@functools.lru_cache(maxsize=None)
def pixels(name, n=vision_ref.SWEEP_N):
    cfg, sd = model(name)
    if isinstance(name, int):
        pv = vision_ref.sweep_pixels(name, n, sd=sd, cfg=cfg)
    else:
        r = np.random.Generator(np.random.PCG64(3))
        pv = r.standard_normal((n, 3, cfg["image_size"], cfg["image_size"]), dtype=np.float32)
    pv.setflags(write=False)
    return pv


@functools.lru_cache(maxsize=None)
def want_of(name, n):
    cfg, sd = model(name)
    return vision_ref.vision_embeds(pixels(name, n), sd, cfg)


@functools.lru_cache(maxsize=None)
def floor_of(name, n, ln_fold, cls_last):
    """The floor of the rounding model the options select; the float64 result is shared by all of them."""
    cfg, sd = model(name)
    residual, fold = LN_FOLD[ln_fold]
    ideal = vision_ref.vision_embeds(pixels(name, n), sd, cfg, bf16_operands=True, residual=residual, ln_fold=fold, cls_last=bool(cls_last))
    return float(np.linalg.norm(ideal - want_of(name, n), axis=1).max())


@pytest.fixture(scope="module")
def engine():
    from dream2real_amd import engine as e
    return e


@pytest.fixture(scope="module")
def ctx(engine):
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scorer(engine, ctx):
    """One scorer per model for the module."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = engine.ClipScorer(ctx, *model(name))
        return made[name]

    yield get
    for sc in made.values():
        sc.close()


class options:
    """ctx options for a block, the defaults restored afterwards."""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        try:
            for k, v in self.kw.items():
                self.ctx.set_option(k, v)
        except Exception:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for k in self.kw:
            self.ctx.set_option(k, DEFAULTS[k])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_parity(tag, got, name, n, ln_fold=4, cls_last=1):
    """The bar: per image |got - want|_2 <= BAR_FACTOR x floor, unit norms, finite; prints HIP / floor and returns the ratio."""
    cfg, _ = model(name)
    want, floor = want_of(name, n), floor_of(name, n, ln_fold, cls_last)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.isfinite(got).all(), f"{tag}: non-finite output"
    dist = np.linalg.norm(got.astype(np.float64) - want, axis=1)
    worst = int(dist.argmax())
    print(f"[vision] {tag}: T {vision_ref.n_tokens(cfg['image_size'], cfg['patch_size'])} n {n} width {cfg['hidden_size']} ln_fold {ln_fold} "
          f"cls_last {cls_last}: floor {floor:.3e}, HIP max {dist.max():.3e} (image {worst}), HIP / floor = {dist.max() / floor:.2f}")
    np.testing.assert_allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, rtol=0, atol=1e-5)
    over = np.nonzero(dist > vision_ref.BAR_FACTOR * floor)[0]
    assert over.size == 0, f"{tag}: images {over.tolist()} beyond {vision_ref.BAR_FACTOR:g} x floor: {(dist[over] / floor).round(2).tolist()}"
    return dist.max() / floor


# ---- a. the token-count sweep

@pytest.mark.parametrize("image_size", vision_ref.SWEEP_SIZES)
def test_token_count_sweep(ctx, scorer, image_size):
    """T = 2 ... 577 on the two-layer tiny geometry: one to nineteen query tiles (n_qt = 8 g + r with r = 0 ... 7 and g = 0, 1, 2), last
    tiles of 1 ... 31 keys; at cls_last 0 both blocks run the streamed attention, at cls_last 1 the last one is k_attention_cls.  The
    images carry the marked patches of vision_ref.sweep_pixels, so that rows and keys past the first tile reach token 0."""
    sc, pv = scorer(image_size), pixels(image_size)
    for cls_last in (0, 1):
        with options(ctx, cls_last=cls_last):
            got = sc.embed_pixels(pv)
        check_parity(f"a sweep S={image_size}", got, image_size, len(pv), cls_last=cls_last)


# ---- b. the remainder launch

@pytest.mark.parametrize("image_size", [256, 272, 384])
def test_remainder_groups_are_bit_identical_to_full_groups(ctx, scorer, image_size):
    """n_qt = 8 g + r with r = 1, 2, 3 (T = 257, 290, 577; g = 1, 1, 2): attn_rem 0 runs the remainder as one more eight-wave group,
    attn_rem 4 on a workgroup of 1 / 2 / 4 waves starting at tile 8 g; the per-wave arithmetic is the same, so are the bits."""
    sc, pv = scorer(image_size), pixels(image_size)
    with options(ctx, cls_last=0):
        base = sc.embed_pixels(pv)
        for rem in (0, 4):
            with options(ctx, attn_rem=rem):
                got = sc.embed_pixels(pv)
            diff = np.nonzero((bits(got) != bits(base)).any(1))[0]
            print(f"[vision] b attn_rem {rem} S={image_size}: {diff.size} of {len(pv)} images differ in bits from attn_rem {DEFAULTS['attn_rem']}")
            assert diff.size == 0, (rem, diff.tolist())
    check_parity(f"b attn_rem S={image_size}", base, image_size, len(pv), cls_last=0)


# ---- c. the real widths

@pytest.mark.parametrize("name", list(WIDE))
def test_real_widths(ctx, scorer, name):
    """768 / 12 / 3072 at T = 197, 1024 / 16 / 4096 at T = 257 (two blocks) and T = 577 (one block): the persistent 256x256 GEMM, the
    padded patch product of patch 14, 12 and 16 heads per image."""
    sc, pv = scorer(name), pixels(name, 3)
    for cls_last in (0, 1):
        with options(ctx, cls_last=cls_last):
            got = sc.embed_pixels(pv)
        check_parity(f"c {name}", got, name, 3, cls_last=cls_last)


# ---- d. the residual-stream modes

@pytest.mark.parametrize("image_size", [128, 256])
def test_ln_fold_modes_each_against_their_own_floor(ctx, scorer, image_size):
    """ln_fold 0 (LayerNorm kernels, fp32 residual), 1 (hi + lo bf16), 3 (fp32 + bf16 copy), 4 (hi + lo byte) and 2 (bf16 residual alone),
    each held to the floor of the rounding model it implements, at T = 65 and 257, both blocks through the streamed attention."""
    sc, pv = scorer(image_size), pixels(image_size)
    ratios = {}
    for mode in (0, 1, 2, 3, 4):
        with options(ctx, ln_fold=mode, cls_last=0):
            got = sc.embed_pixels(pv)
        ratios[mode] = check_parity(f"d ln_fold S={image_size}", got, image_size, len(pv), ln_fold=mode, cls_last=0)
    print(f"[vision] d S={image_size} HIP / floor by ln_fold: " + ", ".join(f"{m}: {r:.2f}" for m, r in ratios.items()))


# ---- e. row counts around the 256-row GEMM panel

@pytest.mark.parametrize("n", [1, 51, 52, 103])
def test_row_panel_edges(scorer, n):
    """T = 5: n T = 5, 255, 260 and 515 rows on either side of one and two 256-row panels; every image is checked."""
    got = scorer(32).embed_pixels(pixels(32, n))
    check_parity(f"e rows={5 * n}", got, 32, n)


# ---- f. independence

def test_batch_order_and_repetition_change_no_bit(scorer):
    """Every kernel is row- or image-independent at fixed shapes: permuting the batch permutes the output rows bit for bit, and a
    second run of the same batch repeats the first."""
    sc, pv = scorer(144), pixels(144, 12)
    first = sc.embed_pixels(pv)
    again = sc.embed_pixels(pv)
    perm = np.random.Generator(np.random.PCG64(5)).permutation(len(pv))
    moved = sc.embed_pixels(pv[perm])
    d_rep = np.nonzero((bits(again) != bits(first)).any(1))[0]
    d_perm = np.nonzero((bits(moved) != bits(first[perm])).any(1))[0]
    print(f"[vision] f: {d_rep.size} of 12 images changed bits on a second run, {d_perm.size} of 12 after the batch was permuted")
    assert d_rep.size == 0 and d_perm.size == 0, (d_rep.tolist(), d_perm.tolist())
    check_parity("f T=82 n=12", first, 144, 12)


# ---- g. refusals

def test_empty_batch_and_null_output_leave_the_buffer_and_the_scorer_untouched(ctx, scorer):
    """n = 0 is an empty batch: D2R_OK, nothing written.  A null output or null pixels is D2R_ERR_INVALID, nothing written.  The
    next call returns the bits of the one before."""
    sc, pv = scorer(96), pixels(96)
    before = sc.embed_pixels(pv)
    out = np.full((len(pv), sc.cfg["proj"]), 7.0, np.float32)
    host = np.ascontiguousarray(pv)
    assert ctx.lib.d2r_clip_embed_pixels(ctx.h, sc.h, _lib.ptr(host), 0, _lib.ptr(out)) == D2R_OK
    assert (out == 7.0).all()
    assert ctx.lib.d2r_clip_embed_pixels(ctx.h, sc.h, _lib.ptr(host), len(pv), None) == D2R_ERR_INVALID
    assert ctx.lib.d2r_clip_embed_pixels(ctx.h, sc.h, None, len(pv), _lib.ptr(out)) == D2R_ERR_INVALID
    assert (out == 7.0).all()
    after = sc.embed_pixels(pv)
    assert np.array_equal(bits(after), bits(before))
    check_parity("g refusals, then embed", after, 96, len(pv))
