"""The two CLIP tower handles own their device memory: a refused create leaves nothing behind that a later create on the same context
could trip over, destroy + create on one context reproduces the first handle's results bit for bit (the lazily built fp8 weight
copies included), and destroying the tower the context's background rows were computed with un-marks them.  On the smallest towers at
which `vit_fp8` (d % 256 == 0, mlp >= 2 d) and `cls_last` apply: hidden 256, 4 heads, mlp 512, 3 layers, 64 / 16 pixels (17 tokens),
projection 64; text: vocab 64, context 16, the same widths.  No allocation failure is provoked and no memory is measured."""
import ctypes as C

import numpy as np
import pytest

from dream2real_amd import _lib

pytestmark = pytest.mark.gpu

TINY = dict(patch_size=16, hidden_size=256, num_layers=3, num_heads=4, mlp=512, image_size=64, proj=64,
            text_hidden=256, text_layers=3, text_heads=4, text_mlp=512, vocab=64, ctx=16)
INVALID, UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def sd():
    from dream2real_amd.clip_model import random_clip_state_dict
    return random_clip_state_dict(TINY, seed=6)


def _captions(Cn=9, T=16):
    r = np.random.default_rng(11)
    ids = r.integers(1, TINY["vocab"] - 1, (Cn, T)).astype(np.int32)
    ids[np.arange(Cn), r.integers(1, T, Cn)] = TINY["vocab"] - 1          # one EOS (the largest id) per caption
    return ids


def test_text_tower_refusals_leave_the_context_usable(sd):
    """A blob one float short (D2R_ERR_INVALID, "blob size") and a head dimension of 51 (D2R_ERR_UNSUPPORTED); after each, the same
    context creates the good tower and encodes exactly what a fresh context's tower encodes."""
    from dream2real_amd import engine
    from dream2real_amd.clip_model import pack_text_weights
    ids = _captions()
    fresh = engine.Context(0)
    ref = engine.TextEncoder(fresh, TINY, sd)
    want = ref.encode(ids)
    assert np.isfinite(want).all() and np.ptp(want, axis=0).max() > 0
    ctx = engine.Context(0)
    lib = ctx.lib
    blob = pack_text_weights(sd, TINY)

    def desc(heads):
        return _lib.TextDesc(TINY["vocab"], TINY["ctx"], TINY["text_hidden"], TINY["text_layers"], heads, TINY["text_mlp"], TINY["proj"])

    refusals = ((desc(TINY["text_heads"]), blob.size - 1, INVALID, "blob size"), (desc(TINY["text_heads"] + 1), blob.size, UNSUPPORTED, "head_dim 64"))
    for d, n_floats, code, text in refusals:
        out = C.c_void_p()
        assert lib.d2r_text_create(ctx.h, C.byref(d), _lib.ptr(blob), C.c_size_t(n_floats), C.byref(out)) == code
        assert text in lib.d2r_last_error(ctx.h).decode() and not out.value
        t = engine.TextEncoder(ctx, TINY, sd)
        np.testing.assert_array_equal(t.encode(ids), want)
        t.close()
    ref.close(); fresh.close(); ctx.close()


def test_create_score_destroy_create_repeats_the_logits(sd):
    """Vision tower, one context: create -> score -> destroy -> create -> score, bitwise-equal logits and embeddings, without and with
    `vit_fp8` (whose e4m3 weight copies are built on the first forward of each handle); the option does change the logits."""
    from dream2real_amd import engine
    r = np.random.default_rng(4)
    frames = r.integers(0, 256, (9, 54, 96, 3), dtype=np.uint8)          # 9 x 17 rows: past one 128-row panel
    text = r.standard_normal((2, TINY["proj"])).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    ctx = engine.Context(0)
    first = {}
    for fp8 in (0, 1):
        ctx.set_option("vit_fp8", fp8)
        for rnd in range(2):
            sc = engine.ClipScorer(ctx, TINY, sd)
            got = sc.score_frames(frames, text, return_embeds=True)
            sc.close()
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
            if rnd == 0:
                first[fp8] = got
            else:
                np.testing.assert_array_equal(got[0], first[fp8][0])
                np.testing.assert_array_equal(got[1], first[fp8][1])
    assert not np.array_equal(first[0][0], first[1][0])
    ctx.close()


def test_destroying_the_background_rows_tower_unmarks_them(tmp_path, sd):
    """The render-score entry point keeps the background's patches and layer-0 rows per context, marked with the tower they were computed
    with.  Destroy that tower, create one with other weights and call the entry point again: the logits are those of the new tower on
    the rendered frames, bit for bit.  A mark left standing would show only if the allocator handed the second tower the first one's
    address, which nothing guarantees: this exercises destroy-then-score, it does not pin the un-marking in d2r_clip_destroy."""
    from dream2real_amd import combined_rendering, engine
    from dream2real_amd.accio2ngp import converter
    from dream2real_amd.clip_model import random_clip_state_dict
    from dream2real_amd.obj_pose_opt import sample_poses_grid
    from dream2real_amd.virtual_cam_pose_sample import get_virtual_cam_poses
    from synthetic_scenes import make_scene, make_task, scene_text_embeds
    scene = make_scene("shopping")                                       # the tiny scene of tests/test_api_path.py
    ctx = engine.Context(0)
    fg, bg = engine.Testbed(ctx, scene.fg), engine.Testbed(ctx, scene.bg)
    fg.background_color = list(scene.fg_background)
    task = make_task(scene, fg, bg)
    text = scene_text_embeds(np.random.default_rng(3).standard_normal(TINY["proj"]))
    poses = converter(sample_poses_grid(task, [3, 2, 1, 1, 1, 1], scene.scene_type).reshape(-1, 4, 4))
    rp = converter(get_virtual_cam_poses(task, [0]))
    rend = combined_rendering.renderer(str(tmp_path), task, resolution=(96, 54))
    frames = np.stack(rend.render(poses, rp, [0], save=False))
    assert ctx.get_option("l0_reuse") == 1 and ctx.get_option("ln_fold") == 4          # the defaults: both marks get set
    logits = []
    for sd_i in (sd, random_clip_state_dict(TINY, seed=7)):
        sc = engine.ClipScorer(ctx, TINY, sd_i)
        got = rend.render_score(poses, rp, [0], sc, text, save=False)
        np.testing.assert_array_equal(got, sc.score_frames(frames, text, rot90=True))
        logits.append(got)
        sc.close()
    assert not np.array_equal(logits[0], logits[1])
    fg.close(); bg.close(); ctx.close()
