"""The drop-in API runs the path that is benchmarked: `optimise_pose_grid` / `renderer.render_score` go
through ONE fused library call (d2r_render_score_host) — chunked, two-stream, frames streamed to cb_render/*.png by the
library — and produce exactly what the reference's two-step route (`renderer.render`, then CLIP on the frames:
reference clip_scoring.py:136-185) produces: bit-identical frames, logits, scores, files.  Host-only parts (PNG codec,
renderer snapshot mode plumbing) run without a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dream2real_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ host only

def test_png_default_encoder_is_a_valid_deflate_stream_on_hard_inputs(tmp_path):
    """The default encoding (Sub filter + the library's own Huffman-only deflate block, pngio.cpp) through a foreign inflater (PIL /
    zlib): incompressible bytes (codes of 8-9 bits), constant images (a two-symbol code), one pixel, a byte distribution whose Huffman
    tree is deeper than deflate's 15-bit limit (Fibonacci counts: the length-limiting fallback), and every explicit zlib level."""
    from PIL import Image
    r = np.random.default_rng(5)
    fib = [1, 1]
    while len(fib) < 27:
        fib.append(fib[-1] + fib[-2])
    vals = np.concatenate([np.full(f, i, np.uint8) for i, f in enumerate(fib)])
    r.shuffle(vals)
    v = vals[:(vals.size // 3072) * 3072].reshape(-1, 1024, 3).astype(np.int64)
    cases = {"random": r.integers(0, 256, (90, 160, 3), dtype=np.uint8), "zeros": np.zeros((54, 96, 3), np.uint8),
             "one pixel": np.full((1, 1, 3), 7, np.uint8), "constant": np.full((3, 5, 3), 255, np.uint8),
             "deep tree": (np.cumsum(v, axis=1) % 256).astype(np.uint8),            # after the Sub filter the bytes are `vals`
             "gradient": np.add.outer(np.arange(64), np.arange(200))[..., None].repeat(3, -1).astype(np.uint8)}
    for name, img in cases.items():
        for level in (-1, 0, 1, 6):
            path = str(tmp_path / "t.png")
            _lib.png_write(img, path, level)
            np.testing.assert_array_equal(np.asarray(Image.open(path).convert("RGB")), img, err_msg=f"{name} level {level}")
    path = str(tmp_path / "t.png")
    _lib.png_write(cases["gradient"], path)
    small = os.path.getsize(path)
    _lib.png_write(cases["gradient"], path, 0)
    assert small * 4 < os.path.getsize(path)                                      # the Sub filter turns a gradient into a constant


def test_png_codec_roundtrip_and_foreign_files(tmp_path):
    """d2r_png_write_batch / read_batch against PIL both ways: our files decode to the same pixels in PIL; PIL's files
    (adaptive filters, RGBA, grey) decode to the same pixels here; missing / wrong-size files are named errors."""
    from PIL import Image
    r = np.random.default_rng(0)
    fr = r.integers(0, 256, (12, 54, 96, 3), dtype=np.uint8)
    fr[:, :20] = 7                                            # long runs: exercises the deflate side
    fr[3] = np.linspace(0, 255, 54 * 96 * 3).reshape(54, 96, 3).astype(np.uint8)    # smooth ramp: PIL picks sub / paeth filters
    d = str(tmp_path)
    _lib.png_write_batch(fr, d, first_index=3, threads=4)
    assert sorted(os.listdir(d)) == [f"cb_rgb_{i:04d}.png" for i in range(3, 15)]
    for i in range(12):
        np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(d, f"cb_rgb_{i + 3:04d}.png"))), fr[i])
    np.testing.assert_array_equal(_lib.png_read_batch(d, 12, first_index=3), fr)
    np.testing.assert_array_equal(_lib.png_read_batch(d, indices=[14, 3, 9]), fr[[11, 0, 6]])
    for k, img in enumerate((fr[3], np.dstack([fr[1], fr[1][..., :1]]), fr[2][..., 0])):          # RGB (filtered), RGBA, grey
        Image.fromarray(img).save(os.path.join(d, f"cb_rgb_{100 + k:04d}.png"))
    b = _lib.png_read_batch(d, 3, first_index=100)
    np.testing.assert_array_equal(b[0], fr[3])
    np.testing.assert_array_equal(b[1], fr[1])
    np.testing.assert_array_equal(b[2], np.repeat(fr[2][..., :1], 3, axis=2))
    _lib.png_write(fr[5], os.path.join(d, "best_render.png"))
    np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(d, "best_render.png"))), fr[5])
    assert _lib.png_size(os.path.join(d, "best_render.png")) == (96, 54)
    with pytest.raises(_lib.D2RError, match="cb_rgb_005"):
        _lib.png_read_batch(d, 2, first_index=50, size=(96, 54))
    Image.fromarray(fr[0][:10]).save(os.path.join(d, "cb_rgb_0200.png"))
    with pytest.raises(_lib.D2RError, match="expected 96x54"):
        _lib.png_read_batch(d, 1, first_index=200, size=(96, 54))
    open(os.path.join(d, "cb_rgb_0300.png"), "wb").write(b"not a png at all, but long enough to be read as one maybe....")
    with pytest.raises(_lib.D2RError, match="not a PNG"):
        _lib.png_read_batch(d, 1, first_index=300, size=(96, 54))
    im = Image.fromarray(fr[0]).convert("P")
    im.save(os.path.join(d, "cb_rgb_0400.png"))
    with pytest.raises(_lib.D2RError, match="unsupported PNG"):
        _lib.png_read_batch(d, 1, first_index=400, size=(96, 54))


def test_png_background_delta_encoder_writes_the_same_pixels(tmp_path):
    """d2r_png_write_batch_bg (round 5): frames that equal a background frame except in a band of scanlines — what a render-and-score
    pass streams out — re-code only the scanlines that differ; the background's scanlines are entropy-coded once with one shared Huffman
    code.  Through a foreign inflater (PIL) every file must hold exactly its frame: no row changed, one pixel changed, a band, every row
    changed (noise: codes of 8-9 bits with a code built for other statistics), a one-pixel-wide and a one-row image, a constant background
    (two-symbol statistics, every other literal kept alive by the floor count), and rows whose bit strings end on every bit offset."""
    import time
    from PIL import Image
    r = np.random.default_rng(9)

    def check(bg, frames, tag):
        d = str(tmp_path / tag)
        os.makedirs(d)
        _lib.png_write_batch_bg(frames, bg, d, first_index=7, threads=3)
        for i, f in enumerate(frames):
            got = np.asarray(Image.open(os.path.join(d, f"cb_rgb_{i + 7:04d}.png")).convert("RGB"))
            np.testing.assert_array_equal(got, f, err_msg=f"{tag} frame {i}")
        np.testing.assert_array_equal(_lib.png_read_batch(d, len(frames), first_index=7), frames)        # and through the library's own reader
        return d

    H, W = 90, 160
    yy, xx = np.mgrid[0:H, 0:W]
    bg = np.stack([(xx * 3 + yy) % 256, (yy * 5) % 256, (xx + 2 * yy) // 3 % 256], -1).astype(np.uint8)
    bg[40:60] = r.integers(0, 256, (20, W, 3), dtype=np.uint8)             # a noisy stripe: long codes in the background itself
    frames = np.repeat(bg[None], 7, 0).copy()
    frames[1, 45, 80, 1] ^= 0x55                                            # one pixel
    frames[2, 30:55, 50:90] = r.integers(0, 256, (25, 40, 3), dtype=np.uint8)   # a band (the object's rectangle)
    frames[3] = r.integers(0, 256, (H, W, 3), dtype=np.uint8)               # every row differs
    frames[4, 0] = 255 - frames[4, 0]                                       # first row
    frames[5, H - 1] = 0                                                    # last row
    frames[6, ::2] = frames[6, ::2][:, ::-1]                                # every other row
    d = check(bg, frames, "band")
    # the delta file of an untouched frame is no larger than the plain encoder's by more than the floor counts cost
    _lib.png_write(frames[0], str(tmp_path / "plain.png"))
    s_delta, s_plain = os.path.getsize(os.path.join(d, "cb_rgb_0007.png")), os.path.getsize(tmp_path / "plain.png")
    assert s_delta <= s_plain * 1.03 + 64, (s_delta, s_plain)
    check(np.full((5, 1, 3), 9, np.uint8), np.stack([np.full((5, 1, 3), 9, np.uint8), r.integers(0, 256, (5, 1, 3), dtype=np.uint8)]), "one_wide")
    check(np.zeros((1, 33, 3), np.uint8), np.stack([np.zeros((1, 33, 3), np.uint8), r.integers(0, 256, (1, 33, 3), dtype=np.uint8)]), "one_row")
    const = np.full((24, 31, 3), 200, np.uint8)
    fr = np.repeat(const[None], 3, 0).copy()
    fr[1, 10:14] = r.integers(0, 256, (4, 31, 3), dtype=np.uint8)
    fr[2, 5, 5] = (1, 2, 3)
    check(const, fr, "constant")
    # speed, for the record (640x360 frames with a 90-row band changed, one thread): delta against plain
    H, W = 360, 640
    bgL = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
    bgL = (bgL // 8 + np.stack([(np.mgrid[0:H, 0:W][1] // 3) % 200] * 3, -1)).astype(np.uint8)          # smooth-ish with texture
    fl = np.repeat(bgL[None], 24, 0).copy()
    for i in range(24):
        fl[i, 100 + i:190 + i, 200:320] = r.integers(0, 256, (90, 120, 3), dtype=np.uint8)
    dd, dp = str(tmp_path / "speed_delta"), str(tmp_path / "speed_plain")
    os.makedirs(dd); os.makedirs(dp)
    t0 = time.perf_counter(); _lib.png_write_batch_bg(fl, bgL, dd, threads=1); t1 = time.perf_counter()
    _lib.png_write_batch(fl, dp, threads=1); t2 = time.perf_counter()
    np.testing.assert_array_equal(_lib.png_read_batch(dd, 24), fl)
    sz = lambda q: sum(os.path.getsize(os.path.join(q, f)) for f in os.listdir(q))
    print(f"[png] 24 frames 640x360, 90-row band changed, one thread: delta {(t1 - t0) * 1e3:.0f} ms ({sz(dd) // 24} B / file), plain {(t2 - t1) * 1e3:.0f} ms ({sz(dp) // 24} B / file)")


def test_cached_renders_are_read_in_sorted_name_order(tmp_path):
    """use_cache_renders reads cb_render/ in SORTED NAME order like the reference (clip_scoring.py:97): index order up
    to 9999, lexical beyond it."""
    from dream2real_amd import clip_scoring
    d = str(tmp_path)
    idx = [0, 1, 2, 9999, 10000, 10001]
    for i in idx:
        _lib.png_write(np.full((4, 6, 3), i % 251, np.uint8), os.path.join(d, f"cb_rgb_{i:04d}.png"))
    n, read = clip_scoring._cached_render_reader(d)
    want = [int(f[7:-4]) % 251 for f in sorted(os.listdir(d))]            # 0000 0001 0002 10000 10001 9999
    assert n == 6 and want == [0, 1, 2, 10000 % 251, 10001 % 251, 9999 % 251]
    assert [int(f[0, 0, 0]) for f in read(0, 6)] == want and [int(f[0, 0, 0]) for f in read(3, 5)] == want[3:5]


def test_convert_poses_writes_render_transforms(tmp_path):
    """renderer.convert_poses (reference combined_rendering.py:211-247) on hand-written transforms files."""
    from dream2real_amd.combined_rendering import INTRINSICS_CLIP_VIEW, renderer
    m = (np.eye(4) + np.arange(16).reshape(4, 4) * 0.01).tolist()
    for name in ("bg", "fg"):
        json.dump({"fl_x": 1.0, "w": 1280, "h": 720, "aabb_scale": 1, "frames": [{"file_path": f"{i}.png", "transform_matrix": m} for i in range(3)]},
                  open(tmp_path / f"{name}_transforms.json", "w"))
    r = renderer.__new__(renderer)
    r.root = str(tmp_path)
    r.convert_poses()
    bg = json.load(open(tmp_path / "bg_render_transforms.json"))
    fg = json.load(open(tmp_path / "fg_render_transforms.json"))
    assert len(bg["frames"]) == 1 and len(fg["frames"]) == 3 and bg["w"] == bg["h"] == fg["w"] == 336
    assert bg["fl_x"] == INTRINSICS_CLIP_VIEW[0, 0] and fg["cy"] == 168.0 and bg["aabb_scale"] == 1
    for i, f in enumerate(fg["frames"]):
        want = np.array(m)
        want[2, 3] -= 0.02 * i
        want[1, 3] -= 0.02 * i
        np.testing.assert_allclose(np.array(f["transform_matrix"]), want, rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="ctx"):
        renderer(str(tmp_path))                        # snapshot mode needs a context to load the .ingp files with
    from dream2real_amd.ngp_visual_model import get_vis_ngps
    with pytest.raises(NotImplementedError, match="NeRF training"):
        get_vis_ngps(None, None, 0, use_cache=False, data_dir=str(tmp_path))
    with pytest.raises(ValueError, match="ctx"):
        get_vis_ngps(None, None, 0, use_cache=True, data_dir=str(tmp_path))


# ------------------------------------------------------------------ GPU

def _setup(W=96, H=54, clip="vit_tiny", lens=None):
    from dream2real_amd import engine
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    from synthetic_scenes import make_scene, make_task, scene_text_embeds
    scene = make_scene("shopping", lens=lens)
    ctx = engine.Context(0)
    if lens is None:
        fg, bg = engine.Testbed(ctx, scene.fg), engine.Testbed(ctx, scene.bg)
        fg.background_color = list(scene.fg_background)
    else:
        fg, bg = scene.testbeds(ctx)            # with the scene's training views: their lens is the render lens, as in smoke()
    cfg = CLIP_CONFIGS[clip]
    sc = engine.ClipScorer(ctx, cfg, random_clip_state_dict(cfg, seed=6))
    task = make_task(scene, fg, bg)
    text = scene_text_embeds(np.random.default_rng(3).standard_normal(cfg["proj"]))
    return scene, ctx, fg, bg, sc, task, text


@pytest.mark.gpu
def test_fused_call_is_bit_identical_to_render_then_score(tmp_path):
    """renderer.render_score (one d2r_render_score_host call: 5 chunks of 16 through the two-stream pipeline, frames
    streamed back through the pinned double buffer, PNGs written by the library) == renderer.render + score_frames:
    frames, logits and files bit for bit, with the pipeline's overlap on and off."""
    _check_fused_call_against_render_then_score(tmp_path, lens=None)


@pytest.mark.gpu
def test_fused_call_through_a_lens_is_bit_identical_to_render_then_score(tmp_path):
    """The same on the scene smoke() uses, whose views carry the reference configs' OpenCV lens: the view's table of
    undistorted directions is built once before the chunk loop, and one chunk / several chunks / overlap on all read it."""
    from dream2real_amd.scene import DEMO_LENS
    _check_fused_call_against_render_then_score(tmp_path, lens=DEMO_LENS)


def _check_fused_call_against_render_then_score(tmp_path, lens):
    from PIL import Image
    from dream2real_amd import combined_rendering
    from dream2real_amd.accio2ngp import converter
    from dream2real_amd.obj_pose_opt import sample_poses_grid
    from dream2real_amd.virtual_cam_pose_sample import get_virtual_cam_poses
    scene, ctx, fg, bg, sc, task, text = _setup(lens=lens)
    poses = converter(sample_poses_grid(task, [9, 8, 1, 1, 1, 1], scene.scene_type).reshape(-1, 4, 4))      # 72
    rp = converter(get_virtual_cam_poses(task, [0]))
    rend = combined_rendering.renderer(str(tmp_path), task, resolution=(96, 54))
    frames_ref = np.stack(rend.render(poses, rp, [0], save=False))
    assert bool(rend._last[0].lens_mode) == (lens is not None)      # the lens reached the view the library renders
    logits_ref = sc.score_frames(frames_ref, text, rot90=True)
    ctx.set_option("chunk", 16)
    for overlap in (1, 0):
        ctx.set_option("overlap", overlap)
        logits, frames = rend.render_score(poses, rp, [0], sc, text, save=True, first_index=5, return_frames=True)
        np.testing.assert_array_equal(frames, frames_ref)
        np.testing.assert_array_equal(logits, logits_ref)
        names = sorted(os.listdir(rend.out_render_path))
        assert names == [f"cb_rgb_{i:04d}.png" for i in range(5, 77)]
        for i in (0, 15, 16, 47, 71):                         # chunk boundaries included
            np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(rend.out_render_path, names[i]))), frames_ref[i])
        # scores only: no frames leave the GPU, same logits; a ragged last chunk (72 = 4 x 16 + 8 above, 3 x 20 + 12 here)
        ctx.set_option("chunk", 20)
        np.testing.assert_array_equal(rend.render_score(poses, rp, [0], sc, text, save=False), logits_ref)
        ctx.set_option("chunk", 16)
    np.testing.assert_array_equal(rend.render_one(poses[33]), frames_ref[33])
    with pytest.raises(_lib.D2RError, match="cannot open"):   # a PNG job that fails is reported, not swallowed
        from dream2real_amd.engine import render_score_host
        view, cam = rend._last
        render_score_host(ctx, fg, sc, view, rend._T_WO_1(), cam, poses[:4], text, png_dir=str(tmp_path / "no_such_dir"))
    sc.close(); fg.close(); bg.close(); ctx.close()


@pytest.mark.gpu
def test_optimise_pose_grid_fused_equals_two_step(tmp_path):
    """optimise_pose_grid through the fused call == through the reference's two-step route (a renderer without
    render_score): scores, best pose, best_render.png, cb_render files; with sensor depth + movable mask as the
    background depth (the caller always passes depths_gt, reference dream2real.py:117-118,344); then use_cache_renders
    on the files the fused call wrote gives the same scores again."""
    from PIL import Image
    from dream2real_amd import clip_scoring, combined_rendering
    scene, ctx, fg, bg, sc, task, text = _setup()
    task.text_embeds = text
    r = np.random.default_rng(1)
    depths = [(0.55 + 0.1 * r.random((72, 128))).astype(np.float32)]
    mask = np.ones((72, 128), np.uint8)
    mask[20:50, 40:90] = 0
    task.movable_masks = [mask]
    res = [6, 5, 2, 1, 1, 1]
    invalid = np.zeros(60, bool)
    invalid[[0, 17, 44]] = True

    def phys(pose_batch, tm, valid):
        import torch
        return valid & ~torch.from_numpy(invalid)

    class TwoStep:                                              # the same renderer, without the fused entry
        def __init__(self, inner):
            self.inner = inner

        def render(self, *a, **k):
            return self.inner.render(*a, **k)

        def wait_saved(self):
            self.inner.wait_saved()

    ctx.set_option("chunk", 16)
    out = {}
    for name in ("fused", "two_step"):
        d = str(tmp_path / name)
        os.makedirs(d)
        rend = combined_rendering.renderer(d, task, resolution=(96, 54))
        best, pb, scores = clip_scoring.optimise_pose_grid(rend if name == "fused" else TwoStep(rend), depths, [0], task, d, sample_res=res,
                                                           phys_check=phys, scene_type=scene.scene_type, scorer=sc)
        files = sorted(os.listdir(os.path.join(d, "cb_render")))
        out[name] = (best.numpy(), scores.numpy(), _lib.png_read_batch(os.path.join(d, "cb_render"), len(files)),
                     np.asarray(Image.open(os.path.join(d, "best_render.png"))))
        assert len(files) == 57 and (scores.numpy()[invalid] == 0).all() and (scores.numpy()[~invalid] != 0).all()
    for a, b in zip(out["fused"], out["two_step"]):
        np.testing.assert_array_equal(a, b)
    # cached renders: scores from the files alone
    d = str(tmp_path / "fused")
    np.savetxt(os.path.join(d, "pose_scores.txt"), out["fused"][1])
    _, _, s2 = clip_scoring.optimise_pose_grid(None, None, [0], task, d, sample_res=res, scene_type=scene.scene_type,
                                               use_cache_renders=True, scorer=sc)
    np.testing.assert_array_equal(s2.numpy(), out["fused"][1])
    sc.close(); fg.close(); bg.close(); ctx.close()


def _run_api_bench(tmp_path, tag, *flags, timeout=900):
    root = str(tmp_path / tag)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--api", "--api-dir", root, "--steps", "1", "--warmup", "0", *flags],
                       env=env, capture_output=True, text=True, timeout=timeout, cwd=REPO)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), os.path.join(root, "run")


@pytest.mark.gpu
def test_api_bench_two_ranks_equal_one(tmp_path):
    """`bench.py --api` (ImaginationEngine.dream_best_pose with the physics pre-filter on the mesh files) on one rank and
    pose-sharded over two ranks (sharing this box's GPU: gloo gather; on two GPUs: d2r_allgather_scores): the same
    pose_scores.txt, goal_pose.txt and the same PNG per valid pose, each rank having written its own block."""
    common = ["--sample-res", "9,8,2,1,1,1", "--clip", "vit_tiny", "--width", "96", "--height", "54", "--api-save", "1", "--chunk", "16"]
    o1, d1 = _run_api_bench(tmp_path, "one", *common)
    o2, d2 = _run_api_bench(tmp_path, "two", "--gpus", "2", *common)
    assert o1["n_gpus"] == 1 and o2["n_gpus"] == 2 and o1["config"]["poses_sampled"] == 144
    assert 10 < o1["config"]["poses_valid"] < 144 and o1["config"]["physics"] and o1["value"] > 0
    assert o1["config"]["poses_valid"] == o2["config"]["poses_valid"] and o1["argmax_pose"] == o2["argmax_pose"]
    for name in ("pose_scores.txt", "goal_pose.txt", "pose_batch.txt"):
        np.testing.assert_array_equal(np.loadtxt(os.path.join(d1, name)), np.loadtxt(os.path.join(d2, name)))
    f1, f2 = sorted(os.listdir(os.path.join(d1, "cb_render"))), sorted(os.listdir(os.path.join(d2, "cb_render")))
    assert f1 == f2 == [f"cb_rgb_{i:04d}.png" for i in range(o1["config"]["poses_valid"])]
    n = len(f1)
    np.testing.assert_array_equal(_lib.png_read_batch(os.path.join(d1, "cb_render"), n), _lib.png_read_batch(os.path.join(d2, "cb_render"), n))
    assert open(os.path.join(d1, "best_render.png"), "rb").read() == open(os.path.join(d2, "best_render.png"), "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("clip,W,H,n", [("vit_b16", 640, 360, 40), ("vit_tiny", 96, 54, 72), ("vit_l14_x2", 336, 336, 12)])
def test_layer0_background_token_reuse_is_bit_identical(clip, W, H, n, tmp_path):
    """"l0_reuse": patch embedding, pre-LayerNorm rows and layer-0 q / k / v of the patches a candidate cannot have touched are
    broadcast from the background's own rows, the products run on the touched tokens only (a device-sized compact list).  The
    logits must be BIT-IDENTICAL to the plain forward — in one chunk, in several chunks, with the two-stream pipeline on —
    and the touched fraction must be small on this scene (the point of the exercise)."""
    from dream2real_amd import combined_rendering
    from dream2real_amd.accio2ngp import converter
    from dream2real_amd.obj_pose_opt import sample_poses_grid
    from dream2real_amd.virtual_cam_pose_sample import get_virtual_cam_poses
    scene, ctx, fg, bg, sc, task, text = _setup(W, H, clip)
    res = {40: [8, 5, 1, 1, 1, 1], 72: [9, 8, 1, 1, 1, 1], 12: [4, 3, 1, 1, 1, 1]}[n]
    poses = converter(sample_poses_grid(task, res, scene.scene_type).reshape(-1, 4, 4))
    rp = converter(get_virtual_cam_poses(task, [0]))
    rend = combined_rendering.renderer(str(tmp_path), task, resolution=(W, H))
    try:
        ctx.set_option("l0_reuse", 0)
        base = rend.render_score(poses, rp, [0], sc, text, save=False)
        for chunk, overlap in ((4096, 0), (16, 0), (16, 1)):
            ctx.set_option("l0_reuse", 1)
            ctx.set_option("chunk", chunk)
            ctx.set_option("overlap", overlap)
            got = rend.render_score(poses, rp, [0], sc, text, save=False)
            np.testing.assert_array_equal(got, base, err_msg=f"chunk {chunk} overlap {overlap}")
        assert np.ptp(base[:, 0]) > 0                                     # the candidates do differ
    finally:
        ctx.set_option("l0_reuse", 1); ctx.set_option("chunk", 4096); ctx.set_option("overlap", 0)
        sc.close(); fg.close(); bg.close(); ctx.close()


@pytest.mark.gpu
def test_fused_call_edge_cases(tmp_path):
    """Ragged and degenerate pose batches through d2r_render_score_host with layer-0 reuse on: no candidate (K = 0), one
    candidate, and candidates whose object is off screen (an EMPTY touched-token list: every token row is the background's) mixed
    with visible ones — each equal to the two-step route bit for bit."""
    from dream2real_amd import combined_rendering
    from dream2real_amd.accio2ngp import converter
    from dream2real_amd.obj_pose_opt import sample_poses_grid
    from dream2real_amd.virtual_cam_pose_sample import get_virtual_cam_poses
    scene, ctx, fg, bg, sc, task, text = _setup()
    rp = converter(get_virtual_cam_poses(task, [0]))
    rend = combined_rendering.renderer(str(tmp_path), task, resolution=(96, 54))
    poses_w = sample_poses_grid(task, [3, 2, 1, 1, 1, 1], scene.scene_type).reshape(-1, 4, 4)
    far = poses_w.copy()
    far[:, :3, 3] += np.array([5.0, 5.0, 0.0], np.float32)                 # metres away: outside every view
    for name, pw in (("none", poses_w[:0]), ("one", poses_w[:1]), ("off screen", far), ("mixed", np.concatenate([far[:2], poses_w, far[2:3]]))):
        poses = converter(pw) if len(pw) else np.zeros((0, 4, 4), np.float32)
        got, frames = rend.render_score(poses, rp, [0], sc, text, save=False, return_frames=True)
        assert got.shape == (len(pw), 2) and frames.shape[0] == len(pw), name
        if len(pw):
            ref_frames = np.stack(rend.render(poses, rp, [0], save=False))
            np.testing.assert_array_equal(frames, ref_frames, err_msg=name)
            np.testing.assert_array_equal(got, sc.score_frames(ref_frames, text, rot90=True), err_msg=name)
            np.testing.assert_array_equal(rend.render_score(poses, rp, [0], sc, text, save=False), got, err_msg=name + " (scores only)")
        if name == "off screen":
            assert (frames == frames[0]).all() and (got == got[0]).all()              # the background, six times
    sc.close(); fg.close(); bg.close(); ctx.close()


@pytest.mark.gpu
def test_fused_multi_view_equals_two_step(tmp_path):
    """more than one render view through the fused route — one d2r_render_score_host per view, each with
    its own background (sensor depth + mask per view, indexed by the loop counter as the reference does, :107-110), logits in
    `render`'s view-major frame order (reference combined_rendering.py:95,118) — bit-identical to render + score_frames, with
    nothing but one chunk of frames ever on the host.  The reference's `if save and render_idx == 0` (:157) stands behind its
    view loop: a two-view call clears cb_render/ and writes nothing; both routes reproduce that.  optimise_pose_grid then fails
    at the scatter for L > 1 exactly as the reference does (K * L logits for K poses, clip_scoring.py:205-206)."""
    from dream2real_amd import clip_scoring, combined_rendering
    from dream2real_amd.accio2ngp import converter
    from dream2real_amd.obj_pose_opt import sample_poses_grid
    from dream2real_amd.virtual_cam_pose_sample import get_virtual_cam_poses
    scene, ctx, fg, bg, sc, task, text = _setup()
    poses = converter(sample_poses_grid(task, [7, 6, 1, 1, 1, 1], scene.scene_type).reshape(-1, 4, 4))      # 42
    idx = [1, 0]
    rp = converter(get_virtual_cam_poses(task, idx))
    r = np.random.default_rng(2)
    depths = [(0.5 + 0.2 * r.random((72, 128))).astype(np.float32) for _ in idx]
    masks = [np.ones((72, 128), np.uint8) for _ in idx]
    masks[0][10:40, 30:80] = 0
    masks[1][30:60, 60:120] = 0
    rend = combined_rendering.renderer(str(tmp_path), task, resolution=(96, 54))
    open(os.path.join(rend.out_render_path, "cb_rgb_0000.png"), "wb").write(b"stale")
    ctx.set_option("chunk", 16)
    for dg, mk in ((None, None), (depths, masks)):
        frames_ref = np.stack(rend.render(poses, rp, idx, dg, mk, save=False))
        assert frames_ref.shape[0] == 2 * len(poses) and (frames_ref[:len(poses)] != frames_ref[len(poses):]).any()
        logits_ref = sc.score_frames(frames_ref, text, rot90=True)
        logits, frames = rend.render_score(poses, rp, idx, sc, text, dg, mk, save=False, return_frames=True)
        np.testing.assert_array_equal(frames, frames_ref)
        np.testing.assert_array_equal(logits, logits_ref)
        np.testing.assert_array_equal(rend.render_score(poses, rp, idx, sc, text, dg, mk, save=True), logits_ref)     # scores only
        assert os.listdir(rend.out_render_path) == []          # cleared, nothing written (reference :87-91,:157)
    st = ctx.render_stats()
    assert st["rays_total"] == len(poses) * 96 * 54
    task.text_embeds = text
    with pytest.raises(ValueError):                             # numpy's shape mismatch where torch raises RuntimeError in the reference
        clip_scoring.optimise_pose_grid(rend, None, idx, task, str(tmp_path), sample_res=[7, 6, 1, 1, 1, 1],
                                        phys_check=lambda pb, tm, v: v, scene_type=scene.scene_type, scorer=sc, save_renders=False)
    sc.close(); fg.close(); bg.close(); ctx.close()


@pytest.mark.gpu
def test_failure_in_a_later_chunk_leaves_the_context_usable(tmp_path):
    """render_score_core used to return mid-loop with the render / copy streams forked and PNG jobs in the
    worker pool.  With `debug_fail_chunk` (fault injection: the pass fails in chunk 1, after chunk 0's frames are on their way to
    the host and chunk 1's render is queued on the second stream) the call must report the injected error — not a later one —
    return with every stream joined and the pool drained, and the NEXT call on the same context must give the reference
    logits, frames and files bit for bit, with overlap on and off."""
    from dream2real_amd import combined_rendering
    from dream2real_amd.accio2ngp import converter
    from dream2real_amd.obj_pose_opt import sample_poses_grid
    from dream2real_amd.virtual_cam_pose_sample import get_virtual_cam_poses
    scene, ctx, fg, bg, sc, task, text = _setup()
    poses = converter(sample_poses_grid(task, [8, 6, 1, 1, 1, 1], scene.scene_type).reshape(-1, 4, 4))      # 48 = 3 chunks of 16
    rp = converter(get_virtual_cam_poses(task, [0]))
    rend = combined_rendering.renderer(str(tmp_path), task, resolution=(96, 54))
    frames_ref = np.stack(rend.render(poses, rp, [0], save=False))
    logits_ref = sc.score_frames(frames_ref, text, rot90=True)
    ctx.set_option("chunk", 16)
    for overlap in (1, 0):
        ctx.set_option("overlap", overlap)
        for fail_at in (1, 2, 0):
            ctx.set_option("debug_fail_chunk", fail_at)
            with pytest.raises(_lib.D2RError, match=f"injected fault in chunk {fail_at}"):
                rend.render_score(poses, rp, [0], sc, text, save=True, return_frames=True)
            with pytest.raises(_lib.D2RError, match="needs a preceding d2r_render_score"):
                ctx.render_stats(collect_K=len(poses))          # the failed pass's counters are not offered as statistics
            assert ctx.get_option("debug_fail_chunk") == -1      # one-shot: the hook disarmed itself when it fired
            logits, frames = rend.render_score(poses, rp, [0], sc, text, save=True, return_frames=True)
            np.testing.assert_array_equal(frames, frames_ref)
            np.testing.assert_array_equal(logits, logits_ref)
            assert sorted(os.listdir(rend.out_render_path)) == [f"cb_rgb_{i:04d}.png" for i in range(48)]
            np.testing.assert_array_equal(_lib.png_read_batch(rend.out_render_path, 48), frames_ref)
    sc.close(); fg.close(); bg.close(); ctx.close()


@pytest.mark.gpu
def test_task_after_task_gives_back_device_and_pinned_memory(tmp_path):
    """A drop-in process runs task after task (reference dream2real.py: one ImaginationEngine per scene): context + two snapshots + a CLIP
    tower created, one render-and-score pass with frames and PNGs (pinned staging buffers, the PNG worker pool, LDS / HBM bricks, the
    background's scanline coding), everything closed — five times.  Device memory in use and the process's resident set after round five
    equal those after round two (the first rounds pay one-time costs: HIP module load, RCCL binding, allocator pools), and the scores of
    every round are bit-identical."""
    import gc
    import torch
    import psutil
    from dream2real_amd import combined_rendering
    from dream2real_amd.accio2ngp import converter
    from dream2real_amd.obj_pose_opt import sample_poses_grid
    from dream2real_amd.virtual_cam_pose_sample import get_virtual_cam_poses
    proc = psutil.Process()
    used, rss, scores = [], [], []
    for rnd in range(5):
        scene, ctx, fg, bg, sc, task, text = _setup(160, 90)
        poses = converter(sample_poses_grid(task, [8, 6, 1, 1, 1, 1], scene.scene_type).reshape(-1, 4, 4))      # 48
        rp = converter(get_virtual_cam_poses(task, [0]))
        out = tmp_path / f"r{rnd}"
        out.mkdir()
        rend = combined_rendering.renderer(str(out), task, resolution=(160, 90))
        ctx.set_option("chunk", 16)
        logits, frames = rend.render_score(poses, rp, [0], sc, text, save=True, return_frames=True)
        assert len(os.listdir(rend.out_render_path)) == len(poses)
        scores.append(logits.copy())
        del rend, task, frames
        sc.close(); fg.close(); bg.close(); ctx.close()
        gc.collect()
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info(0)
        used.append(total - free)
        rss.append(proc.memory_info().rss)
    for s in scores[1:]:
        np.testing.assert_array_equal(s, scores[0])
    print(f"\ndevice bytes in use after each task: {used}; host RSS: {rss}")
    assert abs(used[4] - used[1]) <= (8 << 20), used                       # nothing accumulates on the device ...
    assert rss[4] - rss[1] <= (256 << 20), rss                             # ... nor, grossly, on the host (glibc keeps freed scene arrays: measured +-80 MB of noise)
