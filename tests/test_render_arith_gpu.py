"""Option "render_arith" (1 / 2): the marcher in tiny-cuda-nn's half arithmetic as oracle/d2r_oracle.c emulates it
(d2r_oracle_set_arith) — half corner sums in the hash grid (2: the fma form), half accumulators in both MLPs with one rounding per
16-wide k-step, half activations.  Checked against that emulation: the yardstick of every bound is the distance between the
oracle's OWN modes 0 and m, computed in the run — a mode that does not sit well inside it does not tell the arithmetics apart.

The grid half of the arithmetic is specified bit for bit and is held to that: the library exports no encode entry, so a feature is
read out through d2r_nerf_eval_points with MLP weights that carry it exactly through the half-accumulating layers (see
test_grid_encoding_is_bit_exact).

Figures measured on an MI355X stand in the docstrings of the tests and in docs/history/r09.md."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dream2real_amd import _lib

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.0016914558
# bars of the field test as shares of the yardstick, per column (|dlog sigma| rms, |dlog sigma| max, |drgb| max): twice the largest
# ratio measured on an MI355X (rms 0.0106 / 0.0114 for modes 1 / 2, max 0.13 / 0.14, rgb 0.27 / 0.31), capped at 0.5
FIELD_BAR = (0.023, 0.29, 0.5)


@pytest.fixture(scope="module")
def gpu():
    from dream2real_amd import engine
    ctx = engine.Context(0)
    yield {"engine": engine, "ctx": ctx}
    ctx.close()


def _points(scene, n=20000):
    """the 20 000 points and directions of tests/diag/trained_field_parity.measure_distances"""
    r = np.random.Generator(np.random.PCG64(0))
    occ = np.argwhere(scene.fg.occupancy_bool())
    cells = occ[r.integers(0, len(occ), n)]
    xyz = ((cells[:, ::-1] + r.random((n, 3))) / 128.0).astype(np.float32)
    d = r.standard_normal((n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return xyz, d


def _field_distance(f, ref):
    """(|dlog sigma| rms, |dlog sigma| max, |drgb| max) of a field against `ref`, the first two over ref's active samples (alpha
    neither 0 nor saturated, as measure_distances defines them)"""
    act = (ref[:, 0] * DT > 1e-4) & (ref[:, 0] * DT < 30.0)
    dls = np.abs(np.log(np.maximum(f[:, 0], 1e-30)) - np.log(np.maximum(ref[:, 0], 1e-30)))[act]
    return float(np.sqrt((dls ** 2).mean())), float(dls.max()), float(np.abs(f[:, 1:] - ref[:, 1:]).max())


def _frame_setup(gpu, kind="shopping_trained", W=160, H=90, grid=(6, 4, 1)):
    from oracle import host_ref
    from oracle.pipeline import OraclePipeline
    from tests.scenes import make_scene
    engine, ctx = gpu["engine"], gpu["ctx"]
    scene = make_scene(kind)
    fg = engine.Testbed(ctx, scene.fg)
    fg.background_color = list(scene.fg_background)
    pipe = OraclePipeline(scene, W, H)
    poses = host_ref.sample_poses_grid(scene.scene_centre, list(grid) + [1, 1, 1], scene.scene_type).reshape(-1, 4, 4)
    obg = pipe.background()                          # ONE background (an input of the composite) for every contender
    view = fg.view(W, H)
    ctx.set_background(view, obg[0], obg[1])
    T1 = host_ref.converter(np.asarray(scene.obj_pose, np.float32)[None])[0]
    TC = host_ref.converter(np.asarray(scene.cam_poses, np.float32))[0]
    pn = host_ref.converter(poses.astype(np.float32))
    return scene, fg, pipe, poses, obg, view, T1, TC, pn


def test_option_defaults_round_trips_and_refuses_3(gpu):
    """default 0; 1 and 2 round-trip; 3 is D2R_ERR_INVALID with a message, the stored value stays and the context renders on; back at
    0 the frames, depth and field are bit-identical to a fresh context's."""
    from oracle import host_ref
    from tests.scenes import make_scene
    engine, ctx = gpu["engine"], gpu["ctx"]
    scene = make_scene("shopping")
    xyz, d = _points(scene, 4096)
    cam = host_ref.converter(np.asarray(scene.cam_poses, np.float32))[0][None, :3, :]

    def everything(c):
        fg = engine.Testbed(c, scene.fg)
        fg.background_color = list(scene.fg_background)
        rgba, depth = fg.render_batch(cam, 96, 54)
        f = fg.eval_points(xyz, d)
        fg.close()
        return rgba, depth, f

    assert ctx.get_option("render_arith") == 0
    for m in (1, 2):
        ctx.set_option("render_arith", m)
        assert ctx.get_option("render_arith") == m
    with pytest.raises(_lib.D2RError, match="render_arith"):
        ctx.set_option("render_arith", 3)
    with pytest.raises(_lib.D2RError, match="render_arith"):
        ctx.set_option("render_arith", -1)
    assert ctx.get_option("render_arith") == 2
    try:
        half = everything(ctx)                       # a render after the refusal works, in the mode that was stored
    finally:
        ctx.set_option("render_arith", 0)
    assert np.isfinite(half[0]).all() and np.isfinite(half[2]).all() and half[0][..., 3].max() > 0.5
    back = everything(ctx)
    fresh_ctx = engine.Context(0)
    try:
        assert fresh_ctx.get_option("render_arith") == 0
        fresh = everything(fresh_ctx)
    finally:
        fresh_ctx.close()
    for a, b in zip(back, fresh):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(half[2], back[2])      # and the mode does change the arithmetic


def _read_out_model(model, i):
    """`model` with MLP weights that carry feature i of the encoding, exactly, to the outputs of eval_points.  Every product is a half
    times +-1 or a power of two and every k-step adds it to zeros, so the half accumulators hold it exactly:
      density 1: h0 = relu(f), h1 = relu(-f);  density 2: out0 = out1 = h0 - h1 = f  ->  sigma = exp(f)
      colour 1: c0 = relu(out1), c1 = relu(-out1);  colour 2 passes them on;  colour 3: r = sigmoid(2^7 f), g = sigmoid(2^15 f)
    (2^15 f may overflow to +-inf in the LAST layer only, where it saturates g and feeds nothing)."""
    import dataclasses
    z = lambda a: np.zeros_like(a)
    dw1, dw2, cw1, cw2, cw3 = z(model.dw1), z(model.dw2), z(model.cw1), z(model.cw2), z(model.cw3)
    dw1[0, i], dw1[1, i] = 1, -1
    dw2[0, 0], dw2[0, 1], dw2[1, 0], dw2[1, 1] = 1, -1, 1, -1
    cw1[0, 1], cw1[1, 1] = 1, -1
    cw2[0, 0] = cw2[1, 1] = 1
    cw3[0, 0], cw3[0, 1], cw3[1, 0], cw3[1, 1] = 2.0 ** 7, -2.0 ** 7, 2.0 ** 15, -2.0 ** 15
    return dataclasses.replace(model, dw1=dw1, dw2=dw2, cw1=cw1, cw2=cw2, cw3=cw3)


def _decode_feature(out):
    """The half f behind (sigma, r, g) = (exp(f), sigmoid(2^7 f), sigmoid(2^15 f)), each read where adjacent halves are far apart
    against the error of the fp32 exp2 / rcp (a few ulp, i.e. < 1e-6 in the argument): sigma for |f| >= 2^-6 (halves >= 2^-16 apart),
    r for 2^-13 <= |f| < 2^-6 (2^7 f in [2^-6, 2): >= 2^-16 apart), g below (2^15 f < 4, halves and subnormals 2^-9 apart).  The half
    nearest to the read-out is f; +0 and -0 read the same."""
    o = out.astype(np.float64)
    logit = lambda p: np.log(np.maximum(p, 1e-300)) - np.log(np.maximum(1.0 - p, 1e-300))
    with np.errstate(all="ignore"):
        fs, fr, fg = np.log(np.maximum(o[:, 0], 1e-300)), logit(o[:, 1]) / 2.0 ** 7, logit(o[:, 2]) / 2.0 ** 15
    f = np.where(np.abs(fs) >= 2.0 ** -6, fs, np.where(np.abs(fr) >= 2.0 ** -13, fr, fg))
    return f.astype(np.float16).astype(np.float32)


def _wide_grid(levels, seed):
    """table values over the whole range of a trained table and far below it: heavy-tailed, clipped to +-8, scaled by a power of two
    that steps through 2^0 .. 2^-23 from level to level (plus a jitter of up to 2^-3 per entry) — the features of the levels then
    cover every binade down to the subnormal halves, and many sums sit on ties"""
    r = np.random.Generator(np.random.PCG64(seed))
    shape = (levels.n_entries, levels.n_features)
    e = r.integers(0, 4, size=shape)
    for l in range(levels.n_levels):
        e[levels.offset[l]:levels.offset[l] + levels.size[l]] += (5 * l) % 21
    g = np.clip(r.standard_t(3, size=shape) * 0.7, -8, 8) * 2.0 ** -e
    g[r.random(shape) < 0.02] = 0.0
    return g.astype(np.float16)


@pytest.mark.parametrize("layout", ["l16f2", "l8f4"])
@pytest.mark.parametrize("m", [1, 2])
def test_grid_encoding_is_bit_exact(gpu, m, layout):
    """Every one of the 32 features of the mode-m encoding equals d2r_oracle_encode_points under set_arith(m) bit for bit, on the
    20 000 points of measure_distances, for both grid layouts (dense and hashed levels in each) — on the trained-like scene's own
    table (L = 16, F = 2 only) and on a table whose values span every binade down to the subnormal halves (over 40 % of its features
    are subnormal halves).  Found by this test: with the convert fused into the fma (v_fma_mixlo_f16: one rounding) 2 .. 11 of 20 000
    values per feature were off by one half ulp in mode 2; nerf.hip rn16 keeps the two roundings apart."""
    import dataclasses
    from dream2real_amd.scene import grid_levels
    from oracle import render_ref
    from tests.scenes import make_scene
    engine, ctx = gpu["engine"], gpu["ctx"]
    scene = make_scene("shopping_trained")
    xyz, d = _points(scene)
    levels = grid_levels() if layout == "l16f2" else grid_levels(n_levels=8, n_features=4, log2_hashmap_size=15)
    assert levels.hashed.any() and not levels.hashed.all()
    models = [dataclasses.replace(scene.fg, levels=levels, grid=_wide_grid(levels, 11))]
    if layout == "l16f2":
        models.append(scene.fg)
    for model in models:
        old = render_ref.set_arith(m)
        try:
            want = render_ref.encode_points(render_ref.OracleNerf(model), xyz)
        finally:
            render_ref.set_arith(old)
        assert want.shape == (len(xyz), 32) and (want == want.astype(np.float16).astype(np.float32)).all()
        mag = np.abs(want[want != 0])
        print(f"[render_arith {m}, {layout}] features: |f| from {mag.min():.3g} to {mag.max():.3g}, {(mag < 2.0 ** -14).mean():.2%} subnormal")
        try:
            ctx.set_option("render_arith", m)
            for i in range(32):
                tb = engine.Testbed(ctx, _read_out_model(model, i))
                try:
                    got = _decode_feature(tb.eval_points(xyz, d))
                finally:
                    tb.close()
                bad = np.nonzero(got != want[:, i])[0]
                assert len(bad) == 0, (layout, m, i, len(bad), got[bad[:4]], want[bad[:4], i])
        finally:
            ctx.set_option("render_arith", 0)


@pytest.mark.parametrize("m", [1, 2])
def test_field_sits_well_inside_the_distance_between_the_oracles_modes(gpu, m):
    """shopping_trained, the 20 000 points of measure_distances.  Yardstick: oracle mode 0 <-> oracle mode m in |dlog sigma| rms,
    max and |drgb| max (active samples), computed here.  GPU mode m <-> oracle mode m must be at most FIELD_BAR x the yardstick in
    all three, and GPU mode 0 must sit farther from oracle mode m than GPU mode m does in every column.
    FIELD_BAR: per column, twice the largest measured ratio, capped at 0.5 (0.5 is the purpose: above it the mode does not tell the
    arithmetics apart).  Measured (MI355X), GPU m <-> oracle m against oracle 0 <-> oracle m: mode 1 rms 6.3e-5 / 5.97e-3 (0.011),
    max 0.0039 / 0.0298 (0.13), rgb 0.0019 / 0.0068 (0.27); mode 2 rms 6.7e-5 / 5.90e-3 (0.011), max 0.0039 / 0.0272 (0.14), rgb
    0.0017 / 0.0055 (0.31).  The maxima are single half-ulp flips of a network output (2^-8 at |x| in [4, 8))."""
    from oracle import render_ref
    from tests.scenes import make_scene
    engine, ctx = gpu["engine"], gpu["ctx"]
    scene = make_scene("shopping_trained")
    xyz, d = _points(scene)
    om = render_ref.OracleNerf(scene.fg)
    o = {}
    for mode in (0, m):
        old = render_ref.set_arith(mode)
        try:
            o[mode] = render_ref.eval_points(om, xyz, d)
        finally:
            render_ref.set_arith(old)
    fg = engine.Testbed(ctx, scene.fg)
    g = {}
    try:
        for mode in (0, m):
            ctx.set_option("render_arith", mode)
            g[mode] = fg.eval_points(xyz, d)
    finally:
        ctx.set_option("render_arith", 0)
        fg.close()
    assert np.isfinite(g[m]).all()
    yard = _field_distance(o[0], o[m])
    mine = _field_distance(g[m], o[m])
    spec = _field_distance(g[0], o[m])
    ratio = [a / b for a, b in zip(mine, yard)]
    print(f"[render_arith {m}] |dlog sigma| rms, max, |drgb| max: oracle 0 <-> oracle {m} {yard}; GPU {m} <-> oracle {m} {mine} "
          f"(ratios {ratio}); GPU 0 <-> oracle {m} {spec}")
    assert all(y > 0 for y in yard)
    for name, a, y, s, bar in zip(("dlog_sigma_rms", "dlog_sigma_max", "drgb_max"), mine, yard, spec, FIELD_BAR):
        assert a <= bar * y, (name, a, y, a / y)
        assert s > a, (name, s, a)


@pytest.mark.parametrize("m", [1, 2])
def test_frames_sit_well_inside_the_distance_between_the_oracles_modes(gpu, m):
    """Composited frames, 160x90, the (6, 4, 1) grid: the share of the object's pixels where GPU mode m is off oracle mode m by more
    than one LSB is at most half the same share between oracle mode 0 and oracle mode m; logits of the two through the fp32 oracle
    tower within 1e-3 of the logit scale.  Measured (MI355X), 5 159 object pixels in 24 frames: GPU m <-> oracle m 0 pixels for
    both modes; oracle 0 <-> oracle m 0 pixels (mode 1: the bound is then "none") and 0.039 % (mode 2); logits 8.3e-6 / 1.4e-5."""
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    from oracle import render_ref
    from oracle.pipeline import oracle_logits
    from tests.diag.trained_field_parity import _bg_u8
    from tests.parity_utils import random_unit_text_embeds
    ctx = gpu["ctx"]
    scene, fg, pipe, poses, obg, view, T1, TC, pn = _frame_setup(gpu)
    want = {}
    for mode in (0, m):
        old = render_ref.set_arith(mode)
        try:
            want[mode] = pipe.frames(poses, bg=obg)
        finally:
            render_ref.set_arith(old)
    try:
        ctx.set_option("render_arith", m)
        got = fg.render_composite(view, T1, TC, pn)
    finally:
        ctx.set_option("render_arith", 0)
        fg.close()
    hit = (want[m] != np.broadcast_to(_bg_u8(pipe, obg), want[m].shape)).any(-1)
    share = lambda a, b: float((np.abs(a.astype(int) - b.astype(int)).max(-1)[hit] > 1).mean())
    mine, yard = share(got, want[m]), share(want[0], want[m])
    cfg = CLIP_CONFIGS["vit_b16"]
    sd = random_clip_state_dict(cfg, 6, text=False)
    text = random_unit_text_embeds(cfg["proj"], 3)
    scale = float(np.exp(np.float32(sd.get("logit_scale", 4.6052))))
    lg, _ = oracle_logits(got, cfg, sd, text)
    lw, _ = oracle_logits(want[m], cfg, sd, text)
    dl = float(np.abs(lg - lw).max() / scale)
    print(f"[render_arith {m}] {int(hit.sum())} object pixels in {len(poses)} frames: off by more than one LSB — GPU {m} <-> oracle {m} {mine:.4%}, "
          f"oracle 0 <-> oracle {m} {yard:.4%}; |dlogit|/scale {dl:.2e}")
    assert hit.sum() > 1000
    assert mine <= 0.5 * yard, (mine, yard)
    assert dl <= 1e-3, dl


def test_fused_path_in_half_arithmetic_is_chunk_independent_and_equals_render_then_score(gpu):
    """render_arith 1 through d2r_render_score_host: logits bit-identical across two chunk settings and to scoring the frames that
    d2r_render_composite returned; the frames are the half-arithmetic ones, not the default's."""
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    from tests.parity_utils import random_unit_text_embeds
    engine, ctx = gpu["engine"], gpu["ctx"]
    scene, fg, pipe, poses, obg, view, T1, TC, pn = _frame_setup(gpu, "shopping", 96, 54, (6, 4, 1))
    cfg = CLIP_CONFIGS["vit_tiny"]
    sc = engine.ClipScorer(ctx, cfg, random_clip_state_dict(cfg, 6, text=False))
    text = random_unit_text_embeds(cfg["proj"], 3)
    chunk = ctx.get_option("chunk")
    try:
        plain = fg.render_composite(view, T1, TC, pn)
        ctx.set_option("render_arith", 1)
        frames_ref = fg.render_composite(view, T1, TC, pn)
        logits_ref = sc.score_frames(frames_ref, text, rot90=True)
        out = {}
        for c in (16, 7):                            # 24 candidates: 16 + 8, and 7 + 7 + 7 + 3
            ctx.set_option("chunk", c)
            out[c] = engine.render_score_host(ctx, fg, sc, view, T1, TC, pn, text, return_frames=True)
    finally:
        ctx.set_option("render_arith", 0)
        ctx.set_option("chunk", chunk)
        sc.close()
        fg.close()
    assert not np.array_equal(frames_ref, plain)
    for c in (16, 7):
        np.testing.assert_array_equal(out[c][1], frames_ref, err_msg=f"chunk {c}")
        np.testing.assert_array_equal(out[c][0], logits_ref, err_msg=f"chunk {c}")


@pytest.mark.parametrize("m", [0, 1, 2])
def test_search_forks_finds_the_arithmetic_the_reference_frames_were_rendered_in(m, tmp_path):
    """The oracle in mode m plays the reference run: its composited frames as cb_render/cb_rgb_%04d.png beside stand-in snapshots
    (views with the reference configs' lens), pose_batch.txt and pose_scores.txt.  `validate_artifacts.py --search-forks` must name
    render_arith m with the lens on as the closest combination (mlp_f16 is not asserted for m = 0)."""
    from PIL import Image
    from dream2real_amd.scene import DEMO_LENS
    from oracle import host_ref, render_ref
    from oracle.pipeline import OraclePipeline
    from tests.ingp_writer import save_ingp
    from tests.scenes import make_scene
    W, H = 96, 54
    scene = make_scene("shopping_trained", lens=DEMO_LENS)
    d = str(tmp_path / "method_out" / "shopping")
    os.makedirs(os.path.join(d, "cb_render"))
    save_ingp(os.path.join(d, "fg_base.ingp"), scene.fg, training_views=scene.training_views, background_color=scene.fg_background)
    save_ingp(os.path.join(d, "bg_base.ingp"), scene.bg, training_views=scene.training_views)
    poses = host_ref.sample_poses_grid(scene.scene_centre, [4, 3, 1, 1, 1, 1], scene.scene_type).reshape(-1, 4, 4)
    old = render_ref.set_arith(m)
    try:
        frames = OraclePipeline(scene, W, H).frames(poses)
    finally:
        render_ref.set_arith(old)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(d, "cb_render", f"cb_rgb_{i:04d}.png"))
    np.savetxt(os.path.join(d, "pose_batch.txt"), poses.reshape(-1, 16))
    np.savetxt(os.path.join(d, "pose_scores.txt"), np.ones(len(poses)))
    np.savetxt(str(tmp_path / "obj_pose.txt"), scene.obj_pose)
    np.savetxt(str(tmp_path / "cam_pose.txt"), scene.cam_poses[0])
    out = str(tmp_path / "report.json")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "validate_artifacts.py"), "--method-out", d, "--search-forks",
                        "--obj-pose", str(tmp_path / "obj_pose.txt"), "--cam-pose", str(tmp_path / "cam_pose.txt"), "--resolution", f"{W},{H}",
                        "--out", out], capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.stdout.strip().startswith("{"), (r.stdout[-1500:], r.stderr[-3000:])
    print(r.stderr[-2500:])
    e = json.loads(r.stdout)["sections"]["e_forks"]
    assert "table" in e, e
    assert len(e["table"]) == 8 and e["frames_compared"] == len(poses)
    assert e["closest"]["render_arith"] == m and e["closest"]["lens"] == 1, e["closest"]
    assert json.load(open(out))["sections"]["e_forks"]["closest"] == e["closest"]
    assert "closest: render_arith" in r.stderr
