"""d2r_mesh_render on the GPU against the rule (tests/meshvis_ref.py), byte for byte: the ids image first,
then the frame, each case rendered twice on one context; the refusals; geometry_utils' two pictures and the engine's option."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from dream2real_amd import _lib, geometry_utils
from tests import meshvis_cases as mc
from tests import meshvis_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _view(v):
    return _lib.PcdView(v.width, v.height, v.fx, v.fy, v.cx, v.cy, v.point_size, v.near)


def _gpu(ctx, name):
    a = mc.args(mc.case(name))
    return _lib.mesh_render(ctx, _view(a.pop("view")), a.pop("cam_pose"), return_ids=True, **a)


def _check(ctx, name):
    want_rgb, want_ids, _ = mc.rule(name)
    rgb, ids = _gpu(ctx, name)
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(rgb, want_rgb)
    rgb2, ids2 = _gpu(ctx, name)
    assert rgb2.tobytes() == rgb.tobytes() and ids2.tobytes() == ids.tobytes()
    return rgb, ids


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "E_k0", "E_nt0", "E_empty", "F_many"])
def test_frames_equal_the_rule(ctx, name):
    _check(ctx, name)


def test_sizes_follow_each_other_on_one_context(ctx):
    first = _check(ctx, "F_wide")
    _check(ctx, "F_small")
    again = _gpu(ctx, "F_wide")
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


def test_refusals_leave_outputs_and_context_alone(ctx):
    lib = _lib.load()
    c = mc.case("E")
    before = _gpu(ctx, "E")
    view = _view(c["view"])
    H, W = view.height, view.width
    base = dict(view=C.byref(view), cam=_lib.ptr(c["cam_pose"]), verts=_lib.ptr(c["verts"]), nv=c["verts"].shape[0], tris=_lib.ptr(c["tris"]),
                item=_lib.ptr(c["tri_item"]), nt=c["tris"].shape[0], mats=_lib.ptr(c["item_mats"]), cols=_lib.ptr(c["item_rgb"]),
                n_items=c["item_mats"].shape[0], cc=_lib.ptr(c["cube_centres"]), ch=_lib.ptr(c["cube_half"]), cs=_lib.ptr(c["cube_scores"]),
                K=c["cube_scores"].shape[0], bg=_lib.ptr(np.array(c["background"], np.uint8)))
    bad_tris = c["tris"].copy()
    bad_tris[1, 2] = c["verts"].shape[0]
    bad_item = c["tri_item"].copy()
    bad_item[0] = c["item_mats"].shape[0]
    bad_view = _view(c["view"])
    bad_view.width = 0
    nan_view = _view(c["view"])
    nan_view.fx = float("nan")
    cases = [dict(verts=None), dict(tris=None), dict(item=None), dict(mats=None), dict(cols=None), dict(cc=None), dict(ch=None), dict(cs=None),
             dict(view=None), dict(view=C.byref(bad_view)), dict(view=C.byref(nan_view)), dict(cam=None), dict(bg=None),
             dict(tris=_lib.ptr(bad_tris)), dict(item=_lib.ptr(bad_item))]
    for over in cases:
        a = {**base, **over}
        rgb, ids = np.full((H, W, 3), 0xA5, np.uint8), np.full((H, W), 0xA5A5A5A5 - 2 ** 32, np.int32)
        assert lib.d2r_ctx_set_option(ctx.h, b"no_such_option_planted", C.c_int64(0)) == -1          # plants a message
        planted = lib.d2r_last_error(ctx.h)
        assert b"no_such_option_planted" in planted
        rc = lib.d2r_mesh_render(ctx.h, a["view"], a["cam"], a["verts"], a["nv"], a["tris"], a["item"], a["nt"], a["mats"], a["cols"], a["n_items"],
                                 a["cc"], a["ch"], a["cs"], a["K"], a["bg"], _lib.ptr(rgb), _lib.ptr(ids))
        assert rc == -1, over
        msg = lib.d2r_last_error(ctx.h)
        assert msg and msg != planted, over
        assert (rgb == 0xA5).all() and (ids.view(np.uint32) == 0xA5A5A5A5).all(), over
    assert lib.d2r_mesh_render(None, base["view"], base["cam"], None, 0, None, None, 0, None, None, 0, None, None, None, 0, base["bg"],
                               _lib.ptr(np.zeros((H, W, 3), np.uint8)), None) == -1
    ids = np.full((H, W), 7, np.int32)
    assert lib.d2r_mesh_render(ctx.h, base["view"], base["cam"], None, 0, None, None, 0, None, None, 0, None, None, None, 0, base["bg"], None,
                               _lib.ptr(ids)) == -1 and (ids == 7).all()
    after = _gpu(ctx, "E")
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    np.testing.assert_array_equal(after[1], mc.rule("E")[1])


# ------------------------------------------------------------------------------------------------ the Python layer

def _box(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if b >> a & 1 else lo)[a] for a in range(3)] for b in range(8)], np.float32)
    return v, ref.CUBE_TRIS.astype(np.uint32)


def test_pictures_equal_the_rule_and_their_files(ctx, tmp_path):
    from tests.pcd_edge_cases import look_at, pose
    table = (np.array([[-0.4, -0.4, 0], [0.4, -0.4, 0], [0.4, 0.4, 0], [-0.4, 0.4, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    box = _box((-0.03, -0.03, 0.0), (0.03, 0.03, 0.06))
    paths = [str(tmp_path / "mesh_concave_0.obj"), str(tmp_path / "mesh_concave_1.obj")]
    _lib.obj_write(paths[0], *table)
    _lib.obj_write(paths[1], *box)
    res = (4, 3, 1, 1, 1, 1)
    r = np.random.default_rng(2)
    batch = np.tile(np.eye(4, dtype=np.float32), (12, 1, 1))
    batch[:, :3, 3] = np.stack(np.meshgrid(np.linspace(-0.2, 0.2, 4), np.linspace(-0.15, 0.15, 3), [0.03], indexing="ij"), -1).reshape(12, 3)
    scores = r.uniform(0.2, 0.3, 12).astype(np.float32)
    scores[[2, 7]] = 0
    view = ref.PcdView(width=96, height=54, fx=80.0, fy=80.0, cx=47.5, cy=26.5, point_size=1.0, near=0.01)
    cam = look_at((0.35, -0.3, 0.45), (0.0, 0.0, 0.02))
    init, best = pose((0, 0, 1), 0.3, (0.0, 0.0, 0.0)), batch[5] @ pose((0, 0, 1), 0.9, (0, 0, 0))
    out = [str(tmp_path / "cost_volume.png"), str(tmp_path / "best_pose_vis.png")]
    got_cv = geometry_utils.vis_cost_volume(scores, res, batch.reshape(12, 16), paths[:1], ctx=ctx, view=_view(view), cam_pose=cam, out_path=out[0])
    got_bp = geometry_utils.vis_best_pose(best, paths[:1], paths[1], init, ctx=ctx, view=_view(view), cam_pose=cam, out_path=out[1])
    tv, tt = _lib.obj_read(paths[0])
    bv, bt = _lib.obj_read(paths[1])
    cc, ch, cs = geometry_utils.cost_volume_cubes(scores, res, batch.reshape(12, 16))
    want_cv, ids_cv = ref.render(view, cam, tv, tt, np.zeros(len(tt), np.uint32), np.eye(4)[None], [geometry_utils.BGROUND_GREY], cc, ch, cs)
    M = (best.astype(np.float64) @ np.linalg.inv(init.astype(np.float64))).astype(np.float32)
    want_bp, ids_bp = ref.render(view, cam, np.concatenate([tv, bv]), np.concatenate([tt, bt + np.uint32(len(tv))]),
                                 np.concatenate([np.zeros(len(tt), np.uint32), np.ones(len(bt), np.uint32)]), np.stack([np.eye(4, dtype=np.float32), M]),
                                 geometry_utils.pastel_colors[:2])
    assert ((ids_cv < 0) & (ids_cv != ref.INT32_MIN)).sum() >= 50 and (ids_cv >= 0).sum() >= 50 and (ids_bp >= len(tt)).sum() >= 20
    np.testing.assert_array_equal(got_cv, want_cv)
    np.testing.assert_array_equal(got_bp, want_bp)
    np.testing.assert_array_equal(_lib.png_read_rgb(out[0]), want_cv)
    np.testing.assert_array_equal(_lib.png_read_rgb(out[1]), want_bp)
    with pytest.raises(FileNotFoundError, match="nowhere.obj"):
        geometry_utils.vis_best_pose(best, [str(tmp_path / "nowhere.obj")], paths[1], init, ctx=ctx, view=_view(view), cam_pose=cam)


def _files(d):
    out = {}
    for root, _, names in os.walk(d):
        for n in names:
            out[os.path.relpath(os.path.join(root, n), d)] = open(os.path.join(root, n), "rb").read()
    return out


def test_engine_writes_the_pictures_only_when_asked(ctx, tmp_path):
    """dream_best_pose on the synthetic scan folder of tests/test_engine_gpu.py: the default writes what it wrote before and
    neither picture; vis_cost_vol=True adds best_pose_vis.png, and cost_volume.png too where the reference draws it (not with
    use_vis_pcds), on the use_cache_goal_pose branch as well; every other file keeps its bytes."""
    from dream2real_amd import engine
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    from dream2real_amd.dream2real import CachedLangModel, ImaginationEngine
    from synthetic_scenes import scene_text_embeds
    from tests import test_engine_gpu as teg
    ccfg = CLIP_CONFIGS["vit_tiny"]
    scorer = engine.ClipScorer(ctx, ccfg, random_clip_state_dict(ccfg, seed=6))
    text = scene_text_embeds(np.random.default_rng(3).standard_normal(ccfg["proj"]))
    rgbs, mm, raw_labels, poses = teg._frames()
    hand, scan = str(tmp_path / "hand"), str(tmp_path / "scan")
    teg._write_scan(hand, rgbs, mm, poses)
    _, _, masks, _ = teg._by_hand(ctx, scorer, text, hand, raw_labels)
    teg._write_scan(scan, rgbs, mm, poses, labels=masks)
    lang_path = str(tmp_path / "lang.json")
    CachedLangModel(lang_path).record("parse_instr", [teg.INSTR], [teg.GOAL, teg.NORM]).record("get_movable_obj_idx", [teg.INSTR, teg.CAPTIONS], 1) \
        .record("get_relevant_obj_idxs", [teg.GOAL, teg.CAPTIONS, 1], [1, 2]).save()
    cfg = teg._engine_cfg(tmp_path, scan)
    eng, task, out = teg._run_engine(cfg, ctx, scorer, text, lang_path, teg.CAPTIONS)        # the default
    plain = _files(scan)
    assert "best_render.png" in plain and "cost_volume.png" not in plain and "best_pose_vis.png" not in plain
    for name in ("phys_mod/mesh_concave_0.obj", "phys_mod/mesh_concave_1.obj"):
        assert name in plain
    out2 = eng.dream_best_pose(task, vis_cost_vol=True)                                      # use_vis_pcds: the cost volume is skipped
    for a, b in zip(out, out2):
        np.testing.assert_array_equal(a.numpy(), b.numpy())
    with_vis = _files(scan)
    assert set(with_vis) - set(plain) == {"best_pose_vis.png"}
    assert {k: v for k, v in with_vis.items() if k in plain} == plain                        # every other file byte for byte
    # the cached branch without the ablation draws both
    eng2 = ImaginationEngine(dataclasses.replace(cfg, use_vis_pcds=False, use_cache_goal_pose=True), ctx, scorer, text_embeds=text,
                             lang_model=CachedLangModel(lang_path), intrinsics=teg.K)
    out3 = eng2.dream_best_pose(task, vis_cost_vol=True)
    np.testing.assert_array_equal(out3[2].numpy(), out[2].numpy())
    shape = _lib.png_read_rgb(os.path.join(scan, "best_render.png")).shape
    bg = np.array(geometry_utils.VIS_BACKGROUND)
    cv, bp = (_lib.png_read_rgb(os.path.join(scan, n)) for n in ("cost_volume.png", "best_pose_vis.png"))
    assert cv.shape == shape and bp.shape == shape
    grey = (cv[..., 0] == cv[..., 1]) & (cv[..., 1] == cv[..., 2]) & (cv[..., 0] < 255)     # the shaded grey mesh
    assert grey.sum() >= 50 and ((cv != bg).any(-1) & ~grey).sum() >= 50 and (bp != bg).any(-1).sum() >= 50
    after = _files(scan)
    assert {k: v for k, v in after.items() if k in plain and not k.startswith("cb_render")} == {k: v for k, v in plain.items() if not k.startswith("cb_render")}
    os.remove(os.path.join(scan, "phys_mod", "mesh_concave_1.obj"))
    with pytest.raises(FileNotFoundError, match="mesh_concave_1.obj"):
        eng2.dream_best_pose(task, vis_cost_vol=True)
    scorer.close()
