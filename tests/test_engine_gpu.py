"""The scan-folder engine on the GPU: the label census (d2r_masks_census) bit for bit against np.bincount, and one scene from
RGB-D files to the best pose through ImaginationEngine's three calls (use_vis_pcds, phys_backend="tsdf": frames, scene-bound
masks, cached label masks, census, TSDF physics fields, visual clouds, physics pre-filter, render-and-score), held bit for
bit to the same stages called by hand on the same context."""
import json
import os
import time

import numpy as np
import pytest

from dream2real_amd import _lib, clip_scoring, physics_utils, segmentation
from dream2real_amd.dream2real import CachedLangModel, ImaginationEngine, PathConfig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ census

def _census_case(name):
    r = np.random.default_rng(len(name) * 7 + 1)
    if name in ("1x1x1", "1x1x63", "1x1x64", "1x1x65"):                 # below, at and past one 16-byte segment and one wave
        return r.integers(0, 256, tuple(int(v) for v in name.split("x")), dtype=np.uint8)
    if name == "all 256 labels":                                        # 1799 pixels a frame: every frame starts off any alignment
        m = r.integers(0, 256, (3, 7, 257), dtype=np.uint8)
        for f in range(3):
            m[f].reshape(-1)[r.permutation(7 * 257)[:256]] = np.arange(256, dtype=np.uint8)
        return m
    if name == "last pixel":                                            # a label whose only pixel is the batch's last byte
        m = r.integers(0, 4, (2, 90, 160), dtype=np.uint8)
        m[1, 89, 159] = 200
        return m
    if name == "one label":                                             # 921 600 adds into one bin, 29 workgroups
        return np.full((1, 720, 1280), 7, np.uint8)
    if name == "empty frame":                                           # 1551 pixels a frame, frame 2 all zeros
        m = r.integers(1, 256, (5, 33, 47), dtype=np.uint8)
        m[2] = 0
        return m
    raise KeyError(name)


@pytest.mark.parametrize("name", ["1x1x1", "1x1x63", "1x1x64", "1x1x65", "all 256 labels", "last pixel", "one label", "empty frame"])
def test_census_equals_bincount(ctx, name):
    m = _census_case(name)
    want = np.stack([np.bincount(f.ravel(), minlength=256) for f in m]).astype(np.uint32)
    got = _lib.masks_census(ctx, m)
    assert got.dtype == np.uint32 and got.shape == (m.shape[0], 256)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_lib.masks_census(ctx, m), want)     # a second call starts from zero again
    if name == "all 256 labels":
        assert (want > 0).all()
    if name == "last pixel":
        assert got[1, 200] == 1 and got[0, 200] == 0
    if name == "one label":
        assert got[0, 7] == 921600 and got.sum() == 921600
    if name == "empty frame":
        assert got[2, 0] == 33 * 47 and got[2, 1:].sum() == 0
        with pytest.raises(ValueError, match=r"but not 0\b"):          # frame 2's zeros are label 0; without them the helper refuses
            segmentation.label_census(m[:2], ctx=ctx)
    if name == "last pixel":
        with pytest.raises(ValueError, match=r"but not 4\b"):
            segmentation.label_census(m, ctx=ctx)
        m[1, 89, 159] = 255
        labels, num_objs, counts = segmentation.label_census(m, ctx=ctx)
        assert labels.tolist() == [0, 1, 2, 3, 255] and num_objs == 4 and counts[1, 255] == 1


def test_census_refuses_bad_arguments(ctx):
    import ctypes as C
    lib = _lib.load()
    m, out = np.zeros((1, 2, 2), np.uint8), np.zeros((1, 256), np.uint32)
    assert lib.d2r_masks_census(ctx.h, None, 1, 2, 2, _lib.ptr(out)) == -1
    assert lib.d2r_masks_census(ctx.h, _lib.ptr(m), 1, 2, 2, None) == -1
    assert lib.d2r_masks_census(ctx.h, _lib.ptr(m), 0, 2, 2, _lib.ptr(out)) == -1
    assert lib.d2r_masks_census(C.c_void_p(0), _lib.ptr(m), 1, 2, 2, _lib.ptr(out)) == -1
    np.testing.assert_array_equal(_lib.masks_census(ctx, m)[0, :2], [4, 0])


# ------------------------------------------------------------------------------------------------ the scene

W, H = 192, 108
K = np.array([[200.0, 0.0, 95.5], [0.0, 200.0, 53.5], [0.0, 0.0, 1.0]])
TABLE = (np.array([-0.4, -0.4, -0.02]), np.array([0.4, 0.4, 0.0]))
BOX_A = (np.array([-0.025, -0.025, 0.0]), np.array([0.025, 0.025, 0.05]))            # label 1, the box to move
BOX_B = (np.array([-0.095, -0.075, 0.0]), np.array([-0.045, -0.025, 0.05]))          # label 2, in the way of some candidates
BOUNDS = [[-0.2, -0.18, -0.03], [0.12, 0.14, 0.10]]
# z: the height of the moved box's mesh centre as one view sees it (top and two sides: 0.046), so that a candidate stands on the
# table; 5 mm either way give the same verdicts with the CPU restatement of the rule (tests/sdfphys_ref.py): 4 of 16 valid
CENTRE = [0.0, 0.0, 0.047]
RES = [4, 4, 1, 1, 1, 1]
INSTR = "put the red box next to the blue box"
GOAL, NORM = "a red box next to a blue box", "a red box and a blue box"
CAPTIONS = ["__background__", "red box", "blue box"]


def _look_at(eye, target):
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x = x / np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def _slab(o, d, lo, hi):
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    tn, tf = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
    return np.where((tn <= tf) & (tn > 0), tn, np.inf)


def _raycast(T):
    """-> (rgb uint8 [H,W,3], depth millimetres uint16 [H,W], label uint8 [H,W]) of the table and the two boxes from pose T."""
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    d = np.stack([(jj - K[0, 2]) / K[0, 0], (ii - K[1, 2]) / K[1, 1], np.ones((H, W))], -1) @ T[:3, :3].T
    o = T[:3, 3]
    ts = np.stack([_slab(o, d, *b) for b in (TABLE, BOX_A, BOX_B)])
    t = ts.min(0)
    label = np.where(np.isfinite(t), ts.argmin(0), 0).astype(np.uint8)
    depth = np.where(np.isfinite(t), t, 0.0)
    pts = o + d * depth[..., None]
    shade = (80 + 60 * label + 40 * ((np.floor(pts[..., 0] * 50) + np.floor(pts[..., 1] * 50)) % 2)).astype(np.uint8)
    return np.stack([shade, 255 - shade, shade // 2 + 30 * label], -1).astype(np.uint8), np.round(depth * 1000).astype(np.uint16), label


def _frames():
    target = np.array([-0.03, -0.02, 0.02])
    el = np.deg2rad(55.0)
    poses = np.stack([_look_at(target + 0.45 * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)]), target)
                      for az in 2 * np.pi * np.arange(4) / 4 + 0.4])
    shots = [_raycast(T) for T in poses]
    return np.stack([s[0] for s in shots]), np.stack([s[1] for s in shots]), np.stack([s[2] for s in shots]), poses


def _write_scan(d, rgbs, mm, poses, labels=None):
    from PIL import Image
    for sub in ("images", "depth"):
        os.makedirs(os.path.join(d, sub))
    np.savetxt(os.path.join(d, "poses.txt"), poses.reshape(-1, 16))
    for k in range(len(rgbs)):
        _lib.png_write(rgbs[k], os.path.join(d, "images", "rgb_%04d.png" % k))
        Image.fromarray(mm[k]).save(os.path.join(d, "depth", "depth_%04d.png" % k))
    if labels is not None:
        os.makedirs(os.path.join(d, "XMem_masks"))
        for k in range(len(labels)):
            _lib.png_write_channels(labels[k], os.path.join(d, "XMem_masks", "rgb_%04d.png" % k))


def _by_hand(ctx, scorer, text, d, raw_labels):
    """The stages the engine joins, called one by one."""
    import torch
    from dream2real_amd.data_loader import d2r_dataloader
    from dream2real_amd.pcd_visual_model import PointCloudRenderer
    from dream2real_amd.scene_model import ObjectModel, SceneModel, TaskModel
    cfg = PathConfig(data_dir=d, sample_res=RES, width=W, height=H)
    loader = d2r_dataloader(cfg, ctx)
    rgbs, depths, T_WC = loader.load_rgbds()
    oob = loader.remove_background(K, BOUNDS)
    masks = segmentation.refine_masks(raw_labels, depths, T_WC, K, oob, CENTRE, d, ctx=ctx)
    opt = [torch.tensor(p) for p in T_WC]
    objs = [ObjectModel(CAPTIONS[k], None, None, None, None, k) for k in range(3)]
    sm = SceneModel(CENTRE, objs, objs[0], rgbs, depths, opt, K, masks, BOUNDS, 0)
    mov = objs[1]
    (bg_phys, mov_phys), (_, mov_init) = physics_utils.create_lazy_phys_mods(
        sm, mov, BOUNDS, os.path.join(d, "phys_mod/"), use_phys_tsdf=True, use_vis_pcds=True, single_view_idx=0, ctx=ctx, phys_backend="tsdf")
    mov.vis_model = TaskModel.create_movable_vis_model(sm, mov, oob, os.path.join(d, "movable_vis_mod/"), use_vis_pcds=True, pcds_type=0,
                                                       single_view_idx=0, ctx=ctx)
    bg, bg_masks = TaskModel.create_task_bground_obj(sm, mov, [objs[1], objs[2]], oob, os.path.join(d, "task_bground_vis_mod/"),
                                                     use_vis_pcds=True, pcds_type=0, single_view_idx=0, render_distractors=False, ctx=ctx)
    mov.phys_model, mov.pose, bg.phys_model = mov_phys, mov_init, bg_phys
    task = TaskModel(INSTR, GOAL, [NORM], sm, mov, bg, bg_masks, True)
    check, _, _ = physics_utils.create_unsupcol_check(ctx, task, RES, False, lazy_phys_mods=True)
    n_valid = int(check(torch.from_numpy(clip_scoring.sample_poses_grid(task, RES, 0)), task, torch.ones(16, dtype=torch.bool)).sum())
    out = clip_scoring.optimise_pose_grid(PointCloudRenderer(ctx), np.stack([depths[0]]), [0], task, d, sample_res=RES, phys_check=check,
                                          use_templates=False, scene_type=0, use_vis_pcds=True, smoothing=True, scorer=scorer, text_embeds=text)
    check.shapes.close()
    return out, n_valid, masks, oob


def _engine_cfg(tmp_path, d, **caches):
    group = dict(render_distractors=False, spatial_smoothing=True, physics_only=False, use_vis_pcds=True, pcds_type=0, single_view_idx=0,
                 use_cache_dynamic_masks=False, use_cache_segs=True, use_cache_cam_poses=False, use_cache_captions=False, use_cache_phys=False,
                 use_cache_vis=False, use_cache_llm=True, use_cache_renders=False, use_cache_goal_pose=False, use_phys=True, use_phys_tsdf=True,
                 lazy_phys_mods=True, multi_view_captions=False, scene_type=0, sample_res=RES, scene_centre=CENTRE, scene_phys_bounds=BOUNDS,
                 render_cam_pose_idx=[0], phys_backend="tsdf")
    group.update(caches)
    path = str(tmp_path / ("settings_%d.json" % len(caches)))
    json.dump({"engine": group, "camera": {"w": W, "h": H}, "trainer": {"train": False}}, open(path, "w"))
    return PathConfig.from_json(path, d)


def _run_engine(cfg, ctx, scorer, text, lang_path, captions, laps=None):
    eng = ImaginationEngine(cfg, ctx, scorer, text_embeds=text, lang_model=CachedLangModel(lang_path), intrinsics=K)
    t = [time.perf_counter()]

    def lap(name):
        t.append(time.perf_counter())
        if laps is not None:
            laps[name] = t[-1] - t[-2]
    eng.build_scene_model(captions=captions)
    lap("build_scene_model")
    task = eng.interpret_user_instr(INSTR)
    lap("interpret_user_instr")
    out = eng.dream_best_pose(task)
    lap("dream_best_pose")
    return eng, task, out


def test_scan_folder_to_best_pose(ctx, tmp_path):
    """(a) the three engine calls == the stages by hand, bit for bit; (b) the pre-filter keeps some candidates and drops some;
    (c) the files a later run reads are there; (d) a second engine on every cache the path supports gives the same again (use_cache_renders and use_cache_goal_pose read cb_render/
    files and NeRF snapshots, which the point-cloud ablation does not write); (e) the task
    masks are the reference's rule (scene_model.py:67-80, 104) stated in numpy."""
    from dream2real_amd import engine
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    from synthetic_scenes import scene_text_embeds
    ccfg = CLIP_CONFIGS["vit_tiny"]
    scorer = engine.ClipScorer(ctx, ccfg, random_clip_state_dict(ccfg, seed=6))
    text = scene_text_embeds(np.random.default_rng(3).standard_normal(ccfg["proj"]))
    rgbs, mm, raw_labels, poses = _frames()
    assert all((raw_labels == k).any(axis=(1, 2)).all() for k in (0, 1, 2))                  # every frame sees the table and both boxes
    hand, scan = str(tmp_path / "hand"), str(tmp_path / "scan")
    _write_scan(hand, rgbs, mm, poses)
    (best_h, batch_h, scores_h), n_valid, masks, oob = _by_hand(ctx, scorer, text, hand, raw_labels)
    assert (masks == 255).any() and all((masks == k).any() for k in (0, 1, 2))

    _write_scan(scan, rgbs, mm, poses, labels=masks)
    lang_path = str(tmp_path / "lang.json")
    CachedLangModel(lang_path).record("parse_instr", [INSTR], [GOAL, NORM]).record("get_movable_obj_idx", [INSTR, CAPTIONS], 1) \
        .record("get_relevant_obj_idxs", [GOAL, CAPTIONS, 1], [1, 2]).save()
    laps = {}
    eng, task, (best, batch, scores) = _run_engine(_engine_cfg(tmp_path, scan), ctx, scorer, text, lang_path, CAPTIONS, laps)
    print("engine stages, seconds:", {k: round(v, 3) for k, v in laps.items()})

    # (a)
    for got, want in ((best, best_h), (batch, batch_h), (scores, scores_h)):
        assert got.dtype == want.dtype and got.shape == want.shape
        np.testing.assert_array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    np.testing.assert_array_equal(eng.scene_model.masks, masks)
    np.testing.assert_array_equal(eng.out_scene_bound_masks, oob)
    np.testing.assert_array_equal(eng.label_counts, np.stack([np.bincount(f.ravel(), minlength=256) for f in masks]))
    assert [o.name for o in eng.scene_model.objs] == CAPTIONS and task.movable_obj is eng.scene_model.objs[1]
    assert task.goal_caption == GOAL and task.norm_captions == [NORM] and task.topdown is True
    # (b)
    valid = int((scores.numpy() != 0).sum())
    print("valid poses:", valid, "of 16;", (scores.numpy().reshape(4, 4) != 0).astype(int).tolist())
    assert valid == n_valid and 0 < valid < 16
    # (c)
    names = ["goal_pose.txt", "pose_batch.txt", "pose_scores.txt", "best_render.png", "captions.json", "opt_cam_poses.npy"]
    names += ["phys_mod/sdf_%d.npz" % k for k in (0, 1)] + ["phys_mod/init_pose_%d.txt" % k for k in (0, 1)]
    names += ["images/dynamic_mask_rgb_%04d.png" % k for k in range(4)]
    names += ["movable_vis_mod/obj_vis_0.pcd", "task_bground_vis_mod/obj_vis_0.pcd"]
    for name in names:
        assert os.path.exists(os.path.join(scan, name)), name
    np.testing.assert_array_equal(np.loadtxt(os.path.join(scan, "pose_scores.txt")).astype(np.float32), scores.numpy())
    # (e)
    objs, relevant = eng.scene_model.objs, [eng.scene_model.objs[1], eng.scene_model.objs[2]]
    want_bg = np.zeros_like(masks)
    for obj in objs:
        if obj is task.movable_obj or obj is objs[0] or not any(obj is r for r in relevant):
            want_bg[masks == obj.mask_idx] = 1
    want_bg |= (oob != 0).astype(np.uint8)
    np.testing.assert_array_equal(task.task_bground_masks, want_bg)
    assert want_bg.min() == 0 and want_bg.max() == 1
    np.testing.assert_array_equal(task.movable_masks, np.logical_not(masks == 1))
    # (d)
    caches = {k: True for k in ("use_cache_dynamic_masks", "use_cache_segs", "use_cache_cam_poses", "use_cache_captions", "use_cache_phys",
                                "use_cache_vis", "use_cache_llm")}
    cfg2 = _engine_cfg(tmp_path, scan, **caches)
    _, task2, (best2, batch2, scores2) = _run_engine(cfg2, ctx, scorer, text, lang_path, None)
    for got, want in ((best2, best), (batch2, batch), (scores2, scores)):
        np.testing.assert_array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    np.testing.assert_array_equal(task2.task_bground_masks, want_bg)
    scorer.close()
