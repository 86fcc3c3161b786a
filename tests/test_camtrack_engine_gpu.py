"""ImaginationEngine with cam_pose_refine="tsdf" on the synthetic scan of tests/test_engine_gpu.py with its poses perturbed:
build_scene_model refines the loader's poses against the volume fused so far, saves them and the reports,
and the run reaches a best pose; with "none" the saved poses are the loader's, as before."""
import json
import os

import numpy as np
import pytest

from dream2real_amd import cam_pose_opt, segmentation
from dream2real_amd.dream2real import CachedLangModel, PathConfig
from tests import camtrack_cases as cases
from tests import test_engine_gpu as scan_test

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def test_scan_folder_with_refined_camera_poses(ctx, tmp_path):
    from dream2real_amd import engine
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    from dream2real_amd.data_loader import d2r_dataloader
    from synthetic_scenes import scene_text_embeds
    ccfg = CLIP_CONFIGS["vit_tiny"]
    scorer = engine.ClipScorer(ctx, ccfg, random_clip_state_dict(ccfg, seed=6))
    text = scene_text_embeds(np.random.default_rng(3).standard_normal(ccfg["proj"]))
    rgbs, mm, raw_labels, true_poses = scan_test._frames()
    poses = true_poses.copy()
    for k, (dt, axis, angle) in zip((1, 2, 3), (((0.002, -0.001, 0.001), (0, 0, 1), 0.004), ((-0.001, 0.002, 0.0015), (1, 1, 0), 0.005),
                                                ((0.0015, 0.001, -0.002), (0, 1, 1), 0.003))):
        poses[k] = cases.perturbed(true_poses[k], dt, axis, angle)
    first, scan, plain = str(tmp_path / "first"), str(tmp_path / "scan"), str(tmp_path / "plain")
    scan_test._write_scan(first, rgbs, mm, poses)
    loader = d2r_dataloader(PathConfig(data_dir=first, sample_res=scan_test.RES, width=scan_test.W, height=scan_test.H), ctx)
    _, depths, T_WC = loader.load_rgbds()
    oob = loader.remove_background(scan_test.K, scan_test.BOUNDS)
    masks = segmentation.refine_masks(raw_labels, depths, T_WC, scan_test.K, oob, scan_test.CENTRE, first, ctx=ctx)
    lang_path = str(tmp_path / "lang.json")
    CachedLangModel(lang_path).record("parse_instr", [scan_test.INSTR], [scan_test.GOAL, scan_test.NORM]) \
        .record("get_movable_obj_idx", [scan_test.INSTR, scan_test.CAPTIONS], 1) \
        .record("get_relevant_obj_idxs", [scan_test.GOAL, scan_test.CAPTIONS, 1], [1, 2]).save()

    scan_test._write_scan(scan, rgbs, mm, poses, labels=masks)
    cfg = scan_test._engine_cfg(tmp_path, scan, use_vis_pcds=False, vis_backend="tsdf", cam_pose_refine="tsdf", scene_centre=[0.0, 0.0, 0.034])
    assert cfg.cam_pose_refine == "tsdf"
    eng, task, (best, batch, scores) = scan_test._run_engine(cfg, ctx, scorer, text, lang_path, scan_test.CAPTIONS)
    saved = np.load(os.path.join(scan, "opt_cam_poses.npy"))
    loaded = np.asarray(T_WC, np.float32)
    assert saved.dtype == np.float32 and saved.shape == loaded.shape and (saved != loaded).any()
    np.testing.assert_array_equal(saved[0].view(np.uint32), loaded[0].view(np.uint32))                     # the anchor
    direct, direct_reports = cam_pose_opt.refine_cam_poses(depths, T_WC, scan_test.K, oob, scan_test.BOUNDS, ctx=ctx)
    np.testing.assert_array_equal(saved.view(np.uint32), direct.view(np.uint32))
    reports = json.load(open(os.path.join(scan, "cam_pose_refine.json")))
    assert len(reports) == len(loaded) and reports == json.loads(json.dumps(direct_reports)) and reports[0]["status"] == "anchor"
    print("reports:", reports)
    for got, want in zip(eng.scene_model.opt_cam_poses if hasattr(eng.scene_model, "opt_cam_poses") else [], saved):
        np.testing.assert_array_equal(np.asarray(got), want)
    assert np.isfinite(best.numpy()).all() and 0 < int((scores.numpy() != 0).sum()) <= len(scores)
    for name in ("goal_pose.txt", "pose_batch.txt", "pose_scores.txt", "best_render.png"):
        assert os.path.exists(os.path.join(scan, name)), name

    # "none": the saved poses are the loader's, and no report is written
    scan_test._write_scan(plain, rgbs, mm, poses, labels=masks)
    cfg0 = scan_test._engine_cfg(tmp_path, plain, use_vis_pcds=False, vis_backend="tsdf", scene_centre=[0.0, 0.0, 0.034])
    assert cfg0.cam_pose_refine == "none"
    from dream2real_amd.dream2real import ImaginationEngine
    eng0 = ImaginationEngine(cfg0, ctx, scorer, text_embeds=text, lang_model=CachedLangModel(lang_path), intrinsics=scan_test.K)
    eng0.build_scene_model(captions=scan_test.CAPTIONS)
    np.testing.assert_array_equal(np.load(os.path.join(plain, "opt_cam_poses.npy")), loaded)
    assert not os.path.exists(os.path.join(plain, "cam_pose_refine.json"))
    scorer.close()
