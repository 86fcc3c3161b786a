"""The host side of the scan-folder engine (dream2real.py): PathConfig.from_json on the reference's settings format, the rule that
turns the label census into an object count, CachedLangModel's file, and the paths of build_scene_model / interpret_user_instr
that refuse.  No GPU: frames and scene-bound masks come from files the tests write, and where a test has to get past the census
it stands np.bincount in for the kernel."""
import dataclasses
import json
import os

import numpy as np
import pytest

from dream2real_amd import _lib, segmentation
from dream2real_amd.dream2real import CachedLangModel, ImaginationEngine, PathConfig

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ENGINE_GROUP = {
    "inpaint_holes": False, "caption": True, "visseg": False, "render_distractors": True, "spatial_smoothing": False, "physics_only": True,
    "use_vis_pcds": True, "pcds_type": 1, "single_view_idx": 2, "use_cache_dynamic_masks": True, "use_cache_segs": True,
    "use_cache_cam_poses": True, "use_cache_captions": True, "use_cache_phys": True, "use_cache_vis": True, "use_cache_renders": True,
    "use_cache_goal_pose": True, "use_phys": False, "use_phys_tsdf": False, "lazy_phys_mods": False, "multi_view_captions": True,
    "use_cache_llm": True, "scene_type": 1, "sample_res": [5, 4, 3, 2, 1, 1], "scene_centre": [0.1, 0.2, 0.3],
    "scene_phys_bounds": [[-1.0, -2.0, -3.0], [1.0, 2.0, 3.0]], "render_cam_pose_idx": [1, 3], "phys_backend": "tsdf"}


def _write(tmp_path, engine, camera=None, **groups):
    path = str(tmp_path / "settings.json")
    with open(path, "w") as f:
        json.dump({"dataset": {"files": "transforms.json"}, "engine": engine, "camera": camera or {"w": 640, "h": 360, "fx": 1.0}, **groups}, f)
    return path


def test_from_json_reproduces_every_field(tmp_path):
    """Every field of PathConfig that the file carries comes back as written (each boolean the opposite of its default, so a field
    that was not read shows); the groups the path never reads may hold anything or be absent."""
    cfg = PathConfig.from_json(_write(tmp_path, ENGINE_GROUP, trainer="not even a group", robot={"x": 1}), "/data/scan", embodied=True)
    want = {k: v for k, v in ENGINE_GROUP.items() if k not in ("inpaint_holes", "caption", "visseg")}
    want.update(data_dir="/data/scan", width=640, height=360, embodied=True, resolution=None, save_renders=True)
    got = dataclasses.asdict(cfg)
    assert got == want
    for f in dataclasses.fields(PathConfig):                          # and each differs from the default, except the two the format lacks
        if f.name not in ("data_dir", "sample_res", "resolution", "save_renders"):
            assert got[f.name] != f.default, f.name


def test_from_json_defaults_and_missing_keys(tmp_path):
    """single_view_idx defaults to 0, pcds_type is None (and not needed) without use_vis_pcds, phys_backend defaults to "hulls"; a
    missing key the path needs is a KeyError naming group.key."""
    engine = {k: v for k, v in ENGINE_GROUP.items() if k not in ("single_view_idx", "pcds_type", "phys_backend")}
    engine["use_vis_pcds"] = False
    cfg = PathConfig.from_json(_write(tmp_path, engine), "d")
    assert cfg.single_view_idx == 0 and cfg.pcds_type is None and cfg.phys_backend == "hulls" and cfg.use_vis_pcds is False
    engine["use_vis_pcds"] = True
    with pytest.raises(KeyError, match=r"engine\.pcds_type"):
        PathConfig.from_json(_write(tmp_path, engine), "d")
    for key in ("use_cache_segs", "scene_phys_bounds", "sample_res", "use_phys_tsdf"):
        with pytest.raises(KeyError, match=r"engine\." + key):
            PathConfig.from_json(_write(tmp_path, {k: v for k, v in ENGINE_GROUP.items() if k != key}), "d")
    with pytest.raises(KeyError, match=r"camera\.h"):
        PathConfig.from_json(_write(tmp_path, ENGINE_GROUP, camera={"w": 640}), "d")
    path = str(tmp_path / "no_engine.json")
    json.dump({"camera": {"w": 1, "h": 1}}, open(path, "w"))
    with pytest.raises(KeyError, match=r"engine\.sample_res"):
        PathConfig.from_json(path, "d")


def test_from_json_reads_a_settings_file_of_the_reference():
    """tests/golden/ref_config_shopping_pcd.json is the reference's configs/shopping/pcd.json, byte for byte."""
    cfg = PathConfig.from_json(os.path.join(GOLDEN, "ref_config_shopping_pcd.json"), "/scan")
    assert cfg.use_vis_pcds is True and cfg.pcds_type == 0 and cfg.single_view_idx == 0 and cfg.scene_type == 3
    assert cfg.sample_res == [100, 100, 7, 1, 1, 1] and cfg.scene_centre == [0.5, 0.0, 0.035] and cfg.render_cam_pose_idx == [0]
    assert cfg.scene_phys_bounds == [[0.2, -0.4, 0.0], [1.0, 1.4, 1.2]] and (cfg.width, cfg.height) == (1280, 720)
    assert cfg.use_cache_dynamic_masks and cfg.use_cache_segs and cfg.use_cache_cam_poses and cfg.use_cache_llm
    assert not (cfg.use_cache_captions or cfg.use_cache_phys or cfg.use_cache_vis or cfg.use_cache_renders or cfg.use_cache_goal_pose)
    assert cfg.use_phys and cfg.use_phys_tsdf and cfg.lazy_phys_mods and cfg.spatial_smoothing
    assert not (cfg.multi_view_captions or cfg.render_distractors or cfg.physics_only or cfg.embodied)
    assert cfg.phys_backend == "hulls" and cfg.data_dir == "/scan"


def _counts(*frames):
    return np.stack([np.bincount(np.asarray(f, np.uint8).ravel(), minlength=256) for f in frames]).astype(np.uint32)


def test_census_rule_against_bincount():
    """labels and num_objs from per-frame counts: {0,1,2}; {0,1,2,255} (255 is no object); a gap raises and names the missing label;
    255 alone is no object at all."""
    labels, n = segmentation.labels_from_census(_counts([0, 0, 1], [2, 2, 0]))
    assert labels.tolist() == [0, 1, 2] and n == 3
    labels, n = segmentation.labels_from_census(_counts([0, 255, 1], [2, 255, 255]))
    assert labels.tolist() == [0, 1, 2, 255] and n == 3
    with pytest.raises(ValueError, match=r"but not 1\b"):
        segmentation.labels_from_census(_counts([0, 0, 2, 255]))
    with pytest.raises(ValueError, match=r"but not 0\b"):
        segmentation.labels_from_census(_counts([1, 2]))
    labels, n = segmentation.labels_from_census(_counts([255, 255]))
    assert labels.tolist() == [255] and n == 0
    big = np.zeros((3, 256), np.uint32)                               # totals past 2^32 do not wrap to "absent"
    big[:, 1] = 2 ** 31
    big[0, 0] = 1
    assert segmentation.labels_from_census(big)[1] == 2


def test_cached_lang_model_round_trips_its_file(tmp_path):
    path = str(tmp_path / "lang.json")
    caps = ["__background__", "red box", "blue box"]
    lm = CachedLangModel(path)
    lm.record("parse_instr", ["put the red box next to the blue box"], ["a red box next to a blue box", "a red box and a blue box"])
    lm.record("get_movable_obj_idx", ["put the red box next to the blue box", caps], 1)
    lm.record("get_relevant_obj_idxs", ["a red box next to a blue box", caps, 1], [1, 2])
    lm.save()
    table = json.load(open(path))
    assert sorted(table) == sorted(CachedLangModel.METHODS) and all(len(t) == 1 for t in table.values())
    again = CachedLangModel(path)
    assert again.parse_instr("put the red box next to the blue box") == ("a red box next to a blue box", "a red box and a blue box")
    assert again.get_movable_obj_idx("put the red box next to the blue box", caps) == 1
    assert again.get_relevant_obj_idxs("a red box next to a blue box", tuple(caps), 1) == [1, 2]
    with pytest.raises(KeyError, match="get_movable_obj_idx"):
        again.get_movable_obj_idx("another instruction", caps)
    with pytest.raises(ValueError, match="unknown method"):
        again.record("chat", [], "")
    json.dump({"chat": {}}, open(path, "w"))
    with pytest.raises(ValueError, match="unknown method"):
        CachedLangModel(path)


def _scan_folder(tmp_path, labels):
    """A scan folder of len(labels) tiny frames whose scene-bound masks are already cached, so that nothing needs a GPU."""
    d = str(tmp_path / "scan")
    n, (h, w) = len(labels), labels[0].shape
    for sub in ("images", "depth", "XMem_masks"):
        os.makedirs(os.path.join(d, sub))
    np.savetxt(os.path.join(d, "poses.txt"), np.tile(np.eye(4).reshape(1, 16), (n, 1)))
    for k in range(n):
        _lib.png_write(np.full((h, w, 3), 9 * k, np.uint8), os.path.join(d, "images", "rgb_%04d.png" % k))
        from PIL import Image
        Image.fromarray(np.full((h, w), 500 + k, np.uint16)).save(os.path.join(d, "depth", "depth_%04d.png" % k))
        _lib.png_write_channels(np.zeros((h, w), np.uint8), os.path.join(d, "images", "dynamic_mask_rgb_%04d.png" % k))
        _lib.png_write_channels(labels[k], os.path.join(d, "XMem_masks", "rgb_%04d.png" % k))
    np.save(os.path.join(d, "opt_cam_poses.npy"), np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)))
    return d


def _cfg(d, **over):
    base = dict(data_dir=d, sample_res=[2, 2, 1, 1, 1, 1], use_vis_pcds=True, pcds_type=0, use_cache_dynamic_masks=True, use_cache_segs=True,
                use_cache_cam_poses=True, scene_centre=[0.0, 0.0, 0.0], scene_phys_bounds=[[-1, -1, -1], [1, 1, 1]], width=8, height=6)
    base.update(over)
    return PathConfig(**base)


def test_engine_refuses_as_specified(tmp_path, monkeypatch):
    """interpret_user_instr before build_scene_model; build_scene_model with neither cached masks nor a segmentor (the message names
    both ways in); without cached poses or use_vis_pcds (NeRF training); a caption list of the wrong length or without
    "__background__" first; labels with a gap.  Then the same folder with the right captions builds: objects, masks, census."""
    labels = np.zeros((2, 6, 8), np.uint8)
    labels[0, :2] = 1
    labels[1, 3:] = 2
    labels[1, 0, 0] = 255
    d = _scan_folder(tmp_path, labels)
    eng = ImaginationEngine(_cfg(d), None, None)
    assert eng.intrinsics[0, 0] == 924.66912 and eng.intrinsics[1, 2] == 355.18523        # the 1280-wide RealSense matrix by default
    with pytest.raises(RuntimeError, match="build_scene_model"):
        eng.interpret_user_instr("put the box down")
    with pytest.raises(RuntimeError, match=r"SAM and XMem.*use_cache_segs.*segmentor="):
        ImaginationEngine(_cfg(d, use_cache_segs=False), None, None).build_scene_model()
    monkeypatch.setattr(_lib, "masks_census", lambda ctx, m: _counts(*np.asarray(m)))      # past here the census would need the GPU
    with pytest.raises(NotImplementedError, match="NeRF training"):
        ImaginationEngine(_cfg(d, use_cache_cam_poses=False, use_vis_pcds=False, pcds_type=None), None, None).build_scene_model()
    with pytest.raises(ValueError, match="2 captions"):
        eng.build_scene_model(captions=["__background__", "box"])
    with pytest.raises(ValueError, match="__background__"):
        eng.build_scene_model(captions=["table", "box", "cup"])
    with pytest.raises(RuntimeError, match="captioning models are out of scope"):
        ImaginationEngine(_cfg(d, use_cache_captions=True), None, None).build_scene_model()
    assert eng.scene_model is None
    eng.build_scene_model(captions=["__background__", "box", "cup"])
    sm = eng.scene_model
    assert [o.name for o in sm.objs] == ["__background__", "box", "cup"] and [o.mask_idx for o in sm.objs] == [0, 1, 2]
    assert sm.bground_obj is sm.objs[0] and all(o.phys_model is None and o.vis_model is None and o.thumbnail is None for o in sm.objs)
    np.testing.assert_array_equal(sm.masks, labels)
    np.testing.assert_array_equal(eng.label_counts, _counts(*labels))
    assert eng.depths_gt.shape == (1, 6, 8) and len(sm.opt_cam_poses) == 2 and eng.out_scene_bound_masks.shape == (2, 6, 8)
    assert json.load(open(os.path.join(d, "captions.json"))) == ["__background__", "box", "cup"]      # where the reference's engine keeps them
    again = ImaginationEngine(_cfg(d, use_cache_captions=True), None, None)
    again.build_scene_model()
    assert [o.name for o in again.scene_model.objs] == ["__background__", "box", "cup"]
    with pytest.raises(RuntimeError, match="lang_model"):
        eng.interpret_user_instr("put the box down")
    gap = labels.copy()
    gap[gap == 1] = 0
    d2 = _scan_folder(tmp_path / "gap", gap)
    with pytest.raises(ValueError, match=r"but not 1\b"):
        ImaginationEngine(_cfg(d2), None, None).build_scene_model(captions=["__background__", "cup"])


def test_library_holds_the_census_kernel():
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"k_census" in blob and b"gfx950" in blob
