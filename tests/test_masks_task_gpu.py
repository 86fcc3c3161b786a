"""The task-mask rules of scene_model.TaskModel through the LUT kernel, on a three-object scene with the expected values written
out by hand, and the RGBA export of the task images."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _scene():
    from dream2real_amd.scene_model import ObjectModel, SceneModel
    bg, a, b, c = (ObjectModel(n, None, None, None, None, k) for k, n in enumerate(["bground", "cup", "plate", "fork"]))
    masks = np.array([[[0, 1, 2, 3], [3, 2, 1, 0]]], np.uint8)
    oob = np.array([[[0, 0, 0, 0], [255, 0, 0, 0]]], np.uint8)
    scene = SceneModel(np.zeros(3), [bg, a, b, c], bg, np.zeros((1, 2, 4, 3), np.uint8), None, None, None, masks, None, "shopping")
    return scene, a, [b], oob


def test_task_masks_by_hand(ctx, monkeypatch):
    from dream2real_amd import pcd_visual_model, scene_model
    seen = []
    monkeypatch.setattr(pcd_visual_model, "get_vis_pcds", lambda *a, **k: (seen.append(np.array(a[4])), ["pcd"])[1])
    scene, movable, relevant, oob = _scene()
    # movable (1), background (0) and the distractor (3) are masked, the relevant plate (2) is not; the out-of-scene pixel is
    obj, m = scene_model.TaskModel.create_task_bground_obj(scene, movable, relevant, oob, None, use_vis_pcds=True, ctx=ctx)
    assert m.tolist() == [[[1, 1, 0, 1], [1, 0, 1, 1]]] and obj.name == "__task_bground__" and obj.vis_model == "pcd"
    # render_distractors: only the movable object (and out of scene)
    _, m = scene_model.TaskModel.create_task_bground_obj(scene, movable, relevant, oob, None, use_vis_pcds=True, render_distractors=True, ctx=ctx)
    assert m.tolist() == [[[0, 1, 0, 0], [1, 0, 1, 0]]]
    assert scene_model.TaskModel.create_movable_vis_model(scene, movable, oob, None, use_vis_pcds=True, ctx=ctx) == "pcd"
    assert seen[-1].tolist() == [[[1, 0, 1, 1], [1, 1, 0, 1]]]                 # 0 on the movable object's pixels
    assert (seen[0] == [[[1, 1, 0, 1], [1, 0, 1, 1]]]).all()
    task = scene_model.TaskModel("put the cup on the plate", "cup on plate", [], scene, movable, obj, m, False)
    assert task.movable_masks.tolist() == [[[True, False, True, True], [True, True, False, True]]]
    with pytest.raises(NotImplementedError):                                    # get_vis_ngps is unchanged: no NeRF training here
        scene_model.TaskModel.create_movable_vis_model(scene, movable, oob, None, ctx=ctx)


def test_write_task_images_rgba(ctx, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from dream2real_amd import scene_model
    rng = np.random.default_rng(71)
    rgbs = rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    masks = (rng.random((2, 5, 7)) < 0.5).astype(np.uint8)
    for fg, sub in ((True, "images_fg"), (False, "images_bg")):
        out = scene_model.write_task_images(rgbs, masks, str(tmp_path), fg, ctx=ctx)
        assert out.endswith(sub)
        for k in range(2):
            im = np.asarray(Image.open(tmp_path / sub / ("rgb_%04d.png" % k)))
            assert im.shape == (5, 7, 4) and (im[..., :3] == rgbs[k]).all() and (im[..., 3] == 255 * (1 - masks[k])).all()
