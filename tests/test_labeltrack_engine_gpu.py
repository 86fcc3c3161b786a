"""ImaginationEngine with tracker="geometric" on the scan folder of tests/test_engine_gpu.py: build_scene_model turns the proposer's
masks into the first label image, carries it through the scan by geometry (section 2k) and refines what comes
back, all on the GPU; a callable tracker is called as before; any other name is refused."""
import numpy as np
import pytest

from dream2real_amd import segmentation
from dream2real_amd.dream2real import ImaginationEngine
from tests import test_engine_gpu as scan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def test_build_scene_model_with_the_geometric_tracker(ctx, tmp_path):
    rgbs, mm, raw_labels, poses = scan._frames()
    d = str(tmp_path / "scan")
    scan._write_scan(d, rgbs, mm, poses)
    truth0 = [np.rot90(raw_labels[0] == k, 1) for k in (1, 2)]           # the true masks of frame 0, on the upright frame

    def proposer(image):
        assert image.shape == (scan.W, scan.H, 3)
        return np.stack(truth0)

    cfg = scan._engine_cfg(tmp_path, d, use_cache_segs=False)
    eng = ImaginationEngine(cfg, ctx, None, intrinsics=scan.K, proposer=proposer, tracker="geometric")
    eng.build_scene_model(captions=scan.CAPTIONS)

    from dream2real_amd.data_loader import d2r_dataloader
    loader = d2r_dataloader(cfg, ctx)
    _, depths, T_WC = loader.load_rgbds()
    oob = loader.remove_background(scan.K, scan.BOUNDS)
    labels0 = np.ascontiguousarray(np.rot90(segmentation.proposals_to_labels(np.stack(truth0), np.rot90(np.asarray(oob[0]) == 0), ctx=ctx), 3))
    assert sorted(np.unique(labels0).tolist()) == [0, 1, 2]
    tracked, stats = segmentation.track_labels(depths, T_WC, scan.K, labels0, scan.BOUNDS, ctx=ctx, return_stats=True)
    print("stats:", stats.tolist())
    assert tracked.shape == raw_labels.shape and np.array_equal(tracked[0], labels0) and (stats[1:, 0] > 0).all()
    want = segmentation.refine_masks(tracked, depths, T_WC, scan.K, oob, scan.CENTRE, None, ctx=ctx)
    assert np.array_equal(eng.scene_model.masks, want)
    assert all((want[1:] == k).any() for k in (1, 2))                    # both boxes were carried beyond frame 0
    inside = np.asarray(oob) == 0
    print(f"tracked and refined masks equal the true labels on {(want == raw_labels)[inside].mean():.4f} of the pixels inside the scene bounds")


def test_a_callable_tracker_is_called_as_before(ctx, tmp_path):
    rgbs, mm, raw_labels, poses = scan._frames()
    d = str(tmp_path / "scan")
    scan._write_scan(d, rgbs, mm, poses)
    seen = {}

    def tracker(frames, labels0):
        seen["labels0"] = np.array(labels0)
        return raw_labels

    cfg = scan._engine_cfg(tmp_path, d, use_cache_segs=False)
    eng = ImaginationEngine(cfg, ctx, None, intrinsics=scan.K, proposer=lambda image: np.stack([np.rot90(raw_labels[0] == k, 1) for k in (1, 2)]),
                            tracker=tracker)
    eng.build_scene_model(captions=scan.CAPTIONS)
    assert seen["labels0"].shape == (scan.H, scan.W)
    from dream2real_amd.data_loader import d2r_dataloader
    loader = d2r_dataloader(cfg, ctx)
    _, depths, T_WC = loader.load_rgbds()
    oob = loader.remove_background(scan.K, scan.BOUNDS)
    assert np.array_equal(eng.scene_model.masks, segmentation.refine_masks(raw_labels, depths, T_WC, scan.K, oob, scan.CENTRE, None, ctx=ctx))


def test_another_tracker_name_is_refused(tmp_path):
    cfg = scan._engine_cfg(tmp_path, str(tmp_path))
    with pytest.raises(ValueError, match="xmem"):
        ImaginationEngine(cfg, None, None, proposer=lambda image: None, tracker="xmem")
