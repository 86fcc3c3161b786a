"""ImaginationEngine with proposer= and tracker=: build_scene_model turns the proposer's masks into the first label image on the GPU
(DESIGN.md section 2h), hands it to the tracker and refines what comes back, on the scan folder of tests/test_engine_gpu.py."""
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


def _proposals():
    """Three rectangles on the upright first frame [W, H]: two objects and a sliver that the small rule drops."""
    P = np.zeros((3, scan.W, scan.H), bool)
    P[0, 70:100, 30:60] = True
    P[1, 105:135, 50:80] = True
    P[2, 20:60, 10:14] = True
    return P


def test_build_scene_model_from_a_proposer_and_a_tracker(ctx, tmp_path):
    rgbs, mm, _, poses = scan._frames()
    d = str(tmp_path / "scan")
    scan._write_scan(d, rgbs, mm, poses)
    seen = {}

    def proposer(image):
        seen["image"] = np.array(image)
        return _proposals()

    def tracker(frames, labels0):
        seen["labels0"] = np.array(labels0)
        return np.repeat(np.asarray(labels0)[None], len(frames), axis=0)

    cfg = scan._engine_cfg(tmp_path, d, use_cache_segs=False)
    eng = ImaginationEngine(cfg, ctx, None, intrinsics=scan.K, proposer=proposer, tracker=tracker)
    # the first label image by hand, from the same scene-bound mask the engine builds
    from dream2real_amd.data_loader import d2r_dataloader
    loader = d2r_dataloader(cfg, ctx)
    frames, depths, T_WC = loader.load_rgbds()
    oob = loader.remove_background(scan.K, scan.BOUNDS)
    labels0 = np.rot90(segmentation.proposals_to_labels(_proposals(), np.rot90(np.asarray(oob[0]) == 0), ctx=ctx), 3)
    n_labels = int(labels0.max())
    assert 1 <= n_labels <= 2 and labels0.shape == (scan.H, scan.W)
    eng.build_scene_model(captions=["__background__"] + ["box %d" % k for k in range(n_labels)])
    assert seen["image"].shape == (scan.W, scan.H, 3) and np.array_equal(seen["image"], np.rot90(rgbs[0], 1))
    assert np.array_equal(seen["labels0"], labels0)
    raw = np.repeat(labels0[None], len(rgbs), axis=0)
    want = segmentation.refine_masks(raw, depths, T_WC, scan.K, oob, scan.CENTRE, None, ctx=ctx)
    assert np.array_equal(eng.scene_model.masks, want) and (want == 1).any()
    assert np.array_equal(eng.out_scene_bound_masks, oob)


def test_one_callable_without_the_other_is_refused(tmp_path):
    cfg = scan._engine_cfg(tmp_path, str(tmp_path))
    with pytest.raises(ValueError, match="tracker= is missing"):
        ImaginationEngine(cfg, None, None, proposer=lambda image: None)
    with pytest.raises(ValueError, match="proposer= is missing"):
        ImaginationEngine(cfg, None, None, tracker=lambda frames, labels0: None)
