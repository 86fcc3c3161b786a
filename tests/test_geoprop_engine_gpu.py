"""ImaginationEngine with proposer="geometric", tracker="geometric" on the scan folder of tests/test_engine_gpu.py: build_scene_model
takes its proposals from frame 0's depth and the support plane, turns them into the first label image (2h),
carries it through the scan (2k) and refines what comes back, all on the GPU and without a segmentation callable."""
import numpy as np
import pytest

from dream2real_amd import segmentation
from dream2real_amd.dream2real import ImaginationEngine
from tests import test_engine_gpu as scan
from tests.test_geoprop_host import CHAIN_AGREEMENT, MARGIN, agreement_with_matched_numbers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def test_build_scene_model_without_a_segmentation_callable(ctx, tmp_path):
    rgbs, mm, raw_labels, poses = scan._frames()
    d = str(tmp_path / "scan")
    scan._write_scan(d, rgbs, mm, poses)
    cfg = scan._engine_cfg(tmp_path, d, use_cache_segs=False)
    eng = ImaginationEngine(cfg, ctx, None, intrinsics=scan.K, proposer="geometric", tracker="geometric")
    eng.build_scene_model(captions=scan.CAPTIONS)

    from dream2real_amd.data_loader import d2r_dataloader
    loader = d2r_dataloader(cfg, ctx)
    _, depths, T_WC = loader.load_rgbds()
    oob = loader.remove_background(scan.K, scan.BOUNDS)
    masks, recs, plane = segmentation.propose_masks(depths[0], T_WC[0], scan.K, scan.BOUNDS, ctx=ctx)
    print("plane record:", plane, "records:", recs.tolist())
    assert masks.shape == (2, scan.H, scan.W)                             # the true object count
    labels0 = np.ascontiguousarray(np.rot90(segmentation.proposals_to_labels(np.rot90(masks, 1, axes=(1, 2)), np.rot90(np.asarray(oob[0]) == 0),
                                                                             ctx=ctx), 3))
    assert sorted(np.unique(labels0).tolist()) == [0, 1, 2]
    tracked = segmentation.track_labels(depths, T_WC, scan.K, labels0, scan.BOUNDS, ctx=ctx)
    want = segmentation.refine_masks(tracked, depths, T_WC, scan.K, oob, scan.CENTRE, None, ctx=ctx)
    assert np.array_equal(eng.scene_model.masks, want)
    assert sorted(set(np.unique(want).tolist()) - {255}) == [0, 1, 2] and all((want == k).any(axis=(1, 2)).all() for k in (1, 2))      # the background and two boxes, in every frame
    got = agreement_with_matched_numbers(want, raw_labels, np.asarray(oob) == 0)
    print(f"kept masks equal the true labels (proposal numbers matched on frame 0) on {got:.4f} of the pixels inside the scene bounds")
    assert got >= CHAIN_AGREEMENT - MARGIN


def test_the_shelf_and_unknown_names_are_refused(tmp_path):
    cfg = scan._engine_cfg(tmp_path, str(tmp_path))
    with pytest.raises(ValueError, match="sam"):
        ImaginationEngine(cfg, None, None, proposer="sam", tracker="geometric")
    shelf = scan._engine_cfg(tmp_path, str(tmp_path), scene_type=1)
    with pytest.raises(ValueError, match="scene_type 1"):
        ImaginationEngine(shelf, None, None, proposer="geometric", tracker="geometric")
