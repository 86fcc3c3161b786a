"""tests/proposals_ref.py (DESIGN.md section 2h in numpy) against answers worked out by hand, and the argument errors
segmentation.proposals_to_labels raises before any device work.  No GPU."""
import numpy as np
import pytest

from dream2real_amd import segmentation
from tests import proposals_cases as pc
from tests import proposals_ref as ref


def run(case):
    P, inside = case
    return ref.proposals_to_labels(P, inside)


def test_boundary_counts_a_solid_rectangle_and_a_border_pixel():
    m = np.zeros((6, 7), bool)
    m[1:5, 2:7] = True                         # 4 x 5 touching the right border: its frame is 4 x 5 - 2 x 3 = 14 pixels
    assert ref.boundary(m).sum() == 14
    assert ref.boundary(np.ones((3, 3), bool)).sum() == 8


def test_hull_is_strictly_convex_counter_clockwise_from_the_lowest_y_then_x():
    m = np.zeros((5, 6), bool)
    m[1:4, 1:5] = True                         # collinear pixels on every side
    assert ref.hull(m) == [(1, 1), (4, 1), (4, 3), (1, 3)]
    tri = np.zeros((4, 4), bool)
    for k in range(4):
        tri[k, :4 - k] = True
    assert ref.hull(tri) == [(0, 0), (3, 0), (0, 3)]
    line = np.zeros((4, 4), bool)
    line[np.arange(4), np.arange(4)] = True
    assert ref.hull(line) == [(0, 0), (3, 3)]
    one = np.zeros((2, 2), bool)
    one[1, 0] = True
    assert ref.hull(one) == [(0, 1)]


def test_min_rect_of_a_rectangle_a_triangle_tie_and_a_diamond():
    assert ref.min_rect([(1, 1), (4, 1), (4, 3), (1, 3)]) == (9, 6, 9)                 # edge (3,0): ew = 3 * 3, eh = 3 * 2
    # right isosceles triangle with legs 3: the legs give 9 / 1 each, the hypotenuse (d = (-3, 3), dd = 18) gives 18 * 9 / 18: a tie, first edge
    assert ref.min_rect([(0, 0), (3, 0), (0, 3)]) == (9, 9, 9)
    # a diamond: every edge has d = (+-2, +-2), dd = 8, extents 8 x 8 -> side sqrt(8); an axis-aligned box would be 4 x 4 = 16 > 8
    assert ref.min_rect([(2, 0), (4, 2), (2, 4), (0, 2)]) == (8, 8, 8)
    assert ref.min_rect([(0, 0), (3, 3)]) == (0, 0, 0)
    assert ref.side_test(20 * 3, 99, 9) is False and ref.side_test(21 * 3, 99, 9) is True          # a side of exactly 20 is not above it


def test_scene_bound_and_empties_and_cuts():
    labels, recs, inter = run(pc.scene_bound_and(True))
    assert recs[:, 0].tolist() == [484, 0, 23 * 20] and recs[:, 1].tolist() == [1, 0, 1]
    assert recs[:, 2].tolist() == [0, 1, 4] and recs[:, 3].tolist() == [1, 0, 0]            # C is cut to 20 columns: centres 19 apart
    assert recs[1, 4:].tolist() == [0, 0, 0, 0]
    assert (labels == 1).sum() == 484 and labels[2, 2] == 1 and labels.max() == 1
    labels, recs, inter = run(pc.scene_bound_and(False))
    # B (484) and C (690) share 12 rows x 6 columns: above a tenth of B, which goes; A and C share 4 x 4, under a tenth of either
    assert recs[:, 2].tolist() == [0, 3, 0] and recs[:, 3].tolist() == [1, 0, 2] and inter[1, 2] == 12 * 6
    assert inter[0, 2] == 4 * 4 and inter[0, 1] == 0 and labels[21, 21] == 2 and labels[19, 21] == 1


def test_gap_of_four_joins_and_five_does_not():
    _, recs, _ = run(pc.blob_gaps())
    assert recs[:, 1].tolist() == [1, 2, 1, 2, 1] and recs[:, 2].tolist() == [0, 1, 0, 1, 0]
    assert recs[:, 0].tolist() == [968] * 5 and recs[:, 4].tolist() == [84] * 5              # a 22 x 22 blob has 4 * 21 boundary pixels
    assert recs[0, 5:].tolist() == [21 * 21, 21 * 21, 21 * 21]


def test_diagonal_touch_is_one_component():
    _, recs, _ = run(pc.diagonal_touch())
    assert recs[:, 1].tolist() == [1, 1] and recs[0, 4] == 168 and recs[1, 4] == 2 * (16 + 22) - 4 + 84


@pytest.mark.parametrize("w,h,rows,cols", pc.LARGE)
def test_large_is_above_three_tenths(w, h, rows, cols):
    labels, recs, _ = run(pc.large_threshold(w, h, rows, cols))
    assert recs[:, 0].tolist() == [rows * cols, rows * cols + 1] and recs[:, 2].tolist() == [0, 2]
    assert (labels == 1).sum() == rows * cols and labels.max() == 1


def test_subpart_rules():
    labels, recs, inter = run(pc.subpart_equality(False))
    assert inter[0, 1] == 100 and recs[:, 2].tolist() == [0, 0] and labels[2, 38] == 2 and labels[2, 37] == 1
    labels, recs, inter = run(pc.subpart_equality(True))
    assert inter[0, 1] == 101 and recs[:, 2].tolist() == [3, 0] and recs[:, 3].tolist() == [0, 1] and labels[2, 2] == 0
    _, recs, inter = run(pc.subpart_equal_areas())
    assert inter[0, 1] == 200 and recs[:, 2].tolist() == [0, 3]
    _, recs, inter = run(pc.subpart_chain())
    assert (inter[0, 1], inter[1, 2], inter[0, 2]) == (175, 120, 0) and recs[:, 2].tolist() == [0, 3, 3]
    labels, recs, inter = run(pc.survivors_overlap())
    assert inter[0, 1] == 75 and recs[:, 3].tolist() == [1, 2] and (labels == 2).sum() == 1000 and (labels == 1).sum() == 925


def test_small_by_area_and_by_side():
    _, recs, _ = run(pc.small_area())
    assert recs[:, 0].tolist() == [79, 80] and recs[:, 2].tolist() == [4, 0]
    assert recs[0, 5:].tolist() == [39 * 39, 39 * 39, 39 * 39]        # the legs' rectangle ties the hypotenuse's: the first edge, a leg
    assert recs[1, 6] == 39 * 39 and recs[1, 5] * 39 * 39 == recs[1, 6] * recs[1, 7]          # the same area from whichever edge came first
    for w, h in pc.SIZES:
        _, recs, _ = run(pc.small_side_axis(w, h))
        assert recs[:, 2].tolist() == [4, 0], (w, h)
        assert recs[0, 5:].tolist() == [20 * 20, 25 * 20, 20 * 20] and recs[1, 5:].tolist() == [21 * 21, 25 * 21, 21 * 21]
    _, recs, _ = run(pc.thin_shapes())
    assert recs[:, 0].tolist() == [40, 1, 0] and recs[:, 1].tolist() == [1, 1, 0] and recs[:, 2].tolist() == [4, 4, 1]
    assert recs[:, 4].tolist() == [40, 1, 0] and not recs[:, 5:].any()


@pytest.mark.parametrize("half_short,kept", [(78, False), (82, True)])
def test_rotated_rectangle_is_measured_along_its_own_axes(half_short, kept):
    P, _ = pc.rotated_rect(70, 45, half_short)
    _, recs, _ = run((P, None))
    ew, eh, dd = (int(v) for v in recs[0, 5:])
    # the chosen edge runs along (7, 4) or (-4, 7): dd = 65 k^2, and the short side is 2 half_short / sqrt(65)
    k = round((dd / 65) ** 0.5)
    assert dd == 65 * k * k and min(ew, eh) == 2 * half_short * k
    rows, cols = np.nonzero(P[0])
    assert min(np.ptp(rows), np.ptp(cols)) > 25                                  # an axis-aligned box would pass either way
    assert recs[0, 1] == 1 and (recs[0, 2] == 0) == kept and recs[0, 2] in (0, 4)
    assert (19 * 19 * 65 < 4 * half_short ** 2 < 400 * 65) != kept


def test_component_choice_by_boundary_pixels_and_the_tie():
    P, _ = pc.ring_and_disc()
    ring, solid = P[0].copy(), P[0].copy()
    ring[:, 34:] = False
    solid[:, :34] = False
    assert ring.sum() < solid.sum() and ref.boundary(ring).sum() > ref.boundary(solid).sum()
    _, recs, _ = run((P, None))
    assert recs[0, 1] == 1 and recs[0, 4] == ref.boundary(ring).sum()
    assert recs[0, 5:].tolist() == list(ref.min_rect(ref.hull(ring)))
    _, recs, _ = run(pc.boundary_tie())
    assert recs[0, 1] == 1 and recs[0, 4] == 36 and recs[0, 5:].tolist() == [11 * 11, 7 * 11, 11 * 11]


def test_empty_input():
    labels, recs, inter = ref.proposals_to_labels(np.zeros((0, 33, 65), bool))
    assert labels.shape == (33, 65) and not labels.any() and recs.shape == (0, 8) and inter.shape == (0, 0)


def test_argument_errors_come_before_the_device():
    with pytest.raises(ValueError, match="M, H, W"):
        segmentation.proposals_to_labels(np.zeros((4, 4), bool), ctx=None)
    with pytest.raises(ValueError, match="at most 1024"):
        segmentation.proposals_to_labels(np.zeros((1025, 2, 2), bool), ctx=None)
    with pytest.raises(ValueError, match="height and a width"):
        segmentation.proposals_to_labels(np.zeros((2, 3, 0), bool), ctx=None)
    with pytest.raises(ValueError, match="inside must be"):
        segmentation.proposals_to_labels(np.zeros((2, 3, 4), bool), np.zeros((4, 3), bool), ctx=None)


def test_one_callable_without_the_other_is_refused(tmp_path):
    from dream2real_amd.dream2real import ImaginationEngine, PathConfig
    cfg = PathConfig(data_dir=str(tmp_path), sample_res=[2, 2, 1, 1, 1, 1])
    with pytest.raises(ValueError, match="tracker= is missing"):
        ImaginationEngine(cfg, None, None, proposer=lambda image: None)
    with pytest.raises(ValueError, match="proposer= is missing"):
        ImaginationEngine(cfg, None, None, tracker=lambda frames, labels0: None)


@pytest.mark.parametrize("w,h", pc.LABELLER_SIZES)
def test_the_two_numpy_component_counts_agree_on_the_labeller_cases(w, h):
    """The flood fill of masks_ref and the minimum propagation proposals_ref counts with: one number per image, both sources of the
    GPU cross-check (test_proposals_gpu.py) are held to it."""
    from tests import masks_ref
    for name, B in pc.labeller_images(w, h).items():
        assert B.shape == (h, w) and B.dtype == np.uint8 and B.max() <= 1, name
        D = masks_ref.dilate(B, 5, fast=True)
        flood = masks_ref.components(D)
        fast = masks_ref.components_fast(D)
        n_flood = int((flood.ravel() == np.arange(h * w)).sum())
        assert n_flood == len(np.unique(fast[D != 0])), (name, w, h)
        assert (flood == fast).all(), (name, w, h)
