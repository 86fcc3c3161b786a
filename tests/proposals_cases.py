"""Deterministic proposals for the tests of DESIGN.md section 2h, shared by the host and the GPU tests.  Every builder returns
(proposals bool [M,H,W], inside bool [H,W] or None).  The image sizes (W x H) cross no word boundary of the bit-packed rows, land
exactly on one, pass one by a single bit, and cross two; every height crosses at least two 16-row labelling tiles."""
from __future__ import annotations

import numpy as np

SIZES = ((70, 45), (64, 40), (65, 33), (130, 50))          # W x H


def blank(m, w, h):
    return np.zeros((m, h, w), bool)


def rect(img, r0, c0, rows, cols):
    img[r0:r0 + rows, c0:c0 + cols] = True
    return img


def scene_bound_and(with_inside=True):
    """70 x 45: A lies inside the scene, B wholly in the columns the scene mask clears, C half in them."""
    P = blank(3, 70, 45)
    rect(P[0], 2, 2, 22, 22)
    rect(P[1], 10, 44, 22, 22)
    rect(P[2], 20, 20, 23, 30)
    inside = np.ones((45, 70), bool)
    inside[:, 40:] = False
    return P, (inside if with_inside else None)


def touches_all_borders(w, h):
    """A one-pixel frame around the image and a plus of three-pixel bars from border to border: the dilation window is cut on every side."""
    P = blank(2, w, h)
    P[0, 0, :] = P[0, -1, :] = True
    P[0, :, 0] = P[0, :, -1] = True
    P[1, h // 2 - 1:h // 2 + 2, :] = True
    P[1, :, w // 2 - 1:w // 2 + 2] = True
    return P, None


def blob_gaps():
    """130 x 50, two 22 x 22 blobs per mask: 4 unset columns between them (the 5 x 5 dilation joins them: kept), 5 (dropped), the
    same two gaps between rows, and the 4-gap sitting right before the word boundary at column 64."""
    P = blank(5, 130, 50)
    rect(rect(P[0], 2, 10, 22, 22), 2, 36, 22, 22)          # columns 10..31, 36..57: gap 32..35
    rect(rect(P[1], 2, 10, 22, 22), 2, 37, 22, 22)          # gap of 5
    rect(rect(P[2], 0, 86, 22, 22), 26, 86, 22, 22)         # rows 0..21, 26..47: gap of 4 rows
    rect(rect(P[3], 0, 108, 22, 22), 27, 108, 22, 22)       # gap of 5 rows
    rect(rect(P[4], 24, 38, 22, 22), 24, 64, 22, 22)        # columns 38..59, 64..85: the gap is the last four bits of word 0
    return P, None


def diagonal_touch():
    """130 x 50: two blobs that touch only diagonally are one 8-connected component; the second pair touches across the corner
    where a labelling tile's row 16 and the word boundary at column 64 meet."""
    P = blank(2, 130, 50)
    rect(rect(P[0], 2, 2, 22, 22), 24, 24, 22, 22)
    rect(rect(P[1], 0, 42, 16, 22), 16, 64, 22, 22)
    return P, None


def large_threshold(w, h, rows, cols):
    """rows x cols = 0.3 w h exactly (kept), and one pixel more (dropped as large)."""
    assert (w * h) % 10 == 0 and rows * cols * 10 == 3 * w * h
    P = blank(2, w, h)
    rect(P[0], 1, 1, rows, cols)
    rect(P[1], 1, 1, rows, cols)
    P[1, 1 + rows, 1] = True
    return P, None


LARGE = ((70, 45, 27, 35), (64, 40, 24, 32), (130, 50, 30, 65))


def subpart_equality(extra):
    """130 x 50: A and B of 1000 pixels share 100 (10 inter == area: both kept, B's label wins the overlap).  extra: B gains one
    more pixel inside A, so 10 * 101 > 1000 = area[A] < area[B] and A goes."""
    P = blank(2, 130, 50)
    rect(P[0], 2, 2, 25, 40)              # columns 2..41
    rect(P[1], 2, 38, 25, 40)             # columns 38..77
    if extra:
        P[1, 2, 37] = True
    return P, None


def subpart_equal_areas():
    """Equal areas and an overlap above a tenth: the later one goes."""
    P = blank(2, 130, 50)
    rect(P[0], 2, 2, 25, 40)
    rect(P[1], 2, 34, 25, 40)
    return P, None


def subpart_chain():
    """A (1500) removes B (1000), B although marked removes C (960); A and C do not meet.  Only A survives."""
    P = blank(3, 130, 50)
    rect(P[0], 2, 2, 30, 50)              # columns 2..51
    rect(P[1], 2, 45, 25, 40)             # columns 45..84: 25 x 7 = 175 shared with A
    rect(P[2], 2, 80, 24, 40)             # columns 80..119: 24 x 5 = 120 shared with B
    return P, None


def survivors_overlap():
    """A and B share 75 of their 1000 pixels: both survive, label 2 owns the overlap."""
    P = blank(2, 130, 50)
    rect(P[0], 2, 2, 25, 40)
    rect(P[1], 2, 39, 25, 40)
    return P, None


def small_area():
    """70 x 45: an L of two 40-pixel arms (79 pixels, hull a triangle whose smallest rectangle has a side above 20): dropped as small;
    the same L turned round elsewhere, with an 80th pixel inside the hull: kept."""
    P = blank(2, 70, 45)
    P[0, 2:42, 5] = True
    P[0, 2, 5:45] = True
    P[1, 4:44, 65] = True
    P[1, 43, 26:66] = True
    P[1, 42, 64] = True
    return P, None


def small_side_axis(w, h):
    """Rectangles 26 tall and 21 wide (centres 20 apart: dropped) and 22 wide (kept)."""
    P = blank(2, w, h)
    rect(P[0], 1, 3, 26, 21)
    rect(P[1], 1, 30, 26, 22)
    return P, None


def rotated_rect(w, h, half_short, half_long=130):
    """The lattice points with |7 dx + 4 dy| <= half_long and |-4 dx + 7 dy| <= half_short about the image centre: a rectangle turned
    by atan(4 / 7) = 29.7 degrees.  Its short side is 2 half_short / sqrt(65) where the bounding lines hold lattice points: 78 ->
    19.35, 82 -> 20.34."""
    P = blank(1, w, h)
    cy, cx = h // 2, w // 2
    dy, dx = np.mgrid[0:h, 0:w]
    dy, dx = dy - cy, dx - cx
    P[0] = (np.abs(7 * dx + 4 * dy) <= half_long) & (np.abs(-4 * dx + 7 * dy) <= half_short)
    return P, None


def thin_shapes():
    """70 x 45: a one-pixel-wide diagonal line (a hull of two vertices: side 0), a single pixel, an empty proposal."""
    P = blank(3, 70, 45)
    for k in range(40):
        P[0, 2 + k, 3 + k] = True
    P[1, 44, 69] = True
    return P, None


def disc(img, cy, cx, r2_lo, r2_hi):
    dy, dx = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    d2 = (dy - cy) ** 2 + (dx - cx) ** 2
    img |= (d2 >= r2_lo) & (d2 <= r2_hi)
    return img


def ring_and_disc():
    """130 x 50: a ring (outer radius 12, inner 9) three unset columns from a solid disc of radius 10: the ring has fewer pixels and
    more boundary pixels, so the rectangle is the ring's."""
    P = blank(1, 130, 50)
    disc(P[0], 20, 20, 81, 144)
    disc(P[0], 20, 46, 0, 100)            # columns 36..56; the ring ends at column 32
    return P, None


def boundary_tie():
    """70 x 45: an 8 x 12 rectangle and a 10 x 10 square, 36 boundary pixels each, three columns apart.  The rectangle's first pixel
    comes first in raster order, so the extents are its 11 and 7."""
    P = blank(1, 70, 45)
    rect(P[0], 3, 10, 8, 12)
    rect(P[0], 5, 25, 10, 10)
    return P, None


def random_blobs(m, w, h, seed):
    """m rectangles and ellipses with sides of 8 .. 26 pixels at random places: most pass stages 1 and 2, many overlap."""
    rng = np.random.RandomState(seed)
    P = blank(m, w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    for k in range(m):
        rows, cols = rng.randint(8, min(27, h)), rng.randint(8, 27)
        r0, c0 = rng.randint(0, h - rows + 1), rng.randint(0, w - cols + 1)
        if k % 2:
            rect(P[k], r0, c0, rows, cols)
        else:
            P[k] = (2 * (yy - r0) - rows + 1) ** 2 * cols ** 2 + (2 * (xx - c0) - cols + 1) ** 2 * rows ** 2 <= rows ** 2 * cols ** 2
    return P, None


PAIR_CASES = ((9, 65, 33, 1), (17, 65, 33, 2), (9, 130, 50, 3), (17, 130, 50, 4))


def square_grid(n, pitch=24, side=22, per_row=16):
    """n disjoint side x side squares, one proposal each, on a per_row x per_row grid: every one survives."""
    size = per_row * pitch
    P = blank(n, size, size)
    for k in range(n):
        rect(P[k], (k // per_row) * pitch + 1, (k % per_row) * pitch + 1, side, side)
    return P, None


def all_cases():
    """name -> (proposals, inside): everything the GPU must reproduce bit for bit."""
    cases = {
        "scene_bound_and": scene_bound_and(True),
        "scene_bound_none": scene_bound_and(False),
        "blob_gaps": blob_gaps(),
        "diagonal_touch": diagonal_touch(),
        "subpart_equality": subpart_equality(False),
        "subpart_one_more": subpart_equality(True),
        "subpart_equal_areas": subpart_equal_areas(),
        "subpart_chain": subpart_chain(),
        "survivors_overlap": survivors_overlap(),
        "small_area": small_area(),
        "thin_shapes": thin_shapes(),
        "ring_and_disc": ring_and_disc(),
        "boundary_tie": boundary_tie(),
        "rotated_under": rotated_rect(70, 45, 78),
        "rotated_over": rotated_rect(70, 45, 82),
        "rotated_over_two_words": rotated_rect(130, 50, 82),
    }
    for w, h in SIZES:
        cases[f"borders_{w}x{h}"] = touches_all_borders(w, h)
        cases[f"small_side_{w}x{h}"] = small_side_axis(w, h)
    for w, h, rows, cols in LARGE:
        cases[f"large_{w}x{h}"] = large_threshold(w, h, rows, cols)
    for m, w, h, seed in PAIR_CASES:
        cases[f"pairs_{m}_{w}x{h}"] = random_blobs(m, w, h, seed)
    return cases


# the smallest frames (w, h) at which a tile-staging or seam mistake of the shared labeller shows: exactly one 64 x 16 tile, one
# pixel into the next tile on both axes, one short of a tile, three tiles by three, and the degenerate frames
LABELLER_SIZES = ((64, 16), (65, 17), (63, 15), (129, 33), (1, 1), (1, 70), (70, 1))


def labeller_images(w, h):
    """name -> 0 / 1 image [h, w]: the component cases of tests/masks_cases.py and a random image at density 0.5"""
    from tests import masks_cases
    rng = np.random.default_rng(1000 * w + h)
    return {
        "serpentine": masks_cases.serpentine(h, w),
        "checkerboard": (masks_cases.checkerboard(h, w) == 1).astype(np.uint8),
        "arms": masks_cases.arms(h, w),
        "random": (rng.random((h, w)) < 0.5).astype(np.uint8),
    }
