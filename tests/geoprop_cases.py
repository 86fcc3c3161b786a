"""The frames of tests/test_geoprop_*.py: the scene of tests/labeltrack_cases.py (slab, box, two spheres at 320 x 240), windows cut
from it, and hand-made depth seen straight down from 0.5 m, where a pixel of depth d millimetres lies 500 - d millimetres above the
plane z = 0.  Every case is (depth uint16 [H,W], pose float32 [4,4], K4, bounds, parameters that differ from the defaults); the
restatement's answer is computed once per process and handed out read-only."""
from __future__ import annotations

import functools

import numpy as np

from tests import geoprop_ref as ref
from tests import labeltrack_cases as lc

DOWN = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0.5], [0, 0, 0, 1]], np.float32)
HAND_BOUNDS = np.array([[-0.3, -0.3, -0.05], [0.3, 0.3, 0.2]])
TABLE_MM = 500
# a plane without noise fills one bin, so all five windows that hold it tie and the lowest wins: b* = -2 (a property of the rule)
HAND_PLANE_BIN = -2


def _table(w, h):
    return np.full((h, w), TABLE_MM, np.uint16)


def _k4(w, h):
    return np.array([500.0, 500.0, (w - 1) / 2, (h - 1) / 2])


def _put(d, i0, i1, j0, j1, height_mm):
    """rows i0 .. i1 - 1, columns j0 .. j1 - 1 at height_mm above the table"""
    d[i0:i1, j0:j1] = TABLE_MM - height_mm


def tau():
    """three blocks side by side: the first two exactly tau_mm = 10 apart in depth (linked), the third tau_mm + 1 from the second"""
    d = _table(40, 20)
    _put(d, 2, 12, 2, 10, 30)
    _put(d, 2, 12, 10, 18, 40)
    _put(d, 2, 12, 18, 26, 51)
    return d, dict(min_area=4)


def h_min():
    """three blocks at b* + h_min_mm - 1, b* + h_min_mm and b* + h_min_mm + 1: the first is not above.  A window of one bin, so that
    the plane's window does not take the low blocks in: b* = 0, the table's own bin."""
    d = _table(40, 20)
    for k, height in enumerate((5, 6, 7)):
        _put(d, 4, 12, 2 + 12 * k, 10 + 12 * k, height)
    return d, dict(min_area=4, window_mm=1)


def serpentine():
    """a path one pixel wide over 200 x 70 pixels: every odd row from column 1 to 198, joined at alternate ends.  It crosses every
    seam of the 64 x 16 tiling many times and is one component."""
    d = _table(200, 70)
    rows = list(range(1, 69, 2))
    for k, i in enumerate(rows):
        _put(d, i, i + 1, 1, 199, 20)
        if k + 1 < len(rows):
            j = 198 if k % 2 == 0 else 1
            _put(d, i + 1, i + 2, j, j + 1, 20)
    return d, {}


def diagonal():
    """two 15 x 15 squares that touch at one corner, which lies on a corner of the tiling (row 16, column 64)"""
    d = _table(100, 40)
    _put(d, 1, 16, 49, 64, 20)
    _put(d, 16, 31, 64, 79, 20)
    return d, {}


def min_area():
    """a block of exactly min_area = 200 pixels and one of 199"""
    d = _table(80, 30)
    _put(d, 2, 12, 2, 22, 20)
    _put(d, 2, 12, 30, 50, 20)
    d[11, 49] = TABLE_MM
    return d, {}


def max_props():
    """five blocks of 20, 20, 20, 10 and 30 pixels in raster order, max_props 3: the largest and the first two of the tie stay"""
    d = _table(80, 12)
    for k in range(3):
        _put(d, 2, 6, 2 + 8 * k, 7 + 8 * k, 20)
    _put(d, 2, 4, 26, 31, 20)
    _put(d, 2, 8, 34, 39, 20)
    return d, dict(min_area=4, max_props=3)


def hist_tie():
    """half the frame on the table, half 20 mm higher, the same number of pixels each: the lower plane wins and the upper half is
    one component"""
    d = _table(40, 20)
    _put(d, 0, 20, 20, 40, 20)
    return d, dict(min_area=4)


HAND = dict(tau=tau, h_min=h_min, serpentine=serpentine, diagonal=diagonal, min_area=min_area, max_props=max_props, hist_tie=hist_tie)


def _scene_frame0():
    d16, _, poses = lc.frames(1)
    return d16[0], poses[0], lc.K4, lc.BOUNDS, {}


def _crop(rows, cols):
    d16, _, poses, k4 = lc.crop(1, rows, cols)
    return d16[0], poses[0], k4, lc.BOUNDS, dict(min_area=20)


def _zero_depth():
    d16, _, poses = lc.frames(1)
    return np.zeros_like(d16[0]), poses[0], lc.K4, lc.BOUNDS, {}


def _looks_away():
    d16, _, poses = lc.frames(1)
    pose = poses[0].copy()
    pose[:3, 1:3] *= -1                             # turned by 180 degrees about its own x axis: the scene is behind the camera
    return d16[0], pose, lc.K4, lc.BOUNDS, {}


def _hand(name):
    d, params = HAND[name]()
    h, w = d.shape
    return d, DOWN, _k4(w, h), HAND_BOUNDS, params


CASES = {"scene frame 0": _scene_frame0, "crop 65 x 17": lambda: _crop(17, 65), "crop 129 x 70": lambda: _crop(70, 129),
         "1 x 1": lambda: (np.array([[TABLE_MM]], np.uint16), DOWN, _k4(1, 1), HAND_BOUNDS, {}),
         "zero depth": _zero_depth, "looks away": _looks_away, **{name: functools.partial(_hand, name) for name in HAND}}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (d16, pose, K4, bounds, params), read-only"""
    d16, pose, k4, bounds, params = CASES[name]()
    arrays = [np.array(a) for a in (d16, pose, k4, bounds)]           # copies: the scene's own arrays stay as they are
    for a in arrays:
        a.setflags(write=False)
    return (*arrays, params)


@functools.lru_cache(maxsize=None)
def reference(name, wrong=None):
    """The restatement on a case -> (labels, records, M, plane record), read-only."""
    d16, pose, k4, bounds, params = case(name)
    labels, recs, m, plane = ref.propose(d16, pose, k4, bounds, wrong=wrong, **params)
    for a in (labels, recs, plane):
        a.setflags(write=False)
    return labels, recs, m, plane


def best_iou(labels, m, truth):
    """-> the best IoU of a proposal with the true mask"""
    return max([float(((labels == k) & truth).sum() / ((labels == k) | truth).sum()) for k in range(1, m + 1)] or [0.0])
