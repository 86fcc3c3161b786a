"""DESIGN.md section 2l restated in numpy: mask proposals from frame 0's depth and the support plane.  fp64 one operation at a time in
the written order, a plain union-find over the links.  csrc/geoprop.hip and csrc/geoprop_plane.h are held to this by equality of
every byte of the label image, the records and the plane record.

`wrong=` swaps one clause of the rule for a near miss (tests/test_geoprop_host.py shows that each one changes the output on the
cases of tests/geoprop_cases.py); the rule itself is wrong=None."""
from __future__ import annotations

import numpy as np

NONE = 0xffffffff
REC_WORDS = 6                     # root, area, i0, j0, i1, j1
MAX_BINS = 1 << 16
DEFAULTS = dict(window_mm=5, h_min_mm=6, tau_mm=10, min_area=200, max_props=255)
WRONG = ("conn8", "tau_lt", "hmin_gt", "tie_high", "min_area_gt", "number_by_area", "tie_larger_root", "no_bounds")


def bins(bounds, up=(0.0, 0.0, 1.0)):
    """-> (lo, n): the height bins of the bounds, a millimetre each, widened by one bin on either side."""
    b = np.asarray(bounds, np.float64).reshape(2, 3)
    u = np.asarray(up, np.float64)
    p, q = u * b[0], u * b[1]
    m, M = np.minimum(p, q), np.maximum(p, q)
    lo = np.floor(1000.0 * ((m[0] + m[1]) + m[2]) + 0.5) - 1.0
    hi = np.floor(1000.0 * ((M[0] + M[1]) + M[2]) + 0.5) + 1.0
    assert hi - lo + 1 <= MAX_BINS
    return int(lo), int(hi - lo + 1)


def heights(d16, pose, K4, bounds, up=(0.0, 0.0, 1.0), wrong=None):
    """-> uint32 [H,W]: the pixel's height bin less the first bin of the bounds, NONE without depth or outside the bounds."""
    d16 = np.asarray(d16, np.uint16)
    H, W = d16.shape
    fx, fy, cx, cy = (np.float64(k) for k in K4)
    T = np.asarray(pose, np.float32).reshape(4, 4).astype(np.float64)
    b = np.asarray(bounds, np.float64).reshape(2, 3)
    u = np.asarray(up, np.float64)
    lo, n = bins(bounds, up)
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    z = (d16.astype(np.float32) / np.float32(1000.0)).astype(np.float64)
    x, y = (jj - cx) * z / fx, (ii - cy) * z / fy
    p = [((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)]
    inside = d16 > 0
    if wrong != "no_bounds":
        for a in range(3):
            inside &= (p[a] >= b[0, a]) & (p[a] <= b[1, a])
    hb = np.floor(1000.0 * ((u[0] * p[0] + u[1] * p[1]) + u[2] * p[2]) + 0.5) - np.float64(lo)
    idx = np.minimum(np.maximum(hb, 0.0), np.float64(n - 1)).astype(np.uint32)
    return np.where(inside, idx, np.uint32(NONE)).astype(np.uint32)


def plane(hist, lo, window_mm=5, wrong=None):
    """-> (b*, pixels in its window, inside pixels): the centre of the fullest window of window_mm bins, ties to the lowest bin;
    (0, 0, 0) when the histogram is empty."""
    hist = np.asarray(hist, np.int64)
    if hist.sum() == 0:
        return 0, 0, 0
    half = window_mm // 2
    pad = np.concatenate([np.zeros(half, np.int64), hist, np.zeros(half, np.int64)])
    sums = np.array([pad[b:b + window_mm].sum() for b in range(len(hist))])
    best = int(sums.max())
    at = np.nonzero(sums == best)[0]
    return lo + int(at[-1] if wrong == "tie_high" else at[0]), best, int(hist.sum())


def components(above, right, down, diagonal=False):
    """-> int64 [H,W]: the raster index of the first pixel of each above pixel's component of the link graph, -1 elsewhere."""
    H, W = above.shape
    parent = list(range(H * W))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for i, j in zip(*np.nonzero(right)):
        unite(i * W + j, i * W + j + 1)
    for i, j in zip(*np.nonzero(down)):
        unite(i * W + j, (i + 1) * W + j)
    if diagonal:
        for i, j in zip(*np.nonzero(above[:-1, :-1] & above[1:, 1:])):
            unite(i * W + j, (i + 1) * W + j + 1)
        for i, j in zip(*np.nonzero(above[:-1, 1:] & above[1:, :-1])):
            unite(i * W + j + 1, (i + 1) * W + j)
    roots = np.full((H, W), -1, np.int64)
    for i, j in zip(*np.nonzero(above)):
        roots[i, j] = find(i * W + j)
    return roots


def propose(d16, pose, K4, bounds, up=(0.0, 0.0, 1.0), window_mm=5, h_min_mm=6, tau_mm=10, min_area=200, max_props=255, wrong=None):
    """-> (labels uint16 [H,W], records uint32 [max_props,6], M, plane record int32 [5]: b*, pixels in its window, inside pixels,
    above pixels, components before the selection)."""
    assert wrong is None or wrong in WRONG
    d16 = np.asarray(d16, np.uint16)
    H, W = d16.shape
    lo, n = bins(bounds, up)
    idx = heights(d16, pose, K4, bounds, up, wrong)
    has = idx != NONE
    hist = np.bincount(idx[has].astype(np.int64), minlength=n)
    b_star, count, n_inside = plane(hist, lo, window_mm, wrong)
    if n_inside == 0:
        above = np.zeros((H, W), bool)
    else:
        thr = b_star + h_min_mm - lo
        above = has & ((idx.astype(np.int64) > thr) if wrong == "hmin_gt" else (idx.astype(np.int64) >= thr))
    d = d16.astype(np.int64)
    near = (lambda a, b: np.abs(a - b) < tau_mm) if wrong == "tau_lt" else (lambda a, b: np.abs(a - b) <= tau_mm)
    right, down = np.zeros((H, W), bool), np.zeros((H, W), bool)
    right[:, :-1] = above[:, :-1] & above[:, 1:] & near(d[:, :-1], d[:, 1:])
    down[:-1, :] = above[:-1, :] & above[1:, :] & near(d[:-1, :], d[1:, :])
    roots = components(above, right, down, diagonal=wrong == "conn8")
    recs = []
    for root in np.unique(roots[roots >= 0]):
        ii, jj = np.nonzero(roots == root)
        recs.append((int(root), len(ii), int(ii.min()), int(jj.min()), int(ii.max()), int(jj.max())))
    n_comp = len(recs)
    recs = [r for r in recs if (r[1] > min_area if wrong == "min_area_gt" else r[1] >= min_area)]
    if len(recs) > max_props:
        recs = sorted(recs, key=lambda r: (-r[1], -r[0] if wrong == "tie_larger_root" else r[0]))[:max_props]
    recs = sorted(recs, key=(lambda r: (-r[1], r[0])) if wrong == "number_by_area" else (lambda r: r[0]))
    labels = np.zeros((H, W), np.uint16)
    out = np.zeros((max_props, REC_WORDS), np.uint32)
    for k, r in enumerate(recs):
        labels[roots == r[0]] = k + 1
        out[k] = r
    return labels, out, len(recs), np.array([b_star, count, n_inside, int(above.sum()), n_comp], np.int32)


def masks(labels, m):
    """-> bool [m,H,W]: proposal k + 1's pixels"""
    return labels[None] == np.arange(1, m + 1, dtype=labels.dtype)[:, None, None]
