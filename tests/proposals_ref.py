"""DESIGN.md section 2h in numpy and Python ints: mask proposals -> the first frame's label image, the per-proposal records and the
pair-intersection matrix.  Integer arithmetic only.  The GPU tests hold d2r_proposals_labels to this bit for bit; the host tests pin
this file against hand-computed answers."""
from __future__ import annotations

import numpy as np

from tests import masks_ref

REC_WORDS = 8            # area, ncomp, stage, label, boundary, ew, eh, dd
NONE = 0xffffffff


class TooManySurvivors(ValueError):
    pass


def boundary(mask):
    """Set pixels with an unset 4-neighbour; positions outside the image read as unset, so a set pixel on the border is one."""
    m = np.asarray(mask, bool)
    p = np.zeros((m.shape[0] + 2, m.shape[1] + 2), bool)
    p[1:-1, 1:-1] = m
    return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def chosen_component(mask):
    """-> (bool [H,W] of the component with the most boundary pixels, ties to the lowest raster index of its first pixel; that
    count).  An empty mask: (all False, 0)."""
    m = np.asarray(mask, bool)
    if not m.any():
        return np.zeros_like(m), 0
    keys = masks_ref.components_fast(m.astype(np.uint8))
    edge = boundary(m)
    best_key, best_n = None, -1
    for key in np.unique(keys[m]):                      # ascending: a tie keeps the earlier component
        n = int((edge & (keys == key)).sum())
        if n > best_n:
            best_key, best_n = key, n
    return keys == best_key, best_n


def cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(comp):
    """Strictly convex hull of the pixel centres (x = column, y = row) of a bool image, counter-clockwise in (x, y), starting at the
    vertex with the lowest (y, x): Andrew's monotone chain over the points in (y, x) order.  -> list of (x, y) Python ints."""
    ys, xs = np.nonzero(comp)
    pts = sorted({(int(y), int(x)) for y, x in zip(ys, xs)})
    pts = [(x, y) for y, x in pts]
    if len(pts) == 1:
        return pts

    def chain(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and cross(h[-2], h[-1], p) <= 0:
                h.pop()
            h.append(p)
        return h

    return chain(pts)[:-1] + chain(pts[::-1])[:-1]


def min_rect(vertices):
    """-> (ew, eh, dd) of the hull edge whose rectangle ew eh / dd is smallest, compared exactly, ties to the first edge;
    (0, 0, 0) for fewer than three vertices."""
    n = len(vertices)
    if n < 3:
        return 0, 0, 0
    best = None
    for k in range(n):
        a, b = vertices[k], vertices[(k + 1) % n]
        dx, dy = b[0] - a[0], b[1] - a[1]
        dp = [dx * p[0] + dy * p[1] for p in vertices]
        nq = [-dy * p[0] + dx * p[1] for p in vertices]
        ew, eh, dd = max(dp) - min(dp), max(nq) - min(nq), dx * dx + dy * dy
        if best is None or ew * eh * best[2] < best[0] * best[1] * dd:
            best = (ew, eh, dd)
    return best


def side_test(ew, eh, dd):
    return min(ew, eh) ** 2 > 400 * dd


def proposals_to_labels(proposals, inside=None):
    """proposals bool [M,H,W], inside bool [H,W] or None -> (labels uint8 [H,W], records uint32 [M,8], inter uint32 [M,M]).
    Raises TooManySurvivors past 255."""
    P = np.asarray(proposals).astype(bool)
    M, H, W = P.shape
    if inside is not None:
        P = P & np.asarray(inside).astype(bool)[None]
    recs = np.zeros((M, REC_WORDS), np.uint32)
    inter = np.zeros((M, M), np.uint32)
    area = [int(p.sum()) for p in P]
    stage = [0] * M
    for m in range(M):
        dil = masks_ref.dilate(P[m].astype(np.uint8), 5, fast=True)
        keys = masks_ref.components_fast(dil)
        ncomp = len(np.unique(keys[dil != 0]))
        comp, nb = chosen_component(P[m])
        ew, eh, dd = min_rect(hull(comp)) if nb else (0, 0, 0)
        recs[m, 0], recs[m, 1], recs[m, 4:8] = area[m], ncomp, (nb, ew, eh, dd)
        if ncomp != 1:
            stage[m] = 1
        elif 10 * area[m] > 3 * H * W:
            stage[m] = 2
    surv = [m for m in range(M) if stage[m] == 0]
    marked = set()
    for a, i in enumerate(surv):
        for j in surv[a + 1:]:
            it = int((P[i] & P[j]).sum())
            inter[i, j] = it
            if 10 * it > area[i] or 10 * it > area[j]:
                marked.add(i if area[i] < area[j] else j)
    label = 0
    labels = np.zeros((H, W), np.uint8)
    for m in range(M):
        if stage[m] == 0 and m in marked:
            stage[m] = 3
        if stage[m] == 0 and (area[m] < 80 or not side_test(int(recs[m, 5]), int(recs[m, 6]), int(recs[m, 7]))):
            stage[m] = 4
        recs[m, 2] = stage[m]
        if stage[m] == 0:
            label += 1
            recs[m, 3] = label
    if label > 255:
        raise TooManySurvivors(f"{label} proposals survive")
    for m in range(M):
        if recs[m, 3]:
            labels[P[m]] = recs[m, 3]                   # ascending: the highest label wins
    return labels, recs, inter
