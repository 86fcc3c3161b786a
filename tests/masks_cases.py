"""Inputs shared by tests/test_masks_host.py and tests/test_masks_gpu.py: the pruning cases that pin the reference's quirks,
label images that stress the labelling, and a seeded RGB-D frame for the scene-bound masks."""
from __future__ import annotations

import numpy as np

W, H = 120, 100
K = np.array([[150.0, 0.0, 59.5], [0.0, 150.0, 49.5], [0.0, 0.0, 1.0]])
EYE = np.eye(4, dtype=np.float32)
CENTRE = np.array([0.0, 0.0, 1.0])


def _rect(mask, i0, j0, h, w, label):
    mask[i0:i0 + h, j0:j0 + w] = label


def prune_cases():
    """-> {name: dict(mask, d16, T, K, centre, dup, dis)}; dup / dis: the labels expected at probe pixels {(i, j): label} after
    duplicate_prune / disconnected_prune, written out by hand."""
    cases = {}
    d_flat = np.full((H, W), 1000, np.uint16)

    m = np.zeros((H, W), np.uint8)                       # a single component of area 12 < 200 is kept
    _rect(m, 10, 10, 3, 4, 7)
    cases["single_small_kept"] = dict(mask=m, d16=d_flat, dup={(10, 10): 7}, dis={(10, 10): 7})

    m = np.zeros((H, W), np.uint8)                       # two components, both under 200: the label disappears
    _rect(m, 10, 10, 10, 10, 3)
    _rect(m, 60, 60, 13, 15, 3)
    cases["two_small_dropped"] = dict(mask=m, d16=d_flat, dup={(10, 10): 0, (60, 60): 0}, dis={(10, 10): 0, (60, 60): 0})

    m = np.zeros((H, W), np.uint8)                       # area 199 (nearer the centre) against area 200: only 200 is a candidate
    _rect(m, 45, 50, 10, 20, 5)
    m[45, 50] = 0
    _rect(m, 5, 5, 10, 20, 5)
    cases["199_vs_200"] = dict(mask=m, d16=d_flat, dup={(50, 60): 0, (5, 5): 5}, dis={(50, 60): 0, (5, 5): 5})

    m = np.zeros((H, W), np.uint8)                       # the nearer, larger candidate has no valid depth: duplicate keeps the other
    _rect(m, 40, 45, 20, 30, 9)
    _rect(m, 2, 2, 15, 15, 9)
    d = d_flat.copy()
    d[40:60, 45:75] = 0
    cases["no_valid_depth"] = dict(mask=m, d16=d, dup={(40, 45): 0, (2, 2): 9}, dis={(40, 45): 9, (2, 2): 0})

    m = np.zeros((H, W), np.uint8)                       # mirror images about the principal point: an exact tie in distance and area
    _rect(m, 40, 10, 20, 15, 2)
    _rect(m, 40, 95, 20, 15, 2)
    cases["tie"] = dict(mask=m, d16=d_flat, dup={(40, 10): 2, (40, 95): 0}, dis={(40, 10): 0, (40, 95): 2})

    m = np.zeros((H, W), np.uint8)                       # nearest wins over largest; a second label is untouched; oob overwrites
    _rect(m, 42, 52, 15, 15, 4)                          # 225 px at the centre
    _rect(m, 0, 0, 30, 30, 4)                            # 900 px in the corner
    _rect(m, 70, 70, 5, 5, 200)
    cases["near_vs_large"] = dict(mask=m, d16=d_flat, dup={(42, 52): 4, (0, 0): 0, (70, 70): 200}, dis={(42, 52): 0, (0, 0): 4, (70, 70): 200})
    for c in cases.values():
        c.update(T=EYE, K=K, centre=CENTRE)
    return cases


def serpentine(h=61, w=97):
    """One label winding through the whole frame: horizontal runs every second row joined alternately at the right and the left."""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    for k, i in enumerate(range(1, h, 2)):
        m[i, w - 1 if k % 2 == 0 else 0] = 1
    return m


def checkerboard(h=33, w=70):
    ii, jj = np.indices((h, w))
    return np.where((ii + jj) % 2 == 0, 1, 2).astype(np.uint8)


def arms(h=50, w=130):
    """Two arms of one label that meet only in the last row and the last column."""
    m = np.zeros((h, w), np.uint8)
    left = min(3, w - 1)
    m[:, left] = 1           # the left arm (column 3; the last column of a frame narrower than that)
    m[:, w - 1] = 1          # the right arm: the last column
    m[h - 1, left:] = 1      # the last row joins them
    return m


def many_labels(h=65, w=200, n=254):
    """Labels 1 .. n in 4 x 4 blocks on a 5-pixel pitch, dealt out in raster order: 13 x 40 = 520 blocks, so every label has two
    components and labels 1 .. 12 have three, spread over several labelling tiles."""
    m = np.zeros((h, w), np.uint8)
    k = 0
    for i in range(0, h - 3, 5):
        for j in range(0, w - 3, 5):
            m[i:i + 4, j:j + 4] = 1 + k % n
            k += 1
    assert k >= 2 * n
    return m


def depth_for(shape, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(300, 3000, shape).astype(np.uint16)
    d[rng.random(shape) < 0.1] = 0
    return d


def look_at(eye, target):
    z = np.asarray(target, np.float64) - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T.astype(np.float32)


SCENE_BOUNDS = np.array([[-0.25, -0.30, -0.10], [0.55, 0.45, 0.35]])
SCENE_POSE = look_at(np.array([-0.4, -0.5, 0.9]), np.array([0.25, 0.15, -0.2]))      # oblique: no axis of the camera along a world axis


def scene_frame(w, h, seed):
    """Seeded depth in millimetres: 8 x 8 blocks of a common range (surfaces) plus per-pixel noise and zeros, spread so that world
    points fall on both sides of every bound plane and of the z = -0.40 cut.  -> (d16, K)."""
    rng = np.random.default_rng(seed)
    bh, bw = (h + 7) // 8, (w + 7) // 8
    base = rng.integers(250, 2600, (bh, bw))
    d = np.kron(base, np.ones((8, 8), np.int64))[:h, :w] + rng.integers(-40, 41, (h, w))
    d = d.astype(np.uint16)
    d[rng.random((h, w)) < 0.08] = 0
    f = 0.9 * w
    Kf = np.array([[f, 0.0, (w - 1) / 2], [0.0, f, (h - 1) / 2], [0.0, 0.0, 1.0]])
    return d, Kf
