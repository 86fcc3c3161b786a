"""Inputs shared by tests/test_thumbs_host.py and tests/test_thumbs_gpu.py: 0 / 1 images for the blur and small scans for the
thumbnail rule.  Everything is generated from fixed seeds; the references are computed once per process."""
import functools

import numpy as np

from tests import thumbs_ref as R

BLUR_SIZES = ((150, 200), (70, 130), (30, 40), (300, 1), (1, 300))      # (h, w): 200x150, 130x70, 40x30, 1x300 and 300x1 as w x h
BLUR_KS = (1, 2, 59, 60, 64)


def ring(h, w, r_in=0.25, r_out=0.45):
    """a ring of radii r_in, r_out times the shorter side, centred"""
    i, j = np.mgrid[0:h, 0:w]
    d = np.hypot(i - (h - 1) / 2.0, j - (w - 1) / 2.0)
    s = min(h, w)
    return ((d >= r_in * s) & (d <= r_out * s)).astype(np.uint8)


def half_plane(h, w):
    """set left of a slanted line through the frame's middle"""
    i, j = np.mgrid[0:h, 0:w]
    return (j + 0.3 * i < 0.5 * w + 0.15 * h).astype(np.uint8)


def blobs(h, w, seed):
    """a few random discs: large structures, so that the 0.5 contour of the blur crosses the frame"""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:h, 0:w]
    out = np.zeros((h, w), bool)
    for _ in range(4):
        ci, cj, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.15, 0.3) * max(h, w)
        out |= np.hypot(i - ci, j - cj) <= r
    return out.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def blur_image(kind, h, w):
    """"ring": the complement of a ring, what a ring-shaped container hands the blur; "half": a half-plane; "blobs": random discs"""
    return {"ring": lambda: 1 - ring(h, w), "half": lambda: half_plane(h, w), "blobs": lambda: blobs(h, w, 7 + h + w)}[kind]()


@functools.lru_cache(maxsize=None)
def blur_bit_ref(kind, h, w):
    return R.blur_bit(blur_image(kind, h, w))


def _disc(h, w, ci, cj, r):
    i, j = np.mgrid[0:h, 0:w]
    return np.hypot(i - ci, j - cj) <= r


@functools.lru_cache(maxsize=None)
def scan5():
    """5 frames of 200 x 150 with labels 0 .. 3 (min_area 20, hole_area 40): label 1 a ring whose hole holds label 2 (a container);
    label 2 absent from frame 4 and cut below min_area by out-of-scene pixels in frame 3; label 3 touches the border in all five."""
    H, W, N = 150, 200, 5
    rng = np.random.default_rng(11)
    rgbs = rng.integers(0, 255, (N, H, W, 3), dtype=np.uint8)         # 0 .. 254: a white pixel can only be the fill
    masks = np.zeros((N, H, W), np.uint8)
    oob = np.zeros((N, H, W), np.uint8)
    for f in range(N):
        ci, cj = 70 + 3 * f, 90 + 5 * f
        masks[f][_disc(H, W, ci, cj, 40)] = 1
        masks[f][_disc(H, W, ci, cj, 22)] = 0
        if f != 4:
            masks[f][_disc(H, W, ci + 2, cj - 3, 14)] = 2
        masks[f][130:150, 150 + 4 * f:200] = 3
        oob[f][0:6, :] = 255
    oob[3][_disc(H, W, 70 + 9 + 2, 90 + 15 - 3, 13.9)] = 255            # frame 3: label 2 keeps a thin rim
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return dict(num_objs=4, rgbs=rgbs, masks=masks, oob=oob, noise=noise, min_area=20, hole_area=40, pad=5, dilate_k=60)


@functools.lru_cache(maxsize=None)
def big_container():
    """one 1280 x 720 frame: label 1 a frame-filling ring, label 2 inside its hole; the reference's constants"""
    H, W = 720, 1280
    rng = np.random.default_rng(12)
    rgbs = rng.integers(0, 255, (1, H, W, 3), dtype=np.uint8)
    masks = np.zeros((1, H, W), np.uint8)
    i, j = np.mgrid[0:H, 0:W]
    e = ((i - 360) / 340.0) ** 2 + ((j - 640) / 620.0) ** 2
    masks[0][e <= 1.0] = 1
    masks[0][e <= 0.22] = 0
    masks[0][_disc(H, W, 350, 600, 120)] = 2
    oob = np.zeros((1, H, W), np.uint8)
    oob[0][:, :8] = 255
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return dict(num_objs=3, rgbs=rgbs, masks=masks, oob=oob, noise=noise, min_area=200, hole_area=400, pad=5, dilate_k=60)


@functools.lru_cache(maxsize=None)
def many_objects():
    """two frames of 130 x 70 with labels 0 .. 254: 254 objects of 5 x 6 = 30 pixels on a grid of 26 x 10 cells (min_area 20)"""
    H, W = 70, 130
    rng = np.random.default_rng(13)
    rgbs = rng.integers(0, 255, (2, H, W, 3), dtype=np.uint8)
    masks = np.zeros((2, H, W), np.uint8)
    for o in range(1, 255):
        r, c = divmod(o - 1, 26)
        masks[0][7 * r:7 * r + 6, 5 * c:5 * c + 5] = o
        masks[1][7 * r + 1:7 * r + 7, 5 * c:5 * c + 5] = o
    oob = np.zeros((2, H, W), np.uint8)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return dict(num_objs=255, rgbs=rgbs, masks=masks, oob=oob, noise=noise, min_area=20, hole_area=40, pad=5, dilate_k=60)


@functools.lru_cache(maxsize=None)
def reference(name, topdown, multi_view, single_view_idx):
    """(records, thumbs) of tests/thumbs_ref.py for a scan above"""
    s = {"scan5": scan5, "big": big_container, "many": many_objects}[name]()
    return R.plan_and_thumbs(s["num_objs"], s["rgbs"], s["masks"], s["oob"], s["noise"], topdown, multi_view, single_view_idx,
                             s["min_area"], s["hole_area"], s["pad"], s["dilate_k"])


def records_array(recs):
    """the reference's records as the rows d2r_thumbs_plan returns, without the offset words"""
    return np.array([[r["obj"], r["frame"], r["flags"], r["area"], r["row0"], r["col0"], r["rows"], r["cols"]] for r in recs],
                    np.uint32).reshape(-1, 8)
