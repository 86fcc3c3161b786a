"""DESIGN.md section 2d restated in numpy: scene-bound masks (back-projection, six planes and a height cut, closing by a
k x k rectangle), 8-connected components of equal label with first-pixel order keys, the integer-sum mean point, and the two
pruning rules.  Imports nothing from the product; slow on purpose (brute-force windows, flood fill)."""
from __future__ import annotations

import numpy as np


def depth_u16(depth_f16):
    """The reference's (depth * 1000).astype(np.uint16) with the product in float16."""
    d = np.asarray(depth_f16, np.float16)
    return (d * np.float16(1000)).astype(np.uint16)


def world_points(d16, T_WC, K, z_f32=True):
    """fp64 world point of every pixel [H,W,3]: z = float32(d16) / float32(1000) promoted (the scene-bound rule; z_f32=False:
    d16 / 1000 in fp64, what the integer-sum mean of a component averages), rows summed left to right."""
    d16 = np.asarray(d16, np.uint16)
    H, W = d16.shape
    K = np.asarray(K, np.float64)
    T = np.asarray(T_WC, np.float32).reshape(4, 4).astype(np.float64)
    z = (d16.astype(np.float32) / np.float32(1000)).astype(np.float64) if z_f32 else d16.astype(np.float64) / 1000.0
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x = (jj - K[0, 2]) * z / K[0, 0]
    y = (ii - K[1, 2]) * z / K[1, 1]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], -1)


def scene_bounds_raw(d16, T_WC, K, bounds):
    """uint8 0 / 255 before the closing.  bounds [[xmin,ymin,zmin],[xmax,ymax,zmax]]; zmin is replaced by -100."""
    b = np.array(bounds, np.float64).reshape(2, 3)
    b[0, 2] = -100.0
    p = world_points(d16, T_WC, K)
    out = (p[..., 0] < b[0, 0]) | (p[..., 0] > b[1, 0]) | (p[..., 1] < b[0, 1]) | (p[..., 1] > b[1, 1]) | (p[..., 2] < b[0, 2]) | (p[..., 2] > b[1, 2])
    m = (np.asarray(d16) > 0) & (p[..., 2] > -0.40) & out
    return np.where(m, 255, 0).astype(np.uint8)


def plane_margin(d16, T_WC, K, bounds):
    """Smallest distance of a valid pixel's coordinate from a plane it is tested against (seeds are chosen so that it is > 1e-9)."""
    b = np.array(bounds, np.float64).reshape(2, 3)
    b[0, 2] = -100.0
    p = world_points(d16, T_WC, K)[np.asarray(d16) > 0]
    if p.size == 0:
        return np.inf
    gaps = [np.abs(p[:, 2] + 0.40)] + [np.abs(p[:, a] - b[s, a]) for a in range(3) for s in range(2)]
    return float(min(g.min() for g in gaps))


def _window(src, k, use_max):
    """Brute force: dst(i,j) = max / min of src(i+a, j+b), a, b in [-k//2, -k//2 + k - 1], positions outside ignored."""
    H, W = src.shape
    lo = -(k // 2)
    dst = np.empty_like(src)
    for i in range(H):
        i0, i1 = max(0, i + lo), min(H, i + lo + k)
        for j in range(W):
            j0, j1 = max(0, j + lo), min(W, j + lo + k)
            win = src[i0:i1, j0:j1]
            dst[i, j] = win.max() if use_max else win.min()
    return dst


def _window_fast(src, k, use_max):
    """The same result through k shifted copies per axis (for the large frames of the GPU tests; checked against _window)."""
    H, W = src.shape
    lo = -(k // 2)
    ident = 0 if use_max else 255
    op = np.maximum if use_max else np.minimum
    pad = np.full((H, W + 2 * k), ident, src.dtype)
    pad[:, k:k + W] = src
    acc = np.full((H, W), ident, src.dtype)
    for b in range(lo, lo + k):
        acc = op(acc, pad[:, k + b:k + b + W])
    pad = np.full((H + 2 * k, W), ident, src.dtype)
    pad[k:k + H] = acc
    out = np.full((H, W), ident, src.dtype)
    for a in range(lo, lo + k):
        out = op(out, pad[k + a:k + a + H])
    return out


def dilate(src, k, fast=False):
    return (_window_fast if fast else _window)(np.asarray(src, np.uint8), k, True)


def erode(src, k, fast=False):
    return (_window_fast if fast else _window)(np.asarray(src, np.uint8), k, False)


def close(src, k, fast=False):
    return erode(dilate(src, k, fast), k, fast)


def scene_bound_mask(d16, T_WC, K, bounds, window=50, fast=True):
    return close(scene_bounds_raw(d16, T_WC, K, bounds), window, fast)


def components(mask):
    """-> uint32 [H,W]: each pixel's order key = raster index of the first pixel of its 8-connected component of equal label;
    0xffffffff where the label is 0.  Flood fill in raster order."""
    mask = np.asarray(mask, np.uint8)
    H, W = mask.shape
    keys = np.full((H, W), 0xffffffff, np.uint32)
    for i in range(H):
        for j in range(W):
            if mask[i, j] == 0 or keys[i, j] != 0xffffffff:
                continue
            l, key = mask[i, j], np.uint32(i * W + j)
            keys[i, j] = key
            stack = [(i, j)]
            while stack:
                a, b = stack.pop()
                for da in (-1, 0, 1):
                    for db in (-1, 0, 1):
                        u, v = a + da, b + db
                        if 0 <= u < H and 0 <= v < W and mask[u, v] == l and keys[u, v] == 0xffffffff:
                            keys[u, v] = key
                            stack.append((u, v))
    return keys


def components_fast(mask):
    """The same keys by iterated minimum propagation (vectorised; for the large frames of the GPU tests)."""
    mask = np.asarray(mask, np.uint8)
    H, W = mask.shape
    big = np.uint32(0xffffffff)
    keys = np.where(mask != 0, np.arange(H * W, dtype=np.uint32).reshape(H, W), big)
    padm = np.zeros((H + 2, W + 2), np.uint8)
    padm[1:-1, 1:-1] = mask
    while True:
        pad = np.full((H + 2, W + 2), big, np.uint32)
        pad[1:-1, 1:-1] = keys
        new = keys.copy()
        for da in (0, 1, 2):
            for db in (0, 1, 2):
                same = (padm[da:da + H, db:db + W] == mask) & (mask != 0)
                new = np.where(same, np.minimum(new, pad[da:da + H, db:db + W]), new)
        if (new == keys).all():
            return keys
        keys = new


def component_stats(keys, d16):
    """-> {key: (area, n, sum d, sum j d, sum i d)} as Python ints (exact)."""
    keys = np.asarray(keys)
    d = np.asarray(d16, np.uint16).astype(np.uint64)
    H, W = keys.shape
    jj, ii = np.meshgrid(np.arange(W, dtype=np.uint64), np.arange(H, dtype=np.uint64))
    out = {}
    for key in np.unique(keys[keys != 0xffffffff]):
        m = keys == key
        dv = d[m]
        out[int(key)] = (int(m.sum()), int((dv > 0).sum()), int(dv.sum()), int((jj[m] * dv).sum()), int((ii[m] * dv).sum()))
    return out


def mean_world_point(stat, T_WC, K):
    """The mean world point from the integer sums (None without a valid-depth pixel)."""
    _, n, sd, sjd, sid = stat
    if n == 0:
        return None
    K = np.asarray(K, np.float64)
    T = np.asarray(T_WC, np.float32).reshape(4, 4).astype(np.float64)
    n, sd, sjd, sid = np.float64(n), np.float64(sd), np.float64(sjd), np.float64(sid)
    den = np.float64(1000.0) * n
    z = sd / den
    x = (sjd - K[0, 2] * sd) / (den * K[0, 0])
    y = (sid - K[1, 2] * sd) / (den * K[1, 1])
    return np.array([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)])


def component_distance(stat, T_WC, K, centre):
    p = mean_world_point(stat, T_WC, K)
    if p is None:
        return None
    dlt = p - np.asarray(centre, np.float64)
    return float(np.sqrt((dlt[0] * dlt[0] + dlt[1] * dlt[1]) + dlt[2] * dlt[2]))


def _prune(mask, keys, choose):
    mask = np.asarray(mask, np.uint8)
    out = np.zeros_like(mask)
    for l in np.unique(mask):
        if l == 0:
            continue
        ks = [int(k) for k in np.unique(keys[mask == l])]         # ascending order key
        keep = ks[0] if len(ks) <= 1 else choose(ks)
        if keep is not None:
            out[keys == keep] = l
    return out


def duplicate_prune(mask, d16, T_WC, K, centre, min_area=200, fast=False):
    keys = (components_fast if fast else components)(mask)
    stats = component_stats(keys, d16)

    def choose(ks):
        best, best_d = None, 10000.0
        for k in ks:
            if stats[k][0] < min_area:
                continue
            dist = component_distance(stats[k], T_WC, K, centre)
            if dist is not None and dist < best_d:               # <: ties go to the lower order key
                best, best_d = k, dist
        return best
    return _prune(mask, keys, choose)


def disconnected_prune(mask, min_area=200, fast=False):
    keys = (components_fast if fast else components)(mask)
    stats = component_stats(keys, np.zeros(np.asarray(mask).shape, np.uint16))

    def choose(ks):
        best, best_a = None, 0
        for k in ks:
            if stats[k][0] < min_area:
                continue
            if stats[k][0] >= best_a:                            # >=: ties go to the higher order key
                best, best_a = k, stats[k][0]
        return best
    return _prune(mask, keys, choose)


def refine(mask, oob, pruned):
    return np.where(np.asarray(oob) == 255, 255, pruned).astype(np.uint8)
