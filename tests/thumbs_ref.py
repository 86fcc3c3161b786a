"""The object-thumbnail rule of DESIGN.md section 2g in numpy: the oracle d2r_thumbs_plan / d2r_thumbs_fill / d2r_thumbs_blur_bits
are held to byte for byte.  Restates the image work of reference caption.py:62-130 with cv2's pieces (connectedComponents,
GaussianBlur, dilate) replaced by the written rule.  Test infrastructure: nothing in the product imports it."""
import numpy as np

MIN_AREA, HOLE_AREA, PAD, DILATE_K = 200, 400, 5, 60
ACCEPTED, CONTAINER, ROTATED, EDGE, SMALL = 1, 2, 4, 8, 16

# q[t] for t = 0 .. 100 (q[-t] = q[t]): floor(2^15 g[t] / sum(g) + 1/2), g[t] = exp(-t^2 / (2 * 30.5^2)); literal data, derived again
# by tests/test_thumbs_host.py.  Their sum over t = -100 .. 100 is 32767.
TAPS = (429, 429, 428, 427, 425, 423, 421, 418, 415, 411, 407, 402, 397, 392, 386, 380, 374, 367, 360, 353, 346, 338, 331, 323, 315,
        307, 298, 290, 282, 273, 264, 256, 247, 239, 230, 222, 214, 206, 197, 189, 182, 174, 166, 159, 152, 144, 138, 131, 124, 118,
        112, 106, 100, 95, 89, 84, 80, 75, 70, 66, 62, 58, 54, 51, 47, 44, 41, 38, 36, 33, 31, 29, 26, 24, 23, 21, 19, 18, 16, 15, 14,
        13, 12, 11, 10, 9, 8, 7, 7, 6, 6, 5, 5, 4, 4, 3, 3, 3, 2, 2, 2)
RADIUS = 100
BLUR_THRESHOLD = 1 << 29


def derive_taps():
    t = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    g = np.exp(-(t * t) / (2.0 * 30.5 * 30.5))
    return np.floor(32768.0 * g / g.sum() + 0.5).astype(np.int64)


def full_taps():
    h = np.asarray(TAPS, np.int64)
    return np.concatenate([h[:0:-1], h])


def rot90ccw(a):
    """R(A)[i][j] = A[j][W - 1 - i]"""
    return np.ascontiguousarray(np.swapaxes(a, 0, 1)[::-1])


def reflect101(p, n):
    """index p of any distance outside [0, n) -> the index reflect-101 applied repeatedly reads"""
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    m = np.mod(p, period)
    return np.where(m >= n, period - m, m)


def _blur_axis(a, axis):
    n = a.shape[axis]
    q = full_taps()
    out = np.zeros(a.shape, np.int64)
    base = np.arange(n)
    for k, t in enumerate(range(-RADIUS, RADIUS + 1)):
        out += q[k] * np.take(a, reflect101(base + t, n), axis=axis)
    return out


def blur_values(b):
    """0 / 1 image -> the exact integer sums v (rows first, then columns)"""
    return _blur_axis(_blur_axis((np.asarray(b) != 0).astype(np.int64), 1), 0)


def blur_bit(b):
    return blur_values(b) >= BLUR_THRESHOLD


def dilate(b, k):
    """dst(i, j) = OR src(i + a, j + c), a, c in [-k/2, -k/2 + k - 1], outside ignored (section 2d's convention)"""
    b = np.asarray(b, bool)
    H, W = b.shape
    lo = -(k // 2)
    out = np.zeros_like(b)
    rows = np.zeros_like(b)
    for c in range(lo, lo + k):          # rows(i, j) = OR b(i, j + c)
        if 0 <= c < W:
            rows[:, :W - c] |= b[:, c:]
        elif 0 < -c < W:
            rows[:, -c:] |= b[:, :W + c]
    for a in range(lo, lo + k):
        if 0 <= a < H:
            out[:H - a] |= rows[a:]
        elif 0 < -a < H:
            out[-a:] |= rows[:H + a]
    return out


def blur_bits(b, k):
    """the parity hook: blur bit dilated by k x k, as 0 / 1 uint8"""
    return dilate(blur_bit(b), k).astype(np.uint8)


def components8(b):
    """8-connected components of the set pixels of b -> list of boolean masks"""
    from scipy import ndimage
    lab, n = ndimage.label(np.asarray(b, bool), structure=np.ones((3, 3), bool))
    return [lab == k for k in range(1, n + 1)]


def touches_edge(m):
    return bool(m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any())


def is_container(obj, label, hole_area=HOLE_AREA):
    """some 8-connected component of ~obj with area >= hole_area, 10 |comp & label == 0| <= 7 area, no pixel on the border"""
    for comp in components8(~obj):
        a = int(comp.sum())
        i = int((comp & (label == 0)).sum())
        if a >= hole_area and 10 * i <= 7 * a and not touches_edge(comp):
            return True
    return False


def plan_and_thumbs(num_objs, rgbs, masks, oob, noise, topdown, multi_view=True, single_view_idx=0, min_area=MIN_AREA,
                    hole_area=HOLE_AREA, pad=PAD, dilate_k=DILATE_K):
    """-> (records, thumbs): records a list of dict(obj, frame, flags, area, row0, col0, rows, cols) per (object, visited frame);
    thumbs a list per object 1 .. num_objs - 1 of uint8 [rows, cols, 3] arrays, the accepted records' in order."""
    rgbs, masks, oob = np.asarray(rgbs, np.uint8), np.asarray(masks, np.uint8), np.asarray(oob, np.uint8)
    N = rgbs.shape[0]
    recs, thumbs = [], []
    for o in range(1, num_objs):
        mine, container = [], False
        for f in (range(N) if multi_view else [single_view_idx]):
            rot = (f in (0, 1) and not topdown) or (not multi_view and single_view_idx > 0)
            rgb, lab, out = rgbs[f], masks[f], oob[f]
            if rot:
                rgb, lab, out = rot90ccw(rgb), rot90ccw(lab), rot90ccw(out)
            obj = (lab == o) & (out == 0)
            area = int(obj.sum())
            rec = dict(obj=o, frame=f, flags=ROTATED if rot else 0, area=area, row0=0, col0=0, rows=0, cols=0)
            recs.append(rec)
            edge = area > 0 and touches_edge(obj)
            if edge:
                rec["flags"] |= EDGE
            if area < min_area or area == 0:         # an empty object has no bounding box whatever min_area says
                rec["flags"] |= SMALL
                continue
            if edge and len(mine) >= 3 and not topdown:
                continue
            if f == 0:
                container = is_container(obj, lab, hole_area)
            H, W = obj.shape
            if container:
                frame_noise = rot90ccw(noise) if (f in (0, 1) and not topdown) else np.asarray(noise, np.uint8)
                img = rgb.copy()
                fill = dilate(blur_bit(~obj), dilate_k)
                img[fill] = frame_noise[fill]
                r0, r1, c0, c1 = 0, H, 0, W
                rec["flags"] |= CONTAINER
            else:
                img = rgb.copy()
                img[~obj] = 255
                ii, jj = np.nonzero(obj)
                r0, r1 = max(int(ii.min()) - pad, 0), min(int(ii.max()) + pad + 1, H)
                c0, c1 = max(int(jj.min()) - pad, 0), min(int(jj.max()) + pad + 1, W)
            rec["flags"] |= ACCEPTED
            rec.update(row0=r0, col0=c0, rows=r1 - r0, cols=c1 - c0)
            mine.append(np.ascontiguousarray(img[r0:r1, c0:c1]))
        thumbs.append(mine)
    return recs, thumbs
