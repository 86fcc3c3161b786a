"""The rule of DESIGN.md section 2m in numpy: HF CLIPImageProcessor on one thumbnail (Pillow's antialiased bicubic in 22-bit fixed
point, horizontal pass first, centre crop, normalisation), the class embeddings, the fp32 cosine in its written order, the sum over
an object's thumbnails and the k best names.  dream2real_amd/csrc/captions.hip implements the same rule on the GPU."""
import math

import numpy as np

PRECISION_BITS = 22
MEAN = np.array([0.48145466, 0.4578275, 0.40821073], np.float32)
STD = np.array([0.26862954, 0.26130258, 0.27577711], np.float32)


def resized_size(h, w, S):
    """(nh, nw): the shortest side to S, the longer to int(S * long / short)"""
    short, long_ = min(h, w), max(h, w)
    new_long = int(S * long_ / short)
    return (new_long, S) if w <= h else (S, new_long)


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size, first=0, count=None):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the output positions first .. first + count - 1 -> (bounds [count,2]
    (xmin, taps), kk [count,ksize] int64)"""
    count = out_size - first if count is None else count
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((count, 2), np.int64)
    kk = np.zeros((count, ksize), np.int64)
    ss = 1.0 / filterscale
    for i in range(count):
        centre = (first + i + 0.5) * scale
        xmin = max(int(centre - support + 0.5), 0)
        xmax = min(int(centre + support + 0.5), in_size) - xmin
        k = [_bicubic((x + xmin - centre + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        for x, v in enumerate(k):
            v = v / ww if ww != 0.0 else v
            kk[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[i] = xmin, xmax
    return bounds, kk


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_crop(img, S):
    """uint8 [h,w,3] -> uint8 [S,S,3]: only the columns and rows the centre crop reads are filtered"""
    img = np.asarray(img, np.uint8)
    h, w, _ = img.shape
    nh, nw = resized_size(h, w, S)
    top, left = (nh - S) // 2, (nw - S) // 2
    half = 1 << (PRECISION_BITS - 1)
    if nw != w:
        b, k = coeffs(w, nw, left, S)
        src = img.astype(np.int64)
        hor = np.empty((h, S, 3), np.uint8)
        for x in range(S):
            x0, n = b[x]
            hor[:, x] = _clip8(half + np.einsum("rtc,t->rc", src[:, x0:x0 + n], k[x, :n]))
    else:
        hor = img[:, left:left + S]
    if nh != h:
        b, k = coeffs(h, nh, top, S)
        src = hor.astype(np.int64)
        out = np.empty((S, S, 3), np.uint8)
        for y in range(S):
            y0, n = b[y]
            out[y] = _clip8(half + np.einsum("txc,t->xc", src[y0:y0 + n], k[y, :n]))
    else:
        out = hor[top:top + S]
    return np.ascontiguousarray(out)


def pixel_values(crop):
    """uint8 [S,S,3] -> float32 [3,S,S]: rescale in fp64 rounded once, then (f - mean) / std in fp32"""
    f = (crop.astype(np.float64) * (1.0 / 255.0)).astype(np.float32)
    return np.ascontiguousarray(((f - MEAN) / STD).astype(np.float32).transpose(2, 0, 1))


def class_embeddings(e):
    """e [V,P,D] -> c [V,D] float32 = normalise(mean_p e[v][p]) in fp64, rounded once"""
    e = np.asarray(e, np.float64)
    m = e.sum(axis=1) / e.shape[1]
    return (m / np.sqrt((m * m).sum(axis=1, keepdims=True))).astype(np.float32)


def cosines(img, cls):
    """img [T,D], cls [V,D] float32 -> cos [T,V] float32: 64 partial sums, partial l over k = l, l + 64, ... ascending with a separate
    multiply and add, then the xor butterfly 32, 16, 8, 4, 2, 1"""
    img, cls = np.asarray(img, np.float32), np.asarray(cls, np.float32)
    T, D = img.shape
    V = cls.shape[0]
    assert D % 64 == 0 and cls.shape[1] == D
    p = np.zeros((T, V, 64), np.float32)
    for j in range(D // 64):
        p = p + img[:, None, 64 * j:64 * j + 64] * cls[None, :, 64 * j:64 * j + 64]
    lanes = np.arange(64)
    for x in (32, 16, 8, 4, 2, 1):
        p = p + p[:, :, lanes ^ x]
    assert p.dtype == np.float32 and ((p == p[:, :, :1]) | np.isnan(p)).all()         # every lane holds the same bits
    return np.ascontiguousarray(p[:, :, 0])


def object_scores(cos, obj_of, n_objs):
    """cos [T,V], obj_of [T] non-decreasing -> s [n_objs,V] float32: cos summed per object in record order"""
    s = np.zeros((n_objs, cos.shape[1]), np.float32)
    for t, o in enumerate(obj_of):
        s[o] = s[o] + cos[t]
    s[np.isnan(s)] = -np.inf                     # a score that is no number ranks, and is reported, as minus infinity
    return s


def topk(s, k):
    """s [n_objs,V] -> (idx uint32 [n_objs,k], score float32 [n_objs,k]): score descending, ties to the lower index"""
    idx = np.stack([np.lexsort((np.arange(s.shape[1]), -row.astype(np.float64)))[:k] for row in s]).astype(np.uint32)
    return idx, np.take_along_axis(s, idx.astype(np.int64), 1)


def vote(img, obj_of, cls, n_objs, k):
    return topk(object_scores(cosines(img, cls), obj_of, n_objs), k)
