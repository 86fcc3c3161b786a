"""The colour-TSDF visual model restated in numpy: colour fusion on top of tests/tsdf_ref.py's volume, and
the ray caster.  The GPU (tsdf.hip's k_fuse_rgb, tsdfvis.hip) is held to this byte for byte.  Every step is one fp32 operation in
the rule's order; the ray caster evaluates EVERY sample index s = 0 .. S - 1 of every ray (it never skips), vectorised over rays.

Rule, ray caster: pixel (i, j) casts d_c = ((j - cx) / fx, (i - cy) / fy, 1); M [3,4] fp32 takes the camera frame to the volume's
frame (ray_matrix: composed in fp64, rounded once); o = M[:, 3], d_a = (M[a,0] x + M[a,1] y) + M[a,2]; t_s = near + (float)s voxel,
S = ceil((3 - near) / voxel) in fp64 of the fp32 values; p = o + t d; g = p / voxel, cell = floor(g), fraction g - floor(g); a
sample is observed when its cell's eight corners lie in the grid with weight >= thr; its value is the trilinear tsdf (x, then y,
then z, each a + f (b - a)).  Hit: the first s with sample s - 1 observed > 0 and sample s observed <= 0; t_hit = t_{s-1} +
(voxel v0) / (v0 - v1); colour = trilinear colour at p(t_hit) when that cell is observed, else at sample s; floor(c + 0.5)
clamped to 0 .. 255.  Composite: the movable hit wins where t_mov < t_bg; no hit: (0, 0, 0), depth +inf."""
from __future__ import annotations

import numpy as np

from tests import tsdf_ref

f32 = np.float32
BLOCK = tsdf_ref.BLOCK
DEPTH_MAX = 3.0


class ColourVolume(tsdf_ref.Volume):
    """tsdf_ref.Volume plus col float32 [nz][ny][nx][3]: at exactly the voxels a frame updates, c = (w c + rgb[v][u]) / (w + 1)
    with w the weight before the increment and (u, v) the pixel the voxel projected to."""

    def __init__(self, bounds, voxel=0.002, trunc=None):
        super().__init__(bounds, voxel, trunc)
        self.col = np.zeros(self.tsdf.shape + (3,), np.float32)

    def integrate_rgb(self, depth_u16, mask, rgb, intrinsics, cam_pose, erode_k):
        w0 = self.w.copy()
        if not self.integrate(depth_u16, mask, intrinsics, cam_pose, erode_k):
            return False
        iz, iy, ix = np.nonzero(self.w != w0)                      # the voxels whose (tsdf, weight) this frame updated
        K = np.asarray(intrinsics, np.float64).reshape(3, 3).astype(np.float32)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        Mi = tsdf_ref.rigid_inverse34(np.asarray(cam_pose, np.float64).reshape(4, 4).astype(np.float32))
        px = (ix + self.b0[0] * BLOCK).astype(np.float32) * self.voxel
        py = (iy + self.b0[1] * BLOCK).astype(np.float32) * self.voxel
        pz = (iz + self.b0[2] * BLOCK).astype(np.float32) * self.voxel
        xc, yc, zc = (((Mi[r, 0] * px + Mi[r, 1] * py) + Mi[r, 2] * pz) + Mi[r, 3] for r in range(3))
        u = np.floor(((fx * xc) / zc + cx) + f32(0.5)).astype(np.int64)      # section 2c's projection: these voxels passed its tests
        v = np.floor(((fy * yc) / zc + cy) + f32(0.5)).astype(np.int64)
        c = np.asarray(rgb, np.uint8)[v, u].astype(np.float32)
        w = w0[iz, iy, ix][:, None]
        self.col[iz, iy, ix] = (w * self.col[iz, iy, ix] + c) / (w + f32(1))
        return True

    def block_colours(self):
        """-> float32 [n,16,16,16,3] of the active blocks in active_blocks() order, indexed [z][y][x][channel]."""
        bz, by, bx = np.nonzero(self.ever)
        if not len(bz):
            return np.zeros((0, 16, 16, 16, 3), np.float32)
        return np.stack([self.col[z * 16:z * 16 + 16, y * 16:y * 16 + 16, x * 16:x * 16 + 16] for z, y, x in zip(bz, by, bx)])


# ---------------------------------------------------------------------------------------------------- matrices

def _mul4(A, B):
    C = np.zeros((4, 4), np.float64)
    for i in range(4):
        for j in range(4):
            C[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return C


def _rigid_inverse4(T):
    T = np.asarray(T, np.float32).astype(np.float64).reshape(4, 4)
    out = np.zeros((4, 4), np.float64)
    for i in range(3):
        for j in range(3):
            out[i, j] = T[j, i]
        out[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    out[3, 3] = 1.0
    return out


def ray_matrix(cam_pose, obj_pose_now=None, obj_pose=None):
    """-> float32 [3,4]: cam_pose for the background; (O inv(P)) cam_pose for the movable volume at candidate pose P."""
    C = np.asarray(cam_pose, np.float32).astype(np.float64).reshape(4, 4)
    if obj_pose is None:
        return C[:3].astype(np.float32)
    O = np.asarray(obj_pose_now, np.float32).astype(np.float64).reshape(4, 4)
    return _mul4(_mul4(O, _rigid_inverse4(obj_pose)), C)[:3].astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the ray caster

class View:
    def __init__(self, width, height, fx, fy, cx, cy, near=0.01):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy, self.near = f32(fx), f32(fy), f32(cx), f32(cy), f32(near)


# Wrong rules, one name each, as carry_gaps is: cast(..., wrong={name}) / render(..., wrong={name}) restate the rule with that one
# departure, so that a test can show that its cases tell the two apart (tests/test_tsdfvis_edges_host.py).  The last three are
# departures of the SKIPS (they change nothing unless skips=True).
WRONG_RULES = ("prev_ge", "v_lt", "w_gt", "colour_at_s", "colour_at_hit", "half_even", "wrap", "tie_movable", "s_fewer",
               "slab_no_pad", "rect_no_margin", "chi_lower")


def touched_box(vol):
    """-> (clo, chi) int64 [3] (x, y, z): a cell's lowest corner c (global voxel index) can be observed only for clo <= c <= chi, the
    box of the blocks any frame touched less its last voxel.  No block touched: an empty range."""
    bz, by, bx = np.nonzero(vol.ever)
    if not len(bz):
        return np.zeros(3, np.int64), np.full(3, -2, np.int64)
    lo = np.array([bx.min(), by.min(), bz.min()], np.int64)
    hi = np.array([bx.max(), by.max(), bz.max()], np.int64)
    return (vol.b0 + lo) * BLOCK, (vol.b0 + hi) * BLOCK + BLOCK - 2


def _sample(vol, p, thr, box=None, gt=False):
    """p float32 [n,3] -> (observed bool [n], trilinear tsdf float32 [n], cell (x, y, z) local int64 [n] each, fractions [n,3], cell
    inside bool [n], global cell float32 [n,3]).  box = (clo, chi): the GPU's skip, restated: a cell outside clo .. chi, or whose own
    block no frame touched, is unobserved without a look at its weights.  gt restates a WRONG rule: weight > thr."""
    lo = vol.b0 * BLOCK
    clo, chi = (lo, lo + vol.nv - 2) if box is None else box      # no box: both corners along every axis lie in the grid
    inside, c, fr = tsdf_ref.cell(p, vol.voxel, clo, chi)
    inside = inside.all(axis=1)
    q = [np.where(inside, c[:, a], lo[a]).astype(np.int64) - int(lo[a]) for a in range(3)]
    t = [vol.tsdf[q[2] + (k >> 2), q[1] + ((k >> 1) & 1), q[0] + (k & 1)] for k in range(8)]
    ok = inside.copy()
    if box is not None:
        ok &= vol.ever[q[2] >> 4, q[1] >> 4, q[0] >> 4]
    for k in range(8):
        w = vol.w[q[2] + (k >> 2), q[1] + ((k >> 1) & 1), q[0] + (k & 1)]
        ok &= (w > f32(thr)) if gt else (w >= f32(thr))
    return ok, tsdf_ref.lerp3(t, fr), q, fr, inside, c


def _colour_raw(vol, q, fr):
    t = [vol.col[q[2] + (k >> 2), q[1] + ((k >> 1) & 1), q[0] + (k & 1)] for k in range(8)]          # [n,3] each
    return tsdf_ref.lerp3(t, fr)


def _round_colour(raw, wrong=frozenset()):
    c = np.rint(raw) if "half_even" in wrong else np.floor(raw + f32(0.5))
    if "wrap" in wrong:
        return (np.nan_to_num(c).astype(np.int64) & 255).astype(np.uint8)
    return np.clip(c, 0, 255).astype(np.uint8)


def _colour(vol, q, fr):
    return _round_colour(_colour_raw(vol, q, fr))


def samples(near, voxel):
    return int(max(0.0, np.ceil((float(DEPTH_MAX) - float(f32(near))) / float(f32(voxel)))))


def rays(M, view):
    """-> (o, d) float32 [m H W, 3]: the rays of every pixel under every matrix, candidates outermost."""
    M = np.asarray(M, np.float32).reshape(-1, 3, 4)
    m, H, W = M.shape[0], view.height, view.width
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = ((jj.astype(np.float32) - view.cx) / view.fx).reshape(1, -1)
    y = ((ii.astype(np.float32) - view.cy) / view.fy).reshape(1, -1)
    o = np.stack([np.broadcast_to(M[:, a, 3:4], (m, H * W)).reshape(-1) for a in range(3)], 1)
    d = np.stack([((M[:, a, 0:1] * x + M[:, a, 1:2] * y) + M[:, a, 2:3]).reshape(-1) for a in range(3)], 1).astype(np.float32)
    return o, d


def slab_range(vol, o, d, near, S, pad=2.0, chi_lower=False, facts=None):
    """The GPU's first skip, restated in fp64 exactly as tv_cast computes it: -> (s0, s1) int64 [n], the sample indices whose point can
    lie in the touched-block box widened by two voxels and by what an fp32 sample point can be off; s1 < s0: none.  facts gains
    `d0_inside` / `d0_outside` (rays with a direction component exactly 0 whose origin lies inside / outside that axis's slab),
    `s0_clamped` (rays that start inside the box: the range starts at sample 0) and `s1_clamped` (it ends at S - 1)."""
    n = len(o)
    step, near = float(vol.voxel), float(f32(near))
    t_end = near + float(S) * step
    clo, chi = touched_box(vol)
    chi = chi - 1 if chi_lower else chi
    t0, t1, miss = np.full(n, near), np.full(n, t_end), np.zeros(n, bool)
    zero_in, zero_out = np.zeros(n, bool), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            oa, da = o[:, a].astype(np.float64), d[:, a].astype(np.float64)
            slack = 2.0 * step + 4e-6 * (np.abs(oa) + t_end * np.abs(da))
            L, Hh = float(f32(clo[a])) * step - slack, (float(f32(chi[a])) + 2.0) * step + slack
            nz = np.abs(da) > 0.0
            ta, tb = (L - oa) / da, (Hh - oa) / da
            t0 = np.where(nz, np.fmax(t0, np.fmin(ta, tb)), t0)
            t1 = np.where(nz, np.fmin(t1, np.fmax(ta, tb)), t1)
            out = ~nz & ((oa < L) | (oa > Hh))
            zero_out |= out
            zero_in |= ~nz & ~out
            miss |= out
        miss |= ~(t0 <= t1)
        lo = np.fmax(np.floor((t0 - near) / step) - pad, 0.0)
        hi = np.fmin(np.ceil((t1 - near) / step) + pad, float(S - 1))
    s0 = np.where(miss, 0, np.nan_to_num(lo, posinf=2.0 ** 40, neginf=-2.0 ** 40)).astype(np.int64)
    s1 = np.where(miss, -1, np.nan_to_num(hi, posinf=2.0 ** 40, neginf=-2.0 ** 40)).astype(np.int64)
    if facts is not None:
        live = ~miss & (s1 >= s0)
        for key, val in (("d0_inside", zero_in & ~zero_out), ("d0_outside", zero_out), ("s0_clamped", live & (t0 == near)),
                         ("s1_clamped", live & (s1 == S - 1) & (t1 == t_end))):
            facts[key] = facts.get(key, 0) + int(val.sum())
    return s0, s1


def box_rect(to_cam, lo, hi, slack, fx, fy, cx, cy, near, W, H, margin=1.0):
    """csrc/tsdfvis_rect.h's tv_box_rect restated (fp64): -> (x0, y0, x1, y1) inclusive; x1 < x0: no pixel."""
    whole, none = (0, 0, W - 1, H - 1), (0, 0, -1, -1)
    for a in range(3):
        if not (lo[a] <= hi[a]):
            return none if lo[a] > hi[a] else whole
    u, v = [], []
    with np.errstate(all="ignore"):
        for k in range(8):
            p = [np.float64(hi[a] + slack if (k >> a) & 1 else lo[a] - slack) for a in range(3)]
            q = [((to_cam[r][0] * p[0] + to_cam[r][1] * p[1]) + to_cam[r][2] * p[2]) + to_cam[r][3] for r in range(3)]
            if not (q[2] > near) or not (q[2] > 0.0):
                return whole
            u.append(np.float64(fx) * q[0] / q[2] + np.float64(cx))
            v.append(np.float64(fy) * q[1] / q[2] + np.float64(cy))
            if not np.isfinite(u[-1]) or not np.isfinite(v[-1]):
                return whole
    x0, x1 = max(np.floor(min(u)) - margin, 0.0), min(np.ceil(max(u)) + margin, W - 1.0)
    y0, y1 = max(np.floor(min(v)) - margin, 0.0), min(np.ceil(max(v)) + margin, H - 1.0)
    if x1 < x0 or y1 < y0:
        return none
    return int(x0), int(y0), int(x1), int(y1)


def candidate_rect(vol, view, cam_pose, obj_pose_now, obj_pose, margin=1.0, true_inverse=True):
    """The frame rectangle tv_prepare gives the movable volume `vol` at candidate pose P, restated (fp64): the touched-block box
    widened by a voxel and by what an fp32 sample point can be off, projected by the inverse of the ray matrix.  true_inverse: the
    fp64 inverse of the ROUNDED 3 x 4 matrix the kernel marches with (what tv_prepare does); False restates the first version, which
    composed inv(cam_pose) P inv(O) from transposed inverses and is off by twice a pose's deviation from orthogonal times the
    distance to that pose's origin."""
    C = np.asarray(cam_pose, np.float32).astype(np.float64).reshape(4, 4)
    O = np.asarray(obj_pose_now, np.float32).astype(np.float64).reshape(4, 4)
    P = np.asarray(obj_pose, np.float32).astype(np.float64).reshape(4, 4)
    M = _mul4(_mul4(O, _rigid_inverse4(obj_pose)), C)
    if true_inverse:
        Minv = inverse34(M[:3].astype(np.float32))
    else:
        Minv = _mul4(_mul4(_rigid_inverse4(cam_pose), P), _rigid_inverse4(obj_pose_now))
    step = float(vol.voxel)
    near = float(view.near)
    t_end = near + samples(near, vol.voxel) * step
    W, H = view.width, view.height
    fx, fy, cx, cy = (float(v) for v in (view.fx, view.fy, view.cx, view.cy))
    xmax = max(abs(0.0 - cx), abs(W - 1.0 - cx)) / abs(fx)
    ymax = max(abs(0.0 - cy), abs(H - 1.0 - cy)) / abs(fy)
    clo, chi = touched_box(vol)
    lo = [(float(clo[a]) - 1.0) * step for a in range(3)]           # box_lo - 1
    hi = [(float(chi[a]) + 1.0 + 2.0) * step for a in range(3)]     # box_hi + 2
    omax = max(abs(M[0, 3]), abs(M[1, 3]), abs(M[2, 3]))
    slack = 4e-6 * (omax + t_end * (xmax + ymax + 1.0))
    return box_rect(Minv, lo, hi, slack, fx, fy, cx, cy, near, W, H, margin)


def inverse34(M):
    """float32 [3,4] -> float64 [4,4]: the inverse of the affine map, by cofactors in fp64 in tv_inverse34's order; a singular or
    non-finite matrix gives NaNs (the rectangle is then the whole frame)."""
    m = np.asarray(M, np.float32).astype(np.float64).reshape(3, 4)
    a, b, c, d, e, f, g, h, i = (m[r, k] for r in range(3) for k in range(3))
    co = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f], [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = (a * co[0][0] + b * co[1][0]) + c * co[2][0]
    out = np.zeros((4, 4), np.float64)
    with np.errstate(all="ignore"):
        for r in range(3):
            for k in range(3):
                out[r, k] = co[r][k] / det
            out[r, 3] = -((out[r, 0] * m[0, 3] + out[r, 1] * m[1, 3]) + out[r, 2] * m[2, 3])
    out[3, 3] = 1.0
    return out


def _count(facts, key, n):
    facts[key] = facts.get(key, 0) + n


def cast(vol, M, view, thr=3.0, carry_gaps=False, facts=None, wrong=(), skips=False, rects=None):
    """One volume under the ray matrices M float32 [m,3,4], every pixel of `view` -> (hit bool [m,H,W], t float32 [m,H,W] (+inf: no
    hit), rgb uint8 [m,H,W,3]).  carry_gaps restates a WRONG rule: an unobserved sample between two observed ones does not break the
    pair (the last observed value is carried across the gap); wrong: names from WRONG_RULES.
    skips restates what the GPU leaves out: samples outside slab_range, cells outside touched_box or in an untouched block, and, with
    rects int [m,4], pixels outside their matrix's rectangle.  The result must not depend on it.
    facts: a dict that gains counts of what the march met (frac0, at_clo, at_chi per axis; hit_v0, first_obs_zero, zero_then_neg,
    pos_zero_neg, first_obs_neg, fallback, fallback_differs, hit_s1, hit_last, col_half, col_half_even, col_0, col_255,
    hit_after_empty_block) and `hits`, the number of hits per matrix; counted over every pixel, or, when `rects` is given (render passes
    it with skips only), over the pixels inside them.  A block counts as empty when every weight in it is 0."""
    wrong = frozenset(wrong)
    assert wrong <= set(WRONG_RULES), wrong
    M = np.asarray(M, np.float32).reshape(-1, 3, 4)
    m, H, W = M.shape[0], view.height, view.width
    o, d = rays(M, view)
    n = m * H * W
    step = vol.voxel
    S = samples(view.near, step)
    if "s_fewer" in wrong:
        S = max(S - 1, 0)
    live = np.ones(n, bool)
    if rects is not None:
        r = np.repeat(np.asarray(rects, np.int64).reshape(m, 4), H * W, axis=0)
        jj, ii = np.tile(np.tile(np.arange(W), H), m), np.tile(np.repeat(np.arange(H), W), m)
        live = (jj >= r[:, 0]) & (jj <= r[:, 2]) & (ii >= r[:, 1]) & (ii <= r[:, 3])
    box = None
    if skips:
        clo, chi = touched_box(vol)
        box = (clo, chi - 1 if "chi_lower" in wrong else chi)
        s0, s1 = slab_range(vol, o, d, view.near, S, 0.0 if "slab_no_pad" in wrong else 2.0, "chi_lower" in wrong,
                            None if facts is None else facts)
    tclo, tchi = touched_box(vol)
    occupied = (vol.w > 0).reshape(int(vol.nb[2]), BLOCK, int(vol.nb[1]), BLOCK, int(vol.nb[0]), BLOCK).any(axis=(1, 3, 5))
    hit = np.zeros(n, bool)
    t_hit = np.full(n, np.inf, np.float32)
    rgb = np.zeros((n, 3), np.uint8)
    prev_ok = np.zeros(n, bool)
    prev_v = np.zeros(n, np.float32)
    seen = np.zeros(n, bool)                   # facts: the ray has met an observed sample
    lead0 = np.zeros(n, bool)                  # its first observed sample was exactly 0 and the samples since are its direct successors
    pos0 = np.zeros(n, bool)                   # the previous sample was a hit with v == 0 after a positive one
    empty = np.zeros(n, bool)                  # it has crossed a cell of a block without any weight inside the touched-block box
    for s in range(S):
        t = view.near + f32(s) * step
        with np.errstate(all="ignore"):
            p = o + t * d
        ok, v, q, fr, inside, c = _sample(vol, p, thr, box, "w_gt" in wrong)
        ok &= live
        if skips:
            ok &= (s >= s0) & (s <= s1)
        cross = ((prev_v >= 0) if "prev_ge" in wrong else (prev_v > 0)) & ((v < 0) if "v_lt" in wrong else (v <= 0))
        new = ok & prev_ok & cross & ~hit
        if facts is not None:
            act = live & ~hit
            inbox = np.ones(n, bool)
            for a in range(3):
                inbox &= (c[:, a] >= tclo[a]) & (c[:, a] <= tchi[a])
            inbox &= act
            for a in range(3):
                facts.setdefault("frac0", np.zeros(3, np.int64))[a] += int((inbox & (fr[:, a] == 0)).sum())
                facts.setdefault("at_clo", np.zeros(3, np.int64))[a] += int((inbox & (c[:, a] == tclo[a])).sum())
                facts.setdefault("at_chi", np.zeros(3, np.int64))[a] += int((inbox & (c[:, a] == tchi[a])).sum())
            lo = vol.b0 * BLOCK
            qq = [np.where(inbox, c[:, a], lo[a]).astype(np.int64) - int(lo[a]) for a in range(3)]
            empty |= inbox & ~occupied[qq[2] >> 4, qq[1] >> 4, qq[0] >> 4]
            first = ok & ~seen & act
            _count(facts, "first_obs_zero", int((first & (v == 0)).sum()))
            _count(facts, "first_obs_neg", int((first & (v < 0)).sum()))
            _count(facts, "zero_then_neg", int((ok & lead0 & prev_ok & (prev_v == 0) & (v < 0) & act).sum()))
            _count(facts, "pos_zero_neg", int((ok & pos0 & (v < 0) & live).sum()))
            lead0 = first & (v == 0)
            pos0 = new & (v == 0)
            seen |= ok
        if new.any():
            idx = np.nonzero(new)[0]
            tp = view.near + f32(s - 1) * step
            v0, v1 = prev_v[idx], v[idx]
            with np.errstate(all="ignore"):
                th = (tp + (step * v0) / (v0 - v1)).astype(np.float32)
                ph = o[idx] + th[:, None] * d[idx]
            okh, _, qh, frh, insideh, _ = _sample(vol, ph, thr, box, "w_gt" in wrong)
            raw_s, raw_h = _colour_raw(vol, [a[idx] for a in q], fr[idx]), _colour_raw(vol, qh, frh)
            if "colour_at_s" in wrong:
                use_h = np.zeros(len(idx), bool)
            elif "colour_at_hit" in wrong:
                use_h = insideh                # whatever its weights; a hit cell outside the grid has nothing to read
            else:
                use_h = okh
            raw = np.where(use_h[:, None], raw_h, raw_s)
            rgb[idx] = _round_colour(raw, wrong)
            t_hit[idx] = th
            hit |= new
            if facts is not None:
                _count(facts, "hit_v0", int((v1 == 0).sum()))
                _count(facts, "fallback", int((~okh).sum()))
                _count(facts, "fallback_differs", int((~okh & insideh & (_round_colour(raw_h) != _round_colour(raw_s)).any(axis=1)).sum()))
                _count(facts, "hit_s1", int(s == 1) * len(idx))
                _count(facts, "hit_last", int(s == S - 1) * len(idx))
                half = (raw - np.floor(raw)) == f32(0.5)
                _count(facts, "col_half", int(half.any(axis=1).sum()))
                _count(facts, "col_half_even", int((half & (np.floor(raw) % 2 == 0)).any(axis=1).sum()))
                _count(facts, "col_0", int((rgb[idx] == 0).any(axis=1).sum()))
                _count(facts, "col_255", int((rgb[idx] == 255).any(axis=1).sum()))
                _count(facts, "hit_after_empty_block", int(empty[idx].sum()))
        if carry_gaps:
            prev_ok, prev_v = prev_ok | ok, np.where(ok, v, prev_v).astype(np.float32)
        else:
            prev_ok, prev_v = ok, np.where(ok, v, f32(0)).astype(np.float32)
    if facts is not None:
        facts["hits"] = list(facts.get("hits", [])) + [int(h) for h in hit.reshape(m, -1).sum(axis=1)]
        facts["S"] = S
    return hit.reshape(m, H, W), t_hit.reshape(m, H, W), rgb.reshape(m, H, W, 3)


def render(bg_vol, mv_vol, view, cam_pose, obj_pose_now, obj_poses, thr=3.0, facts=None, wrong=(), skips=False, true_inverse=True):
    """-> (frames uint8 [K,H,W,3], depth float32 [K,H,W], the background's own (hit, t, rgb)).  facts: gains "bg" and "mv", the two
    casts' dicts (see cast), and "rects".  wrong, skips: see cast; with skips the candidates' rectangles are candidate_rect's."""
    wrong = frozenset(wrong)
    poses = np.asarray(obj_poses, np.float32).reshape(-1, 4, 4)
    fb = fm = None
    if facts is not None:
        fb, fm = facts.setdefault("bg", {}), facts.setdefault("mv", {})
    bh, bt, bc = cast(bg_vol, ray_matrix(cam_pose)[None], view, thr, facts=fb, wrong=wrong, skips=skips)
    K = poses.shape[0]
    frames = np.broadcast_to(bc, (K,) + bc.shape[1:]).copy()
    depth = np.broadcast_to(bt, (K,) + bt.shape[1:]).copy()
    if K:
        rects = [candidate_rect(mv_vol, view, cam_pose, obj_pose_now, P, 0.0 if "rect_no_margin" in wrong else 1.0, true_inverse) for P in poses]
        if facts is not None:
            facts["rects"] = rects
        mh, mt, mc = cast(mv_vol, np.stack([ray_matrix(cam_pose, obj_pose_now, P) for P in poses]), view, thr, facts=fm, wrong=wrong,
                          skips=skips, rects=rects if skips else None)
        win = mh & ((mt <= depth) if "tie_movable" in wrong else (mt < depth))      # a tie goes to the background
        frames[win] = mc[win]
        depth[win] = mt[win]
    return frames, depth, (bh[0], bt[0], bc[0])
