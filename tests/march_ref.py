"""numpy restatement of the marcher's sample-set logic (dream2real_amd/csrc/nerf.hip make_ray / occ_cell / next_sample and
the model set-up in api.hip), in fp32 and in the written order of operations, next to brute force over every lattice point
(oracle/d2r_oracle.c d2r_oracle_render's loop).  No GPU.  Used by tests/test_march_edges_host.py to check, case by case, that
the window and the skips lose no lattice point, and to count which cases would notice a wrong rule.

Where numpy cannot restate the device bit for bit it errs toward LONGER skips and NARROWER windows, the direction of a loss:
  * fmaf is formed in float64 and rounded once more to fp32 (the product of two fp32 numbers is exact in float64; the double
    rounding differs from a true fma only on an exact tie of the 53-bit sum, and the brute-force side shares the points);
  * v_rcp_f32 is accurate to 1 ulp: the reciprocals that size a skip are the correctly rounded ones times (1 + 2^-22);
  * __log2f (cone_index_of) is restated with numpy's log2: it only places the window, whose margin of two points absorbs it.
"""
from __future__ import annotations

import numpy as np

from dream2real_amd.scene import DT, GRID

f32, f64 = np.float32, np.float64
INV_DT = f32(1.0) / DT
CONE = f32(0.00390625)
T_LINEAR = DT * f32(256.0)
K_MAX = 1152                      # lattice points per ray held in memory; every ray must have left its box before (asserted)
RULES = ("skip_n_plus_1", "skip_n_plus_2", "window_margin_0", "window_margin_minus_1", "no_tb_clamp", "brick_skip_always", "cascade_gt", "far_face_ge")


def fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _cone_tables():
    lo, hi = np.zeros(64, f32), np.zeros(64, f32)
    p = 1.0
    for i in range(64):
        lo[i] = f32(p)
        p *= 1.00390625
    c64, q = p, 1.0
    for j in range(64):
        hi[j] = f32(q)
        q *= c64
    return lo, hi


CONE_LO, CONE_HI = _cone_tables()


def cone_pow(n):
    n = np.minimum(n, 4095)
    return CONE_HI[n >> 6] * CONE_LO[n & 63]


class Params:
    """api.hip d2r_nerf_create: cascades, bounding box of the occupied cells, render box"""

    def __init__(self, occ, aabb_scale: int, render_aabb=None):
        self.occ = occ                                          # [n_casc, z, y, x]
        self.n_casc = occ.shape[0]
        self.cone = aabb_scale > 1
        self.side = f32(aabb_scale)
        self.inv_side = f32(1.0) / f32(aabb_scale)
        self.word_nonzero = occ.reshape(self.n_casc, 32, 4, 32, 4, 32, 4).any(axis=(2, 4, 6))
        blo, bhi = np.full(3, 2.0, f32), np.full(3, -2.0, f32)
        for c in range(self.n_casc):
            idx = np.argwhere(occ[c])[:, ::-1]                  # x, y, z
            if not len(idx):
                continue
            cside = f32(1 << c) / f32(aabb_scale)
            org = f32(0.5) - f32(0.5) * cside
            blo = np.minimum(blo, org + cside * idx.min(0).astype(f32) / f32(GRID))
            bhi = np.maximum(bhi, org + cside * (idx.max(0) + 1).astype(f32) / f32(GRID))
        empty = bhi < blo
        self.bbox_lo = np.where(empty, f32(2.0), blo - f32(1e-4)).astype(f32)
        self.bbox_hi = np.where(empty, f32(-2.0), bhi + f32(1e-4)).astype(f32)
        half = f32(0.5) * f32(aabb_scale)
        box_lo, box_hi = f32(0.5) - half, f32(0.5) + half
        ra = np.zeros(6, f32) if render_aabb is None else np.asarray(render_aabb, f32)
        crop = bool((ra != 0).any())
        self.raabb_lo = np.maximum(box_lo, ra[:3]) if crop else np.full(3, box_lo, f32)
        self.raabb_hi = np.minimum(box_hi, ra[3:]) if crop else np.full(3, box_hi, f32)
        inv_side = f32(1.0) / (f32(2.0) * half)
        self.rn_lo = fma(self.raabb_lo - f32(0.5), inv_side, f32(0.5)) if self.cone else self.raabb_lo
        self.rn_hi = fma(self.raabb_hi - f32(0.5), inv_side, f32(0.5)) if self.cone else self.raabb_hi


def pixel_rays(cams, W: int, H: int, focal: float, near: float):
    """make_ray's first half for every pixel of every camera: origins and unit directions [R, 3] (R = n_cams H W)"""
    cams = np.asarray(cams, f32).reshape(-1, 3, 4)
    px, py = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    u = (px.reshape(-1) + f32(0.5)) / f32(W)
    v = (py.reshape(-1) + f32(0.5)) / f32(H)
    dcx = (u - f32(0.5)) * f32(W) / f32(focal)
    dcy = (v - f32(0.5)) * f32(H) / f32(focal)
    o, d = [], []
    for cam in cams:
        di = np.stack([fma(cam[i, 2], f32(1.0), fma(cam[i, 1], dcy, cam[i, 0] * dcx)) for i in range(3)], axis=1)
        oi = np.stack([fma(di[:, i], f32(near), cam[i, 3]) for i in range(3)], axis=1)
        inv_len = f32(1.0) / np.sqrt(fma(di[:, 2], di[:, 2], fma(di[:, 1], di[:, 1], di[:, 0] * di[:, 0])))
        o.append(oi)
        d.append(di * inv_len[:, None])
    return np.concatenate(o).astype(f32), np.concatenate(d).astype(f32)


def _slab(lo, hi, o, d):
    with np.errstate(all="ignore"):
        inv = f32(1.0) / d
        a, b = (lo - o) * inv, (hi - o) * inv
        return np.fmax.reduce(np.fmin(a, b), axis=1, initial=-np.inf), np.fmin.reduce(np.fmax(a, b), axis=1, initial=np.inf)


class Lattice:
    """every lattice point k < K_MAX of every ray: distance, position, inside test, cascade, cell and occupancy"""

    def __init__(self, P: Params, o, d, cascade_gt: bool = False):
        self.P = P
        R = o.shape[0]
        tmin, tmax = _slab(P.raabb_lo, P.raabb_hi, o, d)
        with np.errstate(invalid="ignore"):
            self.valid = (tmax >= tmin) & (tmax > 0)
        self.tmax = tmax
        self.t0 = (np.fmax(tmin, f32(0.0)) + f32(1e-6)).astype(f32)
        self.t0[~self.valid] = f32(0.0)
        if P.cone:
            self.o = fma(o - f32(0.5), P.inv_side, f32(0.5))
            self.d = (d * P.inv_side).astype(f32)
            with np.errstate(invalid="ignore"):
                self.k1 = np.where(self.t0 >= T_LINEAR, 0, np.ceil((T_LINEAR - self.t0) * INV_DT)).astype(np.int64)
        else:
            self.o, self.d = o, d
            self.k1 = np.full(R, K_MAX, np.int64)
        self.t1 = fma(self.k1.astype(f32), DT, self.t0)
        k = np.arange(K_MAX)[None, :]
        lin = fma(k.astype(f32), DT, self.t0[:, None])
        self.t = np.where(k <= self.k1[:, None], lin, self.t1[:, None] * cone_pow(np.maximum(k - self.k1[:, None], 0))).astype(f32) if P.cone else lin
        self.p = np.stack([fma(self.t, self.d[:, i, None], self.o[:, i, None]) for i in range(3)], axis=2)
        self.inside = ~((self.p < P.rn_lo) | (self.p > P.rn_hi)).any(axis=2)
        self.before_exit = np.logical_and.accumulate(self.inside, axis=1)
        assert not self.before_exit[self.valid, -1].any(), "K_MAX too small: a ray is still inside its box"
        self.dt = np.fmax(DT, self.t * CONE) if P.cone else np.full_like(self.t, DT)
        mip = np.zeros(self.t.shape, np.int64)
        q = self.p
        self.cell = np.full(self.t.shape, f32(1.0) / f32(GRID), f32)
        self.corg = np.zeros(self.t.shape, f32)
        top = P.n_casc - 1
        if P.cone:
            mxw = np.abs(self.p - f32(0.5)).max(axis=2) * P.side
            dt256 = self.dt * f32(256.0)
            half, step = f32(0.5), f32(1.0)
            for c in range(1, top + 1):
                mip[((mxw > half) | (dt256 > step)) if cascade_gt else ((mxw >= half) | (dt256 >= step))] = c
                half, step = half * f32(2.0), step * f32(2.0)
            sc = P.side / (f32(1.0) * (1 << mip)).astype(f32)
            low = mip != top
            q = np.where(low[..., None], fma(self.p - f32(0.5), sc[..., None], f32(0.5)), self.p)
            self.cell = np.where(low, f32(1.0) / (f32(GRID) * sc), self.cell).astype(f32)
            self.corg = np.where(low, f32(0.5) - f32(0.5) / sc, f32(0.0)).astype(f32)
        self.mip = mip
        with np.errstate(invalid="ignore"):
            self.c = np.clip((q * f32(GRID)).astype(np.int64), 0, GRID - 1)              # C's (int) truncates toward zero
        cx, cy, cz = self.c[..., 0], self.c[..., 1], self.c[..., 2]
        self.occ = P.occ[mip, cz, cy, cx]
        self.word_nonzero = P.word_nonzero[mip, cz >> 2, cy >> 2, cx >> 2]

    def brute_force(self):
        """the oracle's sample set [R, K_MAX]: every occupied lattice point before the first one outside the box"""
        return self.valid[:, None] & self.before_exit & self.occ

    def lost_by_the_oracles_break(self):
        """occupied inside points that FOLLOW an outside point (the subset argument of tests/march_cases.py needs none)"""
        return int((self.valid[:, None] & self.inside & ~self.before_exit & self.occ).sum())


def device_samples(L: Lattice, rule: str | None = None):
    """make_ray's window and next_sample's skips on the points of L -> (sample set [R, K_MAX], skip lengths taken)"""
    P = L.P
    R = L.t.shape[0]
    margin = {"window_margin_0": 0, "window_margin_minus_1": -1}.get(rule, 2 if P.cone else 1)
    bmin, bmax = _slab(P.bbox_lo, P.bbox_hi, L.o, L.d)
    hi = np.fmin(bmax, L.tmax)
    with np.errstate(invalid="ignore"):
        ok = L.valid & (hi >= bmin) & ~(hi < L.t0)
    lo = np.fmax(bmin, L.t0)

    def index_of(t):
        with np.errstate(all="ignore"):
            lin = (t - L.t0) * INV_DT
            if not P.cone:
                return lin
            return np.where(t <= L.t1, lin, L.k1.astype(f32) + np.log2(t / L.t1).astype(f32) * f32(177.79119873046875)).astype(f32)

    with np.errstate(invalid="ignore"):
        kl = np.floor(index_of(lo)) - f32(margin)
        k = np.where(kl > 0, kl, 0).astype(np.int64)
        k_hi = np.nan_to_num(np.ceil(index_of(hi)), nan=0.0, posinf=K_MAX, neginf=0.0).astype(np.int64) + margin
    k_hi = np.minimum(k_hi, K_MAX - 1)
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / L.d) * f32(1.0 + 2.0 ** -22)
    positive = (L.d >= 0) if rule == "far_face_ge" else (L.d > 0)
    out = np.zeros(L.t.shape, bool)
    skips = []
    act = np.flatnonzero(ok)
    top = P.n_casc - 1
    while len(act):
        ka = k[act]
        live = ka <= k_hi[act]
        act, ka = act[live], ka[live]
        live = L.inside[act, ka]
        act, ka = act[live], ka[live]
        hit = L.occ[act, ka]
        out[act[hit], ka[hit]] = True
        k[act[hit]] += 1
        a, kk = act[~hit], ka[~hit]
        if len(a):
            sh = np.where(L.word_nonzero[a, kk] & (rule != "brick_skip_always"), 0, 2)
            cell, corg, t = L.cell[a, kk], L.corg[a, kk], L.t[a, kk]
            cs = (1 << sh).astype(f32) * cell
            lw = fma(((L.c[a, kk] >> sh[:, None]) << sh[:, None]).astype(f32), cell[:, None], corg[:, None])
            with np.errstate(all="ignore"):
                tt = (np.where(positive[a], lw + cs[:, None], lw) - L.p[a, kk]) * inv[a]
                dist = np.fmin(np.fmin(tt[:, 0], tt[:, 1]), tt[:, 2])
                if P.cone:
                    if rule != "no_tb_clamp":
                        _, e = np.frexp(t)
                        tb = np.where(t < 1, f32(1.0), np.ldexp(f32(1.0), e)).astype(f32)       # 1; while (tb <= t) tb *= 2
                        dist = np.where(L.mip[a, kk] != top, np.fmin(dist, tb - t), dist)
                    n = np.floor(dist / np.fmax(DT, (t + np.fmax(dist, f32(0.0))) * CONE))
                else:
                    n = np.floor(dist * INV_DT)
            n = np.nan_to_num(n, nan=0.0, posinf=K_MAX, neginf=0.0).astype(np.int64)
            n = n + {"skip_n_plus_1": 1, "skip_n_plus_2": 2}.get(rule, 0)
            n = np.maximum(n, 1)
            skips.append(n)
            k[a] += n
        act = act[k[act] < K_MAX]
    return out, (np.concatenate(skips) if skips else np.zeros(0, np.int64))
