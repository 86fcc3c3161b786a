"""Marcher edge cases: a constant field, so that a pixel's alpha counts the lattice points the marcher sampled.

THE FIELD.  Every case renders a NerfModel whose five MLP matrices are zero: sigma = exp(0) = 1 and rgb = sigmoid(0) = 0.5 at
every point, on the oracle and on the device in every `mlp_f16` / `render_arith` mode.  The background is (0, 0, 0, 0), so the
frame's alpha channel is the accumulated A itself, and A depends only on WHICH lattice points of the ray were sampled:

  unit-cube models (aabb_scale 1)   every sample has the weight a (1 - A) with a = 1 - exp(-dt), so A = 1 - (1 - a)^n and
                                    n = round(log1p(-A) / log1p(-a))                                       (`decode_counts`)
  cone models (aabb_scale 2, 4)     the steps grow along the ray, so A itself is compared with the oracle's A.  The bar comes
                                    from the reference: half of the smallest weight a single sample can have had in that frame,
                                    0.5 (1 - exp(-dt_min)) (1 - max A_ref)                                     (`alpha_bar`)

`min_transmittance` (MIN_T) is set so that no ray terminates early; `max A_ref < 1 - MIN_T` is asserted on the oracle's frames
before anything is compared (tests/test_march_edges_host.py, and again in the GPU test).

WHY EQUAL COUNTS PROVE EQUAL SETS.  The oracle (oracle/d2r_oracle.c d2r_oracle_render) tests every lattice point k = 0, 1, ...
of a ray until the first one outside the render box.  The device (dream2real_amd/csrc/nerf.hip) jumps: make_ray's window,
next_sample's skips, k_raygen's first sample.  But every point the device DOES sample has passed occ_cell's inside test and its
occupancy bit, and both are the oracle's own fp32 expressions (the same fma order, both built with -ffp-contract=off): the
device's sample set is a subset of {inside and occupied points}.  The oracle's set is the part of that before its first outside
point; the host test checks on every case that no occupied inside point follows an outside one, so the two coincide and the
device's set is a subset of the oracle's.  A subset with the same number of elements is the same set.

The host test also checks that the decoding is exact on the oracle's own frames (the decoded counts add up to the oracle's
n_samples) and that fp32 accumulation error (n_max 2^-24) stays under a quarter of the bar.

Cameras are given in the model's own (ngp) coordinates, 3x4 [x | y | forward | origin]; the views have dataset scale 1 and offset
0, for which nerf_matrix_to_ngp is a permutation with sign flips, i.e. exact (`cams_nerf`).
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from dream2real_amd.scene import DT, GRID, NerfModel, View, grid_levels, pack_bits

f32 = np.float32
MIN_T = 0.02                                          # no case may come within this of saturation (asserted)
A1 = f32(1.0) - np.exp(-DT, dtype=f32)                # weight of one sample of the constant lattice at T = 1
RGBA_ATOL, DEPTH_ATOL = 5e-3, 2e-3                    # the suite's existing bars (tests/test_gpu_parity.py)


def decode_counts(alpha) -> np.ndarray:
    """per-pixel sample count of a unit-cube frame from its alpha channel"""
    return np.rint(np.log1p(-np.asarray(alpha, np.float64)) / np.log1p(-float(A1))).astype(np.int64)


def alpha_bar(alpha_ref) -> float:
    """half of the smallest single-sample weight the oracle can have produced in these frames"""
    return 0.5 * float(A1) * (1.0 - float(np.max(alpha_ref)))


# ------------------------------------------------------------------ models

def n_cascades(aabb_scale: int) -> int:
    return int(aabb_scale).bit_length()


def cell_centre(cascade: int, cell_xyz) -> np.ndarray:
    """world (ngp) position of the centre of a cell of cascade c: the cube of side 2^c about 0.5 in 128^3 cells"""
    return 0.5 + ((np.asarray(cell_xyz, np.float64) + 0.5) / GRID - 0.5) * float(1 << cascade)


_I = np.arange(GRID)
_Z, _Y, _X = np.meshgrid(_I, _I, _I, indexing="ij")


def _cells(cells) -> np.ndarray:
    o = np.zeros((GRID, GRID, GRID), bool)
    for x, y, z in cells:
        o[z, y, x] = True
    return o


def _random(density: float, seed: int) -> np.ndarray:
    return np.random.Generator(np.random.PCG64(seed)).random((GRID, GRID, GRID)) < density


INTERIOR_BRICK = (13, 17, 9)                          # cells (52..55, 68..71, 36..39)

UNIT_PATTERNS = {
    # the whole cube, thinned to a shell 12 cells thick (see test_march_edges_host.py: the full cube's ~1024 samples per ray
    # would let fp32 accumulation error reach a quarter of the bar); the bounding box is still the whole cube
    "shell": lambda: np.minimum(np.minimum(np.minimum(_X, 127 - _X), np.minimum(_Y, 127 - _Y)), np.minimum(_Z, 127 - _Z)) < 12,
    "empty": lambda: np.zeros((GRID, GRID, GRID), bool),
    "corners8": lambda: _cells([(x, y, z) for x in (0, 127) for y in (0, 127) for z in (0, 127)]),
    "cell_000": lambda: _cells([tuple(4 * b for b in INTERIOR_BRICK)]),
    "cell_333": lambda: _cells([tuple(4 * b + 3 for b in INTERIOR_BRICK)]),
    "checker_cells": lambda: ((_X + _Y + _Z) & 1) == 0,
    "checker_bricks": lambda: (((_X >> 2) + (_Y >> 2) + (_Z >> 2)) & 1) == 0,
    "exit_corner": lambda: ((_X & 3) == 3) & ((_Y & 3) == 3) & ((_Z & 3) == 3),
    "slabs": lambda: (_Z == 10) | (_Z == 110),
    "rand0.5": lambda: _random(0.005, 31),
    "rand5": lambda: _random(0.05, 32),
    "rand50": lambda: _random(0.5, 33),
}

# single cells of the cone models: (cascade, cell).  Index 0 / 127 of cascade c touches the boundary of cascade c from inside;
# index 31 / 96 of cascade c + 1 touches it from outside (cascade c + 1 holds cascade c's cube in its cells 32..95).
CONE_CELLS = {
    "c0_lo": (0, (0, 60, 61)), "c0_hi": (0, (127, 64, 70)),
    "c1_out_lo": (1, (31, 64, 64)), "c1_out_hi": (1, (96, 70, 60)),
    "c1_000": (1, (8, 68, 36)), "c1_333": (1, (11, 71, 39)),
    "c1_lo": (1, (60, 0, 61)), "c1_hi": (1, (64, 70, 127)),
    "c2_out_lo": (2, (64, 31, 64)), "c2_out_hi": (2, (70, 60, 96)),
    "c2_only": (2, (5, 6, 7)),
    "tb1": (1, (70, 60, 64)), "tb2": (2, (70, 60, 64)),
}


@functools.lru_cache(maxsize=None)
def occupancy(pattern: str, aabb_scale: int) -> np.ndarray:
    """[n_cascades, z, y, x] bool"""
    nc = n_cascades(aabb_scale)
    if aabb_scale == 1:
        return UNIT_PATTERNS[pattern]()[None]
    occ = np.zeros((nc, GRID, GRID, GRID), bool)
    if pattern in CONE_CELLS:
        c, cell = CONE_CELLS[pattern]
        occ[c] = _cells([cell])
    elif pattern == "empty":
        pass
    elif pattern.startswith("rand"):
        d = float(pattern[4:]) / 100.0
        for c in range(nc):
            occ[c] = _random(d, 40 + 10 * aabb_scale + c)
    elif pattern == "corners8":
        for c in range(nc):
            occ[c] = UNIT_PATTERNS["corners8"]()
    else:
        raise KeyError(pattern)
    return occ


@functools.lru_cache(maxsize=None)
def model(pattern: str, aabb_scale: int = 1, render_aabb=None) -> NerfModel:
    levels = grid_levels(log2_hashmap_size=15, aabb_scale=aabb_scale)
    rg = np.random.Generator(np.random.PCG64(7))
    grid = rg.uniform(-0.5, 0.5, size=(levels.n_entries, levels.n_features)).astype(np.float16)       # any tables
    z = lambda r, c: np.zeros((r, c), np.float16)
    occ = occupancy(pattern, aabb_scale)
    return NerfModel(levels, grid, z(64, levels.n_levels * levels.n_features), z(16, 64), z(64, 32), z(64, 64), z(16, 64),
                     pack_bits(occ if aabb_scale > 1 else occ[0]), aabb_scale, render_aabb)


# ------------------------------------------------------------------ cameras

def look_at(eye, target, up=(0.0, 0.0, 1.0)) -> np.ndarray:
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    if np.linalg.norm(x) < 1e-6:
        x = np.cross((0.0, 1.0, 0.0), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z, eye], axis=1).astype(f32)


def axis_cam(fwd_axis: int, sign: float, eye) -> np.ndarray:
    """rotation = an axis permutation: forward along +-axis, the other two columns the remaining unit vectors"""
    m = np.zeros((3, 4), f32)
    m[(fwd_axis + 1) % 3, 0] = 1.0
    m[(fwd_axis + 2) % 3, 1] = 1.0
    m[fwd_axis, 2] = sign
    m[:, 3] = eye
    return m


def cams_nerf(cams_ngp, scale: float = 1.0) -> np.ndarray:
    """the matrices to hand to set_nerf_camera_matrix so that nerf_matrix_to_ngp (scale a power of two, offset 0) returns
    cams_ngp exactly"""
    g = np.asarray(cams_ngp, f32).reshape(-1, 3, 4)
    r = g[:, [2, 0, 1], :]
    return (r * np.array([1.0, -1.0, -1.0, 1.0 / scale], f32)).astype(f32)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    group: str
    pattern: str
    aabb_scale: int
    width: int
    height: int
    focal: float
    cams: tuple                      # of 3x4 ngp cameras, as nested tuples (hashable)
    near: float = 0.0
    render_aabb: tuple | None = None
    min_hits: int = 1                # hit pixels the oracle must see over the case's cameras
    min_long_skips: int = 0          # device skips longer than one step that the case must contain (numpy restatement)
    scale: float = 1.0               # dataset scale of the view, a power of two (depth = distance / scale; composite cases)

    @property
    def cone(self) -> bool:
        return self.aabb_scale > 1

    def cam_array(self) -> np.ndarray:
        return np.asarray(self.cams, f32).reshape(-1, 3, 4)

    def view(self) -> View:
        return View(self.width, self.height, (self.focal, self.focal), (0.5, 0.5), scale=self.scale, offset=(0.0, 0.0, 0.0),
                    background=(0.0, 0.0, 0.0, 0.0), min_transmittance=MIN_T, near_distance=self.near)

    def model(self) -> NerfModel:
        return model(self.pattern, self.aabb_scale, self.render_aabb)


def _t(cams):
    return tuple(tuple(map(tuple, np.asarray(c, f32).tolist())) for c in cams)


def _case(name, group, pattern, s, w, h, focal, cams, **kw) -> Case:
    return Case(name, group, pattern, s, w, h, float(focal), _t(cams), **kw)


C = (0.5, 0.5, 0.5)
OBLIQUE = [look_at((1.6, 1.3, -0.7), C), look_at((-0.9, 0.2, 1.9), C), look_at((0.3, -1.2, 0.9), C)]


def _first_cell(pattern: str, want: bool):
    """the cell nearest to the grid centre (in index order) that is / is not occupied"""
    occ = occupancy(pattern, 1)[0]
    for z, y, x in np.argwhere(occ[60:70, 60:70, 60:70] == want):
        return (int(x) + 60, int(y) + 60, int(z) + 60)
    raise AssertionError


def _build() -> list:
    cs = []
    # ---- occupancy patterns at aabb_scale 1, oblique cameras outside the cube (33 x 17 and 16 x 16)
    for p in ("shell", "empty", "corners8", "checker_cells", "checker_bricks", "exit_corner", "slabs", "rand0.5", "rand5", "rand50"):
        hits = {"empty": 0, "corners8": 2, "rand0.5": 100}.get(p, 250)
        skips = 0 if p in ("empty", "checker_cells") else 20
        if p == "corners8":              # a corner cell is a tenth of a pixel in the oblique views: aim at two opposite corners
            cams = [look_at(OBLIQUE[0][:, 3], cell_centre(0, (127, 127, 0))), look_at(OBLIQUE[1][:, 3], cell_centre(0, (0, 0, 127)))]
            cs.append(_case(f"{p}-33x17", "patterns", p, 1, 33, 17, 700.0, cams, min_hits=8, min_long_skips=8))
            cs.append(_case(f"{p}-16x16", "patterns", p, 1, 16, 16, 700.0, [look_at(OBLIQUE[2][:, 3], cell_centre(0, (127, 0, 127)))], min_hits=4, min_long_skips=4))
            continue
        cs.append(_case(f"{p}-33x17", "patterns", p, 1, 33, 17, 28.0, OBLIQUE[:2], min_hits=hits, min_long_skips=skips))
        cs.append(_case(f"{p}-16x16", "patterns", p, 1, 16, 16, 13.0, OBLIQUE[2:], min_hits=hits // 12, min_long_skips=skips // 2))
    # one cell, at brick-local (0,0,0) and (3,3,3) of an interior brick, from all eight octants
    for p in ("cell_000", "cell_333"):
        cell = tuple(4 * b + (3 if p == "cell_333" else 0) for b in INTERIOR_BRICK)
        tgt = cell_centre(0, cell)
        cams = [look_at(tgt + 0.9 * np.array([sx * 0.62, sy * 0.55, sz * 0.56]), tgt) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
        cs.append(_case(f"{p}-octants", "patterns", p, 1, 16, 16, 900.0, cams, min_hits=8 * 20, min_long_skips=8))
    # ---- rays
    e, o = _first_cell("rand5", False), _first_cell("rand5", True)
    cs.append(_case("inside-empty-cell", "rays", "rand5", 1, 33, 17, 20.0, [look_at(cell_centre(0, e), (0.9, 0.8, 0.1))], min_hits=300, min_long_skips=20))
    cs.append(_case("inside-occupied-cell", "rays", "rand5", 1, 33, 17, 20.0, [look_at(cell_centre(0, o), (0.1, 0.9, 0.7))], min_hits=300, min_long_skips=20))
    cs.append(_case("near-outside", "rays", "rand5", 1, 33, 17, 28.0, OBLIQUE[:1], near=0.3, min_hits=250, min_long_skips=20))
    cs.append(_case("near-into-cube", "rays", "slabs", 1, 16, 16, 13.0, [look_at((0.5, 0.45, -0.2), C, up=(0, 1, 0))], near=0.4, min_hits=100, min_long_skips=20))
    # rotation = identity / axis permutation at odd sizes: the centre pixel's direction has two exact zeros; origin on cell faces
    # (0.5 = 64 / 128 on both transverse axes) and off them (cell centre)
    for tag, off in (("on-face", 0.0), ("off-face", 1.0 / 256.0)):
        cams = [axis_cam(2, 1.0, (0.5 + off, 0.5 + off, -0.25)), axis_cam(0, -1.0, (1.25, 0.5 + off, 0.5 + off)),
                axis_cam(1, 1.0, (0.5 + off, -0.25, 0.5 + off))]
        for p in ("rand50", "slabs"):
            cs.append(_case(f"axis-{tag}-{p}", "rays", p, 1, 33, 17, 25.0, cams, min_hits=150, min_long_skips=0 if p == "rand50" else 20))
    # the (1,1,1) diagonal from a lattice-aligned origin: tx == ty == tz at every skip (1 x 1 and 3 x 3)
    diag = look_at((-0.25, -0.25, -0.25), (0.75, 0.75, 0.75))
    for p in ("checker_cells", "rand5", "exit_corner"):
        cs.append(_case(f"diagonal-1x1-{p}", "rays", p, 1, 1, 1, 300.0, [diag], min_hits=1))
        cs.append(_case(f"diagonal-3x3-{p}", "rays", p, 1, 3, 3, 300.0, [diag], min_hits=9))
    # grazing: forward along +z with the centre column in the face plane x = 1 (and x = 0), along the cube edge x = y = 1, and just
    # outside (the centre column misses by 0.0005, under a pixel at this focal length)
    for p in ("shell", "rand50"):
        cams = [axis_cam(2, 1.0, (1.0, 0.5, -0.3)), axis_cam(2, 1.0, (0.0, 0.37, -0.3)), axis_cam(2, 1.0, (1.0, 1.0, -0.3)),
                axis_cam(2, 1.0, (1.0005, 0.5, -0.3)), axis_cam(0, 1.0, (-0.3, 0.0, 1.0))]
        cs.append(_case(f"graze-{p}", "rays", p, 1, 33, 17, 40.0, cams, min_hits=500))
    # ---- cone models: one cell per model, seen along one oblique direction from 0.3 (constant steps), just past the crossings
    # t = 1 and t = 2 (the cascade choice changes in empty space just before the cell), and from further out
    dirn = np.array([0.48, -0.62, 0.62])
    dirn /= np.linalg.norm(dirn)
    for s in (2, 4):
        for key, (c, cell) in CONE_CELLS.items():
            if c >= n_cascades(s) or key.startswith("tb"):
                continue
            tgt = cell_centre(c, cell)
            w = float(1 << c) / GRID
            dists = (0.3, 0.98, 1.0 + 1.5 * w, 2.0 + 1.5 * w) if s == 4 else (0.3, 0.98, 1.0 + 1.5 * w, 1.6)
            for D in dists:
                # past t = 2^c the step has grown to the next cascade's cells and cascade c is no longer read (unless it is the
                # top one): such a view of a cascade-c cell sees nothing and could not fail
                if c != n_cascades(s) - 1 and D + w >= float(1 << c):
                    continue
                cs.append(_case(f"s{s}-{key}-d{D:.3f}", "cone", key, s, 16, 16, 7.0 * D / w, [look_at(tgt - D * dirn, tgt)], min_hits=1))
        # the tb clamp, targeted: the ray crosses empty cascade-0 (cascade-1) bricks up to t = 1 (t = 2), where the step has grown
        # to the next cascade's cells, and the one occupied cell of THAT cascade begins a tenth of a cell past the crossing
        for tb, c in ((1, 1), (2, 2)):
            if c >= n_cascades(s):
                continue
            w = float(1 << c) / GRID
            tgt = cell_centre(c, (70, 60, 64))
            D = float(tb) + 0.6 * w
            cs.append(_case(f"s{s}-tb{tb}", "cone", f"tb{tb}", s, 16, 16, 7.0 * D / w, [look_at(tgt - D * dirn, tgt)], min_hits=8, min_long_skips=8))
        # a ray IN the plane x = 1 of the unit cube (centre column of an axis camera at an odd width): max|p - 0.5| * side is
        # exactly 0.5 at every lattice point, the equality of the cascade choice
        cs.append(_case(f"s{s}-on-cascade-face", "cone", "rand5", s, 33, 17, 30.0, [axis_cam(2, 1.0, (1.0, 0.5, -0.3)), axis_cam(1, -1.0, (0.37, 1.4, 0.0))], min_hits=300, min_long_skips=20))
        # t0 >= D2R_T_LINEAR (k1 = 0) and t0 just under it, looking into seeded random occupancy of every cascade
        half = 0.5 * s
        for tag, dz in (("k1-zero", 0.45), ("under-linear", 0.43), ("far", 1.3)):
            cam = look_at((0.55, 0.48, 0.5 - half - dz), (0.5, 0.5, 0.5), up=(0, 1, 0))
            cs.append(_case(f"s{s}-rand5-{tag}", "cone", "rand5", s, 33, 17, 22.0, [cam], min_hits=400, min_long_skips=20))
        cs.append(_case(f"s{s}-rand5-inside", "cone", "rand5", s, 16, 16, 11.0, [look_at((0.2, 0.3, 0.4), (1.4, 1.2, 0.9))], min_hits=200, min_long_skips=20))
        corner = cell_centre(n_cascades(s) - 1, (127, 127, 0))
        cs.append(_case(f"s{s}-corners8", "cone", "corners8", s, 33, 17, 160.0, [look_at((0.5 + 0.8 * s, 0.5 + 0.65 * s, 0.5 - 0.9 * s), corner)], min_hits=2))
        cs.append(_case(f"s{s}-empty", "cone", "empty", s, 16, 16, 11.0, [look_at((0.2, 0.3, 0.4), (1.4, 1.2, 0.9))], min_hits=0))
    # ---- render boxes: through the middle of occupied cells, a single cell layer, and a crop holding no occupied cell
    cs.append(_case("crop-mid-cell", "crop", "rand50", 1, 33, 17, 28.0, OBLIQUE[:2], render_aabb=(0.2539, 0.1, 0.3, 0.7461, 0.9, 0.6), min_hits=150))
    cs.append(_case("crop-one-layer", "crop", "rand50", 1, 33, 17, 28.0, OBLIQUE[:2], render_aabb=(0.0, 0.0, 0.5, 1.0, 1.0, 0.5078125), min_hits=150))
    cs.append(_case("crop-nothing", "crop", "slabs", 1, 33, 17, 28.0, OBLIQUE[:2], render_aabb=(0.0, 0.0, 0.3, 1.0, 1.0, 0.6), min_hits=0))
    cs.append(_case("crop-cone", "crop", "rand5", 2, 33, 17, 22.0, [look_at((0.55, 0.48, -1.4), C, up=(0, 1, 0)), look_at((2.1, 1.7, 1.2), C)],
                    render_aabb=(-0.3, -0.2, 0.1, 1.2, 0.9, 1.4), min_hits=300, min_long_skips=20))
    cs.append(_case("crop-cone-nothing", "crop", "c1_out_hi", 2, 16, 16, 14.0, [look_at((2.1, 1.7, 1.2), C)], render_aabb=(-0.3, -0.2, 0.1, 0.9, 0.9, 1.4), min_hits=0))
    # ---- variants: one sparse and one dense pattern at each aabb_scale; three cameras, the middle one looking away from the box
    for s in (1, 2, 4):
        away = look_at((0.5 + 0.9 * s, 0.5 + 0.7 * s, 0.5 - 1.1 * s), (0.5 + 3.0 * s, 0.5 + 3.0 * s, 0.5 - 3.0 * s))
        seeing = [look_at((0.5 + 0.9 * s, 0.5 + 0.7 * s, 0.5 - 1.1 * s), C), look_at((0.5 - 1.2 * s, 0.5 + 0.1 * s, 0.5 + 0.8 * s), C)]
        for p in ("rand0.5", "rand5" if s > 1 else "rand50"):
            cs.append(_case(f"variants-s{s}-{p}", "variants", p, s, 33, 17, 26.0, [seeing[0], away, seeing[1]], min_hits=100 if p == "rand0.5" else 500))
    # ---- composite path: one cell (the bounding box k_raygen_rect projects is that cell), aimed so that it lands on one or two
    # pixels at each frame edge, just outside the frame, and in the middle.  Dataset scale 1/64: depths are distances x 64, so a
    # single sample already passes the composite's 0.05 depth floor
    for name, p, s, c, cell in (("cell_000", "cell_000", 1, 0, tuple(4 * b for b in INTERIOR_BRICK)),
                                ("cell_333", "cell_333", 1, 0, tuple(4 * b + 3 for b in INTERIOR_BRICK)),
                                ("s2-c1_out_lo", "c1_out_lo", 2, 1, CONE_CELLS["c1_out_lo"][1])):
        tgt = cell_centre(c, cell)
        eye = tgt - 0.9 * dirn
        focal = 1.6 * 0.9 / (float(1 << c) / GRID)
        cams = [aimed(eye, tgt, 33, 17, focal, px, py) for _, px, py in COMPOSITE_AIMS]
        cs.append(_case(f"composite-{name}", "composite", p, s, 33, 17, focal, cams, min_hits=6, scale=1.0 / 64.0))
    return cs


# where the cell's centre is aimed (pixel coordinates) in the seven cameras of a composite case
COMPOSITE_AIMS = [("left", 0.2, 8.0), ("right", 31.8, 8.0), ("top", 16.0, 0.2), ("bottom", 16.0, 15.8),
                  ("out-right", 35.0, 8.0), ("out-top", 16.0, -3.0), ("centre", 16.0, 8.0)]
BG_RGBA, BG_DEPTH = (0.2, 0.4, 0.6, 1.0), 50.0


def aimed(eye, tgt, W, H, focal, px, py) -> np.ndarray:
    """a camera at `eye` in which `tgt` appears (to first order) at pixel coordinates (px, py)"""
    base = look_at(eye, tgt).astype(np.float64)
    D = np.linalg.norm(np.asarray(tgt, np.float64) - np.asarray(eye, np.float64))
    a, b = (px + 0.5 - W / 2) / focal, (py + 0.5 - H / 2) / focal
    return look_at(eye, np.asarray(tgt, np.float64) - (a * base[:, 0] + b * base[:, 1]) * D)


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
GROUPS = sorted({c.group for c in CASES})

# the option sets of the `variants` group (d2r_ctx_set_option); each is held to the oracle's counts, not to another variant
DEFAULTS = dict(ray_sort=1, ray_sort_log2=4, march_compact=1, refill_min=64, bricks=1, march_threads=0)
VARIANTS = {
    "defaults": {},
    "sort-off": dict(ray_sort=0),
    "sort-log2-1": dict(ray_sort=1, ray_sort_log2=1),
    "compact-off": dict(march_compact=0),
    "refill-1": dict(refill_min=1),
    "compact-off-refill-1": dict(march_compact=0, refill_min=1),
    "bricks-off": dict(bricks=0),
    "threads-min": dict(march_threads=64),
    "threads-max": dict(march_threads="max"),
}


# ------------------------------------------------------------------ the oracle's frames, computed once per case

@functools.lru_cache(maxsize=None)
def oracle_frames(name: str):
    """(rgba [n, H, W, 4], depth [n, H, W], n_samples) of the case's cameras; read-only"""
    from oracle import render_ref
    case = BY_NAME[name]
    m = render_ref.OracleNerf(case.model())
    out = [render_ref.render(m, case.view(), cam) for cam in cams_nerf(case.cam_array(), case.scale)]
    rgba, depth = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    rgba.setflags(write=False)
    depth.setflags(write=False)
    return rgba, depth, sum(o[2] for o in out)


@functools.lru_cache(maxsize=None)
def composite_reference(name: str):
    """A composite case as render_composite sees it.  With obj_pose_now = cam_pose = identity the virtual camera of candidate i is
    inv(obj_poses[i]), formed in float64 from the float32 pose and rounded to float32 (k_cameras_virtual): the poses are the
    float32 inverses of the case's cameras, and the oracle renders from the cameras THEY invert to.
    -> (obj_poses [n, 4, 4] f32, oracle fg rgba, fg depth, oracle frames uint8 [n, H, W, 3])"""
    from oracle import render_ref
    case = BY_NAME[name]
    M = np.tile(np.eye(4), (len(case.cams), 1, 1))
    M[:, :3] = cams_nerf(case.cam_array(), case.scale)
    poses = np.linalg.inv(M).astype(f32)
    cams = np.linalg.inv(poses.astype(np.float64)).astype(f32)[:, :3]
    m = render_ref.OracleNerf(case.model())
    out = [render_ref.render(m, case.view(), cam) for cam in cams]
    rgba, depth = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    bg_rgba = np.broadcast_to(np.asarray(BG_RGBA, f32), rgba.shape[1:]).copy()
    bg_depth = np.full(depth.shape[1:], BG_DEPTH, f32)
    frames = np.stack([render_ref.composite(a, d, bg_rgba, bg_depth) for a, d in zip(rgba, depth)])
    return poses, rgba, depth, frames
