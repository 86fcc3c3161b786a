"""Edge inputs of the colour-TSDF ray caster (tests/test_tsdfvis_edges_host.py, tests/test_tsdfvis_edges_gpu.py), each with the
facts that make it an edge: counted by the brute-force restatement (tests/tsdfvis_ref.py, `facts`) and asserted on the host, so
that an input which stops reaching its edge fails where no GPU is present.

Scenes.  "dy": dyadic and axis-aligned: voxels of 2^-8 m, truncation four voxels, fx = fy = 64, three fusing cameras with identity
rotation a whole number of voxels apart, a plane at 96 voxels (0.375 m) and a 32 x 32 voxel plate at 64 voxels (0.25 m) that fills its
volume's two blocks a side: every sdf is a whole number of voxels, every tsdf a multiple of 1/4, exactly 0 on the surfaces' voxel
planes, and the colours are whole numbers (a function of the surface point's voxel, so the cameras agree).  `off` moves the whole
scene by a whole number of voxels.  "blocks": one plane at 64 voxels seen through a mask of two patches in a 5 x 3 x 2 block volume,
with a never-touched block between them.  "sphere": tests/tsdfvis_cases.py's scene, moved rigidly."""
from __future__ import annotations

import functools

import numpy as np

from tests import tsdfvis_cases as cases
from tests import tsdfvis_ref as ref

f32 = np.float32
V = 1.0 / 256.0
W, H = 48, 40
K_DY = np.array([[64.0, 0, 24.0], [0, 64.0, 20.0], [0, 0, 1]])
DY_CAMS = ((-2, 0), (0, 0), (2, 1))                      # the fusing cameras' (x, y) in voxels
OFFSETS = {"0": (0.0, 0.0, 0.0), "40m": (40.0, -25.0, 12.0), "2km": (2048.0, -1024.0, 512.0)}      # whole voxels, exact in fp32
SPHERE_SHIFT = np.array([40.0, -25.0, 12.0])


def dy_frame(cn, patches=None, w=W, cx=24):
    """The fusing camera at (cn) voxels -> (depth u16, plate mask, rgb).  patches: the "blocks" scene: a plane at 64 voxels only."""
    ii, jj = np.meshgrid(np.arange(H), np.arange(w), indexing="ij")
    X, Y = jj - cx + cn[0], ii - 20 + cn[1]              # the voxel column a pixel sees on the plate's plane (fx = 64 = its depth)
    rgb = np.zeros((H, w, 3), np.uint8)
    rgb[..., 0] = (37 * X + 11 * Y) % 256                # neighbours differ by odd amounts
    rgb[..., 1] = np.where((X + Y) % 2 == 0, 255, 0)     # both clamps
    rgb[..., 2] = (3 * X + 5 * Y + 128) % 256
    if patches is not None:
        mask = np.zeros((H, w), bool)
        for x0, x1 in patches:
            mask |= (X >= x0) & (X < x1) & (Y >= -10) & (Y < 10)
        return np.full((H, w), 250, np.uint16), mask, rgb
    plate = (X >= -16) & (X < 16) & (Y >= -16) & (Y < 16)
    return np.where(plate, 250, 375).astype(np.uint16), plate, rgb


def _cam(x=0.0, y=0.0, z=0.0, off=(0, 0, 0)):
    T = np.eye(4)
    T[:3, 3] = np.array([x, y, z]) * V + np.asarray(off, np.float64)
    return T.astype(np.float32)


def build(key, make):
    """key -> (background, movable) volumes from `make(bounds, voxel, trunc)`: tsdfvis_ref.ColourVolume for the restatement,
    physics_utils.TsdfVolume on the GPU; both take the same frames through integrate_rgb."""
    if key[0] == "dy":
        off = np.asarray(OFFSETS[key[1]])
        bg = make(np.array([[-20, -12, 94], [11, 11, 98]]) * V + off, V, 4 * V)
        mv = make(np.array([[-10, -10, 62], [10, 10, 66]]) * V + off, V, 4 * V)
        for cn in DY_CAMS:
            z, plate, rgb = dy_frame(cn)
            mv.integrate_rgb(z, plate, rgb, K_DY, _cam(cn[0], cn[1], 0, off), 1)
            bg.integrate_rgb(z, ~plate, rgb, K_DY, _cam(cn[0], cn[1], 0, off), 1)
        return bg, mv
    if key[0] == "blocks":
        vols = []
        for _ in range(2):
            vol = make(np.array([[-36, -12, 62], [27, 12, 66]]) * V, V, 4 * V)
            for cn in ((0, 0), (0, 0), (0, 0)):
                z, mask, rgb = dy_frame(cn, patches=((-44, -36), (-6, 24)), w=80, cx=48)
                vol.integrate_rgb(z, mask, rgb, np.array([[64.0, 0, 48.0], [0, 64.0, 20.0], [0, 0, 1]]), _cam(), 1)
            vols.append(vol)
        return tuple(vols)
    if key[0] == "sphere":
        vols = []
        for obj, (bounds, voxel, trunc) in ((0, cases.bg_args()), (1, cases.mv_args())):
            vol = make(bounds + SPHERE_SHIFT, voxel, trunc)
            for x in cases.CAM_X:
                z, lab, rgb = cases.frame(x)
                T = cases.cam_pose(x)
                T[:3, 3] += SPHERE_SHIFT
                vol.integrate_rgb((z * 1000).astype(np.uint16), lab == obj, rgb, cases.K, T, cases.ERODE)
            vols.append(vol)
        return tuple(vols)
    if key[0] == "cases":
        return None                                                  # tsdfvis_cases' own volumes: see volumes()
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def volumes(key):
    if key[0] == "cases":
        return cases.ref_volumes(key[1])
    return build(key, ref.ColourVolume)


def _pose(t=(0, 0, 0), R=None, c=(0, 0, 64), off=(0, 0, 0), scale=1.0):
    """The plate's pose T(c) turned by R about the voxel corner c and moved by t (voxels)."""
    P = np.eye(4)
    P[:3, :3] = (np.eye(3) if R is None else np.asarray(R, np.float64)) * scale
    P[:3, 3] = (np.asarray(c, np.float64) + np.asarray(t, np.float64)) * V + np.asarray(off, np.float64)
    return P.astype(np.float32)


def _rot(axis, quarter):
    c, s = (1, 0, -1, 0)[quarter % 4], (0, 1, 0, -1)[quarter % 4]
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[a, a], R[a, b], R[b, a], R[b, b] = c, -s, s, c
    return R


O_DY = _pose()
DY_POSES = np.stack([_pose(), _pose((3, 0, 0)), _pose((0, -2, 5))] + [_pose((0, 0, 10), _rot(a, q)) for a in range(3) for q in (1, 3, 2)])
E_ACCEPT, E_REFUSE = f32(1 + 4.5e-6), f32(1 + 6e-6)


class Case:
    def __init__(self, vol_key, view, cam, o_now, poses, thr=3.0):
        self.vol_key, self.view, self.cam, self.o_now, self.thr = vol_key, view, np.asarray(cam, np.float32), np.asarray(o_now, np.float32), thr
        self.poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)


def _dy_view(near, w=W, h=H, fx=64.0, fy=64.0, cx=24.0, cy=20.0):
    return ref.View(w, h, fx, fy, cx, cy, near)


def _e12(off_name):
    off = OFFSETS[off_name]
    poses = [_pose(t, c=(0, 0, 0), scale=float(s)) for t in ((0, 0, 0), (3, 0, 0), (0, -2, 5)) for s in (E_ACCEPT, f32(2) - E_ACCEPT)]
    return Case(("dy", off_name), _dy_view(2 * V, fx=512.0, fy=512.0), _cam(-16, 0, -64, off), np.eye(4), poses)


THR_E3 = (0.5, 1.0, 2.0, float(np.nextafter(f32(2), f32(3))), float(np.nextafter(f32(3), f32(2))), 3.0, float(np.nextafter(f32(3), f32(4))))
_E8_VIEWS = {"1x1": (1, 1, 0.0, 0.0), "1x17": (1, 17, 0.0, 8.0), "17x1": (17, 1, 8.0, 0.0), "8x8": (8, 8, 4.0, 4.0), "9x9": (9, 9, 4.0, 4.0),
             "16x16": (16, 16, 8.0, 8.0), "17x17": (17, 17, 8.0, 8.0)}
E8_POSES = np.stack([_pose(), _pose((-49, -66, 0)), _pose((-6, 0, 0)), _pose((49, 0, 0)), _pose((0, 0, 10), _rot(2, 1))])
# on the 17 x 17 view: candidate 1's rectangle is the one pixel (0, 0); candidate 2's ends on column 15; candidate 3's starts on column 16
LONG = ref.View(9, 9, 4000.0, 4000.0, 4.0, 4.0)

# E4: the rim of the plate's shadow in the plane is an unobserved band beside the surface.  This camera meets it obliquely (found by
# a search over eyes and targets on the CPU): the interpolated hit point's cell has a corner under thr while sample s's cell is observed.
E4_CAM = cases._look(np.array([30.0, 0.3, 55.0]) * V, np.array([-17.0, 0.0, 96.0]) * V)
# E10: the twin sphere one fp32 ulp of the depth nearer along the optical axis and two ulps to the side.  A sweep of -6 .. 6 ulps along
# the axis alone moves every pixel's depth the same way (all win or all lose, by at most 7 ulps); the sideways part makes the movable
# volume win on one flank and lose on the other: 46 pixels won and 8 lost by <= 8 ulps, 15 exact ties.
_ULP = float(np.spacing(f32(0.2)))
E10_POSE = cases.O_NOW.copy()
E10_POSE[0, 3], E10_POSE[2, 3] = f32(float(cases.O_NOW[0, 3]) + 2 * _ULP), f32(float(cases.O_NOW[2, 3]) - _ULP)

CASES = {
    "E1_on_grid": Case(("dy", "0"), _dy_view(2 * V), _cam(), O_DY, DY_POSES),
    "E1_half_off": Case(("dy", "0"), _dy_view(2.5 * V), _cam(), O_DY, DY_POSES),
    "E1_origin_outside": Case(("dy", "0"), _dy_view(2 * V), _cam(20, 0, 0), O_DY, DY_POSES[:2]),
    "E2_on_surface": Case(("dy", "0"), _dy_view(2 * V), _cam(0, 0, 62), O_DY, np.stack([_pose(), _pose((0, 0, 1))])),
    "E2_inside": Case(("dy", "0"), _dy_view(2.5 * V), _cam(0, 0, 62), O_DY, np.stack([_pose(), _pose((0, 0, 1))])),
    "E4_fallback": Case(("dy", "0"), ref.View(24, 20, 64.0, 64.0, 12.0, 10.0), E4_CAM, O_DY, DY_POSES[:1]),
    "E5_half_colours": Case(("dy", "0"), _dy_view(2.5 * V), _cam(0.5, 0, 0), O_DY, DY_POSES[:3]),
    "E6_far": Case(("sphere",), cases.VIEWS["48x40"], _cam(off=SPHERE_SHIFT), cases.O_NOW + np.pad(SPHERE_SHIFT[:, None], ((0, 1), (3, 0))),
                   np.stack([cases.CANDIDATES[n] + np.pad(SPHERE_SHIFT[:, None], ((0, 1), (3, 0))).astype(np.float32) for n in ("rot_x", "rot_xyz", "rot_z", "near")])),
    "E7_blocks": Case(("blocks",), _dy_view(0.01), cases._look(np.array([-62.0, 3.0, 61.0]) * V, np.array([10.0, 3.0, 64.5]) * V), np.eye(4),
                      np.stack([_pose((0, 6, 0), c=(0, 0, 0)), _pose((0, 0, -2), c=(0, 0, 0))])),
    "E9_last_pair": Case(("cases", "plain"), LONG, _cam(0.058 / V, 0, -2.695 / V), cases.O_NOW, cases.poses(["off"])),
    "E9_one_voxel_more": Case(("cases", "plain"), LONG, _cam(0.058 / V, 0, -2.699 / V), cases.O_NOW, cases.poses(["off"])),
    "E9_inside_box": Case(("cases", "plain"), cases.VIEWS["45x37"], _cam(0.058 / V, 0, 0.289 / V), cases.O_NOW, cases.poses(["off", "behind"])),
    "E10_exact_tie": Case(("cases", "twins"), cases.VIEWS["45x37"], cases.CAM, cases.O_NOW, cases.poses(["front"])),
    "E10_near_tie": Case(("cases", "twins"), cases.VIEWS["45x37"], cases.CAM, cases.O_NOW, E10_POSE[None]),
    "E12_40m": _e12("40m"),
    "E12_2km": _e12("2km"),
}
for _n, (_w, _h, _cx, _cy) in _E8_VIEWS.items():
    CASES["E8_" + _n] = Case(("dy", "0"), ref.View(_w, _h, 24.0, 16.0, _cx, _cy, 2 * V), _cam(), O_DY, E8_POSES)
CASES["E8_pp_left"] = Case(("dy", "0"), ref.View(17, 17, 24.0, 16.0, -5.0, 8.0, 2 * V), _cam(-14, 0, 0), O_DY, E8_POSES[:3])
CASES["E8_pp_right"] = Case(("dy", "0"), ref.View(17, 17, 24.0, 16.0, 21.0, 8.0, 2 * V), _cam(14, 0, 0), O_DY, E8_POSES[:3])
CASES["E8_one_sample"] = Case(("dy", "0"), ref.View(17, 17, 24.0, 16.0, 8.0, 8.0, 3.0 - V / 2), _cam(0, 0, -690), O_DY, E8_POSES[:2])
CASES["E8_no_sample"] = Case(("dy", "0"), ref.View(17, 17, 24.0, 16.0, 8.0, 8.0, 3.0), _cam(0, 0, -690), O_DY, E8_POSES[:2])
for _i, _t in enumerate(THR_E3):
    CASES[f"E3_thr{_i}"] = Case(("cases", "band"), cases.VIEWS["48x40"], cases.CAM, cases.O_NOW, cases.poses(["off", "front"]), thr=_t)
E12_REFUSED = _pose((0, 0, 0), c=(0, 0, 0), scale=float(E_REFUSE))


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (frames, depth, facts) of the brute-force restatement: every sample of every pixel, no skip.  Computed once, never changed."""
    c = CASES[name]
    bg, mv = volumes(c.vol_key)
    facts = {}
    frames, depth, _ = ref.render(bg, mv, c.view, c.cam, c.o_now, c.poses, c.thr, facts=facts)
    frames.setflags(write=False), depth.setflags(write=False)
    return frames, depth, facts


@functools.lru_cache(maxsize=None)
def with_skips(name, wrong=(), skips=True, want_facts=True):
    """-> (frames, depth, facts) of the restatement with the GPU's skips restated and / or the wrong rules `wrong` (a tuple)."""
    c = CASES[name]
    bg, mv = volumes(c.vol_key)
    facts = {} if want_facts else None
    frames, depth, _ = ref.render(bg, mv, c.view, c.cam, c.o_now, c.poses, c.thr, facts=facts, wrong=wrong, skips=skips)
    return frames, depth, facts
