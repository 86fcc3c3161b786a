"""The physics pre-filter from the TSDF volumes on the GPU (tsdf.hip k_tsdf_touch_bits / k_tsdf_solid_*, sdfphys.hip) against the
numpy restatement of DESIGN.md section 2e (tests/sdfphys_ref.py): bits, points and verdicts must be IDENTICAL."""
import ctypes as C
import types

import numpy as np
import pytest

from dream2real_amd import _lib, physics_utils
from dream2real_amd.physics_utils import SdfPhysicsShapes, TsdfVolume, create_lazy_phys_mods
from tests import sdfphys_ref, tsdf_ref, tsdf_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
VOXEL = f32(0.002)
B0, NV = np.array([-2, -1, -1], np.int32), np.array([64, 48, 32], np.uint32)      # a grid of 64 x 48 x 32 voxels that starts at (-32, -16, -16)
LO = B0.astype(np.int64) * 16
RES = (3, 2, 2, 2, 1, 2)                                                          # 12 positions x 4 orientations


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def world(local):
    """Centre of the voxel with local index (x, y, z), as the rule places it: (float)g * voxel."""
    return (np.asarray(local, np.int64) + LO).astype(np.float32) * VOXEL


def pose_at(t, R=None):
    P = np.eye(4)
    if R is not None:
        P[:3, :3] = R
    P[:3, 3] = t
    return P


def rot(axis, a):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def gpu_check(ctx, words, pts, poses, valid_in, res, init, table_z, unsup=0.02, perturb=0.04, stability=True, regrasp=False, b0=B0, nv=NV):
    s = SdfPhysicsShapes(ctx, b0, nv, VOXEL, words, pts)
    try:
        return s.check(poses, valid_in, res, init, table_z, unsup, stability, regrasp, perturb)
    finally:
        s.close()


def both(ctx, words, pts, poses, valid_in, res, init, table_z, unsup=0.02, perturb=0.04, stability=True, regrasp=False):
    want, d = sdfphys_ref.check(B0, NV, VOXEL, words, pts, poses, valid_in, res, init, table_z, unsup, (0, 0, -1.0), perturb, stability, regrasp,
                                detail=True)
    got = gpu_check(ctx, words, pts, poses, valid_in, res, init, table_z, unsup, perturb, stability, regrasp)
    assert got.dtype == bool and (got == want).all(), np.nonzero(got != want)[0]
    return want, d


# ------------------------------------------------------------------------------------------------ synthetic fields
def table_scene():
    """A table (local x 8 .. 47, y 8 .. 39, z 4 .. 7) and a 5 x 5 x 5 block of points around its initial pose; twelve positions chosen
    so that every verdict occurs, four orientations of which the third repeats the first.  unsup_thresh 5 voxels, perturb 10."""
    touch = np.zeros((32, 48, 64), bool)
    touch[4:8, 8:40, 8:48] = True
    k = np.arange(5)
    zz, yy, xx = np.meshgrid(k, k, k, indexing="ij")
    corner = np.array([20, 20, 9])
    pts = world(np.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], 1) + corner)
    init = pose_at(world(corner + 2).astype(np.float64))
    corners = [(20, 20, 6), (20, 20, 9), (40, 20, 9), (10, 20, 9), (20, 32, 9), (20, 10, 9), (20, 20, 20), (52, 20, 1), (20, 20, 8), (56, 40, 20),
               (61, 20, 9), (20, 20, 12)]
    oris = [np.eye(3), rot((0, 0, 1), np.pi / 2), np.eye(3), rot((0, 0, 1), np.pi)]
    poses = np.stack([pose_at(world(np.array(c) + 2).astype(np.float64), R) for c in corners for R in oris])
    return sdfphys_ref.pack_bits(touch), pts, init, poses, float(world((0, 0, 6))[2])


def test_every_verdict_class_on_a_table(ctx):
    words, pts, init, poses, table_z = table_scene()
    valid_in = np.ones(len(poses), bool)
    valid_in[7] = False
    want, d = both(ctx, words, pts, poses, valid_in, RES, init, table_z, unsup=0.01, perturb=0.02)
    hit, below, om = d["hit"], d["below"], d["ori_mask"]
    live = om & valid_in
    assert (~om).sum() == 12 and not om[2] and om[0] and om[1] and om[3]                     # the duplicate orientation, at every position
    assert (live & hit[:, 0]).any()                                                          # collision
    assert (live & ~hit[:, 0] & below).any() and want[live & ~hit[:, 0] & below].all()       # below the table: valid
    assert (live & ~hit[:, 0] & ~below & ~hit[:, 1]).any()                                   # unsupported
    for q in range(2, 6):                                                                    # unstable, each probe the first to fail
        assert (live & ~hit[:, 0] & ~below & hit[:, 1] & hit[:, 2:q].all(1) & ~hit[:, q]).any(), q
    assert (live & ~hit[:, 0] & ~below & hit[:, 1:].all(1)).any()                            # valid
    assert want.any() and not want[~live].any()
    loose, _ = both(ctx, words, pts, poses, valid_in, RES, init, table_z, unsup=0.01, perturb=0.02, stability=False)
    assert loose.sum() > want.sum()
    grasp, dg = both(ctx, words, pts, poses, valid_in, RES, init, table_z, unsup=0.01, perturb=0.02, regrasp=True)
    assert dg["ori_mask"].sum() == 3 * 12 and (grasp == want).all()                          # rotations about z keep the object's z axis up
    tilted = poses.copy()
    tilted[:, :3, :3] = tilted[:, :3, :3] @ rot((1, 0, 0), np.pi / 2)[None]                   # the z axis now faces -y or is horizontal
    both(ctx, words, pts, tilted, valid_in, RES, init, table_z, unsup=0.01, perturb=0.02, regrasp=True)


@pytest.mark.parametrize("density", [0.0, 0.001, 0.05, 1.0])
def test_random_fields_and_point_counts(ctx, density):
    rng = np.random.default_rng(11)
    touch = rng.random((32, 48, 64)) < density
    words = sdfphys_ref.pack_bits(touch)
    centre = world((30, 24, 18)).astype(np.float64)
    init = pose_at(centre, rot((1, 2, 3), 0.3))
    oris = [rot((1, 0, 0), 0.0), rot((1, 1, 0), 0.9), rot((1, 0, 0), 0.0), rot((0, 1, 3), 2.1)]
    offs = rng.uniform(-0.03, 0.03, (12, 3))
    offs[:, 2] = rng.uniform(-0.01, 0.02, 12)
    poses = np.stack([pose_at(centre + o, R @ init[:3, :3]) for o in offs for R in oris])
    valid_in = rng.random(len(poses)) < 0.9
    verdicts = []
    for n in (1, 63, 64, 65, 257, 5000):
        pts = (centre + rng.uniform(-0.008, 0.008, (n, 3))).astype(np.float32)
        want, _ = both(ctx, words, pts, poses, valid_in, RES, init, float(centre[2]) - 0.004, unsup=0.006, perturb=0.012)
        verdicts.append(int(want.sum()))
    print(f"density {density}: valid poses per point count {verdicts}")
    if density in (0.0, 1.0):                                  # nothing to touch: only poses below the table height; everything touches: none
        assert all(v == verdicts[0] for v in verdicts) and (verdicts[0] > 0) == (density == 0.0)


FAR = (22, 10, 16)          # filler points fill 20 x 25 x 10 voxels from here: layers z 16 .. 25, while every bit sits at z 6 and probes lower by 4


def one_touch_case(q, where):
    """5 000 points, one of which (the `where`-th) lands on the field's one bit for probe q, under the identity transform.  For probe 5
    the verdict shows hit[5] only when probes 1 .. 4 hit too: four more bits, and four points that land on them under exactly
    one probe each.  unsup_thresh 4 voxels, perturb 8 voxels: t1 = (0, 0, -4), t2 .. t5 = (+-8, 0, -4), (0, +-8, -4) voxels."""
    shifts = np.array([(0, 0, 0), (0, 0, -4), (8, 0, -4), (-8, 0, -4), (0, 8, -4), (0, -8, -4)])
    bits = {1: (12, 12, 6), 2: (30, 12, 6), 3: (12, 30, 6), 4: (30, 30, 6), 5: (50, 12, 6), 0: (50, 30, 6)}
    touch = np.zeros((32, 48, 64), bool)
    used = [q] if q == 0 else [1, 2, 3, 4, 5]
    for p in used:
        touch[bits[p][2], bits[p][1], bits[p][0]] = True
    k = np.arange(4995 if q else 4999)
    filler = world(np.stack([FAR[0] + k % 20, FAR[1] + (k // 20) % 25, FAR[2] + k // 500], 1))
    special = world(np.array(bits[q]) - shifts[q])[None]
    support = np.stack([world(np.array(bits[p]) - shifts[p]) for p in (1, 2, 3, 4)]) if q else np.zeros((0, 3), np.float32)
    at = {"first": 0, "last": len(filler), "middle": len(filler) // 2, "lane63": 63, "lane64": 64}[where]
    if q == 0:
        pts = np.concatenate([filler[:at], special, filler[at:]])
        without = filler
    elif where == "first":
        pts, without = np.concatenate([special, support, filler]), np.concatenate([support, filler])
    else:
        pts, without = np.concatenate([filler[:at], support, special, filler[at:]]), np.concatenate([filler[:at], support, filler[at:]])
    return sdfphys_ref.pack_bits(touch), pts.astype(np.float32), without.astype(np.float32)


@pytest.mark.parametrize("q", [0, 5])
@pytest.mark.parametrize("where", ["first", "middle", "last", "lane63", "lane64"])
def test_one_point_in_five_thousand_decides(ctx, q, where):
    """Catches vote and stride errors: the answer hangs on one lane of one step.  Probe 0 under a table height above everything (valid
    exactly when nothing collides), probe 5 above the table (valid exactly when the last stability probe finds its bit)."""
    words, pts, without = one_touch_case(q, where)
    assert len(pts) == 5000 and len(without) == 5000 - 1
    init = np.eye(4)
    poses = np.stack([np.eye(4)] * 2)
    for p, expect in ((pts, q == 5), (without, q == 0)):
        want, d = both(ctx, words, p, poses, np.ones(2, bool), (2, 1, 1, 1, 1, 1), init, 1e9 if q == 0 else -1.0, unsup=0.008, perturb=0.016)
        assert want.tolist() == [expect, expect]
        assert d["hit"][0].tolist() == ([p is pts, False, False, False, False, False] if q == 0 else [False, True, True, True, True, p is pts])


def test_points_that_leave_the_grid_and_poses_that_are_not_finite(ctx):
    """Every bit set, one point, the table height above everything: a pose is valid exactly when the point touches nothing, that is
    when it has left the grid.  Through each of the six faces by one voxel, far away, and not a number."""
    words = sdfphys_ref.pack_bits(np.ones((32, 48, 64), bool))
    pts = world((0, 0, 0))[None]
    init = pose_at(world((0, 0, 0)).astype(np.float64))
    last = NV.astype(np.int64) - 1
    cells, expect = [], []
    for a in range(3):
        for inside, v in ((True, 0), (False, -1), (True, last[a]), (False, last[a] + 1)):
            c = np.array([5, 6, 7])
            c[a] = v
            cells.append(c)
            expect.append(not inside)
    poses = [pose_at(world(c).astype(np.float64)) for c in cells]
    for t in ((1e6, 0, 0), (0, -1e6, 0), (0, 0, 1e6), (1e30, 1e30, -1e30)):
        poses.append(pose_at(np.array(t)))
        expect.append(True)
    nan_t = pose_at(world((5, 6, 7)).astype(np.float64))
    nan_t[0, 3] = np.nan                                        # the point is nowhere: no collision, and z is under the table height
    nan_r = pose_at(world((5, 6, 7)).astype(np.float64))
    nan_r[1, 1] = np.nan
    nan_z = pose_at(world((5, 6, 7)).astype(np.float64))
    nan_z[2, 3] = np.nan                                        # not below the table, and nothing under it: unsupported
    inf_t = pose_at(np.array([np.inf, 0, 0]))
    poses += [nan_t, nan_r, nan_z, inf_t]
    expect += [True, True, False, True]
    poses = np.stack(poses)
    want, _ = both(ctx, words, pts, poses, np.ones(len(poses), bool), (len(poses), 1, 1, 1, 1, 1), init, 1e9)
    assert want.tolist() == expect
    many = np.concatenate([pts, world((3, 3, 3))[None] + np.array([[1e6, 0, 0], [np.nan, 0, 0], [0, 0, -np.inf]], np.float32)]).astype(np.float32)
    both(ctx, words, many, poses, np.ones(len(poses), bool), (len(poses), 1, 1, 1, 1, 1), init, 1e9)


def test_nothing_valid_stays_so_and_two_runs_agree(ctx):
    words, pts, init, poses, table_z = table_scene()
    s = SdfPhysicsShapes(ctx, B0, NV, VOXEL, words, pts)
    a = s.check(poses, np.ones(len(poses), bool), RES, init, table_z, 0.01, True, False, 0.02)
    b = s.check(poses, np.ones(len(poses), bool), RES, init, table_z, 0.01, True, False, 0.02, margin=0.5)       # margin is ignored
    none = s.check(poses, np.zeros(len(poses), bool), RES, init, table_z, 0.01, True, False, 0.02)
    up, kernel, down = s.timing()
    s.close()
    assert (a == b).all() and a.any() and not none.any() and min(up, kernel, down) >= 0.0


def test_two_static_grids_are_ored(ctx):
    words, pts, init, poses, table_z = table_scene()
    left, right = words.copy(), words.copy()
    left[:, 24:, :] = 0                      # the table's rows y < 24 in one grid, the rest in the other
    right[:, :24, :] = 0
    want = sdfphys_ref.check(B0, NV, VOXEL, words, pts, poses, np.ones(len(poses), bool), RES, init, table_z, 0.01, (0, 0, -1.0), 0.02)
    got = gpu_check(ctx, np.stack([left, right]), pts, poses, np.ones(len(poses), bool), RES, init, table_z, 0.01, 0.02)
    only = gpu_check(ctx, left, pts, poses, np.ones(len(poses), bool), RES, init, table_z, 0.01, 0.02)
    assert (got == want).all() and (only != want).any()


def test_refusals(ctx, tmp_path):
    words, pts, init, poses, table_z = table_scene()
    lib, h = ctx.lib, C.c_void_p()
    b0, nv = np.ascontiguousarray(B0), np.ascontiguousarray(NV)
    args = lambda **kw: [kw.get(k, d) for k, d in (("ctx", ctx.h), ("b0", _lib.ptr(b0)), ("nv", _lib.ptr(nv)), ("voxel", C.c_float(0.002)),
                                                   ("words", _lib.ptr(words)), ("n", C.c_uint32(1)), ("pts", _lib.ptr(pts)),
                                                   ("np", C.c_uint32(len(pts))), ("out", C.byref(h)))]
    for kw in (dict(b0=None), dict(nv=None), dict(words=None), dict(pts=None), dict(out=None), dict(np=C.c_uint32(0)), dict(n=C.c_uint32(0)),
               dict(voxel=C.c_float(0.0)), dict(nv=_lib.ptr(np.array([2048, 2048, 1024], np.uint32))),           # 2^32 voxels
               dict(nv=_lib.ptr(np.array([0, 48, 32], np.uint32))), dict(b0=_lib.ptr(np.array([1 << 20, 0, 0], np.int32)))):
        assert lib.d2r_sdfphys_create(*args(**kw)) == -1, kw
        assert not h.value and lib.d2r_last_error(ctx.h)
    with pytest.raises(_lib.D2RError, match="2\\^31 voxels"):
        ctx.check(lib.d2r_sdfphys_create(*args(nv=_lib.ptr(np.array([2048, 2048, 1024], np.uint32)))))
    with pytest.raises(ValueError, match="do not fit the grid"):
        SdfPhysicsShapes(ctx, B0, NV, VOXEL, words[:, :, :1], pts)
    s = SdfPhysicsShapes(ctx, B0, NV, VOXEL, words, pts)
    valid = np.ones(len(poses), np.uint8)
    P = np.ascontiguousarray(poses.reshape(-1, 16), np.float32)
    prm = physics_utils._phys_params(RES, init, table_z, 0.01, 0.02, True, False, 0.0)
    for a in ((None, s.h, C.byref(prm), _lib.ptr(P), 48, _lib.ptr(valid)), (ctx.h, None, C.byref(prm), _lib.ptr(P), 48, _lib.ptr(valid)),
              (ctx.h, s.h, None, _lib.ptr(P), 48, _lib.ptr(valid)), (ctx.h, s.h, C.byref(prm), None, 48, _lib.ptr(valid)),
              (ctx.h, s.h, C.byref(prm), _lib.ptr(P), 48, None), (ctx.h, s.h, C.byref(prm), _lib.ptr(P), 47, _lib.ptr(valid))):
        assert lib.d2r_sdfphys_check(*a) == -1
    with pytest.raises(_lib.D2RError, match="does not match sample_res"):
        s.check(poses[:47], np.ones(47, bool), RES, init, table_z)
    sheared = init.copy()
    sheared[0, 1] = 0.5
    with pytest.raises(_lib.D2RError, match="rigid"):
        s.check(poses, np.ones(48, bool), RES, sheared, table_z)
    assert s.check(poses, np.ones(48, bool), RES, init, table_z, 0.01, True, False, 0.02).any()           # the handle still works
    s.close()
    # a volume nothing was fused into has no points ("seen in no frame") and no bits
    vol = TsdfVolume(ctx, tsdf_scene.BOUNDS)
    assert not vol.touch_bits().any()
    with pytest.raises(_lib.D2RError, match="seen in no frame"):
        vol.solid_points()
    vol.close()


# ------------------------------------------------------------------------------------------------ from RGB-D frames
def fuse_gpu(ctx, scene, obj):
    vol = TsdfVolume(ctx, scene["bounds"])
    for f in range(len(scene["depths"])):
        u16 = (scene["depths"][f] * 1000).astype(np.uint16)
        vol.integrate(u16, scene["masks"][f] == obj, scene["intrinsics"], scene["cam_poses"][f], 20 if obj == 0 else 8)
    return vol


def test_bits_and_points_of_the_fused_volumes_equal_the_restatement(ctx):
    scene = tsdf_scene.make_scene()                                  # sphere on slab, 12 views of 320 x 240
    for obj in (0, 1):
        ref = tsdf_ref.fuse(scene["depths"], scene["cam_poses"], scene["intrinsics"], scene["masks"], obj, scene["bounds"])[0]
        vol = fuse_gpu(ctx, scene, obj)
        b0, nv, voxel, trunc = vol.grid()
        rb0, rnv, rvoxel, rtrunc = sdfphys_ref.grid_of(ref)
        assert (b0 == rb0).all() and (nv == rnv).all() and voxel == rvoxel and trunc == rtrunc
        words, pts = vol.touch_bits(), vol.solid_points()
        want_w, want_p = sdfphys_ref.touch_words(ref), sdfphys_ref.solid_points(ref)
        print(f"object {obj}: grid {nv.tolist()} from block {b0.tolist()}, {int(sdfphys_ref.unpack_bits(want_w, int(nv[0])).sum())} touch bits, "
              f"{len(want_p)} solid points")
        assert words.shape == want_w.shape and (words == want_w).all() and want_w.any()
        assert pts.shape == want_p.shape and (pts.view(np.uint32) == want_p.view(np.uint32)).all()
        for thr, contact in ((1.0, 0.0), (6.0, 0.01)):               # other thresholds than the defaults
            assert (vol.touch_bits(thr, contact) == sdfphys_ref.touch_words(ref, thr, contact)).all()
            assert (vol.solid_points(thr).view(np.uint32) == sdfphys_ref.solid_points(ref, thr).view(np.uint32)).all()
        vol.close()


E2E_XY = (-0.04, -0.02, 0.0, 0.02, 0.04)
E2E_Z = (-0.01, 0.008, 0.04)
E2E_SPOT = (3, 1)            # x = +0.02, y = -0.02: on the slab the cameras saw, beside where the sphere stood


def test_end_to_end_from_frames_to_the_pose_filter(ctx, tmp_path):
    """RGB-D frames and masks -> create_lazy_phys_mods(phys_backend="tsdf") -> create_unsupcol_check, no mesh and no hulls on the way.
    A 12 mm sphere on the slab (no mislabelled patch: its voxels would belong to the object and sit inside the slab), 5 x 5 x 3
    positions around the initial pose x 2 orientations.

    The three labelled poses were found with the restatement on the CPU, not assumed: on the column x = +0.02, y = -0.02 the
    reference's verdict by height above the initial pose, in 2 mm steps from -16 mm, reads collide x 8 (up to -2 mm), valid x 10 (0 ..
    +18 mm), unsupported from +20 mm; so sunk 10 mm, set down 8 mm up and hovering 40 mm up each hold with at least three voxels
    to spare, which the test checks again by moving each three voxels along every axis.  At the initial spot itself every
    height is unsupported: the slab under the sphere was never seen, and unobserved voxels never touch."""
    import torch
    scene = tsdf_scene.make_scene(sphere_r=0.012, speckle_r=0.0)
    out = str(tmp_path / "phys")
    scene_model = types.SimpleNamespace(depths=torch.from_numpy(scene["depths"]), opt_cam_poses=torch.from_numpy(scene["cam_poses"]),
                                        intrinsics=scene["intrinsics"], masks=torch.from_numpy(scene["masks"].astype(np.int64)) * 3,
                                        scene_centre=torch.tensor([0.0, 0.0, -0.05]))
    movable = types.SimpleNamespace(mask_idx=3)

    def never(*a):
        raise AssertionError("convexify must not run")

    (bg_path, mov_path), (bg_pose, mov_pose) = create_lazy_phys_mods(scene_model, movable, scene["bounds"], out, ctx=ctx, convexify=never,
                                                                    phys_backend="tsdf")
    assert bg_path.endswith("sdf_0.npz") and mov_path.endswith("sdf_1.npz")
    refs = [tsdf_ref.fuse(scene["depths"], scene["cam_poses"], scene["intrinsics"], scene["masks"], obj, scene["bounds"]) for obj in (0, 1)]
    b0, nv, voxel, _ = sdfphys_ref.grid_of(refs[0][0])
    words, pts = sdfphys_ref.touch_words(refs[0][0]), sdfphys_ref.solid_points(refs[1][0])
    got_bg, got_mov = physics_utils.load_sdf_model(bg_path), physics_utils.load_sdf_model(mov_path)
    assert (got_bg["words"] == words).all() and (got_mov["points"].view(np.uint32) == pts.view(np.uint32)).all()
    movable.pose, movable.phys_model = mov_pose, mov_path
    task = types.SimpleNamespace(movable_obj=movable, task_bground_obj=types.SimpleNamespace(phys_model=bg_path), scene_model=scene_model)
    init = mov_pose.numpy().astype(np.float64)
    Rz = rot((0, 0, 1), np.pi / 2)

    def at(dx, dy, dz, R):
        P = init.copy()
        P[:3, :3] = R
        P[:3, 3] += (dx, dy, dz)
        return P

    poses = np.stack([at(dx, dy, dz, R) for dx in E2E_XY for dy in E2E_XY for dz in E2E_Z for R in (np.eye(3), Rz)])
    res = [5, 5, 3, 1, 1, 2]
    check, static, mov = physics_utils.create_unsupcol_check(ctx, task, res, embodied=False)
    assert static == [bg_path] and mov == [mov_path] and isinstance(check.shapes, SdfPhysicsShapes)
    got = check(torch.from_numpy(poses), task, torch.ones(len(poses), dtype=torch.bool)).numpy()
    want, d = sdfphys_ref.check(b0, nv, voxel, words, pts, poses, np.ones(len(poses), bool), res, init, -0.05, detail=True)
    print("valid by height (rows x, columns y):", [got.reshape(5, 5, 3, 2)[:, :, k, 0].astype(int).tolist() for k in range(3)])
    assert (got == want).all()
    v, hit = want.reshape(5, 5, 3, 2), d["hit"].reshape(5, 5, 3, 2, 6)
    ix, iy = E2E_SPOT
    for o in (0, 1):
        assert hit[ix, iy, 0, o, 0] and not v[ix, iy, 0, o]                                       # sunk 1 cm: colliding
        assert v[ix, iy, 1, o] and not hit[ix, iy, 1, o, 0] and hit[ix, iy, 1, o, 1:].all()      # set down on the seen slab: valid
        assert not hit[ix, iy, 2, o].any() and not v[ix, iy, 2, o]                                # hovering 4 cm up: unsupported
        assert not hit[2, 2, :, o, 1].any() and not v[2, 2, :, o].any()                           # the unseen slab under the initial spot
    # three voxels to spare: the labelled verdicts and their reasons hold three voxels away along every axis (restatement, CPU)
    shifts = [s * 0.006 * np.eye(3)[a] for a in range(3) for s in (-1, 1)]
    near = np.stack([at(E2E_XY[ix] + s[0], E2E_XY[iy] + s[1], dz + s[2], np.eye(3)) for dz in E2E_Z for s in shifts])
    nv_, nd = sdfphys_ref.check(b0, nv, voxel, words, pts, near, np.ones(len(near), bool), [len(near), 1, 1, 1, 1, 1], init, -0.05, detail=True)
    nh = nd["hit"].reshape(3, 6, 6)
    assert nh[0, :, 0].all() and not nh[1, :, 0].any() and nh[1, :, 1:].all() and nv_.reshape(3, 6)[1].all() and not nh[2].any()
    check.shapes.close()
