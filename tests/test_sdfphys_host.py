"""Physics pre-filter from the TSDF volumes, CPU side: the numpy restatement of DESIGN.md section 2e (tests/sdfphys_ref.py) against a
brute-force triple loop and against verdicts written out by hand on a table with edges, and the host plumbing of the product
(sdf_{id}.npz, phys_backend, the dispatch of create_unsupcol_check) with the GPU volume replaced by the TSDF restatement."""
import ctypes
import os
import shutil
import types

import numpy as np
import pytest

from dream2real_amd import _lib, physics_utils
from dream2real_amd.physics_utils import SdfPhysicsShapes, create_lazy_phys_mods, get_phys_models      # the feature: absent before it
from tests import sdfphys_ref, tsdf_ref, tsdf_scene

f32 = np.float32
VOXEL = f32(0.002)


def pose_at(t, R=None):
    P = np.eye(4)
    if R is not None:
        P[:3, :3] = R
    P[:3, 3] = t
    return P


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


# ------------------------------------------------------------------------------------------------ the restatement itself
def brute_force(b0, nv, voxel, touch, points, poses, valid_in, sample_res, init_pose, table_z, unsup, gravity, perturb, stability):
    """The rule, one scalar at a time."""
    oris = sample_res[3] * sample_res[4] * sample_res[5]
    omask = sdfphys_ref.orientation_mask(poses, valid_in, oris, False)
    inv = sdfphys_ref.rigid_inverse(init_pose)
    out = np.zeros(len(poses), bool)
    for n, pose in enumerate(np.asarray(poses, np.float32)):
        if not valid_in[n] or not omask[n % oris]:
            continue
        M = pose.astype(np.float64)
        T = np.array([[((M[i, 0] * inv[0, j] + M[i, 1] * inv[1, j]) + M[i, 2] * inv[2, j]) + M[i, 3] * inv[3, j] for j in range(4)]
                      for i in range(3)]).astype(np.float32)
        t0 = T[:, 3]
        t1 = np.array([t0[k] + f32(unsup) * f32(gravity[k]) for k in range(3)], np.float32)
        p = f32(perturb)
        probes = [t0, t1, t1 + np.array([p, 0, 0], np.float32), t1 + np.array([-p, 0, 0], np.float32),
                  t1 + np.array([0, p, 0], np.float32), t1 + np.array([0, -p, 0], np.float32)]
        hit = [False] * 6
        for q, t in enumerate(probes):
            for (x, y, z) in np.asarray(points, np.float32):
                g = []
                for a in range(3):
                    c = ((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + t[a]
                    g.append(int(np.floor(c / f32(voxel) + f32(0.5))) - 16 * int(b0[a]))
                if all(0 <= g[a] < int(nv[a]) for a in range(3)) and touch[g[2], g[1], g[0]]:
                    hit[q] = True
                    break
        if hit[0]:
            continue
        if pose[2, 3] < f32(table_z):
            out[n] = True
            continue
        if not hit[1]:
            continue
        out[n] = all(hit[2:]) if stability else True
    return out


def test_restatement_equals_a_brute_force_triple_loop():
    rng = np.random.default_rng(5)
    b0, nv = np.array([-1, 0, -1], np.int32), np.array([40, 24, 20], np.uint32)          # nx no multiple of 32: a row's last word is partial
    touch = rng.random((20, 24, 40)) < 0.04
    words = sdfphys_ref.pack_bits(touch)
    assert words.shape == (20, 24, 2) and (sdfphys_ref.unpack_bits(words, 40) == touch).all()
    pts = (rng.integers(0, 8, (30, 3)) + np.array([-10, 6, -10])).astype(np.float32) * VOXEL
    init = pose_at(pts.mean(0).astype(np.float64))
    sample_res = (3, 2, 2, 2, 1, 1)
    poses = []
    for ix in range(3):
        for iy in range(2):
            for iz in range(2):
                for a in (0.0, 0.7):
                    poses.append(pose_at(init[:3, 3] + np.array([0.012 * ix - 0.004, 0.01 * iy, 0.008 * iz - 0.002]), rot_z(a)))
    poses = np.stack(poses)
    valid_in = np.ones(len(poses), bool)
    valid_in[5] = False
    for stability in (True, False):
        for table_z in (-1.0, float(init[2, 3]) + 0.003):
            got, d = sdfphys_ref.check(b0, nv, VOXEL, words, pts, poses, valid_in, sample_res, init, table_z, 0.006, (0, 0, -1.0), 0.008,
                                       stability, detail=True)
            want = brute_force(b0, nv, VOXEL, touch, pts, poses, valid_in, sample_res, init, table_z, 0.006, (0, 0, -1.0), 0.008, stability)
            assert (got == want).all()
            assert d["hit"].any(0).all() and not d["hit"].all()              # every probe hits somewhere, none everywhere
    assert got.any() and not got.all()
    two = sdfphys_ref.check(b0, nv, VOXEL, np.stack([words & np.uint32(0x0f0f0f0f), words & np.uint32(0xf0f0f0f0)]), pts, poses, valid_in,
                            sample_res, init, -1.0, 0.006, (0, 0, -1.0), 0.008, False)
    assert (two == got).all()                                                # grids are ORed


# ------------------------------------------------------------------------------------------------ verdicts written out by hand
# Grid 128 x 64 x 64 voxels of 2 mm from the origin.  The table: bits set for x in 24 .. 63, y in 8 .. 55, z in 10 .. 15 (its top
# layer is z = 15).  The object: the 5 x 5 x 5 voxel centres from voxel (0, 0, 0), initial pose the identity, so a pose's translation
# (X, Y, B) voxels puts it at x X .. X + 4, y Y .. Y + 4, z B .. B + 4.  unsup_thresh 10 voxels, perturb 20 voxels, table_z at voxel 10.
TABLE = dict(x=(24, 64), y=(8, 56), z=(10, 16))
HAND = [  # (X, Y, B), hit[0..5], valid, why
    ((41, 30, 14), (1, 0, 0, 0, 0, 0), False, "collide: z 14 .. 18 reaches the top layer 15 (lowered, z 4 .. 8 is under the table's layers 10 .. 15)"),
    ((41, 30, 18), (0, 1, 1, 1, 1, 1), True, "valid: lowered to z 8 .. 12; x 61 .. 65, 21 .. 25 and y 50 .. 54, 10 .. 14 all still over the table"),
    ((50, 30, 18), (0, 1, 0, 1, 1, 1), False, "unstable, +x first: x 70 .. 74 is past the edge at 64"),
    ((30, 30, 18), (0, 1, 1, 0, 1, 1), False, "unstable, -x first: x 10 .. 14 is before the edge at 24"),
    ((41, 40, 18), (0, 1, 1, 1, 0, 1), False, "unstable, +y first: y 60 .. 64 is past the edge at 56 (and 64 leaves the grid)"),
    ((41, 20, 18), (0, 1, 1, 1, 1, 0), False, "unstable, -y first: y 0 .. 4 is before the edge at 8"),
    ((41, 30, 30), (0, 0, 0, 0, 0, 0), False, "unsupported: lowered to z 20 .. 24, above the top layer"),
    ((80, 30, 5), (0, 0, 0, 0, 0, 0), True, "below the table height and beside the table: valid whatever lies under it"),
    ((62, 30, 18), (0, 1, 0, 1, 1, 1), False, "hanging over the edge: supported by x 62, 63, but +x finds nothing"),
    ((41, 30, 16), (0, 1, 1, 1, 1, 1), True, "resting right on the top layer: z 16 .. 20 does not reach 15"),
]


def hand_table():
    touch = np.zeros((64, 64, 128), bool)
    touch[slice(*TABLE["z"]), slice(*TABLE["y"]), slice(*TABLE["x"])] = True
    k = np.arange(5)
    zz, yy, xx = np.meshgrid(k, k, k, indexing="ij")
    pts = np.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], 1).astype(np.float32) * VOXEL
    poses = np.stack([pose_at(np.array(t, np.float64) * 0.002) for t, _, _, _ in HAND])
    return np.zeros(3, np.int32), np.array([128, 64, 64], np.uint32), touch, pts, poses


def test_table_with_edges_hand_written_verdicts():
    b0, nv, touch, pts, poses = hand_table()
    valid, d = sdfphys_ref.check(b0, nv, VOXEL, sdfphys_ref.pack_bits(touch), pts, poses, np.ones(len(poses), bool), (len(poses), 1, 1, 1, 1, 1),
                                 np.eye(4), table_z=0.02, unsup_thresh=0.02, perturb=0.04, stability_check=True, detail=True)
    for k, (t, hit, ok, why) in enumerate(HAND):
        assert tuple(int(h) for h in d["hit"][k]) == hit, (t, why, d["hit"][k])
        assert bool(valid[k]) == ok, (t, why)
    loose = sdfphys_ref.check(b0, nv, VOXEL, sdfphys_ref.pack_bits(touch), pts, poses, np.ones(len(poses), bool), (len(poses), 1, 1, 1, 1, 1),
                              np.eye(4), table_z=0.02, unsup_thresh=0.02, perturb=0.04, stability_check=False)
    assert loose.tolist() == [not h[0] and (t[2] < 10 or bool(h[1])) for t, h, _, _ in HAND]          # without the stability probes


# ------------------------------------------------------------------------------------------------ host plumbing of the product
class RestatedVolume:
    """Stands where physics_utils.TsdfVolume stands, on the CPU: the fused tsdf_ref.Volume of the object the frames' erosion
    kernel names (20: background, 8: the object), handed out instead of being integrated again."""
    fused = None

    def __init__(self, ctx, bounds):
        self.vol, self.frames = None, 0

    def integrate(self, depth_u16, mask, intrinsics, cam_pose, erode_k):
        self.vol = RestatedVolume.fused[0 if erode_k == 20 else 1][0]
        self.frames += 1

    def extract(self, weight_threshold, crop, cluster_keep):
        v, t = self.vol.marching_cubes(weight_threshold)
        m = tsdf_ref.clean(v, t, crop, cluster_keep)
        return dict(vertices=m["vertices"], triangles=m["triangles"].astype(np.uint32), clusters=m["clusters"], keep=m["keep"], centre=m["centre"])

    def grid(self):
        return sdfphys_ref.grid_of(self.vol)

    def touch_bits(self, weight_threshold, contact):
        return sdfphys_ref.touch_words(self.vol, weight_threshold, contact)

    def solid_points(self, weight_threshold):
        return sdfphys_ref.solid_points(self.vol, weight_threshold)

    def close(self):
        pass


@pytest.fixture(scope="module")
def scene():
    s = tsdf_scene.make_scene(n_views=4, sphere_r=0.012, speckle_r=0.0)
    s["bounds"] = np.array([[-0.04, -0.04, -0.02], [0.04, 0.04, 0.04]])
    return s


@pytest.fixture()
def restated(scene, monkeypatch):
    if RestatedVolume.fused is None:
        RestatedVolume.fused = {obj: tsdf_ref.fuse(scene["depths"], scene["cam_poses"], scene["intrinsics"], scene["masks"], obj, scene["bounds"])
                                for obj in (0, 1)}
    monkeypatch.setattr(physics_utils, "TsdfVolume", RestatedVolume)
    return RestatedVolume.fused


def copy_mesh(concave_path, convex_path, obj_id):
    shutil.copyfile(concave_path, convex_path)


def run_models(scene, out, **kw):
    return get_phys_models(scene["depths"], scene["cam_poses"], scene["intrinsics"], scene["masks"], 2, scene["bounds"], save_dir=str(out),
                           use_cache=False, use_phys_tsdf=True, ctx=object(), **kw)


def files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_hulls_backend_is_todays_path_byte_for_byte(scene, restated, tmp_path):
    a, pa = run_models(scene, tmp_path / "a", convexify=copy_mesh)
    b, pb = run_models(scene, tmp_path / "b", convexify=copy_mesh, phys_backend="hulls")
    fa, fb = files(tmp_path / "a"), files(tmp_path / "b")
    assert sorted(fa) == ["init_pose_0.txt", "init_pose_1.txt", "mesh_0.obj", "mesh_1.obj", "mesh_concave_0.obj", "mesh_concave_1.obj"]
    assert fa == fb and [os.path.basename(p) for p in a] == [os.path.basename(p) for p in b] == ["mesh_0.obj", "mesh_1.obj"]
    assert all((x.numpy() == y.numpy()).all() for x, y in zip(pa, pb))
    with pytest.raises(ValueError, match="phys_backend"):
        run_models(scene, tmp_path / "c", convexify=copy_mesh, phys_backend="vhacd")
    assert not os.path.exists(tmp_path / "c")


def test_tsdf_backend_writes_the_field_files_and_the_cache_finds_them(scene, restated, tmp_path):
    def never(*a):
        raise AssertionError("convexify must not run with phys_backend='tsdf'")

    hulls, _ = run_models(scene, tmp_path / "h", convexify=copy_mesh)
    paths, poses = run_models(scene, tmp_path / "t", convexify=never, phys_backend="tsdf")
    assert paths == [os.path.join(str(tmp_path / "t"), f"sdf_{k}.npz") for k in (0, 1)]
    fh, ft = files(tmp_path / "h"), files(tmp_path / "t")
    assert sorted(ft) == ["init_pose_0.txt", "init_pose_1.txt", "mesh_concave_0.obj", "mesh_concave_1.obj", "sdf_0.npz", "sdf_1.npz"]
    for n in ("init_pose_0.txt", "init_pose_1.txt", "mesh_concave_0.obj", "mesh_concave_1.obj"):
        assert ft[n] == fh[n], n
    for k in (0, 1):                                                         # the round trip through the file
        vol = restated[k][0]
        m = physics_utils.load_sdf_model(paths[k])
        b0, nv, voxel, trunc = sdfphys_ref.grid_of(vol)
        assert (m["b0"] == b0).all() and (m["nv"] == nv).all() and m["voxel"] == voxel and m["trunc"] == trunc
        assert m["b0"].dtype == np.int32 and m["nv"].dtype == np.uint32 and m["words"].dtype == np.uint32 and m["points"].dtype == np.float32
        assert m["weight_threshold"] == f32(3.0) and m["contact"] == f32(0.002)
        assert (m["words"] == sdfphys_ref.touch_words(vol)).all() and m["words"].any()
        assert m["points"].shape[0] > 100 and (m["points"].view(np.uint32) == sdfphys_ref.solid_points(vol).view(np.uint32)).all()
    cached, cposes = get_phys_models(None, None, None, None, 2, None, save_dir=str(tmp_path / "t"), use_cache=True, phys_backend="tsdf")
    assert cached == paths and all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(cposes, poses))
    scene_model = types.SimpleNamespace(depths=scene["depths"], opt_cam_poses=scene["cam_poses"], intrinsics=scene["intrinsics"],
                                        masks=scene["masks"].astype(np.int64) * 3)
    lazy, _ = create_lazy_phys_mods(scene_model, types.SimpleNamespace(mask_idx=3), scene["bounds"], str(tmp_path / "t"), use_cache=True,
                                    phys_backend="tsdf")
    assert lazy == paths
    with pytest.raises(ValueError, match="phys_backend"):
        create_lazy_phys_mods(scene_model, types.SimpleNamespace(mask_idx=3), scene["bounds"], str(tmp_path / "t"), use_cache=True, phys_backend="")


class RestatedShapes:
    """Stands where SdfPhysicsShapes stands: the same files, checked by the restatement."""

    def __init__(self, ctx, b0, nv, voxel, words, points):
        self.args = (b0, nv, voxel, words, points)

    from_files = classmethod(SdfPhysicsShapes.from_files.__func__)

    def check(self, pose_batch, valid_so_far, sample_res, init_pose, table_z, unsup_thresh=0.02, stability_check=True, disallow_regrasp=False,
              perturb=0.04, margin=0.0):
        return sdfphys_ref.check(*self.args, pose_batch, valid_so_far, sample_res, init_pose, table_z, unsup_thresh, (0, 0, -1.0), perturb,
                                 stability_check, disallow_regrasp)


def test_create_unsupcol_check_dispatches_on_what_the_objects_carry(monkeypatch, tmp_path):
    import torch
    b0, nv, touch, pts, poses = hand_table()
    grid = (b0, nv, VOXEL, f32(0.016))
    half = touch.copy()
    half[:, :, 44:] = False
    rest = touch & ~half
    for name, t in (("sdf_0.npz", half), ("sdf_2.npz", rest)):
        physics_utils.save_sdf_model(str(tmp_path / name), grid, 3.0, 0.002, sdfphys_ref.pack_bits(t), np.zeros((0, 3), np.float32))
    physics_utils.save_sdf_model(str(tmp_path / "sdf_1.npz"), grid, 3.0, 0.002, sdfphys_ref.pack_bits(np.zeros_like(touch)), pts)
    monkeypatch.setattr(physics_utils, "SdfPhysicsShapes", RestatedShapes)
    objs = [types.SimpleNamespace(phys_model=str(tmp_path / f"sdf_{k}.npz")) for k in range(3)]
    objs[1].pose = torch.eye(4)
    scene_model = types.SimpleNamespace(objs=objs, scene_centre=torch.tensor([0.0, 0.0, 0.02]))
    task = types.SimpleNamespace(movable_obj=objs[1], task_bground_obj=objs[0], scene_model=scene_model)
    res = [len(poses), 1, 1, 1, 1, 1]
    check, static, movable = physics_utils.create_unsupcol_check(object(), task, res, embodied=False, lazy_phys_mods=False)
    assert static == [objs[0].phys_model, objs[2].phys_model] and movable == [objs[1].phys_model] and isinstance(check.shapes, RestatedShapes)
    got = check(torch.from_numpy(poses), task, torch.ones(len(poses), dtype=torch.bool))
    assert got.dtype == torch.bool and got.tolist() == [ok for _, _, ok, _ in HAND]          # the two halves of the table, ORed
    lazy, static, _ = physics_utils.create_unsupcol_check(object(), task, res, embodied=False)         # background (x < 44 only) + movable
    assert static == [objs[0].phys_model]
    got = lazy(torch.from_numpy(poses), task, torch.ones(len(poses), dtype=torch.bool)).tolist()
    assert got[0] is False and got[1] is False and got[7] is True and got[3] is False      # +x of the resting pose finds no table any more
    # a mix of field files and mesh files names both
    open(tmp_path / "mesh_0.obj", "w").write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    mixed = types.SimpleNamespace(movable_obj=objs[1], task_bground_obj=types.SimpleNamespace(phys_model=str(tmp_path / "mesh_0.obj")),
                                  scene_model=scene_model)
    with pytest.raises(ValueError, match=r"sdf_1\.npz.*mesh_0\.obj"):
        physics_utils.create_unsupcol_check(object(), mixed, res, embodied=False)
    # grids that differ are refused, and so is a movable object without points
    physics_utils.save_sdf_model(str(tmp_path / "sdf_2.npz"), (b0 + 1, nv, VOXEL, f32(0.016)), 3.0, 0.002, sdfphys_ref.pack_bits(rest),
                                 np.zeros((0, 3), np.float32))
    with pytest.raises(ValueError, match="grid differs.*b0"):
        physics_utils.create_unsupcol_check(object(), task, res, embodied=False, lazy_phys_mods=False)
    swapped = types.SimpleNamespace(movable_obj=objs[0], task_bground_obj=objs[1], scene_model=scene_model)
    with pytest.raises(ValueError, match="seen in no frame"):
        physics_utils.create_unsupcol_check(object(), swapped, res, embodied=False)


def test_library_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    assert lib.d2r_tsdf_grid(None, None, None, None, None) == -1 and lib.d2r_tsdf_touch_bits(None, ctypes.c_float(3.0), ctypes.c_float(0.002), None) == -1
    assert lib.d2r_sdfphys_create(None, None, None, ctypes.c_float(0.002), None, 0, None, 0, None) == -1
    assert lib.d2r_sdfphys_check(None, None, None, None, 0, None) == -1
    lib.d2r_sdfphys_destroy(None)
