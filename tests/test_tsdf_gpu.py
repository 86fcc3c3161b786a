"""TSDF physics meshes on the GPU against the numpy restatement (tests/tsdf_ref.py): blocks, voxels,
vertices, triangles, clusters, centre and the bytes of the .obj file must be IDENTICAL; degenerate inputs; and the way
through get_phys_models -> hulls_from_obj -> create_unsupcol_check."""
import os
import shutil
import types

import numpy as np
import pytest

from dream2real_amd import _lib, physics_utils
from dream2real_amd.physics_utils import TsdfVolume, create_lazy_phys_mods, get_phys_models
from tests import tsdf_ref, tsdf_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene():
    return tsdf_scene.make_scene()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_partition(a, b):
    pairs = set(zip(np.asarray(a).tolist(), np.asarray(b).tolist()))
    return len(pairs) == len(set(np.asarray(a).tolist())) == len(set(np.asarray(b).tolist()))


def whole_mesh_hull(concave_path, convex_path, obj_id):
    """Stands where VHACD stands: the mesh as ONE shape, which the physics loader turns into the hull of its faces' vertices."""
    shutil.copyfile(concave_path, convex_path)


def fuse_gpu(ctx, scene, obj, frame_range):
    vol = TsdfVolume(ctx, scene["bounds"])
    for f in frame_range:
        u16 = (scene["depths"][f] * 1000).astype(np.uint16)
        vol.integrate(u16, scene["masks"][f] == obj, scene["intrinsics"], scene["cam_poses"][f], 20 if obj == 0 else 8)
    return vol


def compare(ctx, scene, obj, frame_range, tmp_path):
    ref_vol, rv, rt, rm = tsdf_ref.fuse(scene["depths"], scene["cam_poses"], scene["intrinsics"], scene["masks"], obj, scene["bounds"], frame_range)
    vol = fuse_gpu(ctx, scene, obj, frame_range)
    coords, tsdf, weight = vol.read_voxels()
    want_coords = ref_vol.active_blocks()
    print(f"object {obj}: {len(coords)} active blocks (restatement {len(want_coords)})")
    assert coords.shape == want_coords.shape and (coords == want_coords).all()                     # the active-block set
    want_t, want_w = ref_vol.block_voxels()
    n_dt, n_dw = int((bits(tsdf) != bits(want_t)).sum()), int((bits(weight) != bits(want_w)).sum())
    print(f"object {obj}: voxels whose tsdf bits differ {n_dt}, weight bits {n_dw}, of {tsdf.size}; observed voxels {(want_w > 0).sum()}")
    assert n_dt == 0 and n_dw == 0                                                                 # (tsdf, w) of every active voxel
    raw = vol.extract(3.0, None, 0.0)
    print(f"object {obj}: raw mesh {raw['vertices'].shape[0]} vertices / {raw['triangles'].shape[0]} triangles (restatement {len(rv)} / {len(rt)})")
    assert raw["vertices"].shape == rv.shape and (bits(raw["vertices"]) == bits(rv)).all()         # canonical vertex array
    assert raw["triangles"].shape == rt.shape and (raw["triangles"].astype(np.int64) == rt).all()  # canonical triangle array
    assert raw["keep"].all()
    m = vol.extract(3.0, scene["bounds"], 0.02)
    assert m["vertices"].shape == rm["vertices"].shape and (bits(m["vertices"]) == bits(rm["vertices"])).all()
    assert (m["triangles"].astype(np.int64) == rm["triangles"]).all()
    assert same_partition(m["clusters"], rm["clusters"]) and (m["keep"] == rm["keep"]).all()       # cluster labels' partition
    assert (bits(m["centre"]) == bits(rm["centre"])).all()                                         # init_pose's translation, fp64
    p = str(tmp_path / f"mesh_concave_{obj}.obj")
    _lib.obj_write(p, m["vertices"], m["triangles"], m["keep"])
    assert open(p, "rb").read() == tsdf_ref.obj_bytes(rm["vertices"], rm["triangles"], rm["keep"])
    vol.close()
    return rm


def test_gpu_equals_the_restatement_on_the_twelve_view_scene(ctx, scene, tmp_path):
    for obj in (0, 1):
        rm = compare(ctx, scene, obj, range(12), tmp_path)
        assert rm["keep"].sum() > 1000


def test_gpu_equals_the_restatement_with_one_view_four_times(ctx, tmp_path):
    """use_vis_pcds framing (reference :64-65): the single view repeated four times reaches weight 4 >= 3."""
    scene = tsdf_scene.make_scene(n_views=3)
    for obj in (0, 1):
        rm = compare(ctx, scene, obj, [1] * 4, tmp_path)
        assert rm["keep"].sum() > 50
    # ... and through get_phys_models: the same files
    paths, poses = get_phys_models(scene["depths"], scene["cam_poses"], scene["intrinsics"], scene["masks"], 2, scene["bounds"],
                                   save_dir=str(tmp_path / "out"), use_cache=False, use_phys_tsdf=True, use_vis_pcds=True, single_view_idx=1,
                                   ctx=ctx, convexify=whole_mesh_hull)
    for obj in (0, 1):
        rm = tsdf_ref.fuse(scene["depths"], scene["cam_poses"], scene["intrinsics"], scene["masks"], obj, scene["bounds"], [1] * 4)[3]
        assert open(tmp_path / "out" / f"mesh_concave_{obj}.obj", "rb").read() == tsdf_ref.obj_bytes(rm["vertices"], rm["triangles"], rm["keep"])
        want = np.eye(4, dtype=np.float32)
        want[:3, 3] = rm["centre"]
        assert (bits(poses[obj].numpy()) == bits(want)).all()
        assert (np.loadtxt(tmp_path / "out" / f"init_pose_{obj}.txt") == want.astype(np.float64)).all()


def test_degenerate_inputs(ctx, scene, tmp_path):
    # a frame without the object changes nothing: it is skipped
    extra = dict(scene)
    extra["depths"] = np.concatenate([scene["depths"][:5], scene["depths"][5:6], scene["depths"][5:]])
    extra["masks"] = np.concatenate([scene["masks"][:5], np.zeros_like(scene["masks"][5:6]), scene["masks"][5:]])
    extra["cam_poses"] = np.concatenate([scene["cam_poses"][:5], scene["cam_poses"][5:6], scene["cam_poses"][5:]])
    a, b = fuse_gpu(ctx, extra, 1, range(13)), fuse_gpu(ctx, scene, 1, range(12))
    ref_vol = tsdf_ref.fuse(extra["depths"], extra["cam_poses"], extra["intrinsics"], extra["masks"], 1, extra["bounds"])[0]
    assert ref_vol.frames_used == 12
    (ca, ta, wa), (cb, tb, wb) = a.read_voxels(), b.read_voxels()
    assert (ca == cb).all() and (bits(ta) == bits(tb)).all() and (bits(wa) == bits(wb)).all()
    assert (ca == ref_vol.active_blocks()).all() and (bits(ta) == bits(ref_vol.block_voxels()[0])).all()
    a.close(); b.close()
    # an object no frame shows: a clear error, no fault, no empty mesh file
    none = dict(scene)
    none["masks"] = np.zeros_like(scene["masks"])
    out = tmp_path / "none"
    with pytest.raises(ValueError, match="seen in no frame"):
        get_phys_models(none["depths"], none["cam_poses"], none["intrinsics"], none["masks"], 2, none["bounds"], save_dir=str(out),
                        use_cache=False, use_phys_tsdf=True, ctx=ctx, convexify=whole_mesh_hull)
    assert os.path.exists(out / "mesh_0.obj") and not os.path.exists(out / "mesh_concave_1.obj") and not os.path.exists(out / "mesh_1.obj")
    empty = TsdfVolume(ctx, scene["bounds"])
    assert len(empty.read_voxels()[0]) == 0
    with pytest.raises(_lib.D2RError, match="seen in no frame"):
        empty.extract()
    empty.close()
    # bounds over the cap of the dense volume are refused with the documented message
    with pytest.raises(_lib.D2RError, match="TSDF volume over the cap"):
        TsdfVolume(ctx, [[-3.0, -3.0, -3.0], [3.0, 3.0, 3.0]])
    with pytest.raises(_lib.D2RError):
        TsdfVolume(ctx, [[0.0, 0.0, 0.0], [0.0, 1.0, 1.0]])
    # the context still works
    ok = fuse_gpu(ctx, scene, 1, range(3))
    assert len(ok.read_voxels()[0]) > 0
    ok.close()


def test_end_to_end_meshes_feed_the_physics_prefilter(ctx, tmp_path):
    """RGB-D frames -> get_phys_models -> hulls_from_obj -> create_unsupcol_check: the sphere where it rests is valid, lowered
    into the slab it collides, raised by 5 cm it is unsupported.  A 12 mm sphere: cameras above the table see a sphere down to
    a few millimetres above its equator, and the reference's support test lowers the object by 2 cm, so the rebuilt cap of
    a sphere of more than some 15 mm radius hangs too high above the table to count as supported."""
    import torch
    scene = tsdf_scene.make_scene(sphere_r=0.012, speckle_r=0.0085)      # (a patch small enough to fall under 2 % of this small sphere)
    out = str(tmp_path / "phys")
    scene_model = types.SimpleNamespace(depths=torch.from_numpy(scene["depths"]), opt_cam_poses=torch.from_numpy(scene["cam_poses"]),
                                        intrinsics=scene["intrinsics"], masks=torch.from_numpy(scene["masks"].astype(np.int64)) * 3,
                                        scene_centre=torch.tensor([0.0, 0.0, -0.05]))
    movable = types.SimpleNamespace(mask_idx=3)
    (bg_path, mov_path), (bg_pose, mov_pose) = create_lazy_phys_mods(scene_model, movable, scene["bounds"], out, ctx=ctx, convexify=whole_mesh_hull)
    assert bg_path == os.path.join(out, "mesh_0.obj") and mov_path == os.path.join(out, "mesh_1.obj")
    assert len(physics_utils.hulls_from_obj(mov_path)) == 1 and len(physics_utils.hulls_from_obj(bg_path)) == 1
    for obj, pose in ((0, bg_pose), (1, mov_pose)):            # the restatement's centre, to the bit
        rm = tsdf_ref.fuse(scene["depths"], scene["cam_poses"], scene["intrinsics"], scene["masks"], obj, scene["bounds"])[3]
        want = np.eye(4, dtype=np.float32)
        want[:3, 3] = rm["centre"]
        assert (bits(pose.numpy()) == bits(want)).all()
        assert len(np.unique(rm["clusters"][rm["keep"]])) == 1
    movable.pose, movable.phys_model = mov_pose, mov_path
    task = types.SimpleNamespace(movable_obj=movable, task_bground_obj=types.SimpleNamespace(phys_model=bg_path), scene_model=scene_model)
    xs, zs = [-0.01, 0.0, 0.01], [0.0, -0.02, 0.05]
    poses = []
    for x in xs:                                           # positions outermost, as the pose grid enumerates them
        for z in zs:
            P = mov_pose.numpy().copy()
            P[0, 3] += x
            P[2, 3] += z
            poses.append(P)
    poses = np.stack(poses)
    check, _, _ = physics_utils.create_unsupcol_check(ctx, task, [3, 1, 3, 1, 1, 1], embodied=False)
    valid = check(torch.from_numpy(poses), task, torch.ones(len(poses), dtype=torch.bool)).numpy().reshape(3, 3)
    print("valid (rows x, columns rest / lowered 2 cm / raised 5 cm):", valid.tolist())
    assert (valid[:, 0]).all() and not valid[:, 1].any() and not valid[:, 2].any()
    # lowered into the slab is a COLLISION, not merely a lack of support: a pose below the scene centre's height counts as
    # supported whatever lies under it (reference :332-340) and skips the stability probes, so with the scene centre put above
    # every pose only a collision can make one invalid
    high = types.SimpleNamespace(movable_obj=movable, task_bground_obj=task.task_bground_obj,
                                 scene_model=types.SimpleNamespace(scene_centre=torch.tensor([0.0, 0.0, 1.0])))
    loose, _, _ = physics_utils.create_unsupcol_check(ctx, high, [3, 1, 3, 1, 1, 1], embodied=False)
    v2 = loose(torch.from_numpy(poses), high, torch.ones(len(poses), dtype=torch.bool)).numpy().reshape(3, 3)
    print("collision only (rows x, columns rest / lowered 2 cm / raised 5 cm):", v2.tolist())
    assert v2[:, 0].all() and not v2[:, 1].any() and v2[:, 2].all()
    check.shapes.close(); loose.shapes.close()
    # the cached branch returns the same paths and poses
    (bg2, mov2), (bgp2, movp2) = create_lazy_phys_mods(scene_model, movable, scene["bounds"], out, use_cache=True)
    assert (bg2, mov2) == (bg_path, mov_path) and torch.equal(bgp2, bg_pose) and torch.equal(movp2, mov_pose)
