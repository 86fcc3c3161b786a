"""TSDF physics meshes, CPU side: the numpy restatement of DESIGN.md section 2c (tests/tsdf_ref.py) against analytic truth
on a ray-cast scene, its erosion against hand-derived cases, the marching-cubes table against its numbering, and the host
pieces of the product (the .obj writer, the cached branch of get_phys_models, the branches it refuses)."""
import os
import re

import numpy as np
import pytest

from dream2real_amd import _lib, physics_utils
from dream2real_amd.physics_utils import get_phys_models          # the feature: absent before it, this import fails
from tests import tsdf_ref, tsdf_scene

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL = 0.002


@pytest.fixture(scope="module")
def scene():
    return tsdf_scene.make_scene()


@pytest.fixture(scope="module")
def fused(scene):
    return {obj: tsdf_ref.fuse(scene["depths"], scene["cam_poses"], scene["intrinsics"], scene["masks"], obj, scene["bounds"]) for obj in (0, 1)}


def test_table_follows_the_bourke_numbering_and_the_library_holds_the_same_rows():
    """A case uses exactly the edges whose two corners differ in sign, in whole triangles; the library's header and the
    restatement's copy are the same 256 rows."""
    for case, row in enumerate(tsdf_ref.TRI_TABLE):
        crossed = {e for e, (p, q) in enumerate(tsdf_ref.EDGE_CORNERS) if ((case >> p) & 1) != ((case >> q) & 1)}
        assert set(row) == crossed and len(row) % 3 == 0 and len(row) <= 15, case
    for e, (p, q) in enumerate(tsdf_ref.EDGE_CORNERS):                 # an edge's voxel offset and axis from its corners
        lo = np.minimum(tsdf_ref.CORNERS[p], tsdf_ref.CORNERS[q])
        assert tuple(lo) == tsdf_ref.EDGE_OFF[e] and np.abs(np.subtract(tsdf_ref.CORNERS[p], tsdf_ref.CORNERS[q])).argmax() == tsdf_ref.EDGE_AXIS[e]
    src = open(os.path.join(REPO, "dream2real_amd", "csrc", "mc_table.h")).read()
    rows = re.findall(r"\{([-\d,\s]+)\}", src[src.index("D2R_MC_TABLE_ROWS"):])
    assert len(rows) == 256
    for case, r in enumerate(rows):
        vals = [int(x) for x in r.split(",")]
        assert len(vals) == 16 and tuple(v for v in vals if v >= 0) == tuple(tsdf_ref.TRI_TABLE[case]), case


def test_erosion_hand_derived_cases():
    """cv2's rule for an even kernel: anchor (k // 2, k // 2), so pixel (i, j) survives when rows i - k/2 .. i + k/2 - 1 and the
    same columns are all set; outside the frame counts as set."""
    m = np.zeros((60, 70), bool)
    m[10:40, 20:55] = True                                    # rows 10..39, columns 20..54
    e = tsdf_ref.erode(m, 20)                                 # needs rows i-10 .. i+9 inside 10..39 -> i in 20..30
    want = np.zeros_like(m)
    want[20:31, 30:46] = True                                 # columns j-10 .. j+9 inside 20..54 -> j in 30..45
    assert (e == want).all()
    e8 = tsdf_ref.erode(m, 8)                                 # rows i-4 .. i+3 -> i in 14..36, columns j in 24..51
    want8 = np.zeros_like(m)
    want8[14:37, 24:52] = True
    assert (e8 == want8).all()
    b = np.zeros((60, 70), bool)
    b[0:25, 50:70] = True                                     # a blob in the top-right corner: the frame border does not erode
    eb = tsdf_ref.erode(b, 20)                                # rows up to i+9 <= 24 -> i in 0..15; columns j-10 >= 50 -> j in 60..69
    wantb = np.zeros_like(b)
    wantb[0:16, 60:70] = True
    assert (eb == wantb).all()
    eb8 = tsdf_ref.erode(b, 8)                                # i+3 <= 24 -> 0..21; j-4 >= 50 -> 54..69
    wantb8 = np.zeros_like(b)
    wantb8[0:22, 54:70] = True
    assert (eb8 == wantb8).all()
    assert tsdf_ref.erode(np.ones((5, 5), bool), 20).all()    # a full frame stays full
    one = np.ones((30, 30), bool)
    one[12, 17] = False                                       # one hole removes rows 12-9 .. 12+10, columns 17-9 .. 17+10
    eh = tsdf_ref.erode(one, 20)
    wanth = np.ones_like(one)
    wanth[3:23, 8:28] = False
    assert (eh == wanth).all()


def _visible_centroid(scene, obj, pts, normals, weights):
    """Centroid of the surface samples `pts` that at least three views see through the object's eroded mask, each sample
    weighted by its area times |nx| + |ny| + |nz|: marching cubes puts one vertex on every grid edge the surface crosses,
    and a patch of area dA with unit normal n crosses dA (|nx| + |ny| + |nz|) / voxel^2 grid edges, so that is the density
    the mean of a marching-cubes vertex array samples the surface with."""
    K = scene["intrinsics"]
    seen = np.zeros(len(pts), int)
    for f in range(len(scene["depths"])):
        T = scene["cam_poses"][f]
        u16 = (scene["depths"][f] * 1000).astype(np.uint16)
        ok_px = tsdf_ref.erode(scene["masks"][f] == obj, 20 if obj == 0 else 8) & (u16 > 0) & (u16 <= 3000)
        pc = (pts - T[:3, 3]) @ T[:3, :3]
        front = (normals * (T[:3, 3] - pts)).sum(-1) > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.floor(K[0, 0] * pc[:, 0] / pc[:, 2] + K[0, 2] + 0.5)
            v = np.floor(K[1, 1] * pc[:, 1] / pc[:, 2] + K[1, 2] + 0.5)
        inside = front & (pc[:, 2] > 0) & (u >= 0) & (u < tsdf_scene.W) & (v >= 0) & (v < tsdf_scene.H)
        ui, vi = np.where(inside, u, 0).astype(int), np.where(inside, v, 0).astype(int)
        near = np.abs(u16[vi, ui] / 1000.0 - pc[:, 2]) < 0.003          # the pixel shows this sample, not something in front of it
        seen += inside & ok_px[vi, ui] & near
    w = weights * np.abs(normals).sum(-1) * (seen >= 3)
    return (pts * w[:, None]).sum(0) / w.sum()


def test_restatement_against_analytic_truth(scene, fused):
    """Sphere (object 1) resting on a slab (object 0), 12 views, fp16 depth, a patch of the slab mislabelled as the sphere in
    five views.  The slab is wider than every view, as a table top is: the rule's 20-pixel erosion discards the band along
    a silhouette, so a slab whose side faces were in view would have them rebuilt from free space only."""
    truth = {0: tsdf_scene.slab_distance, 1: tsdf_scene.sphere_distance}
    for obj in (0, 1):
        vol, rv, rt, m = fused[obj]
        kept = np.unique(m["triangles"][m["keep"]])
        d = truth[obj](m["vertices"][kept])
        print(f"object {obj}: {len(rv)} raw vertices, {len(m['vertices'])} after the crop, {m['keep'].sum()} / {len(m['keep'])} triangles kept, "
              f"clusters {np.bincount(m['clusters']).tolist()[:8]}, max distance to the true surface {d.max():.6f} m")
        assert d.max() <= VOXEL
        assert (m["vertices"] >= scene["bounds"][0].astype(np.float32)).all() and (m["vertices"] <= scene["bounds"][1].astype(np.float32)).all()
        assert vol.frames_used == 12
    vol, rv, rt, m = fused[1]
    sizes = np.bincount(m["clusters"])
    assert len(sizes) >= 2                                           # the mislabelled patch made a cluster of its own ...
    speckle = tsdf_scene.sphere_distance(m["vertices"]) > 5 * VOXEL
    assert speckle.any() and np.linalg.norm(m["vertices"][speckle][:, :2] - tsdf_scene.SPECKLE_C[:2], axis=1).max() < tsdf_scene.SPECKLE_R + VOXEL
    kept_labels = np.unique(m["clusters"][m["keep"]])
    assert len(kept_labels) == 1                                     # ... and exactly one cluster is left: the sphere
    assert not speckle[np.unique(m["triangles"][m["keep"]])].any()   # no kept triangle touches the patch
    assert sizes[kept_labels[0]] == sizes.max() and (sizes[np.arange(len(sizes)) != kept_labels[0]] < 0.02 * sizes.max()).all()


def test_init_pose_is_the_centroid_of_the_visible_surface(scene, fused):
    # the sphere: samples on a latitude-longitude grid, area weight cos(latitude)
    lat, lon = np.meshgrid(np.linspace(-np.pi / 2, np.pi / 2, 361)[1:-1], np.linspace(0, 2 * np.pi, 720, endpoint=False), indexing="ij")
    n = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], -1).reshape(-1, 3)
    want1 = _visible_centroid(scene, 1, tsdf_scene.SPHERE_C + tsdf_scene.SPHERE_R * n, n, np.cos(lat).reshape(-1))
    # the slab: its top face inside the crop box, every 0.5 mm
    g = np.arange(scene["bounds"][0][0], scene["bounds"][1][0] + 1e-9, 0.0005)
    xx, yy = np.meshgrid(g, g)
    top = np.stack([xx.reshape(-1), yy.reshape(-1), np.zeros(xx.size)], -1)
    want0 = _visible_centroid(scene, 0, top, np.tile([0.0, 0.0, 1.0], (len(top), 1)), np.ones(len(top)))
    for obj, want in ((0, want0), (1, want1)):
        m = fused[obj][3]
        # the reference's centre is the mean of the vertex array that remove_triangles_by_mask leaves: for the sphere it still
        # holds the mislabelled patch's vertices, which no triangle references any more
        err = np.linalg.norm(m["centre"] - want)
        kept = np.unique(m["triangles"][m["keep"]])
        err_kept = np.linalg.norm(m["vertices"][kept].astype(np.float64).mean(0) - want)
        print(f"object {obj}: centre {m['centre']}, centroid of the visible surface {want}, distance {err:.6f} m (kept vertices only: {err_kept:.6f} m)")
        assert err <= VOXEL


def test_obj_writer_matches_the_restatement(tmp_path, fused):
    m = fused[1][3]
    p = str(tmp_path / "mesh_concave_1.obj")
    _lib.obj_write(p, m["vertices"], m["triangles"], m["keep"])
    data = open(p, "rb").read()
    assert data == tsdf_ref.obj_bytes(m["vertices"], m["triangles"], m["keep"])
    assert data.count(b"\nf ") == int(m["keep"].sum()) and data.count(b"v ") == len(m["vertices"])
    hull = physics_utils.hulls_from_obj(p)                     # vertices of dropped triangles stay in the file, unreferenced
    assert len(hull) == 1 and len(hull[0]) == len(np.unique(m["triangles"][m["keep"]]))
    lib = _lib.load()
    bad = np.array([[0, 1, 7]], np.uint32)
    assert lib.d2r_obj_write(os.fsencode(p), _lib.ptr(m["vertices"][:3].copy()), 3, _lib.ptr(bad), 1, None) == -1
    assert lib.d2r_obj_write(None, None, 0, None, 0, None) == -1


def test_cached_branch_and_refused_branches(tmp_path):
    import torch
    poses = []
    for k in range(2):
        open(tmp_path / f"mesh_{k}.obj", "w").write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
        T = np.eye(4)
        T[:3, 3] = (0.1 * k, 0.2, 0.3)
        np.savetxt(tmp_path / f"init_pose_{k}.txt", T)
        poses.append(T)
    paths, init = get_phys_models(None, None, None, None, 2, None, save_dir=str(tmp_path))           # use_cache defaults to True (:26)
    assert paths == [os.path.join(str(tmp_path), f"mesh_{k}.obj") for k in range(2)]
    assert all(p.dtype == torch.float32 and np.allclose(p.numpy(), T) for p, T in zip(init, poses))
    with pytest.raises(NotImplementedError, match="Poisson"):
        get_phys_models([], [], np.eye(3), [], 1, np.zeros((2, 3)), save_dir=str(tmp_path), use_cache=False, use_phys_tsdf=False)
    try:
        import pybullet  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="PyBullet"):
            physics_utils.vhacd_convexify(str(tmp_path / "a.obj"), str(tmp_path / "b.obj"), 0)
