"""The extraction's chunk scans (tsdf.hip k_mc_scan_chunks / k_tsdf_solid_scan and the emit kernels behind them, all on the
one-workgroup scan of d2r_shared.h) at the row lengths where a scan partitioned over 256 threads goes wrong: 1, 8, 255, 256, 257
and 513 chunks.  A chunk is 4096 voxels in (z, y, x) order, so a volume of n blocks has n chunks; thread t of the scan owns
chunks t * per .. t * per + per - 1, per = ceil(n / 256).

One synthetic frame, integrated four times: a camera looking along +x at a constant depth of 1 m, i.e. the plane
x = (x0 + 0.5) voxel across the whole (y, z) section of the grid.  Every (z, y) row of the grid then carries one vertex (on its
x-edge at x0) and one solid voxel (at x0 + 1), so every chunk is non-empty, the first and the last thread's among them.
Vertices, triangles and solid points must equal the numpy restatements (tests/tsdf_ref.py, tests/sdfphys_ref.py) bit for bit."""
import functools

import numpy as np
import pytest

from tests import sdfphys_ref, tsdf_ref

VOXEL = 1.0 / 128.0                    # exact in fp32; trunc = voxel, so a block of 16 voxels is 0.125 m
CHUNK = 4096
# blocks per axis (x, y, z) -> 1, 8, 255, 256, 257 and 513 chunks
SHAPES = [(1, 1, 1), (8, 1, 1), (255, 1, 1), (16, 16, 1), (257, 1, 1), (19, 9, 3)]
IDS = ["%d_chunks" % (s[0] * s[1] * s[2]) for s in SHAPES]
W = H = 256


def make_case(nb):
    """-> (bounds, depth_u16, mask, intrinsics, cam_pose, x0) for a grid of exactly nb blocks starting at block 0."""
    bs = 16 * VOXEL
    # lo - trunc >= 0 and (nb - 1) bs <= hi + trunc < nb bs on every axis
    bounds = np.array([[2 * VOXEL] * 3, [n * bs - 4 * VOXEL for n in nb]], np.float32)
    x0 = 40 if nb[0] > 2 else 8                              # the plane lies between voxels x0 and x0 + 1 (past x = 16: see the 257-chunk grid)
    half = max(nb[1], nb[2]) * bs / 2
    f = float(int(110.0 / half))                             # the section spans about +-110 of the 128 pixels either side of the centre
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = [[0, 0, 1], [1, 0, 0], [0, 1, 0]]         # camera x -> world y, camera y -> world z, optical axis -> world x
    pose[:3, 3] = [(x0 + 0.5) * VOXEL - 1.0, nb[1] * bs / 2, nb[2] * bs / 2]
    return bounds, np.full((H, W), 1000, np.uint16), np.ones((H, W), bool), K, pose, x0


@functools.lru_cache(maxsize=None)
def reference(nb):
    """The restatement's volume, raw mesh and solid points of a shape: computed once, shared, never written to."""
    bounds, depth, mask, K, pose, _ = make_case(nb)
    vol = tsdf_ref.Volume(bounds, VOXEL, VOXEL)
    for _ in range(4):
        vol.integrate(depth, mask, K, pose, 1)
    verts, tris = vol.marching_cubes(3.0)
    pts = sdfphys_ref.solid_points(vol, 3.0)
    for a in (verts, tris, pts):
        a.setflags(write=False)
    return vol, verts, tris, pts


def chunks_of(xyz, vol):
    """chunk of the voxel each position belongs to (floor per axis: a vertex on an x-edge belongs to the edge's lower voxel)"""
    g = np.floor(np.asarray(xyz, np.float64) / VOXEL).astype(np.int64)
    nx, ny = int(vol.nv[0]), int(vol.nv[1])
    return np.unique(((g[:, 2] * ny + g[:, 1]) * nx + g[:, 0]) // CHUNK)


@pytest.mark.parametrize("nb", SHAPES, ids=IDS)
def test_every_shape_has_surface_in_the_first_and_the_last_threads_range(nb):
    vol, verts, tris, pts = reference(nb)
    n = nb[0] * nb[1] * nb[2]
    assert tuple(int(v) for v in vol.nb) == nb and (vol.b0 == 0).all() and vol.tsdf.size == n * CHUNK
    assert len(tris) >= 1 and len(pts) >= 1
    per = (n + 255) // 256
    last = ((n - 1) // per) * per                            # first chunk of the last thread that owns any
    for what, c in (("vertices", chunks_of(verts, vol)), ("solid points", chunks_of(pts, vol))):
        print(f"{n} chunks, per {per}: {what} in {len(c)} chunks, first {c[0]}, last {c[-1]}")
        assert (c < per).any() and (c >= last).any(), what


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", SHAPES, ids=IDS)
def test_mesh_and_solid_points_equal_the_restatement(ctx, nb):
    from dream2real_amd.physics_utils import TsdfVolume
    ref_vol, rv, rt, rp = reference(nb)
    bounds, depth, mask, K, pose, _ = make_case(nb)
    vol = TsdfVolume(ctx, bounds, VOXEL, VOXEL)
    try:
        assert tuple(int(v) for v in vol.grid()[1]) == tuple(int(v) for v in ref_vol.nv)
        for _ in range(4):
            vol.integrate(depth, mask, K, pose, 1)
        raw = vol.extract(3.0, None, 0.0)
        pts = vol.solid_points(3.0)
    finally:
        vol.close()
    print(f"{nb}: {len(raw['vertices'])} vertices / {len(raw['triangles'])} triangles / {len(pts)} solid points "
          f"(restatement {len(rv)} / {len(rt)} / {len(rp)})")
    assert raw["vertices"].shape == rv.shape and (bits(raw["vertices"]) == bits(rv)).all()
    assert raw["triangles"].shape == rt.shape and (raw["triangles"].astype(np.int64) == rt).all()
    assert pts.shape == rp.shape and (bits(pts) == bits(rp)).all()
