"""The TSDF kernels (csrc/tsdf.hip) against the numpy restatement at the edges of DESIGN.md section 2c: every case of
tests/tsdf_edge_cases.py (all 254 triangle-producing cubes, seams between stamped and never-stamped blocks, exact zeros and
sdf == -trunc, the surface through each face of the grid, a camera inside the volume, an awkward camera and a far grid, band ratios,
erosion at k = 1 .. 32 on frames of 1 x 1 .. 129 x 70, more blocks in one frame than k_integrate has workgroups, touch words of
1 .. 5 words per row), state carried across calls, and the refusals.  Grid, blocks, voxels, vertices, triangles, the clean-up, solid
points and touch words must equal the restatement exactly: floats by their bits, integers by value.
tests/test_tsdf_edges_host.py shows on the CPU that the cases reach those edges and that wrong rules change what is compared here."""
import ctypes

import numpy as np
import pytest

from tests import tsdf_edge_cases as E
from tests import tsdf_ref

pytestmark = pytest.mark.gpu

NO_SURFACE = "seen in no frame"
FIRST = "cubes_seed%d" % E.CUBE_SEEDS[0]


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def same_partition(a, b):
    pairs = set(zip(np.asarray(a).tolist(), np.asarray(b).tolist()))
    return len(pairs) == len(set(np.asarray(a).tolist())) == len(set(np.asarray(b).tolist()))


def volume_of(ctx, c):
    from dream2real_amd.physics_utils import TsdfVolume
    return TsdfVolume(ctx, c["bounds"], c["voxel"], c["trunc"])


def check_grid(vol, c, ref_vol):
    b0, nv, voxel, trunc = vol.grid()
    assert tuple(int(v) for v in b0) == c["b0"] and tuple(int(v) for v in nv) == tuple(16 * n for n in c["nb"])
    assert (b0 == ref_vol.b0).all() and (nv == ref_vol.nv).all()
    assert same_bits(np.float32([voxel, trunc]), np.float32([c["voxel"], c["trunc"]]))


def check_voxels(vol, out, what=""):
    coords, tsdf, weight = vol.read_voxels()
    assert coords.shape == out["blocks"].shape and (coords == out["blocks"]).all(), what
    n_t, n_w = int((bits(tsdf) != bits(out["tsdf"])).sum()), int((bits(weight) != bits(out["w"])).sum())
    print(f"{what}: {len(coords)} blocks, voxels whose tsdf bits differ {n_t}, weight bits {n_w}, of {tsdf.size}; observed {int((out['w'] > 0).sum())}")
    assert n_t == 0 and n_w == 0, what
    return coords, tsdf, weight


def check_clean(got, want):
    assert same_bits(got["vertices"], want["vertices"])
    assert got["triangles"].shape == want["triangles"].shape and (got["triangles"].astype(np.int64) == want["triangles"]).all()
    assert same_partition(got["clusters"], want["clusters"]) and (got["keep"] == want["keep"]).all()
    assert same_bits(got["centre"], want["centre"])


def check_surface(vol, c, out, every_option=False):
    """raw mesh, the cleaned mesh, solid points and touch words of a fused volume against `out`"""
    from dream2real_amd import _lib
    name = c["name"]
    if len(out["tris"]) == 0:
        with pytest.raises(_lib.D2RError, match=NO_SURFACE):
            vol.extract(E.WEIGHT_THRESHOLD, None, 0.0)
    else:
        raw = vol.extract(E.WEIGHT_THRESHOLD, None, 0.0)
        print(f"{name}: raw mesh {len(raw['vertices'])} vertices / {len(raw['triangles'])} triangles (restatement {len(out['verts'])} / {len(out['tris'])})")
        assert same_bits(raw["vertices"], out["verts"])
        assert raw["triangles"].shape == out["tris"].shape and (raw["triangles"].astype(np.int64) == out["tris"]).all()
        assert raw["keep"].all()
        again = vol.extract(E.WEIGHT_THRESHOLD, None, 0.0)
        assert all(raw[k].tobytes() == again[k].tobytes() for k in raw)
        options = [(c["bounds"], 0.02)] + ([(c["bounds"], 0.0), (None, 0.02)] if every_option else [])
        for crop, keep in options:
            want = out["clean"] if (crop is not None and keep == 0.02) else tsdf_ref.clean(out["verts"], out["tris"], crop, keep)
            if len(want["triangles"]) == 0:
                with pytest.raises(_lib.D2RError, match="outside the crop box"):
                    vol.extract(E.WEIGHT_THRESHOLD, crop, keep)
            else:
                check_clean(vol.extract(E.WEIGHT_THRESHOLD, crop, keep), want)
    if len(out["solid"]) == 0:
        with pytest.raises(_lib.D2RError, match=NO_SURFACE):
            vol.solid_points(E.WEIGHT_THRESHOLD)
    else:
        assert same_bits(vol.solid_points(E.WEIGHT_THRESHOLD), out["solid"])
    for (thr, contact), want in out["touch"].items():
        got = vol.touch_bits(thr, contact)
        assert got.shape == want.shape and got.dtype == want.dtype and (got == want).all(), (name, thr, contact)


def compare(ctx, name, every_option=False):
    c = E.case(name)
    ref_vol, out = E.reference(name)
    vol = volume_of(ctx, c)
    try:
        check_grid(vol, c, ref_vol)
        for f in c["frames"]:
            vol.integrate(*f)
        check_voxels(vol, out, name)
        if c["mesh"]:
            check_surface(vol, c, out, every_option)
    finally:
        vol.close()
    return out


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", E.MESH_NAMES)
def test_fused_volume_and_surface_equal_the_restatement(ctx, name):
    compare(ctx, name, every_option=name in (FIRST, "seams", "zeros"))


@pytest.mark.parametrize("name", E.ERODE_NAMES + ["erode_5x3_k32_full", "three_metres"])
def test_eroded_frames_equal_the_restatement(ctx, name):
    c = E.case(name)
    ref_vol, out = E.reference(name)
    vol = volume_of(ctx, c)
    try:
        check_grid(vol, c, ref_vol)
        for f in c["frames"]:
            vol.integrate(*f)
        check_voxels(vol, out, name)
    finally:
        vol.close()


def test_a_frame_with_more_blocks_than_workgroups(ctx):
    import torch
    out = compare(ctx, "many_blocks")
    workgroups = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    print(f"many_blocks: {len(out['blocks'])} blocks stamped in one frame, k_integrate launches at most {workgroups} workgroups")
    assert len(out["blocks"]) > workgroups                        # or the grid-stride loop did not run: enlarge the case


# ------------------------------------------------------------------------------------------------ state across calls
def test_two_volumes_interleaved_on_one_context(ctx):
    names = (FIRST, "seams")
    cases = [E.case(n) for n in names]
    vols = [volume_of(ctx, c) for c in cases]
    try:
        for k in range(6):
            for vol, c in zip(vols, cases):
                vol.integrate(*c["frames"][k])
        for vol, c in zip(vols, cases):
            out = E.reference(c["name"])[1]
            check_voxels(vol, out, c["name"])
            raw = vol.extract(E.WEIGHT_THRESHOLD, None, 0.0)
            assert same_bits(raw["vertices"], out["verts"])
            assert raw["triangles"].shape == out["tris"].shape and (raw["triangles"].astype(np.int64) == out["tris"]).all()
    finally:
        for vol in vols:
            vol.close()


def test_a_frame_after_an_extraction_shows_in_the_next_one(ctx):
    c, more = E.case(FIRST), E.case(FIRST + "_plus")
    before, after = E.reference(FIRST)[1], E.reference(FIRST + "_plus")[1]
    vol = volume_of(ctx, c)
    try:
        for f in c["frames"]:
            vol.integrate(*f)
        a = vol.extract(E.WEIGHT_THRESHOLD, None, 0.0)
        assert same_bits(a["vertices"], before["verts"])
        vol.integrate(*more["frames"][-1])
        b = vol.extract(E.WEIGHT_THRESHOLD, None, 0.0)            # the same arguments: the kept mesh must not be handed out again
        assert not same_bits(a["vertices"], b["vertices"])
        assert same_bits(b["vertices"], after["verts"])
        assert b["triangles"].shape == after["tris"].shape and (b["triangles"].astype(np.int64) == after["tris"]).all()
        check_voxels(vol, after, more["name"])
    finally:
        vol.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_volume_as_it_was(ctx):
    from dream2real_amd import _lib
    lib, ptr = ctx.lib, _lib.ptr
    c = E.case(FIRST)
    out = E.reference(FIRST)[1]
    nan = float("nan")
    v = float(c["voxel"])

    def create(bounds, voxel, trunc):
        h = ctypes.c_void_p()
        b6 = np.ascontiguousarray(bounds, np.float32).reshape(6)
        rc = lib.d2r_tsdf_create(ctx.h, ptr(b6), voxel, trunc, ctypes.byref(h))
        assert rc != 0 and not h.value, (bounds, voxel, trunc)

    b = c["bounds"]
    create(b, v, v / 2)                                           # trunc < voxel
    create(b, nan, 8 * v)
    create([[0, 0, 0], [0, 1, 1]], v, 8 * v)                      # lo == hi
    create([[140000, 0, 0], [140001, 1, 1]], v, 8 * v)            # more than 2^20 blocks of 0.125 m out
    create([[-5000, 0, 0], [5000, 1, 1]], v, 8 * v)               # 80000 blocks wide

    vol = volume_of(ctx, c)
    try:
        for f in c["frames"]:
            vol.integrate(*f)
        check_voxels(vol, out, "before the refusals")
        depth, mask, K, pose, _ = c["frames"][0]
        d16, m8 = np.ascontiguousarray(depth, np.uint16), np.ascontiguousarray(mask, np.uint8)
        K32, P32 = np.ascontiguousarray(K, np.float32).reshape(9), np.ascontiguousarray(pose, np.float32).reshape(16)
        H, W = depth.shape

        def integrate(w=W, h=H, K=K32, P=P32, k=1, d=d16, m=m8):
            assert lib.d2r_tsdf_integrate(vol.h, ptr(d), ptr(m), w, h, ptr(K), ptr(P), k) != 0, (w, h, k)

        def poked(a, i, x):
            a = a.copy()
            a[i] = x
            return a

        integrate(w=0)
        integrate(w=16385, h=1, d=np.zeros(16385, np.uint16), m=np.zeros(16385, np.uint8))
        integrate(k=0)
        integrate(k=33)
        integrate(K=poked(K32, 2, nan))
        integrate(P=poked(P32, 7, nan))
        integrate(K=poked(K32, 0, 0.0))

        nv, nt = len(out["verts"]), len(out["tris"])
        bufs = (np.zeros((nv, 3), np.float32), np.zeros((nt, 3), np.uint32), np.zeros(nt, np.int32), np.zeros(nt, np.uint8), np.zeros(3, np.float64))

        def extract(thr=3.0, keep=0.0, cap_v=nv, cap_t=nt, fill=False):
            n_v, n_t = ctypes.c_uint32(cap_v), ctypes.c_uint32(cap_t)
            args = [ptr(a) for a in bufs] if fill else [None] * 5
            return lib.d2r_tsdf_extract(vol.h, thr, None, keep, ctypes.byref(n_v), ctypes.byref(n_t), *args), n_v.value, n_t.value

        assert extract(thr=0.0)[0] != 0 and extract(thr=nan)[0] != 0
        assert extract(keep=-0.1)[0] != 0 and extract(keep=1.1)[0] != 0
        assert extract() == (0, nv, nt)
        assert extract(cap_v=nv - 1, fill=True)[0] != 0 and extract(cap_t=nt - 1, fill=True)[0] != 0
        assert extract(fill=True)[0] == 0 and same_bits(bufs[0], out["verts"])

        nb = len(out["blocks"])
        coords, ts, ws = np.zeros((nb, 3), np.int32), np.zeros((nb, 16, 16, 16), np.float32), np.zeros((nb, 16, 16, 16), np.float32)
        n = ctypes.c_uint32(nb)
        assert lib.d2r_tsdf_read_voxels(vol.h, ctypes.byref(n), ptr(coords), ptr(ts), None) != 0
        n = ctypes.c_uint32(nb - 1)
        assert lib.d2r_tsdf_read_voxels(vol.h, ctypes.byref(n), ptr(coords), ptr(ts), ptr(ws)) != 0 and n.value == nb

        ns = len(out["solid"])
        xyz = np.zeros((ns, 3), np.float32)
        n = ctypes.c_uint32(ns - 1)
        assert lib.d2r_tsdf_solid_points(vol.h, 3.0, ctypes.byref(n), ptr(xyz)) != 0 and n.value == ns

        words = np.zeros_like(out["touch"][E.TOUCH_ARGS[0]])
        assert lib.d2r_tsdf_touch_bits(vol.h, 0.0, 0.002, ptr(words)) != 0
        assert lib.d2r_tsdf_touch_bits(vol.h, 3.0, nan, ptr(words)) != 0

        check_voxels(vol, out, "after the refusals")
        check_surface(vol, c, out)
    finally:
        vol.close()
    compare(ctx, "erode_65x33_k3")                                # the context still fuses a frame correctly
