"""Camera-pose refinement on the GPU against the numpy restatement tests/camtrack_ref.py: the 29 sums of a
linearisation by integer equality at every edge the rule has, the loop iteration by iteration, the behaviour conditions, refusals."""
import ctypes as C

import numpy as np
import pytest

from dream2real_amd import _lib, cam_pose_opt
from dream2real_amd.physics_utils import TsdfVolume
from tests import camtrack_cases as cases
from tests import camtrack_ref as ref

pytestmark = pytest.mark.gpu
K = cases.INTRINSICS
DOWN = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]], np.float32)      # a camera looking straight down


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _grid(vol):
    coords, tsdf, weight = vol.read_voxels()
    b0, nv, voxel, trunc = vol.grid()
    return ref.grid_from_blocks(coords, tsdf, weight, b0, nv, voxel, trunc)


@pytest.fixture(scope="module")
def scene(ctx):
    """The tracking scene: frames 0 .. 2 fused on the GPU at their true poses, read back once for the restatement."""
    d, T, m = cases.tracking_frames()
    vol = cases.fuse(TsdfVolume(ctx, cases.BOUNDS), d, T, m)
    yield vol, _grid(vol), d, T, m
    vol.close()


def same(ctx, vol, grid, depth, mask, intr, pose, thr=cases.THR, stride=1, facts=None):
    want = ref.system(grid, depth, mask, intr, pose, thr, stride, facts)
    got = cam_pose_opt.camtrack_system(vol, depth, mask, intr, pose, ctx=ctx, weight_threshold=thr, stride=stride)
    assert got.dtype == np.int64 and [int(v) for v in got] == want, (got.tolist(), want)
    return want


def down(x, y, z):
    P = DOWN.copy()
    P[:3, 3] = (x, y, z)
    return P


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_sums_of_the_tracking_scene(ctx, scene, stride):
    vol, grid, d, T, m = scene
    for pose in (T[cases.TRACKED], cases.tracking_start("a")[0]):
        s = same(ctx, vol, grid, d[cases.TRACKED], m, K, pose, stride=stride)
        assert s[28] > 40000 // (stride * stride)


def test_a_67_by_5_frame(ctx, scene):
    vol, grid, d, T, m = scene
    crop = np.ascontiguousarray(d[cases.TRACKED][100:105, 100:167])
    intr = K.copy()
    intr[0, 2] -= 100
    intr[1, 2] -= 100
    for stride in (1, 2, 4):
        assert same(ctx, vol, grid, crop, np.ones_like(crop, np.uint8), intr, T[cases.TRACKED], stride=stride)[28] > 0


def test_no_valid_pixel_gives_zeros(ctx, scene):
    vol, grid, d, T, m = scene
    assert same(ctx, vol, grid, np.zeros_like(d[0]), m, K, T[cases.TRACKED]) == [0] * 29
    assert same(ctx, vol, grid, d[cases.TRACKED], np.zeros_like(m), K, T[cases.TRACKED]) == [0] * 29


def test_depth_0_3000_and_3001(ctx, scene):
    """From 3 m above, 3000 mm lands on the slab's top; 0 and 3001 are invalid."""
    vol, grid, d, T, m = scene
    depth = np.zeros((8, 48), np.uint16)
    depth[:, 16:32], depth[:, 32:] = 3000, 3001
    intr = np.array([[4000.0, 0, 23.5], [0, 4000.0, 3.5], [0, 0, 1]])
    facts = {}
    s = same(ctx, vol, grid, depth, np.ones_like(depth, np.uint8), intr, down(-0.06, 0.06, 3.0), facts=facts)
    print(facts)
    assert facts["valid"] == 8 * 16 and 0 < s[28] <= 8 * 16


def test_cells_at_and_beyond_the_last_voxel_of_each_axis(ctx, scene):
    vol, grid, d, T, m = scene
    vx = float(grid.voxel)
    hi = (grid.lo + grid.nv).astype(np.float64) * vx
    depth = np.full((24, 24), 250, np.uint16)
    intr = np.array([[125.0, 0, 11.0], [0, 125.0, 11.0], [0, 0, 1]])         # a pixel is 2 mm at 0.25 m: the frame spans 48 mm
    facts = {}
    for pose in (down(hi[0] - 0.02, 0.0, 0.25), down(0.0, hi[1] - 0.02, 0.25), down(0.0, 0.0, hi[2] + 0.25 - 0.0021), down(0.0, 0.0, hi[2] + 0.2503)):
        same(ctx, vol, grid, depth, np.ones_like(depth, np.uint8), intr, pose, facts=facts)
    print(facts)
    assert (facts["last_cell"] > 0).all() and (facts["outside"] > 0).all()


def test_negative_coordinates_and_points_on_voxel_planes(ctx, scene):
    vol, grid, d, T, m = scene
    depth = np.full((40, 40), 250, np.uint16)
    intr = np.array([[125.0, 0, 20.0], [0, 125.0, 20.0], [0, 0, 1]])
    facts = {}
    s = same(ctx, vol, grid, depth, np.ones_like(depth, np.uint8), intr, down(0.0, 0.0, 0.25), facts=facts)
    print(facts)
    assert facts["frac0"][2] > 0 and (facts["negative"][:2] > 0).all() and s[28] > 0


def test_weights_at_the_threshold_and_one_below(ctx, scene):
    """Three frames were fused: a cell all three saw has weights exactly 3."""
    vol, grid, d, T, m = scene
    counts = [same(ctx, vol, grid, d[cases.TRACKED], m, K, T[cases.TRACKED], thr=thr, stride=2)[28] for thr in (1.0, 2.0, 3.0, 3.5, 4.0)]
    print(counts)
    assert counts[0] > counts[1] > counts[2] > 0 and counts[3] == counts[4] == 0


def test_phi_exactly_one_does_not_contribute(ctx, scene):
    vol, grid, d, T, m = scene
    facts = {}
    same(ctx, vol, grid, d[cases.TRACKED], m, K, cases.tracking_start("b")[0], facts=facts)
    assert facts["phi_pm1"] > 0, facts


def test_a_1280_by_720_frame_with_every_pixel_valid(ctx, scene):
    vol, grid, d, T, m = scene
    intr = K.copy()
    intr[:2] *= 4
    intr[0, 2], intr[1, 2] = 639.5, 359.5
    big = cases.raycast(np.asarray(T[cases.TRACKED], np.float64), 1280, 720, intr)
    assert (big > 0).all()
    s = same(ctx, vol, grid, big, np.ones_like(big, np.uint8), intr, T[cases.TRACKED])
    assert s[28] > 300000


def test_two_calls_give_the_same_bytes(ctx, scene):
    vol, grid, d, T, m = scene
    a = cam_pose_opt.camtrack_system(vol, d[cases.TRACKED], m, K, T[cases.TRACKED], ctx=ctx)
    b = cam_pose_opt.camtrack_system(vol, d[cases.TRACKED], m, K, T[cases.TRACKED], ctx=ctx)
    assert a.tobytes() == b.tobytes()


def test_a_volume_padded_by_empty_blocks_gives_the_same_sums(ctx):
    """Both volumes are fused from the pixels whose point lies 4 mm inside the bounds: the band of every such pixel stays in the tight
    grid (the bounds padded by the truncation distance), so the four blocks the wide grid adds on every side stay empty."""
    d, T, m = cases.tracking_frames()
    jj, ii = np.meshgrid(np.arange(cases.W), np.arange(cases.H))
    masks = []
    for k in range(cases.N_FUSED):
        z = d[k].astype(np.float64) / 1000
        pc = np.stack([(jj - K[0, 2]) / K[0, 0] * z, (ii - K[1, 2]) / K[1, 1] * z, z], -1)
        pw = pc @ T[k][:3, :3].astype(np.float64).T + T[k][:3, 3].astype(np.float64)
        masks.append(((pw >= cases.BOUNDS[0] + 0.004) & (pw <= cases.BOUNDS[1] - 0.004)).all(-1).astype(np.uint8))
    pad = 4 * 16 * 0.002
    vols = [TsdfVolume(ctx, b) for b in (cases.BOUNDS, cases.BOUNDS + np.array([[-pad] * 3, [pad] * 3]))]
    try:
        for vol in vols:
            for k in range(cases.N_FUSED):
                vol.integrate(d[k], masks[k], K, T[k], 1)
        tight, wide = vols
        assert tuple(wide.grid()[1]) != tuple(tight.grid()[1])
        (ca, ta, wa), (cb, tb, wb) = tight.read_voxels(), wide.read_voxels()
        assert ca.tolist() == cb.tolist() and ta.tobytes() == tb.tobytes() and wa.tobytes() == wb.tobytes()       # the padding is empty
        for stride in (1, 3):
            a = cam_pose_opt.camtrack_system(tight, d[cases.TRACKED], m, K, T[cases.TRACKED], ctx=ctx, stride=stride)
            b = cam_pose_opt.camtrack_system(wide, d[cases.TRACKED], m, K, T[cases.TRACKED], ctx=ctx, stride=stride)
            assert a.tolist() == b.tolist() and a[28] > 0
    finally:
        for vol in vols:
            vol.close()


def test_a_colour_volume_is_accepted(ctx, scene):
    vol, grid, d, T, m = scene
    col = TsdfVolume(ctx, cases.BOUNDS)
    try:
        for k in range(cases.N_FUSED):
            col.integrate_rgb(d[k], m, np.zeros((cases.H, cases.W, 3), np.uint8), K, T[k], 1)
        a = cam_pose_opt.camtrack_system(col, d[cases.TRACKED], m, K, T[cases.TRACKED], ctx=ctx, stride=2)
        assert a.tolist() == cam_pose_opt.camtrack_system(vol, d[cases.TRACKED], m, K, T[cases.TRACKED], ctx=ctx, stride=2).tolist()
    finally:
        col.close()


# ---------------------------------------------------------------------------------------------------- the loop

def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    key = lambda x: np.where(x.view(np.int32) < 0, np.int32(-2 ** 31) - x.view(np.int32), x.view(np.int32)).astype(np.int64)
    return int(np.abs(key(a) - key(b)).max())


@pytest.mark.parametrize("name", sorted(cases.TRACKING))
def test_the_loop_iteration_by_iteration_and_what_it_reaches(ctx, scene, name):
    vol, grid, d, T, m = scene
    start, dt, angle = cases.tracking_start(name)
    pose, rep = cam_pose_opt.refine_cam_pose(vol, d[cases.TRACKED], m, K, start, ctx=ctx, stride=2, trace=True)
    want_pose, want = ref.refine(grid, d[cases.TRACKED], m, K, start, cases.THR, 2)
    assert rep["status"] == want["status"] and rep["iters"] == want["iters"]
    np.testing.assert_array_equal(rep["poses"][0].view(np.uint32), start.view(np.uint32))
    chain = [[float(x) for x in row] for row in start[:3]]          # the pose carried in fp64, stepped by the restatement from the reported sums
    for it in range(rep["iters"]):
        sums = ref.system(grid, d[cases.TRACKED], m, K, rep["poses"][it], cases.THR, 2)
        assert [int(v) for v in rep["sums"][it]] == sums, it
        chain = ref.apply(ref.exp_twist(ref.solve(sums)), chain)
        nxt = rep["poses"][it + 1] if it + 1 < rep["iters"] else pose
        assert _ulps(ref._round(chain), nxt) <= 1, it
        assert _ulps(want["poses"][it], rep["poses"][it]) <= 1, it
    assert _ulps(want_pose, pose) <= 1
    assert rep["pixels_first"] == want["pixels_first"] and rep["pixels_last"] == want["pixels_last"]
    assert abs(rep["rms_first"] - want["rms_first"]) <= 1e-12 and abs(rep["rms_last"] - want["rms_last"]) <= 1e-12
    et, er = ref.pose_error(pose, T[cases.TRACKED])
    print(name, rep["status"], rep["iters"], "rms", rep["rms_first"], rep["rms_last"], "perturbation", dt, angle, "left", et, er,
          "timing ms", cam_pose_opt.camtrack_timing(ctx))
    assert rep["status"] == "converged" and rep["rms_last"] < rep["rms_first"] and et <= 0.5 * dt and er <= 0.5 * angle


def test_too_few_pixels_returns_the_input_pose_bit_for_bit(ctx, scene):
    vol, grid, d, T, m = scene
    start, _, _ = cases.tracking_start("a")
    pose, rep = cam_pose_opt.refine_cam_pose(vol, d[cases.TRACKED], m, K, start, ctx=ctx, stride=2, min_pixels=10 ** 6, trace=True)
    assert rep["status"] == "too_few" and rep["iters"] == 1 and rep["pixels_first"] == rep["pixels_last"] > 0
    np.testing.assert_array_equal(pose.view(np.uint32), start.view(np.uint32))


def test_max_iters_is_reported(ctx, scene):
    vol, grid, d, T, m = scene
    start, _, _ = cases.tracking_start("a")
    pose, rep = cam_pose_opt.refine_cam_pose(vol, d[cases.TRACKED], m, K, start, ctx=ctx, stride=2, max_iters=2, trace=True)
    want_pose, want = ref.refine(grid, d[cases.TRACKED], m, K, start, cases.THR, 2, 2)
    assert rep["status"] == want["status"] == "max_iters" and rep["iters"] == 2 and _ulps(want_pose, pose) <= 1


def test_the_scan_keeps_the_anchor_and_refines_the_rest(ctx):
    d, T, m = cases.tracking_frames()
    given = T.copy()
    given[cases.TRACKED] = cases.tracking_start("a")[0]
    out, reports = cam_pose_opt.refine_cam_poses(d.astype(np.float32) / 1000, given, K, np.zeros_like(d, np.uint8), cases.BOUNDS, ctx=ctx, stride=2)
    assert out.dtype == np.float32 and out.shape == (4, 4, 4) and len(reports) == 4
    np.testing.assert_array_equal(out[0].view(np.uint32), given[0].view(np.uint32))
    assert reports[0]["status"] == "anchor" and all(r["fused"] for r in reports)
    before, after = ref.pose_error(given[cases.TRACKED], T[cases.TRACKED]), ref.pose_error(out[cases.TRACKED], T[cases.TRACKED])
    print("scan:", [r["status"] for r in reports], before, after)
    assert after[0] < before[0]


# ---------------------------------------------------------------------------------------------------- refusals

def test_refusals_leave_outputs_alone_and_the_context_usable(ctx, scene):
    import torch
    vol, grid, d, T, m = scene
    lib = _lib.load()
    depth, mask = np.ascontiguousarray(d[cases.TRACKED]), m
    Kf = np.ascontiguousarray(K.reshape(9), np.float32)
    pose = np.ascontiguousarray(T[cases.TRACKED].reshape(16), np.float32)
    p = _lib.ptr
    sums = np.full(29, -7, np.int64)
    out = np.full(16, -7, np.float32)
    rep = cam_pose_opt.CamtrackReport()
    rep.status = -7
    good = cam_pose_opt.CamtrackParams(1.0, 1, 20, 500)

    def system(**over):
        a = dict(ctx=ctx.h, vol=vol.h, depth=p(depth), mask=p(mask), w=cases.W, h=cases.H, K=p(Kf), pose=p(pose), thr=1.0, stride=1, sums=p(sums))
        a.update(over)
        return lib.d2r_camtrack_system(a["ctx"], a["vol"], a["depth"], a["mask"], a["w"], a["h"], a["K"], a["pose"], a["thr"], a["stride"], a["sums"])

    def refine(params=good, **over):
        a = dict(ctx=ctx.h, vol=vol.h, depth=p(depth), mask=p(mask), w=cases.W, h=cases.H, K=p(Kf), pose=p(pose), params=None if params is None else C.byref(params), out=p(out),
                 rep=C.byref(rep))
        a.update(over)          # (rep=None, out=None: null pointers)
        return lib.d2r_camtrack_refine(a["ctx"], a["vol"], a["depth"], a["mask"], a["w"], a["h"], a["K"], a["pose"], a["params"], a["out"], a["rep"])

    scaled, nan, skew = pose.copy(), pose.copy(), pose.copy()
    scaled[:12] *= np.float32(1.001)
    nan[3] = np.nan
    skew[15] = 2.0
    bad = [dict(ctx=None), dict(vol=None), dict(depth=None), dict(mask=None), dict(K=None), dict(pose=None), dict(pose=p(scaled)),
           dict(pose=p(nan)), dict(pose=p(skew)), dict(stride=0), dict(w=0), dict(h=0), dict(w=2048, h=1025), dict(thr=0.0), dict(thr=-1.0),
           dict(thr=float("nan"))]
    for over in bad:
        assert system(**over) == -1, over
        over = {("params" if k in ("thr", "stride") else k): v for k, v in over.items()}
        if "params" in over:
            continue
        assert refine(**over) == -1, over
    assert system(sums=None) == -1 and refine(out=None) == -1 and refine(rep=None) == -1 and refine(params=None) == -1
    for params in (cam_pose_opt.CamtrackParams(0.0, 1, 20, 500), cam_pose_opt.CamtrackParams(1.0, 0, 20, 500),
                   cam_pose_opt.CamtrackParams(1.0, 1, 0, 500), cam_pose_opt.CamtrackParams(1.0, 1, 65, 500)):
        assert refine(params=params) == -1
    assert b"max_iters" in lib.d2r_last_error(ctx.h)
    if torch.cuda.device_count() > 1:
        from dream2real_amd import engine
        other = engine.Context(1)
        assert system(ctx=other.h) == -1 and refine(ctx=other.h) == -1 and b"another device" in lib.d2r_last_error(other.h)
        other.close()
    assert (sums == -7).all() and (out == -7).all() and rep.status == -7 and rep.iters == 0
    ms = np.zeros(3)
    fresh_lib_ctx = C.c_void_p()
    assert lib.d2r_ctx_create(0, C.byref(fresh_lib_ctx)) == 0
    assert lib.d2r_camtrack_get_timing(fresh_lib_ctx, p(ms)) == -1 and lib.d2r_camtrack_get_timing(ctx.h, None) == -1
    lib.d2r_ctx_destroy(fresh_lib_ctx)
    assert system() == 0 and sums[28] > 0 and refine() == 0 and rep.status == 0
    assert lib.d2r_camtrack_get_timing(ctx.h, p(ms)) == 0 and (ms >= 0).all() and ms[1] > 0
