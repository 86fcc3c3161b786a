"""The ablation's visual clouds built on the GPU (d2r_pcd_build, pcdbuild.hip) against the host rule they restate
(pcd_visual_model.erode_rect / backproject / crop / voxel_down_sample / get_vis_pcds): every comparison is exact, positions
as float32 and colours as uint8."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import pcd_build_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _build(ctx, c, voxel, views=pc.VIEWS, obj_ids=pc.OBJ_IDS, bounds=None, keep=False):
    from dream2real_amd import _lib
    hs = _lib.pcd_build(ctx, c["rgb"], c["d16"], c["labels"].astype(np.uint8), c["poses"], c["K"], c["bounds"] if bounds is None else bounds,
                        voxel, list(views), list(obj_ids))
    clouds = [_lib.pcd_read(ctx, h) for h in hs]
    if keep:
        return clouds, hs
    for h in hs:
        _lib.load().d2r_pcd_destroy(h)
    return clouds


def _same(got, want):
    assert len(got) == len(want)
    for (gx, gc), (wx, wc) in zip(got, want):
        assert gx.dtype == np.float32 and gc.dtype == np.uint8
        np.testing.assert_array_equal(gx, wx)
        np.testing.assert_array_equal(gc, wc)


@pytest.mark.parametrize("voxel", pc.VOXELS)
@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_small_shapes_equal_the_host_rule(ctx, shape, voxel):
    """Three labels (one touching all four borders), two views with different poses out of three frames, the objects asked for
    out of label order.  What makes the comparison worth something is asserted on the host result first."""
    want, facts = pc.expected(*shape, voxel)
    assert facts["points"] > pc.SORT_TILE                       # more than one tile of the sort
    assert all(n > 0 for n in facts["sizes"])                   # every requested object has a cloud
    if voxel == 0.002:
        assert facts["max_index"] > 255                         # a voxel index needs a second digit pass
    if voxel == 0.02:
        assert facts["fullest"] > 64                            # a voxel's sum runs past one wave's worth of points
    print(f"[pcd build] {shape} voxel {voxel}: {facts}")
    _same(_build(ctx, pc.case(*shape), voxel), want)


@pytest.fixture(scope="module")
def full_frame():
    """One 1280 x 720 frame: tests/masks_cases' seeded depth, pose and bounds, three rectangular objects on a background."""
    from tests import masks_cases as mc
    w, h = 1280, 720
    d16, K = mc.scene_frame(w, h, 14)
    depth = ((d16.astype(np.float64) + 0.25) / 1000.0).astype(np.float32)
    depth[d16 == 0] = 0
    rng = np.random.default_rng(5)
    labels = np.zeros((h, w), np.int64)
    labels[60:610, 100:1100] = 1
    labels[200:500, 300:700] = 2
    labels[630:700, 40:1250] = 3
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    c = dict(rgbs=[rgb], depths=[depth], d16=(depth * 1000).astype(np.uint16)[None], labels=labels[None],
             poses=mc.SCENE_POSE.astype(np.float64)[None], K=K, bounds=mc.SCENE_BOUNDS, rgb=rgb[None])
    assert (c["d16"][0] == d16).all()
    return c


def test_one_full_frame_at_two_millimetres(ctx, full_frame):
    ids = (0, 1, 2, 3)
    want = pc.host_clouds(pc.host_segments(full_frame, 0.002, views=(0,), obj_ids=ids))
    assert sum(x.shape[0] for x, _ in want) > 10000 and all(x.shape[0] for x, _ in want)
    _same(_build(ctx, full_frame, 0.002, views=(0,), obj_ids=ids), want)


def _flat(w=40, h=24, mm=500):
    """One label over the whole frame (the frame border does not erode), identity pose, the principal point on a pixel."""
    rng = np.random.default_rng(3)
    depth = np.full((h, w), np.float32((mm + 0.25) / 1000.0), np.float32)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    K = np.array([[50.0, 0.0, 20.0], [0.0, 50.0, 10.0], [0.0, 0.0, 1.0]])
    return dict(rgbs=[rgb], depths=[depth], d16=(depth * 1000).astype(np.uint16)[None], labels=np.zeros((1, h, w), np.int64),
                poses=np.eye(4)[None], K=K, bounds=np.array([[-10.0, -10, -10], [10.0, 10, 10]]), rgb=rgb[None])


@pytest.mark.parametrize("voxel", (0.0, 0.002))
def test_hand_vectors(ctx, voxel):
    c = _flat()
    h, w = c["d16"].shape[1:]
    # a label no pixel carries, next to one that every pixel carries
    got = _build(ctx, c, voxel, views=(0,), obj_ids=(9, 0))
    assert got[0][0].shape == (0, 3) and got[0][1].shape == (0, 3)
    _same(got, pc.host_clouds(pc.host_segments(c, voxel, views=(0,), obj_ids=(9, 0))))
    if voxel == 0.0:
        assert got[1][0].shape[0] == h * w
    # no depth anywhere: empty clouds
    z = dict(c, depths=[np.zeros_like(c["depths"][0])], d16=np.zeros_like(c["d16"]))
    assert [x.shape[0] for x, _ in _build(ctx, z, voxel, views=(0,), obj_ids=(0, 9))] == [0, 0]
    # d16 = 0 is dropped: 0.0004 m becomes 0 mm
    d = dict(c, depths=[c["depths"][0].copy()])
    d["depths"][0][3, 5] = 0.0004
    d["d16"] = (d["depths"][0] * 1000).astype(np.uint16)[None]
    assert d["d16"][0, 3, 5] == 0
    got = _build(ctx, d, voxel, views=(0,), obj_ids=(0,))
    _same(got, pc.host_clouds(pc.host_segments(d, voxel, views=(0,), obj_ids=(0,))))
    if voxel == 0.0:
        assert got[0][0].shape[0] == h * w - 1
    # a point exactly on a bound is kept: x = 0 in column cx = 20, z = the one depth value of the frame
    zval = float(np.float32(np.float32(500) / np.float32(1000)))
    b = np.array([[0.0, -10.0, zval], [10.0, 10.0, zval]])
    want = pc.host_clouds(pc.host_segments(c, voxel, views=(0,), obj_ids=(0,), bounds=b))
    got = _build(ctx, c, voxel, views=(0,), obj_ids=(0,), bounds=b)
    _same(got, want)
    if voxel == 0.0:
        assert got[0][0].shape[0] == h * (w - 20) and (got[0][0][:, 0] == 0).sum() == h and (got[0][0][:, 2] == np.float32(zval)).all()


def test_two_calls_are_byte_identical(ctx):
    c = pc.case(130, 70)
    for voxel in (0.0, 0.002):
        a, b = _build(ctx, c, voxel), _build(ctx, c, voxel)
        for (ax, ac), (bx, bc) in zip(a, b):
            assert ax.tobytes() == bx.tobytes() and ac.tobytes() == bc.tobytes()


@pytest.mark.parametrize("pcds_type", (0, 1))
def test_get_vis_pcds_with_a_context_equals_the_host_path(ctx, tmp_path, pcds_type):
    from dream2real_amd import pcd_visual_model as pvm
    c = pc.case(130, 70)
    args = (c["rgbs"], c["depths"], list(c["poses"]), c["K"], list(c["labels"]), 3, c["bounds"])
    kw = dict(use_cache=False, pcds_type=pcds_type, single_view_idx=2)
    host = pvm.get_vis_pcds(*args, save_dir=str(tmp_path / "host"), **kw)
    dev = pvm.get_vis_pcds(*args, save_dir=str(tmp_path / "dev"), ctx=ctx, **kw)
    assert all(len(p) for p in host)
    for a, b in zip(host, dev):
        assert isinstance(b, pvm.PointCloud)
        np.testing.assert_array_equal(a.xyz, b.xyz)
        np.testing.assert_array_equal(a.rgb, b.rgb)
    names = sorted(os.listdir(tmp_path / "host"))
    assert names == sorted(os.listdir(tmp_path / "dev")) == ["obj_vis_0.pcd", "obj_vis_1.pcd", "obj_vis_2.pcd"]
    for n in names:
        assert open(tmp_path / "host" / n, "rb").read() == open(tmp_path / "dev" / n, "rb").read()


def test_built_handles_render_like_uploaded_clouds(ctx):
    """d2r_pcd_render takes d2r_pcd_build's handles as they are: the same frames as the read-back points uploaded again."""
    from dream2real_amd import _lib
    lib = _lib.load()
    c = pc.case(130, 70)
    clouds, hs = _build(ctx, c, 0.002, keep=True)
    up = []
    for xyz, rgb in clouds:
        h = C.c_void_p()
        ctx.check(lib.d2r_pcd_create(ctx.h, _lib.ptr(xyz), _lib.ptr(rgb), C.c_uint32(xyz.shape[0]), C.byref(h)))
        up.append(h)
    view = _lib.PcdView(96, 64, 60.0, 60.0, 47.5, 31.5, 3.0, 0.01)
    centre = np.concatenate([x for x, _ in clouds]).mean(0)
    cam = np.eye(4, dtype=np.float32)
    cam[:3, 3] = centre - [0, 0, 1.5]
    eye = np.eye(4, dtype=np.float32)
    poses = np.stack([eye, eye]).reshape(2, 16).copy()
    poses[1, 3] = 0.05
    frames = []
    for bg, mv in ((hs[1], hs[0]), (up[1], up[0])):
        f = np.empty((2, 64, 96, 3), np.uint8)
        ctx.check(lib.d2r_pcd_render(ctx.h, bg, mv, C.byref(view), _lib.ptr(cam.reshape(16)), _lib.ptr(eye.reshape(16)), _lib.ptr(poses),
                                     C.c_uint32(2), _lib.ptr(f)))
        frames.append(f)
    for h in list(hs) + up:
        lib.d2r_pcd_destroy(h)
    assert (frames[0] != 0).any() and not (frames[0][0] == frames[0][1]).all()      # points land, the movable cloud moves
    np.testing.assert_array_equal(frames[0], frames[1])
    up_ms, dev_ms = _lib.pcd_build_timing(ctx)
    assert up_ms >= 0 and dev_ms > 0
