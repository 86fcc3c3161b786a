"""d2r_labeltrack_scan against the numpy restatement of DESIGN.md section 2k (tests/labeltrack_ref.py): the label images, the
statistics and the volume are compared by equality of every byte."""
import ctypes as C

import numpy as np
import pytest

from dream2real_amd import _lib, segmentation
from tests import labeltrack_cases as lc
from tests import labeltrack_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _K(k4):
    return np.array([[k4[0], 0, k4[2]], [0, k4[1], k4[3]], [0, 0, 1]], np.float64)


def _gpu(ctx, d16, poses, k4, labels0, bounds=lc.BOUNDS, **params):
    out, stats, (vol, dims, lo) = segmentation.track_labels(d16, poses, _K(k4), labels0, bounds, ctx=ctx, return_stats=True, return_volume=True,
                                                            **params)
    return out, stats, vol, dims, lo


def _same(got, want, what=""):
    for name, g, w in zip(("labels", "stats", "vol", "dims", "lo"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        diff = np.argwhere(g != w)
        assert len(diff) == 0, f"{what} {name}: {len(diff)} entries differ, the first at {diff[0].tolist()}: {g[tuple(diff[0])]} for {w[tuple(diff[0])]}"


def _check(ctx, d16, poses, k4, labels0, bounds=lc.BOUNDS, **params):
    got = _gpu(ctx, d16, poses, k4, labels0, bounds, **params)
    want = ref.scan(d16, poses, k4, labels0, bounds, **params)
    _same(got, want, str(params))
    return want


def test_scene_at_the_defaults(ctx):
    d16, truth, poses = lc.frames(4)
    want = lc.reference(4)
    _same(_gpu(ctx, d16, poses, lc.K4, truth[0]), want)
    stats = want[1]
    assert (stats[1:, 0] > 20000).all() and (stats[1:, 1] > 20000).all() and (stats[1:, 3] == 8).all()       # predicted, filled, all 8 launches grew
    acc, _ = lc.accuracy(want[0], truth)
    assert acc.min() > 0.99


def test_scene_at_a_finer_voxel_and_the_narrowest_band(ctx):
    d16, truth, poses = lc.frames(4)
    _same(_gpu(ctx, d16, poses, lc.K4, truth[0], voxel=0.002, band_voxels=1), lc.reference(4, 0.002, 1))


@pytest.mark.parametrize("grow", [0, 1, 7, 8, 9, 17, 100])
def test_a_frame_with_tails_in_every_tiling(ctx, grow):
    """65 x 17: two tiles along x, the second one pixel wide; grow on both sides of the 8 sweeps of a launch and of two launches, and
    larger than the frame (the fill reaches its fixed point and the later launches return at once)."""
    d16, truth, poses, k4 = lc.crop()
    want = _check(ctx, d16, poses, k4, truth[0], grow=grow)
    launches = -(-grow // ref.SWEEPS_PER_LAUNCH)
    assert (want[1][1:, 3] <= launches).all()
    if grow == 0:
        assert (want[1][1:, 1] == 0).all()
    if grow == 100:
        assert (want[1][1:, 3] < launches).all() and (want[1][1:, 1] > 0).all()


def test_a_hole_without_depth_on_a_silhouette(ctx):
    """Three columns without depth across the box's left silhouette in frames 1 and 2: the hole's pixels take a label from
    whichever side reaches them first and hand it to nothing that has depth."""
    d16, truth, poses = lc.frames(3)
    d16 = d16.copy()
    for f in (1, 2):
        rows = np.nonzero((truth[f] == lc.BOX).any(axis=1))[0]
        r0, r1 = rows[len(rows) // 4], rows[3 * len(rows) // 4]
        j = int(np.nonzero(truth[f][(r0 + r1) // 2] == lc.BOX)[0][0])
        d16[f, r0:r1, j - 1:j + 2] = 0
    want = _check(ctx, d16, poses, lc.K4, truth[0])
    hole = d16[1] == 0
    assert hole.sum() >= 3 * 10 and (want[0][1][hole] == lc.BOX).any()          # the hole was labelled, in part as the box


def test_a_frame_of_zero_depth_changes_nothing(ctx):
    d16, truth, poses = lc.frames(4)
    d16 = d16.copy()
    d16[1] = 0
    want = _check(ctx, d16, poses, lc.K4, truth[0])
    assert want[1][1].tolist() == [0, 0, lc.W * lc.H, 0] and not want[0][1].any()
    keep = [0, 2, 3]
    without = _gpu(ctx, np.ascontiguousarray(d16[keep]), np.ascontiguousarray(poses[keep]), lc.K4, truth[0])
    assert np.array_equal(without[0][1:], want[0][2:]) and np.array_equal(without[1][1:], want[1][2:]) and np.array_equal(without[2], want[2])


def test_a_pose_that_looks_away_from_the_grid(ctx):
    d16, truth, poses = lc.frames(4)
    poses = poses.copy()
    poses[2, :3, 1:3] *= -1                         # turned by 180 degrees about its own x axis: the scene is behind the camera
    want = _check(ctx, d16, poses, lc.K4, truth[0])
    assert want[1][2].tolist() == [0, 0, lc.W * lc.H, 0] and want[1][3][0] > 20000


def test_label_254(ctx):
    d16, truth, poses = lc.frames(3)
    labels0 = np.where(truth[0] == lc.SPHERE_B, 254, truth[0]).astype(np.uint8)
    want = _check(ctx, d16, poses, lc.K4, labels0)
    assert (want[0][2] == 254).sum() > 100 and ((want[2] & 255) == 254).any()


@pytest.mark.parametrize("tau_mm", [0, 65535])
def test_tau_at_both_ends_of_its_range(ctx, tau_mm):
    d16, truth, poses = lc.frames(3)
    want = _check(ctx, d16, poses, lc.K4, truth[0], tau_mm=tau_mm)
    base = lc.reference(3)
    assert not np.array_equal(want[0], base[0])
    if tau_mm == 0:
        assert (want[1][1:, 1] < base[1][1:, 1]).all()          # only pixels of equal depth, and pixels without depth, receive


def _plane_frame(T, k4, n=16):
    """The plane z = 0 seen from T -> uint16 [n,n] millimetres"""
    jj, ii = np.meshgrid(np.arange(n), np.arange(n))
    d = np.stack([(jj - k4[2]) / k4[0], (ii - k4[3]) / k4[1], np.ones((n, n))], -1) @ T[:3, :3].T
    t = -T[2, 3] / d[..., 2]
    return np.round(t * 1000).astype(np.uint16)


def test_counts_saturate_come_down_and_the_label_is_replaced(ctx):
    """16 x 16 frames of the plane z = 0, grow 0.  300 copies of a view straight down, the left half labelled 1 and the right half 2:
    the counts of the voxels in the band reach 255 and stay.  Then 256 copies of a nearer view from 45 degrees on the right-hand side: a voxel
    one below the plane on the left of the labels' edge projects, along the oblique ray, onto a pixel that shows the plane one voxel
    further right, which carries label 2; 255 such votes bring its count to 0 and the 256th replaces the label."""
    k4 = np.array([50.0, 50.0, 8.0, 8.0])           # straight down from 0.2 m a pixel is a 4 mm voxel, centre on centre: the first phase is at rest
    down = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0.2], [0, 0, 0, 1]], np.float64)
    s = np.sqrt(0.5)
    side = np.array([[s, 0, -s, 0.1 * s], [0, -1, 0, 0], [-s, 0, -s, 0.1 * s], [0, 0, 0, 1]], np.float64)
    assert np.allclose(side[:3, :3].T @ side[:3, :3], np.eye(3)) and np.isclose(np.linalg.det(side[:3, :3]), 1)
    n1, n2 = 300, 256
    d16 = np.concatenate([np.repeat(_plane_frame(down, k4)[None], n1, 0), np.repeat(_plane_frame(side, k4)[None], n2, 0)])
    poses = np.concatenate([np.repeat(down[None], n1, 0), np.repeat(side[None], n2, 0)]).astype(np.float32)
    labels0 = np.ascontiguousarray(np.broadcast_to(np.where(np.arange(16) < 8, 1, 2).astype(np.uint8), (16, 16)))
    bounds = np.array([[-0.032, -0.032, -0.008], [0.032, 0.032, 0.008]])
    first = ref.scan(d16[:n1], poses[:n1], k4, labels0, bounds, grow=0)
    want = ref.scan(d16, poses, k4, labels0, bounds, grow=0)
    full = (first[2] >> 8) == 255
    assert full.sum() >= 16 and ((first[2] >> 8) <= 255).all()                                   # saturated, not wrapped
    emptied = full & ((want[2] >> 8) < 255)
    replaced = full & ((first[2] & 255) != (want[2] & 255)) & ((want[2] >> 8) >= 1)          # from 255: 255 opposing votes to 0, one more replaces
    print(f"saturated {full.sum()} voxels; of them {emptied.sum()} came down and {replaced.sum()} carry another label after the second phase, "
          f"with counts {np.unique(want[2][replaced] >> 8).tolist()}")
    assert replaced.any() and ((want[2][replaced] >> 8) == 1).any()                            # ... and exactly 256 opposing votes leave count 1
    _same(_gpu(ctx, d16[:n1], poses[:n1], k4, labels0, bounds, grow=0), first, "300 copies")
    _same(_gpu(ctx, d16, poses, k4, labels0, bounds, grow=0), want, "300 + 256")


def test_two_calls_give_the_same_bytes(ctx):
    d16, truth, poses, k4 = lc.crop()
    a = _gpu(ctx, d16, poses, k4, truth[0])
    b = _gpu(ctx, d16, poses, k4, truth[0])
    _same(a, b)
    ms = segmentation.labeltrack_timing(ctx)
    assert len(ms) == 3 and all(np.isfinite(m) and m >= 0 for m in ms)


def test_every_refusal_leaves_the_outputs_untouched_and_the_context_usable(ctx):
    d16, truth, poses, k4 = lc.crop()
    n, h, w = d16.shape
    lib = ctx.lib
    labels0 = np.ascontiguousarray(truth[0])
    bounds = np.ascontiguousarray(lc.BOUNDS.reshape(6), np.float64)
    dims, lo = segmentation.labeltrack_grid(bounds)
    out = np.full((n, h, w), 0xA5, np.uint8)
    stats = np.full((n, 4), 0xA5A5A5A5, np.uint32)
    vol = np.full(int(dims.prod()), 0xA5A5, np.uint16)
    vdims, vlo = np.full(3, 0xA5A5A5A5, np.uint32), np.full(3, -7, np.int32)

    def call(**over):
        a = dict(ctx=ctx.h, bounds=bounds, params=segmentation.LabeltrackParams(0.004, 2, 10, 64), n=n, w=w, h=h, K=np.ascontiguousarray(k4),
                 d16=d16, poses=np.ascontiguousarray(poses.reshape(n, 16)), labels0=labels0, out=out)
        a.update(over)
        p = a["params"]
        keep = [np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x for x in (a["bounds"], a["K"], a["d16"], a["poses"], a["labels0"], a["out"])]
        ptr = lambda x: _lib.ptr(x) if x is not None else None
        return lib.d2r_labeltrack_scan(a["ctx"], ptr(keep[0]), C.byref(p) if p is not None else None, a["n"], a["w"], a["h"], ptr(keep[1]), ptr(keep[2]),
                                       ptr(keep[3]), ptr(keep[4]), ptr(keep[5]), _lib.ptr(stats), _lib.ptr(vol), _lib.ptr(vdims), _lib.ptr(vlo))

    def bad_pose(k, v):
        p = poses.reshape(n, 16).copy()
        p[1, k] = v
        return p

    P = segmentation.LabeltrackParams
    l255 = labels0.copy()
    l255[3, 5] = 255
    inverted = bounds.copy()
    inverted[[0, 3]] = inverted[[3, 0]]
    refusals = {
        "no context": dict(ctx=None), "no bounds": dict(bounds=None), "no params": dict(params=None), "no K": dict(K=None),
        "no depth": dict(d16=None), "no poses": dict(poses=None), "no labels0": dict(labels0=None), "no output": dict(out=None),
        "n = 0": dict(n=0), "w = 0": dict(w=0), "h = 0": dict(h=0), "too many pixels": dict(w=2048, h=1025),
        "a pose that is not rigid": dict(poses=bad_pose(0, 1.5)), "a pose with NaN": dict(poses=bad_pose(3, np.nan)),
        "a pose with a last row": dict(poses=bad_pose(12, 0.1)),
        "fx = 0": dict(K=np.array([0.0, 380, 1, 1])), "fy = inf": dict(K=np.array([380.0, np.inf, 1, 1])), "cx = NaN": dict(K=np.array([380.0, 380, np.nan, 1])),
        "255 in labels0": dict(labels0=l255),
        "voxel 0": dict(params=P(0.0, 2, 10, 64)), "voxel < 0": dict(params=P(-0.004, 2, 10, 64)), "voxel NaN": dict(params=P(float("nan"), 2, 10, 64)),
        "voxel inf": dict(params=P(float("inf"), 2, 10, 64)), "band 0": dict(params=P(0.004, 0, 10, 64)), "band 9": dict(params=P(0.004, 9, 10, 64)),
        "tau 65536": dict(params=P(0.004, 2, 65536, 64)), "grow 4097": dict(params=P(0.004, 2, 10, 4097)),
        "a grid over the cap": dict(params=P(1e-5, 2, 10, 64)), "bounds with NaN": dict(bounds=np.array([np.nan, 0, 0, 1, 1, 1.0])),
        "inverted bounds": dict(bounds=inverted), "bounds beyond 2^23 voxels": dict(bounds=np.array([0, 0, 0, 1e5, 0.01, 0.01])),
    }
    for name, over in refusals.items():
        rc = call(**over)
        assert rc == -1, (name, rc)
        assert (out == 0xA5).all() and (stats == 0xA5A5A5A5).all() and (vol == 0xA5A5).all() and (vdims == 0xA5A5A5A5).all() and (vlo == -7).all(), name
        if over.get("ctx", 1) is not None:
            assert lib.d2r_last_error(ctx.h), name
    d0, l0 = np.full(3, 7, np.uint32), np.full(3, 7, np.int32)
    assert lib.d2r_labeltrack_grid(_lib.ptr(bounds), C.byref(P(0.004, 0, 10, 64)), _lib.ptr(d0), _lib.ptr(l0)) == -1 and (d0 == 7).all() and (l0 == 7).all()
    assert lib.d2r_labeltrack_get_timing(ctx.h, None) == -1 and lib.d2r_labeltrack_get_timing(None, _lib.ptr(np.zeros(3))) == -1
    # the context still works, and the very same buffers are filled now
    assert call() == 0
    want = ref.scan(d16, poses, k4, labels0, lc.BOUNDS)
    _same((out, stats, vol.reshape(want[2].shape), vdims, vlo), want)
