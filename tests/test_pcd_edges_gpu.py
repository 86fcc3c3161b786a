"""The point-cloud renderer (pcd.hip) on the MI355X at its edges: every scene of tests/pcd_edge_cases.py equal to the numpy rule
(tests/pcd_ref.py) bit for bit, d2r_pcd_render in several passes, workspaces reused across views of different sizes, the fused call
off the default view, and every refusal of check_view / pcd_prepare.  tests/test_pcd_edges_host.py proves on the CPU that the scenes
reach the tile grids, rounding edges and culls they are built for."""
import ctypes as C
import types

import numpy as np
import pytest

from dream2real_amd import _lib
from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
from tests import pcd_edge_cases as cases
from tests import pcd_ref
from tests.parity_utils import random_unit_text_embeds

pytestmark = pytest.mark.gpu

PCD_TILE_PX = 4096           # pcd.hip: the "tiles" scenes are built around tw = min(rw, 4096), th = min(rh, 4096 // tw)
D2R_ERR_INVALID, D2R_ERR_UNSUPPORTED = -1, -4           # include/d2r.h


@pytest.fixture(scope="module")
def gpu():
    from dream2real_amd import engine
    from dream2real_amd import pcd_visual_model as pvm
    ctx = engine.Context(0)
    yield types.SimpleNamespace(engine=engine, pvm=pvm, ctx=ctx)
    ctx.close()


class _Task:
    def __init__(self, pvm, case):
        import torch
        bg_xyz, bg_rgb, mv_xyz, mv_rgb, _, _, now, _ = cases.args(case)
        self.task_bground_obj = types.SimpleNamespace(vis_model=pvm.PointCloud(bg_xyz, bg_rgb))
        self.movable_obj = types.SimpleNamespace(vis_model=pvm.PointCloud(mv_xyz, mv_rgb), pose=torch.from_numpy(np.asarray(now, np.float32)))


def _renderer(gpu, view):
    K = np.array([[view.fx, 0, view.cx], [0, view.fy, view.cy], [0, 0, 1]], np.float64)
    return gpu.pvm.PointCloudRenderer(gpu.ctx, view.width, view.height, intrinsics=K, point_size=view.point_size, near=view.near)


def _render(rend, case, task):
    view, cam, poses = case[4], case[5], case[7]
    frames = rend.render(cam, poses, task)
    assert len(frames) == poses.shape[0]
    return np.asarray(frames, np.uint8).reshape(-1, view.height, view.width, 3)


def _render_case(gpu, name):
    case = cases.build(name)
    rend = _renderer(gpu, case[4])
    try:
        task = _Task(gpu.pvm, case)
        got = _render(rend, case, task)
        again = _render(rend, case, task)
    finally:
        rend.close()
    return case, got, again


@pytest.mark.parametrize("name", list(cases.CASES))
def test_edge_scene_equals_the_rule(gpu, name):
    assert cases.TILE_PX == PCD_TILE_PX
    case, got, again = _render_case(gpu, name)
    view, poses = case[4], case[7]
    assert got.shape == (poses.shape[0], view.height, view.width, 3) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, cases.expected(name))
    np.testing.assert_array_equal(again, got)                    # the same bytes twice


def test_render_in_several_passes(gpu):
    name = "sprites-4"
    case = cases.build(name)
    assert case[7].shape[0] == 8
    ctx = gpu.ctx
    rend = _renderer(gpu, case[4])
    chunk = ctx.get_option("chunk")
    try:
        task = _Task(gpu.pvm, case)
        ctx.set_option("chunk", 3)                               # passes of 3, 3 and 2 candidates: mats + k0 with k0 = 3, 6
        assert ctx.get_option("chunk") == 3
        small = _render(rend, case, task)
        ctx.set_option("chunk", 4096)
        one = _render(rend, case, task)
    finally:
        ctx.set_option("chunk", chunk)
        rend.close()
    assert ctx.get_option("chunk") == chunk
    np.testing.assert_array_equal(small, cases.expected(name))
    np.testing.assert_array_equal(small, one)


def test_workspaces_across_views(gpu):
    """A context of its own, so that the 8229 x 5 view is the one that grows pcd_bg_keys, pcd_bg_frame, pcd_cols and frames; the
    smaller views then run in the larger buffers.  A stale key or colour would show in the empty-background frames."""
    names = ["tiles-8229x5-16", "empty-bg0", "sprites-5", "tiles-8229x5-16"]
    ctx = gpu.engine.Context(0)
    own = types.SimpleNamespace(engine=gpu.engine, pvm=gpu.pvm, ctx=ctx)
    try:
        out = [_render_case(own, n)[1] for n in names]
    finally:
        ctx.close()
    for n, got in zip(names, out):
        np.testing.assert_array_equal(got, cases.expected(n))
    assert out[0].tobytes() == out[3].tobytes()
    bg0 = cases.build("empty-bg0")
    _, Mk = pcd_ref.matrices(bg0[5], bg0[6], bg0[7])
    for k, M in enumerate(Mk):      # where no movable sprite lands, the empty background is white, hence black
        hit = pcd_ref.splat(np.full(40 * 30, pcd_ref.EMPTY, np.uint64), M, bg0[2], 0, bg0[4]).reshape(30, 40) != pcd_ref.EMPTY
        assert not out[1][k][~hit].any() and (~hit).sum() > 600


def test_fused_call_off_the_default_view(gpu):
    name = "sprites-2"
    case = cases.build(name)
    view, cam, poses = case[4], case[5], case[7]
    assert (view.width, view.height, view.point_size) == (97, 61, 2.0)
    ctx = gpu.ctx
    cfg = CLIP_CONFIGS["vit_tiny"]
    sc = gpu.engine.ClipScorer(ctx, cfg, random_clip_state_dict(cfg, seed=6, text=False))
    rend = _renderer(gpu, view)
    text = random_unit_text_embeds(cfg["proj"], 3)
    chunk = ctx.get_option("chunk")
    try:
        task = _Task(gpu.pvm, case)
        ctx.set_option("chunk", 3)
        lg, frames = rend.render_score(cam, poses, task, sc, text, return_frames=True)
        two_step = sc.score_frames(frames, text, rot90=True)
        ctx.set_option("chunk", chunk)
        np.testing.assert_array_equal(frames, _render(rend, case, task))
    finally:
        ctx.set_option("chunk", chunk)
        sc.close()
        rend.close()
    np.testing.assert_array_equal(frames, cases.expected(name))
    assert np.isfinite(lg).all() and lg.shape == (8, 3)
    np.testing.assert_array_equal(lg, two_step)


def _view(**kw):
    d = dict(width=40, height=30, fx=32.0, fy=32.0, cx=20.25, cy=14.75, point_size=3.0, near=0.01)
    d.update(kw)
    return _lib.PcdView(d["width"], d["height"], d["fx"], d["fy"], d["cx"], d["cy"], d["point_size"], d["near"])


REFUSALS = [(f"point_size {p}", dict(view=dict(point_size=p)), D2R_ERR_UNSUPPORTED) for p in (0.0, 0.5, 2.5, 17.0, float("nan"))]
REFUSALS += [(f"{k} {v}", dict(view={k: v}), D2R_ERR_INVALID) for k in ("width", "height") for v in (0, 16385)]
REFUSALS += [(f"near {v}", dict(view=dict(near=v)), D2R_ERR_INVALID) for v in (-1.0, float("nan"), float("inf"))]
REFUSALS += [("fx nan", dict(view=dict(fx=float("nan"))), D2R_ERR_INVALID)]
REFUSALS += [(f"null {w}", dict(null=w), D2R_ERR_INVALID) for w in ("view", "cam_pose", "obj_poses", "frames_out")]


def test_refusals(gpu):
    """Every refusal of check_view and pcd_prepare that d2r_pcd_render can be driven to: its code, a message, and nothing written."""
    ctx, lib = gpu.ctx, gpu.ctx.lib
    case = cases.build("empty-K1")
    bg_xyz, bg_rgb, mv_xyz, mv_rgb, view, cam, now, _ = cases.args(case)
    poses = np.ascontiguousarray(np.stack([cases.shift(), cases.shift(0.1, -0.05)]).reshape(-1, 16))
    cam16, now16 = np.ascontiguousarray(cam.reshape(16)), np.ascontiguousarray(now.reshape(16))
    want = pcd_ref.render(bg_xyz, bg_rgb, mv_xyz, mv_rgb, view, cam, now, poses)
    handles = []
    try:
        for xyz, rgb in ((bg_xyz, bg_rgb), (mv_xyz, mv_rgb)):
            h = C.c_void_p()
            ctx.check(lib.d2r_pcd_create(ctx.h, _lib.ptr(np.ascontiguousarray(xyz)), _lib.ptr(np.ascontiguousarray(rgb)), xyz.shape[0], C.byref(h)))
            handles.append(h)
        bg, mv = handles

        def call(v, out, null=None):
            a = dict(view=C.byref(v), cam_pose=_lib.ptr(cam16), obj_poses=_lib.ptr(poses), frames_out=_lib.ptr(out))
            if null:
                a[null] = None
            return lib.d2r_pcd_render(ctx.h, bg, mv, a["view"], a["cam_pose"], _lib.ptr(now16), a["obj_poses"], 2, a["frames_out"])

        before = np.empty((2, 30, 40, 3), np.uint8)
        assert call(_view(), before) == 0
        np.testing.assert_array_equal(before, want)
        for what, kw, code in REFUSALS:
            probe = C.c_int64(0)                                     # a message of another call in d2r_last_error first
            assert lib.d2r_ctx_get_option(ctx.h, b"no_such_option", C.byref(probe)) == D2R_ERR_INVALID
            stale = lib.d2r_last_error(ctx.h)
            assert stale == b"unknown option no_such_option"
            out = np.full((2, 30, 40, 3), 0xA5, np.uint8)
            rc = call(_view(**kw.get("view", {})), out, kw.get("null"))
            msg = lib.d2r_last_error(ctx.h)
            print(f"[refusal] {what}: code {rc}, {msg.decode()!r}")
            assert rc == code, what
            assert msg and msg != stale, what
            assert (out == 0xA5).all(), what
        after = np.empty((2, 30, 40, 3), np.uint8)
        assert call(_view(), after) == 0
        assert after.tobytes() == before.tobytes()
    finally:
        for h in handles:
            lib.d2r_pcd_destroy(h)
