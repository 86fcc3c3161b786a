"""The colour-TSDF ray caster on the GPU at its edges (tests/tsdfvis_edge_cases.py; the facts that make each input an edge are
asserted in tests/test_tsdfvis_edges_host.py): frames and depths against the brute-force restatement, bit for bit, +inf included."""
import ctypes as C

import numpy as np
import pytest

from dream2real_amd import _lib
from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
from dream2real_amd.physics_utils import TsdfVolume
from tests import tsdfvis_cases as cases
from tests import tsdfvis_edge_cases as ec
from tests.parity_utils import random_unit_text_embeds
from tests.test_tsdfvis_gpu import pcd_view, same

pytestmark = pytest.mark.gpu
INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vols(ctx):
    """volume key -> (background, movable) device volumes, fused from the frames the restatement's volumes were fused from."""
    made = {}

    def get(key):
        if key not in made:
            if key[0] == "cases":
                kind = key[1]
                if kind == "twins":
                    made[key] = (cases.fuse(TsdfVolume(ctx, *cases.mv_args()), 1), cases.fuse(TsdfVolume(ctx, *cases.mv_args()), 1, tint=90))
                else:
                    made[key] = (cases.fuse(TsdfVolume(ctx, *cases.bg_args()), 0, skip_band=cases.SKIP_BANDS.get(kind)),
                                 cases.fuse(TsdfVolume(ctx, *cases.mv_args(kind)), 1))
            else:
                made[key] = ec.build(key, lambda b, v, t: TsdfVolume(ctx, b, v, t))
        return made[key]
    yield get
    for pair in made.values():
        for v in pair:
            v.close()


def render(ctx, pair, c, poses=None, depth=True):
    poses = np.ascontiguousarray((c.poses if poses is None else poses).reshape(-1, 16), np.float32)
    K, v = poses.shape[0], c.view
    frames = np.full((K, v.height, v.width, 3), 77, np.uint8)
    dep = np.full((K, v.height, v.width), -1.0, np.float32) if depth else None
    view = pcd_view(v)
    rc = ctx.lib.d2r_tsdfvis_render(ctx.h, pair[0].h, pair[1].h, C.byref(view), _lib.ptr(np.ascontiguousarray(c.cam, np.float32)),
                                    _lib.ptr(np.ascontiguousarray(c.o_now, np.float32)), _lib.ptr(poses), K, c.thr, _lib.ptr(frames), _lib.ptr(dep))
    return rc, frames, dep


def check(ctx, vols, name):
    c = ec.CASES[name]
    rc, frames, dep = render(ctx, vols(c.vol_key), c)
    ctx.check(rc)
    want_f, want_d, _ = ec.expected(name)
    same(frames, want_f, f"{name} frames")
    same(dep, want_d, f"{name} depth")
    return frames, dep


def fused_equal_the_restatement(vols, key):
    """The device volumes hold the restatement's blocks, tsdf, weights and colours: without that a cast cannot be compared."""
    for dev, rvol in zip(vols(key), ec.volumes(key)):
        coords, tsdf, weight = dev.read_voxels()
        rt, rw = rvol.block_voxels()
        same(coords.astype(np.int64), rvol.active_blocks(), f"{key} blocks")
        same(tsdf, rt, f"{key} tsdf"), same(weight, rw, f"{key} weight"), same(dev.read_colours(), rvol.block_colours(), f"{key} colours")


def test_e1_dyadic_axis_aligned_scene(ctx, vols):
    fused_equal_the_restatement(vols, ("dy", "0"))
    for name in ("E1_on_grid", "E1_half_off", "E1_origin_outside"):
        check(ctx, vols, name)


def test_e2_crossing_signs(ctx, vols):
    check(ctx, vols, "E2_on_surface"), check(ctx, vols, "E2_inside")


def test_e3_threshold_equality(ctx, vols):
    for i in range(len(ec.THR_E3)):
        check(ctx, vols, f"E3_thr{i}")


def test_e4_fallback_colour(ctx, vols):
    check(ctx, vols, "E4_fallback")


def test_e5_colour_rounding_and_clamp(ctx, vols):
    check(ctx, vols, "E5_half_colours")


def test_e6_far_from_the_origin(ctx, vols):
    fused_equal_the_restatement(vols, ("sphere",))
    check(ctx, vols, "E6_far")


def test_e7_untouched_block_inside_the_box(ctx, vols):
    fused_equal_the_restatement(vols, ("blocks",))
    check(ctx, vols, "E7_blocks")


def test_e8_view_and_tile_edges(ctx, vols):
    for name in ec.CASES:
        if name.startswith("E8_"):
            check(ctx, vols, name)


def test_e9_ends_of_the_sample_range(ctx, vols):
    for name in ("E9_last_pair", "E9_one_voxel_more", "E9_inside_box"):
        check(ctx, vols, name)


def test_e10_exact_and_near_ties_between_the_volumes(ctx, vols):
    check(ctx, vols, "E10_exact_tie"), check(ctx, vols, "E10_near_tie")


def test_e11_state_across_calls(ctx, vols):
    """48 x 40 with K = 11, then 1 x 1 with K = 1, then 45 x 37 with K = 5 on one context, depth on some calls only, three passes a
    call; the first call repeated at the end gives its first bytes again."""
    pair = vols(("cases", "plain"))
    names = tuple(cases.CANDIDATES)
    big = ec.Case(("cases", "plain"), cases.VIEWS["48x40"], cases.CAM, cases.O_NOW, cases.poses(names))
    one = ec.CASES["E8_1x1"]
    small = ec.Case(("cases", "plain"), cases.VIEWS["45x37"], cases.CAM, cases.O_NOW, cases.poses(cases.SMALL_VIEW_CANDIDATES))
    chunk = ctx.get_option("chunk")
    try:
        ctx.set_option("chunk", 4)                                    # 11 candidates: 4 + 4 + 3
        rc, f1, d1 = render(ctx, pair, big)
        ctx.check(rc)
        want = cases.expected("48x40", names=names)
        same(f1, want[0], "first call frames"), same(d1, want[1], "first call depth")
        rc, f2, _ = render(ctx, vols(one.vol_key), one, poses=one.poses[:1], depth=False)
        ctx.check(rc)
        same(f2, ec.expected("E8_1x1")[0][:1], "1 x 1 frames")
        ctx.set_option("chunk", 2)                                    # 5 candidates: 2 + 2 + 1
        rc, f3, d3 = render(ctx, pair, small)
        ctx.check(rc)
        want3 = cases.expected("45x37", names=tuple(cases.SMALL_VIEW_CANDIDATES))
        same(f3, want3[0], "third call frames"), same(d3, want3[1], "third call depth")
        ctx.set_option("chunk", 4)
        rc, f4, _ = render(ctx, pair, big, depth=False)
        ctx.check(rc)
        same(f4, f1, "the first call again")
    finally:
        ctx.set_option("chunk", chunk)


def test_e12_poses_at_the_rigidity_tolerance(ctx, vols):
    fused_equal_the_restatement(vols, ("dy", "2km"))
    check(ctx, vols, "E12_40m")
    frames, dep = check(ctx, vols, "E12_2km")
    c = ec.CASES["E12_2km"]
    rc, f, d = render(ctx, vols(c.vol_key), c, poses=np.stack([c.poses[0], ec.E12_REFUSED]))
    assert rc == INVALID and b"candidate pose 1" in ctx.lib.d2r_last_error(ctx.h)
    assert (f == 77).all() and (d == -1.0).all()
    rc, f, d = render(ctx, vols(c.vol_key), c)
    ctx.check(rc)
    same(f, frames, "the good call after the refusal")


def test_fused_call_returns_the_plain_calls_frames_on_17x17(ctx, vols):
    from dream2real_amd import engine
    cfg = CLIP_CONFIGS["vit_tiny"]
    sc = engine.ClipScorer(ctx, cfg, random_clip_state_dict(cfg, seed=6, text=False))
    text = random_unit_text_embeds(cfg["proj"], 3)
    c = ec.CASES["E8_17x17"]
    bg, mv = vols(c.vol_key)
    K = len(c.poses)
    poses = np.ascontiguousarray(c.poses.reshape(-1, 16), np.float32)
    lg, frames = np.zeros((K, 3), np.float32), np.zeros((K, 17, 17, 3), np.uint8)
    view = pcd_view(c.view)
    ctx.check(ctx.lib.d2r_tsdfvis_render_score_host(ctx.h, bg.h, mv.h, sc.h, C.byref(view), _lib.ptr(c.cam), _lib.ptr(c.o_now), _lib.ptr(poses), K, c.thr,
                                                    _lib.ptr(text), 3, sc.logit_scale, _lib.ptr(lg), _lib.ptr(frames)))
    rc, plain, _ = render(ctx, (bg, mv), c, depth=False)
    ctx.check(rc)
    same(frames, plain, "fused frames vs the plain call")
    same(frames, ec.expected("E8_17x17")[0], "fused frames vs the restatement")
    assert np.isfinite(lg).all()
    sc.close()
