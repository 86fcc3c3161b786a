"""The colour-TSDF visual model on the GPU against its numpy restatement (tests/tsdfvis_ref.py): colour fusion
and the ray caster's frames and depths must be IDENTICAL, byte for byte; the fused call; the refusals; determinism."""
import ctypes as C

import numpy as np
import pytest

from dream2real_amd import _lib
from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
from dream2real_amd.physics_utils import TsdfVolume
from tests import tsdfvis_cases as cases
from tests import tsdfvis_ref as ref
from tests.parity_utils import random_unit_text_embeds

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vols(ctx):
    """kind -> (background, movable) device volumes, fused like tsdfvis_cases.ref_volumes(kind); built on first use."""
    made = {}

    def get(kind="plain"):
        if kind not in made:
            if kind == "twins":
                made[kind] = (cases.fuse(TsdfVolume(ctx, *cases.mv_args()), 1), cases.fuse(TsdfVolume(ctx, *cases.mv_args()), 1, tint=90))
            else:
                made[kind] = (cases.fuse(TsdfVolume(ctx, *cases.bg_args()), 0, skip_band=cases.SKIP_BANDS.get(kind)),
                              cases.fuse(TsdfVolume(ctx, *cases.mv_args(kind)), 1))
        return made[kind]
    yield get
    for pair in made.values():
        for v in pair:
            v.close()


def pcd_view(v):
    return _lib.PcdView(v.width, v.height, float(v.fx), float(v.fy), float(v.cx), float(v.cy), 1.0, float(v.near))


def render(ctx, pair, view_name, names, cam=cases.CAM, depth=True):
    v = cases.VIEWS[view_name]
    poses = np.ascontiguousarray(cases.poses(names).reshape(-1, 16), np.float32)
    K = poses.shape[0]
    frames = np.full((K, v.height, v.width, 3), 77, np.uint8)
    dep = np.full((K, v.height, v.width), -1.0, np.float32) if depth else None
    view = pcd_view(v)
    ctx.check(ctx.lib.d2r_tsdfvis_render(ctx.h, pair[0].h, pair[1].h, C.byref(view), _lib.ptr(np.ascontiguousarray(cam, np.float32)),
                                         _lib.ptr(cases.O_NOW), _lib.ptr(poses), K, cases.THR, _lib.ptr(frames), _lib.ptr(dep)))
    return frames, dep


def same(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if g.dtype == np.float32:
        g, w = g.view(np.uint32), w.view(np.uint32)
    bad = int((g != w).sum())
    print(f"{what}: {bad} of {g.size} values differ")
    assert g.shape == w.shape and bad == 0, what


def check(ctx, pair, view_name, names, kind="plain", cam=None):
    frames, dep = render(ctx, pair, view_name, names, cases.CAM if cam is None else cam)
    want_f, want_d, _ = cases.expected(view_name, kind, tuple(names), None if cam is None else tuple(np.asarray(cam).ravel().tolist()))
    same(frames, want_f, f"{view_name} {names} frames")
    same(dep, want_d, f"{view_name} {names} depth")
    return frames, dep


# ---------------------------------------------------------------------------------------------------- colour fusion

def test_colour_fusion_equals_the_restatement_and_leaves_tsdf_and_weight_alone(ctx, vols):
    for which, obj, args in ((0, 0, cases.bg_args()), (1, 1, cases.mv_args())):
        vol, rvol = vols()[which], cases.ref_volumes()[which]
        coords, tsdf, weight = vol.read_voxels()
        plain = TsdfVolume(ctx, *args)
        for f, x in enumerate(cases.CAM_X):
            z, lab, _ = cases.frame(x)
            plain.integrate((z * 1000).astype(np.uint16), lab == obj, cases.K, cases.cam_pose(x), cases.ERODE)
        pc, pt, pw = plain.read_voxels()
        same(coords, pc, "blocks"), same(tsdf, pt, "tsdf rgb call vs plain call"), same(weight, pw, "weight rgb call vs plain call")
        same(coords.astype(np.int64), rvol.active_blocks(), "blocks vs restatement")
        cols = vol.read_colours()
        same(cols, rvol.block_colours(), "colours vs restatement")
        assert (weight >= 3).sum() > 500 and cols.max() > 100
        # the plain volume holds no colour, and refuses an rgb frame; the colour volume refuses a plain frame
        n = C.c_uint32(0)
        assert ctx.lib.d2r_tsdf_read_colours(plain.h, C.byref(n), None) == INVALID and "no colour" in ctx.lib.d2r_last_error(ctx.h).decode()
        z, lab, rgb = cases.frame(0.0)
        with pytest.raises(_lib.D2RError, match="mixes"):
            plain.integrate_rgb((z * 1000).astype(np.uint16), lab == obj, rgb, cases.K, cases.cam_pose(0.0), cases.ERODE)
        extra = cases.fuse(TsdfVolume(ctx, *args), obj, n=1)
        with pytest.raises(_lib.D2RError, match="mixes"):
            extra.integrate((z * 1000).astype(np.uint16), lab == obj, cases.K, cases.cam_pose(0.0), cases.ERODE)
        # a voxel one frame saw keeps that frame's pixel colour exactly: whole numbers 0 .. 255, and they occur
        _, _, w1 = extra.read_voxels()
        c1 = extra.read_colours()
        once = w1 == 1
        assert once.sum() > 100 and (c1[once] == np.floor(c1[once])).all() and c1[once].max() <= 255 and (c1[~(w1 > 0)] == 0).all()
        same(c1, cases.fuse(ref.ColourVolume(*args), obj, n=1).block_colours(), "one frame's colours")
        plain.close(), extra.close()


# ---------------------------------------------------------------------------------------------------- the ray caster

def test_all_candidates_48x40(ctx, vols):
    frames, dep = check(ctx, vols(), "48x40", list(cases.CANDIDATES))
    assert np.isinf(dep).any() and np.isfinite(dep).any()


def test_small_view_45x37_a_multiple_of_no_tile(ctx, vols):
    check(ctx, vols(), "45x37", list(cases.SMALL_VIEW_CANDIDATES))


def test_candidate_off_screen_gives_the_background_frame(ctx, vols):
    frames, dep = check(ctx, vols(), "48x40", ["off"])
    _, _, (hit, t, rgb) = cases.expected("48x40", names=("off",))
    same(frames[0], rgb, "background frame"), same(dep[0], t, "background depth")


def test_box_corner_behind_near_takes_the_whole_frame(ctx, vols):
    frames, dep = check(ctx, vols(), "48x40", ["near"])
    bg = cases.expected("48x40", names=("off",))[0][0]
    changed = (frames[0] != bg).any(axis=2)
    assert changed[0].any() or changed[-1].any() or changed[:, 0].any() or changed[:, -1].any() or changed.mean() > 0.3


def test_movable_in_front_of_and_behind_the_background(ctx, vols):
    frames, dep = check(ctx, vols(), "48x40", ["front", "behind"])
    assert (frames[0][..., 0] >= 195).sum() > 20                  # the sphere's red in front
    bgd = cases.expected("48x40", names=("off",))[1][0]
    shown = (frames[1][..., 0] >= 195)
    assert shown.any() and np.isinf(bgd[shown]).all()             # behind: it shows only through the hole in the plane


def test_equal_depth_goes_to_the_background(ctx, vols):
    """The same geometry twice (two volumes fused from the same depth, with other colours) at the same pose: every hit ties."""
    pair = vols("twins")
    frames, dep = check(ctx, pair, "48x40", ["front"], kind="twins")
    alone, _ = render(ctx, (pair[0], pair[0]), "48x40", ["front"])
    same(frames, alone, "a tie shows the background volume's colours")
    other, _ = render(ctx, (pair[1], pair[1]), "48x40", ["front"])
    assert (other != alone).any()


def test_no_hit_through_a_band_seen_by_two_frames(ctx, vols):
    frames, dep = check(ctx, vols("band"), "48x40", ["off"], kind="band")
    full = cases.expected("48x40", names=("off",))[1][0]
    assert (np.isinf(dep[0]) & np.isfinite(full)).sum() > 10


def test_an_unobserved_sample_between_two_observed_ones_breaks_the_pair(ctx, vols):
    """A slab of two observations standing in depth, met obliquely: rays are observed > 0 in front of the plane on one side of it,
    unobserved inside it where they cross the plane, observed <= 0 behind the plane on the other side.  The rule gives no hit there;
    the wrong rule that carries the last observed value across the gap does, as the whole volume does."""
    frames, dep = check(ctx, vols("gap"), "48x40", ["off"], kind="gap", cam=cases.OBLIQUE_CAM)
    v, M = cases.VIEWS["48x40"], ref.ray_matrix(cases.OBLIQUE_CAM)[None]
    carried = ref.cast(cases.ref_volumes("gap")[0], M, v, cases.THR, carry_gaps=True)[0][0]
    whole = ref.cast(cases.ref_volumes("plain")[0], M, v, cases.THR)[0][0]
    through = whole & carried & np.isinf(dep[0])
    print("rays that cross the plane inside the slab:", int(through.sum()))
    assert through.sum() >= 10 and (frames[0][through] == 0).all()


def test_volumes_seen_from_behind_give_no_hit(ctx, vols):
    frames, dep = check(ctx, vols(), "48x40", ["front"], cam=cases.BEHIND_CAM)
    assert (frames == 0).all() and np.isinf(dep).all()


def test_rotated_candidates_cross_blocks_and_leave_through_faces_edges_corners(ctx, vols):
    frames, dep = check(ctx, vols(), "48x40", ["rot_x", "rot_xyz", "rot_z"])
    assert all((f[..., 0] >= 195).any() for f in frames)


def test_rectangle_clipped_by_each_frame_border(ctx, vols):
    frames, dep = check(ctx, vols(), "48x40", ["left", "right", "top", "bottom"])
    red = frames[..., 0] >= 195
    assert red[0][:, 0].any() and red[1][:, -1].any() and red[2][0].any() and red[3][-1].any()


def test_the_two_volumes_lie_on_different_grids(ctx, vols):
    bg, mv = vols()
    (b0a, nva, va, _), (b0b, nvb, vb, _) = bg.grid(), mv.grid()
    assert va != vb and (b0a.astype(np.float64) * 16 * va != b0b.astype(np.float64) * 16 * vb).any()              # voxel size and origin
    check(ctx, (bg, mv), "45x37", ["front"])


def test_k_1_k_0_and_more_than_one_chunk(ctx, vols):
    check(ctx, vols(), "45x37", ["rot_xyz"])
    frames, dep = render(ctx, vols(), "45x37", [])
    assert frames.shape[0] == 0
    names = list(cases.SMALL_VIEW_CANDIDATES)
    chunk = ctx.get_option("chunk")
    ctx.set_option("chunk", 2)                                    # three passes, a remainder
    try:
        check(ctx, vols(), "45x37", names)
    finally:
        ctx.set_option("chunk", chunk)


def test_padding_the_movable_volume_by_empty_blocks_changes_nothing(ctx, vols):
    names = ["front", "rot_xyz", "left"]
    frames, dep = check(ctx, vols("padded"), "48x40", names, kind="padded")
    plain_f, plain_d = render(ctx, vols(), "48x40", names)
    same(frames, plain_f, "padded frames"), same(dep, plain_d, "padded depth")
    assert (vols("padded")[1].grid()[1] > vols()[1].grid()[1] + 100).all()


def test_fused_logits_equal_the_two_step_route(ctx, vols):
    from dream2real_amd import engine
    cfg = CLIP_CONFIGS["vit_tiny"]
    sc = engine.ClipScorer(ctx, cfg, random_clip_state_dict(cfg, seed=6, text=False))
    text = random_unit_text_embeds(cfg["proj"], 3)
    names = list(cases.CANDIDATES)
    v = cases.VIEWS["48x40"]
    view, poses = pcd_view(v), np.ascontiguousarray(cases.poses(names).reshape(-1, 16), np.float32)
    K = len(names)
    lg, frames = np.zeros((K, 3), np.float32), np.zeros((K, v.height, v.width, 3), np.uint8)
    bg, mv = vols()
    chunk = ctx.get_option("chunk")
    ctx.set_option("chunk", 4)
    try:
        ctx.check(ctx.lib.d2r_tsdfvis_render_score_host(ctx.h, bg.h, mv.h, sc.h, C.byref(view), _lib.ptr(cases.CAM), _lib.ptr(cases.O_NOW), _lib.ptr(poses),
                                                        K, cases.THR, _lib.ptr(text), 3, sc.logit_scale, _lib.ptr(lg), _lib.ptr(frames)))
        ms = np.zeros(4)
        ctx.check(ctx.lib.d2r_tsdfvis_get_timing(ctx.h, _lib.ptr(ms)))
        print("fused call: upload, background cast, candidate casts, copies to the host (ms):", ms)
        assert (ms >= 0).all() and ms[1] > 0 and ms[2] > 0 and ms[3] == 0
        hook, _ = render(ctx, (bg, mv), "48x40", names, depth=False)
        ctx.check(ctx.lib.d2r_tsdfvis_get_timing(ctx.h, _lib.ptr(ms)))
        assert ms[2] > 0 and ms[3] > 0
    finally:
        ctx.set_option("chunk", chunk)
    same(frames, hook, "fused frames vs the parity hook")
    same(lg, sc.score_frames(hook, text, rot90=True), "fused logits vs d2r_clip_score_frames")
    sc.close()


def test_refusals_leave_outputs_alone_and_the_context_usable(ctx, vols):
    bg, mv = vols()
    v = cases.VIEWS["48x40"]
    poses = np.ascontiguousarray(cases.poses(["front"]).reshape(-1, 16), np.float32)
    frames = np.full((1, v.height, v.width, 3), 77, np.uint8)
    dep = np.full((1, v.height, v.width), -1.0, np.float32)
    plain = TsdfVolume(ctx, *cases.mv_args())
    z, lab, _ = cases.frame(0.0)
    plain.integrate((z * 1000).astype(np.uint16), lab == 1, cases.K, cases.cam_pose(0.0), cases.ERODE)

    def call(bg_h=bg.h, mv_h=mv.h, view=pcd_view(v), cam=cases.CAM, now=cases.O_NOW, p=poses, thr=cases.THR, out=frames):
        return ctx.lib.d2r_tsdfvis_render(ctx.h, bg_h, mv_h, C.byref(view) if view is not None else None, _lib.ptr(cam), _lib.ptr(now), _lib.ptr(p), 1, thr,
                                          _lib.ptr(out), _lib.ptr(dep))
    skew, nan, far = cases.CAM.copy(), poses.copy(), pcd_view(v)
    skew[0, 0] = 1.001                                           # off orthogonal by 2e-3: past the 1e-5 the rule allows
    nan[0, 3] = np.nan
    bad_views = []
    for field, value in (("width", 0), ("height", 20000), ("point_size", 2.5), ("near", -1.0), ("fx", float("inf"))):
        b = pcd_view(v)
        setattr(b, field, value)
        bad_views.append(b)
    refused = [dict(bg_h=None), dict(mv_h=None), dict(view=None), dict(cam=None), dict(now=None), dict(p=None), dict(out=None),
               dict(bg_h=plain.h), dict(mv_h=plain.h), dict(cam=skew), dict(now=skew), dict(p=nan), dict(thr=0.0)] + [dict(view=b) for b in bad_views]
    for kw in refused:
        rc = call(**kw)
        assert rc == INVALID or (rc == UNSUPPORTED and "point_size" in ctx.lib.d2r_last_error(ctx.h).decode()), (kw.keys(), rc)
        assert ctx.lib.d2r_last_error(ctx.h)
        assert (frames == 77).all() and (dep == -1.0).all(), kw.keys()
        assert call() == 0                                        # one good call: the context still works
        same(frames, cases.expected("48x40", names=("front",))[0], "the good call after a refusal")
        frames[:] = 77
        dep[:] = -1.0
    plain.close()


def test_fused_call_refusals_leave_outputs_alone_and_the_context_usable(ctx, vols):
    from dream2real_amd import engine
    cfg = CLIP_CONFIGS["vit_tiny"]
    sc = engine.ClipScorer(ctx, cfg, random_clip_state_dict(cfg, seed=6, text=False))
    text = random_unit_text_embeds(cfg["proj"], 3)
    bg, mv = vols()
    v = cases.VIEWS["48x40"]
    view, poses = pcd_view(v), np.ascontiguousarray(cases.poses(["front", "rot_x"]).reshape(-1, 16), np.float32)
    lg, frames = np.full((2, 3), -5.0, np.float32), np.full((2, v.height, v.width, 3), 77, np.uint8)
    plain = TsdfVolume(ctx, *cases.mv_args())

    def call(clip=sc.h, mv_h=mv.h, p=poses, t=text, C_=3, out=lg, cam=cases.CAM):
        return ctx.lib.d2r_tsdfvis_render_score_host(ctx.h, bg.h, mv_h, clip, C.byref(view), _lib.ptr(cam), _lib.ptr(cases.O_NOW), _lib.ptr(p), 2, cases.THR,
                                                     _lib.ptr(t), C_, sc.logit_scale, _lib.ptr(out), _lib.ptr(frames))
    skew = cases.CAM.copy()
    skew[1, 1] = 1.001                                            # off orthogonal by 2e-3: past the 1e-5 the rule allows
    want = None
    for kw in (dict(clip=None), dict(out=None), dict(t=None), dict(C_=0), dict(C_=2000), dict(mv_h=plain.h), dict(mv_h=None), dict(p=None), dict(cam=skew)):
        assert call(**kw) == INVALID and ctx.lib.d2r_last_error(ctx.h), kw.keys()
        assert (lg == -5.0).all() and (frames == 77).all(), kw.keys()
        assert call() == 0                                        # one good call: the context still works
        want = lg.copy() if want is None else want
        same(lg, want, "the good call after a refusal")
        same(frames, cases.expected("48x40", names=("front", "rot_x"))[0], "its frames")
        lg[:], frames[:] = -5.0, 77
    # a pass of more than 65535 candidates cannot be one launch: refused, not truncated
    chunk = ctx.get_option("chunk")
    try:
        ctx.set_option("chunk", 16384)
        assert call() == 0                                        # the largest pass the option allows is below the limit
    finally:
        ctx.set_option("chunk", chunk)
    plain.close()
    sc.close()


def test_colour_that_would_pass_the_size_cap_is_refused_before_it_is_allocated(ctx):
    """1024 x 1024 x 928 voxels of 2 mm are 7.25 GiB of (tsdf, weight), under the 16 GiB cap; with 12 bytes of colour a voxel they
    would be 18.1 GiB, over it.  The plain call takes the frame; the rgb call is refused by arithmetic alone."""
    z, lab, rgb = cases.frame(0.0)
    args = ((z * 1000).astype(np.uint16), lab == 0)
    big = TsdfVolume(ctx, np.array([[-1.0, -1.0, 0.0], [1.0, 1.0, 1.8]]))
    try:
        nv = big.grid()[1].astype(np.int64)
        assert nv.prod() * 8 < 2 ** 34 < nv.prod() * 20
        with pytest.raises(_lib.D2RError, match="TSDF volume over the cap"):
            big.integrate_rgb(*args, rgb, cases.K, cases.cam_pose(0.0), cases.ERODE)
        n = C.c_uint32(0)
        assert ctx.lib.d2r_tsdf_read_colours(big.h, C.byref(n), None) == INVALID                # nothing was allocated
        big.integrate(*args, cases.K, cases.cam_pose(0.0), cases.ERODE)                          # and the volume is not marked as a colour volume
    finally:
        big.close()


def test_two_calls_give_the_same_bytes(ctx, vols):
    a = render(ctx, vols(), "48x40", list(cases.CANDIDATES))
    b = render(ctx, vols(), "48x40", list(cases.CANDIDATES))
    same(a[0], b[0], "frames, second call"), same(a[1], b[1], "depth, second call")
