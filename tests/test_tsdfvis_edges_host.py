"""The colour-TSDF ray caster's edge inputs without a GPU (tests/tsdfvis_edge_cases.py): every case reaches the edge it is named
for (the facts, counted by the brute-force restatement); the GPU's three skips, restated in numpy (tsdfvis_ref.slab_range, the
touched-block box and block flags in _sample, candidate_rect), change no byte of any case; every wrong rule changes a byte of a named
case or is shown unable to; the rectangle at the rigidity tolerance, which the first version of tv_prepare got wrong."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import tsdfvis_edge_cases as ec
from tests import tsdfvis_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def facts(name):
    f = ec.expected(name)[2]
    for part in ("bg", "mv"):
        print(name, part, {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in f[part].items() if np.any(v)})
    print(name, "rects", f.get("rects"))
    return f


def total(f, key):
    return np.asarray(f["bg"].get(key, 0)) + np.asarray(f["mv"].get(key, 0))


def differs(a, b):
    return bool((a[0] != b[0]).any() or (a[1].view(np.uint32) != b[1].view(np.uint32)).any())


# ---------------------------------------------------------------------------------------------------- the facts

def test_e1_dyadic_scene_puts_samples_on_voxel_planes_box_ends_and_exact_zeros():
    f = facts("E1_on_grid")
    assert (total(f, "frac0") >= 8).all() and (total(f, "at_clo") >= 1).all() and (total(f, "at_chi") >= 1).all()
    assert total(f, "hit_v0") >= 8
    h = facts("E1_half_off")
    assert h["mv"]["frac0"][2] > 0 and h["bg"]["frac0"][2] == 0          # z fractions 0.5 for the background, whose matrix is the identity
    s = ec.with_skips("E1_on_grid")[2]
    o = ec.with_skips("E1_origin_outside")[2]
    print("d == 0 with the origin inside / outside the slab:", s["bg"]["d0_inside"], s["mv"]["d0_inside"], o["bg"]["d0_outside"])
    assert s["bg"]["d0_inside"] + s["mv"]["d0_inside"] >= 1 and o["bg"]["d0_outside"] >= 1


def test_e2_crossing_signs():
    a, b = facts("E2_on_surface"), facts("E2_inside")
    assert a["mv"]["zero_then_neg"] >= 4 and a["mv"]["hits"][0] == 0      # observed 0, then negative: no hit
    assert a["mv"]["pos_zero_neg"] >= 4                                    # +, 0, -: a hit on the 0
    assert b["mv"]["first_obs_neg"] >= 4 and b["mv"]["hits"][0] == 0       # near inside the plate: the ray passes it; behind it lies the
    assert np.isinf(ec.expected("E2_inside")[1][0]).all()                  # plate's own shadow in the plane: nothing


def test_e3_threshold_equality_follows_the_weights():
    bg, _ = ec.volumes(("cases", "band"))
    masks = [np.isfinite(ec.expected(f"E3_thr{i}")[1]) for i in range(len(ec.THR_E3))]
    for i in range(len(ec.THR_E3) - 1):
        a, b = np.float32(ec.THR_E3[i]), np.float32(ec.THR_E3[i + 1])
        moved = bool(((bg.w >= a) != (bg.w >= b)).any())
        print(f"thr {a!r} -> {b!r}: observed set changes: {moved}, hit mask changes: {bool((masks[i] != masks[i + 1]).any())}")
        assert bool((masks[i] != masks[i + 1]).any()) == moved
    assert (bg.w == 2).any() and (bg.w == 3).any() and bg.w.max() == 3
    assert masks[0].any() and not masks[-1].any()                          # nextafter(3, 4): no hit at all


def test_e4_e5_fallback_colour_half_way_colours_and_both_clamps():
    f = facts("E4_fallback")
    assert total(f, "fallback") >= 4 and total(f, "fallback_differs") >= 1
    g = facts("E5_half_colours")
    assert total(g, "col_half") >= 4 and total(g, "col_half_even") >= 4    # x.5 with x even: where round-half-to-even differs
    h = facts("E1_on_grid")
    assert total(h, "col_0") >= 1 and total(h, "col_255") >= 1


def test_e6_e7_far_scene_and_untouched_block():
    f = facts("E6_far")
    assert all(n > 0 for n in f["mv"]["hits"])
    g = facts("E7_blocks")
    bg, _ = ec.volumes(("blocks",))
    assert tuple(bg.nb) == (5, 3, 2)
    # block occupancy from the weights, not from the flags the skip reads: here the two agree, and a weightless block lies in the box
    occupied = (bg.w > 0).reshape(2, 16, 3, 16, 5, 16).any(axis=(1, 3, 5))
    assert (occupied == bg.ever).all()
    bz, by, bx = np.nonzero(occupied)
    inside_box = np.zeros_like(occupied)
    inside_box[bz.min():bz.max() + 1, by.min():by.max() + 1, bx.min():bx.max() + 1] = True
    assert (inside_box & ~occupied).any()
    assert total(g, "hit_after_empty_block") >= 8


def test_e8_view_and_tile_edges():
    f = facts("E8_17x17")
    r = f["rects"]
    assert r[1] == (0, 0, 0, 0) and r[2][2] == 15 and r[3][0] == 16
    assert facts("E8_one_sample")["mv"]["S"] == 1 and facts("E8_no_sample")["mv"].get("S", 0) == 0
    for n in ("1x1", "1x17", "17x1", "8x8", "9x9", "16x16"):
        assert np.isfinite(ec.expected("E8_" + n)[1]).any(), n
    assert np.isfinite(ec.expected("E8_pp_left")[1]).any() and np.isfinite(ec.expected("E8_pp_right")[1]).any()


def test_e9_ends_of_the_sample_range():
    f = facts("E9_last_pair")
    assert f["bg"]["hit_last"] >= 1 and f["bg"]["hits"][0] == f["bg"]["hit_last"]
    assert facts("E9_one_voxel_more")["bg"].get("hits") == [0]
    g = facts("E9_inside_box")
    s = ec.with_skips("E9_inside_box")[2]
    print("rays whose range starts at sample 0 / ends at S - 1:", s["bg"]["s0_clamped"], ec.with_skips("E9_last_pair")[2]["bg"]["s1_clamped"])
    assert s["bg"]["s0_clamped"] >= 1 and g["bg"]["hit_s1"] >= 1
    assert ec.with_skips("E9_last_pair")[2]["bg"]["s1_clamped"] >= 1


def test_e10_near_tie_is_won_and_lost_by_a_few_ulps():
    c = ec.CASES["E10_near_tie"]
    bg, mv = ec.volumes(c.vol_key)
    bh, bt, _ = ref.cast(bg, ref.ray_matrix(c.cam)[None], c.view, c.thr)
    mh, mt, _ = ref.cast(mv, ref.ray_matrix(c.cam, c.o_now, c.poses[0])[None], c.view, c.thr)
    both = bh[0] & mh[0]
    d = mt[0][both].view(np.int32).astype(np.int64) - bt[0][both].view(np.int32).astype(np.int64)
    won, lost, tied = int(((d < 0) & (d >= -8)).sum()), int(((d > 0) & (d <= 8)).sum()), int((d == 0).sum())
    print(f"E10_near_tie: movable wins by <= 8 ulp on {won} pixels, loses by <= 8 ulp on {lost}, ties on {tied}; largest |difference| {int(np.abs(d).max())} ulp")
    assert won >= 1 and lost >= 1
    frames, depth, _ = ec.expected("E10_near_tie")
    assert (depth[0][both] == np.minimum(mt[0][both], bt[0][both])).all()


# ---------------------------------------------------------------------------------------------------- the skips

@pytest.mark.parametrize("name", list(ec.CASES))
def test_the_skips_change_no_byte(name):
    want = ec.expected(name)
    got = ec.with_skips(name)
    assert not differs(got, want), name


def _e12(name):
    c = ec.CASES[name]
    bg, mv = ec.volumes(c.vol_key)
    want = ec.expected(name)
    for P in c.poses:
        R = P[:3, :3].astype(np.float64)
        dev = np.abs(R.T @ R - np.eye(3)).max()
        assert 8e-6 < dev <= 1e-5
    old = ref.render(bg, mv, c.view, c.cam, c.o_now, c.poses, c.thr, skips=True, true_inverse=False)
    shift = max(max(abs(a - b) for a, b in zip(ref.candidate_rect(mv, c.view, c.cam, c.o_now, P, 1.0, False), ref.candidate_rect(mv, c.view, c.cam, c.o_now, P, 1.0, True)))
                for P in c.poses)
    cut = int(((old[0] != want[0]).any(axis=-1)).sum())
    print(f"{name}: rectangle displaced by up to {shift} pixels (clipped to the frame); transposed-inverse rectangle cuts {cut} pixels")
    return shift, cut


def test_e12_rectangle_at_the_rigidity_tolerance_40m_and_2km():
    """Poses scaled by 1 +- 4.5e-6 (R^T R off by 9e-6: accepted), obj_pose_now = I, world-frame candidate translations.  The first
    tv_prepare projected the box with inv(cam) P inv(O) from transposed inverses; the kernel marches with the rounded O inv(P) cam.
    Restated both ways: the rectangle from the true inverse of the rounded matrix changes no byte (test_the_skips_change_no_byte);
    the first version's is displaced by about 2 e |scene - pose origin|: a pixel at 40 m, 19 pixels at 2 km, where it cuts hits."""
    s40, cut40 = _e12("E12_40m")
    s2k, cut2k = _e12("E12_2km")
    assert cut40 == 0 and s40 <= 2
    assert cut2k > 0 and s2k >= 8
    R = ec.E12_REFUSED[:3, :3].astype(np.float64)
    assert np.abs(R.T @ R - np.eye(3)).max() > 1.1e-5


# ---------------------------------------------------------------------------------------------------- wrong rules

# rule -> (case, with the skips restated).  None: the rule cannot change a byte, for the reason given.
SHOWN_BY = {
    "prev_ge": ("E2_on_surface", False), "v_lt": ("E1_on_grid", False), "w_gt": ("E3_thr5", False), "colour_at_s": ("E5_half_colours", False),
    "colour_at_hit": ("E4_fallback", False), "half_even": ("E5_half_colours", False), "tie_movable": ("E10_exact_tie", False),
    "s_fewer": ("E9_last_pair", False), "chi_lower": ("E1_on_grid", True),
    # no clamp: a colour is a chain of a + f (b - a) with 0 <= f <= 1 over fused values that are means of bytes, so it stays in
    # 0 .. 255 up to an ulp and floor(c + 0.5) never leaves 0 .. 255; the clamp only catches NaN (a volume with non-finite colours)
    "wrap": None,
    # the slab already spans the box widened by two voxels and by a bound on the fp32 sample point's error, and floor / ceil round
    # outward: a sample outside floor(..) .. ceil(..) lies outside the box for sure.  The +- 2 is a second margin on top of a sound one
    "slab_no_pad": None,
    # likewise: the box is widened by a voxel and the slack, floor(umin) .. ceil(umax) rounds outward and pixel j's ray passes
    # through u = j exactly, so the one-pixel margin is never the only thing that keeps a pixel in
    "rect_no_margin": None,
}


@pytest.mark.parametrize("rule", ref.WRONG_RULES)
def test_every_wrong_rule_changes_a_byte_or_cannot(rule):
    shown = SHOWN_BY[rule]
    if shown is not None:
        name, skips = shown
        assert differs(ec.with_skips(name, (rule,), skips, False), ec.expected(name)), (rule, name)
        return
    for name in ("E1_on_grid", "E5_half_colours", "E7_blocks", "E8_17x17", "E12_2km"):
        assert not differs(ec.with_skips(name, (rule,), True, False), ec.expected(name)), (rule, name)


def test_rectangle_inputs_of_e8_and_e12_under_the_sanitizers(tmp_path):
    """tests/tsdfvis_host_main.cpp with the rectangle inputs of E8 (one pixel, column 15, column 16) and E12 (the inverse of a scaled
    matrix at 2 km): the C++ gives the rectangles the numpy restatement gives."""
    c = ec.CASES["E8_17x17"]
    _, mv = ec.volumes(c.vol_key)
    assert [ref.candidate_rect(mv, c.view, c.cam, c.o_now, P) for P in c.poses[1:4]] == [(0, 0, 0, 0), (0, 1, 15, 15), (16, 1, 16, 15)]
    c = ec.CASES["E12_2km"]
    _, mv = ec.volumes(c.vol_key)
    assert ref.candidate_rect(mv, c.view, c.cam, c.o_now, c.poses[1]) == (19, 0, 47, 39)
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (g++ or clang++): it is part of the toolchain this project builds with"
    exe = str(tmp_path / "tsdfvis_host")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        os.path.join(REPO, "tests", "tsdfvis_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout, r.stderr)
