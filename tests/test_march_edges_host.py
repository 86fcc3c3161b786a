"""Host side of the marcher edge tests (tests/march_cases.py, tests/test_march_edges_gpu.py).  No GPU.

For every case: the conditions under which a pixel's alpha decodes to its sample count (no saturation, exact decoding of the
oracle's own frames, fp32 accumulation error under a quarter of the bar), that the case is not trivial, and the numpy
restatement of make_ray's window and next_sample's skips (tests/march_ref.py) against brute force over every lattice point.
Then the table of wrong rules: how many cases notice each.

Wrong rules that do not show, or barely, and why:
  skip_n_plus_1 (skip floor(dist / dt) + 1 steps)  NOT a wrong rule but for rounding.  dist is the distance to the far face of the
                empty cell or brick, so the points k + 1 .. k + n are still inside it and k + n + 1 is the first one past it:
                skipping n steps lands on the last EMPTY point, which is tested again and left by a one-step skip; skipping
                n + 1 lands on the first point that can be occupied.  It loses a point only where rounding puts dist / dt just
                above a whole number (measured: 1 case of 131).  skip_n_plus_2 is the rule that loses points, and the table
                holds it to >= 3 cases.  (That the marcher re-tests one point per skipped region is a cost, not a fault.)
  window_margin_0 (no margin on [k_lo, k_hi])  The window is cut from the occupied cells' bounding box padded by 1e-4 per side,
                i.e. by >= 1e-4 / dt = 0.059 steps along any ray (|d_i| <= 1), and floor / ceil round outward.  At aabb_scale 1
                the index (lo - t0) / dt <= 1024 carries three roundings, 1024 * 3 * 2^-24 = 1.8e-4 steps < 0.059: the margin of
                one point can never be needed, proven.  With cone stepping the index goes through __log2f * 177.8, whose
                index error is bounded too: v_log_f32 is accurate to 1 ulp (CDNA ISA guide), <= 4 * 2^-23 on log2(t / t1) <= 4, times
                177.8 = 8.5e-5 points; the division and the constant add 1.5e-5 and 6.5e-5; the lattice itself (t1 times a product
                of two fp32 table entries, 2 ulp) sits within 2.4e-7 * 256.5 = 6e-5 points of the closed form: 2.3e-4 points in
                all.  The padding is 1e-4 box units = 1e-4 * side in distance, over a step of at most t / 256 <= side * 2 sqrt(3)
                / 256: >= 0.0074 points.  So the margin of two points can never be needed there either: proven invisible, and the
                table asserts 0 cases.
                window_margin_minus_1 (the window shrunk by a point at each end) is the rule that loses points.
  far_face_ge   (`r.dx >= 0.f` for `r.dx > 0.f` in the far-face choice)  The two differ only for a direction component of
                exactly +-0.  Its reciprocal is +-inf, so that axis' crossing distance (face - p) * inf is +inf, -inf or
                (0 * inf) NaN under either rule, never a finite wrong number.  fminf drops the NaN, +inf is never the minimum
                (another axis is finite), and -inf gives n = INT_MIN -> a skip of one step, which loses nothing.  The rule
                changes how far such a ray skips, never which points it samples.
  cascade_gt    (`>` for `>=` in the cascade choice) shows only when a lattice point has max|p - 0.5| * side or dt * 256
                EXACTLY on a threshold in fp32.  The `on-cascade-face` cases put a whole pixel column there: an axis camera at an
                odd width whose centre column runs in the plane x = 1 of the unit cube, where max|p - 0.5| * side == 0.5 at every
                point.  The table asserts that both see the rule.
"""
import numpy as np
import pytest

from tests import march_cases as mc
from tests import march_ref as mr


def _lattice(name: str, cascade_gt: bool = False) -> mr.Lattice:
    """(not cached: a case's lattice is up to 200 MB)"""
    case = mc.BY_NAME[name]
    P = mr.Params(mc.occupancy(case.pattern, case.aabb_scale), case.aabb_scale, case.render_aabb)
    o, d = mr.pixel_rays(case.cam_array(), case.width, case.height, case.focal, case.near)
    return mr.Lattice(P, o, d, cascade_gt)


# Section 4's "a ray whose first occupied lattice point is index 0 of the oracle's lattice, and one whose last occupied point is the
# last point inside the box" is asserted PER CASE, both ways: a case listed here must lack such a ray, a case not listed must have
# one.  (regex on the case name, why no ray can START on an occupied point or None, why none can END on one or None)
_INTERIOR = "the occupied cell lies inside the render box, not on its boundary, and the camera is outside the cell"
_NOTHING = "no occupied cell inside the render box"
_FEW = "cells on the boundary exist, but none of these few rays crosses the boundary inside one"
ENDS_EXEMPT = [
    (r"^(empty-|crop-nothing|crop-cone-nothing|s\d-empty)", _NOTHING, _NOTHING),
    (r"^(cell_(000|333)-octants|composite-)", _INTERIOR, _INTERIOR),
    (r"^s\d-(c0_|c1_out_|c1_000|c1_333|c2_out_|c2_only|tb\d)", _INTERIOR, _INTERIOR),
    (r"^s4-c1_(lo|hi)-", _INTERIOR, _INTERIOR),
    (r"^s2-c1_(lo|hi)-", "the cell is on a face of the box the rays leave through, not the one they enter by", None),
    (r"^(slabs-16x16|near-into-cube)", "the slabs are layers 10 and 110, off the z faces; " + _FEW, "the slabs are layers 10 and 110, off the z faces; " + _FEW),
    (r"^(exit_corner-16x16|rand0\.5-16x16|axis-(on|off)-face-slabs|diagonal-\dx\d-exit_corner)", _FEW, None),
    (r"^diagonal-\dx\d-rand5", _FEW, _FEW),
    (r"^diagonal-1x1-checker_cells", None, "one ray: it leaves through cell (127,127,127), which the checkerboard leaves empty"),
    (r"^s\d-corners8", None, "the camera faces one corner cell, which the rays enter from outside the box and leave inside it"),
    (r"^(inside-empty-cell|s\d-rand5-inside)", "the camera sits in an empty cell inside the box", None),
    (r"^s\d-on-cascade-face", _FEW, None),
]


def _ends_expected(name):
    import re
    first = last = True
    for rx, why_first, why_last in ENDS_EXEMPT:
        if re.match(rx, name):
            first, last = first and why_first is None, last and why_last is None
    return first, last


def _counts(samples, case):
    return samples.sum(axis=1).reshape(len(case.cams), case.height, case.width)


@pytest.mark.parametrize("group", mc.GROUPS)
def test_alpha_decodes_to_the_sample_count_and_the_skips_lose_nothing(group):
    rows = []
    for case in (c for c in mc.CASES if c.group == group):
        rgba, depth, n_samples = mc.oracle_frames(case.name)
        A = rgba[..., 3]
        # condition on the inputs: no ray comes near saturation, so none terminates early
        assert A.max() < 1.0 - mc.MIN_T, case.name
        L = _lattice(case.name)
        brute = L.brute_force()
        n_ref = _counts(brute, case)
        # the restatement's lattice IS the oracle's: same total, and (unit cube) the same count in every pixel
        assert n_ref.sum() == n_samples, (case.name, int(n_ref.sum()), n_samples)
        if not case.cone:
            n_dec = mc.decode_counts(A)
            assert n_dec.sum() == n_samples, (case.name, int(n_dec.sum()), n_samples)          # the decoding is exact
            np.testing.assert_array_equal(n_dec, n_ref, err_msg=case.name)
        # fp32 accumulation error (one rounding of A per sample) cannot reach the bar
        bar = mc.alpha_bar(A)
        assert n_ref.max() * 2.0 ** -24 < 0.25 * bar, (case.name, int(n_ref.max()), bar)
        # the oracle's break at the first outside point drops no occupied inside point (subset argument)
        assert L.lost_by_the_oracles_break() == 0, case.name
        # the window and the skips lose nothing
        dev, skips = mr.device_samples(L)
        bad = np.argwhere(dev != brute)
        assert not len(bad), f"{case.name}: ray {bad[0][0]} lattice point {bad[0][1]}: restated device {dev[tuple(bad[0])]}, brute force {brute[tuple(bad[0])]}"
        # the case is not trivial
        hits = int((n_ref > 0).sum())
        long_skips = int((skips > 1).sum())
        assert hits >= case.min_hits, (case.name, hits)
        assert long_skips >= case.min_long_skips, (case.name, long_skips)
        if case.min_hits == 0 and case.pattern == "empty":
            assert hits == 0 and n_samples == 0
        rows.append((case.name, hits, int(n_ref.max()), int(skips.max()) if len(skips) else 0))
        n_in = L.before_exit.sum(axis=1)
        r = np.flatnonzero(L.valid & (n_in > 0))
        has = (bool(brute[:, 0].any()), bool(brute[r, n_in[r] - 1].any()))
        assert has == _ends_expected(case.name), (case.name, "rays that start / end on an occupied point", has)
    print(f"\n[march edges] group {group}: case, hit pixels, max samples per ray, longest skip (steps)")
    for r in rows:
        print("   %-34s %6d %6d %6d" % r)


def test_wrong_rules_are_noticed():
    seen = {rule: [] for rule in mr.RULES}
    for case in mc.CASES:
        L = _lattice(case.name)
        brute = L.brute_force()
        for rule in mr.RULES:
            if rule in ("no_tb_clamp", "cascade_gt") and not case.cone:
                continue
            dev, _ = mr.device_samples(_lattice(case.name, cascade_gt=True) if rule == "cascade_gt" else L, rule)
            if (dev != brute).any():
                seen[rule].append(case.name)
    print("\n[march edges] wrong rule -> cases that notice it")
    for rule, names in seen.items():
        print(f"   {rule:22s} {len(names):4d} of {len(mc.CASES)}   {names if len(names) <= 12 else names[:3]}")
    assert not seen["far_face_ge"] and not seen["window_margin_0"]          # provably invisible (module docstring)
    assert {"s2-on-cascade-face", "s4-on-cascade-face"} <= set(seen["cascade_gt"]), seen["cascade_gt"]
    # the tb clamp is seen by the case aimed at each crossing: t = 1 at both scales, t = 2 where a third cascade exists
    assert {"s2-tb1", "s4-tb1", "s4-tb2"} <= set(seen["no_tb_clamp"]), seen["no_tb_clamp"]
    for rule in ("skip_n_plus_2", "window_margin_minus_1", "no_tb_clamp", "brick_skip_always"):
        assert len(seen[rule]) >= 3, (rule, seen[rule])


@pytest.mark.parametrize("name", [c.name for c in mc.CASES if c.group == "composite"])
def test_composite_cases_sit_at_the_frame_edges(name):
    """conditions on the composite cases, from the oracle alone: the cell lands on the two pixel columns / rows at each frame edge,
    misses the frame in the two `out` cameras, and every hit pixel is a foreground pixel of the composite that differs from the
    background.  With rgb 0.5 and alpha from the count, a composited pixel is the background colour for n = 0 and black for
    1 <= n < 419 (quantised alpha under 130 of 255; 419 samples reach it): the frames separate n = 0 from n >= 1, pixel by pixel."""
    poses, rgba, depth, frames = mc.composite_reference(name)
    A = rgba[..., 3]
    hit = A > 0
    assert A.max() < 129.5 / 255.0 and mc.decode_counts(A).max() < 419
    assert (depth[hit] >= 0.05).all() and (depth[hit] < mc.BG_DEPTH).all()        # the fg pixel wins the depth test, as itself
    bg = frames[4, 0, 0]
    assert (frames[4] == bg).all() and (frames[5] == bg).all() and bg.min() > 0     # the `out` cameras: background only
    np.testing.assert_array_equal((frames != bg).any(-1), hit)                       # non-background pixels == hit pixels
    ys, xs = [np.nonzero(h)[0] for h in hit], [np.nonzero(h)[1] for h in hit]
    for i, (tag, _, _) in enumerate(mc.COMPOSITE_AIMS):
        n = int(hit[i].sum())
        assert (n == 0) == tag.startswith("out"), (name, tag, n)
        if tag == "left":
            assert xs[i].max() <= 1 and xs[i].min() == 0, (name, tag, xs[i])
        if tag == "right":
            assert xs[i].min() >= 31 and xs[i].max() == 32, (name, tag, xs[i])
        if tag == "top":
            assert ys[i].max() <= 1 and ys[i].min() == 0, (name, tag, ys[i])
        if tag == "bottom":
            assert ys[i].min() >= 15 and ys[i].max() == 16, (name, tag, ys[i])
