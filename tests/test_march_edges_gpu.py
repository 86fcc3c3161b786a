"""Marcher edges on the device: per-pixel sample sets equal brute force (the oracle tests every lattice point of a ray, one by
one) at every window, skip, first-sample and cascade edge of tests/march_cases.py.  Run on the MI355X:  pytest -m gpu.

The field is constant (tests/march_cases.py: why alpha counts the samples, and why equal counts prove equal sets), so on every
case, for every pixel:
  unit-cube models   the sample count decoded from the device's alpha == the count decoded from the oracle's, exactly
  cone models        |A_device - A_oracle| <= 0.5 (1 - exp(-dt_min)) (1 - max A_oracle): half the smallest weight one sample
                     can have had in the oracle's frames, a bar that comes from the reference alone
and for every case  Testbed.last_samples == the oracle's n_samples exactly, depth within 2e-3, RGBA within 5e-3 (the suite's
existing bars; the count is the test).  tests/test_march_edges_host.py checks on the CPU that the decoding is exact, that fp32
accumulation error stays under a quarter of the bar and that no case saturates.

The composite path (k_raygen_rect's rectangle cull) runs the `composite` cases through render_composite with raygen_rect 1 and 0:
the same bytes, the oracle's composite of the oracle's frames within 1 LSB on at most 2 % of pixels, and exactly the oracle's set
of non-background pixels (a composited pixel is the background for n = 0 and black for 1 <= n < 419: the host test).
"""
import ctypes as C

import numpy as np
import pytest

from tests import march_cases as mc

pytestmark = pytest.mark.gpu


class Device:
    def __init__(self):
        from dream2real_amd import _lib, engine
        self._lib, self.engine = _lib, engine
        self.ctx = engine.Context(0)
        self.beds = {}

    def testbed(self, case):
        key = (case.pattern, case.aabb_scale, case.render_aabb)
        if key not in self.beds:
            self.beds[key] = self.engine.Testbed(self.ctx, case.model(), dataset_scale=1.0, dataset_offset=(0.0, 0.0, 0.0))
        return self.beds[key]

    def render(self, case):
        """d2r_render with the case's own view (Testbed.render_batch has no near_distance) -> rgba, depth, samples"""
        tb = self.testbed(case)
        cams = np.ascontiguousarray(mc.cams_nerf(case.cam_array(), case.scale), np.float32)
        n = cams.shape[0]
        rgba = np.empty((n, case.height, case.width, 4), np.float32)
        depth = np.empty((n, case.height, case.width), np.float32)
        v = self._lib.view_c(case.view())
        ns = C.c_uint64(0)
        self.ctx.check(self.ctx.lib.d2r_render(self.ctx.h, tb.h, C.byref(v), self._lib.ptr(cams), n, self._lib.ptr(rgba), self._lib.ptr(depth), C.byref(ns)))
        return rgba, depth, int(ns.value)

    def close(self):
        for tb in self.beds.values():
            tb.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def check(case, rgba, depth, samples, what=""):
    orgba, odepth, n_ref = mc.oracle_frames(case.name)
    A_ref, A = orgba[..., 3], rgba[..., 3]
    tag = f"{case.name}{what}"
    assert A_ref.max() < 1.0 - mc.MIN_T, tag                       # condition on the inputs: no early termination
    assert np.isfinite(rgba).all() and np.isfinite(depth).all(), tag
    if case.pattern == "empty":                                    # every pixel an empty_pixel
        assert samples == 0 and not A.any() and not depth.any(), tag
    if not case.cone:
        got, want = mc.decode_counts(A), mc.decode_counts(A_ref)
        bad = np.argwhere(got != want)
        assert not len(bad), (f"{tag}: {len(bad)} pixels differ; first: camera {bad[0][0]} pixel (x {bad[0][2]}, y {bad[0][1]}): "
                              f"device {got[tuple(bad[0])]} samples, oracle {want[tuple(bad[0])]}")
    else:
        bar = mc.alpha_bar(A_ref)
        bad = np.argwhere(np.abs(A.astype(np.float64) - A_ref) > bar)
        assert not len(bad), (f"{tag}: {len(bad)} pixels differ by more than {bar:.3e}; first: camera {bad[0][0]} pixel (x {bad[0][2]}, y {bad[0][1]}): "
                              f"device alpha {A[tuple(bad[0])]:.7f}, oracle {A_ref[tuple(bad[0])]:.7f} "
                              f"(~{(A[tuple(bad[0])] - A_ref[tuple(bad[0])]) / (float(mc.A1) * (1 - A_ref[tuple(bad[0])])):+.2f} samples)")
    assert samples == n_ref, f"{tag}: device {samples} samples, oracle {n_ref}"
    np.testing.assert_allclose(depth, odepth, rtol=0, atol=mc.DEPTH_ATOL, err_msg=tag)
    np.testing.assert_allclose(rgba, orgba, rtol=0, atol=mc.RGBA_ATOL, err_msg=tag)


@pytest.mark.parametrize("name", [c.name for c in mc.CASES if c.group != "variants"])
def test_sample_sets_equal_brute_force(dev, name):
    case = mc.BY_NAME[name]
    check(case, *dev.render(case))


def _set(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)


def _max_march_threads(ctx) -> int:
    """the largest workgroup the marcher was compiled for: the largest multiple of 64 the option accepts"""
    for t in range(1024, 0, -64):
        try:
            ctx.set_option("march_threads", t)
        except Exception:
            continue
        ctx.set_option("march_threads", 0)
        return t
    raise AssertionError("march_threads accepts no value")


@pytest.mark.parametrize("variant", list(mc.VARIANTS))
def test_every_variant_is_held_to_the_oracles_counts(dev, variant):
    """ray sort, lane compaction, refill threshold, bricks and workgroup size only change which lane marches a ray; each is
    compared with the oracle, not with another variant.  Three cameras (1683 rays: more than one 128-entry reservation of the
    queue per wave), the middle one seeing nothing."""
    opts = dict(mc.VARIANTS[variant])
    if opts.get("march_threads") == "max":
        opts["march_threads"] = _max_march_threads(dev.ctx)
        assert opts["march_threads"] > 64
    try:
        _set(dev.ctx, opts)
        for case in (c for c in mc.CASES if c.group == "variants"):
            rgba, depth, samples = dev.render(case)
            if "march_threads" in opts:                            # the launch really ran at that size
                assert dev.ctx.get_option("march_threads_used") == opts["march_threads"]
            assert not rgba[1, ..., 3].any()                       # the camera between the two that see something
            check(case, rgba, depth, samples, f" [{variant}]")
    finally:
        _set(dev.ctx, mc.DEFAULTS)


@pytest.mark.parametrize("opts", [dict(mlp_f16=0), dict(render_arith=1), dict(render_arith=2)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_the_field_is_constant_in_every_arithmetic_mode(dev, opts):
    """zero MLP matrices give sigma = 1 and rgb = 0.5 whatever the operand format: the counts hold in every mode"""
    old = {k: dev.ctx.get_option(k) for k in opts}
    try:
        _set(dev.ctx, opts)
        for name in ("rand5-33x17", "s2-rand5-far"):
            case = mc.BY_NAME[name]
            check(case, *dev.render(case), f" [{opts}]")
    finally:
        _set(dev.ctx, old)


@pytest.mark.parametrize("name", [c.name for c in mc.CASES if c.group == "composite"])
def test_rect_cull_keeps_every_pixel_at_the_frame_edges(dev, name):
    """render_composite of a one-cell object whose box projects to one or two pixels at each frame edge, just outside the frame
    (cameras 4 and 5) and in the middle, with the rectangle-culled and the full-frame ray generator."""
    case = mc.BY_NAME[name]
    poses, orgba, odepth, want = mc.composite_reference(name)
    tb, view = dev.testbed(case), case.view()
    H, W = case.height, case.width
    dev.ctx.set_background(view, np.broadcast_to(np.asarray(mc.BG_RGBA, np.float32), (H, W, 4)).copy(), np.full((H, W), mc.BG_DEPTH, np.float32))
    out = {}
    try:
        for flag in (1, 0):
            dev.ctx.set_option("raygen_rect", flag)
            out[flag] = tb.render_composite(view, np.eye(4), np.eye(4), poses)
    finally:
        dev.ctx.set_option("raygen_rect", 1)
    np.testing.assert_array_equal(out[0], out[1])
    diff = np.abs(out[1].astype(int) - want.astype(int)).max(-1)
    assert diff.max() <= 1 and (diff > 0).mean() <= 0.02
    bg = out[1][4, 0, 0]
    assert (out[1][4] == bg).all() and (out[1][5] == bg).all()     # the box just outside the frame: background only
    got_set, want_set = (out[1] != bg).any(-1), (want != want[4, 0, 0]).any(-1)
    bad = np.argwhere(got_set != want_set)
    assert not len(bad), (f"{name}: {len(bad)} pixels differ from the oracle's non-background set; first: camera {bad[0][0]} "
                          f"({mc.COMPOSITE_AIMS[bad[0][0]][0]}) pixel (x {bad[0][2]}, y {bad[0][1]}): device {'hit' if got_set[tuple(bad[0])] else 'background'}, "
                          f"oracle {mc.decode_counts(orgba[..., 3])[tuple(bad[0])]} samples")
    assert want_set.sum() >= case.min_hits
