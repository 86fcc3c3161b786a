"""The cases of tests/tsdf_edge_cases.py can fail: on the CPU, with the numpy restatement alone (tests/tsdf_ref.py), each case is
shown to reach the edge of DESIGN.md section 2c it is named for, and each of a list of wrong rules is shown to change an output
that tests/test_tsdf_edges_gpu.py compares.  Nothing here needs a device.

Three conditions hold in a narrower form than one might write them down first, for reasons of arithmetic, not of the code under test:
  * "the eroded mask differs from the input mask" cannot hold at k = 1 (erosion by one pixel is the identity) nor on the 1 x 1 frame
    (its pixel's window is the pixel and the border, which counts as set): there the test asserts the identity instead;
  * the wrong rule "zc >= 0 accepted" cannot change any output: at zc == 0 the pixel (fx xc) / zc is +-inf or NaN and fails the frame
    test under either rule.  The case on_plane holds 1024 such voxels, and the test asserts that the outputs stay the same;
  * one block cannot hold bounds padded by 8 voxels on both sides, so the touch-word grids (one block high) use trunc = 4 voxels.
"""
import ctypes

import numpy as np
import pytest

from tests import tsdf_edge_cases as E
from tests import tsdf_ref


def kept_rows(name):
    vol = E.fuse(E.case(name), probe=True)
    vol.marching_cubes(E.WEIGHT_THRESHOLD)
    return vol, set(np.unique(vol.probe["cube"]).tolist()) - {0}


# ------------------------------------------------------------------------------------------------ the grids are the intended ones
@pytest.mark.parametrize("name", list(E.BUILDERS))
def test_bounds_give_the_intended_grid(name):
    c = E.case(name)
    vol = tsdf_ref.Volume(c["bounds"], c["voxel"], c["trunc"]) if name == "many_blocks" else E.reference(name)[0]
    assert tuple(int(v) for v in vol.nb) == c["nb"] and tuple(int(v) for v in vol.b0) == c["b0"]
    assert (c["bounds"][0] < c["bounds"][1]).all() and c["trunc"] >= c["voxel"]


# ------------------------------------------------------------------------------------------------ a. all 254 cubes
def test_the_seeds_together_keep_every_triangle_producing_row():
    union = set()
    for s in E.CUBE_SEEDS:
        _, rows = kept_rows("cubes_seed%d" % s)
        print(f"seed {s}: {len(rows)} distinct rows")
        assert len(rows) >= 240
        union |= rows
    assert union == set(range(1, 255))


# ------------------------------------------------------------------------------------------------ b. seams
def test_seams_has_kept_cubes_in_blocks_beside_never_stamped_ones():
    vol, _ = kept_rows("seams")
    ever = vol.ever
    pad = np.ones(tuple(n + 2 for n in ever.shape), bool)
    pad[1:-1, 1:-1, 1:-1] = ever
    beside = np.zeros_like(ever)
    for ax in range(3):
        for sh in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[ax] = slice(sh, sh + ever.shape[ax])
            beside |= ever & ~pad[tuple(sl)]
    cz, cy, cx = np.nonzero(vol.probe["cube"])
    on_seam = beside[cz // 16, cy // 16, cx // 16]
    print(f"seams: {int(ever.sum())} of {ever.size} blocks stamped, {int(beside.sum())} of them beside a never-stamped one, {int(on_seam.sum())} of {len(cz)} kept cubes in those")
    assert beside.sum() >= 1 and on_seam.sum() >= 1


# ------------------------------------------------------------------------------------------------ c. exact zeros, sdf == -trunc
def test_zeros_holds_exact_zeros_beside_negatives_and_degenerate_triangles():
    vol, out = E.reference("zeros")
    zero = (vol.w >= 3) & (vol.tsdf == 0)
    beside = zero[:, :, :-1] & (vol.tsdf[:, :, 1:] < 0) & (vol.w[:, :, 1:] >= 3)
    b = out["verts"][out["tris"]].view(np.uint32)
    degenerate = (b[:, 0] == b[:, 1]).all(1) | (b[:, 1] == b[:, 2]).all(1) | (b[:, 0] == b[:, 2]).all(1)
    one = E.reference("minus_one")[0]
    minus = (one.w == 1) & (one.tsdf == -1)
    print(f"zeros: {int(beside.sum())} exact zeros beside a negative voxel, {int(degenerate.sum())} of {len(b)} triangles with two identical vertices; "
          f"minus_one: {int(minus.sum())} voxels at exactly -1 after one frame")
    assert beside.sum() >= 16 and degenerate.sum() >= 1 and minus.sum() >= 16
    assert len(E.reference("minus_one")[1]["tris"]) == 0          # weight 1 < 3: the "seen in no frame" answer on the device


# ------------------------------------------------------------------------------------------------ d. faces
@pytest.mark.parametrize("n", range(6))
def test_face_cases_leave_the_grid_and_reach_the_outermost_cubes(n):
    c = E.case("face_%d" % n)
    vol = E.fuse(c, probe=True)
    verts, _ = vol.marching_cubes(E.WEIGHT_THRESHOLD)
    axis, high = n // 2, n % 2 == 0
    layer = np.floor(verts[:, axis].astype(np.float64) / float(c["voxel"])).astype(np.int64)
    want = 14 if high else 0                                      # the last cube that x + 1 < nv admits, or the first
    outside = int(vol.probe["steps_outside"][axis][1 if high else 0])
    print(f"face {n}: {outside} band samples beyond the face, {int((layer == want).sum())} of {len(verts)} vertices in cube layer {want}")
    assert outside >= 1 and (layer == want).sum() >= 1


# ------------------------------------------------------------------------------------------------ e. camera inside
def test_inside_stamps_blocks_behind_and_just_before_the_camera():
    vol = E.fuse(E.case("inside"), probe=True, frames=1)
    print("inside, one frame:", {k: vol.probe[k] for k in ("zc_nonpositive", "zc_tiny", "zc_zero")})
    assert vol.probe["zc_nonpositive"] >= 100 and vol.probe["zc_tiny"] >= 1
    vol = E.fuse(E.case("on_plane"), probe=True, frames=1)
    assert vol.probe["zc_zero"] == 32 * 32 and (vol.w[:, :, 0] == 0).all() and (vol.w[:, :, 1] > 0).any()


# ------------------------------------------------------------------------------------------------ g. band ratios
def test_band_steps_round_half_to_even():
    for ratio, steps in zip(E.BAND_RATIOS, E.BAND_STEPS):
        vol = E.reference("band_%g" % ratio)[0]
        assert float(vol.trunc) / float(vol.voxel) == ratio and vol.steps == steps
    assert E.BAND_STEPS == (1, 2, 4, 8)


# ------------------------------------------------------------------------------------------------ h. erosion and frame shapes
@pytest.mark.parametrize("size", E.SIZES, ids=["%dx%d" % s for s in E.SIZES])
def test_every_pixel_is_read_with_a_full_mask(size):
    W, H = size
    c = E.erosion(W, H, 1, full=True)
    c["frames"][0][0][:] = 1000
    vol = E.fuse(c, probe=True)
    read = vol.probe["pixels_read"][0]
    assert read.shape == (H, W) and read.all()
    for r, col in ((0, 0), (H - 1, W - 1), (H // 2, W // 3)):     # ... by the voxel pixel_voxel names
        assert vol.w[E.pixel_voxel(c, r, col)] == 1


@pytest.mark.parametrize("name", E.ERODE_NAMES + ["erode_5x3_k32_full"])
def test_erosion_cases_erode(name):
    c = E.case(name)
    depth, _, _, _, k = c["frames"][0]
    H, W = depth.shape
    vol = E.reference(name)[0]
    survived = np.zeros((H, W), np.int64)                         # frames in which the pixel's mask bit survives the erosion
    for _, mask, _, _, kk in c["frames"]:
        out = tsdf_ref.erode(mask, kk)
        print(f"{name}: {int(mask.sum())} of {mask.size} set, {int(out.sum())} after erosion")
        assert kk == k and mask.shape == (H, W)
        if k == 1 or (W, H) == (1, 1) or name.endswith("_full"):
            assert (out == mask).all() and (not name.endswith("_full") or (mask.all() and k > W))
        else:
            assert (out != mask).any()
        assert ((vol.valid_depth(depth, mask, k) > 0) == (out & (depth > 0) & (depth <= 3000))).all()
        survived += out
    # a pixel at 1000 mm shows in its own voxel: weight = the number of frames in which it was valid
    for r in range(H):
        for col in range(W):
            if depth[r, col] == 1000:
                assert vol.w[E.pixel_voxel(c, r, col)] == survived[r, col]


@pytest.mark.parametrize("size,k", E.ERODE, ids=["%dx%d_k%d" % (s[0], s[1], k) for s, k in E.ERODE])
def test_each_hole_removes_its_k_by_k_footprint(size, k):
    W, H = size
    a, b = k // 2, k - 1 - k // 2
    holes = E.holes_of(W, H, k)
    assert {c for _, c in holes} == {c for c in (0, 63, 64, W - 1, a, b, W - 1 - a, W - 1 - b) if 0 <= c < W}
    assert {r for r, _ in holes} == {r for r in (0, 31, 32, H - 1, a, b, H - 1 - a, H - 1 - b) if 0 <= r < H}
    masks = [f[1] for f in E.erosion(W, H, k)["frames"]]
    if (W, H) != (1, 1):                                          # every hole is in a mask of the case, at every k
        assert all(any(not m[r, col] for m in masks) for r, col in holes) and len(masks) == (1 if k <= 8 else len(holes))
    through = set()                                               # which halo of k_erode's 64 x 32 tile a hole is read through
    for r, col in holes:
        m = np.ones((H, W), bool)
        m[r, col] = False
        gone = ~tsdf_ref.erode(m, k)
        want = np.zeros((H, W), bool)                              # pixel (i, j) reads rows i - a .. i - a + k - 1: it sees row r for i = r - (k - 1 - a) .. r + a
        want[max(0, r - b):r + a + 1, max(0, col - b):col + a + 1] = True
        assert (gone == want).all() and gone.sum() <= k * k
        gi, gj = np.nonzero(gone)
        for side, crosses in (("left", gj // 64 > col // 64), ("right", gj // 64 < col // 64), ("top", gi // 32 > r // 32), ("bottom", gi // 32 < r // 32)):
            if crosses.any():
                through.add(side)
    if k >= 2 and W > 64 and H > 32:                              # 65 x 33 and 129 x 70: a hole is read across every side of a tile that has a halo
        assert through == ({"left", "top"} if b == 0 else {"left", "right", "top", "bottom"}), through    # k = 2 reads rows i - 1 .. i only


def test_depth_limits_show_in_the_weights():
    c = E.case("three_metres")
    vol = E.reference("three_metres")[0]
    got = {d: float(vol.w[E.pixel_voxel(c, r, col)]) for (r, col), d in E.THREE_M_PIXELS.items()}
    got[3000] = float(vol.w[E.pixel_voxel(c, 0, 0)])
    print("three_metres: weight behind the pixel at depth", got)
    assert got == {2999: 1.0, 3000: 1.0, 3001: 0.0, 65535: 0.0, 0: 0.0}
    big = E.case("erode_129x70_k1")
    depth = big["frames"][0][0]
    assert {int(depth[p]) for p in E.special_pixels(129, 70)} == set(E.SPECIAL_DEPTHS)


# ------------------------------------------------------------------------------------------------ i. many blocks
def test_many_blocks_stamps_more_than_4096_blocks_in_one_frame():
    vol, out = E.reference("many_blocks")
    print(f"many_blocks: {len(out['blocks'])} blocks stamped by its one frame")
    assert vol.frames_used == 1 and len(out["blocks"]) >= 4097


# ------------------------------------------------------------------------------------------------ j. state across calls
def test_mixed_frames_and_the_extra_frame_change_the_answer():
    c = E.case("mixed_frames")
    assert [f[0].shape for f in c["frames"]] == [(70, 129), (3, 5), (70, 129)]
    two = E.outputs(c, E.fuse(c, frames=2))
    assert E.differs(two, E.reference("mixed_frames")[1]) and E.differs(two, E.outputs(c, E.fuse(c, frames=1)))
    a, b = E.reference("cubes_seed%d" % E.CUBE_SEEDS[0])[1], E.reference("cubes_seed%d_plus" % E.CUBE_SEEDS[0])[1]
    assert E.differs(a["verts"], b["verts"])


# ------------------------------------------------------------------------------------------------ k. touch words
@pytest.mark.parametrize("nbx", E.TOUCH_NBX)
def test_touch_rows_end_in_a_partly_filled_mixed_word(nbx):
    vol, out = E.reference("touch_%d" % nbx)
    nx = int(vol.nv[0])
    assert nx == 16 * nbx and nx % 32 == 16
    for args in E.TOUCH_ARGS:
        words = out["touch"][args]
        assert words.shape[2] == (nx + 31) // 32
        last = words[:, :, -1]
        assert (last >> np.uint32(16) == 0).all()                  # bits past nx stay clear
        mixed = (last != 0) & (last != 0xffff)
        print(f"nx {nx}, threshold / contact {args}: {int(mixed.sum())} rows with a mixed last word")
        assert mixed.sum() >= 1
    assert len({out["touch"][a].tobytes() for a in E.TOUCH_ARGS}) == len(E.TOUCH_ARGS)


# ------------------------------------------------------------------------------------------------ wrong rules must show
CAUGHT_BY = {
    "anchor_low": "erode_65x33_k2",
    "border_unset": "erode_5x3_k32_full",
    "z_lt_3": "three_metres",
    "sdf_le": "minus_one",
    "rint": "erode_65x33_k1",
    "steps_floor": "band_3.5",
    "inside_le": "zeros",
    "seven_of_eight": "seams",
    "other_end": "cubes_seed1",
    "inv_fp32": "awkward_far",
}


@pytest.mark.parametrize("rule", list(CAUGHT_BY))
def test_a_wrong_rule_changes_a_compared_output(rule):
    c = E.case(CAUGHT_BY[rule])
    right = E.reference(c["name"])[1]
    wrong = E.outputs(c, E.fuse(c, rules={rule}))
    changed = [k for k in right if E.differs(right[k], wrong[k])]
    print(f"{rule} on {c['name']}: changes {changed}")
    assert changed


def test_accepting_zc_of_zero_cannot_show():
    assert set(CAUGHT_BY) | {"zc_ge_0"} == set(tsdf_ref.WRONG_RULES)
    for name in ("on_plane", "inside"):
        c = E.case(name)
        assert not E.differs(E.reference(name)[1], E.outputs(c, E.fuse(c, rules={"zc_ge_0"})))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.float32([-3.0, 0.0, 2.5]) / np.float32(0.0) + np.float32(12.0)
    assert not ((u >= 0) & (u < 24)).any()                        # -inf, NaN, +inf: outside every frame


def test_a_swapped_triangle_of_any_row_shows():
    seen = set()
    for s in E.CUBE_SEEDS:
        vol, rows = kept_rows("cubes_seed%d" % s)
        cube, vid = vol.probe["cube"], vol.probe["vid"]
        for r in sorted(rows - seen):
            only = np.where(cube == r, cube, 0)                    # the other cubes' triangles do not depend on row r
            assert (tsdf_ref.Volume.triangles(only, vid) != tsdf_ref.Volume.triangles(only, vid, swap_row=r)).any(), r
        seen |= rows
    assert seen == set(range(1, 255))


# ------------------------------------------------------------------------------------------------ refusals that need no device
def test_library_refuses_null_handles_without_a_device():
    from dream2real_amd import _lib
    lib = _lib.load()
    n = ctypes.c_uint32(0)
    f = np.zeros(16, np.float32)
    out = ctypes.c_void_p()
    assert lib.d2r_tsdf_create(None, _lib.ptr(f), 0.002, 0.016, ctypes.byref(out)) == -1 and not out.value
    lib.d2r_tsdf_destroy(None)
    d, m = np.zeros(4, np.uint16), np.zeros(4, np.uint8)
    assert lib.d2r_tsdf_integrate(None, _lib.ptr(d), _lib.ptr(m), 2, 2, _lib.ptr(f), _lib.ptr(f), 1) == -1
    assert lib.d2r_tsdf_read_voxels(None, ctypes.byref(n), None, None, None) == -1
    assert lib.d2r_tsdf_extract(None, 3.0, None, 0.02, ctypes.byref(n), ctypes.byref(n), None, None, None, None, None) == -1
    assert lib.d2r_tsdf_grid(None, _lib.ptr(f), _lib.ptr(f), _lib.ptr(f), _lib.ptr(f)) == -1
    assert lib.d2r_tsdf_touch_bits(None, 3.0, 0.002, _lib.ptr(f)) == -1
    assert lib.d2r_tsdf_solid_points(None, 3.0, ctypes.byref(n), None) == -1
