"""The rule of DESIGN.md section 2k on the CPU: hand vectors for the fill and the vote of the numpy restatement
(tests/labeltrack_ref.py), what the rule reaches on the scene of tests/labeltrack_cases.py, and csrc/labeltrack_grid.h in a program of
its own under the sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import labeltrack_cases as lc
from tests import labeltrack_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = ref.UNKNOWN


def _fill(labels, d16, tau_mm=10, grow=1):
    return ref.fill(np.array(labels, np.uint8), np.array(d16, np.uint16), tau_mm, grow)[0].tolist()


# ------------------------------------------------------------------------------------------------ (a) the fill by hand

def test_labels_do_not_cross_a_depth_step():
    d = [[500, 501, 520, 521, 522]]                                       # a step of 19 mm in the middle, tau 10
    assert _fill([[1, U, U, U, 2]], d, grow=1) == [[1, 1, U, 2, 2]]
    assert _fill([[1, U, U, U, 2]], d, grow=8) == [[1, 1, 2, 2, 2]]         # the middle pixel belongs to the far side: 520 - 501 > 10
    assert _fill([[1, U, U, U, U]], d, grow=64) == [[1, 1, U, U, U]]        # ... and nothing crosses, however long it grows
    assert _fill([[1, U, U, U, U]], d, tau_mm=19, grow=64) == [[1, 1, 1, 1, 1]]
    assert _fill([[1, U, U, U, U]], d, tau_mm=18, grow=64) == [[1, 1, U, U, U]]


def test_a_pixel_without_depth_takes_and_does_not_hand_on():
    # between two labels: W comes before E
    assert _fill([[1, U, 2]], [[500, 0, 500]]) == [[1, 1, 2]]
    # N before W before E before S
    lab = [[U, 3, U], [1, U, 2], [U, 4, U]]
    dep = [[0, 500, 0], [500, 0, 500], [0, 500, 0]]
    assert _fill(lab, dep)[1][1] == 3
    lab[0][1] = U
    assert _fill(lab, dep)[1][1] == 1
    lab[1][0] = U
    assert _fill(lab, dep)[1][1] == 2
    lab[1][2] = U
    assert _fill(lab, dep)[1][1] == 4
    # a label reaches a pixel without depth across any step, runs along pixels without depth, and stops where depth starts again
    assert _fill([[1, U, U, U, U]], [[500, 0, 0, 900, 900]], grow=64) == [[1, 1, 1, U, U]]
    assert _fill([[1, U, U, U, 2]], [[500, 0, 0, 0, 900]], grow=1) == [[1, 1, U, 2, 2]]
    # depth outside 0 < z <= 3 m is no depth
    assert _fill([[1, U, U]], [[500, 3001, 3001]], grow=2) == [[1, 1, 1]]
    assert _fill([[1, U, U]], [[500, 3000, 3000]], grow=2, tau_mm=65535) == [[1, 1, 1]]
    assert _fill([[1, U, U]], [[500, 3000, 3000]], grow=2) == [[1, U, U]]


def test_the_smallest_difference_wins_and_a_tie_goes_to_the_earlier_neighbour():
    assert _fill([[1, U, 2]], [[505, 500, 497]]) == [[1, 2, 2]]            # 5 against 3
    assert _fill([[1, U, 2]], [[503, 500, 497]]) == [[1, 1, 2]]            # 3 against 3: W before E
    lab = [[U, 3, U], [1, U, 2], [U, 4, U]]
    assert _fill(lab, [[0, 504, 0], [504, 500, 496], [0, 496, 0]])[1][1] == 3          # four ties: N
    assert _fill(lab, [[0, 504, 0], [504, 500, 496], [0, 497, 0]])[1][1] == 4          # S is nearest
    assert _fill(lab, [[0, 511, 0], [504, 500, 496], [0, 511, 0]])[1][1] == 1          # N and S do not give at all
    # a sweep reads the image it started from: two unknown neighbours do not feed each other within one sweep
    assert _fill([[1, U, U, U]], [[500, 500, 500, 500]], grow=1) == [[1, 1, U, U]]
    assert _fill([[1, U, U, U]], [[500, 500, 500, 500]], grow=3) == [[1, 1, 1, 1]]


def test_launches_that_changed_a_pixel_are_counted_in_eights():
    lab, dep = np.full((1, 20), U, np.uint8), np.full((1, 20), 500, np.uint16)
    lab[0, 0] = 7
    for grow, launches, reached in ((0, 0, 1), (7, 1, 8), (8, 1, 9), (9, 2, 10), (16, 2, 17), (19, 3, 20), (24, 3, 20), (64, 3, 20)):
        out, n = ref.fill(lab, dep, 10, grow)
        assert n == launches and int((out == 7).sum()) == reached, (grow, n, (out == 7).sum())


# ------------------------------------------------------------------------------------------------ (b) Boyer-Moore by hand

def test_boyer_moore_counts_up_to_255_down_to_0_and_replaces():
    s = 0
    for k in range(300):
        s = ref.boyer_moore(s, 5)
        assert s == (5 | min(k + 1, 255) << 8)
    for k in range(255):
        s = ref.boyer_moore(s, 9)
        assert s == (5 | (254 - k) << 8)                                  # the old label byte stays, down to count 0
    assert s == 5
    s = ref.boyer_moore(s, 9)
    assert s == (9 | 1 << 8)
    assert ref.boyer_moore(ref.boyer_moore(s, 5), 0) == (0 | 1 << 8)      # the background is a label like any other


def test_the_vote_of_the_restatement_is_that_rule_per_voxel():
    """One 1 x 1 frame straight down on a column of voxels: those within the band of the pixel's depth vote, the others keep their word."""
    lo, n, voxel, band = ref.grid([[0, 0, -0.02], [0, 0, 0.02]], 0.004, 2)
    pose = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0.2], [0, 0, 0, 1]], np.float32)
    k4 = np.array([50.0, 50.0, 0.0, 0.0])
    vol = np.zeros((n[2], n[1], n[0]), np.uint16)
    vol[:, :, :] = 4 | 2 << 8
    d16 = np.array([[202]], np.uint16)                                    # the surface 2 mm below z = 0: no voxel sits on the band's edge
    ref.vote(vol, lo, n, voxel, band, d16, pose, k4, np.array([[6]], np.uint8))
    z = (np.arange(n[2]) + lo[2]) * 0.004
    near = np.abs(z + 0.002) <= 0.008
    col = vol[:, -lo[1], -lo[0]]
    assert near.sum() == 4 and (col[near] == (4 | 1 << 8)).all() and (col[~near] == (4 | 2 << 8)).all()
    ref.vote(vol, lo, n, voxel, band, d16, pose, k4, np.array([[U]], np.uint8))                   # an unknown pixel votes nothing
    ref.vote(vol, lo, n, voxel, band, np.array([[0]], np.uint16), pose, k4, np.array([[6]], np.uint8))     # nor does one without depth
    assert (col[near] == (4 | 1 << 8)).all()
    off = vol.copy()
    off[:, -lo[1], -lo[0]] = 4 | 2 << 8
    assert (off == (4 | 2 << 8)).all()                                     # no other column was touched


# ------------------------------------------------------------------------------------------------ (c) what the rule reaches

# The restatement at the defaults (voxel 0.004, band 2, tau 10, grow 64), labels0 = frame 0's truth, recorded in docs/history/r28.md.
# Per frame 1 .. 7 of the arc: share of pixels equal to the truth, IoU of the box, of the larger and of the smaller sphere.
ARC = {1: (0.9997, 0.9944, 1.0, 1.0), 2: (0.9958, 0.9341, 1.0, 0.9947), 3: (0.9980, 0.9652, 1.0, 1.0), 4: (0.9952, 0.9331, 1.0, 0.9835),
       5: (0.9984, 0.9716, 1.0, 1.0), 6: (0.9956, 0.9380, 1.0, 0.9663), 7: (0.9973, 0.9532, 1.0, 0.9934)}
# the full orbit, frames 8 .. 23: the share of pixels alone is held (the box's IoU falls to 0.71 at frame 18: the crease split of 2k)
ORBIT_ACC = {8: 0.9930, 9: 0.9964, 10: 0.9925, 11: 0.9964, 12: 0.9923, 13: 0.9941, 14: 0.9934, 15: 0.9923, 16: 0.9933, 17: 0.9921,
             18: 0.9882, 19: 0.9924, 20: 0.9886, 21: 0.9938, 22: 0.9920, 23: 0.9968}
MARGIN = 0.02                   # the restatement is deterministic: the margin is for a later change of the scene helper, nothing else


def test_what_the_rule_reaches_on_the_arc():
    _, truth, _ = lc.frames(lc.N_ARC)
    labels, stats, vol, dims, lo = lc.reference(lc.N_ARC)
    acc, iou = lc.accuracy(labels, truth[:lc.N_ARC])
    for f in range(lc.N_ARC):
        print(f"frame {f}: accuracy {acc[f]:.4f}, IoU box {iou[f, 0]:.4f} spheres {iou[f, 1]:.4f} {iou[f, 2]:.4f}, stats {stats[f].tolist()}")
    assert np.array_equal(labels[0], truth[0]) and stats[0].tolist() == [lc.W * lc.H, 0, 0, 0]
    assert dims.tolist() == [51, 51, 33] and lo.tolist() == [-25, -25, -10] and vol.shape == (33, 51, 51)
    for f, want in ARC.items():
        got = (acc[f], iou[f, 0], iou[f, 1], iou[f, 2])
        assert all(g >= w - MARGIN for g, w in zip(got, want)), (f, got, want)
    assert set(np.unique(labels).tolist()) == {0, 1, 2, 3}                # 255 never leaves the unit


def test_accuracy_over_the_full_orbit():
    _, truth, _ = lc.frames(24)
    labels = lc.reference(24)[0]
    assert np.array_equal(labels[:lc.N_ARC], lc.reference(lc.N_ARC)[0])  # a frame depends on the frames before it alone
    acc, iou = lc.accuracy(labels, truth)
    for f in range(lc.N_ARC, 24):
        print(f"frame {f}: accuracy {acc[f]:.4f}, IoU box {iou[f, 0]:.4f} spheres {iou[f, 1]:.4f} {iou[f, 2]:.4f}")
    for f, want in ORBIT_ACC.items():
        assert acc[f] >= want - MARGIN, (f, acc[f], want)


def test_the_ray_caster_with_primitives_gives_the_tracking_scene_its_depth():
    from tests import camtrack_cases, tsdf_scene
    d16, truth, poses = lc.frames(4)
    for k in (0, 3):
        assert np.array_equal(d16[k], camtrack_cases.raycast(tsdf_scene.cameras(24)[k]))
    assert all((truth[0] == p).sum() > 300 for p in (lc.SLAB, lc.BOX, lc.SPHERE_A, lc.SPHERE_B))


# ------------------------------------------------------------------------------------------------ (d) the host header

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (g++ or clang++): it is part of the toolchain this project builds with"
    exe = str(tmp_path_factory.mktemp("labeltrack") / "labeltrack_host")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        os.path.join(REPO, "tests", "labeltrack_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


GRIDS = [
    ("the scene", 0.004, 2, lc.BOUNDS.reshape(-1)),
    ("the scene at 2 mm, band 1", 0.002, 1, lc.BOUNDS.reshape(-1)),
    ("all negative", 0.004, 2, [-0.5, -0.31, -0.2, -0.1, -0.01, -0.05]),
    ("straddling zero, band 8", 0.004, 8, [-0.013, -0.001, -0.1, 0.017, 0.001, 0.1]),
    ("bounds exactly on voxels", 0.004, 1, [-0.008, 0.0, 0.004, 0.012, 0.0, 0.004]),
    ("bounds on voxels at 2 mm", 0.002, 2, [-0.008, -0.002, 0.0, 0.008, 0.002, 0.006]),
    ("a power-of-two voxel, exact in every format", 0.00390625, 2, [-0.125, 0.0, 0.0625, 0.125, 0.03125, 0.0625]),
    ("a single point", 0.004, 1, [0.1, 0.1, 0.1, 0.1, 0.1, 0.1]),
]


@pytest.mark.parametrize("name,voxel,band,bounds", GRIDS, ids=[g[0] for g in GRIDS])
def test_grid_of_the_header_equals_the_restatement(host_exe, name, voxel, band, bounds):
    r = subprocess.run([host_exe, "grid", repr(float(voxel)), str(band)] + [repr(float(b)) for b in bounds], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = [int(x) for x in r.stdout.split()]
    lo, n, _, _ = ref.grid(np.array(bounds, np.float64).reshape(2, 3), voxel, band)
    assert got == [0] + lo.tolist() + n.tolist() + [int(n.prod())], (name, got)


def test_refusals_of_the_header_under_the_sanitizers(host_exe):
    r = subprocess.run([host_exe, "refusals"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout, r.stderr)


def test_library_grid_call_and_struct_mirror_without_a_gpu(tmp_path):
    """d2r_labeltrack_grid is host only: the same numbers through the library, refusals as codes; the ctypes mirror of
    d2r_labeltrack_params has the layout a C compiler gives the header's struct."""
    from dream2real_amd import _lib, segmentation
    for _, voxel, band, bounds in GRIDS:
        dims, lo = segmentation.labeltrack_grid(bounds, voxel, band)
        want_lo, want_n, _, _ = ref.grid(np.array(bounds, np.float64).reshape(2, 3), voxel, band)
        assert dims.tolist() == want_n.tolist() and lo.tolist() == want_lo.tolist()
    with pytest.raises(_lib.D2RError, match="band_voxels"):
        segmentation.labeltrack_grid(lc.BOUNDS, 0.004, 9)
    with pytest.raises(_lib.D2RError, match="2\\^31"):
        segmentation.labeltrack_grid(lc.BOUNDS, 1e-5, 2)
    P = segmentation.LabeltrackParams
    assert [f for f, _ in P._fields_] == ["voxel", "band_voxels", "tau_mm", "grow"]
    gcc = shutil.which("gcc")
    assert gcc, "no gcc: it is part of the toolchain this project builds with"
    src = tmp_path / "layout.c"
    fields = "".join(f'printf("%zu ", offsetof(d2r_labeltrack_params, {f}));' for f, _ in P._fields_)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "d2r.h"\nint main(void) { printf("%zu ", sizeof(d2r_labeltrack_params)); ' + fields + " return 0; }\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout.split()]
    assert got == [ctypes.sizeof(P)] + [getattr(P, f).offset for f, _ in P._fields_]


def test_engine_refuses_an_unknown_tracker_name(tmp_path):
    from dream2real_amd.dream2real import ImaginationEngine, PathConfig
    cfg = PathConfig(data_dir=str(tmp_path), sample_res=[2, 2, 1, 1, 1, 1])
    with pytest.raises(ValueError, match="xmem"):
        ImaginationEngine(cfg, None, None, proposer=lambda image: None, tracker="xmem")
    with pytest.raises(ValueError, match="proposer= is missing"):
        ImaginationEngine(cfg, None, None, tracker="geometric")
    assert ImaginationEngine(cfg, None, None, proposer=lambda image: None, tracker="geometric").tracker == "geometric"
