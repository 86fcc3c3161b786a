"""Camera-pose refinement on the CPU: the numpy restatement tests/camtrack_ref.py checked against finite
differences and known systems, the inputs of tests/camtrack_cases.py checked to be fair (the restatement alone meets the behaviour
conditions the GPU test asks of the library), PathConfig's cam_pose_refine, and the struct mirrors against a C compiler."""
import ctypes
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import camtrack_cases as cases
from tests import camtrack_ref as ref
from tests import tsdf_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tracking():
    d, T, m = cases.tracking_frames()
    grid = ref.grid_from_volume(cases.fuse(tsdf_ref.Volume(cases.BOUNDS), d, T, m))
    return grid, d, T, m


def _twisted(pose, k, delta):
    xi = [0.0] * 6
    xi[k] = delta
    T = [[float(x) for x in row] for row in np.asarray(pose, np.float32)[:3]]
    return ref._round(ref.apply(ref.exp_twist(xi), T))


def test_jacobian_equals_a_central_difference_of_the_residual(tracking):
    """J_k against (r(exp(+d e_k) T) - r(exp(-d e_k) T)) / 2d at pixels whose point stays inside its cell (fractions in [0.25, 0.75]:
    0.5 mm from every face; d = 2e-4 moves a point by 2e-4 m, or by 2e-4 rad x 0.45 m = 9e-5 m).  Inside a cell r is a polynomial of
    degree one per axis, so the truncation error of the central difference is of third order in d (< 1e-6).  What is left is the fp32
    evaluation: p_w carries about six roundings of values below 0.5 m (1.8e-7 m an axis), r follows with |n|_1 <= 2 times that plus
    the interpolation's own roundings (1e-8): 4e-7; two evaluations over 2d = 4e-4: 2e-3."""
    grid, d, T, m = tracking
    pose, delta, tol = T[cases.TRACKED], 2e-4, 2e-3
    keep, J, r, f = ref.rows(grid, d[cases.TRACKED], m, cases.INTRINSICS, pose, cases.THR, 1, full=True)
    inner = keep & ((f >= 0.25) & (f <= 0.75)).all(axis=1) & (np.abs(J[:, :3]).sum(axis=1) <= 2.0)
    assert inner.sum() > 300          # (the slab's top lies on a voxel plane: most of its pixels sit at a face in z)
    for k in range(6):
        kp, _, rp, _ = ref.rows(grid, d[cases.TRACKED], m, cases.INTRINSICS, _twisted(pose, k, delta), cases.THR, 1, full=True)
        km, _, rm, _ = ref.rows(grid, d[cases.TRACKED], m, cases.INTRINSICS, _twisted(pose, k, -delta), cases.THR, 1, full=True)
        use = inner & kp & km
        fd = (rp[use].astype(np.float64) - rm[use].astype(np.float64)) / (2 * delta)
        err = np.abs(fd - J[use, k]).max()
        print("twist", k, "pixels", int(use.sum()), "max |fd - J|", err)
        assert use.sum() > 300 and err <= tol, (k, err)


def test_ldlt_solves_a_known_system():
    rng = np.random.default_rng(5)
    B = rng.integers(-8, 9, (40, 6)).astype(np.float64)
    A, x = B.T @ B, np.array([1.0, -2.0, 0.5, 3.0, -0.25, 2.0])
    b = -(A @ x)                                           # xi = -A^-1 b = x; integer entries, exactly representable at scale 2^29
    sums = [int(A[i, j] * ref.SCALE) for i in range(6) for j in range(i, 6)] + [int(v * ref.SCALE) for v in b] + [0, 40]
    xi = ref.solve(sums)
    np.testing.assert_allclose(xi, x, rtol=0, atol=64 * np.finfo(np.float64).eps * np.linalg.cond(A))
    sums[0] = 0                                            # a zero pivot
    assert ref.solve(sums) is None
    A2 = np.ones((6, 6))                                   # rank one: the second pivot is 0
    assert ref.solve([int(ref.SCALE)] * 21 + [0] * 6 + [0, 6]) is None and np.linalg.matrix_rank(A2) == 1


def test_exp_is_orthonormal_and_matches_the_series():
    for xi in ([1e-3, 2e-3, -1e-3, 0.3, -0.2, 0.1], [0.0, 0.0, 0.0, 1e-7, 2e-7, 0.0], [0.01, 0, 0, 0, 0, 9.9e-5], [0, 0, 0.1, 0, 0, 1.01e-4],
               [0.5, 0.5, 0.5, 2.0, -1.0, 0.5]):
        E = np.array(ref.exp_twist([float(v) for v in xi]))
        R = E[:, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 8 * np.finfo(np.float64).eps and abs(np.linalg.det(R) - 1) <= 8 * np.finfo(np.float64).eps
        M = np.zeros((4, 4))                               # exp by its power series
        w, v = xi[3:], xi[:3]
        M[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
        M[:3, 3] = v
        S, term = np.eye(4), np.eye(4)
        for n in range(1, 30):
            term = term @ M / n
            S = S + term
        assert np.abs(S[:3] - E).max() <= 1e-14, xi


def test_the_degenerate_scene_is_reported_degenerate():
    """tests/tsdf_scene.py's sphere on a slab as its exact distance field (camtrack_cases.degenerate_field), the frames ray-cast
    analytically to millimetres: yaw about the sphere's axis is not constrained, the sixth pivot falls below PIVOT_REL of the largest
    diagonal entry from every view and at both strides, and the loop started from a perturbed pose stops degenerate at once with the
    pose it had.  What is left in that pivot is the interpolant's own floor (DESIGN.md section 2j derives h^2 / 12 per pixel).  A
    volume FUSED from the same millimetre frames is not flagged: the depth steps and the bands behind silhouettes put 7e-5 of the
    largest diagonal entry into the yaw pivot, which is noise the rule cannot tell from information (section 2j says so)."""
    d, T, m = cases.degenerate_frames()
    grid = ref.Grid(*cases.degenerate_field())
    for k in range(len(d)):
        for stride in (1, 2):
            pivots = []
            xi = ref.solve(ref.system(grid, d[k], m, cases.INTRINSICS, T[k], cases.THR, stride), pivots)
            print(k, stride, "pivots / max diag:", [p / (bound / ref.PIVOT_REL) for p, bound in pivots])
            assert xi is None and len(pivots) == 6
    start = cases.perturbed(T[cases.TRACKED], (0.002, 0.001, -0.001), (0, 0, 1), np.deg2rad(0.3))
    pose, rep = ref.refine(grid, d[cases.TRACKED], m, cases.INTRINSICS, start, cases.THR, 2)
    assert rep["status"] == "degenerate" and rep["iters"] == 1 and rep["pixels_first"] > 500
    np.testing.assert_array_equal(pose.view(np.uint32), start.view(np.uint32))


def test_an_exact_plane_is_degenerate():
    """A hand-made field that is exactly a plane (tsdf = z / trunc, every weight 1): the in-plane translations and the rotation about
    the normal have exactly zero columns, the first pivot is 0 and the loop stops with the pose it had."""
    nz, ny, nx = 16, 48, 48
    zz = (np.arange(nz, dtype=np.float32) - 8) * np.float32(0.002) / np.float32(0.016)
    grid = ref.Grid(np.broadcast_to(zz[:, None, None], (nz, ny, nx)).copy(), np.ones((nz, ny, nx), np.float32), [-24, -24, -8], 0.002, 0.016)
    pose = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0.25], [0, 0, 0, 1]], np.float32)       # looking straight down from 0.25 m
    depth = np.full((60, 80), 251, np.uint16)
    out, rep = ref.refine(grid, depth, np.ones_like(depth, np.uint8), cases.INTRINSICS[:] * [[0.25], [0.25], [1]], pose, 1.0, 1, 20, 100)
    assert rep["status"] == "degenerate" and rep["iters"] == 1 and rep["pixels_first"] > 100
    np.testing.assert_array_equal(out.view(np.uint32), pose.view(np.uint32))


@pytest.mark.parametrize("name", sorted(cases.TRACKING))
@pytest.mark.parametrize("stride", [1, 2])
def test_the_restatement_tracks_the_perturbed_frame(tracking, name, stride):
    """The behaviour conditions of the GPU test, asked of the restatement alone: converged, the final rms residual below the first,
    translation and rotation errors each at most half the perturbation's."""
    grid, d, T, m = tracking
    start, dt, angle = cases.tracking_start(name)
    pose, rep = ref.refine(grid, d[cases.TRACKED], m, cases.INTRINSICS, start, cases.THR, stride)
    et, er = ref.pose_error(pose, T[cases.TRACKED])
    print(name, stride, rep["status"], rep["iters"], "pixels", rep["pixels_first"], rep["pixels_last"], "rms", rep["rms_first"], rep["rms_last"],
          "perturbation", dt, angle, "left", et, er, "last step", rep["last_step"])
    assert rep["status"] == "converged" and rep["rms_last"] < rep["rms_first"]
    assert et <= 0.5 * dt and er <= 0.5 * angle
    # no stopping norm sits within a few fp64 ulps of the threshold: the library's count will be the same
    assert all(abs(x - ref.CONVERGED) > 1e-9 for x in rep["last_step"])
    # ... and no pivot anywhere near the degeneracy threshold: every iteration's weakest is a hundred times above it
    for sums in rep["sums"]:
        pivots = []
        ref.solve(sums, pivots)
        assert min(p / bound for p, bound in pivots) > 100


def test_too_few_pixels_returns_the_input_pose(tracking):
    grid, d, T, m = tracking
    start, _, _ = cases.tracking_start("a")
    pose, rep = ref.refine(grid, d[cases.TRACKED], m, cases.INTRINSICS, start, cases.THR, 2, 20, 10 ** 6)
    assert rep["status"] == "too_few" and rep["iters"] == 1
    np.testing.assert_array_equal(pose.view(np.uint32), start.view(np.uint32))


def test_overflow_bound_of_the_integer_scale():
    """Section 2j's derivation, in integers: under the gates every factor is at most 64 (|n| <= 4, |p x n| <= 2 * 8 * 4, |r| <= 1), a
    product at most 2^12, a term at most 2^41 after scaling, and 2^21 of them stay below 2^63; one more bit of scale would not."""
    worst = max(4.0, 2 * 8.0 * 4.0, 1.0) ** 2
    assert worst == 2 ** 12
    assert 2 ** 21 * int(worst * 2 ** ref.SCALE_LOG2) <= 2 ** 63 - 1 < 2 ** 21 * int(worst * 2 ** (ref.SCALE_LOG2 + 1))


# ---------------------------------------------------------------------------------------------------- PathConfig

def _settings(tmp_path, **engine):
    group = dict(render_distractors=False, spatial_smoothing=True, physics_only=False, use_vis_pcds=False, single_view_idx=0,
                 use_cache_dynamic_masks=False, use_cache_segs=True, use_cache_cam_poses=False, use_cache_captions=False, use_cache_phys=False,
                 use_cache_vis=False, use_cache_llm=True, use_cache_renders=False, use_cache_goal_pose=False, use_phys=True, use_phys_tsdf=True,
                 lazy_phys_mods=True, multi_view_captions=False, scene_type=0, sample_res=[2, 2, 1, 1, 1, 1], scene_centre=[0, 0, 0],
                 scene_phys_bounds=[[0, 0, 0], [1, 1, 1]], render_cam_pose_idx=[0])
    group.update(engine)
    path = str(tmp_path / "settings.json")
    json.dump({"engine": group, "camera": {"w": 64, "h": 48}}, open(path, "w"))
    return path


def test_path_config_cam_pose_refine(tmp_path):
    import dataclasses
    from dream2real_amd.dream2real import PathConfig
    cfg = PathConfig(data_dir="x", sample_res=[1] * 6)
    assert cfg.cam_pose_refine == "none" and PathConfig.CAM_POSE_REFINES == ("none", "tsdf")
    assert "cam_pose_refine" not in [f.name for f in dataclasses.fields(cfg)] and "cam_pose_refine" not in dataclasses.asdict(cfg)
    assert PathConfig(data_dir="x", sample_res=[1] * 6, vis_backend="tsdf", cam_pose_refine="tsdf").cam_pose_refine == "tsdf"
    assert PathConfig(data_dir="x", sample_res=[1] * 6, use_vis_pcds=True, pcds_type=0, cam_pose_refine="tsdf").cam_pose_refine == "tsdf"
    with pytest.raises(ValueError, match="not one of"):
        PathConfig(data_dir="x", sample_res=[1] * 6, vis_backend="tsdf", cam_pose_refine="icp")
    with pytest.raises(ValueError, match="use_cache_cam_poses"):
        PathConfig(data_dir="x", sample_res=[1] * 6, vis_backend="tsdf", cam_pose_refine="tsdf", use_cache_cam_poses=True)
    with pytest.raises(ValueError, match="use_vis_pcds or"):
        PathConfig(data_dir="x", sample_res=[1] * 6, cam_pose_refine="tsdf")
    assert PathConfig.from_json(_settings(tmp_path), "x").cam_pose_refine == "none"
    assert PathConfig.from_json(_settings(tmp_path, vis_backend="tsdf", cam_pose_refine="tsdf"), "x").cam_pose_refine == "tsdf"
    assert PathConfig.from_json(_settings(tmp_path, vis_backend="tsdf"), "x", cam_pose_refine="tsdf").cam_pose_refine == "tsdf"
    with pytest.raises(ValueError, match="use_vis_pcds or"):
        PathConfig.from_json(_settings(tmp_path, cam_pose_refine="tsdf"), "x")


# ---------------------------------------------------------------------------------------------------- the ABI's two structs

def test_struct_mirrors_have_the_c_layout(tmp_path):
    """cam_pose_opt's ctypes mirrors against sizeof / offsetof of include/d2r.h's d2r_camtrack_params and d2r_camtrack_report."""
    from dream2real_amd import cam_pose_opt
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    pairs = (("d2r_camtrack_params", cam_pose_opt.CamtrackParams), ("d2r_camtrack_report", cam_pose_opt.CamtrackReport))
    lines = []
    for c_name, cls in pairs:
        lines.append(f'printf("{c_name} %zu\\n", sizeof({c_name}));')
        lines += [f'printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));' for f, _ in cls._fields_]
    lines.append('printf("consts %d %d %d\\n", D2R_CAMTRACK_SUMS, D2R_CAMTRACK_SCALE_LOG2, D2R_CAMTRACK_MAX_ITERS);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "d2r.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split(None, 1) for line in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.splitlines())
    assert out["consts"].split() == [str(cam_pose_opt.SUMS), str(cam_pose_opt.SCALE_LOG2), str(cam_pose_opt.MAX_ITERS_CAP)]
    assert cam_pose_opt.SUMS == ref.SUMS and cam_pose_opt.SCALE_LOG2 == ref.SCALE_LOG2 and cam_pose_opt.STATUS == ref.STATUS
    for c_name, cls in pairs:
        assert int(out[c_name]) == ctypes.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(out[f"{c_name}.{f}"]) == getattr(cls, f).offset, (c_name, f)
