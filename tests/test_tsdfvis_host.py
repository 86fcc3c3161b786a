"""The colour-TSDF visual backend without a GPU: the numpy restatement of DESIGN.md section 2i (tests/tsdfvis_ref.py) against
analytic scenes, PathConfig's vis_backend, and the ray caster's host arithmetic (csrc/tsdfvis_rect.h) as a stand-alone program
under the address and undefined-behaviour sanitizers."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import tsdfvis_cases as cases
from tests import tsdfvis_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_facing_the_camera_is_hit_within_a_voxel():
    """The background alone (the candidate is off screen): every pixel that hits lies within one voxel of the plane's depth, the
    hits cover the plane's observed part, and the colour is the frames' checker."""
    frames, depth, (hit, t, rgb) = cases.expected("48x40", names=("off",))
    assert hit.mean() > 0.3
    err = np.abs(t[hit] - cases.PLANE_Z)
    print(f"plane: {hit.sum()} of {hit.size} pixels hit, max |t - z| = {err.max():.5f} m (voxel {cases.BG_VOXEL})")
    assert err.max() <= cases.BG_VOXEL
    assert (frames[0] == rgb).all() and (depth[0][hit] == t[hit]).all() and np.isinf(depth[0][~hit]).all()
    assert (rgb[~hit] == 0).all() and rgb[hit][:, 0].min() >= 40 and rgb[hit][:, 0].max() <= 190       # between the checker's two reds


def test_sphere_in_front_of_the_plane_is_nearer_on_its_silhouette():
    frames, depth, (hit, t, _) = cases.expected("48x40", names=("front",))
    v = cases.VIEWS["48x40"]
    ii, jj = np.meshgrid(np.arange(v.height), np.arange(v.width), indexing="ij")
    dx, dy = (jj - float(v.cx)) / float(v.fx), (ii - float(v.cy)) / float(v.fy)
    c = cases.SPHERE_C
    b = dx * c[0] + dy * c[1] + c[2]
    # pixels well inside the silhouette (the rim is lost to the masks' erosion): all hit, nearer than the plane, in the sphere's colour
    inside = b * b - (dx * dx + dy * dy + 1) * (c @ c - (cases.SPHERE_R - 0.014) ** 2) > 0
    assert inside.sum() > 20
    print(f"sphere: {inside.sum()} pixels inside, depth {depth[0][inside].min():.4f} .. {depth[0][inside].max():.4f} m")
    assert (depth[0][inside] < cases.PLANE_Z - 0.08).all() and (depth[0][inside] >= cases.SPHERE_C[2] - cases.SPHERE_R - cases.MV_VOXEL).all()
    assert (frames[0][inside][:, 0] >= 190).all()                                             # red 200
    assert (depth[0][hit & ~inside] >= depth[0][inside].max()).all()                          # and the plane behind it everywhere else


def test_pathconfig_vis_backend_round_trip_and_refusals(tmp_path):
    from dream2real_amd.dream2real import PathConfig
    src = json.load(open(os.path.join(REPO, "tests", "golden", "ref_config_shopping_pcd.json")))
    src["engine"]["use_vis_pcds"] = False
    src["engine"]["vis_backend"] = "tsdf"
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(src))
    cfg = PathConfig.from_json(str(p), str(tmp_path))
    assert cfg.vis_backend == "tsdf"
    del src["engine"]["vis_backend"]
    p.write_text(json.dumps(src))
    assert PathConfig.from_json(str(p), str(tmp_path)).vis_backend == "default"
    src["engine"]["vis_backend"] = "voxels"
    p.write_text(json.dumps(src))
    with pytest.raises(ValueError, match="default.*tsdf"):
        PathConfig.from_json(str(p), str(tmp_path))
    src["engine"]["vis_backend"] = "tsdf"
    src["engine"]["use_vis_pcds"] = True
    p.write_text(json.dumps(src))
    with pytest.raises(ValueError, match="use_vis_pcds"):
        PathConfig.from_json(str(p), str(tmp_path))


def test_rectangle_helper_under_the_sanitizers(tmp_path):
    """csrc/tsdfvis_rect.h in a program of its own, built with -fsanitize=address,undefined: rigidity, the rectangle of a box in
    front, clipped, behind the near plane, empty, and with non-finite input."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (g++ or clang++): it is part of the toolchain this project builds with"
    exe = str(tmp_path / "tsdfvis_host")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        os.path.join(REPO, "tests", "tsdfvis_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout, r.stderr)
