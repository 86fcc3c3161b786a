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


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_sampler_header_under_the_sanitizers_equals_the_restatements_bit_for_bit(tmp_path):
    """csrc/tsdf_sample.h in a program of its own (tests/tsdf_sample_host_main.cpp), built like the rectangle helper plus
    -ffp-contract=off: a volume of two blocks by one by one with a negative lo on x, random (tsdf, weight) with weights exactly at the
    threshold and just below, the second block's flag cleared.  Every point goes through three readers: the whole grid with the block
    flags (the ray caster's form), the whole grid without them (the tracker's), a smaller box of the caller's with them.  The cell,
    the fractions, the observed flag and the value are tests/tsdfvis_ref.py's _sample, value and gradient tests/tsdf_ref.py's
    lerp3_grad, and on the points a small depth image back-projects to, the tracker's rows are tests/camtrack_ref.py's
    rows(full=True): all compared as bits.  The address sanitizer watches the loads: the voxel array is exactly the grid."""
    from tests import camtrack_ref, tsdf_ref
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (g++ or clang++): it is part of the toolchain this project builds with"
    f32 = np.float32
    voxel, trunc, thr = f32(1.0 / 64.0), f32(0.05), f32(3.0)
    vol = tsdf_ref.Volume([[-0.2, 0.05, 0.3], [0.2, 0.2, 0.45]], voxel, f32(1.0 / 32.0))
    vol.trunc = trunc                                        # (the bounds were padded by a dyadic one; rows scales by this one)
    assert list(vol.nb) == [2, 1, 1] and list(vol.b0) == [-1, 0, 1]
    r = np.random.default_rng(7)
    vol.tsdf[:] = r.uniform(-1, 1, vol.tsdf.shape).astype(np.float32)
    vol.w[:] = r.choice(np.array([thr, np.nextafter(thr, f32(0)), 2.0, 4.0, 9.0], np.float32), vol.w.shape, p=[0.25, 0.1, 0.05, 0.3, 0.3])
    vol.w[2:9, 2:9, 2:9] = 5.0                               # a stretch of observed cells in the first block ...
    vol.w[2:9, 2:9, 12:24] = 5.0                             # ... and one across the seam of the two
    vol.ever[:] = True
    vol.ever[0, 0, 1] = False
    lo = (vol.b0 * 16).astype(np.int64)
    nv = vol.nv.astype(np.int64)
    grid = (lo, lo + nv - 2)
    small = (lo + [3, 2, 1], lo + nv - 2 - [2, 3, 1])
    modes = [(1, grid), (0, grid), (1, small)]

    def at(c, frac=(0.25, 0.5, 0.75)):                       # dyadic: the point of cell c at these fractions, exactly
        return (np.asarray(c, np.float64) + frac) * float(voxel)
    mid = lo + [5, 5, 5]
    pts = [at(grid[0]), at(grid[1]), at(small[0]), at(small[1]), at(mid, (0.0, 0.0, 0.0)), at(mid, (0.0, 0.5, 0.0)), at(lo + [4, 3, 3]),
           at(lo + [20, 4, 4]), at(lo + [15, 4, 4]), at(lo + [14, 3, 3]),
           [np.nan, 0.1, 0.3], [0.1, np.inf, 0.3], [0.1, 0.1, -np.inf], [np.inf, np.nan, -np.inf], [1e30, 0.1, 0.3], [-1e30, 0.1, 0.3]]
    for a in range(3):
        for box in (grid, small):
            for c in (box[0][a] - 1, box[1][a] + 1):
                q = mid.copy()
                q[a] = c
                pts.append(at(q))
    pts = np.asarray(pts, np.float64).astype(np.float32)
    assert pts[6][0] < 0                                     # a negative coordinate; [7]: the cleared block; [8]: astride the seam
    # the tracker's points: a 16 x 12 depth image through camtrack_ref.rows' own back-projection
    K = np.array([[20.0, 0, 8.0], [0, 20.0, 0.0], [0, 0, 1.0]])
    pose = np.eye(4, dtype=np.float32)
    depth = r.integers(240, 520, (12, 16)).astype(np.uint16)
    mask = np.ones((12, 16), np.uint8)
    z = depth.reshape(-1).astype(np.float32) / f32(1000)
    vv, uu = np.meshgrid(np.arange(12), np.arange(16), indexing="ij")
    back = np.stack([((uu.reshape(-1).astype(np.float32) - f32(8)) / f32(20)) * z, ((vv.reshape(-1).astype(np.float32) - f32(0)) / f32(20)) * z, z], 1)
    n_edge = len(pts)
    pts = np.concatenate([pts, back.astype(np.float32)])

    src, dst, exe = str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "tsdf_sample_host")
    with open(src, "wb") as f:
        f.write(np.array(list(nv) + list(vol.nb) + list(lo) + [len(pts), len(modes)], "<i4").tobytes())
        f.write(np.array([voxel, thr], "<f4").tobytes())
        f.write(np.stack([vol.tsdf, vol.w], -1).astype("<f4").tobytes())
        f.write(vol.ever.astype(np.uint8).tobytes())
        for flags, (clo, chi) in modes:
            f.write(np.array([flags], "<i4").tobytes() + np.array(list(clo) + list(chi), "<f4").tobytes())
        f.write(pts.astype("<f4").tobytes())
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-ffp-contract=off", os.path.join(REPO, "tests", "tsdf_sample_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    b = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert b.returncode == 0 and b.stdout.strip() == "ok", (b.returncode, b.stdout, b.stderr)
    rec = np.dtype([("cell", "<i4"), ("obs", "<i4"), ("base", "<i8"), ("f", "<f4", 3), ("val", "<f4"), ("g", "<f4", 3)])
    got = np.fromfile(dst, rec).reshape(len(modes), len(pts))

    met = {}
    for (flags, box), out in zip(modes, got):
        ok, val, q, fr, inside, c = ref._sample(vol, pts, thr, box)      # (with the flags; `inside` is the box alone)
        flag = vol.ever[q[2] >> 4, q[1] >> 4, q[0] >> 4]
        if not flags:                                                    # the tracker's reader: the weights decide alone
            ok = inside.copy()
            for k in range(8):
                ok &= vol.w[q[2] + (k >> 2), q[1] + ((k >> 1) & 1), q[0] + (k & 1)] >= thr
        cell = inside & (flag | (not flags))
        assert (out["cell"] == cell).all() and (out["obs"] == (cell & ok)).all()
        assert (_bits(out["f"]) == _bits(fr)).all()                      # written for every point, NaN and the infinities included
        base = (q[2] * nv[1] + q[1]) * nv[0] + q[0]
        assert (out["base"][cell] == base[cell]).all() and (out["base"][~cell] == 0).all()
        t = [vol.tsdf[q[2] + (k >> 2), q[1] + ((k >> 1) & 1), q[0] + (k & 1)] for k in range(8)]
        phi, grad = tsdf_ref.lerp3_grad(t, fr)
        assert (_bits(phi) == _bits(val)).all()
        assert (_bits(out["val"][cell]) == _bits(val[cell])).all() and (_bits(out["g"][cell]) == _bits(np.stack(grad, 1)[cell])).all()
        assert (out["val"][~cell] == 0).all() and (out["g"][~cell] == 0).all()
        for key, n in (("cells", cell[:n_edge].sum()), ("observed", (cell & ok)[:n_edge].sum()), ("unobserved", (cell & ~ok)[:n_edge].sum()),
                       ("flag", (inside & ~flag)[:n_edge].sum())):
            met[key, flags, box is small] = int(n)
        # the points the list promises, as the restatement sees them
        e = slice(0, n_edge)
        assert (c[0] == box[0]).all() == (box is grid) and (c[1] == grid[1]).all() and (c[2] == small[0]).all() and (c[3] == small[1]).all()
        assert (fr[4] == 0).all() and c[6][0] < 0 and not cell[10:16].any()
        assert inside[7] and cell[7] == (not flags)                      # in the cleared block: only its flag refuses it
        assert c[8][0] == -1 and cell[8]                                 # astride the seam: its own block is the touched one
        for a in range(3):
            assert (c[e][:, a] == box[0][a] - 1).any() and (c[e][:, a] == box[1][a] + 1).any()
    print("sampler host test met:", met)
    assert all(met["cells", fl, sm] >= 4 and met["observed", fl, sm] >= 2 for fl, sm in ((1, False), (0, False), (1, True)))
    assert met["flag", 1, False] >= 2 and met["unobserved", 0, False] >= 1

    # the tracker's rows from the same value and gradient
    keep, J, rr, fr = camtrack_ref.rows(camtrack_ref.grid_from_volume(vol), depth, mask, K, pose, thr, full=True)
    out = got[1][n_edge:]
    print(f"tracker rows: {keep.sum()} of {len(keep)} back-projected points contribute, {out['obs'].sum()} observed")
    assert keep.sum() >= 20 and (out["obs"][keep] == 1).all()
    assert (_bits(out["f"]) == _bits(fr)).all()
    with np.errstate(all="ignore"):
        n = (out["g"] * trunc) / voxel
        assert (_bits(n[keep]) == _bits(J[keep][:, :3])).all() and (_bits((out["val"] * trunc)[keep]) == _bits(rr[keep])).all()
