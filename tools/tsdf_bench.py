"""TSDF physics meshes at the reference's shape: 100 RGB-D frames of 1280 x 720, 2 mm voxels, a table-top scene (a plane
with a sphere on it) ray-cast analytically.  Prints one JSON line and writes it to profiles/tsdf_bench.json:

  integrate_fps            frames per second through d2r_tsdf_integrate (upload, erosion, block marking, integration; the
                           call is synchronous), background object (20 x 20 erosion)
  bytes_bound_ms_per_frame the voxels of the blocks a frame touches x 8 B of state, read and written once each, at 8 TB/s
  fraction_of_bytes_bound  that bound over the measured time per frame
  get_phys_models_s        the whole call for both objects (fusion, extraction, clean-up, files; convexify = a copy)

    python tools/tsdf_bench.py [--frames 100] [--views 12] [--width 1280] [--height 720] [--out profiles/tsdf_bench.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SPHERE_C, SPHERE_R = np.array([0.0, 0.0, 0.04]), 0.04
BOUNDS = np.array([[-0.5, -0.5, -0.05], [0.5, 0.5, 0.35]])
HBM_BYTES_PER_S = 8.0e12


def look_at(eye, target):
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def raycast(T, K, w, h):
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    d = np.stack([(jj - K[0, 2]) / K[0, 0], (ii - K[1, 2]) / K[1, 1], np.ones((h, w))], -1) @ T[:3, :3].T
    o = T[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t_plane = np.where(d[..., 2] < 0, -o[2] / d[..., 2], np.inf)
    oc = o - SPHERE_C
    a, b, c = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    t_sph = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    t = np.minimum(t_plane, t_sph)
    hit = np.isfinite(t) & (t < 3.0)
    return np.where(hit, t, 0.0).astype(np.float16), (hit & (t_sph < t_plane)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--views", type=int, default=12, help="distinct ray-cast views, cycled")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tsdf_bench.json"))
    a = ap.parse_args()

    from dream2real_amd import engine, physics_utils
    K = np.array([[0.72 * a.width, 0, (a.width - 1) / 2], [0, 0.72 * a.width, (a.height - 1) / 2], [0, 0, 1.0]])
    views = []
    for k in range(a.views):
        az, el = 2 * np.pi * k / a.views, np.deg2rad(35.0 if k % 2 == 0 else 55.0)
        T = look_at(np.array([0.0, 0.0, 0.03]) + 0.8 * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)]), np.array([0.0, 0.0, 0.03]))
        views.append((T,) + raycast(T, K, a.width, a.height))
    depths = [views[f % a.views][1] for f in range(a.frames)]
    masks = [views[f % a.views][2] for f in range(a.frames)]
    poses = [views[f % a.views][0] for f in range(a.frames)]
    ctx = engine.Context(0)

    # blocks one frame touches (a fresh volume per view), then the timed loop
    u16 = [(d * 1000).astype(np.uint16) for d in depths[:a.views]]
    bg = [m == 0 for m in masks[:a.views]]
    touched = []
    for k in range(a.views):
        vol = physics_utils.TsdfVolume(ctx, BOUNDS)
        vol.integrate(u16[k], bg[k], K, poses[k], physics_utils.ERODE_BACKGROUND)
        n = physics_utils.C.c_uint32(0)
        ctx.check(ctx.lib.d2r_tsdf_read_voxels(vol.h, physics_utils.C.byref(n), None, None, None))
        touched.append(int(n.value))
        vol.close()
    vol = physics_utils.TsdfVolume(ctx, BOUNDS)
    for k in range(a.views):                                   # warm-up: every shape, code objects loaded
        vol.integrate(u16[k], bg[k], K, poses[k], physics_utils.ERODE_BACKGROUND)
    t0 = time.perf_counter()
    for f in range(a.frames):
        vol.integrate(u16[f % a.views], bg[f % a.views], K, poses[f % a.views], physics_utils.ERODE_BACKGROUND)
    dt = time.perf_counter() - t0
    t1 = time.perf_counter()
    mesh = vol.extract(crop=BOUNDS)
    t_extract = time.perf_counter() - t1
    vol.close()

    out_dir = tempfile.mkdtemp(prefix="tsdf_bench_")
    t2 = time.perf_counter()
    physics_utils.get_phys_models(depths, poses, K, masks, 2, BOUNDS, save_dir=out_dir, use_cache=False, use_phys_tsdf=True, ctx=ctx,
                                  convexify=lambda src, dst, obj_id: shutil.copyfile(src, dst))
    t_all = time.perf_counter() - t2
    shutil.rmtree(out_dir, ignore_errors=True)
    ctx.close()

    voxels = float(np.mean(touched)) * 4096
    bound_ms = voxels * 8 * 2 / HBM_BYTES_PER_S * 1e3
    res = dict(bench="tsdf", frames=a.frames, width=a.width, height=a.height, voxel_m=physics_utils.TSDF_VOXEL,
               bounds=BOUNDS.tolist(), integrate_fps=a.frames / dt, integrate_ms_per_frame=dt / a.frames * 1e3,
               blocks_touched_per_frame=float(np.mean(touched)), voxels_touched_per_frame=voxels,
               bytes_bound_ms_per_frame=bound_ms, fraction_of_bytes_bound=bound_ms / (dt / a.frames * 1e3),
               extract_s=t_extract, mesh_vertices=int(len(mesh["vertices"])), mesh_triangles=int(mesh["keep"].sum()),
               get_phys_models_s=t_all, note="integrate time includes the frame's upload and a stream synchronise per frame")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
