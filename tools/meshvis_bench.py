#!/usr/bin/env python
"""Times one d2r_mesh_render call on one GPU at the shape of a cost-volume picture: 640x360, a synthetic height-field mesh of
about 10^6 triangles a few pixels across (a 2 mm TSDF surface seen from 0.7 m), 1 600 score cubes.  The wall time of a call holds
the argument checks, the upload of the mesh, the kernels and the read-back of the frame.  There is no reference time to compare
with: the reference opens an Open3D window.  Writes profiles/meshvis_bench.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def height_field(n, side, seed=0):
    """an n x n grid of vertices over side x side metres with a smooth bump field -> (verts, tris): 2 (n - 1)^2 triangles"""
    rng = np.random.default_rng(seed)
    x = np.linspace(-side / 2, side / 2, n)
    X, Y = np.meshgrid(x, x, indexing="ij")
    Z = 0.03 * np.sin(X * 9) * np.cos(Y * 7) + 0.002 * rng.standard_normal((n, n))
    verts = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).ravel()
    tris = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)]).astype(np.uint32)
    return verts, tris


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=708, help="vertices per side: 2 (grid - 1)^2 triangles (708 -> 999 698)")
    ap.add_argument("--cubes", type=int, default=1600)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "meshvis_bench.json"))
    a = ap.parse_args()
    from dream2real_amd import _lib, engine
    ctx = engine.Context(0)
    verts, tris = height_field(a.grid, 1.4)
    item = np.zeros(tris.shape[0], np.uint32)
    rng = np.random.default_rng(1)
    side = int(round(a.cubes ** 0.5))
    g = np.stack(np.meshgrid(np.linspace(-0.3, 0.3, side), np.linspace(-0.3, 0.3, side), [0.06], indexing="ij"), -1).reshape(-1, 3)[:a.cubes]
    half = np.full(len(g), 0.3 / (side - 1), np.float32)
    scores = rng.integers(0, 65536, len(g)).astype(np.uint16)
    view = _lib.PcdView(640, 360, 500.0, 500.0, 319.5, 179.5, 1.0, 0.01)
    eye, target = np.array([0.45, -0.4, 0.4]), np.array([0.0, 0.0, 0.0])
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    cam = np.eye(4, dtype=np.float32)
    cam[:3, 0], cam[:3, 1], cam[:3, 2], cam[:3, 3] = x, np.cross(z, x), z, eye
    mats, cols = np.eye(4, dtype=np.float32)[None], np.array([[100, 100, 100]], np.uint8)

    def call():
        return _lib.mesh_render(ctx, view, cam, verts, tris, item, mats, cols, g, half, scores, return_ids=True)
    rgb, ids = call()                                            # the first call allocates the workspaces
    times = []
    for _ in range(a.reps):
        t = time.perf_counter()
        rgb2, ids2 = call()
        times.append(time.perf_counter() - t)
    assert rgb2.tobytes() == rgb.tobytes() and ids2.tobytes() == ids.tobytes()
    res = dict(width=640, height=360, triangles=int(tris.shape[0]), cubes=int(len(g)), reps=a.reps,
               mesh_pixels=int((ids >= 0).sum()), cube_pixels=int(((ids < 0) & (ids != -2 ** 31)).sum()),
               call_ms_min=1e3 * min(times), call_ms_median=1e3 * float(np.median(times)), call_ms_max=1e3 * max(times))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
