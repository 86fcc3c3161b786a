"""The point-cloud ablation (use_vis_pcds) at the shape of configs/shopping/pcd.json: ~8 000 valid candidates of a
70 000-pose grid, 336 x 336 frames, a background cloud of ~500 k points and a movable cloud of ~20 k, ViT-L/14-336 with
random weights.  Prints one JSON line: valid candidates/s of the fused call (d2r_pcd_render_score_host) and the
render / CLIP split.  The render half is bounded from above by the same fused call on the 2-layer `vit_tiny` tower
(render + preprocess + a negligible tower); the CLIP half is the ViT-L/14-336 call minus that.

    python tools/pcd_bench.py [--candidates 8000] [--bg-points 500000] [--movable-points 20000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=8000)
    ap.add_argument("--bg-points", type=int, default=500_000)
    ap.add_argument("--movable-points", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import torch
    from dream2real_amd import engine
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    from dream2real_amd.pcd_visual_model import PointCloud, PointCloudRenderer
    from synthetic_scenes import look_at_opencv
    import types

    r = np.random.default_rng(0)
    centre = np.array([0.5, 0.0, 0.035])
    nt = a.bg_points * 4 // 5                            # a table plane plus clutter
    table = np.concatenate([r.uniform([0.1, -0.5], [0.9, 0.5], (nt, 2)), np.zeros((nt, 1))], 1)
    clutter = r.uniform([0.2, -0.4, 0.0], [0.8, 0.4, 0.25], (a.bg_points - nt, 3))
    bg = PointCloud(np.concatenate([table, clutter]), r.integers(0, 256, (a.bg_points, 3), dtype=np.uint8))
    d = r.normal(size=(a.movable_points, 3))
    mv = PointCloud(centre + 0.04 * d / np.linalg.norm(d, axis=1, keepdims=True),
                    r.integers(0, 256, (a.movable_points, 3), dtype=np.uint8))
    O = np.eye(4, dtype=np.float32)
    O[:3, 3] = centre
    task = types.SimpleNamespace(task_bground_obj=types.SimpleNamespace(vis_model=bg),
                                 movable_obj=types.SimpleNamespace(vis_model=mv, pose=torch.from_numpy(O)))
    poses = np.tile(np.eye(4, dtype=np.float32), (a.candidates, 1, 1))
    poses[:, :3, 3] = centre + r.uniform([-0.3, -0.4, 0.0], [0.3, 0.4, 0.02], (a.candidates, 3))
    cam = look_at_opencv([0.5, -0.75, 0.55], centre).astype(np.float32)

    ctx = engine.Context(0)
    rend = PointCloudRenderer(ctx)
    res = {"candidates": a.candidates, "bg_points": a.bg_points, "movable_points": a.movable_points, "frame": [336, 336]}
    for name in ("vit_tiny", "vit_l14_336"):
        cfg = CLIP_CONFIGS[name]
        sc = engine.ClipScorer(ctx, cfg, random_clip_state_dict(cfg, seed=6, text=False))
        text = np.eye(2, cfg["proj"], dtype=np.float32)
        rend.render_score(cam, poses[:64], task, sc, text)          # warm-up: uploads, workspaces, kernels
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            rend.render_score(cam, poses, task, sc, text)
            ts.append(time.perf_counter() - t0)
        res[f"{name}_s"] = float(np.median(ts))
        sc.close()
    res["cand_per_s"] = a.candidates / res["vit_l14_336_s"]
    res["render_share_upper_bound"] = res["vit_tiny_s"] / res["vit_l14_336_s"]
    rend.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
