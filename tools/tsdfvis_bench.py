"""The colour-TSDF visual backend (vis_backend="tsdf") at the shape of configs/shopping/pcd.json: ~8 000 valid
candidates of a 70 000-pose grid, 336 x 336 frames, a movable object of 0.15 m and a background over table-top bounds, both
fused on the GPU from synthetic RGB-D frames into 2 mm colour volumes, ViT-L/14-336 with random weights.  Prints one JSON line:
    upload / background cast / candidates' casts / copies to the host, by device events (d2r_tsdfvis_get_timing): of the fused
        call (whose frames stay on the device: no copy), and of the parity hook d2r_tsdfvis_render on --hook-candidates frames;
    valid candidates/s of the fused call (d2r_tsdfvis_render_score_host) and the render / CLIP split: the render half is bounded
        from above by the same fused call on the 2-layer `vit_tiny` tower (render + preprocess + a negligible tower), as in
        tools/pcd_bench.py; the casts alone are the device-event figure;
    the same call's point-cloud figure: tools/pcd_bench.py run in a process of its own right after, in the same session
        (--no-pcd leaves it out), beside the recorded state profiles/pcd_bench_shopping.json.

    python tools/tsdfvis_bench.py [--candidates 8000] [--frames 8] [--reps 3] [--out profiles/tsdfvis_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CENTRE = np.array([0.5, 0.0, 0.075])                     # the movable object: a sphere of 0.15 m standing on the table
RADIUS = 0.075
BG_BOUNDS = [[0.1, -0.5, -0.05], [0.9, 0.5, 0.30]]      # table-top bounds
FW, FH = 640, 480                                        # the synthetic sensor
FK = np.array([[600.0, 0.0, 319.5], [0.0, 600.0, 239.5], [0.0, 0.0, 1.0]])


def frame(T):
    """The scene from the OpenCV camera-to-world pose T -> (depth float32 [H,W] metres, labels uint8 [H,W]: 1 the sphere, 0 the
    table, 255 nothing; rgb uint8 [H,W,3])."""
    jj, ii = np.meshgrid(np.arange(FW), np.arange(FH))
    d = np.stack([(jj - FK[0, 2]) / FK[0, 0], (ii - FK[1, 2]) / FK[1, 1], np.ones((FH, FW))], -1) @ T[:3, :3].T
    o = T[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        tp = np.where(d[..., 2] < 0, -o[2] / d[..., 2], np.inf)                 # the table plane z = 0
    oc = o - CENTRE
    a, b, c = (d * d).sum(-1), (d * oc).sum(-1), oc @ oc - RADIUS ** 2
    disc = b * b - a * c
    ts = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
    ts = np.where(ts > 0, ts, np.inf)
    t = np.minimum(tp, ts)
    label = np.where(np.isfinite(t), (ts < tp).astype(np.uint8), 255).astype(np.uint8)
    depth = np.where(np.isfinite(t) & (t < 2.9), t, 0.0)
    p = o + d * depth[..., None]
    check = ((np.floor(p[..., 0] * 25) + np.floor(p[..., 1] * 25)) % 2).astype(np.uint8)
    rgb = np.stack([60 + 120 * check + 60 * (label == 1), 200 - 100 * check, 40 + (np.clip(p[..., 2], 0, 0.2) * 1000).astype(np.uint8)], -1)
    return depth.astype(np.float32), label, rgb.astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=8000)
    ap.add_argument("--frames", type=int, default=8, help="synthetic RGB-D frames on a ring around the table")
    ap.add_argument("--hook-candidates", type=int, default=512, help="frames the parity hook copies to the host for the download figure")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-pcd", action="store_true", help="do not run tools/pcd_bench.py afterwards")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import torch
    from dream2real_amd import engine
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    from dream2real_amd.physics_utils import ERODE_BACKGROUND, ERODE_OBJECT
    from dream2real_amd.tsdf_visual_model import TsdfRenderer, get_vis_tsdfs
    from synthetic_scenes import look_at_opencv

    r = np.random.default_rng(0)
    ring = [look_at_opencv(CENTRE + 0.8 * np.array([np.cos(az) * 0.7, np.sin(az) * 0.7, 0.7]), CENTRE) for az in 2 * np.pi * np.arange(a.frames) / a.frames + 0.3]
    shots = [frame(T) for T in ring]
    depths, labels, rgbs = (np.stack([s[k] for s in shots]) for k in range(3))
    mv_bounds = [list(CENTRE - RADIUS - 0.01), list(CENTRE + RADIUS + 0.01)]

    ctx = engine.Context(0)
    t0 = time.perf_counter()
    bg = get_vis_tsdfs(rgbs, depths, ring, FK, labels != 0, BG_BOUNDS, ctx=ctx, erode_k=ERODE_BACKGROUND)
    mv = get_vis_tsdfs(rgbs, depths, ring, FK, labels != 1, mv_bounds, ctx=ctx, erode_k=ERODE_OBJECT)
    fuse_s = time.perf_counter() - t0
    O = np.eye(4, dtype=np.float32)
    O[:3, 3] = CENTRE
    task = types.SimpleNamespace(task_bground_obj=types.SimpleNamespace(vis_model=bg),
                                 movable_obj=types.SimpleNamespace(vis_model=mv, pose=torch.from_numpy(O)))
    poses = np.tile(np.eye(4, dtype=np.float32), (a.candidates, 1, 1))
    poses[:, :3, 3] = CENTRE + r.uniform([-0.3, -0.4, 0.0], [0.3, 0.4, 0.02], (a.candidates, 3))
    cam = look_at_opencv([0.5, -0.75, 0.55], CENTRE).astype(np.float32)

    rend = TsdfRenderer(ctx)
    res = {"candidates": a.candidates, "frame": [336, 336], "fused_frames": a.frames, "fuse_s": fuse_s,
           "bg_voxels": [int(v) for v in bg.grid()[1]], "movable_voxels": [int(v) for v in mv.grid()[1]], "voxel": float(bg.grid()[2])}
    names = ("upload_ms", "background_cast_ms", "candidate_casts_ms", "download_ms")
    for name in ("vit_tiny", "vit_l14_336"):
        cfg = CLIP_CONFIGS[name]
        sc = engine.ClipScorer(ctx, cfg, random_clip_state_dict(cfg, seed=6, text=False))
        text = np.eye(2, cfg["proj"], dtype=np.float32)
        rend.render_score(cam, poses[:64], task, sc, text)          # warm-up: workspaces, kernels
        ts, ev = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            rend.render_score(cam, poses, task, sc, text)
            ts.append(time.perf_counter() - t0)
            ev.append(rend.timing())
        res[f"{name}_s"] = float(np.median(ts))
        res[f"{name}_events"] = dict(zip(names, (float(x) for x in np.median(np.array(ev), axis=0))))
        sc.close()
    frames = rend.render(cam, poses[:a.hook_candidates], task)       # the parity hook: frames to the host
    res["hook"] = dict(zip(names, rend.timing()), candidates=a.hook_candidates)
    hit = np.stack(frames[:16]).any(axis=3)
    res["pixels_hit_share"] = float(hit.mean())                       # a picture, not an empty frame
    ev = res["vit_l14_336_events"]
    res["cand_per_s"] = a.candidates / res["vit_l14_336_s"]
    res["render_share_upper_bound"] = res["vit_tiny_s"] / res["vit_l14_336_s"]                       # render + preprocess (+ a 2-layer tower)
    res["cast_share_of_fused_call"] = (ev["background_cast_ms"] + ev["candidate_casts_ms"]) / 1000.0 / res["vit_l14_336_s"]
    bg.close()
    mv.close()
    ctx.close()

    recorded = os.path.join(REPO, "profiles", "pcd_bench_shopping.json")
    if os.path.exists(recorded):
        with open(recorded) as f:
            res["pcd_recorded"] = json.loads(f.readline())
    if not a.no_pcd:          # the yardstick, same machine, same session, a process of its own
        p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "pcd_bench.py"), "--candidates", str(a.candidates), "--reps", str(a.reps)],
                           capture_output=True, text=True, cwd=REPO)
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0 or not lines:
            sys.exit(f"tools/pcd_bench.py failed ({p.returncode}): {p.stderr[-2000:]}")
        res["pcd_same_session"] = json.loads(lines[-1])
        res["render_upper_bound_vs_pcd"] = res["vit_tiny_s"] / res["pcd_same_session"]["vit_tiny_s"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
