"""Times the camera-pose refinement: one 1280 x 720 frame at stride 1 and 2 against a scene-sized volume ->
device-event milliseconds per linearisation and per refine call, beside the bytes the rule must read (3 bytes a selected pixel, 64
bytes of corners per contributing pixel before cache reuse).  Writes profiles/camtrack_bench.json.
    python tools/camtrack_bench.py [--reps 5]"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from dream2real_amd import cam_pose_opt, engine                      # noqa: E402
from dream2real_amd.physics_utils import TsdfVolume                  # noqa: E402
from tests import camtrack_cases as cases                            # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
ctx = engine.Context(0)
K = cases.INTRINSICS.copy()
K[:2] *= 4
K[0, 2], K[1, 2] = 639.5, 359.5
T = cases.poses()
depth = np.stack([cases.raycast(t, 1280, 720, K) for t in T])
mask = np.ones((720, 1280), np.uint8)
bounds = np.array([[-0.5, -0.5, -0.03], [0.5, 0.5, 0.47]])            # a table-top scene: 1 m x 1 m x 0.5 m
vol = TsdfVolume(ctx, bounds)
for k in range(cases.N_FUSED):
    vol.integrate(depth[k], mask, K, T[k].astype(np.float32), 1)
start = cases.tracking_start("a")[0]
out = {"frame": [1280, 720], "volume_voxels": [int(v) for v in vol.grid()[1]], "reps": reps, "strides": {}}
for stride in (1, 2):
    rows = []
    for _ in range(reps + 1):
        pose, rep = cam_pose_opt.refine_cam_pose(vol, depth[cases.TRACKED], mask, K, start, ctx=ctx, stride=stride)
        up, kern, down = cam_pose_opt.camtrack_timing(ctx)
        rows.append((up, kern, down, rep["iters"], rep["pixels_last"], rep["status"]))
    rows = rows[1:]                                                  # the first call sizes the workspaces
    kern, iters = np.median([r[1] for r in rows]), rows[0][3]
    selected = ((1280 + stride - 1) // stride) * ((720 + stride - 1) // stride)
    out["strides"][str(stride)] = dict(status=rows[0][5], iterations=iters, contributing_pixels=rows[0][4], selected_pixels=selected,
                                       upload_ms=float(np.median([r[0] for r in rows])), kernels_ms_per_refine=float(kern),
                                       kernels_ms_per_linearisation=float(kern / iters), downloads_ms_per_refine=float(np.median([r[2] for r in rows])),
                                       bytes_per_linearisation=int(3 * selected + 64 * rows[0][4]))
vol.close()
ctx.close()
path = os.path.join(REPO, "profiles", "camtrack_bench.json")
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out))
