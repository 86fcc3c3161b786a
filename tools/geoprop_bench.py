"""Times the geometric proposer: one 1280 x 720 frame of the slab with a box and two spheres over a 1 m x 1 m x
0.5 m table top at the defaults -> device-event milliseconds of upload, the three kernel stages and download
(d2r_geoprop_get_timing), median of --reps calls after one that sizes the workspaces.  The second and the third stage each hold one
small copy to the host and the host's part of the rule (the plane choice, the selection), so they are more than their kernels.
Beside them: the bytes the height stage must move (the depth read, the bins written) and the share of the 8 TB/s HBM peak that is.
Nothing in the parent does this work: no ratio is stated.  Writes profiles/geoprop_bench.json.
    python tools/geoprop_bench.py [--reps 5]"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from dream2real_amd import engine, segmentation                     # noqa: E402
from tests import labeltrack_cases as lc                             # noqa: E402
from tests import tsdf_scene                                         # noqa: E402

HBM_PEAK = 8.0e12
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
W, H = 1280, 720
K = lc.cases.INTRINSICS.copy()
K[:2] *= 4
K[0, 2], K[1, 2] = 639.5, 359.5
T = tsdf_scene.cameras(24)[0]
d16, truth = lc.raycast(T, W, H, K)
bounds = np.array([[-0.5, -0.5, -0.03], [0.5, 0.5, 0.47]])            # a table-top scene: 1 m x 1 m x 0.5 m
ctx = engine.Context(0)
rows = []
for _ in range(reps + 1):
    masks, recs, plane = segmentation.propose_masks(d16, T, K, bounds, ctx=ctx)
    rows.append(segmentation.geoprop_timing(ctx))
ctx.close()
ms = np.median(np.array(rows[1:]), axis=0)                            # the first call sizes the workspaces
ious = [max([float((m & (truth == obj)).sum() / (m | (truth == obj)).sum()) for m in masks] or [0.0]) for obj in (lc.BOX, lc.SPHERE_A, lc.SPHERE_B)]
height_bytes = 6 * W * H
res = {"frame": [W, H], "reps": reps, "params": dict(window_mm=5, h_min_mm=6, tau_mm=10, min_area=200, max_props=255),
       "call_ms": dict(upload=float(ms[0]), heights_and_histogram=float(ms[1]), plane_links_labelling_statistics=float(ms[2]),
                       selection_and_label_image=float(ms[3]), download=float(ms[4]), total=float(ms.sum())),
       "all_calls_ms": [[float(x) for x in r] for r in rows[1:]],
       "height_stage_bytes": height_bytes, "height_stage_bytes_per_s": height_bytes / (ms[1] * 1e-3) if ms[1] > 0 else None,
       "height_stage_share_of_hbm_peak": height_bytes / (ms[1] * 1e-3) / HBM_PEAK if ms[1] > 0 else None,
       "plane": {k: int(plane[k]) for k in plane.dtype.names}, "proposals": len(masks), "areas": [int(a) for a in recs["area"]],
       "best_iou_box_sphere_a_sphere_b": ious}
path = os.path.join(REPO, "profiles", "geoprop_bench.json")
json.dump(res, open(path, "w"), indent=1)
print(json.dumps(res))
