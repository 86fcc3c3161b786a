"""Times the geometric label tracker: 20 frames of 1280 x 720 over a 1 m x 1 m x 0.5 m table top at the
defaults -> device-event milliseconds of upload, kernels and download (d2r_labeltrack_get_timing), median of --reps calls after one
that sizes the workspaces.  The kernels' time is split by three runs of the same frames: all 20 at grow 64 (everything), all 20 at grow
0 (no fill launches), frame 0 alone (one vote and the two copies of the first label image); fill = the first minus the second,
vote = the third, predict and finish = what is left of the second, per frame.  Beside the vote: the bytes the rule must move per
frame (every voxel's 2-byte state read once, the frame's depth and labels read once; the voxels of the band are written on top and
are not counted) and the share of the 8 TB/s HBM peak that is.  Writes profiles/labeltrack_bench.json.
    python tools/labeltrack_bench.py [--reps 5]"""
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
N, W, H = 20, 1280, 720
K = lc.cases.INTRINSICS.copy()
K[:2] *= 4
K[0, 2], K[1, 2] = 639.5, 359.5
T = np.stack(tsdf_scene.cameras(24)[:N])
shots = [lc.raycast(t, W, H, K) for t in T]
d16, labels0 = np.stack([s[0] for s in shots]), shots[0][1]
bounds = np.array([[-0.5, -0.5, -0.03], [0.5, 0.5, 0.47]])            # a table-top scene: 1 m x 1 m x 0.5 m
dims, lo = segmentation.labeltrack_grid(bounds)
ctx = engine.Context(0)


def timed(n, grow):
    rows = []
    for _ in range(reps + 1):
        out, stats = segmentation.track_labels(d16[:n], T[:n], K, labels0, bounds, ctx=ctx, grow=grow, return_stats=True)
        rows.append(segmentation.labeltrack_timing(ctx))
    return np.median(np.array(rows[1:]), axis=0), out, stats          # the first call sizes the workspaces


full, out, stats = timed(N, 64)
nofill, _, _ = timed(N, 0)
first, _, _ = timed(1, 0)
ctx.close()
n_vox = int(dims.astype(np.int64).prod())
vote_bytes = 2 * n_vox + 3 * W * H
vote_ms = float(first[1])
res = {"frames": N, "frame": [W, H], "grid": [int(v) for v in dims], "grid_lo": [int(v) for v in lo], "voxels": n_vox, "reps": reps,
       "params": dict(voxel=0.004, band_voxels=2, tau_mm=10, grow=64),
       "call_ms": dict(upload=float(full[0]), kernels=float(full[1]), download=float(full[2])),
       "per_frame_ms": dict(upload=float(full[0] / N), predict_and_finish=float((nofill[1] - N * vote_ms) / (N - 1)),
                            fill=float((full[1] - nofill[1]) / (N - 1)), vote=vote_ms, download=float(full[2] / N)),
       "vote_bytes_per_frame": vote_bytes, "vote_bytes_per_s": vote_bytes / (vote_ms * 1e-3) if vote_ms > 0 else None,
       "vote_share_of_hbm_peak": vote_bytes / (vote_ms * 1e-3) / HBM_PEAK if vote_ms > 0 else None,
       "fill_launches_that_changed_a_pixel": [int(v) for v in stats[:, 3]],
       "pixels_left_unknown": [int(v) for v in stats[:, 2]], "labels_seen": [int(v) for v in np.unique(out)]}
path = os.path.join(REPO, "profiles", "labeltrack_bench.json")
json.dump(res, open(path, "w"), indent=1)
print(json.dumps(res))
