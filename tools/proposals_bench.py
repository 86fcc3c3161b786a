#!/usr/bin/env python
"""Times d2r_proposals_labels on one GPU: M synthetic discs and rectangles of 1280x720, the sizes a mask
generator returns for a table-top frame.  Prints the call's wall time and d2r_proposals_get_timing (upload, kernels, download, device
events) of the best of --repeat warm calls, and writes profiles/proposals_bench.json.  No comparison with anything else is made."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def proposals(m, w, h, seed=0):
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    P = np.zeros((m, h, w), np.uint8)
    for k in range(m):
        ci, cj = int(rng.integers(40, h - 40)), int(rng.integers(40, w - 40))
        if k % 2:
            r = int(rng.integers(15, 120))
            P[k] = (ii - ci) ** 2 + (jj - cj) ** 2 < r * r
        else:
            a, b = int(rng.integers(10, 150)), int(rng.integers(10, 150))
            P[k, max(0, ci - a):ci + a, max(0, cj - b):cj + b] = 1
    inside = np.zeros((h, w), np.uint8)
    inside[h // 10:h - h // 10, w // 10:w - w // 10] = 1
    return P, inside


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", type=int, default=128)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "proposals_bench.json"))
    a = ap.parse_args()
    from dream2real_amd import _lib, engine
    ctx = engine.Context(0)
    P, inside = proposals(a.masks, a.width, a.height)
    wall, stages = [], []
    for _ in range(a.repeat + 1):                            # the first round grows the workspaces
        t0 = time.perf_counter()
        labels, recs = _lib.proposals_labels(ctx, P, inside, records=True)
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append(_lib.proposals_timing(ctx))
    best = min(range(1, len(wall)), key=lambda k: stages[k][1])
    res = dict(masks=a.masks, width=a.width, height=a.height, survivors=int(labels.max()),
               dropped_by_stage={str(s): int((recs[:, 2] == s).sum()) for s in range(5)}, wall_ms=wall[best], upload_ms=stages[best][0],
               kernels_ms=stages[best][1], download_ms=stages[best][2])
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
