#!/usr/bin/env python
"""Times the device route of captioner="clip"  on one GPU: 20 frames of 1280x720 with 8 objects, multi view,
ViT-B/16 with random weights, the default vocabulary under the nine templates.  Prints d2r_caption_get_timing (upload, preprocess,
tower, scoring, download, device events) of the best of --repeat warm d2r_caption_names calls and their wall time, and in the same
session the route a user had before: the thumbnails downloaded by the fill, one Pillow resize and crop per thumbnail on the host,
ClipScorer.embed_pixels, and the sums in numpy.  Writes profiles/caption_bench.json."""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def scene(n, w, h, objs, seed=0):
    """objs discs that drift from frame to frame over a noisy table"""
    rng = np.random.default_rng(seed)
    rgbs = rng.integers(0, 255, (n, h, w, 3), dtype=np.uint8)
    masks = np.zeros((n, h, w), np.uint8)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    for o in range(1, objs + 1):
        ci, cj, r = h * (0.25 + 0.5 * (o % 2)), w * (o - 0.5) / objs, 30 + 6 * o
        for f in range(n):
            masks[f][(ii - ci - 2 * f) ** 2 + (jj - cj - 3 * f) ** 2 < r * r] = o
    return rgbs, masks, np.zeros((n, h, w), np.uint8)


def word_tokenizer(vocab, ctx_len):
    def tok(captions):
        rows = [[vocab - 2] + [2 + zlib.crc32(x.encode()) % (vocab - 4) for x in c.split()][:ctx_len - 2] + [vocab - 1] for c in captions]
        T = max(len(r) for r in rows)
        return np.array([r + [vocab - 1] * (T - len(r)) for r in rows], np.int32)
    return tok


def pillow_pixel_values(img, S):
    from PIL import Image
    h, w, _ = img.shape
    short, long_ = min(h, w), max(h, w)
    nl = int(S * long_ / short)
    nh, nw = (nl, S) if w <= h else (S, nl)
    big = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BICUBIC))
    top, left = (nh - S) // 2, (nw - S) // 2
    f = (big[top:top + S, left:left + S].astype(np.float64) * (1.0 / 255.0)).astype(np.float32)
    mean = np.array([0.48145466, 0.4578275, 0.40821073], np.float32)
    std = np.array([0.26862954, 0.26130258, 0.27577711], np.float32)
    return np.ascontiguousarray(((f - mean) / std).transpose(2, 0, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "caption_bench.json"))
    a = ap.parse_args()
    from dream2real_amd import _lib, caption, engine
    from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
    cfg = CLIP_CONFIGS["vit_b16"]
    sd = random_clip_state_dict(cfg, seed=6)
    ctx = engine.Context(0)
    scorer, text = engine.ClipScorer(ctx, cfg, sd), engine.TextEncoder(ctx, cfg, sd)
    t0 = time.perf_counter()
    cap = caption.ClipCaptioner(ctx, scorer, text, word_tokenizer(cfg["vocab"], cfg["ctx"]))
    vocab_ms = (time.perf_counter() - t0) * 1e3
    rgbs, masks, oob = scene(a.frames, a.width, a.height, a.objects)
    num_objs = a.objects + 1
    noise = np.random.default_rng(0).integers(0, 256, rgbs[0].shape, np.uint8)
    recs, total = _lib.thumbs_plan(ctx, rgbs, masks, oob, num_objs, True, True, 0)
    packed = _lib.thumbs_fill(ctx, noise, total)
    acc = [r for r in recs if r[2] & _lib.THUMB_ACCEPTED]
    wall, stages = [], []
    for _ in range(a.repeat + 1):                            # the first round grows the workspaces
        t0 = time.perf_counter()
        idx, sc = _lib.caption_names(ctx, scorer, cap.class_embeds, a.objects, cap.k)
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append(_lib.caption_timing(ctx))
    best = min(range(1, len(wall)), key=lambda k: wall[k])
    # the route before: host thumbnails -> Pillow -> embed_pixels -> numpy
    host = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        thumbs = [packed[(int(r[8]) | int(r[9]) << 32):][:int(r[6]) * int(r[7]) * 3].reshape(int(r[6]), int(r[7]), 3) for r in acc]
        pv = np.stack([pillow_pixel_values(t, cfg["image_size"]) for t in thumbs])
        t1 = time.perf_counter()
        emb = scorer.embed_pixels(pv)
        t2 = time.perf_counter()
        cos = emb @ cap.class_embeds.T
        s = np.stack([cos[[int(r[0]) == o for r in acc]].sum(axis=0) for o in range(1, num_objs)])
        host_idx = np.argsort(-s, axis=1, kind="stable")[:, :cap.k]
        host.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3))
    hb = min(host, key=sum)
    res = dict(frames=a.frames, objects=a.objects, width=a.width, height=a.height, thumbnails=len(acc), packed_bytes=int(total),
               vocabulary=len(cap.names), templates=len(cap.templates), model="vit_b16", class_embeddings_once_ms=vocab_ms,
               wall_ms=wall[best], upload_ms=stages[best][0], preprocess_ms=stages[best][1], tower_ms=stages[best][2],
               scoring_ms=stages[best][3], download_ms=stages[best][4],
               host_route=dict(pillow_ms=hb[0], embed_pixels_ms=hb[1], numpy_scoring_ms=hb[2], total_ms=sum(hb)),
               same_first_names=bool(np.array_equal(idx[:, 0], host_idx[:, 0])))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
