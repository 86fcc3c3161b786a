"""TEST INFRASTRUCTURE ONLY: the CLIP text forward in float64 (the operation of oracle/clip_ref.py::text_embeds: token + position
embedding, pre-LN causal blocks with quick_gelu, final LayerNorm, pooling at argmax of the raw ids, text_projection, L2 norm).

Two options make it the yardstick of the text tower's GPU tests (tests/test_text_tower_gpu.py):

  bf16_operands  every matrix-product operand of the blocks is rounded to bf16 (x and W of each Linear, the stored q / k / v, and P
                 before P V) and everything else stays float64: the text counterpart of oracle/clip_bf16.py, i.e. what a bf16-MFMA
                 tower computes when nothing else loses precision.  Its distance from the plain float64 result is the FLOOR of any
                 such tower on a given (weights, ids) pair.  The projection after the pooled LayerNorm is fp32 in the HIP tower
                 (k_head) and so is not rounded here.
  mask           a boolean [T, T] visibility matrix (mask[query, key]) in place of the causal key <= query: the CPU tests feed wrong
                 masks through it to prove that the GPU bar separates them from a correct tower.

Ids are clipped to [0, vocab - 1] for the embedding lookup and pooled on the raw values, as k_text_embed does.
"""
from __future__ import annotations

import numpy as np

from oracle.clip_bf16 import round_bf16

f64 = np.float64


def _bf16(a):
    """float64 -> nearest bf16 (through fp32), back in float64."""
    return round_bf16(np.asarray(a, f64).astype(np.float32)).astype(f64)


def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(w, f64) + np.asarray(b, f64)


def quick_gelu(x):
    return x / (1.0 + np.exp(-1.702 * x))


def causal_mask(T):
    """mask[query, key] = key <= query."""
    return np.tril(np.ones((T, T), bool))


def _linear(x, sd, name, rnd):
    w = np.asarray(sd[name + ".weight"], f64)
    y = rnd(x) @ rnd(w).T
    if name + ".bias" in sd:
        y = y + np.asarray(sd[name + ".bias"], f64)
    return y


def _attention(x, sd, pre, n_heads, mask, rnd):
    B, T, D = x.shape
    dh = D // n_heads
    q, k, v = (rnd(_linear(x, sd, f"{pre}.{n}_proj", rnd)) for n in "qkv")             # q / k / v are stored in the operand format
    sh = lambda t: t.reshape(B, T, n_heads, dh).transpose(0, 2, 1, 3)
    q, k, v = sh(q), sh(k), sh(v)
    s = (q @ k.transpose(0, 1, 3, 2)) * dh ** -0.5
    s = np.where(mask, s, -np.inf)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    o = (rnd(p) @ v) / p.sum(-1, keepdims=True)                                          # P is the second product's operand; the sum is not rounded
    return _linear(o.transpose(0, 2, 1, 3).reshape(B, T, D), sd, pre + ".out_proj", rnd)


def text_embeds(input_ids, sd, cfg, *, bf16_operands=False, mask=None):
    """input_ids [C, T] integers -> L2-normalised float64 [C, proj]."""
    ids = np.asarray(input_ids)
    Cn, T = ids.shape
    rnd = _bf16 if bf16_operands else (lambda a: a)
    mask = causal_mask(T) if mask is None else np.asarray(mask, bool)
    assert mask.shape == (T, T) and mask.any(-1).all(), "every query needs a visible key"
    tok = sd["text_model.embeddings.token_embedding.weight"]
    look = np.clip(ids, 0, tok.shape[0] - 1)
    x = tok[look].astype(f64) + sd["text_model.embeddings.position_embedding.weight"][None, :T].astype(f64)
    for l in range(cfg["text_layers"]):
        p = f"text_model.encoder.layers.{l}"
        h = layer_norm(x, sd[p + ".layer_norm1.weight"], sd[p + ".layer_norm1.bias"])
        x = x + _attention(h, sd, p + ".self_attn", cfg["text_heads"], mask, rnd)
        h = layer_norm(x, sd[p + ".layer_norm2.weight"], sd[p + ".layer_norm2.bias"])
        x = x + _linear(quick_gelu(_linear(h, sd, p + ".mlp.fc1", rnd)), sd, p + ".mlp.fc2", rnd)
    pooled = x[np.arange(Cn), ids.argmax(-1)]                                            # the raw ids; first maximum
    pooled = layer_norm(pooled, sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"])
    e = pooled @ np.asarray(sd["text_projection.weight"], f64).T
    return e / np.linalg.norm(e, axis=-1, keepdims=True)


def floor_and_want(ids, sd, cfg):
    """(want, floor): the float64 embeddings and the largest per-caption L2 distance of the ideal bf16 tower from them."""
    want = text_embeds(ids, sd, cfg)
    ideal = text_embeds(ids, sd, cfg, bf16_operands=True)
    return want, float(np.linalg.norm(ideal - want, axis=1).max())


# ---- the inputs the CPU bite proof and the GPU sweep share

SWEEP_OVERRIDE = dict(text_hidden=128, text_heads=2, text_mlp=256, proj=64, vocab=512, text_layers=2, ctx=77)
BAR_FACTOR = 3.0          # per caption: |got - want|_2 <= BAR_FACTOR * floor


def sweep_ids(T, vocab, seed=17):
    """[T, T]: caption c carries the largest id (vocab - 1) at position c and random smaller ids elsewhere, so that pooling reads
    every row of the causal attention, one caption per row."""
    r = np.random.Generator(np.random.PCG64(seed + T))
    ids = r.integers(0, vocab - 1, size=(T, T))
    ids[np.arange(T), np.arange(T)] = vocab - 1
    return ids.astype(np.int32)


def eos_ids(positions, T, vocab, seed=23):
    """[len(positions), T]: the largest id at the given position of each caption, random smaller ids elsewhere."""
    r = np.random.Generator(np.random.PCG64(seed + T))
    ids = r.integers(0, vocab - 1, size=(len(positions), T))
    ids[np.arange(len(positions)), np.asarray(positions)] = vocab - 1
    return ids.astype(np.int32)


def wrong_masks(T):
    """name -> [T, T] visibility matrices of a causal attention that is wrong only past the first 32-row tile."""
    q, k = np.arange(T)[:, None], np.arange(T)[None, :]
    ok = k <= q
    return {
        "one future key visible (key <= query + 1)": k <= q + 1,
        "diagonal dropped for queries >= 32": ok & ~((k == q) & (q >= 32)),
        "key 32 hidden from queries > 32": ok & ~((k == 32) & (q > 32)),
        "diagonal tile's mask on earlier tiles": ok & ~((k // 32 < q // 32) & (k % 32 > q % 32)),
    }
