"""TEST INFRASTRUCTURE ONLY: the CLIP vision forward in float64 (the operation of oracle/clip_ref.py::vision_embeds: patch embedding as a
matrix product, class + position embeddings, pre-LayerNorm, pre-LN blocks with quick_gelu, post-LayerNorm of token 0, visual_projection,
L2 norm), the yardstick of tests/test_vision_tower_gpu.py as tests/text_ref.py is the text tower's.

  bf16_operands  rounds where dream2real_amd/csrc/clip.hip rounds and keeps everything else float64.  Its distance from the plain
                 float64 result is the FLOOR of the tower on a given (weights, pixels) pair.  The rounding points, by kernel:
                   k_patchify / k_convert_bf16   the patches and the patch weight;
                   ln_fold 0 (k_layernorm)       LayerNorm(x) and W of q / k / v and fc1; the q rows of W carry 2^-3 log2(e) BEFORE
                                                 their rounding (ATTN_Q_SCALE, d2r_clip_create), the scores are in the exp2 domain;
                   ln_fold 1-4 (k_fold_ln_weight, EPI_LN_*)  the A operand is the RAW residual row rounded to bf16, the weight is
                                                 bf16(W o gamma [x the q scale]), and the epilogue applies
                                                 rstd (acc - mean cs) + (b + W beta), cs = the column sums of the ROUNDED weight;
                                                 mean and rstd are those of the residual BEFORE it is stored (EPI_RESID_STATS_*);
                   GEMM epilogues                the stored q, k, v, the attention output and gelu(fc1) (operands of the next product);
                   attn_qtile / k_attention_s    P before P V (the row sum is of the unrounded P); k_attention_cls keeps P in fp32;
                   last_block_cls (cls_last)     the last block runs on token 0 alone: fp32 residual from the stored one, k_layernorm
                                                 and the UNFOLDED fc1 whatever ln_fold says.
                 post-LayerNorm, the projection and the normalisation are fp32 in k_head and are not rounded.
  residual       how the ln_fold modes store the residual stream between blocks: "exact" (ln_fold 0 and 3, fp32), "hi_lo" (1 and 4:
                 bf16 hi + a bf16 / one-byte lo, 16 significant bits), "bf16" (2).  Only read with bf16_operands.
  ln_fold        False models ln_fold 0 (operands LayerNorm(x), W), True the folded modes.  Only read with bf16_operands.
  cls_last       the last block as last_block_cls runs it (see above).  Only read with bf16_operands: in float64 it is the same function.
  attn           a hook `attn(layer) -> (mult, src)` for the mutants of wrong_attention(): `mult` [T, T] multiplies P[query, key]
                 (0 hides a key, m counts it m times), `src` [T] makes query row i receive the attention output of row src[i];
                 either may be None.
"""
from __future__ import annotations

import numpy as np

from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
from tests import text_ref
from tests.text_ref import _bf16, f64, layer_norm, quick_gelu

BAR_FACTOR = text_ref.BAR_FACTOR          # per image: |got - want|_2 <= BAR_FACTOR * floor
Q_SCALE = float(np.float32(0.125) * np.float32(1.4426950408889634))       # ATTN_Q_SCALE: head_dim^-0.5 * log2(e), head_dim 64
RESIDUALS = ("exact", "hi_lo", "bf16")


def _sig16(a):
    """float64 -> fp32 rounded to 16 significant bits (the hi + lo-byte residual of EPI_RESID_STATS_SPLIT8), back in float64."""
    u = np.ascontiguousarray(np.asarray(a, f64).astype(np.float32)).view(np.uint32)
    return ((u + (((u >> 8) & 1) + 0x7F)) & 0xFFFFFF00).view(np.float32).astype(f64)


def _same(a):
    return a


def _w(sd, name):
    return np.asarray(sd[name], f64)


class _Rounding:
    """The rounding points of one forward: `op` rounds a matrix-product operand, `store` the residual stream between blocks."""

    def __init__(self, bf16_operands, residual, ln_fold):
        assert residual in RESIDUALS, residual
        self.on = bool(bf16_operands)
        self.op = _bf16 if self.on else _same
        self.fold = self.on and ln_fold
        self.store = {"exact": _same, "hi_lo": _sig16, "bf16": _bf16}[residual] if self.fold else _same


def _ln_linear(x, sd, ln, lin, R, scale=1.0, fold=None):
    """Linear(LayerNorm(x)) * scale, with the operand roundings of the unfolded (k_layernorm + GEMM) or folded (EPI_LN_*) path."""
    g, b = _w(sd, ln + ".weight"), _w(sd, ln + ".bias")
    W, bias = _w(sd, lin + ".weight"), _w(sd, lin + ".bias")
    if not (R.fold if fold is None else fold):
        return R.op(layer_norm(x, g, b)) @ R.op(W * scale).T + bias * scale
    mu = x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt((x * x).mean(-1, keepdims=True) - mu * mu + 1e-5)
    Wf = R.op(W * g * scale)                                                  # k_fold_ln_weight
    return rstd * (R.op(x) @ Wf.T) - rstd * mu * Wf.sum(1) + (bias + W @ b) * scale


def _attention(x, sd, p, n_heads, R, hook, cls_only):
    """The attention output [B, T or 1, D] of the block's input x (the residual as the kernels see it), before out_proj."""
    B, T, D = x.shape
    dh = D // n_heads
    ln, pre = p + ".layer_norm1", p + ".self_attn."
    scale = Q_SCALE if R.on else dh ** -0.5 * np.log2(np.e)                                   # the fp32 constant is a rounding too
    q = R.op(_ln_linear(x[:, :1] if cls_only else x, sd, ln, pre + "q_proj", R, scale))       # exp2 domain
    k = R.op(_ln_linear(x, sd, ln, pre + "k_proj", R))
    v = R.op(_ln_linear(x, sd, ln, pre + "v_proj", R))
    sh = lambda t: t.reshape(B, t.shape[1], n_heads, dh).transpose(0, 2, 1, 3)
    q, k, v = sh(q), sh(k), sh(v)
    s = q @ k.transpose(0, 1, 3, 2)
    mult, src = hook if hook is not None else (None, None)
    if mult is not None:
        mult = np.asarray(mult, f64)[:s.shape[2]]
        assert (mult > 0).any(-1).all(), "every query needs a visible key"
        s = np.where(mult > 0, s, -np.inf)
    pr = np.exp2(s - s.max(-1, keepdims=True))
    if mult is not None:
        pr = pr * mult
    o = ((pr if cls_only else R.op(pr)) @ v) / pr.sum(-1, keepdims=True)      # k_attention_cls: fp32 P; the sum is never rounded
    if src is not None:
        o = o[:, :, np.asarray(src)[:o.shape[2]]]
    return R.op(o.transpose(0, 2, 1, 3).reshape(B, -1, D))


def vision_embeds(pixel_values, sd, cfg, *, bf16_operands=False, residual="exact", ln_fold=True, cls_last=False, attn=None, hidden_out=None):
    """pixel_values [B, 3, S, S] -> L2-normalised float64 [B, proj]; hidden_out (a list) receives the residual entering each block."""
    R = _Rounding(bf16_operands, residual, ln_fold)
    P, d, L, H = cfg["patch_size"], cfg["hidden_size"], cfg["num_layers"], cfg["num_heads"]
    pv = np.asarray(pixel_values, f64)
    B, _, S, _ = pv.shape
    g = S // P
    patches = pv.reshape(B, 3, g, P, g, P).transpose(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * P * P)
    w = _w(sd, "vision_model.embeddings.patch_embedding.weight").reshape(d, 3 * P * P)
    x = R.op(patches) @ R.op(w).T
    cls = np.broadcast_to(_w(sd, "vision_model.embeddings.class_embedding"), (B, 1, d))
    x = np.concatenate([cls, x], 1) + _w(sd, "vision_model.embeddings.position_embedding.weight")[None]
    x = layer_norm(x, sd["vision_model.pre_layrnorm.weight"], sd["vision_model.pre_layrnorm.bias"])
    # x: the residual as computed (LayerNorm statistics and the bf16 operand copy come from it); xs: as stored and re-read
    xs = R.store(x)
    for l in range(L):
        p = f"vision_model.encoder.layers.{l}"
        lin = lambda a, name: a @ R.op(_w(sd, f"{p}.{name}.weight")).T + _w(sd, f"{p}.{name}.bias")
        hook = attn(l) if attn is not None else None
        if hidden_out is not None:
            hidden_out.append(xs)
        if R.on and cls_last and l == L - 1:
            x0 = xs[:, :1] + lin(_attention(x, sd, p, H, R, hook, True), "self_attn.out_proj")
            h = R.op(quick_gelu(_ln_linear(x0, sd, p + ".layer_norm2", p + ".mlp.fc1", R, fold=False)))
            x = xs = x0 + lin(h, "mlp.fc2")
            break
        x = xs + lin(_attention(x, sd, p, H, R, hook, False), "self_attn.out_proj")
        xs = R.store(x)
        x = xs + lin(R.op(quick_gelu(_ln_linear(x, sd, p + ".layer_norm2", p + ".mlp.fc1", R))), "mlp.fc2")
        xs = R.store(x)
    pooled = layer_norm(xs[:, 0], sd["vision_model.post_layernorm.weight"], sd["vision_model.post_layernorm.bias"])
    e = pooled @ _w(sd, "visual_projection.weight").T
    return e / np.linalg.norm(e, axis=-1, keepdims=True)


def floor_and_want(pv, sd, cfg, residual="exact", *, ln_fold=True, cls_last=False):
    """(want, floor): the float64 embeddings and the largest per-image L2 distance of the bf16-operand forward from them."""
    want = vision_embeds(pv, sd, cfg)
    ideal = vision_embeds(pv, sd, cfg, bf16_operands=True, residual=residual, ln_fold=ln_fold, cls_last=cls_last)
    return want, float(np.linalg.norm(ideal - want, axis=1).max())


# ---- the mutants: ways the streamed kernels can be wrong past the first tile or at a tail

def wrong_attention(T, n_layers=2, cls_last=True):
    """name -> attn hook.  The first four act in every layer that runs the full attention (all of them, or all but the last under
    cls_last); the last one in the last block only (k_attention_cls).  Mutants that do not apply at this T are left out."""
    n_qt = (T + 31) // 32
    T_pad, last0 = 32 * n_qt, 32 * (n_qt - 1)
    full = range(n_layers - 1 if cls_last else n_layers)
    q, k = np.arange(T)[:, None], np.arange(T)[None, :]
    ones = np.ones((T, T))

    def in_full(mult=None, src=None):
        return lambda l: (mult, src) if l in full else None

    out = {}
    if T_pad > T:
        out["pad_keys_visible"] = in_full(mult=np.where(k == T - 1, 1.0 + T_pad - T, ones))
    if n_qt >= 2:
        out["last_key_tile_hidden_from_last_query_tile"] = in_full(mult=np.where((k >= last0) & (q >= last0), 0.0, ones))
        src = np.arange(T)
        src[last0:] -= 32
        out["last_query_tile_off_by_one_tile"] = in_full(src=src)
    if T > 33:
        out["key_32_hidden_from_queries_past_32"] = in_full(mult=np.where((k == 32) & (q > 32), 0.0, ones))
    if cls_last and T >= 2:
        out["cls_misses_last_key"] = lambda l: (np.where((k == T - 1) & (q == 0), 0.0, ones), None) if l == n_layers - 1 else None
    return out


# ---- the inputs the CPU bite proof and the GPU sweep share

SWEEP_SIZES = (16, 32, 64, 96, 128, 144, 176, 208, 224, 240, 256, 272, 384)      # T = 2, 5, 17, 37, 65, 82, 122, 170, 197, 226, 257, 290, 577
SWEEP_N = 7


def n_tokens(image_size, patch=16):
    return (image_size // patch) ** 2 + 1


def sweep_cfg(image_size):
    """The two-layer tiny geometry (hidden 128, 2 heads, MLP 256, patch 16) at another image size."""
    return dict(CLIP_CONFIGS["vit_tiny"], image_size=image_size)


def sweep_weights(image_size):
    cfg = sweep_cfg(image_size)
    return cfg, random_clip_state_dict(cfg, seed=6, text=False)


def marked_roles(T):
    """(a, [b ...]) per image, cycling: the class token of the last block is drawn to token a, and token a in block 0 to the tokens b
    (two of them share its attention).  a and b sit where the mutants of wrong_attention() act: the last row, the first row of the
    last 32-row tile, key 32, the last key."""
    last0 = 32 * ((T + 31) // 32 - 1)
    first = last0 if 0 < last0 < T - 1 else 1
    return [(T - 1, [32 if T > 34 else 1]),
            (T - 1, [first if first != T - 1 else T - 2]),
            (first, [T - 1, 2 if first != 2 else 3])]


def sweep_pixels(image_size, n=SWEEP_N, sd=None, cfg=None):
    """[n, 3, S, S] fp32: standard-normal images, each with marked patches (marked_roles) whose pixels are solved for through the
    patch embedding (a linear map onto the token's embedding), so that single rows and keys of the attention carry weight in the
    class token's output.  With Gaussian weights and pixels alone every attention row is nearly flat and an error in one row or key
    past the first tile reaches token 0 divided by about T."""
    r = np.random.Generator(np.random.PCG64(1000 + image_size))
    pv = r.standard_normal((n, 3, image_size, image_size), dtype=np.float32)
    if cfg is None:
        cfg, sd = sweep_weights(image_size)
    P, d, L = cfg["patch_size"], cfg["hidden_size"], cfg["num_layers"]
    T, g = n_tokens(image_size, P), image_size // P
    if T < 5:
        return pv
    hs = []
    vision_embeds(pv, sd, cfg, hidden_out=hs)
    pos = _w(sd, "vision_model.embeddings.position_embedding.weight")
    pre = "vision_model.pre_layrnorm"
    wp_inv = np.linalg.pinv(_w(sd, "vision_model.embeddings.patch_embedding.weight").reshape(d, 3 * P * P))

    def toward(x_query, layer):
        """The residual direction whose keys in `layer` score highest against the query rows x_query [.., d]."""
        p = f"vision_model.encoder.layers.{layer}"
        h = layer_norm(x_query, sd[p + ".layer_norm1.weight"], sd[p + ".layer_norm1.bias"])
        q = h @ _w(sd, p + ".self_attn.q_proj.weight").T + _w(sd, p + ".self_attn.q_proj.bias")
        return (q @ _w(sd, p + ".self_attn.k_proj.weight")) / _w(sd, p + ".layer_norm1.weight")

    def embed(direction):
        """A patch embedding (rms 1 per channel, so that the position embedding hardly matters) whose pre-LayerNorm row points along it."""
        e = (direction - _w(sd, pre + ".bias")) / _w(sd, pre + ".weight")
        e = e - e.mean()
        return e * np.sqrt(d) / np.linalg.norm(e)

    def put(img, token, e):
        py, px = divmod(token - 1, g)
        pv[img, :, py * P:(py + 1) * P, px * P:(px + 1) * P] = (wp_inv @ e).reshape(3, P, P).astype(np.float32)

    roles = marked_roles(T)
    for i in range(n):
        a, bs = roles[i % len(roles)]
        ra = toward(hs[L - 1][i, 0], L - 1)
        ra *= np.sqrt(d) / np.linalg.norm(ra)
        e_a = embed(ra)
        put(i, a, e_a)
        x_a = layer_norm(e_a + pos[a], sd[pre + ".weight"], sd[pre + ".bias"])
        rb = toward(x_a, 0)
        rb *= np.sqrt(d) / np.linalg.norm(rb)
        side = r.standard_normal(d)
        side -= (side @ rb) / (rb @ rb) * rb
        side *= np.sqrt(d) / np.linalg.norm(side)
        for j, b in enumerate(bs):
            put(i, b, embed(rb + (0.0 if len(bs) == 1 else (1.0, -1.0)[j]) * side))
    return pv
