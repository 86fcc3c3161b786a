"""CPU tests of tests/vision_ref.py, the float64 yardstick of the vision tower's GPU tests (tests/test_vision_tower_gpu.py): it agrees with
the fp32 oracle and the committed Hugging Face goldens, and on the GPU sweep's own inputs every mutant of the streamed attention (a tail
or a tile past the first handled wrongly) lands beyond the GPU bar (BAR_FACTOR x the ideal-bf16 floor), with a margin of two."""
import os

import numpy as np
import pytest

from dream2real_amd.clip_model import CLIP_CONFIGS, adversarial_clip_state_dict, random_clip_state_dict
from oracle import clip_ref
from tests import vision_ref

# (mutant, T) pairs the tower-level test cannot see, with the reason.  Everything else must clear 2 x BAR_FACTOR.
# Where the last 32-row tile holds ONE token, "the last key tile hidden from the last query tile" hides key T - 1 from query T - 1 alone,
# i.e. one self-attention weight; the marked inputs draw row T - 1 to OTHER keys (their purpose for every other mutant), so that
# weight is ~1 / T and the change stays below the floor (measured: 0.0 ... 0.2 x floor).  The same code path (the last key tile's mask
# in the last query tile) is seen at every T whose last tile holds two or more tokens.
UNSEEN = {("last_key_tile_hidden_from_last_query_tile", T): "one-token last tile: a single self-attention weight" for T in (65, 257, 577)}


def _pv(n, cfg, seed=77):
    r = np.random.Generator(np.random.PCG64(seed))
    return r.standard_normal((n, 3, cfg["image_size"], cfg["image_size"]), dtype=np.float32)


@pytest.mark.parametrize("name,tol", [("vit_tiny", 2e-6), ("vit_b16", 2e-5), ("vit_tiny_adversarial", 2e-5)])
def test_float64_reference_agrees_with_the_fp32_oracle_and_the_hf_goldens(goldens, name, tol):
    """To fp32 noise: the bounds are those tests/test_oracle_goldens.py holds the fp32 oracle to against Hugging Face on the same
    pixels (two fp32 evaluations of one function differ by at most what each differs from the exact result)."""
    if name == "vit_tiny_adversarial":
        cfg = CLIP_CONFIGS["vit_tiny"]
        sd, pv = adversarial_clip_state_dict(cfg, 6), _pv(4, cfg)
        hf = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hf_clip_r05.npz"))["g5adv_vit_tiny_image_embeds"]
    else:
        cfg = CLIP_CONFIGS[name]
        sd = random_clip_state_dict(cfg, seed=6)
        pv = goldens["g5_vit_tiny_pv"] if name == "vit_tiny" else _pv(2, cfg)
        hf = goldens[f"g5_{name}_image_embeds"]
    got = vision_ref.vision_embeds(pv, sd, cfg)
    assert got.dtype == np.float64 and got.shape == hf.shape
    e_oracle = np.abs(got - clip_ref.vision_embeds(pv, sd, cfg)).max()
    e_hf = np.abs(got - hf).max()
    print(f"[vision_ref] {name}: max |f64 - fp32 oracle| = {e_oracle:.2e}, max |f64 - HF golden| = {e_hf:.2e} (bound {tol:.0e})")
    assert e_oracle <= tol and e_hf <= tol
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, rtol=0, atol=1e-12)


def test_options_that_round_nothing_change_nothing_and_the_identity_hook_is_exact():
    cfg, sd = vision_ref.sweep_weights(96)
    pv = vision_ref.sweep_pixels(96, 3)
    want = vision_ref.vision_embeds(pv, sd, cfg)
    T = vision_ref.n_tokens(96)
    ident = lambda l: (np.ones((T, T)), np.arange(T))
    for kw in (dict(residual="bf16"), dict(ln_fold=False), dict(cls_last=True), dict(attn=ident)):
        assert np.array_equal(vision_ref.vision_embeds(pv, sd, cfg, **kw), want), kw
    # every rounding model is a different function, and a small perturbation of the exact one
    seen = [want]
    for residual, fold, cl in (("exact", False, False), ("exact", True, False), ("hi_lo", True, False), ("bf16", True, False), ("hi_lo", True, True)):
        got = vision_ref.vision_embeds(pv, sd, cfg, bf16_operands=True, residual=residual, ln_fold=fold, cls_last=cl)
        dist = np.linalg.norm(got - want, axis=1)
        assert (0 < dist).all() and (dist < 0.1).all(), (residual, fold, cl, dist)
        assert not any(np.array_equal(got, s) for s in seen)
        seen.append(got)


@pytest.mark.parametrize("image_size", vision_ref.SWEEP_SIZES)
def test_attention_mutants_land_beyond_twice_the_gpu_bar(image_size):
    """The bite proof on the inputs of the GPU sweep: floor = the ideal bf16 tower's largest per-image L2 distance from float64 (the
    product's default rounding model: folded LayerNorm, hi + lo residual); every mutant that applies at this T, run in float64 in the
    layers the full attention runs in (cls_last 1: all but the last; cls_last 0: all), must push at least one image beyond
    BAR_FACTOR x floor, and its worst image beyond 2 x BAR_FACTOR x floor.  Prints the multiples; asserts the condition only."""
    T = vision_ref.n_tokens(image_size)
    cfg, sd = vision_ref.sweep_weights(image_size)
    pv = vision_ref.sweep_pixels(image_size, sd=sd, cfg=cfg)
    want = vision_ref.vision_embeds(pv, sd, cfg)
    for cls_last in (True, False):
        ideal = vision_ref.vision_embeds(pv, sd, cfg, bf16_operands=True, residual="hi_lo", cls_last=cls_last)
        floor = float(np.linalg.norm(ideal - want, axis=1).max())
        assert 0 < floor < 0.1               # bf16 operands move a unit vector, but by far less than its length
        mutants = vision_ref.wrong_attention(T, cfg["num_layers"], cls_last)
        assert "pad_keys_visible" in mutants and (T <= 33 or len(mutants) == 4 + cls_last)
        for name, hook in mutants.items():
            dist = np.linalg.norm(vision_ref.vision_embeds(pv, sd, cfg, attn=hook) - want, axis=1)
            over, mult = int((dist > vision_ref.BAR_FACTOR * floor).sum()), float(dist.max() / floor)
            unseen = (name, T) in UNSEEN
            print(f"[vision_ref] T {T} cls_last {int(cls_last)} floor {floor:.3e} {name}: {mult:.1f} x floor, {over} of {len(pv)} images over the bar"
                  + (f"  (not seen: {UNSEEN[(name, T)]})" if unseen else ""))
            if unseen:
                assert mult < vision_ref.BAR_FACTOR, "seen after all: take the pair out of UNSEEN"
                continue
            assert over >= 1, (name, T)
            assert mult > 2 * vision_ref.BAR_FACTOR, (name, T, mult)
