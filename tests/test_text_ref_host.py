"""CPU tests of tests/text_ref.py, the float64 yardstick of the text tower's GPU tests (tests/test_text_tower_gpu.py): it agrees with
the fp32 oracle and the committed Hugging Face goldens, and on the GPU sweep's own inputs every wrong causal mask that acts only past
the first 32-row attention tile lands beyond the GPU bar (BAR_FACTOR x the ideal-bf16 floor), so a tower with such a mask cannot pass."""
import numpy as np
import pytest

from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
from oracle import clip_ref
from tests import text_ref


@pytest.mark.parametrize("name,tol", [("vit_tiny", 2e-6), ("vit_b16", 2e-5)])
def test_float64_reference_agrees_with_the_fp32_oracle_and_the_hf_goldens(goldens, name, tol):
    """To fp32 noise: the bounds are those tests/test_oracle_goldens.py holds the fp32 oracle to against Hugging Face on the same
    inputs (two fp32 evaluations of one function differ by at most what each differs from the exact result)."""
    cfg = CLIP_CONFIGS[name]
    sd = random_clip_state_dict(cfg, seed=6)
    ids = goldens[f"g5_{name}_ids"]
    got = text_ref.text_embeds(ids, sd, cfg)
    assert got.dtype == np.float64
    e_oracle = np.abs(got - clip_ref.text_embeds(ids, sd, cfg)).max()
    e_hf = np.abs(got - goldens[f"g5_{name}_text_embeds"]).max()
    print(f"[text_ref] {name}: max |f64 - fp32 oracle| = {e_oracle:.2e}, max |f64 - HF golden| = {e_hf:.2e} (bound {tol:.0e})")
    assert e_oracle <= tol and e_hf <= tol
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, rtol=0, atol=1e-12)


def test_explicit_causal_mask_and_id_clipping():
    cfg = dict(CLIP_CONFIGS["vit_tiny"], **text_ref.SWEEP_OVERRIDE)
    sd = random_clip_state_dict(cfg, seed=6)
    V = cfg["vocab"]
    ids = text_ref.eos_ids([20, 5, 36, 39], 40, V)
    want = text_ref.text_embeds(ids, sd, cfg)
    assert np.array_equal(text_ref.text_embeds(ids, sd, cfg, mask=text_ref.causal_mask(40)), want)
    # embedded as the clipped id, pooled on the raw value: the first of two maxima; an id past the vocabulary is the maximum
    raw, same = ids.copy(), ids.copy()
    raw[0, 3], same[0, 3] = -7, 0        # before the end token at 20, so the pooled row sees it
    raw[1, 9] = V - 1                    # a second end token after the one at 5: pooled at 5, which does not see position 9
    raw[2, 36] = V + 40                  # the only maximum: pooled at 36 and embedded as V - 1, which `same` holds there
    got = text_ref.text_embeds(raw, sd, cfg)
    np.testing.assert_allclose(got, text_ref.text_embeds(same, sd, cfg), rtol=0, atol=1e-13)
    assert np.abs(got[0] - want[0]).max() > 1e-3                   # the replaced token is seen
    # the fp32 oracle on the equivalent ids it accepts says the same
    assert np.abs(got - clip_ref.text_embeds(same, sd, cfg)).max() <= 2e-6


def test_wrong_masks_past_the_first_tile_land_beyond_the_gpu_bar():
    """The bite proof on the inputs of the GPU sweep at T = Cn = 77: floor = the ideal bf16 tower's largest per-caption L2 distance
    from float64; each wrong mask (run in float64) must push at least one caption beyond BAR_FACTOR x floor, the bar the GPU tests
    hold the HIP tower to.  Prints the multiple of the floor and the number of captions over the bar per mask."""
    T = 77
    cfg = dict(CLIP_CONFIGS["vit_tiny"], **text_ref.SWEEP_OVERRIDE)
    sd = random_clip_state_dict(cfg, seed=6)
    ids = text_ref.sweep_ids(T, cfg["vocab"])
    assert (ids.argmax(1) == np.arange(T)).all()
    want, floor = text_ref.floor_and_want(ids, sd, cfg)
    bar = text_ref.BAR_FACTOR * floor
    print(f"[text_ref] sweep inputs T = Cn = {T}: ideal-bf16 floor {floor:.3e}, GPU bar {bar:.3e}")
    assert 0 < floor < 0.1               # bf16 operands move a unit vector, but by far less than its length
    smallest = np.inf
    for name, m in text_ref.wrong_masks(T).items():
        assert not np.array_equal(m, text_ref.causal_mask(T))
        dist = np.linalg.norm(text_ref.text_embeds(ids, sd, cfg, mask=m) - want, axis=1)
        over = int((dist > bar).sum())
        print(f"[text_ref]   {name}: max {dist.max():.3e} = {dist.max() / floor:.1f} x floor, {over} of {T} captions over the bar")
        assert over >= 1, name
        smallest = min(smallest, dist.max() / floor)
    print(f"[text_ref] smallest wrong-mask multiple {smallest:.1f} x floor vs the bar's {text_ref.BAR_FACTOR:g}")
    assert smallest > text_ref.BAR_FACTOR
