"""tools/validate_artifacts.py --search-forks, the part that needs no GPU: the enumeration of the fork combinations, the ranking
(share of pixels off by more than one LSB, ties by mean PSNR, then by enumeration order) and the restoration of every touched
option — with a fake renderer and a fake option store."""
import importlib.util
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("validate_artifacts", os.path.join(REPO, "tools", "validate_artifacts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class FakeOptions:
    def __init__(self, **kv):
        self.kv = dict(kv)
        self.sets = []

    def get_option(self, key):
        return self.kv[key]

    def set_option(self, key, value):
        self.sets.append((key, value))
        self.kv[key] = value


def _reference(seed=0, n=3, h=8, w=10):
    return np.random.Generator(np.random.PCG64(seed)).integers(8, 248, (n, h, w, 3)).astype(np.uint8)


def test_enumeration_is_two_plus_two_arithmetics_times_the_lens(tool):
    combos = tool.fork_combinations()
    assert len(combos) == 8 and len({tuple(sorted(c.items(), key=str)) for c in combos}) == 8
    arith = {(c["render_arith"], c["mlp_f16"]) for c in combos}
    assert arith == {(0, 0), (0, 1), (1, None), (2, None)}           # mlp_f16 only with render_arith 0: the half arithmetic is fp16
    for a in arith:
        assert {c["lens"] for c in combos if (c["render_arith"], c["mlp_f16"]) == a} == {0, 1}


def test_ranking_by_share_then_psnr_then_order(tool):
    ref = _reference()

    def render(c):
        f = ref.astype(np.int32)
        if c["lens"] == 0:
            f[:, :4] += 3                                   # 4 of the 8 rows: half of the pixels off by 3
        elif c["render_arith"] == 2:
            pass                                            # exact
        elif c["render_arith"] == 1:
            f[:, 0, 0] += 1                                 # nothing off by more than 1, PSNR below the exact one
        elif c["mlp_f16"] == 1:
            f[:, 0, :2] += 1                                # nothing off by more than 1 either, PSNR lower still
        else:
            f[:, 0, 0] += 2                                 # one pixel per frame off by 2
        return f.astype(np.uint8)

    res = tool.rank_forks(render, ref)
    t = res["table"]
    assert len(t) == 8 and res["closest"] == dict(render_arith=2, mlp_f16=None, lens=1) and len(res["tied"]) == 1
    assert [(r["render_arith"], r["mlp_f16"]) for r in t[:4]] == [(2, None), (1, None), (0, 1), (0, 0)] and all(r["lens"] == 1 for r in t[:4])
    assert t[0]["share_off_by_more_than_1"] == t[1]["share_off_by_more_than_1"] == t[2]["share_off_by_more_than_1"] == 0.0
    assert t[0]["psnr_db_min"] == 99.0 and t[0]["psnr_db_mean"] > t[1]["psnr_db_mean"] > t[2]["psnr_db_mean"]
    assert t[3]["share_off_by_more_than_1"] == pytest.approx(1 / 80) and t[3]["max_abs_diff"] == 2
    # the four lens-off rows are indistinguishable: they keep the order of enumeration
    assert all(r["lens"] == 0 and r["share_off_by_more_than_1"] == pytest.approx(0.5) for r in t[4:])
    assert [r["order"] for r in t[4:]] == sorted(r["order"] for r in t[4:])
    assert "closest: render_arith 2, mlp_f16 -, lens on" in tool.format_fork_table(res)


def test_ties_are_reported(tool):
    ref = _reference(1)
    res = tool.rank_forks(lambda c: ref if c["lens"] else 255 - ref, ref)
    assert res["closest"] == dict(render_arith=0, mlp_f16=0, lens=1)                 # first in the order of enumeration
    assert len(res["tied"]) == 4 and all(c["lens"] == 1 for c in res["tied"])
    assert "(4 combinations tied)" in tool.format_fork_table(res)


def test_a_frame_of_another_size_is_an_error(tool):
    ref = _reference(2)
    with pytest.raises(ValueError, match="--resolution"):
        tool.rank_forks(lambda c: ref[:, :4], ref)


def test_options_are_restored_also_after_an_exception(tool):
    ref = _reference(3)
    opts = FakeOptions(render_arith=0, mlp_f16=1, chunk=4096)
    lens = {"on": True}

    def render(c):
        opts.set_option("render_arith", c["render_arith"])
        if c["mlp_f16"] is not None:
            opts.set_option("mlp_f16", c["mlp_f16"])
        lens["on"] = bool(c["lens"])
        return ref

    restore = lambda: lens.update(on=True)
    res = tool.search_forks(opts, ("render_arith", "mlp_f16"), render, ref, restore=(restore,))
    assert len(res["table"]) == 8 and opts.kv == dict(render_arith=0, mlp_f16=1, chunk=4096) and lens["on"] is True
    assert ("render_arith", 2) in opts.sets and ("mlp_f16", 0) in opts.sets

    def failing(c):
        render(c)
        if c["render_arith"] == 1 and not c["lens"]:
            raise RuntimeError("the march failed")
        return ref

    with pytest.raises(RuntimeError, match="the march failed"):
        tool.search_forks(opts, ("render_arith", "mlp_f16"), failing, ref, restore=(restore,))
    assert opts.kv == dict(render_arith=0, mlp_f16=1, chunk=4096) and lens["on"] is True
