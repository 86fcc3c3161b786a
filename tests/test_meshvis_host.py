"""The mesh-picture rule (tests/meshvis_ref.py) on the cases of tests/meshvis_cases.py, without a GPU: every
case reaches what it claims — so that no GPU comparison can pass on an empty picture — and can tell the rule from its near misses;
the .obj reader; the cost-volume cubes against the reference's formula restated in torch; the engine's default."""
import inspect

import numpy as np
import pytest

from dream2real_amd import _lib, geometry_utils
from tests import meshvis_cases as mc
from tests import meshvis_ref as ref

INT32_MIN = -2 ** 31


def _ids(name):
    return mc.rule(name)[1]


def test_fill_rule_case_reaches_edges_and_shared_edges_are_covered_once():
    rgb, ids, det = mc.rule("A")
    on_edge, cover = det["on_edge"], det["cover"]
    assert (on_edge >= 1).sum() >= 40 and (on_edge >= 2).sum() >= 10
    assert cover.max() == 1                                      # no two triangles of this case overlap
    inner = [(8, 8)] + [(8 + s * d, 8) for d in (1, 2, 3) for s in (1, -1)] + [(8, 8 + s * d) for d in (1, 2, 3) for s in (1, -1)]
    inner += [(8 + sx * d, 8 + sy * d) for d in (1, 2) for sx in (1, -1) for sy in (1, -1)] + [(u, u - 14) for u in range(17, 28)]
    assert len(inner) >= 10
    for u, v in inner:                                           # centres on an edge two triangles share, inside their union
        assert on_edge[v, u] >= 2 and cover[v, u] == 1, (u, v)
    assert on_edge[8, 8] == 8
    assert not det["mesh"]["keep"][mc.case("A")["what"]["zero_area"]]
    # the quad's top and left edges own their centres, its bottom and right edges do not
    assert (ids[2, 16:28] >= 8).all() and (ids[2:14, 16] >= 8).all() and (ids[14, 16:29] == INT32_MIN).all() and (ids[2:14, 28] == INT32_MIN).all()
    # the half-way points of rint snapped to even: 16.5 -> 16, 49.5 -> 50
    S = det["mesh"]
    assert sorted(set(S["X"][12].tolist())) == [16, 50] and sorted(set(S["Y"][12].tolist())) == [16, 50]
    assert set(np.unique(ids[ids >= 0]).tolist()) == set(range(10)) | {11, 12}


def test_clipping_case_reaches_both_launches_and_every_drop():
    rgb, ids, det = mc.rule("B")
    what, S = mc.case("B")["what"], det["mesh"]
    shown = set(np.unique(ids[ids >= 0]).tolist())
    for name in ("quad0", "quad1", "whole", "below_limit", "z_above_near", "small"):
        assert what[name] in shown and S["keep"][what[name]], name
    for name in ("at_limit", "z_eq_near", "nan", "inf", "z_inf", "off_frame", "behind"):
        assert what[name] not in shown and not S["keep"][what[name]], name
    bx0, by0, bx1, by1 = S["box"]
    px = ((bx1 - bx0 + 1) * (by1 - by0 + 1))[S["keep"]]
    assert (px > ref.LARGE_PX).any() and (px <= ref.LARGE_PX).any()          # the workgroup launch and the thread launch
    assert px.max() == 97 * 61 and (ids != INT32_MIN).all()
    assert S["X"][what["below_limit"]].max() == 16 * 131072            # u = 2^17 - 1/64 snaps to 2^21


def test_depth_case_has_ties_a_crossing_and_one_ulp():
    rgb, ids, det = mc.rule("C")
    what = mc.case("C")["what"]
    for lo, hi in (("co_a0", "co_a1"), ("co_b0", "co_b1")):
        alone = [ref.render(**{**mc.args(mc.case("C")), "tris": mc.case("C")["tris"][[what[n]]], "tri_item": np.zeros(1, np.uint32)})[1] >= 0
                 for n in (lo, hi)]
        both = alone[0] & alone[1]
        assert both.sum() >= 20 and (ids[both] == what[lo]).all()             # exact ties go to the lower index
    assert (ids == what["cross0"]).sum() >= 50 and (ids == what["cross1"]).sum() >= 50
    assert (ids == what["ulp_near"]).sum() >= 50 and (ids == what["ulp_far"]).sum() == 0


def test_items_case_shows_three_items_and_every_facing():
    rgb, ids, det = mc.rule("D")
    c = mc.case("D")
    assert c["tris"].shape[0] == 3000 and not (np.asarray(c["item_mats"])[:, :3, :3] == 0).any()
    shown = np.unique(ids[ids >= 0])
    assert set(c["tri_item"][shown].tolist()) == {0, 1, 2} and (ids >= 0).sum() >= 300
    shade = det["shade"][shown]
    assert shade.min() <= 105 and shade.max() >= 250 and len(np.unique(shade)) >= 50      # 0.35 .. 1.0: bytes 89 .. 255
    assert det["shade"].min() >= 89


def test_cube_case_has_front_behind_cut_ties_and_the_score_ends():
    rgb, ids, det = mc.rule("E")
    no_mesh = _ids("E_nt0")
    n = lambda a, k: int((a == -1 - k).sum())
    assert n(ids, 0) >= 50 and n(ids, 0) == n(no_mesh, 0)                      # in front of the wall
    assert n(ids, 1) == 0 and n(no_mesh, 1) >= 50                              # behind it
    assert 0 < n(ids, 2) < n(no_mesh, 2)                                       # cut by it
    c = mc.case("E")
    one = lambda k: ref.render(**{**mc.args(mc.case("E_nt0")), "cube_centres": c["cube_centres"][[k]], "cube_half": c["cube_half"][[k]],
                                  "cube_scores": c["cube_scores"][[k]]})[1] == -1
    both = one(3) & one(4)
    assert both.sum() >= 10 and (ids[both] == -4).all() and n(ids, 4) > 0      # equal scores: the lower index shows
    assert n(ids, 5) == 0 and n(ids, 6) > 0 and n(ids, 7) > 0                  # scores 0, 1, 65535
    assert (rgb[ids == -8] == (253, 231, 37)).all()
    np.testing.assert_array_equal(mc.rule("E_k0")[0][ids >= 0], rgb[ids >= 0])
    assert (_ids("E_k0") >= 0).sum() >= 50 and (_ids("E_k0") < 0).sum() == (_ids("E_k0") == INT32_MIN).sum()
    rgb0, ids0, _ = mc.rule("E_empty")
    assert (ids0 == INT32_MIN).all() and (rgb0 == (250, 250, 250)).all()


def test_size_cases_pass_sixteen_bits_and_fill_their_frames():
    ids = _ids("F_many")
    assert mc.case("F_many")["tris"].shape[0] == 70000 and (ids > 65535).sum() >= 100 and (ids >= 0).mean() > 0.5
    for name in ("F_wide", "F_small"):
        ids = _ids(name)
        assert (ids >= 0).sum() >= 50 and ((ids < 0) & (ids != INT32_MIN)).sum() >= 20, name
    assert _ids("F_wide").shape == (3, 4100) and (_ids("F_wide")[:, 4000:] != INT32_MIN).any()


@pytest.mark.parametrize("wrong,name,least", [("ge_all_edges", "A", 10), ("ties_high", "C", 20), ("keep_z_eq_near", "B", 1), ("linear_z", "C", 20)])
def test_near_misses_of_the_rule_change_pixels(wrong, name, least):
    assert wrong in ref.WRONG_RULES
    assert (mc.rule(name, wrong)[1] != mc.rule(name)[1]).sum() >= least


def test_viridis5_hits_its_stops():
    np.testing.assert_array_equal(ref.viridis5([0, 65535]), [[68, 1, 84], [253, 231, 37]])
    mid = ref.viridis5(np.arange(0, 65536, 257))
    assert (np.abs(np.diff(mid, axis=0)) <= 3).all()                  # (253 - 94) * 4 * 257 / 65535 = 2.5 a step at the steepest


# ------------------------------------------------------------------------------------------------ .obj reader

def test_obj_read_round_trips_obj_write(tmp_path):
    r = np.random.default_rng(5)
    v = (r.standard_normal((200, 3)) * 3).astype(np.float32)
    t = r.integers(0, 200, (350, 3)).astype(np.uint32)
    path = str(tmp_path / "m.obj")
    _lib.obj_write(path, v, t)
    v2, t2 = _lib.obj_read(path)
    assert v2.dtype == np.float32 and t2.dtype == np.uint32
    np.testing.assert_array_equal(t2, t)
    np.testing.assert_array_equal(v2, np.array([[np.float32(float("%f" % x)) for x in row] for row in v], np.float32))
    _lib.obj_write(path, v2, t2)                               # what the writer wrote reads back exactly, and again
    v3, t3 = _lib.obj_read(path)
    np.testing.assert_array_equal(v3, v2)
    np.testing.assert_array_equal(t3, t2)


def test_obj_read_fans_negative_indices_slashes_and_groups(tmp_path):
    path = tmp_path / "g.obj"
    path.write_text("# two parts\no part0\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvt 0.5 0.5\nf 1 2 3 4\n"
                    "g part1\nv 0 0 1\nv 1 0 1\r\nv 0.5 1e0 1\nf -3 -2 -1\nf 5/1/1 6/2/1 7//1\nf 1/1 2/1 3/1 4/1 5/1\n")
    v, t = _lib.obj_read(str(path))
    assert v.shape == (7, 3) and v[6].tolist() == [0.5, 1.0, 1.0]
    np.testing.assert_array_equal(t, [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 5, 6], [0, 1, 2], [0, 2, 3], [0, 3, 4]])
    for text, word in (("v 0 0\nf 1 1 1\n", "line 1"), ("v 0 0 0\nf 1 2 1\n", "line 2"), ("v 0 0 0\nf 1 -2 1\n", "out of range"),
                       ("v 0 0 0\nf 1 1\n", "three corners"), ("v 0 0 0\nf 0 1 1\n", "out of range")):
        path.write_text(text)
        with pytest.raises(_lib.D2RError, match=word):
            _lib.obj_read(str(path))
    with pytest.raises(_lib.D2RError, match="missing.obj"):
        _lib.obj_read(str(tmp_path / "missing.obj"))
    path.write_text("# nothing\n")
    v, t = _lib.obj_read(str(path))
    assert v.shape == (0, 3) and t.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ cost-volume cubes

def _reference_formula(pose_scores, sample_res, pose_batch):
    """reference vision_3d/geometry_utils.py:139-167 restated in torch (fp64), with the two departures of cost_volume_cubes"""
    import torch
    s = torch.as_tensor(pose_scores).clone().double()
    nz = torch.nonzero(s, as_tuple=True)
    s[nz] = 10 ** (s[nz] * 10)
    lo = torch.min(s[nz])
    s[nz] = (s[nz] - lo) / (torch.max(s[nz]) - lo) if torch.max(s[nz]) > lo else torch.ones_like(s[nz])
    P, R = sample_res[0] * sample_res[1] * sample_res[2], sample_res[3] * sample_res[4] * sample_res[5]
    pos_scores, best = torch.max(s.view(P, R), dim=1)
    pos = torch.as_tensor(pose_batch).double().view(P, R, 4, 4)[torch.arange(P), best][:, :3, 3]
    gaps = [((pos[:, a].max() - pos[:, a].min()) / (sample_res[a] - 1)).item() for a in range(3) if sample_res[a] > 1]
    return pos.numpy(), min(gaps), pos_scores.numpy()


@pytest.mark.parametrize("res", [(4, 3, 1, 1, 1, 1), (3, 2, 2, 2, 1, 1)])
def test_cost_volume_cubes_agree_with_the_reference_formula(res):
    r = np.random.default_rng(sum(res))
    N = int(np.prod(res))
    P, R = res[0] * res[1] * res[2], res[3] * res[4] * res[5]
    grid = np.stack(np.meshgrid(np.linspace(-0.2, 0.1, res[0]), np.linspace(0.0, 0.3, res[1]), np.linspace(0.05, 0.11, res[2]), indexing="ij"), -1)
    batch = np.tile(np.eye(4, dtype=np.float32), (P, R, 1, 1))
    batch[:, :, :3, 3] = grid.reshape(P, 1, 3) + r.uniform(-1e-3, 1e-3, (P, R, 3))
    scores = r.uniform(0.15, 0.35, N).astype(np.float32)
    scores[r.permutation(N)[:N // 3]] = 0                      # invalid poses scattered in
    scores.reshape(P, R)[1] = 0                                # and one position with no valid pose at all
    centres, half, s16 = geometry_utils.cost_volume_cubes(scores, res, batch.reshape(N, 16))
    pos, width, want = _reference_formula(scores, list(res), batch.reshape(N, 4, 4))
    assert centres.dtype == np.float32 and half.dtype == np.float32 and s16.dtype == np.uint16 and centres.shape == (P, 3)
    np.testing.assert_array_equal(centres, pos.astype(np.float32))
    np.testing.assert_array_equal(half, np.full(P, np.float32(0.5 * width)))
    # 10 ** x is not correctly rounded in either library: an ulp of the score moves 65535 s by 1e-11, so a half-way case is the
    # only way to differ, by one
    assert np.abs(s16.astype(np.int64) - np.rint(65535.0 * want).astype(np.int64)).max() <= 1
    assert s16[1] == 0 and s16.max() == 65535 and (s16 > 0).sum() >= P // 2


def test_cost_volume_cubes_departures():
    batch = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    batch[:, 0, 3] = [0.0, 0.1, 0.2]
    c, h, s = geometry_utils.cost_volume_cubes(np.array([0.0, 0.3, 0.0]), (3, 1, 1, 1, 1, 1), batch)
    assert s.tolist() == [0, 65535, 0] and np.allclose(h, 0.05)                # one non-zero score -> 1; y and z left out of the spacing
    c, h, s = geometry_utils.cost_volume_cubes(np.zeros(3), (3, 1, 1, 1, 1, 1), batch)
    assert s.tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ the engine's default

def test_dream_best_pose_keeps_its_default():
    from dream2real_amd.dream2real import ImaginationEngine
    p = inspect.signature(ImaginationEngine.dream_best_pose).parameters
    assert list(p) == ["self", "task_model", "vis_cost_vol"] and p["vis_cost_vol"].default is False
    for fn, extras in ((geometry_utils.vis_cost_volume, ["ctx", "view", "cam_pose", "out_path"]), (geometry_utils.vis_best_pose, ["ctx", "view", "cam_pose", "out_path"])):
        q = inspect.signature(fn).parameters
        assert [k for k, v in q.items() if v.kind is v.KEYWORD_ONLY] == extras
    q = inspect.signature(geometry_utils.vis_cost_volume).parameters
    assert list(q)[:8] == ["pose_scores", "sample_res", "pose_batch", "bground_geoms", "use_phys_mods", "colourmap", "fixed_ori", "exp"]
