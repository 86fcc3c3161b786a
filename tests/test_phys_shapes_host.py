"""CPU side of the hull backend's shape tests: the inputs of tests/test_phys_shapes_gpu.py are what they claim to be, and
the oracle alone is unambiguous on them — its masks at margin - BAND, margin and margin + BAND coincide for every case,
margin and stability setting the GPU file uses, so no pose lies within the +-1e-5 m band in which a float32 GJK and a
double LP / QP may differ, and the GPU test may demand equality."""
import time

import numpy as np
import pytest
from scipy.spatial import ConvexHull

from oracle import phys_ref
from tests import phys_cases as pc


def check_band_free(case):
    t0 = time.time()
    for m in case.margins:
        for stab in case.stabs:
            lo, at, hi = pc.band_masks(case, m, stab)
            diff = np.nonzero((lo != at) | (hi != at))[0]
            assert diff.size == 0, f"{case.name} margin {m} stability {stab}: poses {diff[:10]} lie inside the band: move the grid"
            if case.mixed:
                assert 0 < at.sum() < len(at), (case.name, m, stab, int(at.sum()))
            assert not (at & ~case.valid0()).any()
    print(f"[oracle] {case.name}: {len(case.poses)} poses, {time.time() - t0:.1f} s")


def test_margin_constant_matches_the_package():
    from dream2real_amd import physics_utils
    assert pc.MESH_MARGIN == physics_utils.PYBULLET_MESH_MARGIN


@pytest.mark.parametrize("kind", ["sixdof", "edges"])
def test_sweep_worlds_are_band_free(kind):
    case = pc.sweep_case(kind)
    check_band_free(case)
    if kind == "sixdof":
        assert not np.allclose(case.init[:3, :3], np.eye(3))                       # a non-identity initial pose is in play
        R = case.poses.reshape(-1, 4, 4)[:, :3, :3]
        assert (np.abs(R - np.eye(3)).max(axis=(1, 2)) > 0.1).mean() > 0.5         # general support directions
    for m in case.margins:                                                          # stability and the margin matter on these grids
        assert len(case.stabs) == 1 or (pc.want(case, m, True) != pc.want(case, m, False)).any()
    if kind == "edges":
        assert (pc.want(case, 0.0) != pc.want(case, pc.MESH_MARGIN)).any()


@pytest.mark.parametrize("kind", ["sixdof", "edges"])
def test_offset_worlds_are_band_free(kind):
    case = pc.offset_case(kind)
    check_band_free(case)
    base = pc.sweep_case(kind)
    assert np.allclose(case.movable[0] - base.movable[0], pc.OFFSET, atol=1e-6)
    # float32 spacing out there: 2.4e-7 m, a fortieth of the band
    assert np.spacing(np.float32(np.abs(pc.OFFSET).max())) < 2.5e-7


@pytest.mark.parametrize("kind", ["sixdof", "edges"])
@pytest.mark.parametrize("n", pc.COUNTS)
def test_padding_keeps_the_hull_and_puts_the_extremes_where_it_says(kind, n):
    case = pc.sweep_case(kind)
    for E in (case.movable[0], case.statics[1]):
        k = len(E)
        hull = ConvexHull(E)
        assert len(hull.vertices) == k                                               # E is an extreme set: every vertex a corner
        for pl in pc.PLACEMENTS:
            P, idx = pc.pad_hull(E, n, pl)
            assert P.shape == (n, 3) and (P == P.astype(np.float32)).all() and np.isfinite(P).all()
            copy = (P[:, None, :] == E[None, :, :]).all(2).any(1)
            assert copy[idx.reshape(-1)].all() and (P[idx.reshape(-1)] == np.concatenate([E] * idx.ndim)).all()
            # every other point lies strictly inside conv(E): conv(padded) = conv(E)
            depth = (P[~copy] @ hull.equations[:, :3].T + hull.equations[:, 3]).max(1) if (~copy).any() else np.array([-1.0])
            assert depth.max() < -1e-4 * np.ptp(E, axis=0).min(), (pl, depth.max())
            assert (~copy).sum() >= (n - 2 * k) // 2                                 # and most of the padding is such points
            last = pc.last_stride_start(n)
            where = np.nonzero(copy)[0]
            if pl == "a":
                assert where.max() < 64 and len(where) == k
            elif pl == "b":
                assert len(where) == k and where.min() == n - k and copy[n - 1]
                if n - last >= k:
                    assert where.min() >= last                                       # e.g. n = 1000: all at indices >= 960
                else:
                    assert n - last == 1                                             # 65, 129: index n - 1 is the last stride
            elif pl == "c":
                assert set(idx // 64) == set(range(pc.strides(n))) or k < pc.strides(n)
                if pc.strides(n) > 1:
                    assert len(set(idx // 64)) == min(k, pc.strides(n))
            else:
                assert idx.shape == (2, k) and idx[0].max() < 64 and (idx[1] == np.arange(n - k, n)).all()
                assert (idx[0] < idx[1]).all() and (P[idx[0]] == P[idx[1]]).all()      # the tie rule has a lower index to pick


@pytest.mark.parametrize("role", ["movable", "pebble"])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_small_hull_worlds_are_band_free(k, role):
    case = pc.small_case(k, role)
    assert len(case.movable[0] if role == "movable" else case.statics[1]) == k
    check_band_free(case)
    assert (pc.want(case, 0.0) != pc.want(case, 0.001)).any()


@pytest.mark.parametrize("P,p", pc.COMBS)
def test_comb_worlds_are_band_free_and_hang_on_one_part(P, p):
    case = pc.comb_case(P, p)
    assert len(case.movable) == P
    check_band_free(case)
    for j, m in enumerate(case.margins):
        w = pc.want(case, m)
        assert w.tolist() == [ans[j] for _, ans in pc.COMB_PROBES]                  # the hand-written expectation
        if P > 1:                                                                     # without part p the mask changes: that part decides
            rest = [h for i, h in enumerate(case.movable) if i != p]
            w_rest = phys_ref.unsupcol_check(case.poses, case.init, rest, list(case.statics), list(case.res), case.valid0(),
                                             case.table_z, margin=m)
            assert (w_rest != w).any() and not w_rest.any()


@pytest.mark.parametrize("p", [15, 16])
def test_comb_sixdof_world_is_band_free(p):
    case = pc.comb_case(17, p, True)
    check_band_free(case)
    R = case.poses.reshape(-1, 4, 4)[:, :3, :3]
    assert (np.abs(R - np.eye(3)).max(axis=(1, 2)) > 0.04).sum() >= 4 * len(pc.COMB_PROBES)
    for m in case.margins:
        rest = [h for i, h in enumerate(case.movable) if i != p]
        w_rest = phys_ref.unsupcol_check(case.poses, case.init, rest, list(case.statics), list(case.res), case.valid0(),
                                         case.table_z, margin=m)
        assert not w_rest.any() and pc.want(case, m).sum() >= 5


@pytest.mark.parametrize("S", [1, 64, 257])
def test_tile_worlds_are_band_free_and_reach_the_last_tile(S):
    case = pc.tiles_case(S)
    assert len(case.statics) == S
    check_band_free(case)
    if S > 1:
        for m in case.margins:
            w_rest = phys_ref.unsupcol_check(case.poses, case.init, list(case.movable), list(case.statics[:-1]), list(case.res),
                                             case.valid0(), case.table_z, margin=m)
            assert (w_rest != pc.want(case, m)).any()                                  # the tile at index S - 1 decides some poses


def test_pose_count_worlds_are_band_free():
    full = pc.count_case(259, "all")
    check_band_free(full)
    w = pc.want(full, 0.0)
    assert 0 < w.sum() < 259 and w[-1]
    for N in pc.POSE_COUNTS:
        assert w[N - 1] and (N == 1 or 0 < w[:N].sum() < N)
        for pat in pc.V0_PATTERNS:
            case = pc.count_case(N, pat)
            check_band_free(case)
            # one orientation per position: a pose's answer depends on nothing but itself and its own valid_so_far
            assert (pc.want(case, 0.0) == (w[:N] & case.v0)).all()
    assert (np.arange(259) // 4 == 64).sum() == 3                                    # 259 leaves the 65th block with three poses


def test_orientation_world_is_band_free_and_the_duplicate_rule_clears_some():
    case = pc.orientation_case()
    check_band_free(case)
    n_ori = int(np.prod(case.res[3:]))
    m = phys_ref.unique_orientation_mask(case.poses.reshape(-1, 4, 4)[:n_ori, :3, :3])
    assert 1 < m.sum() < n_ori
    w = pc.want(case, 0.0)
    assert not w.reshape(-1, n_ori)[:, ~m].any() and w.reshape(-1, n_ori)[:, m].any()


def test_no_statics_means_unsupported_unless_below_the_table():
    case = pc.nostatic_case()
    check_band_free(case)
    z = case.poses.reshape(-1, 4, 4)[:, 2, 3]
    for m in case.margins:
        assert (pc.want(case, m) == (z < np.float32(case.table_z))).all()


def test_cap_world_keeps_clear_of_the_band():
    """The oracle's QP on 1000 + 8 weights takes minutes per pair, so the reference and the band condition of this one case
    are the closed form its geometry allows: over the table's middle the hull distance is the height of the lowest vertex."""
    case = pc.cap_case()
    assert len(ConvexHull(case.movable[0]).vertices) == pc.CAP_N == len(case.movable[0])   # 1000 extreme vertices, no padding
    assert case.margins == (0.0, pc.MESH_MARGIN) and len(case.poses) == pc.CAP_TURNS * len(pc.CAP_GAPS)
    z, z_low = pc.cap_heights(case)
    assert np.abs(z.reshape(pc.CAP_TURNS, -1) - np.array(pc.CAP_GAPS)).max() < 1e-7       # the heights are the ones listed
    xy = case.poses.reshape(-1, 4, 4)[:, :2, 3]
    assert (np.abs(xy) + pc.CAP_R < 0.5).all()                                        # well inside the slab's footprint
    for m in case.margins:
        for h in (z, z_low):                                                           # 1.9e-5 m, nearly two band widths, clear of the contact distance
            assert (np.abs(h - 2 * m) > 1.9 * 2 * pc.BAND).all()
        masks = [pc.cap_want(case, mm) for mm in (max(0.0, m - pc.BAND), m, m + pc.BAND)]
        assert (masks[0] == masks[1]).all() and (masks[2] == masks[1]).all() and 0 < masks[1].sum() < len(z)
        for h in (z, z_low):                                                           # both answers within 0.1 mm of the contact distance
            assert (np.abs(h - 2 * m) < 1.05e-4).sum() >= 2 * pc.CAP_TURNS and ((h > 2 * m) & (h - 2 * m < 1.05e-4)).any()
    # at margin 0 the oracle's LP does run on all 1008 points: it agrees with the closed form (the first two turns)
    sub = slice(0, 2 * len(pc.CAP_GAPS))
    w = phys_ref.unsupcol_check(case.poses[sub], case.init, list(case.movable), list(case.statics), [2 * len(pc.CAP_GAPS), 1, 1, 1, 1, 1],
                                np.ones(2 * len(pc.CAP_GAPS), bool), case.table_z, stability_check=False, margin=0.0)
    assert (w == pc.cap_want(case, 0.0)[sub]).all()
