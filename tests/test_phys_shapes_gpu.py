"""The hull backend (phys.hip k_phys_check, one wave per pose, GJK) at the hull sizes, part counts, static counts and pose
counts beyond tests/test_physics.py: vertex counts across the 64-lane stride (63 ... 1000, the extreme vertices in the
first stride, the last, spread, or doubled), hulls of 1 to 4 vertices, compounds of up to 33 parts (the boxes of the
first 16 are kept per wave), 257 statics, partly filled blocks and every kind of incoming mask, a world a few metres from
the origin, and 1000 extreme vertices near contact.

Two comparisons, both over whole masks and with no tolerance: GPU(padded) == GPU(E) — an interior point never wins a
support query and a duplicate that wins has the same coordinates, so every GJK iterate is the same float — and
GPU(E) == oracle(E): tests/test_phys_shapes_host.py shows on the CPU that the oracle's masks at margin - BAND, margin and
margin + BAND coincide on every case here, so no pose lies in the band where float32 and double may differ."""
import numpy as np
import pytest

from tests import phys_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def gpu_mask(ctx, case, margin, stab=True, movable=None, statics=None):
    from dream2real_amd import physics_utils
    sh = physics_utils.PhysicsShapes(ctx, list(case.movable if movable is None else movable),
                                     list(case.statics if statics is None else statics))
    try:
        return sh.check(case.poses, case.valid0(), list(case.res), case.init, case.table_z, stability_check=stab, margin=margin)
    finally:
        sh.close()


def assert_equals_oracle(ctx, case, **shapes):
    """GPU == oracle on the small shapes, for every margin and stability setting of the case, no pose exempt; -> the GPU masks"""
    out = {}
    for m in case.margins:
        for stab in case.stabs:
            got = gpu_mask(ctx, case, m, stab, **shapes)
            w = pc.want(case, m, stab)
            print(f"[parity] physics {case.name} margin {m} stability {stab}: {int((got != w).sum())} of {len(w)} poses differ from the oracle")
            assert (got == w).all(), (case.name, m, stab, np.nonzero(got != w)[0][:10])
            assert not case.mixed or 0 < w.sum() < len(w)
            out[m, stab] = got
    return out


def assert_padding_is_invisible(ctx, case, target, n, base):
    for pl in pc.PLACEMENTS:
        for roll in pc.rolls(case, target, n, pl):
            mov, stat = pc.padded_shapes(case, target, n, pl, roll)
            for (m, stab), ref in base.items():
                got = gpu_mask(ctx, case, m, stab, mov, stat)
                assert (got == ref).all(), (case.name, target, n, pl, roll, m, stab, np.nonzero(got != ref)[0][:10])


@pytest.fixture(scope="module")
def sweep_base(ctx):
    """GPU masks on the small shapes of the two sweep worlds, checked against the oracle once"""
    return {kind: assert_equals_oracle(ctx, pc.sweep_case(kind)) for kind in ("sixdof", "edges")}


@pytest.mark.parametrize("n", pc.COUNTS)
@pytest.mark.parametrize("target", ["movable", "static"])
@pytest.mark.parametrize("kind", ["sixdof", "edges"])
def test_vertex_count_sweep(ctx, sweep_base, kind, target, n):
    case = pc.sweep_case(kind)
    base = sweep_base[kind]
    if n != 129:                                            # stability on and off at one count, on for the rest
        base = {k: v for k, v in base.items() if k[1]}
    assert_padding_is_invisible(ctx, case, target, n, base)


@pytest.mark.parametrize("kind", ["sixdof", "edges"])
def test_vertex_count_both_hulls_padded(ctx, sweep_base, kind):
    assert_padding_is_invisible(ctx, pc.sweep_case(kind), "both", 129, sweep_base[kind])


@pytest.mark.parametrize("role", ["movable", "pebble"])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_very_small_hulls(ctx, k, role):
    case = pc.small_case(k, role)
    base = assert_equals_oracle(ctx, case)
    # the same hull with every vertex listed three times
    small = case.movable[0] if role == "movable" else case.statics[1]
    triple = np.concatenate([small] * 3)
    shapes = dict(movable=[triple]) if role == "movable" else dict(statics=[case.statics[0], triple])
    for (m, stab), ref in base.items():
        got = gpu_mask(ctx, case, m, stab, **shapes)
        assert (got == ref).all(), (case.name, "tripled", m, np.nonzero(got != ref)[0][:10])


@pytest.mark.parametrize("P,p", pc.COMBS)
def test_part_count_boundary(ctx, P, p):
    case = pc.comb_case(P, p)
    got = assert_equals_oracle(ctx, case)
    for j, m in enumerate(case.margins):
        assert got[m, True].tolist() == [ans[j] for _, ans in pc.COMB_PROBES]


@pytest.mark.parametrize("p", [15, 16])
def test_part_count_boundary_sixdof(ctx, p):
    assert_equals_oracle(ctx, pc.comb_case(17, p, True))


@pytest.mark.parametrize("S", [1, 64, 257])
def test_many_statics(ctx, S):
    assert_equals_oracle(ctx, pc.tiles_case(S))


@pytest.mark.parametrize("N", pc.POSE_COUNTS)
def test_pose_count_and_mask_edges(ctx, N):
    for pat in pc.V0_PATTERNS:
        case = pc.count_case(N, pat)
        got = assert_equals_oracle(ctx, case)[0.0, True]
        assert not (got & ~case.v0).any()                   # a pose that comes in invalid stays invalid
        if pat == "none":
            assert not got.any()
        if pat == "only-last":
            assert got[-1] and got.sum() == 1               # the last wave of a partly filled block is live


def test_orientation_mask_clears_duplicates(ctx):
    case = pc.orientation_case()
    got = assert_equals_oracle(ctx, case)[0.0, True]
    assert not (got & ~case.v0).any()


def test_no_static_shapes(ctx):
    case = pc.nostatic_case()
    got = assert_equals_oracle(ctx, case)
    z = case.poses.reshape(-1, 4, 4)[:, 2, 3]
    for g in got.values():
        assert (g == (z < np.float32(case.table_z))).all()  # every pose not below table_z is unsupported


@pytest.mark.parametrize("kind", ["sixdof", "edges"])
def test_offset_world(ctx, kind):
    """The world of the sweep moved by (2.3, -1.7, 0.9) m, where float32 spacing is 2.4e-7 m: the +-1e-5 m band must still hold."""
    case = pc.offset_case(kind)
    base = assert_equals_oracle(ctx, case)
    for target in ("movable", "static", "both"):
        assert_padding_is_invisible(ctx, case, target, 129, base)
    near = pc.sweep_case(kind)                              # and the answers are those of the world at the origin
    for m in case.margins:
        assert (pc.want(case, m) == pc.want(near, m)).all()


@pytest.mark.parametrize("margin", [0.0, pc.MESH_MARGIN])
def test_iteration_cap_on_a_thousand_extreme_vertices(ctx, margin):
    """1000 extreme vertices over a 2 m slab, the lowest 2e-5 m to 0.1 mm either side of the contact distance (0, and 2 mm
    at the production margin), at the pose or after the 2 cm drop: the input that takes the GJK nearest its 48-step cap
    and its simplex routines nearest their rounding.  Reference: the closed form (height of the lowest vertex), whose band
    condition the host test shows; the mask must equal it at every pose, and repeat.  Before round 14's fix of the
    triangle's interior point a host copy of the loop gave 5 wrong answers and 3 runs into the cap on these 520 queries;
    with it none, and at most 9 steps (docs/history/r14.md)."""
    case = pc.cap_case()
    want = pc.cap_want(case, margin)
    first = gpu_mask(ctx, case, margin, False)
    print(f"[parity] physics {case.name} margin {margin}: {int((first != want).sum())} of {len(want)} poses differ from the closed form")
    assert (first == want).all(), (margin, np.nonzero(first != want)[0][:10])
    assert (gpu_mask(ctx, case, margin, False) == first).all()
