"""Shapes, pose grids and shared helpers of the hull backend's shape tests (tests/test_phys_shapes_host.py on the CPU,
tests/test_phys_shapes_gpu.py on the GPU; BAND and assert_equal_away_from_band also serve tests/test_physics.py).

The oracle (oracle/phys_ref.py: an LP at margin 0, a QP in double for margin > 0) is slow on large vertex sets, so a large
hull is built from a small extreme set E: E plus points strictly inside conv(E) plus exact copies of vertices of E.  Then
conv(padded) = conv(E), the oracle runs on E and the GPU receives the padded array.  A `Case` holds the small shapes, the
poses and the settings; `want(case, margin, stab)` is the oracle's mask, computed once per process and never written to."""
import dataclasses
import functools

import numpy as np

from oracle import host_ref, phys_ref
from synthetic_scenes import box, icosphere

BAND = 5e-6      # metres of collision margin = 1e-5 m of hull distance
MESH_MARGIN = 0.001                      # dream2real_amd.physics_utils.PYBULLET_MESH_MARGIN (asserted equal in the host test)
PLACEMENTS = ("a", "b", "c", "d")
COUNTS = (63, 64, 65, 127, 128, 129, 1000)
OFFSET = np.array([2.3, -1.7, 0.9])      # case 6: the whole world moved a few metres out


def assert_equal_away_from_band(got, want_fn, margin, what=""):
    """The GPU decides contact by float32 distance GJK, the oracle by an LP / QP in double: a pair whose hull distance lies
    within BAND-rounding of the contact distance 2 * margin may fall either way; everywhere else the masks must be EQUAL.
    Checked as: every pose's GPU answer equals the oracle's answer for the margin itself or for a margin BAND smaller or
    larger (a contact distance within +-1e-5 m)."""
    w0 = want_fn(margin)
    ok = got == w0
    n_off = int((~ok).sum())
    if n_off:
        ok |= got == want_fn(max(0.0, margin - BAND))
        ok |= got == want_fn(margin + BAND)
    print(f"[parity] physics {what} margin {margin}: {n_off} of {len(got)} poses differ from the oracle at the margin itself, "
          f"{int((~ok).sum())} outside the +-{2 * BAND:.0e} m band")
    assert ok.all(), (what, margin, np.nonzero(~ok)[0][:10])
    return w0


def f32(a):
    """the values the GPU sees (float32), as float64 for the oracle: both sides then work on the same points"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def pose_list(ts, Rs=None):
    """[N,16] float32 poses from translations (and rotations)"""
    out = np.tile(np.eye(4, dtype=np.float32).reshape(16), (len(ts), 1)).reshape(-1, 4, 4)
    out[:, :3, 3] = np.asarray(ts, np.float64)
    if Rs is not None:
        out[:, :3, :3] = np.asarray(Rs, np.float64)
    return out.reshape(-1, 16)


def grid(xs, ys, zs):
    return pose_list([(x, y, z) for x in xs for y in ys for z in zs])


# ---------------------------------------------------------------------------------------------------- padding

def strides(n):
    return (n - 1) // 64 + 1


def last_stride_start(n):
    return 64 * ((n - 1) // 64)


def pad_hull(E, n, placement, seed=0, roll=0):
    """-> (padded [n,3] float64 of float32 values, idx [|E|] or [2,|E|]: where E's vertices sit).
    (a) E in the first stride, indices 0..63;  (b) E in the last |E| indices, which is inside the last stride
    (>= 64 * ((n - 1) // 64)) whenever that stride has |E| slots — at n = 65 and 129 it has one, then the vertex at n - 1 is
    the stride's only occupant and the rest sit right below it;  (c) dealt round-robin over the strides;  (d) every vertex
    twice, in the first stride and at the (b) positions.  The fill is interior points — convex combinations of E pulled
    towards E's centroid by a factor in [0.3, 0.9] — in (a), (b), (c), so that the claim 'no extreme vertex elsewhere' is
    sharp; (c) also gets exact copies of vertices of E in an eighth of the free slots, (d) in a quarter.
    roll: E's vertices are taken in an order rolled by this much, which decides who sits at index n - 1."""
    E = np.roll(f32(E), roll, axis=0)
    k = len(E)
    need = 2 * k if placement == "d" else k
    assert need <= n and (placement != "a" or k <= 64), (k, n, placement)
    r = np.random.default_rng(1000 * n + 10 * seed + PLACEMENTS.index(placement))
    S = strides(n)
    tail = np.arange(n - k, n)
    if placement == "a":
        idx = np.sort(r.choice(min(n, 64), k, replace=False))
    elif placement == "b":
        idx = tail
    elif placement == "c":
        free = [list(r.permutation(np.arange(64 * s, min(n, 64 * s + 64)))) for s in range(S)]
        idx = np.zeros(k, np.int64)
        for j in range(k):
            s = j % S
            while not free[s]:
                s = (s + 1) % S
            idx[j] = free[s].pop()
    else:
        first = np.setdiff1d(np.arange(min(n, 64)), tail)
        idx = np.stack([np.sort(r.choice(first, k, replace=False)), tail])
    out = np.full((n, 3), np.nan)
    out[idx.reshape(-1)] = np.concatenate([E] * (2 if placement == "d" else 1))
    rest = np.nonzero(np.isnan(out[:, 0]))[0]
    w = r.dirichlet(np.ones(k), len(rest))
    pull = r.uniform(0.3, 0.9, (len(rest), 1))
    c = E.mean(0)
    out[rest] = c + pull * (w @ E - c)
    share = {"c": 8, "d": 4}.get(placement)
    if share and len(rest):
        cp = rest[r.random(len(rest)) < 1.0 / share]
        out[cp] = E[r.integers(0, k, len(cp))]
    return f32(out), idx


# ---------------------------------------------------------------------------------------------------- cases

@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    movable: tuple               # convex parts (E form), float64 arrays of float32 values
    statics: tuple
    poses: np.ndarray            # [N,16] float32
    res: tuple
    init: np.ndarray             # 4x4 float32
    table_z: float
    margins: tuple = (0.0, MESH_MARGIN)
    stabs: tuple = (True,)
    v0: np.ndarray = None        # valid_so_far; None: all true
    mixed: bool = True           # the oracle's mask must hold both answers

    def valid0(self):
        return np.ones(len(self.poses), bool) if self.v0 is None else self.v0

    def moved(self, d):
        """the same world translated by d: shapes, initial pose, poses and the table height"""
        init = self.init.copy()
        init[:3, 3] = (self.init[:3, 3].astype(np.float64) + d).astype(np.float32)
        poses = self.poses.reshape(-1, 4, 4).copy()
        poses[:, :3, 3] = (poses[:, :3, 3].astype(np.float64) + d).astype(np.float32)
        return dataclasses.replace(self, name=self.name + "+offset", movable=tuple(f32(m + d) for m in self.movable),
                                   statics=tuple(f32(s + d) for s in self.statics), poses=poses.reshape(-1, 16), init=init,
                                   table_z=self.table_z + float(d[2]))


def _case(name, movable, statics, poses, res=None, init=None, table_z=-0.3, **kw):
    movable = movable if isinstance(movable, (list, tuple)) else [movable]
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    res = tuple(res) if res is not None else (len(poses), 1, 1, 1, 1, 1)
    assert int(np.prod(res)) == len(poses)
    init = np.eye(4, dtype=np.float32) if init is None else np.asarray(init, np.float32)
    for a in (poses, init):
        a.setflags(write=False)
    return Case(name, tuple(f32(m) for m in movable), tuple(f32(s) for s in statics), poses, res, init, float(table_z), **kw)


_WANT = {}


def want(case, margin, stab=True):
    """the oracle's mask on the case's small shapes; computed once, shared, never written to"""
    key = (case.name, float(margin), bool(stab))
    if key not in _WANT:
        w = phys_ref.unsupcol_check(case.poses, case.init, list(case.movable), list(case.statics), list(case.res), case.valid0(),
                                    case.table_z, stability_check=stab, margin=margin)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def band_masks(case, margin, stab=True):
    return [want(case, m, stab) for m in (max(0.0, margin - BAND), margin, margin + BAND)]


TABLE = box([-1, -1, -0.1], [1, 1, 0.0])
BLOCK = box([0.30, -0.10, 0.0], [0.50, 0.10, 0.20])
MOV_BOX = box([-0.05, -0.05, 0.0], [0.05, 0.05, 0.10]) + [0, 0, 0.005]      # 5 mm above the table at its initial pose


@functools.lru_cache(maxsize=None)
def sweep_case(kind):
    """case 1's two worlds.  'sixdof': scene type 1 eulers, a rounded 24-vertex movable hull at a non-identity initial pose
    over a shelf and a rounded 30-vertex blob.  'edges': the table-and-block scene, a translation grid across the block's
    edge (x = 0.30) and the table's edge (x = 1)."""
    if kind == "sixdof":
        mov = icosphere([0.45, 0.85, 0.27], 0.05, 24, 1) * [1.0, 1.0, 1.6] - [0, 0, 0.16]
        shelf = box([-0.3, 1.1, 0.18], [1.2, 1.5, 0.22])
        blob = icosphere([0.55, 1.27, 0.30], 0.07, 30, 2)
        init = np.eye(4, dtype=np.float32)
        init[:3, :3] = rot("z", 0.4).astype(np.float32)
        init[:3, 3] = (0.45, 0.85, 0.2)
        res = (3, 2, 5, 2, 2, 2)
        poses = host_ref.sample_poses_grid([0.4513, 0.8507, 0.2011], res, 1)
        return _case("sweep-sixdof", mov, [shelf, blob], poses, res, init, 0.2)
    xs = np.r_[np.linspace(0.18, 0.42, 9), np.linspace(0.9, 1.1, 6)] + 0.0013
    # 5 mm initial gap, lowered by 2 cm: z offsets 0.0165 / 0.0185 leave 1.5 / 3.5 mm, inside / outside the 2 mm of two margins
    poses = grid(xs, [0.0007, 0.1207], [0.0, 0.0165, 0.0185, 0.1, 0.2055, 0.2165, 0.2185, -0.5])
    return _case("sweep-edges", MOV_BOX, [TABLE, BLOCK], poses, (len(xs), 2, 8, 1, 1, 1), stabs=(True, False))


def padded_shapes(case, target, n, placement, roll=0):
    """(movable parts, statics) with one hull ('movable' / 'static') or both ('both') padded to n vertices"""
    mov, stat = list(case.movable), list(case.statics)
    if target in ("movable", "both"):
        mov[0] = pad_hull(mov[0], n, placement, seed=1, roll=roll)[0]
    if target in ("static", "both"):
        stat[1] = pad_hull(stat[1], n, placement, seed=2, roll=roll)[0]
    return mov, stat


def rolls(case, target, n, placement):
    """orders of E to run: one, except where the last stride is the single index n - 1 and E sits at the tail (n = 65, 129,
    placement b) — there every vertex of E takes its turn as that stride's only occupant"""
    if placement != "b" or n - last_stride_start(n) != 1:
        return range(1)
    return range(max(len(case.movable[0]) if target != "static" else 0, len(case.statics[1]) if target != "movable" else 0))


SMALL = {1: np.array([[0.0, 0.0, 0.0]]),
         2: np.array([[-0.04, 0.0, 0.0], [0.04, 0.01, 0.03]]),
         3: np.array([[-0.04, -0.02, 0.0], [0.04, -0.01, 0.01], [0.0, 0.03, 0.03]]),
         4: np.array([[-0.04, -0.02, 0.0], [0.04, -0.01, 0.0], [0.0, 0.03, 0.01], [0.0, 0.0, 0.04]])}


@functools.lru_cache(maxsize=None)
def small_case(k, role):
    """case 2: a hull of k = 1..4 vertices as the movable object over the table-and-block scene, or as a static pebble on the
    table under a movable box.  The grids keep a millimetre off coplanarity."""
    if role == "movable":
        xs = np.r_[np.linspace(0.22, 0.58, 10), [0.93, 1.07]] + 0.0013
        poses = grid(xs, [0.0007, 0.0907], [0.0, 0.0165, 0.0185, 0.1, 0.2055, 0.2165, 0.2185])
        return _case(f"small-{k}-movable", SMALL[k] + [0, 0, 0.005], [TABLE, BLOCK], poses, (len(xs), 2, 7, 1, 1, 1))
    pebble = SMALL[k] + [0.7, 0.0, 0.03]                     # its lowest vertex 3 cm above the table: the box fits over it or not
    xs = np.linspace(0.58, 0.82, 13) + 0.0013
    poses = grid(xs, [0.0007, 0.0607], [0.0115, 0.0165, 0.0375, 0.0565, 0.0895, 0.12])
    return _case(f"small-{k}-pebble", MOV_BOX, [TABLE, pebble], poses, (len(xs), 2, 6, 1, 1, 1))


PART, PITCH, COMB_H = 0.10, 0.12, 0.03     # comb: parts of 10 x 10 x 3 cm, 2 cm apart: the +-4 cm probes of a pose over a part's middle stay over it
PEBBLE = box([-0.005, -0.005, 0.0], [0.005, 0.005, 0.02])
COMBS = [(1, 0), (15, 0), (15, 14), (16, 0), (16, 15), (17, 0), (17, 15), (17, 16), (33, 0), (33, 15), (33, 16), (33, 32)]


def comb(P):
    return [box([PITCH * i, 0.0, 0.0], [PITCH * i + PART, PART, COMB_H]) for i in range(P)]


# offsets of the part's middle from the pebble (dx, dy) and heights of the comb's underside above the pebble's top, with
# the hand-written answer: inside the pebble -> collision; 1.15 cm above -> supported, and stable while all four probes
# stay over the part (|dx|, |dy| + 4.5 cm <= 5 cm) ; 2.35 cm above -> the 2 cm drop does not reach
#  (answers at margin 0 and at 1 mm);  2.15 cm above -> the drop leaves 1.5 mm: contact only with the 2 mm of two margins
COMB_PROBES = [((0.0013, 0.0007, -0.0065), (False, False)), ((0.0013, 0.0007, 0.0115), (True, True)),
               ((0.0013, 0.0007, 0.0235), (False, False)), ((-0.0037, 0.0043, 0.0115), (True, True)),
               ((0.0213, 0.0007, 0.0115), (False, False)), ((0.0013, -0.0187, 0.0115), (False, False)),
               ((0.0033, -0.0027, 0.0185), (True, True)), ((0.0013, 0.0007, 0.0215), (False, True))]


@functools.lru_cache(maxsize=None)
def comb_case(P, p, sixdof=False):
    """case 3: a row of P boxes; the statics are a table far below and one pebble; every pose puts the pebble under, or
    inside, part p alone.  sixdof: the comb also turned (about z, about y, upside down), so the rotated parts' boxes matter."""
    table = box([-9, -9, -3.1], [9, 9, -3.0])
    peb = PEBBLE + [0.4, 0.3, 0.0]
    mid = np.array([PITCH * p + PART / 2, PART / 2, 0.0])            # part p's underside centre, comb frame
    top = np.array([0.4, 0.3, 0.02])
    ts, Rs = [], []
    rots = [np.eye(3)] if not sixdof else [np.eye(3), rot("z", 0.3), rot("z", -2.1), rot("y", 0.05) @ rot("z", 0.7),
                                           rot("x", np.pi) @ rot("z", 0.2)]
    for R in rots:
        under = mid + ([0, 0, COMB_H] if R[2, 2] < 0 else 0)          # upside down: the other face looks at the pebble
        for (dx, dy, dz), _ in COMB_PROBES:
            ts.append(top + [dx, dy, dz] - R @ under)
            Rs.append(R)
    return _case(f"comb-{P}-{p}" + ("-sixdof" if sixdof else ""), comb(P), [table, peb], pose_list(ts, Rs), table_z=-5.0)


def tiles(S):
    """case 4: S tiles of 10 x 10 x 2 cm, 2 cm apart, 16 to a row, every third raised by 1.3 cm"""
    return [box([PITCH * (i % 16), PITCH * (i // 16), 0.0], [PITCH * (i % 16) + PART, PITCH * (i // 16) + PART, 0.02]) +
            [0, 0, 0.013 * (i % 3 == 2)] for i in range(S)]


@functools.lru_cache(maxsize=None)
def tiles_case(S):
    """a 5 cm cube dragged along x over the last tiles of the floor (edges, gaps, the raised tile, past the end) and, where
    there is one, along y from the row before"""
    cube = box([-0.025, -0.025, 0.0], [0.025, 0.025, 0.05])
    last = S - 1
    x_end, y_row = PITCH * (last % 16) + PART, PITCH * (last // 16) + PART / 2
    xs = np.linspace(x_end - 0.25, x_end + 0.05, 11) + 0.0013
    ys = [y_row + 0.0007, y_row + 0.0557] if S == 1 else [y_row + 0.0007, y_row - 0.0593, y_row - PITCH + 0.0007]
    zs = [0.0105, 0.0215, 0.0315, 0.0385, 0.0545]
    return _case(f"tiles-{S}", cube, tiles(S), grid(xs, ys, zs), (len(xs), len(ys), len(zs), 1, 1, 1))


V0_PATTERNS = ("all", "alternating", "none", "all-but-last", "only-last")
POSE_COUNTS = (1, 3, 4, 5, 259)


def v0_pattern(N, pattern):
    v = np.ones(N, bool)
    if pattern == "alternating":
        v[1::2] = False
    elif pattern == "none":
        v[:] = False
    elif pattern == "all-but-last":
        v[-1] = False
    elif pattern == "only-last":
        v[:-1] = False
    return v


@functools.lru_cache(maxsize=None)
def count_poses():
    """259 poses of the table-and-block scene, ordered so that every prefix of 1, 3, 4 and 5 holds both answers when all
    come in valid, and the last pose of each is a valid one"""
    head = [(0.0013, 0.0007, 0.0), (0.4013, 0.0007, 0.1), (0.4013, 0.0007, 0.2055), (0.0013, 0.0907, 0.0135), (-0.1487, 0.0007, 0.0115)]
    r = np.random.default_rng(7)
    rest = np.c_[np.round(r.uniform(0.15, 1.1, 253), 2) + 0.0013, np.round(r.uniform(-0.15, 0.15, 253), 2) + 0.0007,
                 r.choice([0.0, 0.0115, 0.0135, 0.1, 0.2055, 0.2175], 253)]
    return pose_list(head + [tuple(t) for t in rest] + [(0.0513, 0.0307, 0.0115)])


@functools.lru_cache(maxsize=None)
def count_case(N, pattern):
    """case 5: N poses (a block takes four, so 1, 3, 5 and 259 leave the last block partly filled), valid_so_far by pattern"""
    v0 = v0_pattern(N, pattern)
    return _case(f"count-{N}-{pattern}", MOV_BOX, [TABLE, BLOCK], count_poses()[:N], margins=(0.0,), v0=v0,
                 mixed=False)


@functools.lru_cache(maxsize=None)
def orientation_case():
    """case 5's orientation mask: the six-DoF world with 3 x 3 x 2 eulers per position, of which the duplicate rule clears
    some (eulers of -pi on two axes are the third axis' half turn), and a valid_so_far with holes"""
    c = sweep_case("sixdof")
    res = (2, 1, 4, 3, 3, 2)
    poses = host_ref.sample_poses_grid([0.4513, 0.8507, 0.2011], res, 1)
    v0 = np.random.default_rng(11).random(len(poses)) > 0.15
    return _case("orientations", c.movable, c.statics, poses, res, c.init, c.table_z, margins=(0.0,), v0=v0)


@functools.lru_cache(maxsize=None)
def nostatic_case():
    """no static shape at all, a movable hull of one vertex: nothing to collide with, nothing to stand on — every pose not below
    table_z is unsupported"""
    poses = grid([0.0013, 0.5], [0.0007], [-0.5, -0.3005, -0.2995, 0.0, 0.2])
    return _case("no-statics", SMALL[1], [], poses, (2, 1, 5, 1, 1, 1), margins=(0.0, MESH_MARGIN))


@functools.lru_cache(maxsize=None)
def offset_case(kind):
    """case 6: a sweep world moved by OFFSET"""
    return dataclasses.replace(sweep_case(kind).moved(OFFSET), stabs=(True,))


CAP_N, CAP_R = 1000, 0.06
# heights of the lowest vertex above the table's top, metres: either side of contact at margin 0 (0) and at the production
# margin (2 mm), each 2e-5 m = two band widths away or more, and either side of the same two after the 2 cm drop
CAP_GAPS = (-0.0001, 0.0001, 0.0019, 0.00197, 0.00198, 0.00202, 0.00203, 0.0021, 0.0199, 0.0201, 0.02197, 0.02203, 0.0231)
CAP_TURNS = 10


@functools.lru_cache(maxsize=None)
def cap_case():
    """case 7: a rounded hull of 1000 extreme vertices (every one on the sphere: none is padding) over the middle of a
    table, turned CAP_TURNS ways, its lowest vertex at each of CAP_GAPS above the table.  The only static shape is the
    table's slab, whose top is the plane z = 0 and whose footprint holds the whole hull, so a query's hull distance is the
    height of its lowest vertex: the reference and the band condition of this case are that closed form (cap_want), since
    the oracle's QP does not finish on 1008 weights."""
    ball = icosphere([0.0, 0.0, 0.0], CAP_R, CAP_N, 3)
    r = np.random.default_rng(17)
    ts, Rs = [], []
    for j in range(CAP_TURNS):
        R = np.eye(3) if j == 0 else np.linalg.qr(r.standard_normal((3, 3)))[0]
        R = R * np.sign(np.linalg.det(R))
        low = (f32(ball) @ R.T)[:, 2].min()
        for i, gap in enumerate(CAP_GAPS):
            ts.append((0.0113 * j - 0.05, 0.04 - 0.0071 * i, gap - low))
            Rs.append(R)
    return _case("cap-1000", ball, [TABLE], pose_list(ts, Rs), stabs=(False,))


def cap_heights(case):
    """height above the table's top of the lowest vertex, per pose, at the pose itself and lowered by the 2 cm drop"""
    T = case.poses.reshape(-1, 4, 4).astype(np.float64) @ np.linalg.inv(case.init.astype(np.float64))
    z = np.array([(case.movable[0] @ t[:3, :3].T + t[:3, 3])[:, 2].min() for t in T])
    return z, z - 0.02


def cap_want(case, margin):
    """closed form of the mask, stability off: no contact at the pose, contact after the drop (contact: distance <= 2 margin;
    at margin 0 a lowest vertex below the top is inside the slab)"""
    z, z_low = cap_heights(case)
    return (z > 2 * margin) & (z_low <= 2 * margin)


def write_cap_queries(path, margin=0.0):
    """the GJK queries of cap_case (each pose at itself and lowered by 2 cm) for tools/gjk_steps.cpp, and their closed-form
    answers (1 contact, 0 apart) in the last column"""
    case = cap_case()
    T = case.poses.reshape(-1, 4, 4).astype(np.float64) @ np.linalg.inv(case.init.astype(np.float64))
    a, b = case.movable[0], case.statics[0]
    z, z_low = cap_heights(case)
    with open(path, "w") as f:
        f.write(f"{len(a)} {len(b)} {2 * len(T)} {2 * margin:.9g}\n")
        for v in np.concatenate([a, b]):
            f.write("%.9g %.9g %.9g\n" % tuple(v))
        for t, h, hl in zip(T, z, z_low):
            for drop, hh in ((0.0, h), (0.02, hl)):
                f.write(" ".join("%.9g" % x for x in np.r_[t[:3, :3].reshape(9), t[:3, 3] - [0, 0, drop]].astype(np.float32)) +
                        " %d\n" % (hh <= 2 * margin))


if __name__ == "__main__":
    import sys
    if len(sys.argv) in (3, 4) and sys.argv[1] == "cap":
        write_cap_queries(sys.argv[2], float(sys.argv[3]) if len(sys.argv) == 4 else 0.0)
    else:
        sys.exit("usage: python -m tests.phys_cases cap FILE [MARGIN]")
