"""Inputs that put the TSDF kernels (csrc/tsdf.hip) at the edges of the rule of DESIGN.md section 2c, with the numpy restatement's
answer to each (tests/tsdf_ref.py, tests/sdfphys_ref.py).  Pure numpy: nothing of the product is imported here.

A case is a dict: name, bounds float32 [2,3], voxel, trunc, frames = [(depth_u16, mask, K, pose, erode_k), ...] in the order they are
integrated, nb / b0 = the grid the bounds are meant to give, mesh = whether the extraction is compared (False where only blocks
and voxels are, see many_blocks).  `case(name)` builds one, `reference(name)` holds the restatement's outputs, computed once and
write-protected.  test_tsdf_edges_host.py proves on the CPU that each case reaches the edge it is named for;
test_tsdf_edges_gpu.py compares the device with `reference` bit for bit.

Voxel 1/128 m is exact in fp32, so a plane at 1000 mm can lie exactly ON a voxel plane (tsdf == 0, sdf == -trunc).  Grids are
placed by block: bounds_of(b0, nb, ...) returns bounds whose padded extent is exactly blocks b0 .. b0 + nb - 1."""
from __future__ import annotations

import functools

import numpy as np

from tests import sdfphys_ref, tsdf_ref

VOXEL = 1.0 / 128.0
WEIGHT_THRESHOLD = 3.0


# ------------------------------------------------------------------------------------------------ toolkit
def bounds_of(b0, nb, voxel, trunc_voxels, margin=1):
    """bounds [2,3] with floor((lo - trunc) / (16 voxel)) == b0 and floor((hi + trunc) / (16 voxel)) == b0 + nb - 1 per axis; `margin`
    voxels away from the block faces (more than the rounding of a voxel size that is not a power of two)."""
    b0, nb = np.asarray(b0, np.int64), np.asarray(nb, np.int64)
    t = int(np.ceil(trunc_voxels))
    lo = (b0 * 16 + t + margin) * float(np.float32(voxel))
    hi = ((b0 + nb) * 16 - t - margin) * float(np.float32(voxel))
    assert (hi > lo).all(), "the grid is too small for this truncation distance"
    return np.stack([lo, hi]).astype(np.float32)


def look(pos, fwd, right):
    """cam_pose float32 [4,4]: camera at pos, optical axis along fwd, image x along `right` made perpendicular to it (fp64, then rounded)."""
    z = np.asarray(fwd, np.float64) / np.linalg.norm(fwd)
    x = np.asarray(right, np.float64) - np.dot(right, z) * z
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, pos
    return T.astype(np.float32)


def intrinsics(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def centre_of(b0, nb, voxel):
    return (np.asarray(b0, np.float64) * 16 + np.asarray(nb, np.float64) * 8) * float(np.float32(voxel))


AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def right_of(d):
    """an image x axis for a camera that looks along the grid axis d"""
    return (0, 1, 0) if d[0] else (0, 0, 1) if d[1] else (1, 0, 0)


def make(name, b0, nb, trunc_voxels, frames, voxel=VOXEL, mesh=True, margin=1):
    v = np.float32(voxel)
    return dict(name=name, bounds=bounds_of(b0, nb, voxel, trunc_voxels, margin), voxel=v, trunc=np.float32(trunc_voxels) * v, frames=frames,
                b0=tuple(int(b) for b in b0), nb=tuple(int(n) for n in nb), mesh=mesh)


def six_noisy_views(target, size, seed, f=128):
    """One frame along each of +-x, +-y, +-z, 1 m from `target` looking at it: fx = fy = f (128: one pixel per voxel at 1 m), a full
    mask, erode_k 1, depth 1000 + integers(-15, 16) mm drawn per frame in that order from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    c = np.asarray(target, np.float64)
    K = intrinsics(f, f, size / 2, size / 2)
    frames = []
    for d in AXES:
        depth = (1000 + rng.integers(-15, 16, (size, size))).astype(np.uint16)
        frames.append((depth, np.ones((size, size), bool), K, look(c + np.asarray(d, np.float64), [-a for a in d], right_of(d)), 1))
    return frames


# ------------------------------------------------------------------------------------------------ a, b: cube cases and seams
CUBE_SEEDS = (1, 5)                        # 249 rows each, all 254 together (seeds 0 .. 7 keep 246 .. 251 each)


def cubes(seed):
    return make("cubes_seed%d" % seed, (0, 0, 0), (2, 2, 2), 8, six_noisy_views(centre_of((0, 0, 0), (2, 2, 2), VOXEL), 48, seed))


def cubes_plus(seed=CUBE_SEEDS[0]):
    """a. with its first frame once more: what a second extraction must show (section j)"""
    c = cubes(seed)
    return dict(c, name="cubes_seed%d_plus" % seed, frames=c["frames"] + [c["frames"][0]])


def seams():
    """The same six views of the block corner at voxel (16, 16, 16) of a 3 x 3 x 3 grid, 2.5 pixels per voxel: frames and band reach
    voxels 2 .. 30, so blocks 0 and 1 of every axis are stamped and block 2 never is; the surface lies in the stamped blocks next
    to it.  (One pixel per voxel about the grid's centre stamps all 27 blocks: the band 24 +- 10 leaves block 1 on both sides.)"""
    return make("seams", (0, 0, 0), (3, 3, 3), 8, six_noisy_views(np.full(3, 16 * VOXEL), 64, 7, f=320))


# ------------------------------------------------------------------------------------------------ c: exact zeros, sdf == -trunc
X0 = 8                                     # the 1000 mm plane of the +x camera is the voxel plane x = X0


def along_x(nb, W, H, x0=X0, z_m=1.0, b0=(0, 0, 0)):
    """(K, pose): a camera on the -x side looking along +x whose depth z_m is exactly the voxel plane x0 and whose pixel (i, j) is
    exactly the voxel (x0, y, z) = (y0 + j - (W + 1) // 2, z0 + i - (H + 1) // 2) about the grid's middle: 128 pixels per voxel-metre
    at z_m, principal point (W / 2, H / 2).  For an odd W every u is a whole number + 0.5 before it is rounded: half up by the rule."""
    y0, z0 = b0[1] * 16 + nb[1] * 8, b0[2] * 16 + nb[2] * 8
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = [[0, 0, 1], [1, 0, 0], [0, 1, 0]]          # camera x -> world y, camera y -> world z, optical axis -> world x
    pose[:3, 3] = [(b0[0] * 16 + x0) * VOXEL - z_m, y0 * VOXEL, z0 * VOXEL]
    return intrinsics(128 * z_m, 128 * z_m, W / 2, H / 2), pose


def zeros(times=4):
    """trunc = voxel.  Depth 1000 mm in separate 4 x 4 pixel patches, 996 mm between them: behind a 1000 mm pixel voxel X0 holds
    tsdf == 0 and X0 + 1 holds -1 (sdf == -trunc, kept); behind a 996 mm pixel X0 holds -0.512 and X0 + 1 is out of the band.  The zero
    voxel at a patch's last corner has negative neighbours along +y, +z and across: the cube at X0 - 1 (table row 100) gets two
    vertices at that voxel's own position, both in its first triangle."""
    W = H = 40
    K, pose = along_x((2, 2, 2), W, H)
    i, j = np.mgrid[0:H, 0:W]
    depth = np.where(((i // 4) % 2 == 0) & ((j // 4) % 2 == 0), 1000, 996).astype(np.uint16)
    return make("zeros" if times == 4 else "minus_one", (0, 0, 0), (2, 2, 2), 1, [(depth, np.ones((H, W), bool), K, pose, 1)] * times)


# ------------------------------------------------------------------------------------------------ d: surface through the grid's faces
def face(n):
    """One block, trunc 4 voxels, a noisy plane half a voxel inside face n (AXES order: n = 0 the high x face seen from outside it, ...):
    the band's near samples leave the grid through that face and the surface lies in the outermost layer of cubes."""
    d = np.asarray(AXES[n], np.float64)
    rng = np.random.default_rng(100 + n)
    c = centre_of((0, 0, 0), (1, 1, 1), VOXEL)
    plane = c + d * (6.5 if d.sum() > 0 else 7.5) * VOXEL     # at 14.5 voxels (between the last two), or at 0.5 on a low face
    W = 48
    depth = (1000 + rng.integers(-2, 3, (W, W))).astype(np.uint16)
    frame = (depth, np.ones((W, W), bool), intrinsics(128, 128, W / 2, W / 2), look(plane + d, -d, right_of(AXES[n])), 1)
    return make("face_%d" % n, (0, 0, 0), (1, 1, 1), 4, [frame] * 4)


# ------------------------------------------------------------------------------------------------ e: camera inside the volume
def inside():
    """The camera at the grid centre looking along a rotated direction at a noisy shell 150 .. 300 mm away: the blocks it stamps hold
    voxels behind the camera (zc <= 0) and voxels a fraction of a voxel in front of it (u, v huge or infinite)."""
    rng = np.random.default_rng(5)
    nb = (3, 3, 3)
    W = H = 64
    c = centre_of((0, 0, 0), nb, VOXEL) + np.array([0.3, 0.2, 0.1]) * VOXEL
    depth = rng.integers(150, 301, (H, W)).astype(np.uint16)
    frame = (depth, np.ones((H, W), bool), intrinsics(40, 40, W / 2, H / 2), look(c, (0.48, 0.6, 0.64), (0.8, -0.6, 0.1)), 1)
    return make("inside", (0, 0, 0), nb, 8, [frame] * 4)


def on_plane():
    """The +x camera ON the voxel plane x = 0 of the grid, 8 voxels before a noisy wall: that plane's voxels have zc == 0 exactly, so
    (fx xc) / zc is +-inf, or NaN on the optical axis, and none of them may be written."""
    W = H = 24
    K, pose = along_x((2, 2, 2), W, H, z_m=8 * VOXEL)
    depth = np.random.default_rng(9).integers(60, 66, (H, W)).astype(np.uint16)
    return make("on_plane", (0, 0, 0), (2, 2, 2), 2, [(depth, np.ones((H, W), bool), K, pose, 1)] * 4)


# ------------------------------------------------------------------------------------------------ f: awkward camera and grid
def awkward(where):
    """fx != fy, fy < 0, the principal point outside the frame, a general rotation, voxel 0.002; the grid 40 m out (blocks around
    +-1250) or straddling the origin with a negative first block on every axis."""
    b0 = dict(far=(1249, -1251, 624), origin=(-1, -2, -1))[where]
    nb = (3, 3, 3)
    voxel = 0.002
    W, H = 64, 48
    K = intrinsics(97.25, -143.5, -7.5, H - 0.25)
    rng = np.random.default_rng(11 if where == "far" else 12)
    ang = np.array([0.37, -0.81, 1.23])
    cx, cy, cz = np.cos(ang)
    sx, sy, sz = np.sin(ang)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ray = np.array([(W / 2 + 7.5) / 97.25, (H / 2 - (H - 0.25)) / -143.5, 1.0])      # the middle pixel's ray at depth 1
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = centre_of(b0, nb, voxel) - R @ ray * 0.5
    depth = (500 + rng.integers(-6, 7, (H, W))).astype(np.uint16)
    return make("awkward_" + where, b0, nb, 8, [(depth, np.ones((H, W), bool), K, T.astype(np.float32), 1)] * 4, voxel=voxel, margin=3)


# ------------------------------------------------------------------------------------------------ g: band ratios
BAND_RATIOS = (1.0, 2.5, 3.5, 8.0)
BAND_STEPS = (1, 2, 4, 8)                  # round half to even


def band(ratio):
    nb = (2, 2, 2)
    W = 56
    d = np.array([0.36, 0.48, 0.8])
    c = centre_of((0, 0, 0), nb, VOXEL)
    # the plane 3.5 voxels short of the middle (a corner of all eight blocks): only the band's last samples reach the eighth block
    frame = (np.full((W, W), 1000, np.uint16), np.ones((W, W), bool), intrinsics(128, 128, W / 2, W / 2),
             look(c - d * (1 + 3.5 * VOXEL), d, (0.8, -0.6, 0)), 1)
    return make("band_%g" % ratio, (0, 0, 0), nb, ratio, [frame] * 4)


# ------------------------------------------------------------------------------------------------ h: erosion and frame shapes
SIZES = [(1, 1), (5, 3), (63, 31), (64, 32), (65, 33), (129, 70), (7, 300)]              # (W, H)
ALL_K = (1, 2, 3, 8, 20, 31, 32)
ERODE = [(s, k) for s in SIZES for k in (ALL_K if s in ((65, 33), (129, 70)) else (1, 2, 32))]
SPECIAL_DEPTHS = (0, 1, 2999, 3000, 3001, 65535)


def holes_of(W, H, k):
    """One-pixel holes at every k: columns 0, 63, 64, W - 1 and k // 2, k - 1 - k // 2 pixels inside either border, rows 0, 31, 32, H - 1
    and the same insets (those that lie in the frame), paired in order so that every such row and every such column carries one."""
    a, b = k // 2, k - 1 - k // 2
    cols = sorted({c for c in (0, 63, 64, W - 1, a, b, W - 1 - a, W - 1 - b) if 0 <= c < W})
    rows = sorted({r for r in (0, 31, 32, H - 1, a, b, H - 1 - a, H - 1 - b) if 0 <= r < H})
    return [(rows[n % len(rows)], cols[n % len(cols)]) for n in range(max(len(rows), len(cols)))]


def erode_masks(W, H, k):
    """The masks of one (size, k), one frame each.  k <= 8: ONE mask, random at density 0.97 (a k x k window of it survives with
    probability 0.97^64 = 0.14 at k = 8) with every hole of holes_of.  k >= 20: a random mask leaves no window (0.97^400 = 5e-6)
    and the holes together erode most frames whole, so there is one otherwise all-set mask PER hole: each hole's k x k footprint
    is cut out of its own frame, the voxel behind a pixel counts the frames in which the pixel survived, and a hole read through
    the left, right, top or bottom halo of a tile shows on its own.  The 1 x 1 frame keeps its pixel."""
    if (W, H) == (1, 1):
        return [np.ones((1, 1), bool)]
    holes = holes_of(W, H, k)
    if k <= 8:
        mask = np.random.default_rng(1000 * W + 10 * H + k).random((H, W)) < 0.97
        for r, c in holes:
            mask[r, c] = False
        return [mask]
    masks = []
    for r, c in holes:
        masks.append(np.ones((H, W), bool))
        masks[-1][r, c] = False
    return masks


def special_pixels(W, H):
    """where SPECIAL_DEPTHS sit: spread over the frame's flat index (frames of fewer than 12 pixels carry none)"""
    n = W * H
    return [] if n < 12 else [divmod((2 * q + 1) * n // 12, W) for q in range(6)]


def erosion(W, H, k, full=False):
    """trunc = voxel, the camera along +x with the 1000 mm plane ON voxel plane X0 and pixel (i, j) exactly one voxel of that plane
    (pixel_voxel): a valid pixel at 1000 mm adds weight 1 there per frame, an invalid one nothing.  One frame per mask of erode_masks."""
    nb = (1, (W + 15) // 16 + 1, (H + 15) // 16 + 1)
    K, pose = along_x(nb, W, H)
    depth = np.full((H, W), 1000, np.uint16)
    for (r, c), d in zip(special_pixels(W, H), SPECIAL_DEPTHS):
        depth[r, c] = d
    masks = [np.ones((H, W), bool)] if full else erode_masks(W, H, k)
    return make("erode_%dx%d_k%d%s" % (W, H, k, "_full" if full else ""), (0, 0, 0), nb, 1, [(depth, m, K, pose, k) for m in masks])


def three_metres():
    """the volume 3 m from the camera, 384 pixels per unit of x / z so that pixels are voxels again; depth 3000 mm everywhere but single
    pixels at 2999, 3001 and 65535 mm"""
    W, H = 24, 16
    nb = (1, 3, 2)
    K, pose = along_x(nb, W, H, z_m=3.0)
    depth = np.full((H, W), 3000, np.uint16)
    for (r, c), d in THREE_M_PIXELS.items():
        depth[r, c] = d
    return make("three_metres", (0, 0, 0), nb, 1, [(depth, np.ones((H, W), bool), K, pose, 1)])


THREE_M_PIXELS = {(4, 5): 2999, (4, 9): 3001, (9, 13): 65535, (11, 3): 0}


def pixel_voxel(c, r, col, x0=X0):
    """local (z, y, x) of the voxel that pixel (r, col) of an along_x frame of case c is"""
    W, H = c["frames"][0][0].shape[1], c["frames"][0][0].shape[0]
    return (c["nb"][2] * 8 + r - (H + 1) // 2, c["nb"][1] * 8 + col - (W + 1) // 2, x0)


# ------------------------------------------------------------------------------------------------ i: many blocks in one frame
def many_blocks():
    """72 x 72 x 1 blocks (170 MB of voxel state), one frame from 2.9 m above with a wide lens: more blocks stamped in one frame than
    k_integrate launches workgroups (16 per CU), so its grid-stride loop runs.  Blocks and voxels only."""
    nb = (72, 72, 1)
    W = H = 176
    c = centre_of((0, 0, 0), nb, VOXEL)
    rng = np.random.default_rng(3)
    depth = (2900 + rng.integers(-8, 9, (H, W))).astype(np.uint16)
    frame = (depth, np.ones((H, W), bool), intrinsics(52, 52, W / 2, H / 2), look(c + np.array([0, 0, 2.9]), (0, 0, -1), (1, 0, 0)), 1)
    return make("many_blocks", (0, 0, 0), nb, 4, [frame], mesh=False)


# ------------------------------------------------------------------------------------------------ j: frames of different sizes
def mixed_frames():
    """a 129 x 70 frame, a 5 x 3 frame, the 129 x 70 frame again into one volume: the library's frame buffers are reused, not reallocated"""
    big = erosion(129, 70, 3)
    K, pose = along_x(big["nb"], 5, 3)
    small = (np.array([[1000, 1001, 0, 999, 1000], [1002, 1000, 1000, 1000, 998], [1000, 1000, 997, 1000, 1000]], np.uint16), np.ones((3, 5), bool), K, pose, 2)
    return dict(big, name="mixed_frames", frames=[big["frames"][0], small, big["frames"][0]])


# ------------------------------------------------------------------------------------------------ k: touch words
TOUCH_NBX = (1, 3, 5, 9)                   # nx = 16, 48, 80, 144: 1, 2, 3, 5 words per row, the last one half filled
TOUCH_ARGS = [(3.0, 0.002), (3.0, 0.0), (3.0, -0.004), (1.0, 0.002), (1.0, 0.0), (1.0, -0.004)]


def touch(nbx):
    """A noisy x-z plane through the middle of a grid nbx blocks long, seen along +y three times, twice of them through a mask of the
    frame's upper half only (weights 3 and 1, so the two thresholds differ): every x of the rows about the plane is observed and
    the rows' bits are mixed right up to the last, partly filled word.  trunc 4 voxels: a one-block axis cannot hold bounds padded
    by 8."""
    nb = (nbx, 1, 1)
    W, H = nbx * 16 + 16, 32
    rng = np.random.default_rng(40 + nbx)
    c = centre_of((0, 0, 0), nb, VOXEL)
    depth = (1000 + rng.integers(-15, 16, (H, W))).astype(np.uint16)
    upper = np.arange(H)[:, None] * np.ones(W, int) < H // 2
    K, pose = intrinsics(128, 128, W / 2, H / 2), look(c - np.array([0, 1.0, 0]), (0, 1, 0), (1, 0, 0))
    return make("touch_%d" % nbx, (0, 0, 0), nb, 4, [(depth, upper, K, pose, 1), (depth, np.ones((H, W), bool), K, pose, 1), (depth, upper, K, pose, 1)])


# ------------------------------------------------------------------------------------------------ registry
def _builders():
    b = {}
    for s in CUBE_SEEDS:
        b["cubes_seed%d" % s] = functools.partial(cubes, s)
    b["cubes_seed%d_plus" % CUBE_SEEDS[0]] = cubes_plus
    b["seams"] = seams
    b["zeros"] = zeros
    b["minus_one"] = functools.partial(zeros, 1)
    for n in range(6):
        b["face_%d" % n] = functools.partial(face, n)
    b["inside"] = inside
    b["on_plane"] = on_plane
    b["awkward_far"] = functools.partial(awkward, "far")
    b["awkward_origin"] = functools.partial(awkward, "origin")
    for r in BAND_RATIOS:
        b["band_%g" % r] = functools.partial(band, r)
    for (W, H), k in ERODE:
        b["erode_%dx%d_k%d" % (W, H, k)] = functools.partial(erosion, W, H, k)
    b["erode_5x3_k32_full"] = functools.partial(erosion, 5, 3, 32, True)
    b["three_metres"] = three_metres
    b["many_blocks"] = many_blocks
    b["mixed_frames"] = mixed_frames
    for n in TOUCH_NBX:
        b["touch_%d" % n] = functools.partial(touch, n)
    return b


BUILDERS = _builders()
ERODE_NAMES = ["erode_%dx%d_k%d" % (W, H, k) for (W, H), k in ERODE]
MESH_NAMES = [n for n in BUILDERS if not n.startswith("erode_") and n not in ("many_blocks", "three_metres")]


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert c["name"] == name
    for f in c["frames"]:
        for a in f[:4]:
            a.setflags(write=False)
    return c


def fuse(c, rules=(), probe=False, frames=None):
    """the restatement's volume of a case (a fresh one: with wrong rules, with the probe, or of its first `frames` frames)"""
    vol = tsdf_ref.Volume(c["bounds"], c["voxel"], c["trunc"], rules=rules, probe=probe)
    for f in c["frames"][:frames]:
        vol.integrate(*f)
    return vol


def outputs(c, vol, swap_row=None):
    """everything the GPU test compares, from a restated volume: dict(blocks, tsdf, w, and with c["mesh"]: verts, tris, clean (None when
    there is no surface), solid, touch = {(threshold, contact): words})"""
    out = dict(blocks=vol.active_blocks())
    out["tsdf"], out["w"] = vol.block_voxels()
    if c["mesh"]:
        out["verts"], out["tris"] = vol.marching_cubes(WEIGHT_THRESHOLD)
        out["clean"] = tsdf_ref.clean(out["verts"], out["tris"], c["bounds"], 0.02) if len(out["tris"]) else None
        out["solid"] = sdfphys_ref.solid_points(vol, WEIGHT_THRESHOLD)
        out["touch"] = {a: sdfphys_ref.touch_words(vol, *a) for a in (TOUCH_ARGS if c["name"].startswith("touch_") else TOUCH_ARGS[:1])}
    return out


def protect(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            protect(v)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (volume, outputs) of the rule as written: computed once, shared, never written to"""
    c = case(name)
    vol = fuse(c)
    out = outputs(c, vol)
    protect(out)
    for a in (vol.tsdf, vol.w, vol.ever):
        a.setflags(write=False)
    return vol, out


def differs(a, b):
    """do two `outputs` differ in anything compared (floats by their bits)?"""
    def ne(x, y):
        if x is None or y is None:
            return (x is None) != (y is None)
        if isinstance(x, dict):
            return set(x) != set(y) or any(ne(x[k], y[k]) for k in x)
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.shape != y.shape:
            return True
        if x.dtype.kind == "f":
            x, y = x.view("u%d" % x.dtype.itemsize), y.view("u%d" % y.dtype.itemsize)
        return bool((x != y).any())
    return ne(a, b)
