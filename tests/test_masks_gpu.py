"""masks.hip on the GPU against tests/masks_ref.py, bit for bit and over whole arrays: the scene-bound masks before and after the
closing, the labelling and its integer statistics through the parity hook, both pruning rules, the LUT pass, and the way from a
raw label image to the physics meshes."""
import os

import numpy as np
import pytest

from tests import masks_cases, masks_ref, tsdf_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dream2real_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib():
    from dream2real_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ scene-bound masks

@pytest.mark.parametrize("w,h,seed,windows", [(200, 150, 11, (1, 2, 49, 50, 64)), (40, 30, 12, (1, 2, 49, 50, 64)), (130, 70, 13, (1, 2, 49, 50, 64)),
                                              (1280, 720, 14, (50,))])
def test_scene_bound_masks_equal_the_rule(ctx, lib, w, h, seed, windows):
    d16, K = masks_cases.scene_frame(w, h, seed)
    d2 = d16.copy()
    d2[: h // 2] = 0                                        # a second frame with another pose: frames of a batch are independent
    T2 = masks_cases.look_at(np.array([0.7, -0.3, 0.8]), np.array([0.1, 0.2, -0.1]))
    depth = np.stack([d16, d2])
    poses = np.stack([masks_cases.SCENE_POSE, T2])
    bounds = masks_cases.SCENE_BOUNDS.copy()
    raws = [masks_ref.scene_bounds_raw(depth[f], poses[f], K, bounds) for f in range(2)]
    assert masks_ref.plane_margin(d2, T2, K, bounds) > 1e-9
    for k in windows:
        out, raw = lib.scene_bound_masks(ctx, depth, poses, K, bounds, k, return_raw=True)
        for f in range(2):
            assert (raw[f] == raws[f]).all(), ("raw", k, f, int((raw[f] != raws[f]).sum()))
            want = masks_ref.close(raws[f], k, fast=True)
            assert (out[f] == want).all(), ("closed", k, f, int((out[f] != want).sum()))
    assert (bounds == masks_cases.SCENE_BOUNDS).all()


def test_closing_hand_vectors_on_the_gpu(ctx, lib):
    """An all-zero-depth frame gives an empty mask; the closing itself is driven through depth that sets chosen pixels."""
    K = np.array([[100.0, 0, 99.5], [0, 100.0, 99.5], [0, 0, 1]])
    d = np.zeros((200, 200), np.uint16)
    d[100, 100] = 1000                                      # identity pose: the point (0.005, 0.005, 1) lies above zmax = 0.5
    d[0, 0] = 1000
    out, raw = lib.scene_bound_masks(ctx, d[None], np.eye(4, dtype=np.float32)[None], K, [[-9, -9, -9], [9, 9, 0.5]], 50, return_raw=True)
    assert np.argwhere(raw[0]).tolist() == [[0, 0], [100, 100]]
    assert np.argwhere(out[0]).tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [101, 101]]


# ------------------------------------------------------------------------------------------------ components

def _check_components(ctx, lib, mask, d16, keys_want=None):
    keys, area, sums = lib.masks_components(ctx, mask, d16)
    if keys_want is None:
        keys_want = masks_ref.components(mask)
    assert (keys == keys_want).all(), int((keys != keys_want).sum())
    stats = masks_ref.component_stats(keys_want, d16)
    area_want, sums_want = np.zeros(mask.shape, np.uint32).ravel(), np.zeros(mask.shape + (4,), np.uint64).reshape(-1, 4)
    for key, st in stats.items():
        area_want[key] = st[0]
        sums_want[key] = st[1:]
    assert (area.ravel() == area_want).all() and (sums.reshape(-1, 4) == sums_want).all()
    return len(stats)


@pytest.mark.parametrize("name", ["serpentine", "checkerboard", "arms", "many_labels", "1x1", "1x300", "300x1", "random"])
def test_components_equal_the_flood_fill(ctx, lib, name):
    if name == "1x1":
        mask = np.array([[5]], np.uint8)
    elif name == "1x300":
        mask = (np.arange(300)[None] // 7 % 3).astype(np.uint8)
    elif name == "300x1":
        mask = (np.arange(300)[:, None] // 5 % 2).astype(np.uint8) * 9
    elif name == "random":
        rng = np.random.default_rng(21)
        mask = (rng.integers(1, 4, (75, 131)) * (rng.random((75, 131)) < 0.62)).astype(np.uint8)
    else:
        mask = getattr(masks_cases, name)()
    if name == "many_labels":
        assert len(np.unique(mask)) - 1 == 254 and mask.max() == 254
    n = _check_components(ctx, lib, mask, masks_cases.depth_for(mask.shape, 22))
    assert n == {"serpentine": 1, "checkerboard": 2, "arms": 1, "1x1": 1, "many_labels": 520}.get(name, n)


def test_a_frame_filling_component_at_1280x720(ctx, lib):
    mask = np.full((720, 1280), 3, np.uint8)
    d16 = masks_cases.depth_for(mask.shape, 23)
    d16[:, :7] = 65535                                       # the largest products the sums meet
    _check_components(ctx, lib, mask, d16, keys_want=np.zeros(mask.shape, np.uint32))


# ------------------------------------------------------------------------------------------------ pruning

def test_both_prune_rules_on_the_quirk_cases(ctx, lib):
    cases = masks_cases.prune_cases()
    names = sorted(cases)
    masks = np.stack([cases[n]["mask"] for n in names])
    d16 = np.stack([cases[n]["d16"] for n in names])
    poses = np.stack([cases[n]["T"] for n in names])
    rng = np.random.default_rng(31)
    oob = np.where(rng.random(masks.shape) < 0.05, 255, 0).astype(np.uint8)
    oob[0, 0, 0] = 7                                         # only 255 overwrites
    for o in (oob, None):
        dup = lib.masks_prune(ctx, 0, masks, d16, o, poses, masks_cases.K, masks_cases.CENTRE)
        dis = lib.masks_prune(ctx, 1, masks, oob=o)
        for f, n in enumerate(names):
            c = cases[n]
            want_dup = masks_ref.duplicate_prune(c["mask"], c["d16"], c["T"], c["K"], c["centre"])
            want_dis = masks_ref.disconnected_prune(c["mask"])
            if o is not None:
                want_dup, want_dis = masks_ref.refine(c["mask"], o[f], want_dup), masks_ref.refine(c["mask"], o[f], want_dis)
            else:
                for (i, j), l in c["dup"].items():
                    assert dup[f, i, j] == l, (n, i, j)
                for (i, j), l in c["dis"].items():
                    assert dis[f, i, j] == l, (n, i, j)
            assert (dup[f] == want_dup).all(), ("duplicate", n)
            assert (dis[f] == want_dis).all(), ("disconnected", n)


def test_both_prune_rules_with_254_labels(ctx, lib):
    """Every label 1 .. 254 has two or three 16-pixel components: with the area rule at 10 each label keeps exactly one (the per-label
    slots up to 254 are all in use); at 200 every label disappears."""
    mask = masks_cases.many_labels()
    assert len(np.unique(mask)) - 1 == 254
    d16 = masks_cases.depth_for(mask.shape, 24)
    K = np.array([[180.0, 0, 99.5], [0, 180.0, 32.0], [0, 0, 1]])
    T = masks_cases.look_at(np.array([0.2, -0.4, 0.6]), np.array([0.0, 0.1, 0.0]))
    centre = np.array([0.05, 0.1, 0.0])
    for min_area in (10, 200):
        dup = lib.masks_prune(ctx, 0, mask[None], d16[None], None, T[None], K, centre, min_area=min_area)[0]
        dis = lib.masks_prune(ctx, 1, mask[None], min_area=min_area)[0]
        assert (dup == masks_ref.duplicate_prune(mask, d16, T, K, centre, min_area=min_area)).all(), min_area
        assert (dis == masks_ref.disconnected_prune(mask, min_area=min_area)).all(), min_area
        kept = 254 if min_area == 10 else 0
        assert len(np.unique(dup)) - 1 == kept and len(np.unique(dis)) - 1 == kept
        if kept:
            assert (dup != dis).any()                          # nearest and last are not the same choice


_FIVE = {}


def _five_poses():
    """Five frames of blobs under five poses with their expected results, computed once."""
    if _FIVE:
        return _FIVE
    rng = np.random.default_rng(41)
    h, w = 90, 150
    K = np.array([[140.0, 0, 74.5], [0, 140.0, 44.5], [0, 0, 1]])
    masks, d16, poses = [], [], []
    for f in range(5):
        m = np.zeros((h, w), np.uint8)
        for l in range(1, 6):                                # every label several blobs of random size, some under 200 px
            for _ in range(3):
                bh, bw = rng.integers(6, 28, 2)
                i0, j0 = rng.integers(0, h - bh), rng.integers(0, w - bw)
                m[i0:i0 + bh, j0:j0 + bw] = l
        masks.append(m)
        d16.append(masks_cases.depth_for((h, w), 50 + f))
        poses.append(masks_cases.look_at(np.array([0.3 * f - 0.5, -0.6, 0.7 + 0.1 * f]), np.array([0.1, 0.1 * f, 0.0])))
    masks, d16, poses = np.stack(masks), np.stack(d16), np.stack(poses)
    centre = np.array([0.1, 0.2, 0.0])
    _FIVE.update(masks=masks, d16=d16, poses=poses, K=K, centre=centre,
                 dup=np.stack([masks_ref.duplicate_prune(masks[f], d16[f], poses[f], K, centre) for f in range(5)]),
                 dis=np.stack([masks_ref.disconnected_prune(masks[f]) for f in range(5)]))
    return _FIVE


def test_prune_a_batch_of_five_poses_and_twice_the_same_bytes(ctx, lib):
    b = _five_poses()
    masks, d16, poses, K, centre = b["masks"], b["d16"], b["poses"], b["K"], b["centre"]
    dup = lib.masks_prune(ctx, 0, masks, d16, None, poses, K, centre)
    dis = lib.masks_prune(ctx, 1, masks)
    for f in range(5):
        assert (dup[f] == b["dup"][f]).all(), f
        assert (dis[f] == b["dis"][f]).all(), f
    assert (dup != masks).any() and (dup != dis).any()
    assert lib.masks_prune(ctx, 0, masks, d16, None, poses, K, centre).tobytes() == dup.tobytes()
    up, dev, down = lib.masks_timing(ctx)
    assert up >= 0 and dev > 0 and down >= 0


def test_prune_in_several_passes_over_a_shared_workspace(ctx, lib, monkeypatch):
    """100 frames of 1280 x 720 go through d2r_masks_prune in passes of 26 frames that reuse one labelling workspace.  With the
    workspace budget lowered to two of this batch's frames, five frames take passes of 2, 2 and 1: the later passes' frame offsets
    into the per-label slots, the poses, the out-of-scene masks and the output are all in play."""
    b = _five_poses()
    masks, d16, poses, K, centre = b["masks"], b["d16"], b["poses"], b["K"], b["centre"]
    rng = np.random.default_rng(42)
    oob = np.where(rng.random(masks.shape) < 0.05, 255, 0).astype(np.uint8)
    monkeypatch.setenv("D2R_MASKS_WS_BYTES", str(2 * masks.shape[1] * masks.shape[2] * 44))      # 44 B per pixel: parent + 5 statistics words
    dup = lib.masks_prune(ctx, 0, masks, d16, oob, poses, K, centre)
    dis = lib.masks_prune(ctx, 1, masks, oob=oob)
    for f in range(5):
        assert (dup[f] == masks_ref.refine(masks[f], oob[f], b["dup"][f])).all(), f
        assert (dis[f] == masks_ref.refine(masks[f], oob[f], b["dis"][f])).all(), f


def test_refusals_that_need_a_context(ctx, lib):
    d = np.zeros((1, 4, 4), np.uint16)
    with pytest.raises(lib.D2RError, match="window must be 1 .. 64"):
        lib.scene_bound_masks(ctx, d, np.eye(4)[None], np.eye(3), np.zeros(6), 65)
    with pytest.raises(lib.D2RError, match="window must be 1 .. 64"):
        lib.scene_bound_masks(ctx, d, np.eye(4)[None], np.eye(3), np.zeros(6), 0)
    with pytest.raises(lib.D2RError, match="mode must be"):
        lib.masks_prune(ctx, 2, np.zeros((1, 4, 4), np.uint8))
    with pytest.raises(lib.D2RError, match="null argument"):
        lib.masks_prune(ctx, 0, np.zeros((1, 4, 4), np.uint8))
    import ctypes as C
    rc = lib.load().d2r_masks_prune(ctx.h, C.c_int(1), lib.ptr(d), None, None, C.c_uint32(1), C.c_uint32(65536), C.c_uint32(32768), None, None,
                                    None, C.c_uint32(200), lib.ptr(d))
    assert rc == -4 and b"2^31" in lib.load().d2r_last_error(ctx.h)


def test_lut_and_alpha(ctx, lib):
    rng = np.random.default_rng(61)
    for shape in [(2, 33, 47), (1, 5, 3), (3, 64, 64)]:      # totals that are and are not multiples of four
        masks = rng.integers(0, 256, shape).astype(np.uint8)
        oob = np.where(rng.random(shape) < 0.2, rng.integers(1, 256, shape), 0).astype(np.uint8)
        lut = (rng.random(256) < 0.3).astype(np.uint8) * rng.integers(1, 256, 256).astype(np.uint8)
        out, alpha = lib.masks_lut(ctx, masks, lut, oob, alpha=True)
        want = ((lut[masks] != 0) | (oob != 0)).astype(np.uint8)
        assert (out == want).all() and (alpha == 255 * (1 - want)).all()
        assert (lib.masks_lut(ctx, masks, lut) == (lut[masks] != 0)).all()


# ------------------------------------------------------------------------------------------------ end to end

BLOB_C = np.array([0.12, 0.0])      # in all five views: inside the frame, >= 500 px, apart from the sphere's silhouette


def test_refined_masks_give_the_clean_scene_and_the_same_meshes(ctx, lib, tmp_path):
    """The 12-view sphere-on-a-slab scene with a second blob of the sphere's label (>= 200 px) on the far table in five views:
    refine_masks removes it, and get_phys_models then writes the same .obj bytes as from the clean masks."""
    from dream2real_amd import segmentation
    from dream2real_amd.physics_utils import get_phys_models
    scene = tsdf_scene.make_scene(speckle_r=0.0)
    clean = scene["masks"]
    dirty = clean.copy()
    for f in range(5):
        _, _, pts = tsdf_scene.raycast(scene["cam_poses"][f])      # a 2 cm disc of the table top, 12 cm from the sphere
        blob = (clean[f] == 0) & (scene["depths"][f] > 0) & (np.abs(pts[..., 2]) < 1e-6) & (np.linalg.norm(pts[..., :2] - BLOB_C, axis=-1) < 0.02)
        assert blob.sum() >= 200
        dirty[f][blob] = 1
    assert (dirty != clean).any()
    centre = np.array([0.0, 0.0, 0.03])
    refined = segmentation.refine_masks(dirty, scene["depths"], scene["cam_poses"], scene["intrinsics"], np.zeros_like(clean), centre,
                                        str(tmp_path), ctx=ctx)
    assert (refined == clean).all()
    assert (segmentation.load_cached_masks(str(tmp_path), len(clean)) == clean).all()
    for f in (0, 7):
        assert (segmentation.duplicate_prune(dirty[f], scene["depths"][f], scene["cam_poses"][f], scene["intrinsics"], centre, ctx=ctx) == clean[f]).all()
        assert (segmentation.disconnected_prune(dirty[f], ctx=ctx) == clean[f]).all()
    hull = lambda concave, convex, obj_id: open(convex, "w").write(open(concave).read())
    files = {}
    for name, masks in (("clean", clean), ("refined", refined)):
        out = str(tmp_path / name)
        get_phys_models(scene["depths"], scene["cam_poses"], scene["intrinsics"], masks, 2, scene["bounds"], save_dir=out, use_cache=False,
                        use_phys_tsdf=True, ctx=ctx, convexify=hull)
        files[name] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if f.endswith(".obj")}
    assert files["clean"] and files["clean"] == files["refined"]
