"""tests/masks_ref.py (the numpy restatement of DESIGN.md section 2d) against independent statements of the same rule, and the
host-side pieces of the mask path: PNG forms, the data loader's file handling, the ABI's refusals.  No GPU."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from tests import masks_cases, masks_ref


def _close_triple_loop(src, k):
    H, W = src.shape
    lo = -(k // 2)

    def run(a, use_max):
        out = np.zeros_like(a)
        for i in range(H):
            for j in range(W):
                v = 0 if use_max else 255
                for da in range(lo, lo + k):
                    for db in range(lo, lo + k):
                        u, w = i + da, j + db
                        if 0 <= u < H and 0 <= w < W:
                            v = max(v, a[u, w]) if use_max else min(v, a[u, w])
                out[i, j] = v
        return out
    return run(run(src, True), False)


@pytest.mark.parametrize("shape,k,seed", [((30, 40), 5, 0), ((61, 97), 6, 1), ((30, 40), 50, 2)])
def test_closing_equals_a_direct_triple_loop(shape, k, seed):
    rng = np.random.default_rng(seed)
    src = np.where(rng.random(shape) < 0.02, 255, 0).astype(np.uint8)
    want = _close_triple_loop(src, k)
    assert (masks_ref.close(src, k) == want).all()
    assert (masks_ref.close(src, k, fast=True) == want).all()


def test_closing_hand_vectors():
    src = np.zeros((200, 200), np.uint8)
    src[100, 100] = 255
    out = masks_ref.close(src, 50, fast=True)
    assert np.argwhere(out).tolist() == [[101, 101]]        # an isolated pixel far from every border moves by (+1, +1)
    src = np.zeros((200, 200), np.uint8)
    src[0, 0] = 255
    out = masks_ref.close(src, 50, fast=True)
    # dilation sets rows and columns 0 .. 25; the erosion's window of pixel (i, j) reaches i + 24, so it survives up to 25 - 24 = 1
    assert np.argwhere(out).tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
    src = np.zeros((30, 40), np.uint8)                       # a frame smaller than the window: one pixel fills what its dilation reaches
    src[3, 4] = 255
    out = masks_ref.close(src, 50, fast=True)
    want = np.zeros((30, 40), np.uint8)
    want[:, :] = 255
    # dilated rows 0 .. 28 (3 + 25), columns 0 .. 29 (4 + 25); erosion of (i, j) sees rows up to i + 24 and columns up to j + 24
    want[5:, :] = 0
    want[:, 6:] = 0
    assert (out == want).all() and (out == masks_ref.close(src, 50)).all()


def test_label_partition_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    mask = (rng.integers(0, 4, (48, 75)) * (rng.random((48, 75)) < 0.7)).astype(np.uint8)
    for m in (mask, masks_cases.serpentine(), masks_cases.checkerboard(), masks_cases.arms()):
        keys = masks_ref.components(m)
        assert (keys == masks_ref.components_fast(m)).all()
        assert ((keys == 0xffffffff) == (m == 0)).all()
        for l in np.unique(m[m != 0]):
            lab, n = ndi.label(m == l, structure=np.ones((3, 3)))
            ks = keys[m == l]
            assert len(np.unique(ks)) == n
            for c in range(1, n + 1):                         # one key per scipy component, and it is its first pixel
                sel = lab == c
                assert len(np.unique(keys[sel])) == 1 and keys[sel][0] == np.flatnonzero(sel.ravel())[0]
    assert len(np.unique(masks_ref.components(masks_cases.serpentine()))) == 2     # one component + background
    assert len(np.unique(masks_ref.components(masks_cases.arms()))) == 2
    assert len(np.unique(masks_ref.components(masks_cases.checkerboard()))) == 2   # one per label, through the diagonals


def test_integer_sum_mean_equals_the_mean_of_the_points():
    """Against the fp64 mean of the points back-projected with z = d16 / 1000 in fp64: 1e-12 relative.  Against points whose z went
    through float32 first (the scene-bound rule's staging) the means differ by about 1e-9 relative, the float32 rounding of each z
    averaged over the component: asserted below as a bound of 1e-7, and listed in DESIGN.md section 9 as a fork."""
    rng = np.random.default_rng(4)
    d16 = masks_cases.depth_for((60, 80), 5)
    T = masks_cases.SCENE_POSE
    K = np.array([[70.0, 0, 39.5], [0, 72.0, 29.5], [0, 0, 1]])
    mask = np.zeros((60, 80), np.uint8)
    mask[10:40, 20:70] = 1
    mask[rng.random((60, 80)) < 0.1] = 0
    keys = masks_ref.components(mask)
    stats = masks_ref.component_stats(keys, d16)
    pts = masks_ref.world_points(d16, T, K, z_f32=False)
    pts32 = masks_ref.world_points(d16, T, K)
    for key, st in stats.items():
        sel = (keys == key) & (d16 > 0)
        if st[1] == 0:
            continue
        want = pts[sel].mean(0)
        got = masks_ref.mean_world_point(st, T, K)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(got - pts32[sel].mean(0)).max() <= 1e-7 * np.abs(want).max()
        assert st[1] == sel.sum()


@pytest.mark.parametrize("name", sorted(masks_cases.prune_cases()))
def test_prune_quirks(name):
    c = masks_cases.prune_cases()[name]
    dup = masks_ref.duplicate_prune(c["mask"], c["d16"], c["T"], c["K"], c["centre"])
    dis = masks_ref.disconnected_prune(c["mask"])
    for (i, j), l in c["dup"].items():
        assert dup[i, j] == l, ("duplicate", name, i, j)
    for (i, j), l in c["dis"].items():
        assert dis[i, j] == l, ("disconnected", name, i, j)
    for out in (dup, dis):                                   # a kept pixel keeps its label; nothing appears
        assert ((out == 0) | (out == c["mask"])).all()


def test_scene_frames_stay_clear_of_the_planes():
    """The seeds of the GPU comparison: no compared coordinate within 1e-9 of a plane, both sides of every reachable plane hit.
    (zmin = -100 lies below the -0.40 cut, so no set pixel can depend on it.)"""
    for (w, h, seed) in [(200, 150, 11), (40, 30, 12), (130, 70, 13), (1280, 720, 14)]:
        d16, K = masks_cases.scene_frame(w, h, seed)
        assert masks_ref.plane_margin(d16, masks_cases.SCENE_POSE, K, masks_cases.SCENE_BOUNDS) > 1e-9
        if w >= 130:
            p = masks_ref.world_points(d16, masks_cases.SCENE_POSE, K)[d16 > 0]
            b = masks_cases.SCENE_BOUNDS
            for a, s in [(0, 0), (0, 1), (1, 0), (1, 1), (2, 1)]:
                assert (p[:, a] < b[s, a]).any() and (p[:, a] > b[s, a]).any(), (w, a, s)
            assert (p[:, 2] < -0.40).any() and (p[:, 2] > -0.40).any()
            raw = masks_ref.scene_bounds_raw(d16, masks_cases.SCENE_POSE, K, b)
            assert 0.05 < (raw == 255).mean() < 0.95


def test_depth_u16_is_the_float16_product():
    d = np.array([0.0, 0.5, 1.2344, 2.0, 65.0], np.float16)
    assert masks_ref.depth_u16(d).tolist() == (d * np.float16(1000)).astype(np.uint16).tolist()
    from dream2real_amd.segmentation import depth_to_u16
    assert (depth_to_u16(d) == masks_ref.depth_u16(d)).all()


# ------------------------------------------------------------------------------------------------ files

def test_png_grey_rgba_and_16_bit_round_trip_through_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from dream2real_amd import _lib
    rng = np.random.default_rng(6)
    for shape in [(31, 47), (31, 47, 3), (31, 47, 4)]:
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        p = str(tmp_path / "a.png")
        _lib.png_write_channels(a, p)
        b = np.asarray(Image.open(p))
        assert b.shape == a.shape and (a == b).all()
        assert _lib.png_info(p) == (47, 31, 1 if a.ndim == 2 else shape[2], 8)
    d = rng.integers(0, 65536, (33, 21), dtype=np.uint16)
    p = str(tmp_path / "d.png")
    Image.fromarray(d).save(p)
    assert _lib.png_info(p) == (21, 33, 1, 16) and (_lib.png_read_grey(p, 16) == d).all()
    with pytest.raises(_lib.D2RError, match="8-bit grey"):
        _lib.png_read_grey(p, 8)
    g = rng.integers(0, 256, (33, 21), dtype=np.uint8)
    _lib.png_write_channels(g, p)
    assert (_lib.png_read_grey(p, 8) == g).all()
    with pytest.raises(_lib.D2RError, match="unsupported PNG"):      # the RGB reader still refuses 16-bit files
        Image.fromarray(d).save(p)
        _lib.png_read_rgb(p)


def _scan_dir(tmp_path, n=3, w=24, h=16):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    os.makedirs(tmp_path / "images")
    os.makedirs(tmp_path / "depth")
    rgbs = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    d16 = rng.integers(0, 4000, (n, h, w)).astype(np.uint16)
    poses = np.stack([np.eye(4) + 0.01 * k for k in range(n)])
    np.savetxt(tmp_path / "poses.txt", poses.reshape(n, 16), delimiter=" ")
    for k in range(n):
        Image.fromarray(rgbs[k]).save(tmp_path / "images" / ("rgb_%04d.png" % k))
        Image.fromarray(d16[k]).save(tmp_path / "depth" / ("depth_%04d.png" % k))
    cfg = types.SimpleNamespace(data_dir=str(tmp_path), width=w, height=h)
    return cfg, rgbs, d16, poses


def test_load_rgbds_and_the_cache_branches(tmp_path):
    from dream2real_amd import _lib, data_loader, segmentation
    cfg, rgbs, d16, poses = _scan_dir(tmp_path)
    dl = data_loader.d2r_dataloader(cfg, ctx=None)
    rgb, depth, T = dl.load_rgbds()
    assert rgb.dtype == np.uint8 and (rgb == rgbs).all()
    assert depth.dtype == np.float16 and (depth == d16.astype(np.float16) / np.float16(1000)).all()
    assert T.dtype == np.float32 and T.shape == (3, 4, 4) and np.allclose(T, poses)
    masks = np.random.default_rng(8).integers(0, 2, d16.shape).astype(np.uint8) * 255
    for k in range(3):
        _lib.png_write_channels(masks[k], str(tmp_path / "images" / ("dynamic_mask_rgb_%04d.png" % k)))
    bounds = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
    got = dl.remove_background(np.eye(3), bounds, use_cache=True)
    assert got.dtype == np.uint8 and (got == masks).all() and bounds[0][2] == 0.0
    os.makedirs(tmp_path / "XMem_masks")
    labels = np.random.default_rng(9).integers(0, 256, d16.shape).astype(np.uint8)
    for k in range(3):
        _lib.png_write_channels(labels[k], str(tmp_path / "XMem_masks" / ("rgb_%04d.png" % k)))
    assert (segmentation.load_cached_masks(str(tmp_path), 3) == labels).all()


def test_the_abi_refuses_bad_arguments_before_touching_a_device():
    from dream2real_amd import _lib
    lib = _lib.load()
    d = np.zeros((1, 4, 4), np.uint16)
    m = np.zeros((1, 4, 4), np.uint8)
    T = np.eye(4, dtype=np.float32).reshape(1, 16)
    K = np.eye(3).reshape(9)
    b = np.zeros(6)
    out = np.zeros((1, 4, 4), np.uint8)
    u = C.c_uint32
    ptr = _lib.ptr

    def err():
        return lib.d2r_last_error(None).decode()
    assert lib.d2r_scene_bound_masks(None, ptr(d), u(1), u(4), u(4), ptr(T), ptr(K), ptr(b), u(50), ptr(out), None) == -1 and "null" in err()
    assert lib.d2r_masks_prune(None, C.c_int(0), ptr(m), ptr(d), None, u(1), u(4), u(4), ptr(T), ptr(K), ptr(b), u(200), ptr(out)) == -1
    assert lib.d2r_masks_components(None, ptr(m), ptr(d), u(4), u(4), None, None, None) == -1
    assert lib.d2r_masks_lut(None, ptr(m), None, u(1), u(4), u(4), None, ptr(out), None) == -1
    assert lib.d2r_masks_get_timing(None, None) == -1
    assert lib.d2r_abi_version() == 10
    with pytest.raises(ValueError):
        _lib.scene_bound_masks(None, d[0], T, K, b)             # [h, w] where [n, h, w] is expected
    with pytest.raises(ValueError):
        _lib.masks_prune(None, 1, m, depth_u16=np.zeros((1, 5, 4), np.uint16))
    with pytest.raises(ValueError):
        _lib.masks_lut(None, m, np.zeros(255, np.uint8))
