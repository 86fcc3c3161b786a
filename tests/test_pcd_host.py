"""The point-cloud ablation (use_vis_pcds) on the host: PCD files, get_vis_pcds, the numpy render oracle against a
brute-force per-pixel loop, and the wiring of optimise_pose_grid / ImaginationEngine.  CPU only."""
import os
import types

import numpy as np
import pytest

from dream2real_amd import clip_scoring, dream2real
from dream2real_amd import pcd_visual_model as pvm
from tests import pcd_ref


def _cloud(n=57, seed=0):
    r = np.random.default_rng(seed)
    return pvm.PointCloud(r.normal(size=(n, 3)).astype(np.float32), r.integers(0, 256, (n, 3), dtype=np.uint8))


# ------------------------------------------------------------------------------------------------ PCD files

@pytest.mark.parametrize("data", ["ascii", "binary", "binary_compressed"])
def test_pcd_round_trip(tmp_path, data):
    pcd = _cloud()
    pcd.xyz[:10] = pcd.xyz[0]                     # repeats: the LZF encoder emits back references
    path = str(tmp_path / f"c_{data}.pcd")
    pvm.write_point_cloud(path, pcd, data=data)
    got = pvm.read_point_cloud(path)
    np.testing.assert_array_equal(got.xyz, pcd.xyz)
    np.testing.assert_array_equal(got.rgb, pcd.rgb)


def test_default_writer_layout(tmp_path):
    path = str(tmp_path / "c.pcd")
    pvm.write_point_cloud(path, _cloud(5))
    head = open(path, "rb").read().split(b"DATA binary\n")[0].decode()
    assert "FIELDS x y z rgb" in head and "SIZE 4 4 4 4" in head and "TYPE F F F F" in head and "POINTS 5" in head


def test_lzf_codec():
    r = np.random.default_rng(3)
    for raw in (b"", b"a", b"abcabcabcabcabcabc" * 40, bytes(r.integers(0, 4, 5000, dtype=np.uint8)), bytes(700)):
        assert pvm.lzf_decompress(pvm.lzf_compress(raw), len(raw)) == raw
    # a hand-made stream: literal "ab", then a back reference of length 6 at distance 2 (overlapping copy)
    assert pvm.lzf_decompress(bytes([1, 97, 98, (4 << 5) | 0, 1]), 8) == b"abababab"
    with pytest.raises(ValueError):
        pvm.lzf_decompress(bytes([1, 97, 98, (4 << 5) | 0, 9]), 8)


def _write_custom(path, fields, sizes, types, counts, rows, data="binary"):
    n = len(rows)
    hdr = (f"VERSION 0.7\nFIELDS {' '.join(fields)}\nSIZE {' '.join(map(str, sizes))}\nTYPE {' '.join(types)}\n"
           f"COUNT {' '.join(map(str, counts))}\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA {data}\n")
    np_t = {("F", 4): "<f4", ("U", 1): "u1", ("U", 4): "<u4", ("F", 8): "<f8"}
    dt = np.dtype([(f"{f}{k}", np_t[(t, s)]) for f, s, t, c in zip(fields, sizes, types, counts) for k in range(c)])
    if data == "binary":
        body = np.array([tuple(r) for r in rows], dt).tobytes()
    else:
        body = "".join(" ".join(repr(v) for v in r) + "\n" for r in rows).encode()
    open(path, "wb").write(hdr.encode() + body)


@pytest.mark.parametrize("data", ["binary", "ascii"])
def test_accepted_field_layouts(tmp_path, data):
    xyz = np.array([[0.5, -1.25, 2.0], [3.0, 0.125, -0.5]], np.float32)
    rgb = np.array([[10, 200, 255], [0, 1, 2]], np.uint8)
    packed = [int(r) << 16 | int(g) << 8 | int(b) for r, g, b in rgb]
    as_f = [float(np.array([p], "<u4").view("<f4")[0]) for p in packed]
    cases = {
        "rgb_float": (["x", "y", "z", "rgb"], [4] * 4, ["F"] * 4, [1] * 4, [[*x, c] for x, c in zip(xyz.tolist(), as_f)]),
        "rgba_uint": (["x", "y", "z", "rgba"], [4] * 4, ["F", "F", "F", "U"], [1] * 4,
                      [[*x, c | (255 << 24)] for x, c in zip(xyz.tolist(), packed)]),
        "r_g_b": (["x", "y", "z", "r", "g", "b"], [4, 4, 4, 1, 1, 1], ["F"] * 3 + ["U"] * 3, [1] * 6,
                  [[*x, *c] for x, c in zip(xyz.tolist(), rgb.tolist())]),
        "normals_first": (["normal_x", "normal_y", "normal_z", "x", "y", "z", "rgb", "curvature"], [4] * 8, ["F"] * 8, [1] * 8,
                          [[0.0, 0.0, 1.0, *x, c, 0.5] for x, c in zip(xyz.tolist(), as_f)]),
        "count_3_extra": (["x", "y", "z", "rgb", "descriptor"], [4] * 5, ["F"] * 5, [1, 1, 1, 1, 3],
                          [[*x, c, 1.0, 2.0, 3.0] for x, c in zip(xyz.tolist(), as_f)]),
    }
    for name, (f, s, t, c, rows) in cases.items():
        if data == "ascii" and name == "rgb_float":
            continue                               # a float's repr does not survive the NaN payloads packed colours can be
        p = str(tmp_path / f"{name}.pcd")
        _write_custom(p, f, s, t, c, rows, data)
        got = pvm.read_point_cloud(p)
        np.testing.assert_array_equal(got.xyz, xyz, err_msg=name)
        np.testing.assert_array_equal(got.rgb, rgb, err_msg=name)


def test_refusals_name_the_file_and_key(tmp_path):
    p = str(tmp_path / "nocolour.pcd")
    _write_custom(p, ["x", "y", "z", "intensity"], [4] * 4, ["F"] * 4, [1] * 4, [[0.0, 0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="nocolour.pcd.*colour"):
        pvm.read_point_cloud(p)
    p = str(tmp_path / "noz.pcd")
    _write_custom(p, ["x", "y", "rgb"], [4] * 3, ["F"] * 3, [1] * 3, [[0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="noz.pcd.*'z'"):
        pvm.read_point_cloud(p)
    p = str(tmp_path / "bad.pcd")
    open(p, "wb").write(b"FIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nPOINTS 1\nDATA binary_lzma\n")
    with pytest.raises(ValueError, match="bad.pcd.*DATA"):
        pvm.read_point_cloud(p)


# ------------------------------------------------------------------------------------------------ get_vis_pcds

def test_erosion_keeps_the_frame_border():
    m = np.ones((20, 30), bool)
    np.testing.assert_array_equal(pvm.erode_rect(m), m)          # border pixels do not erode
    m[10, 20] = False
    e = pvm.erode_rect(m)
    want = np.ones_like(m)
    want[3:18, 13:28] = False                                     # a 15 x 15 hole centred on the zero
    np.testing.assert_array_equal(e, want)
    m = np.zeros((20, 30), bool)
    m[:, :8] = True                                               # touches the left border: columns 0 .. 8 - 7 - 1 survive
    e = pvm.erode_rect(m)
    np.testing.assert_array_equal(e[:, :1], True)
    assert not e[:, 1:].any()


def _scene(h=24, w=32):
    K = np.array([[30.0, 0, 15.5], [0, 31.0, 11.5], [0, 0, 1]])
    depth = np.full((h, w), 0.8, np.float32)
    depth[5:15, 10:25] = 0.5
    rgb = np.zeros((h, w, 3), np.uint8)
    rgb[..., 0] = np.arange(w, dtype=np.uint8)[None] * 5
    rgb[..., 1] = np.arange(h, dtype=np.uint8)[:, None] * 7
    rgb[..., 2] = 9
    masks = np.zeros((h, w), np.int64)
    masks[:, :] = 0
    masks[2:22, 5:30] = 1
    return K, depth, rgb, masks


def test_backprojection_formula():
    K, depth, rgb, _ = _scene()
    T = np.eye(4)
    T[:3, 3] = [0.1, -0.2, 0.3]
    xyz, col = pvm.backproject(rgb, depth, T, K)
    assert xyz.shape == (depth.size, 3)
    i, j = 7, 12                                                  # row-major order: index i * w + j
    k = i * depth.shape[1] + j
    z = float(np.float32(np.uint16(np.float32(0.5) * 1000) / np.float32(1000)))
    np.testing.assert_allclose(xyz[k], [(j - 15.5) * z / 30.0 + 0.1, (i - 11.5) * z / 31.0 - 0.2, z + 0.3], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(col[k], rgb[i, j])
    d = depth.copy()
    d[0, 0] = 0.0004                                              # (0.0004 * 1000) -> uint16 0: dropped
    assert pvm.backproject(rgb, d, T, K)[0].shape[0] == depth.size - 1


def test_inclusive_crop_and_voxel_means():
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0000001, 0.5, 0.5], [0.5, 0.5, 0.5]])
    rgb = np.arange(12, dtype=np.uint8).reshape(4, 3)
    cx, cc = pvm.crop(xyz, rgb, [[0, 0, 0], [1, 1, 1]])
    np.testing.assert_array_equal(cx, xyz[[0, 1, 3]])
    np.testing.assert_array_equal(cc, rgb[[0, 1, 3]])
    v = 0.002
    pts = np.array([[0.0005, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0101, 0.0, 0.0], [0.0104, 0.0, 0.0], [0.005, 0.0, 0.0]])
    col = np.array([[10, 0, 0], [11, 0, 0], [100, 5, 5], [101, 6, 5], [50, 50, 50]], np.uint8)
    mx, mc = pvm.voxel_down_sample(pts, col, v)
    # origin = min - v / 2 = -0.001: voxels 0 (points 0, 1), 3 (point 4), 5 (points 2, 3), emitted in sorted order
    np.testing.assert_allclose(mx, [[0.00025, 0, 0], [0.005, 0, 0], [0.01025, 0, 0]], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(mc, [[11, 0, 0], [50, 50, 50], [101, 6, 5]])   # 10.5 -> 11, 100.5 -> 101, 5.5 -> 6


def test_get_vis_pcds_single_multi_and_cache(tmp_path):
    K, depth, rgb, masks = _scene()
    T0, T1 = np.eye(4), np.eye(4)
    T1[:3, 3] = [0.01, 0, 0]
    args = ([rgb, rgb], [depth, depth], [T0, T1], K, [masks, masks], 2, [[-1, -1, 0], [1, 1, 0.6]])
    single = pvm.get_vis_pcds(*args, use_cache=False, pcds_type=0, single_view_idx=1)
    e1 = pvm.erode_rect(masks == 1)
    sel = e1 & (depth <= 0.6)
    assert len(single[1]) == int(sel.sum())
    xyz, col = pvm.backproject(np.where(e1[..., None], rgb, 0), np.where(e1, depth, 0), T1, K)
    xyz, col = pvm.crop(xyz, col, args[6])
    np.testing.assert_array_equal(single[1].xyz, xyz.astype(np.float32))
    np.testing.assert_array_equal(single[1].rgb, col)
    multi = pvm.get_vis_pcds(*args, save_dir=str(tmp_path), use_cache=False, pcds_type=1)
    parts = []
    for T in (T0, T1):
        x, c = pvm.backproject(np.where(e1[..., None], rgb, 0), np.where(e1, depth, 0), T, K)
        parts.append(pvm.voxel_down_sample(*pvm.crop(x, c, args[6]), 0.002))
    np.testing.assert_array_equal(multi[1].xyz, np.concatenate([p[0] for p in parts]).astype(np.float32))
    np.testing.assert_array_equal(multi[1].rgb, np.concatenate([p[1] for p in parts]))
    assert sorted(os.listdir(tmp_path)) == ["obj_vis_0.pcd", "obj_vis_1.pcd"]
    cached = pvm.get_vis_pcds(*args, save_dir=str(tmp_path), use_cache=True)
    for a, b in zip(multi, cached):
        np.testing.assert_array_equal(a.xyz, b.xyz)
        np.testing.assert_array_equal(a.rgb, b.rgb)


# ------------------------------------------------------------------------------------------------ render oracle

def _brute(bg_xyz, bg_rgb, mv_xyz, mv_rgb, view, cam, now, poses):
    """Per pixel: every point of both clouds, its coverage tested directly, the least (z, index) pair wins."""
    Mb, Mk = pcd_ref.matrices(cam, now, poses)
    f = np.float32
    out = []
    for M in Mk:
        pts = [(Mb, p, i) for i, p in enumerate(np.asarray(bg_xyz, np.float32))]
        pts += [(M, p, len(bg_xyz) + i) for i, p in enumerate(np.asarray(mv_xyz, np.float32))]
        proj = []
        for Mx, p, idx in pts:
            x, y, z = (((Mx[r, 0] * p[0] + Mx[r, 1] * p[1]) + Mx[r, 2] * p[2]) + Mx[r, 3] for r in range(3))
            if not z > f(view.near):
                continue
            u = (f(view.fx) * x) / z + f(view.cx)
            v = (f(view.fy) * y) / z + f(view.cy)
            lo_u, lo_v = u - f(view.point_size / 2), v - f(view.point_size / 2)
            proj.append((float(z), idx, float(lo_u), float(lo_v)))
        cols = np.concatenate([bg_rgb, mv_rgb], 0)
        img = np.zeros((view.height, view.width, 3), np.uint8)
        for i in range(view.height):
            for j in range(view.width):
                best = None
                for z, idx, lo_u, lo_v in proj:
                    # centre (j, i) inside [lo, lo + ps) on both axes, with lo rounded up to the pixel grid
                    if np.ceil(lo_u) <= j < np.ceil(lo_u) + view.point_size and np.ceil(lo_v) <= i < np.ceil(lo_v) + view.point_size:
                        if best is None or (z, idx) < best:
                            best = (z, idx)
                c = np.array([255, 255, 255], np.uint8) if best is None else cols[best[1]]
                img[i, j] = 0 if np.all(c > 220) else c
        out.append(img)
    return np.stack(out)


def test_oracle_against_brute_force():
    view = pcd_ref.PcdView(width=9, height=7, fx=5.0, fy=5.0, cx=4.0, cy=3.0, point_size=3.0, near=0.5)
    cam = np.eye(4, dtype=np.float32)
    now = np.eye(4, dtype=np.float32)
    # background: two points on the same pixel at the same depth (tie -> lower index), one beyond the frame edge whose
    # sprite still reaches in, one exactly on a sprite edge (u - 1.5 an integer), one at z == near (culled)
    bg = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 2.0], [2.0, 0.0, 2.0], [0.3, 0.2, 1.0], [0.1, 0.1, 0.5], [-0.8, -0.6, 2.0]],
                  np.float32)
    bg_rgb = np.array([[10, 20, 30], [200, 0, 0], [0, 90, 0], [221, 230, 240], [5, 5, 5], [7, 8, 9]], np.uint8)
    mv = np.array([[0.0, 0.0, 0.0], [0.2, 0.0, 0.0], [0.0, 0.0, -1.5]], np.float32)
    mv_rgb = np.array([[1, 2, 3], [250, 250, 10], [40, 50, 60]], np.uint8)
    poses = []
    for t in ([0, 0, 2.0], [0, 0, 1.0], [0.4, 0.2, 0.55], [5, 0, 2.0], [0, 0, 0.4], [-0.6, 0.3, 1.2]):
        P = np.eye(4, dtype=np.float32)
        P[:3, 3] = t
        poses.append(P)
    poses = np.stack(poses)
    got = pcd_ref.render(bg, bg_rgb, mv, mv_rgb, view, cam, now, poses)
    want = _brute(bg, bg_rgb, mv, mv_rgb, view, cam, now, poses)
    np.testing.assert_array_equal(got, want)
    # the pinned cases themselves: the tie goes to background point 0; white (no point) and > 220 become black
    f0 = got[3]                                                    # movable cloud off-screen
    np.testing.assert_array_equal(f0[2, 4], [10, 20, 30])             # background points 0 and 1 tie at z = 2
    assert (f0[4, 5] == 0).all() and (f0[0, 8] == 0).all()             # (221, 230, 240) and the empty corner: black
    z, j0, i0, ok = pcd_ref.project(np.eye(4, dtype=np.float32)[:3], np.array([[0.1, 0.1, 0.5], [0.1, 0.1, 0.5000001]]), view)
    assert not ok[0] and ok[1]                                     # z == near is culled


# ------------------------------------------------------------------------------------------------ wiring

class FakePcdRenderer:
    point_cloud = True

    def __init__(self):
        self.calls = []

    def render(self, render_pose, pose_batch, task_model, hide_movable=False):
        self.calls.append((np.array(render_pose), np.array(pose_batch)))
        out = []
        for T in np.asarray(pose_batch).reshape(-1, 4, 4):
            f = np.zeros((6, 8, 3), np.uint8)
            f[..., 0] = int(np.clip((T[0, 3] + 1) * 60, 0, 255))
            out.append(f)
        return out


class FakeScorer:
    def score_frames(self, frames, text_embeds, rot90=True):
        assert rot90
        f = np.asarray(frames, np.float32)
        g = 20 + f[..., 0].mean(axis=(1, 2)) / 10
        return np.stack([g, np.full_like(g, 18.0)], 1).astype(np.float32)


def _task():
    import torch
    cam0 = np.eye(4, dtype=np.float32)
    cam0[:3, 3] = [0.1, 0.2, 0.3]
    cam0[:3, :3] = [[0, 1, 0], [1, 0, 0], [0, 0, -1]]
    sm = types.SimpleNamespace(scene_centre=torch.tensor([0.5, 0.0, 0.035]),
                               opt_cam_poses=[torch.eye(4), torch.from_numpy(cam0)])
    return types.SimpleNamespace(scene_model=sm, goal_caption="g", norm_captions=["n"], movable_masks=None,
                                 movable_obj=types.SimpleNamespace(pose=torch.eye(4)),
                                 task_bground_obj=types.SimpleNamespace())


def test_optimise_pose_grid_pcd_branch(tmp_path):
    from oracle import host_ref
    res = [4, 3, 2, 1, 1, 1]
    mask = np.ones(24, bool)
    mask[[1, 5]] = False

    def check(pose_batch, task_model, valid_so_far):
        import torch
        v = valid_so_far.clone()
        v[~torch.from_numpy(mask)] = False
        return v
    rend = FakePcdRenderer()
    best, poses, scores = clip_scoring.optimise_pose_grid(rend, None, [1, 0], _task(), str(tmp_path), sample_res=res,
                                                          phys_check=check, scene_type=3, use_vis_pcds=True, smoothing=False,
                                                          scorer=FakeScorer(), text_embeds=np.eye(2, 8, dtype=np.float32))
    poses = poses.numpy()
    cam, seen = rend.calls[0]
    # view 0 of render_cam_pose_idx ([1, 0] -> opt_cam_poses[1]), NOT converted to NGP; the world-frame valid poses
    np.testing.assert_array_equal(cam, _task().scene_model.opt_cam_poses[1].numpy())
    np.testing.assert_array_equal(seen.reshape(-1, 16), poses[mask])
    # the arg-max candidate is rendered once more, alone, for best_render.png
    k = int(np.argmax(scores.numpy()))
    np.testing.assert_array_equal(rend.calls[-1][1].reshape(-1, 16), poses[k:k + 1])
    lg = FakeScorer().score_frames(np.stack(rend.render(cam, poses[mask], None)), None)
    want = np.zeros(24, np.float32)
    want[mask] = host_ref.score_logits(lg, True)
    np.testing.assert_allclose(scores.numpy(), want, rtol=1e-6)
    np.testing.assert_array_equal(best.numpy().reshape(16), poses[k])
    assert sorted(os.listdir(tmp_path)) == ["best_render.png"]                   # no cb_render/*.png on this branch


def test_pcd_branch_refusals(tmp_path, monkeypatch):
    kw = dict(sample_res=[2, 2, 1, 1, 1, 1], phys_check=lambda p, t, v: v, scene_type=3, use_vis_pcds=True,
              scorer=FakeScorer(), text_embeds=np.eye(2, 8, dtype=np.float32))

    class NerfStyle:
        def render(self, *a, **k):
            raise AssertionError("not called")
    with pytest.raises(NotImplementedError, match="PointCloudRenderer"):
        clip_scoring.optimise_pose_grid(NerfStyle(), None, [0], _task(), str(tmp_path), **kw)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="sharding"):
        clip_scoring.optimise_pose_grid(FakePcdRenderer(), None, [0], _task(), str(tmp_path), **kw)
    with pytest.raises(NotImplementedError):
        pvm.PointCloudRenderer(types.SimpleNamespace()).render(np.eye(4), np.eye(4)[None], _task(), hide_movable=True)


def test_engine_picks_the_point_cloud_renderer(tmp_path, monkeypatch):
    seen = {}

    def fake_grid(renderer, *a, **k):
        import torch
        seen["renderer"], seen["use_vis_pcds"] = renderer, k["use_vis_pcds"]
        return torch.eye(4), torch.zeros((1, 16)), torch.zeros(1)
    monkeypatch.setattr(clip_scoring, "optimise_pose_grid", fake_grid)
    monkeypatch.setattr(clip_scoring, "save_pose_outputs", lambda *a: None)
    ctx = types.SimpleNamespace()
    cfg = dream2real.PathConfig(data_dir=str(tmp_path), sample_res=[2, 2, 1, 1, 1, 1], use_phys=False, use_vis_pcds=True)
    eng = dream2real.ImaginationEngine(cfg, ctx, object())
    eng.dream_best_pose(_task())
    r = seen["renderer"]
    assert isinstance(r, pvm.PointCloudRenderer) and r.ctx is ctx and seen["use_vis_pcds"] is True
    v = r.view
    assert (v.width, v.height, v.point_size) == (336, 336, 3.0)
    np.testing.assert_allclose([v.fx, v.fy, v.cx, v.cy], [436.01158022, 435.90814372, 168.0, 168.0], rtol=1e-7)
