"""The point-cloud ablation renderer (pcd.hip) on the MI355X: frames bit-identical to the numpy oracle (tests/pcd_ref.py),
the fused render-and-score call against the two-step route and the fp32 oracle, and dream_best_pose with use_vis_pcds.
All clouds are seeded synthetic data: a table plane and boxes for the background, a coloured sphere for the movable
object."""
import os

import numpy as np
import pytest

from dream2real_amd.clip_model import CLIP_CONFIGS, random_clip_state_dict
from oracle import host_ref
from oracle.pipeline import oracle_logits
from synthetic_scenes import look_at_opencv
from tests import pcd_ref
from tests.parity_utils import logit_bar, random_unit_text_embeds

pytestmark = pytest.mark.gpu

CENTRE = np.array([0.5, 0.0, 0.05])


def _background(seed=1):
    r = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.linspace(0.0, 1.0, 400), np.linspace(-0.5, 0.5, 400), indexing="ij"), -1).reshape(-1, 2)
    table = np.concatenate([g, np.zeros((g.shape[0], 1))], 1)
    boxes = []
    for lo, hi in (([0.2, -0.3, 0.0], [0.3, -0.15, 0.12]), ([0.65, 0.1, 0.0], [0.8, 0.3, 0.2])):
        boxes.append(r.uniform(lo, hi, (20000, 3)))
    xyz = np.concatenate([table] + boxes, 0).astype(np.float32)
    rgb = r.integers(0, 256, (xyz.shape[0], 3), dtype=np.uint8)
    rgb[: table.shape[0] // 3] = r.integers(215, 256, (table.shape[0] // 3, 3), dtype=np.uint8)   # many > 220 colours
    return xyz, rgb


def _sphere(n=6000, r0=0.04, seed=2, dup_from=None):
    r = np.random.default_rng(seed)
    d = r.normal(size=(n, 3))
    xyz = (CENTRE + r0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rgb = np.stack([np.full(n, 230), (xyz[:, 2] * 2000 % 256), r.integers(0, 256, n)], 1).astype(np.uint8)
    if dup_from is not None:     # exact copies of background points: equal-depth ties at the identity candidate
        xyz = np.concatenate([xyz, dup_from[:500], xyz[:50]], 0)      # ... and copies of its own points (movable ties)
        rgb = np.concatenate([rgb, np.full((500, 3), 7, np.uint8), np.full((50, 3), 9, np.uint8)], 0)
    return xyz, rgb


def _candidates(K=80, seed=3):
    r = np.random.default_rng(seed)
    out = [np.eye(4, dtype=np.float32)]                         # the identity: movable copies tie with the background
    eye = np.array([0.5, -0.7, 0.45])
    for k in range(K - 1):
        P = np.eye(4)
        a = r.uniform(0, 2 * np.pi)
        P[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        kind = k % 5
        if kind == 0:
            t = r.uniform([-0.4, -0.4, 0], [0.4, 0.4, 0.1])            # on the table, occluding / occluded by the boxes
        elif kind == 1:
            t = r.uniform([-1.5, -0.5, 0], [1.5, 0.5, 0.5])            # partly or wholly off-screen
        elif kind == 2:
            t = eye - CENTRE + r.uniform(-0.06, 0.06, 3)               # around the camera centre: behind it, straddling near
        elif kind == 3:
            t = (eye - CENTRE) * r.uniform(0.75, 0.95)                 # close to the camera: large rectangles, several tiles
        else:
            t = r.uniform([-0.2, -0.2, 0], [0.2, 0.2, 0.05])
        P[:3, 3] = CENTRE + t - P[:3, :3] @ CENTRE                  # turn about the sphere's centre, then move it by t
        out.append(P.astype(np.float32))
    return np.stack(out)


@pytest.fixture(scope="module")
def gpu():
    from dream2real_amd import engine
    from dream2real_amd import pcd_visual_model as pvm
    ctx = engine.Context(0)
    bx, bc = _background()
    mx, mc = _sphere(dup_from=bx)
    task = _Task(pvm.PointCloud(bx, bc), pvm.PointCloud(mx, mc))
    cam = look_at_opencv([0.5, -0.7, 0.45], CENTRE).astype(np.float32)
    yield dict(engine=engine, pvm=pvm, ctx=ctx, task=task, cam=cam)
    ctx.close()


class _Task:
    def __init__(self, bg, mv, pose=None):
        import types
        import torch
        self.task_bground_obj = types.SimpleNamespace(vis_model=bg)
        self.movable_obj = types.SimpleNamespace(vis_model=mv, pose=torch.eye(4) if pose is None else torch.from_numpy(pose))


def _oracle(task, view, cam, poses):
    return pcd_ref.render(task.task_bground_obj.vis_model.xyz, task.task_bground_obj.vis_model.rgb,
                          task.movable_obj.vis_model.xyz, task.movable_obj.vis_model.rgb, view, cam,
                          task.movable_obj.pose.numpy(), poses)


@pytest.mark.parametrize("W,H", [(336, 336), (200, 120)])
def test_frames_equal_the_oracle(gpu, W, H):
    pvm, ctx, task, cam = gpu["pvm"], gpu["ctx"], gpu["task"], gpu["cam"]
    K = np.array([[436.01158022 * W / 336, 0, W / 2], [0, 435.90814372 * W / 336, H / 2], [0, 0, 1]])
    rend = pvm.PointCloudRenderer(ctx, W, H, intrinsics=K)
    poses = _candidates()
    got = np.stack(rend.render(cam, poses, task))
    view = pcd_ref.PcdView(W, H, float(np.float32(K[0, 0])), float(np.float32(K[1, 1])), W / 2, H / 2, 3.0, pvm.NEAR)
    want = _oracle(task, view, cam, poses)
    bad = np.nonzero((got != want).any(axis=(1, 2, 3)))[0]
    assert bad.size == 0, f"candidates {bad[:10]} differ in {(got != want).any(-1).sum()} pixels"
    # the fixture exercises what it claims: black (> 220 and empty) pixels, large rectangles, candidates wholly off-screen
    # (several identical frames: the background alone)
    diff = (got != got[0]).any(-1).sum(axis=(1, 2))
    assert (got == 0).all(-1).any() and diff.max() > 0.2 * W * H and len({f.tobytes() for f in got}) < len(got) - 2
    again = np.stack(rend.render(cam, poses, task))
    np.testing.assert_array_equal(again, got)                    # order-free: two runs give the same bytes
    rend.close()


def test_movable_cloud_larger_than_the_frame(gpu):
    """A movable cloud right in front of the camera: its rectangle is the whole frame (28 LDS tiles at 336 x 336)."""
    pvm, ctx, cam = gpu["pvm"], gpu["ctx"], gpu["cam"]
    bx, bc = _background(seed=5)
    r = np.random.default_rng(9)
    fwd = cam[:3, 2]
    plane = cam[:3, 3] + 0.2 * fwd + (r.uniform(-0.2, 0.2, (150000, 1)) * cam[:3, 0] + r.uniform(-0.2, 0.2, (150000, 1)) * cam[:3, 1])
    task = _Task(pvm.PointCloud(bx, bc), pvm.PointCloud(plane.astype(np.float32), r.integers(0, 200, (150000, 3), dtype=np.uint8)))
    rend = pvm.PointCloudRenderer(ctx)
    poses = np.stack([np.eye(4, dtype=np.float32)] * 3)
    poses[1, :3, 3] = [0.01, 0.0, 0.005]
    poses[2, :3, 3] = [0.0, 0.0, -0.3]
    got = np.stack(rend.render(cam, poses, task))
    view = pcd_ref.PcdView()
    np.testing.assert_array_equal(got, _oracle(task, view, cam, poses))
    # the movable sprites of candidate 0 reach all four frame edges: its rectangle is the whole frame
    _, Mk = pcd_ref.matrices(cam, np.eye(4), poses[:1])
    hit = (pcd_ref.splat(np.full(336 * 336, pcd_ref.EMPTY, np.uint64), Mk[0], task.movable_obj.vis_model.xyz, 0, view)
           != pcd_ref.EMPTY).reshape(336, 336)
    assert hit[0].any() and hit[-1].any() and hit[:, 0].any() and hit[:, -1].any() and hit.mean() > 0.5
    rend.close()


def test_fused_logits_equal_the_two_step_route(gpu):
    engine, pvm, ctx, task, cam = gpu["engine"], gpu["pvm"], gpu["ctx"], gpu["task"], gpu["cam"]
    cfg = CLIP_CONFIGS["vit_tiny"]
    sc = engine.ClipScorer(ctx, cfg, random_clip_state_dict(cfg, seed=6, text=False))
    rend = pvm.PointCloudRenderer(ctx)
    poses = _candidates(70, seed=4)
    text = random_unit_text_embeds(cfg["proj"], 3)
    chunk = ctx.get_option("chunk")
    ctx.set_option("chunk", 32)                                   # several passes, a remainder
    try:
        lg, frames = rend.render_score(cam, poses, task, sc, text, return_frames=True)
        two_step = sc.score_frames(frames, text, rot90=True)
    finally:
        ctx.set_option("chunk", chunk)
    np.testing.assert_array_equal(frames, np.stack(rend.render(cam, poses, task)))
    np.testing.assert_array_equal(lg, two_step)
    np.testing.assert_array_equal(rend.render_score(cam, poses, task, sc, text), sc.score_frames(frames, text, rot90=True))
    sc.close()
    rend.close()


def test_fused_logits_vit_l14_336_against_the_oracle(gpu):
    engine, pvm, ctx, task, cam = gpu["engine"], gpu["pvm"], gpu["ctx"], gpu["task"], gpu["cam"]
    cfg = CLIP_CONFIGS["vit_l14_336"]
    sd = random_clip_state_dict(cfg, seed=6, text=False)
    sc = engine.ClipScorer(ctx, cfg, sd)
    rend = pvm.PointCloudRenderer(ctx)
    poses = _candidates(4, seed=7)
    text = random_unit_text_embeds(cfg["proj"], 3)
    lg = rend.render_score(cam, poses, task, sc, text)
    frames = _oracle(task, pcd_ref.PcdView(), cam, poses)
    olg, _ = oracle_logits(frames, cfg, sd, text)
    err = float(np.abs(lg - olg).max() / sc.logit_scale)
    assert err <= logit_bar(cfg, err, "pcd frames, full-depth vit_l14_336, 4 candidates x 3 captions")
    sc.close()
    rend.close()


def test_dream_best_pose_with_point_clouds(gpu, tmp_path):
    import torch
    from PIL import Image
    from dream2real_amd import dream2real
    import types
    engine, pvm, ctx, task, cam = gpu["engine"], gpu["pvm"], gpu["ctx"], gpu["task"], gpu["cam"]
    cfg_clip = CLIP_CONFIGS["vit_tiny"]
    sd = random_clip_state_dict(cfg_clip, seed=6)
    sc = engine.ClipScorer(ctx, cfg_clip, sd)
    O = np.eye(4, dtype=np.float32)
    O[:3, 3] = CENTRE
    mv = task.movable_obj.vis_model
    t = _Task(task.task_bground_obj.vis_model, mv, O)
    t.scene_model = types.SimpleNamespace(scene_centre=torch.tensor([0.5, 0.0, 0.05]), opt_cam_poses=[torch.from_numpy(cam)],
                                          device="cpu")
    t.goal_caption, t.norm_captions, t.movable_masks = "g", ["n"], None
    frames0 = _oracle(t, pcd_ref.PcdView(), cam, O[None])
    _, e0 = oracle_logits(frames0, cfg_clip, sd, np.zeros((1, cfg_clip["proj"])))
    r = np.random.default_rng(5)
    te = e0[0][None] + 0.8 * r.standard_normal((2, e0.shape[1])) / np.sqrt(e0.shape[1]) * np.linalg.norm(e0[0])
    t.text_embeds = (te / np.linalg.norm(te, axis=-1, keepdims=True)).astype(np.float32)
    sample_res = [6, 5, 2, 1, 1, 1]
    cfg = dream2real.PathConfig(data_dir=str(tmp_path), sample_res=sample_res, scene_type=3, use_phys=False,
                                use_vis_pcds=True, spatial_smoothing=False)
    eng = dream2real.ImaginationEngine(cfg, ctx, sc)
    best, pose_batch, scores = eng.dream_best_pose(t)
    assert isinstance(eng.renderer, pvm.PointCloudRenderer)
    poses = pose_batch.numpy()
    frames = _oracle(t, pcd_ref.PcdView(), cam, poses)
    lg, _ = oracle_logits(frames, cfg_clip, sd, t.text_embeds)
    want = host_ref.score_logits(lg, True)
    tol = float((100.0 * logit_bar(cfg_clip) * (1.0 + np.abs(want)) / np.abs(lg[:, 1])).max())
    got = scores.numpy()
    print(f"[parity] dream_best_pose use_vis_pcds (vit_tiny): max |score - oracle| = {np.abs(got - want).max():.2e} (bar {tol:.2e})")
    np.testing.assert_allclose(got, want, rtol=0, atol=tol)
    k = int(np.argmax(got))
    assert k == int(np.argmax(want))
    np.testing.assert_array_equal(best.numpy().reshape(16), poses[k])
    png = np.asarray(Image.open(os.path.join(str(tmp_path), "best_render.png")).convert("RGB"))
    np.testing.assert_array_equal(png, np.rot90(frames[k], k=1, axes=(0, 1)))
    assert not os.path.exists(os.path.join(str(tmp_path), "cb_render"))
    for name in ("goal_pose.txt", "pose_batch.txt", "pose_scores.txt"):
        assert os.path.exists(os.path.join(str(tmp_path), name))
    eng.renderer.close()
    sc.close()
