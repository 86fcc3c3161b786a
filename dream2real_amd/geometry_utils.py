"""Heat-map smoothing of the path (reference vision_3d/geometry_utils.py:252-269) and the pictures that follow it: the cost
volume and the best pose (:137-206 and dream2real.py:392-400, Open3D windows there) rendered by d2r_mesh_render (DESIGN.md
section 2f) into uint8 frames and PNG files."""
import numpy as np


def gaussian_kernel_3(sigma: float = 0.7) -> np.ndarray:
    """torchvision gaussian_blur(kernel_size=3): normalised pdf at x in {-1,0,1}, outer product."""
    x = np.array([-1.0, 0.0, 1.0], np.float32)
    k = np.exp(np.float32(-0.5) * (x / np.float32(sigma)) ** 2).astype(np.float32)
    k = (k / k.sum()).astype(np.float32)
    return np.outer(k, k).astype(np.float32)


def spatially_smooth_heatmap(pose_scores, sample_res, sigma: float = 0.7) -> np.ndarray:
    """3x3 Gaussian over the (x, y) plane of every (z, orientation) slice.  Invalid (zero)
    scores and the 1-cell border take the minimum non-zero score; invalid cells are zeroed
    again afterwards.  pose_scores: [prod(sample_res)] -> same shape, float32."""
    s = np.array(pose_scores, np.float32, copy=True).reshape(-1)
    X, Y = int(sample_res[0]), int(sample_res[1])
    R = int(np.prod([int(v) for v in sample_res[2:]]))
    zero = s == 0
    mn = s[~zero].min()
    s[zero] = mn
    planes = s.reshape(X, Y, R)
    padded = np.full((X + 2, Y + 2, R), mn, np.float32)
    padded[1:-1, 1:-1] = planes
    k = gaussian_kernel_3(sigma)
    out = np.zeros((X, Y, R), np.float32)
    for di in range(3):
        for dj in range(3):
            out += k[di, dj] * padded[di:di + X, dj:dj + Y]
    out = out.reshape(-1)
    out[zero] = 0
    return out


# the reference's vis_utils.pastel_colors; mesh i takes entry i % 10 (dream2real.py:396)
pastel_colors = np.array([[142, 236, 245], [140, 251, 140], [255, 120, 120], [251, 248, 204], [207, 186, 240], [241, 192, 232],
                          [253, 228, 207], [163, 196, 243], [144, 219, 244], [152, 245, 225]], np.uint8)
BGROUND_GREY = (100, 100, 100)         # the background meshes under the cost volume (:181)
VIS_BACKGROUND = (255, 255, 255)
VIS_NEAR = 0.01


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def cost_volume_cubes(pose_scores, sample_res, pose_batch):
    """reference :139-167 on the host in fp64 -> (centres float32 [P,3], half-widths float32 [P], scores uint16 [P]) of the
    P = sample_res[0] * sample_res[1] * sample_res[2] positions.  Non-zero scores become 10 ** (10 s), are min-max normalised over
    the non-zero scores, and each position takes the maximum over its orientations and the position of that pose; the cube width is
    the smallest spacing between samples; the score is rint(65535 s).  Two departures: an axis with sample_res == 1 is left out of
    the spacing minimum (the reference divides by zero there; with no axis left the width is 0), and a single non-zero score (or
    equal ones) normalises to 1 where the reference divides by zero."""
    s = np.array(_np(pose_scores), np.float64).reshape(-1)
    res = [int(v) for v in sample_res]
    P, R = res[0] * res[1] * res[2], res[3] * res[4] * res[5]
    batch = np.asarray(_np(pose_batch), np.float64).reshape(P, R, 4, 4)
    nz = s != 0
    if nz.any():
        s[nz] = 10.0 ** (s[nz] * 10.0)
        lo, hi = s[nz].min(), s[nz].max()
        s[nz] = (s[nz] - lo) / (hi - lo) if hi > lo else 1.0
    s = s.reshape(P, R)
    best = s.argmax(1)                              # the first maximum, as torch.max
    pos = batch[np.arange(P), best, :3, 3]
    spacing = [(pos[:, a].max() - pos[:, a].min()) / (res[a] - 1) for a in range(3) if res[a] > 1]
    width = min(spacing) if spacing else 0.0
    scores = np.rint(65535.0 * s[np.arange(P), best]).astype(np.uint16)
    return pos.astype(np.float32), np.full(P, 0.5 * width, np.float32), scores


def _soup(mesh_paths):
    """.obj files -> (verts float32 [nv,3], tris uint32 [nt,3], tri_item uint32 [nt]): one item per file"""
    import os
    from . import _lib
    verts, tris, item, base = [], [], [], 0
    for i, path in enumerate(mesh_paths):
        if not os.path.exists(path):
            raise FileNotFoundError(f"mesh file {path} is missing")
        v, t = _lib.obj_read(path)
        verts.append(v)
        tris.append(t + np.uint32(base))
        item.append(np.full(t.shape[0], i, np.uint32))
        base += v.shape[0]
    return np.concatenate(verts), np.concatenate(tris), np.concatenate(item)


def _finish(frame, out_path):
    if out_path is not None:
        from . import _lib
        _lib.png_write(frame, out_path)
    return frame


def vis_cost_volume(pose_scores, sample_res, pose_batch, bground_geoms, use_phys_mods=True, colourmap=True, fixed_ori=None, exp=True, *,
                    ctx, view, cam_pose, out_path=None):
    """reference :137-206 as a picture: the background meshes (.obj paths) in grey, one cube per sampled position coloured and
    weighted by its normalised score.  view: an _lib.PcdView; cam_pose: OpenCV camera-to-world [4,4].  -> uint8 [h,w,3], written
    to out_path as a PNG when given.  Only the reference's defaults (use_phys_mods, colourmap, exp, no fixed_ori) are drawn."""
    from . import _lib
    if not (use_phys_mods and colourmap and exp and fixed_ori is None):
        raise NotImplementedError("vis_cost_volume draws the reference's defaults: use_phys_mods, colourmap, exp, fixed_ori=None")
    verts, tris, item = _soup(bground_geoms)
    n = len(bground_geoms)
    centres, half, scores = cost_volume_cubes(pose_scores, sample_res, pose_batch)
    frame = _lib.mesh_render(ctx, view, cam_pose, verts, tris, item, np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)),
                             np.tile(np.array(BGROUND_GREY, np.uint8), (n, 1)), centres, half, scores, background=VIS_BACKGROUND)
    return _finish(frame, out_path)


def vis_best_pose(best_pose, bground_geoms, movable_geom, movable_init_pose, *, ctx, view, cam_pose, out_path=None):
    """reference dream2real.py:392-400 as a picture: the background meshes and the movable mesh (.obj paths) in pastel_colors by
    index, the last one moved by best_pose @ inv(movable_init_pose).  -> uint8 [h,w,3], written to out_path when given."""
    from . import _lib
    paths = list(bground_geoms) + [movable_geom]
    verts, tris, item = _soup(paths)
    mats = np.tile(np.eye(4), (len(paths), 1, 1))
    mats[-1] = np.asarray(_np(best_pose), np.float64).reshape(4, 4) @ np.linalg.inv(np.asarray(_np(movable_init_pose), np.float64).reshape(4, 4))
    cols = pastel_colors[np.arange(len(paths)) % pastel_colors.shape[0]]
    frame = _lib.mesh_render(ctx, view, cam_pose, verts, tris, item, mats.astype(np.float32), cols, background=VIS_BACKGROUND)
    return _finish(frame, out_path)
