"""reference scene_model.py: ObjectModel, SceneModel, TaskModel.  The task masks go through the LUT kernel (`d2r_masks_lut`:
out = lut[mask] | (oob != 0)); the models come from get_vis_pcds / get_vis_ngps / physics_utils.create_lazy_phys_mods.  `ctx=`
stands where the reference assumes a CUDA device."""
from __future__ import annotations

import os

import numpy as np

from . import _lib, physics_utils


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


class ObjectModel:
    """One object of the scene: its visual and physics models, its pose (world from object, 4 x 4), a thumbnail for captioning and
    the label it carries in the scene's masks."""

    def __init__(self, name, vis_model, phys_model, init_pose, thumbnail, mask_idx):
        self.name, self.mask_idx, self.thumbnail = name, mask_idx, thumbnail
        self.vis_model, self.phys_model = vis_model, phys_model
        self.pose = init_pose

    def update_pose(self, new_pose):
        self.pose = new_pose


class SceneModel:
    """What build_scene_model hands on: the objects (`objs` holds the background object too), the frames they were built from
    (rgbs [N,H,W,3], depths, optimised camera poses, intrinsics, label masks) and the scene's centre, bounds and type."""

    _FIELDS = ("scene_centre", "objs", "bground_obj", "rgbs", "depths", "opt_cam_poses", "intrinsics", "masks", "scene_bounds", "scene_type")

    def __init__(self, scene_centre, objs, bground_obj, rgbs, depths, opt_cam_poses, intrinsics, masks, scene_bounds, scene_type, device=None):
        given = locals()
        for field in self._FIELDS:
            setattr(self, field, given[field])
        self.device = device               # kept for callers that pass one; the GPU work here goes through ctx=


def task_bground_lut(scene_model, movable_obj, relevant_objs, render_distractors):
    """The 256-entry table of create_task_bground_obj's rule (:67-76): 1 for the labels that are NOT task background."""
    lut = np.zeros(256, np.uint8)
    for obj in scene_model.objs:
        if render_distractors:
            if obj is movable_obj:
                lut[obj.mask_idx] = 1
        elif obj is movable_obj or obj is scene_model.bground_obj or not any(obj is r for r in relevant_objs):
            lut[obj.mask_idx] = 1
    return lut


class TaskModel:
    def __init__(self, user_instr, goal_caption, norm_captions, scene_model, movable_obj, task_bground_obj, task_bground_masks, topdown):
        self.scene_model, self.movable_obj = scene_model, movable_obj
        self.user_instr, self.goal_caption, self.norm_captions = user_instr, goal_caption, norm_captions
        self.task_bground_obj, self.task_bground_masks = task_bground_obj, task_bground_masks
        self.topdown = topdown
        self.movable_masks = _np(scene_model.masks) != movable_obj.mask_idx          # True off the movable object (host side, bool)

    @staticmethod
    def create_task_bground_obj(scene_model, movable_obj, relevant_objs, out_scene_bound_masks, save_dir, use_vis_pcds=False, pcds_type=None,
                                single_view_idx=0, render_distractors=False, use_cache=False, data_dir=None, *, ctx, vis_backend="default"):
        """-> (task_bground_obj, task_bground_masks uint8 [N,H,W]): 0 = task background, 1 = movable / distractor / out of scene."""
        lut = task_bground_lut(scene_model, movable_obj, relevant_objs, render_distractors)
        task_bground_masks = _lib.masks_lut(ctx, _np(scene_model.masks).astype(np.uint8), lut, _np(out_scene_bound_masks).astype(np.uint8))
        if vis_backend == "tsdf":
            from .tsdf_visual_model import ERODE_BACKGROUND, get_vis_tsdfs
            vis_model = get_vis_tsdfs(scene_model.rgbs, scene_model.depths, scene_model.opt_cam_poses, scene_model.intrinsics, task_bground_masks,
                                      scene_model.scene_bounds, ctx=ctx, erode_k=ERODE_BACKGROUND)
        elif use_vis_pcds:
            from .pcd_visual_model import get_vis_pcds
            vis_model = get_vis_pcds(scene_model.rgbs, scene_model.depths, scene_model.opt_cam_poses, scene_model.intrinsics, task_bground_masks, 1,
                                     scene_model.scene_bounds, save_dir=save_dir, vis=False, use_cache=use_cache, pcds_type=pcds_type,
                                     single_view_idx=single_view_idx, ctx=ctx)[0]
        else:
            from .ngp_visual_model import get_vis_ngps
            vis_model = get_vis_ngps(scene_model.rgbs, task_bground_masks, scene_model.scene_type, use_cache=use_cache, data_dir=data_dir, fg=False,
                                     render_distract=render_distractors, ctx=ctx)
        import torch
        return ObjectModel("__task_bground__", vis_model, None, torch.eye(4), None, None), task_bground_masks

    @staticmethod
    def movable_masks_of(scene_model, movable_obj, *, ctx):
        """uint8 [N,H,W]: 0 on the movable object's pixels, 1 elsewhere (the reference's logical_not(masks == mask_idx))."""
        lut = np.ones(256, np.uint8)
        lut[movable_obj.mask_idx] = 0
        return _lib.masks_lut(ctx, _np(scene_model.masks).astype(np.uint8), lut)

    @staticmethod
    def create_movable_vis_model(scene_model, movable_obj, out_scene_bound_masks, save_dir, use_vis_pcds=False, pcds_type=None, single_view_idx=0,
                                 use_cache=False, data_dir=None, *, ctx, vis_backend="default"):
        movable_masks = TaskModel.movable_masks_of(scene_model, movable_obj, ctx=ctx)
        if vis_backend == "tsdf":
            from .tsdf_visual_model import ERODE_OBJECT, get_vis_tsdfs
            return get_vis_tsdfs(scene_model.rgbs, scene_model.depths, scene_model.opt_cam_poses, scene_model.intrinsics, movable_masks,
                                 scene_model.scene_bounds, ctx=ctx, erode_k=ERODE_OBJECT)
        if use_vis_pcds:
            from .pcd_visual_model import get_vis_pcds
            return get_vis_pcds(scene_model.rgbs, scene_model.depths, scene_model.opt_cam_poses, scene_model.intrinsics, movable_masks, 1,
                                scene_model.scene_bounds, save_dir=save_dir, vis=False, use_cache=use_cache, pcds_type=pcds_type,
                                single_view_idx=single_view_idx, ctx=ctx)[0]
        from .ngp_visual_model import get_vis_ngps
        return get_vis_ngps(scene_model.rgbs, movable_masks, scene_model.scene_type, use_cache=use_cache, data_dir=data_dir, fg=True, ctx=ctx)

    @staticmethod
    def create_lazy_phys_mods(scene_model, movable_obj, scene_bounds, save_dir, embodied=False, vis=False, use_cache=False, use_phys_tsdf=True,
                              use_vis_pcds=False, single_view_idx=0, *, ctx=None, convexify=None, phys_backend="hulls"):
        return physics_utils.create_lazy_phys_mods(scene_model, movable_obj, scene_bounds, save_dir, embodied=embodied, vis=vis, use_cache=use_cache,
                                                   use_phys_tsdf=use_phys_tsdf, use_vis_pcds=use_vis_pcds, single_view_idx=single_view_idx, ctx=ctx,
                                                   convexify=convexify, phys_backend=phys_backend)

    def free_visual_models(self):
        self.task_bground_obj.vis_model = None


def write_task_images(rgbs, masks, data_dir, fg, *, ctx):
    """The reference's export step (reconstruction/ngp_visual_model.py:31-46): images_fg | images_bg / rgb_%04d.png as RGBA, R, G, B
    in that order, alpha = 255 (1 - mask).  masks: 0 / non-zero [N,H,W]."""
    rgb = _np(rgbs).astype(np.uint8)
    lut = np.ones(256, np.uint8)
    lut[0] = 0
    _, alpha = _lib.masks_lut(ctx, _np(masks).astype(np.uint8), lut, alpha=True)
    out_dir = os.path.join(data_dir, "images_fg" if fg else "images_bg")
    os.makedirs(out_dir, exist_ok=True)
    for k in range(rgb.shape[0]):
        _lib.png_write_channels(np.concatenate([rgb[k], alpha[k][..., None]], -1), os.path.join(out_dir, "rgb_%04d.png" % k))
    return out_dir
