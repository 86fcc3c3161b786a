"""The colour-TSDF visual backend (`engine.vis_backend = "tsdf"`): this package's own third visual model beside the NeRF
snapshots and the point-cloud ablation; nothing here stands where a stage of the reference stands.  A visual model is a
physics_utils.TsdfVolume fused with colour from the masked RGB-D frames (d2r_tsdf_integrate_rgb), the renderer a ray caster over a
background volume and a movable volume (d2r_tsdfvis_render): dense and hole-free, built on the MI355X
from the scan alone."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .pcd_visual_model import INTRINSICS_CLIP_VIEW, NEAR, _np, _poses16
from .physics_utils import ERODE_BACKGROUND, ERODE_OBJECT, TSDF_WEIGHT_THRESHOLD, TsdfVolume


def get_vis_tsdfs(rgbs, depths, cam_poses, intrinsics, masks, scene_bounds, *, ctx, erode_k: int = ERODE_OBJECT) -> TsdfVolume:
    """Every frame fused into one colour volume over scene_bounds.  masks[f]: non-zero = excluded, as in get_vis_pcds' masking;
    erode_k: section 2c's erosion for the object class (ERODE_BACKGROUND for a background, ERODE_OBJECT for an object)."""
    vol = TsdfVolume(ctx, np.asarray(_np(scene_bounds), np.float64).reshape(2, 3))
    try:
        for f in range(len(depths)):
            u16 = (_np(depths[f]) * 1000).astype(np.uint16)
            vol.integrate_rgb(u16, _np(masks[f]) == 0, _np(rgbs[f]).astype(np.uint8), intrinsics, cam_poses[f], erode_k)
    except Exception:
        vol.close()
        raise
    return vol


class TsdfRenderer:
    """The world-pose surface of pcd_visual_model.PointCloudRenderer over colour volumes: renders the task's background volume
    plus the movable volume at each candidate pose, 336 x 336 through INTRINSICS_CLIP_VIEW by default."""

    world_poses = True          # optimise_pose_grid takes its world-pose branch (view 0, OpenCV pose, world-frame candidates)

    def __init__(self, ctx, width: int = 336, height: int = 336, intrinsics=INTRINSICS_CLIP_VIEW, near: float = NEAR,
                 weight_threshold: float = TSDF_WEIGHT_THRESHOLD):
        K = np.asarray(intrinsics, np.float64)
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.weight_threshold = float(weight_threshold)
        self.view = _lib.PcdView(self.width, self.height, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), 1.0, float(near))

    @staticmethod
    def _handle(vol):
        if not isinstance(vol, TsdfVolume) or not vol.h:
            raise TypeError(f"the TSDF renderer needs open physics_utils.TsdfVolume visual models, got {type(vol).__name__}")
        return vol.h

    def _args(self, render_pose, pose_batch, task_model):
        bg = self._handle(task_model.task_bground_obj.vis_model)
        mv = self._handle(task_model.movable_obj.vis_model)
        cam = np.ascontiguousarray(_np(render_pose).reshape(16), np.float32)
        now = np.ascontiguousarray(_np(task_model.movable_obj.pose).reshape(16), np.float32)
        return bg, mv, cam, now, _poses16(pose_batch)

    def render(self, render_pose, pose_batch, task_model, return_depth: bool = False):
        """-> list of uint8 [H,W,3], one per pose of pose_batch ([K,16] or [K,4,4]); render_pose is the OpenCV camera-to-world
        pose.  With return_depth also float32 [K,H,W], the camera depth of each pixel's hit (+inf: none)."""
        bg, mv, cam, now, poses = self._args(render_pose, pose_batch, task_model)
        K = poses.shape[0]
        frames = np.empty((K, self.height, self.width, 3), np.uint8)
        depth = np.empty((K, self.height, self.width), np.float32) if return_depth else None
        self.ctx.check(self.ctx.lib.d2r_tsdfvis_render(self.ctx.h, bg, mv, C.byref(self.view), _lib.ptr(cam), _lib.ptr(now), _lib.ptr(poses), K,
                                                       self.weight_threshold, _lib.ptr(frames), _lib.ptr(depth)))
        return (list(frames), depth) if return_depth else list(frames)

    def render_score(self, render_pose, pose_batch, task_model, scorer, text_embeds, return_frames: bool = False):
        """The fused call (d2r_tsdfvis_render_score_host): frames ray-cast and scored on the GPU -> logits [K,C] (and the frames
        uint8 [K,H,W,3] with return_frames).  Equal to scorer.score_frames(render(...), rot90=True)."""
        bg, mv, cam, now, poses = self._args(render_pose, pose_batch, task_model)
        K = poses.shape[0]
        t = np.ascontiguousarray(text_embeds, np.float32)
        logits = np.empty((K, t.shape[0]), np.float32)
        frames = np.empty((K, self.height, self.width, 3), np.uint8) if return_frames else None
        if K:
            self.ctx.check(self.ctx.lib.d2r_tsdfvis_render_score_host(
                self.ctx.h, bg, mv, scorer.h, C.byref(self.view), _lib.ptr(cam), _lib.ptr(now), _lib.ptr(poses), K, self.weight_threshold,
                _lib.ptr(t), t.shape[0], scorer.logit_scale, _lib.ptr(logits), _lib.ptr(frames)))
        return (logits, frames) if return_frames else logits

    def timing(self):
        """d2r_tsdfvis_get_timing -> (upload, background cast, candidates' casts, copies to the host) of the context's last call,
        device-event milliseconds."""
        ms = np.zeros(4, np.float64)
        self.ctx.check(self.ctx.lib.d2r_tsdfvis_get_timing(self.ctx.h, _lib.ptr(ms)))
        return tuple(float(x) for x in ms)


__all__ = ["get_vis_tsdfs", "TsdfRenderer", "ERODE_BACKGROUND", "ERODE_OBJECT"]
