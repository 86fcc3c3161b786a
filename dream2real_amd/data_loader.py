"""reference data_loader.py (d2r_dataloader): the RGB-D frames of a scan directory and the scene-bound ("dynamic") masks, the
latter on the GPU instead of Open3D and two 50 x 50 cv2 morphology passes per frame on the CPU."""
from __future__ import annotations

import os

import numpy as np

from . import _lib
from .segmentation import depth_to_u16

CLOSE_WINDOW = 50            # data_loader.py:108-109


def _frame_file(folder, stem, idx):
    return os.path.join(folder, "%s_%04d.png" % (stem, idx))


class d2r_dataloader:
    """One scan directory: poses.txt (one 4 x 4 T_WC per frame, 16 numbers each), images/rgb_%04d.png, depth/depth_%04d.png (16-bit
    grey, millimetres).  cfg supplies data_dir, width and height; ctx is the engine context the masks are computed on."""

    def __init__(self, cfg, ctx):
        self.cfg, self.ctx = cfg, ctx
        self.width, self.height = int(cfg.width), int(cfg.height)
        self.root_dir = cfg.data_dir
        self.rgb_dir, self.depth_dir = (os.path.join(cfg.data_dir, sub) for sub in ("images", "depth"))
        self.traj_file = os.path.join(cfg.data_dir, "poses.txt")
        self.size = None                                   # frames, known once load_rgbds has read the poses
        self.rgb_data = self.depth_data = self.T_WC_data = self.dynamic_masks = None

    def load_rgbds(self, show=False):
        """-> (rgb uint8 [N,H,W,3] in R, G, B order, depth float16 [N,H,W] in metres, T_WC float32 [N,4,4]).  `show` is the
        reference's viewer switch; there is no viewer here, so anything but False is refused."""
        if show:
            raise NotImplementedError("load_rgbds(show=True): this package has no frame viewer")
        poses = np.loadtxt(self.traj_file, dtype=np.float64).reshape(-1, 4, 4)
        wh = (self.width, self.height)
        n = self.size = poses.shape[0]
        rgb = np.empty((n, self.height, self.width, 3), np.uint8)
        mm = np.empty((n, self.height, self.width), np.uint16)
        for k in range(n):
            rgb[k] = _lib.png_read_rgb(_frame_file(self.rgb_dir, "rgb", k), wh)
            mm[k] = _lib.png_read_grey(_frame_file(self.depth_dir, "depth", k), 16, wh)
        with np.errstate(over="ignore"):                   # millimetres past float16's range become inf, as in the reference
            metres = mm.astype(np.float16) / np.float16(1000)
        self.rgb_data, self.depth_data, self.T_WC_data = rgb, metres, poses.astype(np.float32)
        return self.rgb_data, self.depth_data, self.T_WC_data

    def remove_background(self, intrinsics, scene_phys_bounds, use_cache=False):
        """-> uint8 [N,H,W], 255 outside the scene bounds; written to / read from images/dynamic_mask_rgb_%04d.png."""
        if self.size is None:
            raise RuntimeError("remove_background: call load_rgbds first")
        files = [_frame_file(self.rgb_dir, "dynamic_mask_rgb", k) for k in range(self.size)]
        if use_cache:
            self.dynamic_masks = np.stack([_lib.png_read_grey(f, 8, (self.width, self.height)) for f in files])
            return self.dynamic_masks
        box = np.array(scene_phys_bounds, np.float64).reshape(2, 3)          # a copy: the caller's bounds are not modified
        box[0, 2] = -100.0                                                   # the rule's zmin
        K = np.asarray(intrinsics, np.float64)
        self.dynamic_masks = _lib.scene_bound_masks(self.ctx, depth_to_u16(self.depth_data), self.T_WC_data, K, box, CLOSE_WINDOW)
        for f, m in zip(files, self.dynamic_masks):
            _lib.png_write_channels(m, f)
        return self.dynamic_masks
