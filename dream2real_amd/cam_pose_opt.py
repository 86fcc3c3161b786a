"""Camera poses refined against a TSDF volume (`engine.cam_pose_refine = "tsdf"`): this package's own stand-in
for the poses NeRF training optimises in the reference.  Each frame's pose is refined against the volume fused so far --
frame-to-model tracking on the signed distance field itself -- by d2r_camtrack_refine: the linearisation on the GPU, 29 integer sums
back per iteration, the 6 x 6 solve on the host in fp64."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .physics_utils import ERODE_BACKGROUND, TsdfVolume

SUMS = 29                   # D2R_CAMTRACK_SUMS
SCALE_LOG2 = 29             # D2R_CAMTRACK_SCALE_LOG2
MAX_ITERS_CAP = 64          # D2R_CAMTRACK_MAX_ITERS
STATUS = ("converged", "max_iters", "degenerate", "too_few")      # D2R_CAMTRACK_*
FUSING_WEIGHT_THRESHOLD = 1.0       # while a scan is fused frame by frame: after one frame nothing has weight 3
MIN_PIXELS = 500


# the mirrors of include/d2r.h's d2r_camtrack_params and d2r_camtrack_report (tests/test_camtrack_host.py holds their layout to a C compiler's)
class CamtrackParams(C.Structure):
    _fields_ = [("weight_threshold", C.c_float), ("stride", C.c_uint32), ("max_iters", C.c_uint32), ("min_pixels", C.c_uint32)]


class CamtrackReport(C.Structure):
    _fields_ = [("status", C.c_int32), ("iters", C.c_uint32), ("pixels_first", C.c_uint64), ("pixels_last", C.c_uint64),
                ("rms_first", C.c_double), ("rms_last", C.c_double), ("poses", (C.c_float * 16) * MAX_ITERS_CAP),
                ("sums", (C.c_int64 * SUMS) * MAX_ITERS_CAP)]


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _frame(vol, depth_u16, mask, intrinsics, pose):
    if not isinstance(vol, TsdfVolume) or not vol.h:
        raise TypeError(f"camera tracking needs an open physics_utils.TsdfVolume, got {type(vol).__name__}")
    d = np.ascontiguousarray(_np(depth_u16), np.uint16)
    m = np.ascontiguousarray(_np(mask), np.uint8)
    if d.ndim != 2 or m.shape != d.shape:
        raise ValueError(f"depth_u16 {d.shape} and mask {m.shape} must be [h, w] of one shape")
    K = np.ascontiguousarray(np.asarray(_np(intrinsics), np.float64).reshape(9), np.float32)
    T = np.ascontiguousarray(np.asarray(_np(pose), np.float64).reshape(16), np.float32)
    return d, m, K, T


def camtrack_system(vol, depth_u16, mask, intrinsics, pose, *, ctx, weight_threshold: float = FUSING_WEIGHT_THRESHOLD, stride: int = 1):
    """d2r_camtrack_system (parity hook): one linearisation of a frame (uint16 millimetre depth [h,w], mask non-zero = use) against
    `vol` at `pose` -> the 29 sums, int64: the upper triangle of J^T J row by row, J^T r, sum r^2 (all times 2^SCALE_LOG2), the count."""
    d, m, K, T = _frame(vol, depth_u16, mask, intrinsics, pose)
    sums = np.zeros(SUMS, np.int64)
    ctx.check(ctx.lib.d2r_camtrack_system(ctx.h, vol.h, _lib.ptr(d), _lib.ptr(m), d.shape[1], d.shape[0], _lib.ptr(K), _lib.ptr(T),
                                          float(weight_threshold), int(stride), _lib.ptr(sums)))
    return sums


def refine_cam_pose(vol, depth_u16, mask, intrinsics, pose, *, ctx, weight_threshold: float = FUSING_WEIGHT_THRESHOLD, stride: int = 1,
                    max_iters: int = 20, min_pixels: int = MIN_PIXELS, trace: bool = False):
    """d2r_camtrack_refine: the pose of one frame refined against `vol` -> (pose float32 [4,4], report).  report: status (one of STATUS),
    iters (linearisations done), pixels_first / pixels_last, rms_first / rms_last (metres); with trace also poses float32 [iters,4,4]
    (the fp32 pose each linearisation used) and sums int64 [iters,29]."""
    d, m, K, T = _frame(vol, depth_u16, mask, intrinsics, pose)
    params = CamtrackParams(float(weight_threshold), int(stride), int(max_iters), int(min_pixels))
    rep = CamtrackReport()
    out = np.zeros(16, np.float32)
    ctx.check(ctx.lib.d2r_camtrack_refine(ctx.h, vol.h, _lib.ptr(d), _lib.ptr(m), d.shape[1], d.shape[0], _lib.ptr(K), _lib.ptr(T),
                                          C.byref(params), _lib.ptr(out), C.byref(rep)))
    report = dict(status=STATUS[rep.status], iters=int(rep.iters), pixels_first=int(rep.pixels_first), pixels_last=int(rep.pixels_last),
                  rms_first=float(rep.rms_first), rms_last=float(rep.rms_last))
    if trace:
        n = int(rep.iters)
        report["poses"] = np.ctypeslib.as_array(rep.poses)[:n].reshape(n, 4, 4).copy()
        report["sums"] = np.ctypeslib.as_array(rep.sums)[:n].copy()
    return out.reshape(4, 4), report


def camtrack_timing(ctx):
    """d2r_camtrack_get_timing -> (upload, kernels, downloads) of the context's last refine_cam_pose, device-event milliseconds."""
    ms = np.zeros(3, np.float64)
    ctx.check(ctx.lib.d2r_camtrack_get_timing(ctx.h, _lib.ptr(ms)))
    return tuple(float(x) for x in ms)


def refine_cam_poses(depths, cam_poses, intrinsics, masks, scene_bounds, *, ctx, anchor: int = 0, stride: int = 1, max_iters: int = 20,
                     min_pixels: int = MIN_PIXELS, erode_k: int = ERODE_BACKGROUND):
    """The scan: one plain volume over scene_bounds; the anchor frame is fused at its given pose and returned
    unchanged; every other frame, in order, is refined against the volume at weight threshold 1 and, when it ends converged or at
    max_iters, fused at its refined pose; a frame that ends degenerate or with too few pixels keeps its input pose and is not fused.
    depths [N,h,w] metres, cam_poses [N,4,4], masks [N,h,w] scene-bound masks (0 = inside the bounds: used), erode_k the fusion's
    erosion (the background's, as get_vis_tsdfs uses for one) -> (float32 [N,4,4], list of N reports; each has `fused`)."""
    poses = np.array([np.asarray(_np(p), np.float64).reshape(4, 4) for p in cam_poses]).astype(np.float32)
    n = len(depths)
    if poses.shape[0] != n or len(masks) != n:
        raise ValueError(f"{poses.shape[0]} poses and {len(masks)} masks for {n} frames")
    if not 0 <= anchor < n:
        raise ValueError(f"anchor {anchor} is not one of the {n} frames")
    out = poses.copy()
    reports = [None] * n
    vol = TsdfVolume(ctx, np.asarray(_np(scene_bounds), np.float64).reshape(2, 3))
    try:
        for f in [anchor] + [k for k in range(n) if k != anchor]:
            u16 = (_np(depths[f]) * 1000).astype(np.uint16)
            inside = _np(masks[f]) == 0
            if f == anchor:
                reports[f] = dict(status="anchor", iters=0, fused=True)
            else:
                pose, rep = refine_cam_pose(vol, u16, inside, intrinsics, poses[f], ctx=ctx, stride=stride, max_iters=max_iters,
                                            min_pixels=min_pixels)
                rep["fused"] = rep["status"] in ("converged", "max_iters")
                if rep["fused"]:
                    out[f] = pose
                reports[f] = rep
            if reports[f]["fused"]:
                vol.integrate(u16, inside, intrinsics, out[f], erode_k)
    finally:
        vol.close()
    return out, reports


__all__ = ["camtrack_system", "refine_cam_pose", "refine_cam_poses", "camtrack_timing", "STATUS", "SUMS", "SCALE_LOG2"]
