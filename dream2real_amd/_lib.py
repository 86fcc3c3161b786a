"""ctypes binding of libd2r.so (include/d2r.h).  Fails loudly when the library is missing or
there is no gfx950 device: this package has no CPU compute path."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libd2r.so")
ABI_VERSION = 10        # D2R_ABI_VERSION of include/d2r.h this binding was written against

# One line per function of include/d2r.h: name: (restype, (argtypes...)).  The rule: a scalar (int, int32_t, uint32_t, int64_t,
# uint64_t, size_t, float, double) is its exact ctypes type; `const char *`, as a parameter or a return type, is c_char_p; every
# other pointer (char * output buffers, arrays, pointers to structs, handles, pointers to handles) is c_void_p, which takes None,
# byref(...), ctypes arrays, bytes and c_void_p, so NULL and wrong-handle arguments still reach the library's own checks; a void
# return is None.  tests/test_abi.py compares this table and the struct mirrors below with the header.
_int, _u32, _i64, _u64, _size, _f32, _f64, _str, _ptr = (C.c_int, C.c_uint32, C.c_int64, C.c_uint64, C.c_size_t, C.c_float, C.c_double,
                                                          C.c_char_p, C.c_void_p)
PROTOTYPES = {
    "d2r_abi_version": (_int, ()),
    "d2r_ctx_create": (_int, (_int, _ptr)),
    "d2r_ctx_destroy": (None, (_ptr,)),
    "d2r_ctx_set_stream": (_int, (_ptr, _ptr)),
    "d2r_ctx_synchronize": (_int, (_ptr,)),
    "d2r_last_error": (_str, (_ptr,)),
    "d2r_nerf_create": (_int, (_ptr, _ptr, _ptr)),
    "d2r_nerf_destroy": (None, (_ptr,)),
    "d2r_nerf_load_ingp": (_int, (_ptr, _ptr, _size, _ptr, _ptr, _ptr, _u32)),
    "d2r_ingp_inspect": (_int, (_ptr, _size, _ptr, _size, _ptr)),
    "d2r_ingp_validate": (_int, (_ptr, _size, _ptr)),
    "d2r_render": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _ptr, _ptr, _ptr)),
    "d2r_lens_undistort_view": (_int, (_ptr, _ptr, _ptr)),
    "d2r_nerf_eval_points": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _ptr)),
    "d2r_set_background": (_int, (_ptr, _ptr, _ptr, _ptr)),
    "d2r_rectify_background_depth": (_int, (_ptr, _ptr, _int, _ptr, _u32, _u32, _u32, _u32, _ptr, _ptr)),
    "d2r_render_composite": (_int, (_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr)),
    "d2r_clip_create": (_int, (_ptr, _ptr, _ptr, _size, _ptr)),
    "d2r_clip_destroy": (None, (_ptr,)),
    "d2r_clip_score_frames": (_int, (_ptr, _ptr, _ptr, _u32, _u32, _u32, _int, _ptr, _u32, _f32, _ptr, _ptr)),
    "d2r_clip_preprocess": (_int, (_ptr, _ptr, _ptr, _u32, _u32, _u32, _int, _ptr)),
    "d2r_clip_embed_pixels": (_int, (_ptr, _ptr, _ptr, _u32, _ptr)),
    "d2r_debug_gemm_fp8": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr)),
    "d2r_text_create": (_int, (_ptr, _ptr, _ptr, _size, _ptr)),
    "d2r_text_destroy": (None, (_ptr,)),
    "d2r_text_encode": (_int, (_ptr, _ptr, _ptr, _u32, _u32, _ptr)),
    "d2r_render_score": (_int, (_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr, _u32, _f32, _ptr, _ptr)),
    "d2r_render_score_host": (_int, (_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr, _u32, _f32, _ptr, _ptr, _ptr)),
    "d2r_png_write": (_int, (_ptr, _u32, _u32, _str, _int)),
    "d2r_png_write_batch": (_int, (_ptr, _u32, _u32, _u32, _str, _u32, _int, _int)),
    "d2r_png_write_batch_bg": (_int, (_ptr, _u32, _u32, _u32, _ptr, _str, _u32, _int)),
    "d2r_png_read_batch": (_int, (_str, _ptr, _u32, _u32, _u32, _u32, _ptr, _int)),
    "d2r_png_size": (_int, (_str, _ptr, _ptr)),
    "d2r_savetxt": (_int, (_str, _ptr, _u64, _u64, _int)),
    "d2r_get_render_stats": (_int, (_ptr, _ptr)),
    "d2r_collect_render_stats": (_int, (_ptr, _u32)),
    "d2r_get_timing": (_int, (_ptr, _ptr)),
    "d2r_ctx_set_option": (_int, (_ptr, _str, _i64)),
    "d2r_ctx_get_option": (_int, (_ptr, _str, _ptr)),
    "d2r_comm_get_unique_id": (_int, (_ptr,)),
    "d2r_comm_init": (_int, (_ptr, _ptr, _int, _int)),
    "d2r_comm_destroy": (_int, (_ptr,)),
    "d2r_allgather_scores": (_int, (_ptr, _ptr, _size, _ptr)),
    "d2r_phys_create": (_int, (_ptr, _ptr, _ptr, _u32, _ptr, _ptr, _u32, _ptr)),
    "d2r_phys_destroy": (None, (_ptr,)),
    "d2r_phys_check": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _ptr)),
    "d2r_pcd_create": (_int, (_ptr, _ptr, _ptr, _u32, _ptr)),
    "d2r_pcd_destroy": (None, (_ptr,)),
    "d2r_pcd_render": (_int, (_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr)),
    "d2r_pcd_render_score_host": (_int, (_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr, _u32, _f32, _ptr, _ptr)),
    "d2r_pcd_build": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr, _f64, _ptr, _u32, _ptr, _u32, _ptr)),
    "d2r_pcd_size": (_int, (_ptr, _ptr)),
    "d2r_pcd_read": (_int, (_ptr, _ptr, _ptr, _ptr)),
    "d2r_pcd_build_get_timing": (_int, (_ptr, _ptr)),
    "d2r_tsdf_create": (_int, (_ptr, _ptr, _f32, _f32, _ptr)),
    "d2r_tsdf_destroy": (None, (_ptr,)),
    "d2r_tsdf_integrate": (_int, (_ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _u32)),
    "d2r_tsdf_read_voxels": (_int, (_ptr, _ptr, _ptr, _ptr, _ptr)),
    "d2r_tsdf_extract": (_int, (_ptr, _f32, _ptr, _f64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr)),
    "d2r_obj_write": (_int, (_str, _ptr, _u32, _ptr, _u32, _ptr)),
    "d2r_obj_read": (_int, (_str, _ptr, _ptr, _ptr, _ptr)),
    "d2r_mesh_render": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _ptr, _ptr, _u32, _ptr, _ptr, _u32, _ptr, _ptr, _ptr, _u32, _ptr, _ptr, _ptr)),
    "d2r_tsdf_grid": (_int, (_ptr, _ptr, _ptr, _ptr, _ptr)),
    "d2r_tsdf_touch_bits": (_int, (_ptr, _f32, _f32, _ptr)),
    "d2r_tsdf_solid_points": (_int, (_ptr, _f32, _ptr, _ptr)),
    "d2r_sdfphys_create": (_int, (_ptr, _ptr, _ptr, _f32, _ptr, _u32, _ptr, _u32, _ptr)),
    "d2r_sdfphys_destroy": (None, (_ptr,)),
    "d2r_sdfphys_check": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _ptr)),
    "d2r_sdfphys_get_timing": (_int, (_ptr, _ptr, _ptr)),
    "d2r_tsdf_integrate_rgb": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _u32)),
    "d2r_tsdf_read_colours": (_int, (_ptr, _ptr, _ptr)),
    "d2r_tsdfvis_render": (_int, (_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _f32, _ptr, _ptr)),
    "d2r_tsdfvis_render_score_host": (_int, (_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _f32, _ptr, _u32, _f32, _ptr, _ptr)),
    "d2r_tsdfvis_get_timing": (_int, (_ptr, _ptr)),
    "d2r_camtrack_system": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _f32, _u32, _ptr)),
    "d2r_camtrack_refine": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr)),
    "d2r_camtrack_get_timing": (_int, (_ptr, _ptr)),
    "d2r_png_write_channels": (_int, (_ptr, _u32, _u32, _u32, _str, _int)),
    "d2r_png_info": (_int, (_str, _ptr, _ptr, _ptr, _ptr)),
    "d2r_png_read_rgb": (_int, (_str, _u32, _u32, _ptr)),
    "d2r_png_read_grey": (_int, (_str, _u32, _u32, _u32, _ptr)),
    "d2r_scene_bound_masks": (_int, (_ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr, _u32, _ptr, _ptr)),
    "d2r_masks_prune": (_int, (_ptr, _int, _ptr, _ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr, _u32, _ptr)),
    "d2r_masks_components": (_int, (_ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _ptr)),
    "d2r_masks_lut": (_int, (_ptr, _ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr)),
    "d2r_masks_census": (_int, (_ptr, _ptr, _u32, _u32, _u32, _ptr)),
    "d2r_masks_get_timing": (_int, (_ptr, _ptr)),
    "d2r_thumbs_plan": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr)),
    "d2r_thumbs_fill": (_int, (_ptr, _ptr, _ptr, _u64)),
    "d2r_thumbs_blur_bits": (_int, (_ptr, _ptr, _u32, _u32, _u32, _ptr)),
    "d2r_thumbs_get_timing": (_int, (_ptr, _ptr)),
    "d2r_proposals_labels": (_int, (_ptr, _ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr)),
    "d2r_proposals_get_timing": (_int, (_ptr, _ptr)),
    "d2r_labeltrack_grid": (_int, (_ptr, _ptr, _ptr, _ptr)),
    "d2r_labeltrack_scan": (_int, (_ptr, _ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr)),
    "d2r_labeltrack_get_timing": (_int, (_ptr, _ptr)),
    "d2r_geoprop_masks": (_int, (_ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr)),
    "d2r_geoprop_get_timing": (_int, (_ptr, _ptr)),
    "d2r_caption_embed": (_int, (_ptr, _ptr, _ptr, _ptr, _ptr)),
    "d2r_caption_vote": (_int, (_ptr, _ptr, _ptr, _u32, _ptr, _u32, _u32, _u32, _u32, _ptr, _ptr)),
    "d2r_caption_names": (_int, (_ptr, _ptr, _ptr, _u32, _u32, _u32, _u32, _ptr, _ptr)),
    "d2r_caption_load_packed": (_int, (_ptr, _ptr, _u64, _ptr, _u32, _u32)),
    "d2r_caption_get_timing": (_int, (_ptr, _ptr)),
}
EXPORTS = list(PROTOTYPES)


class D2RError(RuntimeError):
    pass


class NerfDesc(C.Structure):
    _fields_ = [("n_levels", C.c_uint32), ("n_features", C.c_uint32), ("level_scale", C.c_void_p),
                ("level_res", C.c_void_p), ("level_size", C.c_void_p), ("level_offset", C.c_void_p),
                ("n_entries", C.c_uint32), ("grid_fp16", C.c_void_p), ("dw1_fp16", C.c_void_p),
                ("dw2_fp16", C.c_void_p), ("cw1_fp16", C.c_void_p), ("cw2_fp16", C.c_void_p),
                ("cw3_fp16", C.c_void_p), ("occupancy_bits", C.c_void_p), ("aabb_scale", C.c_uint32),
                ("render_aabb", C.c_float * 6)]


class ViewC(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("focal", C.c_float * 2),
                ("center", C.c_float * 2), ("scale", C.c_float), ("offset", C.c_float * 3),
                ("background", C.c_float * 4), ("min_transmittance", C.c_float),
                ("near_distance", C.c_float), ("lens_mode", C.c_uint32), ("lens_params", C.c_float * 4)]


class ClipDesc(C.Structure):
    _fields_ = [("image_size", C.c_uint32), ("patch_size", C.c_uint32), ("hidden_size", C.c_uint32),
                ("num_layers", C.c_uint32), ("num_heads", C.c_uint32), ("mlp_size", C.c_uint32),
                ("proj_dim", C.c_uint32)]


class TextDesc(C.Structure):
    _fields_ = [("vocab_size", C.c_uint32), ("context_length", C.c_uint32), ("hidden_size", C.c_uint32),
                ("num_layers", C.c_uint32), ("num_heads", C.c_uint32), ("mlp_size", C.c_uint32),
                ("proj_dim", C.c_uint32)]


class PhysParams(C.Structure):
    _fields_ = [("sample_res", C.c_uint32 * 6), ("init_pose", C.c_float * 16), ("table_z", C.c_float),
                ("unsup_thresh", C.c_float), ("gravity", C.c_float * 3), ("perturb", C.c_float),
                ("stability_check", C.c_int32), ("disallow_regrasp", C.c_int32), ("margin", C.c_float)]


class IngpView(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("w", C.c_uint32), ("h", C.c_uint32),
                ("lens_mode", C.c_uint32), ("lens_params", C.c_float * 4)]


class IngpInfo(C.Structure):
    _fields_ = [("n_levels", C.c_uint32), ("n_features", C.c_uint32), ("aabb_scale", C.c_uint32),
                ("has_background", C.c_int32), ("dataset_scale", C.c_double), ("dataset_offset", C.c_double * 3),
                ("background_color", C.c_float * 4), ("n_views", C.c_uint32), ("n_views_written", C.c_uint32),
                ("n_unknown_keys", C.c_uint32), ("render_with_lens_distortion", C.c_int32)]


class PcdView(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("point_size", C.c_float), ("near", C.c_float)]


class FrameSink(C.Structure):
    _fields_ = [("png_dir", C.c_char_p), ("png_first_index", C.c_uint32), ("png_threads", C.c_int32), ("png_level", C.c_int32)]


class RenderStats(C.Structure):
    _fields_ = [("rays_total", C.c_uint64), ("rays_alive", C.c_uint64), ("samples", C.c_uint64),
                ("wave_iters", C.c_uint64), ("l0_tokens", C.c_uint64), ("l0_touched", C.c_uint64)]


class Timing(C.Structure):
    _fields_ = [("march_ms", C.c_double), ("march_launches", C.c_uint64), ("raygen_ms", C.c_double),
                ("raygen_launches", C.c_uint64), ("prep_ms", C.c_double), ("prep_launches", C.c_uint64),
                ("clip_ms", C.c_double), ("clip_launches", C.c_uint64), ("sort_ms", C.c_double), ("sort_launches", C.c_uint64),
                ("vit_qkv_ms", C.c_double), ("vit_qkv_launches", C.c_uint64), ("vit_attn_ms", C.c_double), ("vit_attn_launches", C.c_uint64),
                ("vit_out_ms", C.c_double), ("vit_out_launches", C.c_uint64), ("vit_fc1_ms", C.c_double), ("vit_fc1_launches", C.c_uint64),
                ("vit_fc2_ms", C.c_double), ("vit_fc2_launches", C.c_uint64)]


COMM_ID_BYTES = 128      # D2R_COMM_ID_BYTES

_lib = None


def load() -> C.CDLL:
    """dlopen libd2r.so and declare prototypes.  Raises if the library has not been built
    (`python -c "import __graft_entry__ as g; g.build()"`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise D2RError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                       "(make -C dream2real_amd/csrc); there is no CPU fallback")
    # torch wheels bundle their own libamdhip64.so.7; whichever copy of that soname is mapped first
    # serves the whole process.  Load torch's first so libd2r, torch tensors/streams and RCCL all
    # share ONE HIP runtime (with /opt/rocm's copy mapped first, torch finds no GPU afterwards).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)     # every declared symbol must be exported
        fn.restype, fn.argtypes = restype, argtypes
    if lib.d2r_abi_version() != ABI_VERSION:
        raise D2RError("libd2r.so ABI version mismatch")
    _lib = lib
    return lib


def ingp_inspect(data: bytes) -> str:
    """d2r_ingp_inspect: the msgpack tree of a snapshot as text, each leaf marked as read / ignored by the loader,
    plus the sizes the loader derives (host only: works without a GPU)."""
    lib = load()
    need = C.c_size_t(0)
    check(lib.d2r_ingp_inspect(data, len(data), None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    check(lib.d2r_ingp_inspect(data, len(data), buf, need.value, None))
    return buf.value.decode("utf-8", "replace")


def png_write(rgb, path: str, level: int = -1):
    """d2r_png_write: one uint8 [h,w,3] image -> an RGB PNG file (host only)."""
    a = np.ascontiguousarray(rgb, np.uint8)
    assert a.ndim == 3 and a.shape[2] == 3
    check(load().d2r_png_write(ptr(a), a.shape[1], a.shape[0], os.fsencode(path), level))


def png_write_batch(frames, out_dir: str, first_index: int = 0, threads: int = 0, level: int = -1):
    """d2r_png_write_batch: uint8 [n,h,w,3] -> <out_dir>/cb_rgb_%04d.png on a pool of host threads (the GIL is released
    for the duration of the call)."""
    a = np.ascontiguousarray(frames, np.uint8)
    assert a.ndim == 4 and a.shape[3] == 3
    check(load().d2r_png_write_batch(ptr(a), a.shape[0], a.shape[2], a.shape[1], os.fsencode(out_dir), first_index, threads, level))


def png_write_batch_bg(frames, background, out_dir: str, first_index: int = 0, threads: int = 0):
    """d2r_png_write_batch_bg: like png_write_batch for frames that equal `background` [h,w,3] in most scanlines (those are entropy-coded
    once); same pixels in the files."""
    a = np.ascontiguousarray(frames, np.uint8)
    b = np.ascontiguousarray(background, np.uint8)
    assert a.ndim == 4 and a.shape[3] == 3 and b.shape == a.shape[1:]
    check(load().d2r_png_write_batch_bg(ptr(a), a.shape[0], a.shape[2], a.shape[1], ptr(b), os.fsencode(out_dir), first_index, threads))


def png_write_channels(pixels, path: str, level: int = -1):
    """d2r_png_write_channels: uint8 [h,w] (grey), [h,w,3] (RGB) or [h,w,4] (RGBA) -> a PNG file (host only)."""
    a = np.ascontiguousarray(pixels, np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4):
        raise ValueError(f"expected [h,w], [h,w,3] or [h,w,4], got shape {a.shape}")
    check(load().d2r_png_write_channels(ptr(a), a.shape[1], a.shape[0], a.shape[2], os.fsencode(path), level))


def png_info(path: str):
    """d2r_png_info -> (w, h, channels, bits)."""
    v = [C.c_uint32(0) for _ in range(4)]
    check(load().d2r_png_info(os.fsencode(path), *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def png_read_rgb(path: str, size=None) -> np.ndarray:
    """d2r_png_read_rgb: one 8-bit PNG -> uint8 [h,w,3] in R, G, B order (grey replicated, alpha dropped)."""
    w, h = size or png_info(path)[:2]
    out = np.empty((h, w, 3), np.uint8)
    check(load().d2r_png_read_rgb(os.fsencode(path), w, h, ptr(out)))
    return out


def png_read_grey(path: str, bits: int = 8, size=None) -> np.ndarray:
    """d2r_png_read_grey: a grey PNG of `bits` (8 or 16) -> uint8 / uint16 [h,w].  `size` = (w, h) expected, default the file's."""
    w, h = size or png_info(path)[:2]
    out = np.empty((h, w), np.uint16 if bits == 16 else np.uint8)
    check(load().d2r_png_read_grey(os.fsencode(path), bits, w, h, ptr(out)))
    return out


def png_size(path: str):
    w, h = C.c_uint32(0), C.c_uint32(0)
    check(load().d2r_png_size(os.fsencode(path), C.byref(w), C.byref(h)))
    return int(w.value), int(h.value)


def png_read_batch(in_dir: str, n: int = 0, first_index: int = 0, threads: int = 0, indices=None, size=None) -> np.ndarray:
    """d2r_png_read_batch: <in_dir>/cb_rgb_%04d.png for n consecutive indices from first_index (or for the given
    `indices`) -> uint8 [n,h,w,3].  `size` = (w, h), default the first file's; a file of another size is an error."""
    idx = None if indices is None else np.ascontiguousarray(indices, np.uint32)
    if idx is not None:
        n = idx.shape[0]
    if n == 0:
        return np.empty((0, 0, 0, 3), np.uint8)
    w, h = size or png_size(os.path.join(in_dir, f"cb_rgb_{int(idx[0]) if idx is not None else first_index:04d}.png"))
    out = np.empty((n, h, w, 3), np.uint8)
    check(load().d2r_png_read_batch(os.fsencode(in_dir), ptr(idx), first_index, n, w, h, ptr(out), threads))
    return out


def savetxt(path: str, array):
    """d2r_savetxt: np.savetxt(path, array) with numpy's defaults, byte for byte, formatted on the library's worker
    threads (1-D: one number per line; 2-D: one row per line; 0-D is refused like np.savetxt does)."""
    a = np.asarray(array)
    if a.ndim == 0 or a.ndim > 2:
        raise ValueError(f"Expected 1D or 2D array, got {a.ndim}D array instead")
    a = np.ascontiguousarray(a, np.float64)
    rows, cols = (a.shape[0], 1) if a.ndim == 1 else a.shape
    check(load().d2r_savetxt(os.fsencode(path), ptr(a), rows, cols, 0))


def obj_write(path: str, vertices, triangles, keep=None):
    """d2r_obj_write: float32 [nv,3] vertices and uint32 [nt,3] triangles -> a Wavefront .obj of `v` and `f` lines (faces
    with keep[t] == 0 are left out, their vertices stay).  Host only."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    k = None if keep is None else np.ascontiguousarray(keep, np.uint8).reshape(-1)
    assert k is None or k.shape[0] == t.shape[0]
    check(load().d2r_obj_write(os.fsencode(path), ptr(v), v.shape[0], ptr(t), t.shape[0], ptr(k)))


def obj_read(path: str):
    """d2r_obj_read: a Wavefront .obj -> (vertices float32 [nv,3], triangles uint32 [nt,3]); faces of more than three corners become
    fans, groups are concatenated.  Host only."""
    lib = load()
    nv, nt = C.c_uint32(0), C.c_uint32(0)
    check(lib.d2r_obj_read(os.fsencode(path), C.byref(nv), C.byref(nt), None, None))
    v, t = np.empty((nv.value, 3), np.float32), np.empty((nt.value, 3), np.uint32)
    check(lib.d2r_obj_read(os.fsencode(path), C.byref(nv), C.byref(nt), ptr(v), ptr(t)))
    return v, t


def mesh_render(ctx, view: PcdView, cam_pose, verts, tris, tri_item, item_mats, item_rgb, cube_centres=None, cube_half=None,
                cube_scores=None, background=(255, 255, 255), return_ids: bool = False):
    """d2r_mesh_render: a triangle soup of coloured items and score cubes -> uint8 [h,w,3] (and the int32
    [h,w] ids image: the triangle, -1 - cube, or INT32_MIN)."""
    f32 = lambda a, shape: np.ascontiguousarray(a, np.float32).reshape(shape)
    cam = f32(cam_pose, 16)
    v = f32(verts if verts is not None else [], (-1, 3))
    t = np.ascontiguousarray(tris if tris is not None else [], np.uint32).reshape(-1, 3)
    it = np.ascontiguousarray(tri_item if tri_item is not None else [], np.uint32).reshape(-1)
    mats = f32(item_mats if item_mats is not None else [], (-1, 16))
    cols = np.ascontiguousarray(item_rgb if item_rgb is not None else [], np.uint8).reshape(-1, 3)
    cc = f32(cube_centres if cube_centres is not None else [], (-1, 3))
    ch = f32(cube_half if cube_half is not None else [], -1)
    cs = np.ascontiguousarray(cube_scores if cube_scores is not None else [], np.uint16).reshape(-1)
    if it.shape[0] != t.shape[0] or cols.shape[0] != mats.shape[0] or not (cc.shape[0] == ch.shape[0] == cs.shape[0]):
        raise ValueError("mesh_render: tri_item per triangle, one colour per item matrix, one half-width and one score per cube")
    bg = np.ascontiguousarray(background, np.uint8).reshape(3)
    rgb = np.empty((view.height, view.width, 3), np.uint8)
    ids = np.empty((view.height, view.width), np.int32) if return_ids else None
    some = lambda a: ptr(a) if a.size else None
    check(load().d2r_mesh_render(_h(ctx), C.byref(view), ptr(cam), some(v), v.shape[0], some(t), some(it), t.shape[0], some(mats), some(cols),
                                 mats.shape[0], some(cc), some(ch), some(cs), cs.shape[0], ptr(bg), ptr(rgb), ptr(ids)), _h(ctx))
    return (rgb, ids) if return_ids else rgb


def _h(ctx):
    """The d2r_ctx pointer of an engine.Context (or a raw handle)."""
    return getattr(ctx, "h", ctx)


def _frames(a, dtype, name):
    a = np.ascontiguousarray(a, dtype)
    if a.ndim != 3:
        raise ValueError(f"{name} must be [n, h, w], got shape {a.shape}")
    return a


def scene_bound_masks(ctx, depth_u16, poses, K, bounds, window: int = 50, return_raw: bool = False):
    """d2r_scene_bound_masks: uint16 millimetre depth [n,h,w], float32 poses [n,4,4], K [3,3], bounds [[min xyz],[max xyz]] ->
    uint8 0 / 255 [n,h,w]; with return_raw also the mask before the closing.  ctx: a d2r_ctx pointer."""
    d = _frames(depth_u16, np.uint16, "depth_u16")
    n, h, w = d.shape
    T = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    if T.shape[0] != n:
        raise ValueError(f"{T.shape[0]} poses for {n} frames")
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    b = np.array(bounds, np.float64).reshape(6)          # a copy: the caller's bounds stay as they are
    out = np.empty((n, h, w), np.uint8)
    raw = np.empty((n, h, w), np.uint8) if return_raw else None
    check(load().d2r_scene_bound_masks(_h(ctx), ptr(d), n, w, h, ptr(T), ptr(Kd), ptr(b), window, ptr(out), ptr(raw)), _h(ctx))
    return (out, raw) if return_raw else out


def masks_prune(ctx, mode: int, masks, depth_u16=None, oob=None, poses=None, K=None, centre=None, min_area: int = 200):
    """d2r_masks_prune: mode 0 duplicate_prune (needs depth_u16, poses, K, centre), 1 disconnected_prune; uint8 labels [n,h,w] ->
    pruned uint8 labels with 255 where oob == 255."""
    m = _frames(masks, np.uint8, "masks")
    n, h, w = m.shape
    d = None if depth_u16 is None else _frames(depth_u16, np.uint16, "depth_u16")
    o = None if oob is None else _frames(oob, np.uint8, "oob")
    for a in (d, o):
        if a is not None and a.shape != m.shape:
            raise ValueError(f"shape {a.shape} does not match the masks' {m.shape}")
    T = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    if T is not None and T.shape[0] != n:
        raise ValueError(f"{T.shape[0]} poses for {n} frames")
    Kd = None if K is None else np.ascontiguousarray(K, np.float64).reshape(9)
    c = None if centre is None else np.ascontiguousarray(centre, np.float64).reshape(3)
    out = np.empty((n, h, w), np.uint8)
    check(load().d2r_masks_prune(_h(ctx), mode, ptr(m), ptr(d), ptr(o), n, w, h, ptr(T), ptr(Kd), ptr(c), min_area, ptr(out)), _h(ctx))
    return out


def masks_components(ctx, mask, depth_u16):
    """d2r_masks_components (parity hook, one frame [h,w]) -> (order-key image uint32 [h,w], area uint32 [h,w], sums uint64 [h,w,4])."""
    m = np.ascontiguousarray(mask, np.uint8)
    d = np.ascontiguousarray(depth_u16, np.uint16)
    if m.ndim != 2 or d.shape != m.shape:
        raise ValueError("mask and depth_u16 must be [h, w] of one shape")
    h, w = m.shape
    keys, area, sums = np.empty((h, w), np.uint32), np.empty((h, w), np.uint32), np.empty((h, w, 4), np.uint64)
    check(load().d2r_masks_components(_h(ctx), ptr(m), ptr(d), w, h, ptr(keys), ptr(area), ptr(sums)), _h(ctx))
    return keys, area, sums


def masks_lut(ctx, masks, lut, oob=None, alpha: bool = False):
    """d2r_masks_lut: (lut[masks] != 0) | (oob != 0) as uint8 0 / 1 [n,h,w]; with alpha also 255 (1 - out)."""
    m = _frames(masks, np.uint8, "masks")
    n, h, w = m.shape
    o = None if oob is None else _frames(oob, np.uint8, "oob")
    if o is not None and o.shape != m.shape:
        raise ValueError(f"shape {o.shape} does not match the masks' {m.shape}")
    t = np.ascontiguousarray(lut, np.uint8).reshape(-1)
    if t.shape[0] != 256:
        raise ValueError("lut must have 256 entries")
    out = np.empty((n, h, w), np.uint8)
    al = np.empty((n, h, w), np.uint8) if alpha else None
    check(load().d2r_masks_lut(_h(ctx), ptr(m), ptr(o), n, w, h, ptr(t), ptr(out), ptr(al)), _h(ctx))
    return (out, al) if alpha else out


def masks_census(ctx, masks):
    """d2r_masks_census: uint8 labels [n,h,w] -> uint32 [n,256], the pixels of every label in every frame."""
    m = _frames(masks, np.uint8, "masks")
    n, h, w = m.shape
    out = np.empty((n, 256), np.uint32)
    check(load().d2r_masks_census(_h(ctx), ptr(m), n, w, h, ptr(out)), _h(ctx))
    return out


def masks_timing(ctx):
    """d2r_masks_get_timing -> (upload, kernels, download) of the context's last batch mask call, device-event milliseconds."""
    ms = np.zeros(3, np.float64)
    check(load().d2r_masks_get_timing(_h(ctx), ptr(ms)), _h(ctx))
    return tuple(float(x) for x in ms)


THUMB_REC_WORDS = 10                                    # D2R_THUMB_REC_WORDS: object, frame, flags, area, row0, col0, rows, cols, offset low / high
THUMB_ACCEPTED, THUMB_CONTAINER, THUMB_ROTATED, THUMB_EDGE, THUMB_SMALL = 1, 2, 4, 8, 16


def thumbs_plan(ctx, rgbs, masks, oob, num_objs: int, topdown: bool, multi_view: bool = True, single_view_idx: int = 0,
                min_area: int = 200, hole_area: int = 400, pad: int = 5, dilate_k: int = 60):
    """d2r_thumbs_plan: uint8 rgbs [n,h,w,3], labels [n,h,w], out-of-scene masks [n,h,w] -> (records uint32
    [n_recs, THUMB_REC_WORDS], one per (object, visited frame), total bytes of the packed thumbnails).  The frames stay on the
    device for thumbs_fill."""
    c = np.ascontiguousarray(rgbs, np.uint8)
    m = _frames(masks, np.uint8, "masks")
    o = _frames(oob, np.uint8, "oob")
    n, h, w = m.shape
    if c.shape != (n, h, w, 3) or o.shape != m.shape:
        raise ValueError(f"rgbs {c.shape}, masks {m.shape} and oob {o.shape} do not describe the same frames")
    params = np.array([bool(topdown), bool(multi_view), single_view_idx, min_area, hole_area, pad, dilate_k], np.uint32)
    count = max(int(num_objs) - 1, 0) * (n if multi_view else 1)
    recs = np.zeros((max(count, 1), THUMB_REC_WORDS), np.uint32)
    n_recs, total = C.c_uint32(recs.shape[0]), C.c_uint64(0)
    check(load().d2r_thumbs_plan(_h(ctx), ptr(c), ptr(m), ptr(o), n, w, h, num_objs, ptr(params), ptr(recs), C.byref(n_recs),
                                 C.byref(total)), _h(ctx))
    return recs[:n_recs.value], int(total.value)


def thumbs_fill(ctx, noise, total: int) -> np.ndarray:
    """d2r_thumbs_fill: the noise image uint8 [h,w,3] -> the packed thumbnails uint8 [total] of the context's last thumbs_plan; an
    accepted record's image is out[offset : offset + rows * cols * 3].reshape(rows, cols, 3)."""
    z = np.ascontiguousarray(noise, np.uint8)
    out = np.zeros(max(total, 1), np.uint8)
    check(load().d2r_thumbs_fill(_h(ctx), ptr(z), ptr(out), total), _h(ctx))
    return out[:total]


def thumbs_blur_bits(ctx, bits, dilate_k: int = 60) -> np.ndarray:
    """d2r_thumbs_blur_bits (parity hook): a 0 / 1 image [h,w] -> its blur bit dilated by dilate_k x dilate_k, uint8 0 / 1."""
    b = np.ascontiguousarray(bits, np.uint8)
    if b.ndim != 2:
        raise ValueError(f"bits must be [h, w], got shape {b.shape}")
    out = np.empty(b.shape, np.uint8)
    check(load().d2r_thumbs_blur_bits(_h(ctx), ptr(b), b.shape[1], b.shape[0], dilate_k, ptr(out)), _h(ctx))
    return out


PROP_REC_WORDS = 8                                      # D2R_PROP_REC_WORDS: area, ncomp, stage, label, boundary, ew, eh, dd
PROP_MAX = 1024                                         # D2R_PROP_MAX


def proposals_labels(ctx, props, inside=None, records: bool = False, inter: bool = False):
    """d2r_proposals_labels: proposals uint8 [m,h,w] (non-zero = set), inside uint8 [h,w] or None -> the label
    image uint8 [h,w]; with records / inter also uint32 [m, PROP_REC_WORDS] / uint32 [m,m] (a tuple in that order)."""
    p = np.ascontiguousarray(props, np.uint8)
    assert p.ndim == 3
    m, h, w = p.shape
    s = None if inside is None else np.ascontiguousarray(inside, np.uint8)
    assert s is None or s.shape == (h, w)
    labels = np.zeros((h, w), np.uint8)
    recs = np.zeros((m, PROP_REC_WORDS), np.uint32) if records else None
    mat = np.zeros((m, m), np.uint32) if inter else None
    check(load().d2r_proposals_labels(_h(ctx), ptr(p), ptr(s), m, w, h, ptr(labels), ptr(recs), ptr(mat)), _h(ctx))
    out = (labels,) + ((recs,) if records else ()) + ((mat,) if inter else ())
    return out if len(out) > 1 else labels


def proposals_timing(ctx):
    """d2r_proposals_get_timing -> (upload, kernels, download) of the context's last proposals_labels, device-event milliseconds."""
    ms = np.zeros(3, np.float64)
    check(load().d2r_proposals_get_timing(_h(ctx), ptr(ms)), _h(ctx))
    return tuple(float(x) for x in ms)


def thumbs_timing(ctx):
    """d2r_thumbs_get_timing -> (upload, kernels, download) of the context's last thumbs_plan plus thumbs_fill, device-event milliseconds."""
    ms = np.zeros(3, np.float64)
    check(load().d2r_thumbs_get_timing(_h(ctx), ptr(ms)), _h(ctx))
    return tuple(float(x) for x in ms)


CAPTION_MAX_K, CAPTION_MAX_V, CAPTION_MAX_D = 8, 8192, 1024     # D2R_CAPTION_MAX_K / _V / _D


def caption_embed(ctx, scorer, n_thumbs: int, crops: bool = False, pixel_values: bool = False):
    """d2r_caption_embed: the context's n_thumbs packed thumbnails (thumbs_fill, or caption_load_packed) ->
    L2-normalised embeddings float32 [n_thumbs, proj]; with crops / pixel_values also uint8 [n_thumbs,S,S,3] / float32
    [n_thumbs,3,S,S] (a tuple in that order).  scorer: an engine.ClipScorer."""
    S, D = scorer.cfg["image_size"], scorer.cfg["proj"]
    emb = np.zeros((max(n_thumbs, 1), D), np.float32)
    u8 = np.zeros((max(n_thumbs, 1), S, S, 3), np.uint8) if crops else None
    pv = np.zeros((max(n_thumbs, 1), 3, S, S), np.float32) if pixel_values else None
    check(load().d2r_caption_embed(_h(ctx), scorer.h, ptr(emb), ptr(u8), ptr(pv)), _h(ctx))
    out = (emb[:n_thumbs],) + ((u8[:n_thumbs],) if crops else ()) + ((pv[:n_thumbs],) if pixel_values else ())
    return out if len(out) > 1 else out[0]


def caption_vote(ctx, embeds, obj_of, class_embeds, n_objs: int, k: int):
    """d2r_caption_vote (parity hook): embeds float32 [T,D], obj_of [T] (0 .. n_objs - 1, non-decreasing), class_embeds float32 [V,D]
    -> (indices uint32 [n_objs,k], scores float32 [n_objs,k])."""
    c = np.ascontiguousarray(class_embeds, np.float32)
    e = np.ascontiguousarray(embeds, np.float32).reshape(-1, c.shape[1])
    o = np.ascontiguousarray(obj_of, np.uint32).reshape(-1)
    if o.shape[0] != e.shape[0]:
        raise ValueError(f"{o.shape[0]} objects for {e.shape[0]} embeddings")
    idx, sc = np.zeros((n_objs, k), np.uint32), np.zeros((n_objs, k), np.float32)
    check(load().d2r_caption_vote(_h(ctx), ptr(e), ptr(o), e.shape[0], ptr(c), c.shape[0], c.shape[1], n_objs, k, ptr(idx), ptr(sc)), _h(ctx))
    return idx, sc


def caption_names(ctx, scorer, class_embeds, n_objs: int, k: int):
    """d2r_caption_names: the context's thumbnails of the plan's objects 1 .. n_objs -> (indices uint32 [n_objs,k] into class_embeds
    float32 [V,D], scores float32 [n_objs,k]); only these cross back to the host.  n_objs must be the plan's num_objs - 1."""
    c = np.ascontiguousarray(class_embeds, np.float32)
    idx, sc = np.zeros((n_objs, k), np.uint32), np.zeros((n_objs, k), np.float32)
    check(load().d2r_caption_names(_h(ctx), scorer.h, ptr(c), c.shape[0], c.shape[1], n_objs, k, ptr(idx), ptr(sc)), _h(ctx))
    return idx, sc


def caption_load_packed(ctx, images, obj_of, n_objs: int):
    """d2r_caption_load_packed (parity hook): uint8 [h,w,3] images of any sizes, packed at offsets that are multiples of 4 as
    thumbs_fill packs them, stand on the context where a plan's thumbnails would.  obj_of: the object 0 .. n_objs - 1 per image,
    non-decreasing.  -> the packed buffer."""
    recs, parts, off = [], [], 0
    for img, o in zip(images, obj_of):
        a = np.ascontiguousarray(img, np.uint8)
        assert a.ndim == 3 and a.shape[2] == 3
        recs.append([int(o), a.shape[0], a.shape[1], off & 0xffffffff, off >> 32])
        pad = -a.size % 4
        parts += [a.reshape(-1), np.zeros(pad, np.uint8)]
        off += a.size + pad
    packed = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, np.uint8)
    r = np.ascontiguousarray(recs, np.uint32).reshape(-1, 5)
    check(load().d2r_caption_load_packed(_h(ctx), ptr(packed), packed.size, ptr(r), r.shape[0], n_objs), _h(ctx))
    return packed


def caption_timing(ctx):
    """d2r_caption_get_timing -> (upload, preprocess, tower, scoring, download) of the context's last caption call, device-event
    milliseconds."""
    ms = np.zeros(5, np.float64)
    check(load().d2r_caption_get_timing(_h(ctx), ptr(ms)), _h(ctx))
    return tuple(float(x) for x in ms)


def pcd_build(ctx, rgb, depth_u16, labels, cam_poses, K, bounds, voxel: float, views, obj_ids):
    """d2r_pcd_build: uint8 rgb [n,h,w,3], uint16 millimetre depth [n,h,w], uint8 labels [n,h,w], fp64 poses [n,4,4], K [3,3], bounds
    [[min xyz],[max xyz]], voxel (0: no down-sampling), frame indices `views`, labels `obj_ids` -> one d2r_pcd handle per object id
    (DESIGN.md section 2b); each goes to d2r_pcd_render as it is, to pcd_read for its points, and to d2r_pcd_destroy in the end."""
    c = np.ascontiguousarray(rgb, np.uint8)
    d = _frames(depth_u16, np.uint16, "depth_u16")
    m = _frames(labels, np.uint8, "labels")
    n, h, w = d.shape
    if c.shape != (n, h, w, 3) or m.shape != d.shape:
        raise ValueError(f"rgb {c.shape}, depth {d.shape} and labels {m.shape} do not describe the same frames")
    T = np.ascontiguousarray(cam_poses, np.float64).reshape(-1, 16)
    if T.shape[0] != n:
        raise ValueError(f"{T.shape[0]} poses for {n} frames")
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    b = np.ascontiguousarray(bounds, np.float64).reshape(6)
    vw = np.ascontiguousarray(views, np.uint32).reshape(-1)
    ids = np.ascontiguousarray(obj_ids, np.uint8).reshape(-1)
    out = (C.c_void_p * max(1, ids.size))()
    check(load().d2r_pcd_build(_h(ctx), ptr(c), ptr(d), ptr(m), n, w, h, ptr(T), ptr(Kd), ptr(b), voxel, ptr(vw), vw.size, ptr(ids),
                               ids.size, out), _h(ctx))
    return [C.c_void_p(out[i]) for i in range(ids.size)]


def pcd_read(ctx, handle):
    """d2r_pcd_size + d2r_pcd_read: a device cloud -> (xyz float32 [n,3], rgb uint8 [n,3])."""
    n = C.c_uint32()
    check(load().d2r_pcd_size(handle, C.byref(n)))
    xyz, rgb = np.empty((n.value, 3), np.float32), np.empty((n.value, 3), np.uint8)
    check(load().d2r_pcd_read(_h(ctx), handle, ptr(xyz), ptr(rgb)), _h(ctx))
    return xyz, rgb


def pcd_build_timing(ctx):
    """d2r_pcd_build_get_timing -> (upload, kernels) of the context's last d2r_pcd_build, device-event milliseconds."""
    ms = np.zeros(2, np.float64)
    check(load().d2r_pcd_build_get_timing(_h(ctx), ptr(ms)), _h(ctx))
    return tuple(float(x) for x in ms)


def ingp_validate(data: bytes) -> IngpInfo:
    """d2r_ingp_validate: raises D2RError with the loader's message (naming the key) when d2r_nerf_load_ingp would refuse
    the snapshot; returns what the loader would report about it otherwise.  Host only."""
    info = IngpInfo()
    check(load().d2r_ingp_validate(data, len(data), C.byref(info)))
    return info


def check(rc: int, ctx=None):
    if rc != 0:
        msg = load().d2r_last_error(ctx)
        raise D2RError(f"libd2r error {rc}: {msg.decode() if msg else '?'}")


def ptr(a) -> C.c_void_p:
    """Host pointer of a C-contiguous numpy array (or None)."""
    if a is None:
        return C.c_void_p(0)
    assert a.flags["C_CONTIGUOUS"]
    return C.c_void_p(a.ctypes.data)


def view_c(v) -> ViewC:
    return ViewC(v.width, v.height, (C.c_float * 2)(*v.focal), (C.c_float * 2)(*v.center), v.scale,
                 (C.c_float * 3)(*v.offset), (C.c_float * 4)(*v.background), v.min_transmittance,
                 v.near_distance, int(v.lens_mode), (C.c_float * 4)(*[float(x) for x in v.lens_params]))
