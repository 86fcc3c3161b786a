/*
 * d2r.h — C ABI of libd2r.so: the MI355X (gfx950) render-and-score path of Dream2Real.
 *
 * The reference has no C ABI in tree; its two native seams on this path are Python
 * extension surfaces:
 *   (1) pyngp.Testbed  — load_snapshot / set_camera_to_training_view /
 *       set_nerf_camera_matrix / background_color / render_mode / render(w,h,spp,linear)
 *       used at reference reconstruction/combined_rendering.py:98-105,112-113,116,123-130
 *       and reconstruction/ngp_visual_model.py:24-28;
 *   (2) transformers.CLIPModel / CLIPProcessor used at reference clip_scoring.py:150-151,
 *       177-181.
 * Each entry point below names the reference interface it replaces.  The Python host
 * (dream2real_amd/) binds these with ctypes; INTEGRATION.md shows the binding a
 * reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative d2r_status; the message is
 *     available from d2r_last_error(ctx) (or d2r_last_error(NULL) for create failures);
 *   - no C++ exception crosses the ABI, nothing calls abort();
 *   - "host" pointers are read/written before the call returns; "dev" pointers are HIP
 *     device pointers on the context's device, used on the context's stream;
 *   - the library owns its handles; parameter blobs are copied to the device at create;
 *   - one context per GPU; calls on one context must be serialised by the caller;
 *   - there is NO CPU fallback: every compute entry point needs a gfx950 device.
 */
#ifndef D2R_H
#define D2R_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2R_API __attribute__((visibility("default")))
#define D2R_ABI_VERSION 10

typedef enum {
    D2R_OK = 0,
    D2R_ERR_INVALID = -1,   /* bad argument */
    D2R_ERR_DEVICE = -2,    /* HIP error, or no gfx950 device */
    D2R_ERR_MEMORY = -3,    /* allocation failed */
    D2R_ERR_UNSUPPORTED = -4
} d2r_status;

typedef struct d2r_ctx d2r_ctx;
typedef struct d2r_nerf d2r_nerf;
typedef struct d2r_clip d2r_clip;

/* ------------------------------------------------------------------ context */

D2R_API int d2r_abi_version(void);
/* One context per GPU.  Owns a HIP stream and a workspace that grows on demand. */
D2R_API int d2r_ctx_create(int device, d2r_ctx **out);
D2R_API void d2r_ctx_destroy(d2r_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream); NULL restores the
 * context's own stream. */
D2R_API int d2r_ctx_set_stream(d2r_ctx *ctx, void *hip_stream);
D2R_API int d2r_ctx_synchronize(d2r_ctx *ctx);
D2R_API const char *d2r_last_error(d2r_ctx *ctx);

/* --------------------------------------------------------------- NeRF model */

/* State a pyngp.Testbed holds after load_snapshot (reference ngp_visual_model.py:24-28):
 * tiny-cuda-nn hash grid + density/colour MLPs + 128^3 occupancy bitfield(s). */
typedef struct {
    uint32_t n_levels;          /* L: 16, or 8 */
    uint32_t n_features;        /* F: 2 with L = 16, 4 with L = 8 (the two layouts with L*F = 32 inputs) */
    const float *level_scale;   /* host [L]: exp2(l*log2(b))*N_min - 1 */
    const uint32_t *level_res;  /* host [L]: ceil(scale)+1 */
    const uint32_t *level_size; /* host [L]: entries per level */
    const uint32_t *level_offset; /* host [L]: first entry of each level */
    uint32_t n_entries;         /* sum(level_size) */
    const uint16_t *grid_fp16;  /* host [n_entries][F] */
    const uint16_t *dw1_fp16;   /* host [64][L*F]  density layer 1, row-major [out][in] */
    const uint16_t *dw2_fp16;   /* host [16][64]   density layer 2 */
    const uint16_t *cw1_fp16;   /* host [64][32]   colour layer 1, in = [density out 16 | SH 16] */
    const uint16_t *cw2_fp16;   /* host [64][64] */
    const uint16_t *cw3_fp16;   /* host [16][64]   rows 0..2 = rgb */
    const uint8_t *occupancy_bits; /* host [n_cascades][128^3/8], bit x+128*(y+128*z), LSB first */
    uint32_t aabb_scale;        /* a power of two, 1..128 (0 is read as 1): the model's box is the cube of that side
                                 * centred at 0.5; n_cascades = log2(aabb_scale)+1 occupancy grids, cascade c covering
                                 * side 2^c; aabb_scale >= 2 marches with cone-angle 1/256 steps */
    float render_aabb[6];       /* Testbed.render_aabb: lo xyz, hi xyz in ngp coordinates — rays start where they
                                 * enter it and stop where they leave it; all zeros = the model's whole box */
} d2r_nerf_desc;

/* replaces Testbed(mode=Nerf) + load_snapshot */
D2R_API int d2r_nerf_create(d2r_ctx *ctx, const d2r_nerf_desc *desc, d2r_nerf **out);
D2R_API void d2r_nerf_destroy(d2r_nerf *m);

/*
 * replaces Testbed(mode=Nerf) + load_snapshot(path) on the bytes of an instant-ngp `.ingp` file (reference
 * reconstruction/ngp_visual_model.py:24-28): zlib/gzip msgpack -> level table, fp16 tables and MLPs, occupancy
 * bitfield (instant-ngp's threshold rule and cascade max-pool), render_aabb -> d2r_nerf_create.  `info` / `views`
 * (optional) receive what a Testbed keeps beside the model: dataset scale/offset for nerf_matrix_to_ngp, the saved
 * background colour, per-training-view intrinsics AND lens for set_camera_to_training_view.
 * The layout is the BELIEVED one (no instant-ngp file or source offline), so nothing is defaulted: every key the loader
 * needs must be there with the right msgpack kind and size (params_binary: fp16, density MLP | colour MLP | hash tables;
 * density_grid_binary: fp16 128^3 per cascade), every key that changes the rendered function must carry the value the
 * kernels implement (activations, interpolation, SH degree, exposure 0, no envmap / extra dims / rotated crop box, a
 * perspective or OpenCV lens per view, cone angle tied to aabb_scale), unknown keys inside encoding / network / rgb_network / dir_encoding
 * are refused; each failure returns D2R_ERR_INVALID / D2R_ERR_UNSUPPORTED with a d2r_last_error message naming the key.
 */
/* Lens of a training view (instant-ngp's Lens {mode, params}) as this path meets it.  The reference renders every frame after
 * set_camera_to_training_view (reconstruction/combined_rendering.py:98,116), which switches
 * nerf.render_with_lens_distortion on and makes the view's lens the render lens; its configs carry OpenCV coefficients
 * (configs/shopping_demo.json:51-56 -> the transforms the NeRFs are trained from, reconstruction/train_ngp.py:171-180,
 * utils/accio2ngp.py:47-56; train_ngp.py:70 sets the flag as well).  Other lens models (fisheye, f-theta, lat-long,
 * equirectangular, orthographic) are refused by the loader with D2R_ERR_UNSUPPORTED naming the view. */
enum { D2R_LENS_PERSPECTIVE = 0, D2R_LENS_OPENCV = 1 };
typedef struct {
    double fx, fy, cx, cy;   /* pixels at the training resolution */
    uint32_t w, h;
    uint32_t lens_mode;      /* D2R_LENS_*: metadata[].lens (no lens / an empty one = perspective) */
    float lens_params[4];    /* OpenCV k1, k2, p1, p2 */
} d2r_ingp_view;
typedef struct {
    uint32_t n_levels, n_features, aabb_scale;
    int32_t has_background;
    double dataset_scale, dataset_offset[3];
    float background_color[4];
    uint32_t n_views;            /* training views in the snapshot */
    uint32_t n_views_written;    /* how many of them went into `views` (at most views_cap) */
    uint32_t n_unknown_keys;     /* keys of the snapshot the loader neither reads, checks nor knows to be irrelevant to
                                  * rendering (d2r_ingp_inspect lists them with a '?') */
    int32_t render_with_lens_distortion;   /* snapshot.nerf.render_with_lens_distortion when the file carries it (else 0): the
                                  * Testbed's flag BEFORE the first set_camera_to_training_view, which sets it to 1 (ABI 9) */
} d2r_ingp_info;
D2R_API int d2r_nerf_load_ingp(d2r_ctx *ctx, const void *bytes, size_t len, d2r_nerf **out, d2r_ingp_info *info,
                               d2r_ingp_view *views, uint32_t views_cap);
/*
 * What a snapshot holds next to what d2r_nerf_load_ingp reads of it — the first check to run on a real
 * `method_out/<scene>/{fg,bg}_base.ingp` (reference install.sh:38-50), since the loader is written against the believed
 * layout.  HOST ONLY: needs no device and no context (errors go to d2r_last_error(NULL)).  Writes NUL-terminated text
 * into out[cap] (truncated if short; *needed = bytes for all of it): one line per leaf of the msgpack tree,
 * "<R|C|-|?> <kind> <elements or bytes> <path> [= value]" with R = read by the loader, C = checked (changes the rendered
 * function; one value implemented, anything else is a load error), - = known not to affect rendering (training state,
 * GUI camera, ...), ? = unknown to the loader; then "# unknown_keys N" and "# derived:" lines with the
 * parameter / density-grid counts and the level table the loader computes from the config, beside the sizes of
 * params_binary / density_grid_binary.  Malformed or truncated input returns D2R_ERR_INVALID.
 */
D2R_API int d2r_ingp_inspect(const void *bytes, size_t len, char *out, size_t cap, size_t *needed);
/* HOST ONLY: every check d2r_nerf_load_ingp makes on the bytes, without a device and without creating a model — 0 when the
 * loader would take the snapshot, else the loader's error (message in d2r_last_error(NULL), naming the key).  info
 * (optional) is filled as the loader would fill it. */
D2R_API int d2r_ingp_validate(const void *bytes, size_t len, d2r_ingp_info *info);

/* Camera state set on a Testbed before render(): set_camera_to_training_view (intrinsics),
 * background_color, nerf.render_min_transmittance, dataset scale/offset used by
 * set_nerf_camera_matrix (reference combined_rendering.py:98-105,116,123-127). */
typedef struct {
    uint32_t width, height;
    float focal[2];          /* pixels at this render size (rel. focal length * height) */
    float center[2];         /* principal point, relative (cx/w, cy/h) */
    float scale;             /* dataset scale */
    float offset[3];         /* dataset offset */
    float background[4];     /* Testbed.background_color RGBA */
    float min_transmittance; /* 0.01 */
    float near_distance;     /* 0 */
    /* ABI 9 — the render lens: what set_camera_to_training_view leaves in nerf.render_lens when
     * nerf.render_with_lens_distortion is on (D2R_LENS_PERSPECTIVE otherwise).  With D2R_LENS_OPENCV every ray's camera-space
     * direction (x, y, 1) goes through instant-ngp's iterative OpenCV undistortion (Newton steps on a central-difference
     * Jacobian, at most 100, |step|^2 < 1e-10) before the camera rotation; the rectangle cull of the composite passes stays
     * conservative under it (frames are bit-identical with "raygen_rect" 0 and 1). */
    uint32_t lens_mode;
    float lens_params[4];    /* k1, k2, p1, p2 */
} d2r_view;

/*
 * replaces n x { set_nerf_camera_matrix(cam); render_mode=Shade; render(w,h,1,True);
 *                render_mode=Depth; render(w,h,1,True) }   (combined_rendering.py:123-130)
 * in one pass.  cams_nerf: host [n][12], row-major 3x4, the matrix handed to
 * set_nerf_camera_matrix.  rgba_out: host [n][h][w][4] Shade frames; depth_out: host
 * [n][h][w] channel 0 of the Depth frames.  Either output may be NULL.
 * n_samples_out (optional): network evaluations performed.
 */
D2R_API int d2r_render(d2r_ctx *ctx, const d2r_nerf *model, const d2r_view *view,
                       const float *cams_nerf, uint32_t n, float *rgba_out, float *depth_out,
                       uint64_t *n_samples_out);

/* Parity hook for the lens: the camera-space direction (x, y) — z = 1 — of every pixel centre of `view` after the iterative
 * OpenCV undistortion, i.e. what the ray generators rotate by the camera matrix.  dirs_out: host [h][w][2].  The view must carry
 * a lens (lens_mode D2R_LENS_OPENCV).  (ABI 9) */
D2R_API int d2r_lens_undistort_view(d2r_ctx *ctx, const d2r_view *view, float *dirs_out);

/* Field evaluation at arbitrary unit-cube points (parity hook for the hash-grid encode and
 * both MLPs): xyz, dirs host [n][3] (dirs unit length); out host [n][4] = sigma, r, g, b
 * with rgb the network's sRGB-space prediction. */
D2R_API int d2r_nerf_eval_points(d2r_ctx *ctx, const d2r_nerf *model, const float *xyz,
                                 const float *dirs, uint32_t n, float *sigma_rgb_out);

/* ------------------------------------------------- background + compositing */

/* Fixes the per-view background the candidates are composited over: bg_image / bg_depth
 * of reference combined_rendering.py:105-113 (host [h][w][4] and [h][w]; depth is
 * channel 0, already rectified/masked if it came from depths_gt). */
D2R_API int d2r_set_background(d2r_ctx *ctx, const d2r_view *view, const float *bg_rgba,
                               const float *bg_depth);

/*
 * Sensor-depth background of a render view (reference combined_rendering.py:107-110 with rectify_depth :166-187 and
 * rectify_mask :189-209): depth (host, [src_h][src_w] metres, fp32 or fp16 as data_loader.py:43,58 stores it) and
 * the movable-object mask (host uint8 [src_h][src_w], 0 / 1; NULL = no masking) are centre-cropped to a square and
 * resized to w x h as cv2.resize(..., interpolation=cv2.INTER_CUBIC) does (float path for the depth, 8-bit
 * fixed-point path for the mask); where the resized mask is 0 the depth becomes 100.  depth_out: host [h][w] fp32,
 * what d2r_set_background takes as bg_depth; mask_out (optional): host [h][w] uint8, the resized mask.
 */
D2R_API int d2r_rectify_background_depth(d2r_ctx *ctx, const void *depth, int depth_is_fp16, const uint8_t *mask,
                                         uint32_t src_w, uint32_t src_h, uint32_t w, uint32_t h, float *depth_out,
                                         uint8_t *mask_out);

/*
 * replaces the body of renderer.render's loop over valid poses
 * (reference combined_rendering.py:118-155 with convert_virtual_pose :250-263):
 *   obj_pose_now  host [16]    T_WO_1, row-major 4x4, NGP convention (after converter)
 *   cam_pose      host [16]    T_WC_1 of the render view, NGP convention
 *   obj_poses     host [K][16] candidate poses T_WO_2, NGP convention
 *   frames_out    host [K][h][w][3] uint8 composited sRGB frames
 */
D2R_API int d2r_render_composite(d2r_ctx *ctx, const d2r_nerf *fg, const d2r_view *view,
                                 const float *obj_pose_now, const float *cam_pose,
                                 const float *obj_poses, uint32_t K, uint8_t *frames_out);

/* -------------------------------------------------------------------- CLIP */

typedef struct {
    uint32_t image_size;   /* S: 224 / 336 */
    uint32_t patch_size;   /* P: 16 / 14 */
    uint32_t hidden_size;  /* d: 768 / 1024 */
    uint32_t num_layers;   /* 12 / 24 */
    uint32_t num_heads;    /* 12 / 16 (head dim must be 64) */
    uint32_t mlp_size;     /* 3072 / 4096 */
    uint32_t proj_dim;     /* D: 512 / 768 */
} d2r_clip_desc;

/*
 * replaces CLIPModel.from_pretrained(...).to(device) (vision tower + visual projection,
 * reference clip_scoring.py:150).  weights: host fp32 blob, tensors concatenated in this
 * order (Hugging Face names; Linear weights row-major [out][in]):
 *   patch_embedding.weight [d][3*P*P], class_embedding [d], position_embedding [T][d],
 *   pre_layrnorm.{weight,bias},
 *   per layer: layer_norm1.{weight,bias}, q_proj.{weight,bias}, k_proj.{weight,bias},
 *              v_proj.{weight,bias}, out_proj.{weight,bias}, layer_norm2.{weight,bias},
 *              fc1.{weight,bias}, fc2.{weight,bias},
 *   post_layernorm.{weight,bias}, visual_projection.weight [D][d]
 * n_floats must equal the size this order implies.
 */
D2R_API int d2r_clip_create(d2r_ctx *ctx, const d2r_clip_desc *desc, const float *weights,
                            size_t n_floats, d2r_clip **out);
D2R_API void d2r_clip_destroy(d2r_clip *clip);

/*
 * replaces np.rot90 (clip_scoring.py:145) + CLIPProcessor(images=...) (:177) +
 * CLIPModel vision forward and logits_per_image (:180-181) for frames already on the host:
 *   frames       host [n][h][w][3] uint8
 *   rot90        non-zero: rotate each frame 90 degrees CCW first
 *   text_embeds  host [C][D], L2-normalised text embeddings (cached, computed once)
 *   logit_scale  exp(logit_scale) of the checkpoint (100 for OpenAI CLIP)
 *   logits_out   host [n][C]   logits_per_image
 *   embeds_out   host [n][D]   optional, L2-normalised image embeddings
 */
D2R_API int d2r_clip_score_frames(d2r_ctx *ctx, const d2r_clip *clip, const uint8_t *frames,
                                  uint32_t n, uint32_t w, uint32_t h, int rot90,
                                  const float *text_embeds, uint32_t C, float logit_scale,
                                  float *logits_out, float *embeds_out);

/* CLIPProcessor(images=...) alone: pixel_values host [n][3][S][S] fp32 (parity hook). */
D2R_API int d2r_clip_preprocess(d2r_ctx *ctx, const d2r_clip *clip, const uint8_t *frames,
                                uint32_t n, uint32_t w, uint32_t h, int rot90,
                                float *pixel_values_out);

/* CLIPModel vision forward on given pixel_values host [n][3][S][S] -> embeds [n][D]
 * (parity hook for the ViT alone). */
D2R_API int d2r_clip_embed_pixels(d2r_ctx *ctx, const d2r_clip *clip, const float *pixel_values,
                                  uint32_t n, float *embeds_out);

/*
 * Parity hook for the vision tower's fp8 mode (option "vit_fp8", below): ONE product C = q(A) q(W)^T s_w + bias through the kernels
 * the mode uses — activations as OCP e4m3 with one E8M0 scale byte per (row, 64 columns), the bf16-rounded weights as e4m3 with one
 * power-of-two scale per matrix, fp32 accumulation on v_mfma_scale_f32_32x32x64_f8f6f4 (oracle/clip_fp8.py restates the format).
 *   A host [M][K], W host [N][K], bias host [N] fp32; N and K multiples of 256
 *   kind 0: out [M][N] = the bf16 result; kind 1: out = quick_gelu(...) quantised to e4m3 per (row, 64 columns), dequantised
 *   a_q8 [M][K] / a_scales [M][K/64] (optional): the quantised A;  w_scale_out (optional): s_w
 *   out_q8 [M][N] / out_scales [M][N/64] (kind 1, optional): the raw bytes of the result
 */
D2R_API int d2r_debug_gemm_fp8(d2r_ctx *ctx, const float *A, const float *W, const float *bias, uint32_t M, uint32_t N,
                               uint32_t K, int kind, float *out, uint8_t *a_q8, uint8_t *a_scales, float *w_scale_out,
                               uint8_t *out_q8, uint8_t *out_scales);

/* ------------------------------------------------------------- text tower */

typedef struct {
    uint32_t vocab_size;      /* 49408 */
    uint32_t context_length;  /* 77 */
    uint32_t hidden_size;     /* 512 / 768 (head dim must be 64) */
    uint32_t num_layers;      /* 12 */
    uint32_t num_heads;       /* 8 / 12 */
    uint32_t mlp_size;        /* 2048 / 3072 */
    uint32_t proj_dim;        /* D */
} d2r_text_desc;
typedef struct d2r_text d2r_text;

/*
 * replaces the text tower of CLIPModel (reference clip_scoring.py:150,180).  weights: host fp32
 * blob in this order (Hugging Face names): token_embedding.weight [V][d],
 * position_embedding.weight [ctx][d], per layer the same 16 tensors as d2r_clip_create,
 * final_layer_norm.{weight,bias}, text_projection.weight [D][d].
 */
D2R_API int d2r_text_create(d2r_ctx *ctx, const d2r_text_desc *desc, const float *weights,
                            size_t n_floats, d2r_text **out);
D2R_API void d2r_text_destroy(d2r_text *text);
/*
 * input_ids host [C][T] int32 (tokenised captions, EOS = largest id) -> embeds_out host [C][D],
 * L2-normalised: the cached text embeddings d2r_clip_score_frames / d2r_render_score take.
 * The reference re-encodes the captions for every image batch (clip_scoring.py:176-180); here the
 * caller does it once per task.
 */
D2R_API int d2r_text_encode(d2r_ctx *ctx, const d2r_text *text, const int32_t *input_ids, uint32_t C,
                            uint32_t T, float *embeds_out);

/* --------------------------------------------------- the fused hot path */

/*
 * Pose batch in, logits out: HOT LOOP A + HOT LOOP B of reference clip_scoring.py:136-185
 * with nothing but poses and logits crossing PCIe.  Needs d2r_set_background first.
 *   obj_poses_dev  DEVICE [K][16] fp32 candidate poses T_WO_2 (NGP convention)
 *   text_embeds    host [C][D]
 *   logits_dev     DEVICE [K][C] fp32
 *   frames_out     host [K][h][w][3] uint8, optional (NULL in benchmark mode)
 * Asynchronous on the context's stream when frames_out is NULL; call
 * d2r_ctx_synchronize (or synchronise the caller-owned stream) before reading logits_dev.
 * K is processed in chunks ("chunk" option); the render half of a chunk runs on a second, library-owned stream that
 * forks from and joins the context's stream inside the call ("overlap" option).
 */
D2R_API int d2r_render_score(d2r_ctx *ctx, const d2r_nerf *fg, const d2r_clip *clip,
                             const d2r_view *view, const float *obj_pose_now,
                             const float *cam_pose, const float *obj_poses_dev, uint32_t K,
                             const float *text_embeds, uint32_t C, float logit_scale,
                             float *logits_dev, uint8_t *frames_out);

/*
 * Where the composited frames of a pass go besides (or instead of) the caller's array: the files the reference's
 * renderer writes inside its loop, `cb_render/cb_rgb_%04d.png` (reference reconstruction/combined_rendering.py:157-159),
 * which a later run re-scores with use_cache_renders (clip_scoring.py:89-104).  The library encodes them on a pool of
 * host threads while the GPU works on the next chunk.
 */
typedef struct {
    const char *png_dir;        /* existing directory for cb_rgb_%04d.png; NULL = write no files */
    uint32_t png_first_index;   /* file index of candidate 0 (a pose shard passes its first global render index) */
    int32_t png_threads;        /* encoder threads; 0 = the CPUs the process may use (hardware threads capped by the container's CPU quota), at most 64 */
    int32_t png_level;          /* negative = the default: Sub-filtered scanlines (cv2.imwrite's filter), Huffman-only deflate;
                                   0..9 = unfiltered scanlines at that zlib level (PNG is lossless: this only trades time for size) */
} d2r_frame_sink;

/*
 * The same pass for a caller that holds HOST memory — what the Python host's optimise_pose_grid / renderer call
 * (reference clip_scoring.py:136-185: `renderer.render(...)`, then the CLIP batches): candidate poses in, logits out,
 * frames kept on the GPU unless asked for.  Synchronous.
 *   obj_poses    host [K][16] fp32 candidate poses T_WO_2 (NGP convention)
 *   logits_out   host [K][C]
 *   frames_out   host [K][h][w][3] uint8, optional
 *   sink         optional: PNG files of the frames (streamed chunk by chunk; the host never holds more than two chunks
 *                of at most 1 GiB each in the library's pinned staging buffers)
 */
D2R_API int d2r_render_score_host(d2r_ctx *ctx, const d2r_nerf *fg, const d2r_clip *clip,
                                  const d2r_view *view, const float *obj_pose_now, const float *cam_pose,
                                  const float *obj_poses, uint32_t K, const float *text_embeds, uint32_t C,
                                  float logit_scale, float *logits_out, uint8_t *frames_out,
                                  const d2r_frame_sink *sink);

/* ------------------------------------------------- frame files (host only: no device, no context) */

/* One uint8 RGB image [h][w][3] -> an 8-bit RGB PNG file (best_render.png, reference clip_scoring.py:222-223).  level: see
 * d2r_frame_sink.png_level (negative = the default encoding). */
D2R_API int d2r_png_write(const uint8_t *rgb, uint32_t w, uint32_t h, const char *path, int level);
/* frames host [n][h][w][3] -> <dir>/cb_rgb_%04d.png for indices first_index .. first_index+n-1, encoded on `threads`
 * host threads (0 = auto): what renderer.render(save=True) leaves behind (combined_rendering.py:157-159). */
D2R_API int d2r_png_write_batch(const uint8_t *frames, uint32_t n, uint32_t w, uint32_t h, const char *dir,
                                uint32_t first_index, int threads, int level);
/* The same for frames that equal `background` ([h][w][3]) in most scanlines — the frames of a render-and-score pass, where a candidate's
 * object covers a band of the frame: the background's scanlines are entropy-coded once and a frame re-codes only the scanlines that differ
 * (default encoding only; identical pixels, files a few per cent larger).  d2r_render_score_host's frame sink writes its files this way. */
D2R_API int d2r_png_write_batch_bg(const uint8_t *frames, uint32_t n, uint32_t w, uint32_t h, const uint8_t *background, const char *dir,
                                   uint32_t first_index, int threads);
/* The reverse, for use_cache_renders (clip_scoring.py:95-104): n files of w x h -> frames_out host [n][h][w][3]; file i is
 * cb_rgb_%04d.png of indices[i], or of first_index + i when indices is NULL.  Reads 8-bit grey / RGB PNGs with or without
 * alpha, every scanline filter (what cv2.imwrite and PIL write); a file of another size, a missing file or an
 * unsupported format is an error naming the file. */
D2R_API int d2r_png_read_batch(const char *dir, const uint32_t *indices, uint32_t first_index, uint32_t n, uint32_t w,
                               uint32_t h, uint8_t *frames_out, int threads);
D2R_API int d2r_png_size(const char *path, uint32_t *w, uint32_t *h);
/* np.savetxt(path, data) with numpy's defaults ('%.18e', ' ', '\n'), byte for byte: the format of goal_pose.txt,
 * pose_batch.txt and pose_scores.txt (reference dream2real.py:356-358).  data host [rows][cols] fp64 (a 1-D array is
 * rows x 1: one number per line); formatted in row blocks on `threads` host threads (0 = auto). */
D2R_API int d2r_savetxt(const char *path, const double *data, uint64_t rows, uint64_t cols, int threads);

/* Counters of the last d2r_render / d2r_render_composite / d2r_render_score call, for
 * roofline accounting (bench.py): rays generated, rays that reached occupied space,
 * network evaluations (hash-grid samples). */
typedef struct {
    uint64_t rays_total;
    uint64_t rays_alive;
    uint64_t samples;
    uint64_t wave_iters;   /* marcher wave-iterations; lane utilisation = samples / (64 * wave_iters) */
    uint64_t l0_tokens;    /* d2r_render_score with "l0_reuse": patch tokens of the pass (0 when the reuse did not run) ... */
    uint64_t l0_touched;   /* ... and how many of them were recomputed (the others took the background's layer-0 rows) */
} d2r_render_stats;
D2R_API int d2r_get_render_stats(d2r_ctx *ctx, d2r_render_stats *out);
/* After an asynchronous d2r_render_score over K poses: synchronises the stream and gathers
 * the per-chunk device counters into the stats d2r_get_render_stats returns. */
D2R_API int d2r_collect_render_stats(d2r_ctx *ctx, uint32_t K);

/* Per-kernel device time of the calls made since timing was switched on with
 * d2r_ctx_set_option(ctx, "timing", 1): HIP events recorded on the launch stream around the
 * ray-march kernel, the ray-generation kernel, the CLIP preprocess kernel and the CLIP
 * forward (all its kernels).  d2r_get_timing synchronises the stream, sums the elapsed
 * times and resets the event list. */
typedef struct {
    double march_ms;   uint64_t march_launches;
    double raygen_ms;  uint64_t raygen_launches;
    double prep_ms;    uint64_t prep_launches;
    double clip_ms;    uint64_t clip_launches;   /* one "launch" = one forward over a chunk */
    /* ABI 9 */
    double sort_ms;    uint64_t sort_launches;   /* the ray sort's passes (k_sort_*), one "launch" = one sort; NOT part of raygen_ms */
    /* "timing" 2 only (an event pair per kernel launch: a few tenths of a per cent of a step, so not for timed regions): the
     * vision tower's full-size products of the default schedule — LayerNorm-folded QKV, streamed attention, out-projection,
     * fc1 (+ quick_gelu), fc2; layer 0's compact QKV under "l0_reuse", the class-token-only last block, row statistics, patch
     * embedding and head are clip_ms minus these five */
    double vit_qkv_ms;  uint64_t vit_qkv_launches;
    double vit_attn_ms; uint64_t vit_attn_launches;
    double vit_out_ms;  uint64_t vit_out_launches;
    double vit_fc1_ms;  uint64_t vit_fc1_launches;
    double vit_fc2_ms;  uint64_t vit_fc2_launches;
} d2r_timing;
D2R_API int d2r_get_timing(d2r_ctx *ctx, d2r_timing *out);

/* Tunables; unknown keys return D2R_ERR_INVALID.
 * "chunk" (default 4096, 1..16384): candidates / images per pass; the library lowers it per model and
 *     view so that one pass stays inside the 32-bit indexing of the ray queue and the GEMM outputs.
 * "refill_min" (default 64, 1..64): free lanes a marcher wave accumulates before it takes new rays
 *     from the queue (64 = a wave runs its 64 rays to the end).
 * "ray_sort" (default 1): before the march the ray queue is sorted (three small counting-sort passes) by the cell of
 *     the object's occupied box a ray's first sample lies in — 2^"ray_sort_log2" (default 4, 1..4) cells per axis,
 *     Morton order: every candidate renders the same object, so the waves running at one time then read the same few
 *     regions of the level tables / bricks.  Same pixels; 0 marches the rays in generation order.
 * "march_threads" (default 0 = auto; else a multiple of 64 up to the compiled 768 — larger values are refused): threads per marcher
 *     workgroup (one workgroup per CU).  Auto: 768 (three waves per SIMD); with "ray_sort" 0: 512 where the HBM
 *     bricks exceed "march_threads_auto_mib" (default 64) MiB — the unsorted marcher is bound by the L2-miss path
 *     there and fewer waves thrash less.  Read-only: "march_threads_used", "march_hbm_brick_bytes" (of the last march launch).
 * "march_compact" (default 1): once a marcher wave has no more than 32 rays left it moves them to its
 *     lanes 0..31, so that the second 32-sample tile of its iterations costs nothing (same pixels).
 * "bricks" (default 1): serve the de-hashed coarse levels of small models from LDS; 0 forces every
 *     level through the global tables.  Behind the LDS slots, further slots are served from de-hashed dense bricks in HBM:
 *     "gbrick_slots" (default 8, 0..8) caps how many, "brick_slots_total" (default 7, 0..8) the first slot that is never
 *     bricked (the finest one measured slower).  "raygen_rect" (default 1): composite mode generates rays only inside the
 *     projected occupied bounding box.  Results are bit-identical whatever these are set to.
 *     Read at d2r_nerf_create / d2r_nerf_load_ingp time (set them BEFORE creating the model): "lds_slots_max" (default 5,
 *     0..5): at most this many leading slots as LDS bricks; "gbrick_max_mib" (default 512, 0..512): a slot gets an HBM brick
 *     only while that brick stays below this size (the bricks of a model total at most 512 MiB).
 * "mlp_f16" (default 1 since round 6): operand type of the NeRF MLPs' MFMAs, fp32 accumulation either way, same MFMA rate.  1 = fp16: the
 *     reference's operand type (tiny-cuda-nn's fully fused MLPs are __half; BASELINE.json configs[4] names an "fp16 render") — the
 *     snapshot's fp16 weights enter the MFMA unrounded, features and activations keep 11 significant bits; activations must stay below
 *     65504, as in the reference.  0 = bf16 (north_star's wording: 8 significant bits).  The default follows the measurement: against an
 *     emulation of tiny-cuda-nn's half-accumulating arithmetic on a trained-like field the fp16-operand marcher sits where the fp32
 *     specification sits (|dlog sigma| 0.032 vs 0.030, no object pixel off by more than one LSB), the bf16-operand one twice as far
 *     (0.064, 9 % of the object's pixels) — DESIGN.md section 5.
 * "render_arith" (0 default, 1, 2): arithmetic of the NeRF field evaluation, honoured by every entry point that marches (d2r_render,
 *     d2r_render_composite, d2r_render_score, d2r_render_score_host) and by d2r_nerf_eval_points.  0: the specification — fp16
 *     tables and weights, fp32 accumulation.  1: tiny-cuda-nn's half arithmetic as oracle/d2r_oracle.c emulates it
 *     (d2r_oracle_set_arith(1)): the hash grid's eight corner terms summed in half, acc = half(acc + half(w v)) in corner order; both
 *     MLPs with half accumulators, one rounding per 16-wide k-step (one fp16 MFMA from a zero accumulator, then a convert), half
 *     activations and half network outputs; exp and sigmoid stay fp32.  2: the same with the grid's newer form,
 *     acc = half(fma(half(w), v, acc)).  The grid part restates the emulation operation by operation; the MLPs sum a k-step's 16
 *     products in the MFMA's order, not the emulation's, so a rounding that sits on a tie can fall the other way (DESIGN.md
 *     section 5).  With 1 / 2 the MLP operands are fp16 whatever "mlp_f16" says: the half arithmetic has no bf16 form.  A
 *     validation mode for telling arithmetic apart from other differences against a reference run's frames
 *     (tools/validate_artifacts.py --search-forks): brick-free kernels, slower than 0.  Values outside 0..2 are
 *     refused (D2R_ERR_INVALID) and the stored value stays.
 * "ln_fold" (default 4): schedule of the vision tower.  0: LayerNorm kernels between the GEMMs, fp32 residual
 *     stream.  1-3: LayerNorm folded into the QKV / fc1 GEMMs (LN(x) W^T + b = rstd (x (gamma o W)^T - mean
 *     colsum) + b'), row statistics emitted by the residual GEMMs' epilogues, which also write the bf16 operand
 *     copy of the residual row; the residual stream itself is kept as 1: two bf16 arrays hi + lo (16 mantissa
 *     bits), 2: one bf16 array (fastest; its accumulated rounding puts the logit error past 1e-3 of the logit
 *     scale in the tail, so it is not the default), 3: fp32 next to the bf16 copy, 4 (default): bf16 hi + ONE lo byte per
 *     element — the next 8 bits of the fp32 bit pattern, rounded (16 significant bits like 1, a quarter less residual
 *     traffic; measured logit error 4.2e-4 of the scale on 300 images against 5.1e-4 for 1, CLIP time -1.3 %).
 * "cls_last" (default 1): the last transformer block of the vision tower runs on the class-token rows only (the head
 *     reads nothing else; same result, ~6 % less ViT work).  "gemm_nsplit" (default 0 = 2 where the column tiles and
 *     XCDs divide evenly; 1 = off): XCD sets own column sections of the persistent GEMM's outputs so that a section's
 *     weight panels stay in their L2s; results do not depend on it.
 * "prep_reuse" (default 1): in d2r_render_score, the rows of CLIP patches of a candidate frame that its object cannot have
 *     touched (outside the rectangle its rays are generated in) are copied from the background frame's own patches,
 *     computed once per d2r_set_background; bit-identical to resampling them.
 * "attn_rem" (default 1, 0..4): vision-tower attention on a sequence of 8 g + r query tiles of 32: a remainder of at most this
 *     many tiles runs on workgroups of r waves (each staging whole key tiles itself) instead of one more eight-wave
 *     workgroup with 8 - r idle waves; 257 tokens (r = 1): -7 % kernel time, 577 tokens (r = 3): neutral.  Bit-identical.
 * "overlap" (default 0): 1 = d2r_render_score / d2r_render_score_host run the render half of chunk i+1 (cameras, ray
 *     generation, march, preprocess) on a second stream while the ViT scores chunk i; 0 = one stream, in program order.
 *     Results do not depend on it; measured neutral on MI355X (the marcher and the persistent GEMMs each fill whole CUs —
 *     LDS and registers — so the two streams time-share the CUs: DESIGN.md section 4).  Frames that leave the GPU are
 *     copied on their own stream under the ViT either way.  "march_blocks" (default 0 = one per CU): workgroups of the persistent marcher.
 * "l0_reuse" (default 1): in d2r_render_score / d2r_render_score_host, a candidate's patches whose resampling footprint lies outside the
 *     rectangle its rays were generated in are the background's own patches, so their patch embedding, pre-LayerNorm residual row
 *     and layer-0 q / k / v rows are broadcast from rows computed once per background, and the patch-embedding and layer-0 QKV
 *     products run on the touched tokens only (needs "ln_fold" 4, "prep_reuse" and "raygen_rect" on, at most 1024 patches
 *     per image).  Bit-identical logits; configs[1]: 17 % of the tokens touched, CLIP -2.1 ms per 4096 candidates.
 * "vit_fp8" (default 0): 1 = the four Linear products of every transformer block except the first (when its rows are reused, "l0_reuse")
 *     and the class-token-only last one run on the MX-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, twice the bf16 MFMA rate):
 *     activations quantised to OCP e4m3 with one power-of-two scale per (row, 64 columns), weights to e4m3 with one power-of-two scale
 *     per matrix, fp32 accumulation; residual stream, LayerNorm statistics, q / k / v and attention arithmetic unchanged.  This is the
 *     "fp8 MFMA ViT" BASELINE.json configs[4] names.  It is NOT within north_star's 1e-3 cosine of the fp32 reference (measured
 *     in tests/test_fp8.py and DESIGN.md section 7) — which is why it is off unless asked for.  Runs for models whose hidden and MLP sizes are
 *     multiples of 256 under "ln_fold" 4 (ViT-B/16, ViT-L/14: yes); any other model or residual mode stays in bf16.
 * "debug_fail_chunk" (default -1 = off): fault injection for the error path of a chunked pass — the NEXT d2r_render_score /
 *     d2r_render_score_host fails with D2R_ERR_DEVICE when it reaches this chunk index, exactly as if a launch of that chunk had
 *     failed (streams joined, worker pool drained, context usable afterwards), and the hook disarms itself (one-shot).
 * "timing" (0/1/2): record HIP events per kernel group for d2r_get_timing; 2 adds an event pair around every product of the vision tower.
 * Development builds of the library (make DEV=1) also know experiment switches — schedules that were measured no faster
 * and tile configurations kept for comparison; they are not part of this interface. */
D2R_API int d2r_ctx_set_option(d2r_ctx *ctx, const char *key, int64_t value);
/* Reads a tunable back (the keys of d2r_ctx_set_option), plus read-only facts about the last ray-march launch on this
 * context: "march_lds_slots" / "march_hbm_brick_slots" = the brick configuration it ran with (ABI 8). */
D2R_API int d2r_ctx_get_option(d2r_ctx *ctx, const char *key, int64_t *value);

/* ------------------------------------------------------ multi-GPU (one process per GPU) */

/*
 * The path's only collective: candidate poses are sharded in contiguous
 * blocks over the GPUs of a node and every rank needs ALL logits before spatially_smooth_heatmap
 * (reference vision_3d/geometry_utils.py:252-269) and the argmax (clip_scoring.py:218).  The reference
 * itself is single-GPU (README.md:27) and has no counterpart.  Implemented on RCCL (ncclAllGather
 * over xGMI), bound at run time; bootstrap is the caller's: rank 0 obtains an id blob and hands it to
 * the other ranks by any means (torch.distributed, MPI, a file).
 */
#define D2R_COMM_ID_BYTES 128
/* rank 0 only: fills id_out[D2R_COMM_ID_BYTES] (ncclGetUniqueId) */
D2R_API int d2r_comm_get_unique_id(void *id_out);
/* every rank, collectively: joins the communicator on the context's device (ncclCommInitRank).
 * world == 1 with a NULL id needs no RCCL: the gather degenerates to a device copy (with an id, a
 * one-rank RCCL communicator is created all the same). */
D2R_API int d2r_comm_init(d2r_ctx *ctx, const void *id_blob, int rank, int world);
D2R_API int d2r_comm_destroy(d2r_ctx *ctx);
/*
 *   local_dev   DEVICE [n_local] fp32: this rank's logits (K_local * C values; ranks with a shorter
 *               shard pad to the common n_local)
 *   global_dev  DEVICE [world][n_local] fp32, rank-major
 * Asynchronous on the context's stream, ordered after the d2r_render_score that produced local_dev.
 */
D2R_API int d2r_allgather_scores(d2r_ctx *ctx, const float *local_dev, size_t n_local, float *global_dev);

/* ------------------------------------------ batched physics pre-filter */

/*
 * replaces the per-pose PyBullet loop of unsupcol_check (reference vision_3d/physics_utils.py:248-375), the
 * phys_check the path calls before rendering (clip_scoring.py:108-113, dream2real.py:304-326): duplicate
 * orientations (:260-278), optional regrasp rule (:281-301), then per pose collision (:314-321), support
 * (:329-340) and stability (:349-365).  Shapes are convex hulls given as vertex sets — PyBullet's GEOM_MESH
 * without the concave flag (:239) turns every shape (`o` / `g` group) of the mesh file into the convex hull of its
 * vertices, so a VHACD-decomposed object is a compound of convex parts; two bodies "collide / touch" when any pair
 * of their parts is in contact (GJK, one wavefront per pose), contact meaning the hulls come closer than the sum of
 * the two shapes' collision margins (d2r_phys_params.margin; 0 = plain hull intersection).
 *   movable_verts    host [movable_offsets[n_movable]][3]  the movable object's convex parts, concatenated, world
 *                    frame, at the object's initial pose (the reference's mesh files are written in world coordinates)
 *   movable_offsets  host [n_movable + 1]  first vertex of each movable part (movable_offsets[0] = 0)
 *   static_verts     host [static_offsets[n_static]][3]  convex parts of all static objects, concatenated
 *   static_offsets   host [n_static + 1]  first vertex of each static part
 */
typedef struct d2r_phys d2r_phys;
D2R_API int d2r_phys_create(d2r_ctx *ctx, const float *movable_verts, const uint32_t *movable_offsets, uint32_t n_movable,
                            const float *static_verts, const uint32_t *static_offsets, uint32_t n_static, d2r_phys **out);
D2R_API void d2r_phys_destroy(d2r_phys *phys);
typedef struct {
    uint32_t sample_res[6];   /* the pose grid's resolution: orientations per position = res[3] * res[4] * res[5] */
    float init_pose[16];      /* task_model.movable_obj.pose, row-major 4x4 (world) */
    float table_z;            /* scene_centre[2]: a pose below it counts as supported (:332-334) */
    float unsup_thresh;       /* 0.02: how far the object is lowered for the support test */
    float gravity[3];         /* GRAVITY_DIRECTION (0, 0, -1) */
    float perturb;            /* 0.04: sideways offset of the four stability probes */
    int32_t stability_check;  /* non-zero: run the stability probes */
    int32_t disallow_regrasp; /* non-zero: keep only orientations whose object z axis faces +z or -y (:281-301) */
    float margin;             /* collision margin of every convex part, metres: two parts are in contact when their hulls
                               * are closer than 2 * margin.  PyBullet loads GEOM_MESH convex hulls with a margin of 0.001
                               * (believed: its default collision margin for file-loaded convex shapes; PyBullet is not
                               * available offline, so this is unpinned); 0 = exact hull intersection */
} d2r_phys_params;
/*
 *   pose_batch  host [N][16] sampled poses (world, sample_poses_grid order: orientations fastest)
 *   valid_io    host [N] uint8: valid_so_far in, is_valid out
 */
D2R_API int d2r_phys_check(d2r_ctx *ctx, const d2r_phys *phys, const d2r_phys_params *params, const float *pose_batch,
                           uint32_t N, uint8_t *valid_io);

/* ------------------------------------------------- point-cloud ablation renderer (use_vis_pcds)
 *
 * replaces reference vision_3d/pcd_visual_model.py:98-155 (PointCloudRenderer.render: Open3D / Filament, one frame per
 * candidate, serially) behind clip_scoring.py:129-131.  The render rule is pinned in DESIGN.md section 2 instead of
 * Filament's rasteriser: pinhole projection u = fx x / z + cx, v = fy y / z + cy (pixel (row i, col j) centred at
 * (u, v) = (j, i)); points with z <= near are culled; a point covers the point_size x point_size pixels from
 * (ceil(u - point_size / 2), ceil(v - point_size / 2)); the nearest point wins, ties to the lower global index (background
 * points in cloud order, then movable points); its 8-bit colour is written unchanged, white where no point lands; then any
 * pixel whose three channels are all > 220 becomes (0, 0, 0) (reference :145-147).
 */
typedef struct d2r_pcd d2r_pcd;

/* A coloured point cloud on the context's device: xyz host [n][3] fp32, rgb host [n][3] uint8 (n may be 0). */
D2R_API int d2r_pcd_create(d2r_ctx *ctx, const float *xyz, const uint8_t *rgb, uint32_t n, d2r_pcd **out);
D2R_API void d2r_pcd_destroy(d2r_pcd *pcd);

typedef struct {
    uint32_t width, height;     /* 336 x 336 in the reference */
    float fx, fy, cx, cy;       /* INTRINSICS_CLIP_VIEW: 436.01158022, 435.90814372, 168, 168 */
    float point_size;           /* sprite side in pixels: a whole number 1 .. 16 (the reference's MaterialRecord: 3) */
    float near;                 /* points with camera-space z <= near are culled (believed value 0.01 m) */
} d2r_pcd_view;

/*
 * Parity hook: K frames to the host.
 *   cam_pose      host [16] fp32, row-major camera-to-world pose in the OpenCV convention (get_virtual_cam_poses(...)[0],
 *                 NOT passed through accio2ngp.converter); the camera's extrinsic is its rigid inverse
 *   obj_pose_now  host [16] the movable object's current pose O
 *   obj_poses     host [K][16] candidate poses P_k; the movable cloud moves by P_k inv(O), the background does not move
 *   frames_out    host [K][h][w][3] uint8
 * Per candidate the 3x4 matrix inv(cam_pose) P_k inv(O) is composed in fp64 (rigid inverses [R^T | -R^T t], each entry
 * summed over l = 0..3 in order), rounded to fp32; points then take fp32 multiply-adds ((m0 x + m1 y) + m2 z) + m3 per
 * row and a correctly rounded fp32 divide.  Synchronous.
 */
D2R_API int d2r_pcd_render(d2r_ctx *ctx, const d2r_pcd *bg, const d2r_pcd *movable, const d2r_pcd_view *view,
                           const float *cam_pose, const float *obj_pose_now, const float *obj_poses, uint32_t K,
                           uint8_t *frames_out);

/*
 * The fused pass of the ablation (reference clip_scoring.py:129-185): render the K candidates on the GPU and score them
 * (rot90 + CLIPProcessor + vision tower + logits_per_image), in the chunks d2r_clip_score_frames uses; the frames never
 * leave the device unless frames_out (host [K][h][w][3] uint8) is given.  Logits equal d2r_clip_score_frames(frames,
 * rot90 = 1) of the same frames.  Synchronous.
 */
D2R_API int d2r_pcd_render_score_host(d2r_ctx *ctx, const d2r_pcd *bg, const d2r_pcd *movable, const d2r_clip *clip,
                                      const d2r_pcd_view *view, const float *cam_pose, const float *obj_pose_now,
                                      const float *obj_poses, uint32_t K, const float *text_embeds, uint32_t C,
                                      float logit_scale, float *logits_out, uint8_t *frames_out);

/*
 * The ablation's visual clouds built on the device (reference vision_3d/pcd_visual_model.py:18-95, get_vis_pcds; the rule is
 * DESIGN.md section 2b, bullet "Clouds"): one call, every listed view, every listed object.
 *   rgb         host [n][h][w][3] uint8
 *   depth_u16   host [n][h][w] millimetres ((depth * 1000).astype(uint16) of the metric depth)
 *   labels      host [n][h][w] uint8 label image
 *   cam_poses   host [n][16] fp64 row-major camera-to-world poses, used as given (not inverted)
 *   K           host [9] fp64 intrinsics; bounds host [2][3] fp64 crop box, inclusive on both ends
 *   voxel       0: every surviving point in pixel order (pcds_type 0); > 0: each (object, view) segment voxel-downsampled
 *   views       host [n_views] frame indices, each < n; an object's cloud is its views' segments in this order
 *   obj_ids     host [n_objs] labels, each listed once
 *   out         host [n_objs] receives one handle per object (d2r_pcd_destroy each); d2r_pcd_render takes them as they are
 * A pixel with label L belongs to object L iff every in-frame pixel of the 15 x 15 window centred on it carries L and its depth
 * is not 0; z = (double)((float)d16 / 1000.0f), x = ((j - cx) z) / fx, y = ((i - cy) z) / fy, world_r = ((T[r][0] x + T[r][1] y) +
 * T[r][2] z) + T[r][3] in fp64; points outside the bounds are dropped.  With voxels, per segment: origin = min - voxel / 2, index =
 * floor((p - origin) / voxel), voxels in ascending (ix, iy, iz), each the fp64 sum of its points in pixel order divided by their
 * count and rounded to fp32, each colour channel floor(sum / count + 0.5).
 * Refused with D2R_ERR_INVALID before any device work: null or zero-size arguments, a view index >= n, an object id listed twice,
 * non-finite poses or intrinsics, a negative voxel, and bounds for which (max - min) / voxel + 2 needs more than 21 bits on an axis.
 * On any failure every out[] entry is NULL and nothing is left allocated.  Synchronous.
 */
D2R_API int d2r_pcd_build(d2r_ctx *ctx, const uint8_t *rgb, const uint16_t *depth_u16, const uint8_t *labels, uint32_t n, uint32_t w,
                          uint32_t h, const double *cam_poses, const double *K, const double *bounds, double voxel,
                          const uint32_t *views, uint32_t n_views, const uint8_t *obj_ids, uint32_t n_objs, d2r_pcd **out);
/* The number of points of a cloud; its points to the host: xyz [n][3] fp32, rgb [n][3] uint8 (both may be NULL when n is 0). */
D2R_API int d2r_pcd_size(const d2r_pcd *pcd, uint32_t *n);
D2R_API int d2r_pcd_read(d2r_ctx *ctx, const d2r_pcd *pcd, float *xyz, uint8_t *rgb);
/* Device-event times of the last d2r_pcd_build on this context: ms_out host [2] = upload, kernels (the three small count reads that
 * size the buffers included), milliseconds. */
D2R_API int d2r_pcd_build_get_timing(d2r_ctx *ctx, double *ms_out);

/* ------------------------------------------------- TSDF fusion of RGB-D frames into a triangle mesh (use_phys_tsdf)
 *
 * replaces the TSDF branch of reference vision_3d/physics_utils.py:58-115 (get_phys_models: Open3D VoxelBlockGrid on the
 * CPU, extract_triangle_mesh, crop, cluster removal, centre).  The rule is DESIGN.md section 2c; Open3D's defaults in it are
 * believed, not checked against Open3D.  State is a DENSE grid of (tsdf, weight) fp32 pairs over the bounds padded by
 * `trunc` and rounded out to whole blocks of 16^3 voxels; voxel g sits at g * voxel on every axis.
 */
typedef struct d2r_tsdf d2r_tsdf;

/* bounds: host [6] min xyz, max xyz.  voxel 0.002 and trunc 0.016 in the reference.  A volume of more than 2^31 voxels
 * (16 GiB of state) is refused with D2R_ERR_UNSUPPORTED and a message that starts "TSDF volume over the cap". */
D2R_API int d2r_tsdf_create(d2r_ctx *ctx, const float *bounds, float voxel, float trunc, d2r_tsdf **out);
D2R_API void d2r_tsdf_destroy(d2r_tsdf *vol);

/*
 * One frame, in call order.  depth_u16 host [h][w] millimetres, mask_u8 host [h][w] (non-zero = the object), intrinsics
 * host [9] row-major 3x3, cam_pose host [16] row-major camera-to-world, erode_k 1 .. 32 (1 = no erosion).
 * The mask is eroded by an erode_k x erode_k rectangle anchored at (k/2, k/2) (outside the frame counts as set); a pixel is
 * valid when it survives and 0 < z = u16 / 1000 <= 3.  Blocks a valid pixel's ray crosses for depths z - trunc .. z + trunc
 * in voxel steps are the frame's blocks; their voxels take tsdf = (w tsdf + t) / (w + 1), w += 1 with
 * t = min((z_pixel - z_cam) / trunc, 1) where the voxel projects (rounded to nearest) onto a valid pixel, z_cam > 0 and
 * z_pixel - z_cam >= -trunc.  A frame without a valid pixel changes nothing.  Synchronous.
 */
D2R_API int d2r_tsdf_integrate(d2r_tsdf *vol, const uint16_t *depth_u16, const uint8_t *mask_u8, uint32_t w, uint32_t h,
                               const float *intrinsics, const float *cam_pose, uint32_t erode_k);

/*
 * Parity hook: the blocks any frame touched, in (z, y, x) order.  *n_blocks holds the capacity of the buffers on entry and
 * the count on return; with all three buffers NULL only the count is returned.  block_coords host [n][3] (x, y, z of the
 * block, voxel 16 b .. 16 b + 15), tsdf / weight host [n][16][16][16] indexed [z][y][x].
 */
D2R_API int d2r_tsdf_read_voxels(d2r_tsdf *vol, uint32_t *n_blocks, int32_t *block_coords, float *tsdf, float *weight);

/*
 * Marching cubes over cubes whose eight corners all have weight >= weight_threshold (3 in the reference's setting), one
 * vertex per crossed edge at p0 + ((p1 - p0) t0) / (t0 - t1), vertices ordered by (z, y, x of the edge's lower voxel, axis),
 * triangles by (cube z, y, x, table order); then on the host the inclusive crop (host [6], NULL = none; a triangle survives
 * when its three vertices do, unreferenced vertices are dropped), clusters of triangles that share vertices, and
 * keep[t] = 0 for triangles of clusters smaller than cluster_keep (0.02) times the largest.  centre = mean of the vertex
 * array in fp64.  *n_vertices / *n_triangles: capacities on entry, counts on return; call once with every buffer NULL for
 * the counts, then again to fill (the result is kept in between).  vertices host [nv][3], triangles host [nt][3],
 * clusters host [nt], keep host [nt], centre host [3]; each may be NULL.  A volume without a surface is D2R_ERR_INVALID
 * ("seen in no frame").  Synchronous.
 */
D2R_API int d2r_tsdf_extract(d2r_tsdf *vol, float weight_threshold, const float *crop, double cluster_keep, uint32_t *n_vertices,
                             uint32_t *n_triangles, float *vertices, uint32_t *triangles, int32_t *clusters, uint8_t *keep,
                             double *centre);

/* mesh_concave_{id}.obj: "v %f %f %f" per vertex, "f a b c" (1-based) per triangle with keep[t] != 0 (keep NULL = all).
 * Vertices of dropped triangles stay in the file, as Open3D's remove_triangles_by_mask leaves them.  Host only. */
D2R_API int d2r_obj_write(const char *path, const float *vertices, uint32_t n_vertices, const uint32_t *triangles,
                          uint32_t n_triangles, const uint8_t *keep);
/* A Wavefront .obj -> vertices host [nv][3] fp32 and triangles host [nt][3] (0-based).  Reads `v x y z` and `f` lines; a face
 * index may be negative (counted back from the last vertex read so far) and may carry `/vt/vn` parts, which are ignored; a face of
 * more than three vertices becomes the fan (0, i, i + 1); `o` and `g` groups (one per convex part in VHACD's files) are
 * concatenated; every other line is skipped.  *n_vertices / *n_triangles: capacities on entry, counts on return; call once with
 * both buffers NULL for the counts, then again to fill.  A missing file, an unreadable number or an index out of range is
 * D2R_ERR_INVALID with a message that names the path (and the line).  A number is read as fp64 and rounded to fp32; the file
 * d2r_obj_write wrote reads back to exactly the numbers in it.  Host only. */
D2R_API int d2r_obj_read(const char *path, uint32_t *n_vertices, uint32_t *n_triangles, float *vertices, uint32_t *triangles);

/* ------------------------------------------------- pictures of the cost volume and the best pose
 *
 * replaces the windows of reference vision_3d/geometry_utils.py:137-206 (vis_cost_volume) and dream2real.py:392-400
 * (draw_geometries) with one frame: a triangle soup of coloured items, flat-shaded, and K score cubes drawn over it as a
 * maximum-intensity projection.  Every step of the rule is integer or IEEE-exact, so the frame is the same bytes on every call.
 *   view          d2r_pcd_view with d2r_pcd_render's limits (point_size is checked and otherwise unused); no lens
 *   cam_pose      host [16] fp32 row-major camera-to-world pose, OpenCV convention (rigid)
 *   verts         host [nv][3] fp32; tris host [nt][3] indices < nv; tri_item host [nt] item of each triangle, < n_items
 *   item_mats     host [n_items][16] fp32 row-major model matrices; item_rgb host [n_items][3]
 *   cube_centres  host [K][3] fp32 world frame; cube_half host [K] half-widths; cube_scores host [K], 0 = not drawn
 *   background    host [3] the colour of pixels nothing covers
 *   rgb_out       host [h][w][3]; ids_out host [h][w] or NULL: the winning triangle, -1 - cube where a cube shows, INT32_MIN
 *                 where nothing does
 * nt = 0 and K = 0 are valid.  D2R_ERR_INVALID, with the outputs untouched: a null array with a non-zero count, a view outside
 * the limits, a triangle index >= nv, a tri_item >= n_items.  Synchronous. */
D2R_API int d2r_mesh_render(d2r_ctx *ctx, const d2r_pcd_view *view, const float *cam_pose, const float *verts, uint32_t nv,
                            const uint32_t *tris, const uint32_t *tri_item, uint32_t nt, const float *item_mats,
                            const uint8_t *item_rgb, uint32_t n_items, const float *cube_centres, const float *cube_half,
                            const uint16_t *cube_scores, uint32_t K, const uint8_t *background, uint8_t *rgb_out, int32_t *ids_out);

/* ------------------------------------------------- the physics pre-filter straight from TSDF volumes
 *
 * A second backend of the pre-filter beside d2r_phys_*: no mesh and no convex parts.  All volumes of a scene are created
 * over the same bounds and so share one grid.  The static scene is one "touch" bit per voxel, the movable object the centres
 * of its observed solid voxels; a pose collides / is supported / is stable when any of its points lands on a set bit under
 * the probe translations of d2r_phys_check (the pose; lowered by unsup_thresh along gravity; the lowered pose pushed by
 * +-perturb along x, then y).
 */

/* The grid of a volume: b0 host [3] first block per axis (block b holds voxels 16 b .. 16 b + 15, voxel g sits at g * voxel),
 * nv host [3] voxels per axis (x, y, z). */
D2R_API int d2r_tsdf_grid(const d2r_tsdf *vol, int32_t *b0, uint32_t *nv, float *voxel, float *trunc);

/* touch[g] = weight[g] >= weight_threshold && tsdf[g] * trunc <= contact (fp32), packed along x: bit x & 31 of word x >> 5,
 * words_out host [nz][ny][ceil(nx / 32)].  The reference setting: weight_threshold 3, contact 0.002 (twice PyBullet's mesh
 * margin).  Unobserved voxels never touch.  Synchronous. */
D2R_API int d2r_tsdf_touch_bits(d2r_tsdf *vol, float weight_threshold, float contact, uint32_t *words_out);

/* The centres (float)g * voxel of the voxels with weight >= weight_threshold && tsdf <= 0 (the observed solid shell), in
 * (z, y, x) order.  *n_points: the capacity of xyz on entry, the count on return; xyz host [n][3], NULL = count only.  A
 * volume without such a voxel is D2R_ERR_INVALID ("seen in no frame").  Synchronous. */
D2R_API int d2r_tsdf_solid_points(d2r_tsdf *vol, float weight_threshold, uint32_t *n_points, float *xyz);

typedef struct d2r_sdfphys d2r_sdfphys;
/* words host [n_static_grids][nz][ny][ceil(nx / 32)]: the touch bits of the static objects, all on the grid (b0, nv, voxel);
 * they are ORed.  points host [n_points][3]: the movable object's points, world frame at its initial pose.  Refused with
 * D2R_ERR_INVALID: null pointers, no grid, no points, nv[a] = 0 or > 2^20, |b0[a]| > 2^19, more than 2^31 voxels. */
D2R_API int d2r_sdfphys_create(d2r_ctx *ctx, const int32_t *b0, const uint32_t *nv, float voxel, const uint32_t *words,
                               uint32_t n_static_grids, const float *points, uint32_t n_points, d2r_sdfphys **out);
D2R_API void d2r_sdfphys_destroy(d2r_sdfphys *h);
/* d2r_phys_check's arguments and verdict sequence.  params->margin is IGNORED: the contact distance was baked into the bits
 * (d2r_tsdf_touch_bits' contact).  params->init_pose must be rigid; T = pose inv(init_pose) is composed in fp64 with the
 * rigid inverse and rounded once.  A point whose voxel lies outside the grid, or is not finite, touches nothing. */
D2R_API int d2r_sdfphys_check(d2r_ctx *ctx, d2r_sdfphys *h, const d2r_phys_params *params, const float *pose_batch, uint32_t N,
                              uint8_t *valid_io);
/* Device-event times of the handle's last check: ms_out host [3] = upload, kernel, download, in milliseconds. */
D2R_API int d2r_sdfphys_get_timing(d2r_ctx *ctx, const d2r_sdfphys *h, double *ms_out);

/* ------------------------------------------------- the colour-TSDF visual model (vis_backend "tsdf")
 *
 * This package's own third visual backend beside the NeRF snapshots and the point-cloud ablation; nothing here stands where a
 * stage of the reference stands.  A volume fused from RGB-D frames carries three fp32 colour channels per voxel, and a ray
 * caster renders the K candidates of a pose grid from a background volume and a movable volume, dense and hole-free.
 */

/* d2r_tsdf_integrate with colour: rgb_u8 host [h][w][3].  (tsdf, weight) take exactly what d2r_tsdf_integrate gives them: the
 * same bytes.  At exactly the voxels whose tsdf the frame updates, each colour channel takes c = (w c + (float)rgb[v][u][ch]) /
 * (w + 1), w the weight before the increment, (u, v) the pixel the voxel projected to; fp32, nothing contracted.  The colour
 * storage (12 bytes a voxel) is allocated by the first call; a volume whose state with it would pass the cap of
 * d2r_tsdf_create is refused with D2R_ERR_UNSUPPORTED ("TSDF volume over the cap").  A volume takes frames through one of the
 * two calls only: the other one is refused with D2R_ERR_INVALID ("mixes").  Synchronous. */
D2R_API int d2r_tsdf_integrate_rgb(d2r_tsdf *vol, const uint16_t *depth_u16, const uint8_t *mask_u8, const uint8_t *rgb_u8, uint32_t w,
                                   uint32_t h, const float *intrinsics, const float *cam_pose, uint32_t erode_k);

/* Parity hook: the blocks of d2r_tsdf_read_voxels in its order, colours host [n][16][16][16][3] fp32 indexed [z][y][x][channel].
 * *n_blocks: capacity on entry, count on return; colours NULL = count only.  D2R_ERR_INVALID for a volume without colour. */
D2R_API int d2r_tsdf_read_colours(d2r_tsdf *vol, uint32_t *n_blocks, float *colours);

/*
 * Parity hook: K ray-cast frames to the host.  Both volumes carry colour; they may lie on different grids.
 *   view          d2r_pcd_view with d2r_pcd_render's limits (point_size is checked and otherwise unused)
 *   cam_pose      host [16] fp32 row-major camera-to-world pose, OpenCV convention (rigid)
 *   obj_pose_now  host [16] the movable object's pose O when its volume was fused; obj_poses host [K][16] candidate poses P_k
 *   frames_out    host [K][h][w][3] uint8; depth_out host [K][h][w] fp32 or NULL: the camera depth of the winning hit, +inf
 *                 where neither volume is hit
 * The rule: pixel (i, j) casts d_c = ((j - cx) / fx, (i - cy) / fy, 1); a volume stays put and the ray
 * moves by M = cam_pose (background) or M_k = (O inv(P_k)) cam_pose (movable), composed in fp64 and rounded once; samples at
 * t_s = near + s voxel up to depth 3; a sample is observed when the eight corners of its cell have weight >= weight_threshold;
 * the hit is the first observed pair (value > 0, then value <= 0), its depth the linear zero crossing, its colour the trilinear
 * colour there; the movable hit wins where it is strictly nearer than the background's; a pixel without a hit is black.
 * K = 0 is valid.  Refused before any device work, outputs untouched: null arguments, a volume without colour (or of another
 * device), a non-rigid or non-finite pose, a view outside the limits, weight_threshold not > 0, a voxel so small that a ray
 * would take more than 2^20 samples (D2R_ERR_UNSUPPORTED).  Synchronous.
 */
D2R_API int d2r_tsdfvis_render(d2r_ctx *ctx, d2r_tsdf *bg_vol, d2r_tsdf *movable_vol, const d2r_pcd_view *view, const float *cam_pose,
                               const float *obj_pose_now, const float *obj_poses, uint32_t K, float weight_threshold,
                               uint8_t *frames_out, float *depth_out);

/* The fused pass: d2r_tsdfvis_render's frames scored as d2r_pcd_render_score_host scores its own, in the same chunks; the frames
 * never leave the device unless frames_out is given.  Logits equal d2r_clip_score_frames(frames, rot90 = 1) of the frames
 * d2r_tsdfvis_render gives.  Synchronous. */
D2R_API int d2r_tsdfvis_render_score_host(d2r_ctx *ctx, d2r_tsdf *bg_vol, d2r_tsdf *movable_vol, const d2r_clip *clip,
                                          const d2r_pcd_view *view, const float *cam_pose, const float *obj_pose_now,
                                          const float *obj_poses, uint32_t K, float weight_threshold, const float *text_embeds,
                                          uint32_t C, float logit_scale, float *logits_out, uint8_t *frames_out);

/* Device-event times of the context's last d2r_tsdfvis_render / d2r_tsdfvis_render_score_host with K > 0: ms_out host [4] = upload
 * (matrices and rectangles), the background's cast, the candidates' casts summed over the passes, the copies of frames and depths
 * to the host summed over the passes (parity hook; 0 for the fused call, whose frames stay on the device unless frames_out is
 * given, and whose scoring is not in these figures), in milliseconds. */
D2R_API int d2r_tsdfvis_get_timing(d2r_ctx *ctx, double *ms_out);

/* ------------------------------------------------- camera poses refined against a TSDF volume (cam_pose_refine "tsdf")
 *
 * This package's own stand-in for the camera poses NeRF training optimises in the reference: frame-to-model tracking on the signed
 * distance field itself.  One linearisation: every pixel with u % stride == 0, v % stride == 0, a set mask and 0 < z = u16 / 1000
 * <= 3 is back-projected through the fp32 pose; where the eight corners of its cell carry weight >= weight_threshold and the
 * trilinear tsdf phi has |phi| < 1 (and the gates of section 2j hold) it contributes the residual r = phi trunc and the Jacobian
 * row J = [n, p_w x n], n the analytic gradient of the trilinear interpolant in metres per metre, of the left-multiplied twist
 * (T <- exp(xi^) T).  The 29 sums -- the upper triangle of J^T J row by row (21), J^T r (6), sum r^2, the count -- are signed 64-bit
 * integers: each term is the exact fp64 product of two fp32 factors times 2^D2R_CAMTRACK_SCALE_LOG2 rounded to nearest even (the
 * count is plain), so the sums are the same bits in any order.
 */
#define D2R_CAMTRACK_SUMS 29
#define D2R_CAMTRACK_SCALE_LOG2 29
#define D2R_CAMTRACK_MAX_ITERS 64
enum { D2R_CAMTRACK_CONVERGED = 0, D2R_CAMTRACK_MAX_ITERS_REACHED = 1, D2R_CAMTRACK_DEGENERATE = 2, D2R_CAMTRACK_TOO_FEW = 3 };

typedef struct d2r_camtrack_params {
    float weight_threshold;   /* > 0; 1 while a scan is being fused frame by frame */
    uint32_t stride;          /* >= 1 */
    uint32_t max_iters;       /* 1 .. D2R_CAMTRACK_MAX_ITERS; 20 by default in the Python layer */
    uint32_t min_pixels;      /* fewer contributing pixels than this in a linearisation: D2R_CAMTRACK_TOO_FEW */
} d2r_camtrack_params;

typedef struct d2r_camtrack_report {
    int32_t status;           /* D2R_CAMTRACK_* */
    uint32_t iters;           /* linearisations done: the valid entries of poses and sums */
    uint64_t pixels_first, pixels_last;   /* contributing pixels of the first and the last linearisation */
    double rms_first, rms_last;           /* sqrt(sum r^2 / count) of those two, metres */
    float poses[64][16];      /* the fp32 pose each linearisation used */
    int64_t sums[64][29];     /* ... and its sums */
} d2r_camtrack_report;

/* Parity hook: one linearisation.  depth_u16 host [h][w] millimetres, mask_u8 host [h][w] (non-zero = use; no erosion here),
 * intrinsics host [9] row-major 3x3, cam_pose host [16] row-major camera-to-world, sums_out host [D2R_CAMTRACK_SUMS].  A volume
 * fed through d2r_tsdf_integrate_rgb is accepted as well.  Refused with D2R_ERR_INVALID before any device work, sums_out
 * untouched: null arguments, a volume of another device than ctx's, a non-rigid (R^T R = I to 1e-5, last row 0 0 0 1) or non-finite
 * pose, non-finite intrinsics or a zero focal length, stride 0, w h = 0 or above 2^21, weight_threshold not > 0.  Synchronous. */
D2R_API int d2r_camtrack_system(d2r_ctx *ctx, d2r_tsdf *vol, const uint16_t *depth_u16, const uint8_t *mask_u8, uint32_t w, uint32_t h,
                                const float *intrinsics, const float *cam_pose, float weight_threshold, uint32_t stride,
                                int64_t *sums_out);

/* The loop: linearise at the pose rounded to fp32, solve the 6 x 6 system on the host in fp64 (LDL^T; a pivot <= 1e-6 of the
 * largest diagonal entry is D2R_CAMTRACK_DEGENERATE and stops with the pose it had), T <- exp(xi^) T carried in fp64, until |v| <
 * 1e-5 m and |omega| < 1e-5 rad, max_iters linearisations, or fewer than min_pixels contributing pixels (cam_pose_out = cam_pose_in
 * bit for bit).  Depth and mask are uploaded once; each iteration brings 29 sums back.  cam_pose_out host [16].  Refusals as
 * d2r_camtrack_system's plus max_iters 0 or above D2R_CAMTRACK_MAX_ITERS; cam_pose_out and report untouched.  Synchronous. */
D2R_API int d2r_camtrack_refine(d2r_ctx *ctx, d2r_tsdf *vol, const uint16_t *depth_u16, const uint8_t *mask_u8, uint32_t w, uint32_t h,
                                const float *intrinsics, const float *cam_pose_in, const d2r_camtrack_params *params,
                                float *cam_pose_out, d2r_camtrack_report *report);

/* Device-event times of the context's last d2r_camtrack_refine: ms_out host [3] = upload of depth and mask, the kernels summed
 * over the iterations, the downloads of the sums summed over the iterations, in milliseconds. */
D2R_API int d2r_camtrack_get_timing(d2r_ctx *ctx, double *ms_out);

/* 8-bit images of 1 (grey), 3 (RGB) or 4 (RGBA) interleaved channels -> a PNG file (mask files, the RGBA task images); a grey PNG
 * of 8 or 16 bits -> uint8 / uint16 [h][w] in host byte order (mask files, the 16-bit millimetre depth files; w, h: the expected
 * size, 0 = any); d2r_png_info reads the header.  Host only. */
D2R_API int d2r_png_write_channels(const uint8_t *pixels, uint32_t w, uint32_t h, uint32_t channels, const char *path, int level);
D2R_API int d2r_png_info(const char *path, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bits);
D2R_API int d2r_png_read_rgb(const char *path, uint32_t w, uint32_t h, uint8_t *rgb_out);   /* one 8-bit file of any name -> [h][w][3] */
D2R_API int d2r_png_read_grey(const char *path, uint32_t bits, uint32_t w, uint32_t h, void *out);

/* ------------------------------------------------- scene-bound masks and the pruning of segmentation masks
 *
 * replaces reference data_loader.py:71-122 (remove_background: Open3D back-projection, six planes and a height cut, a
 * closing by a 50 x 50 rectangle, per frame on the CPU) and segmentation/XMem_infer.py:264-351 (duplicate_prune,
 * disconnected_prune: cv2.connectedComponents per label per frame) with the out-of-scene overwrite of :224.  The rule is
 * DESIGN.md section 2d.  Both batch calls upload all n frames once, run without a host synchronisation between frames and
 * return when the result is in the caller's memory.  Frames are [n][h][w], w * h < 2^31; poses host [n][16] fp32 row-major
 * camera-to-world; K host [9] row-major fp64.
 */

/* bounds host [6]: xmin ymin zmin xmax ymax zmax (zmin is replaced by -100 as the reference does); window 1 .. 64 (the
 * reference: 50); out_u8 host [n][h][w] 0 / 255 after the closing; raw_out_u8 (optional) the same before it. */
D2R_API int d2r_scene_bound_masks(d2r_ctx *ctx, const uint16_t *depth_u16, uint32_t n, uint32_t w, uint32_t h, const float *poses,
                                  const double *K, const double *bounds, uint32_t window, uint8_t *out_u8, uint8_t *raw_out_u8);

/* mode 0 duplicate_prune (depth_u16, poses, K, centre host [3] required), 1 disconnected_prune (they may be NULL).  masks_u8
 * label images, 0 = background; oob_u8 (optional): where it is 255 the output is 255; min_area 200 in the reference. */
D2R_API int d2r_masks_prune(d2r_ctx *ctx, int mode, const uint8_t *masks_u8, const uint16_t *depth_u16, const uint8_t *oob_u8,
                            uint32_t n, uint32_t w, uint32_t h, const float *poses, const double *K, const double *centre,
                            uint32_t min_area, uint8_t *out_u8);

/* Parity hook, one frame: keys_out host [h][w] the order key (raster index of the first pixel) of each pixel's component,
 * 0xffffffff where the label is 0; area_out host [h][w] and sums_out host [h][w][4] (n, sum d, sum j d, sum i d over the
 * pixels with d16 > 0) hold a component's statistics at its order key and 0 elsewhere. */
D2R_API int d2r_masks_components(d2r_ctx *ctx, const uint8_t *mask_u8, const uint16_t *depth_u16, uint32_t w, uint32_t h,
                                 uint32_t *keys_out, uint32_t *area_out, uint64_t *sums_out);

/* out = (lut[mask] != 0) | (oob != 0) as 0 / 1 (oob_u8 optional), alpha_out_u8 (optional) = 255 (1 - out).  lut host [256]. */
D2R_API int d2r_masks_lut(d2r_ctx *ctx, const uint8_t *masks_u8, const uint8_t *oob_u8, uint32_t n, uint32_t w, uint32_t h,
                          const uint8_t *lut, uint8_t *out_u8, uint8_t *alpha_out_u8);

/* The label census of build_scene_model (reference dream2real.py:141-144, torch.unique over all frames): counts_out host
 * [n][256] uint32, counts_out[f][l] = the number of pixels of frame f that carry label l.  Any w, h and n the batch calls take;
 * a row need not be a multiple of any load width.  Integer sums only: the result does not depend on the order of the adds. */
D2R_API int d2r_masks_census(d2r_ctx *ctx, const uint8_t *masks_u8, uint32_t n, uint32_t w, uint32_t h, uint32_t *counts_out);

/* Device-event times of the last d2r_scene_bound_masks / d2r_masks_prune / d2r_masks_census on this context: ms_out host [3] =
 * upload, kernels, download, in milliseconds. */
D2R_API int d2r_masks_get_timing(d2r_ctx *ctx, double *ms_out);

/* ------------------------------------------------- object thumbnails for captioning
 *
 * replaces the image work of reference caption.py:62-130 (Captioner.caption_objs: per object and frame a mask against the scene
 * bounds, its area, bounding box and border contact, the container test of frame 0, for containers a 201 x 201 Gaussian blur,
 * a dilation and noise, the crop).  The rule is DESIGN.md section 2g.  Count, then fill: d2r_thumbs_plan uploads the frames,
 * runs the statistics and the container test and applies the acceptance rule; d2r_thumbs_fill writes every accepted thumbnail
 * into one packed buffer.  The frames stay on the device in between; another plan replaces them.
 */
#define D2R_THUMB_REC_WORDS 10u       /* object, frame, flags, area, row0, col0, rows, cols, offset low, offset high */
#define D2R_THUMB_ACCEPTED 1u         /* flags: the record has a thumbnail of rows x cols x 3 bytes at its offset */
#define D2R_THUMB_CONTAINER 2u        /*        the object is a container (decided on frame 0) */
#define D2R_THUMB_ROTATED 4u          /*        the frame is rotated counter-clockwise by 90 degrees; the crop is in the rotated frame */
#define D2R_THUMB_EDGE 8u             /*        the object touches the frame's border */
#define D2R_THUMB_SMALL 16u           /*        area < min_area */
#define D2R_THUMB_PARAM_WORDS 7u      /* topdown, multi_view, single_view_idx, min_area, hole_area, pad, dilate_k */

/* rgbs host [n][h][w][3], masks_u8 host [n][h][w] labels (0 the background object), oob_u8 host [n][h][w] (non-zero: outside
 * the scene); params host [D2R_THUMB_PARAM_WORDS] (the reference: min_area 200, hole_area 400, pad 5, dilate_k 60).  One record
 * per (object 1 .. num_objs - 1, visited frame), objects outermost, frames increasing: (num_objs - 1) * (multi_view ? n : 1) of
 * them.  *n_recs: the capacity of recs_out in records on entry (ignored when recs_out is NULL), the count on return; recs_out
 * host [n_recs][D2R_THUMB_REC_WORDS], NULL = run, keep the plan, return the counts only.  *total_bytes: the size of the packed
 * buffer d2r_thumbs_fill writes; a record's offset is a multiple of 4.  Refused with D2R_ERR_INVALID: num_objs 0 or > 255,
 * dilate_k outside 1 .. 64, single_view_idx >= n (without multi_view), a capacity below the count. */
D2R_API int d2r_thumbs_plan(d2r_ctx *ctx, const uint8_t *rgbs, const uint8_t *masks_u8, const uint8_t *oob_u8, uint32_t n, uint32_t w,
                            uint32_t h, uint32_t num_objs, const uint32_t *params, uint32_t *recs_out, uint32_t *n_recs,
                            uint64_t *total_bytes);

/* noise_u8 host [h][w][3]; out_u8 host [total_bytes], at least the plan's total.  Runs blur and dilation for the accepted
 * container records, then one launch composes every accepted thumbnail.  Refused: no plan on this context, total_bytes too small. */
D2R_API int d2r_thumbs_fill(d2r_ctx *ctx, const uint8_t *noise_u8, uint8_t *out_u8, uint64_t total_bytes);

/* Parity hook on one image: bits_u8 host [h][w] (non-zero = 1) -> out_u8 host [h][w] 0 / 1, the blur bit of section 2g dilated
 * by dilate_k x dilate_k (1 .. 64; 1 = the blur bit itself). */
D2R_API int d2r_thumbs_blur_bits(d2r_ctx *ctx, const uint8_t *bits_u8, uint32_t w, uint32_t h, uint32_t dilate_k, uint8_t *out_u8);

/* Device-event times of the context's last d2r_thumbs_plan plus its last d2r_thumbs_fill: ms_out host [3] = upload, kernels,
 * download, in milliseconds. */
D2R_API int d2r_thumbs_get_timing(d2r_ctx *ctx, double *ms_out);

/* ------------------------------------------------- mask proposals to the first frame's label image
 *
 * replaces the post-processing of reference segmentation/sam_seg.py:80-115 (Segmentor.segment after the mask generator: the
 * scene-bound AND, the disconnected / large / subpart / small rules with cv2.dilate, cv2.connectedComponents, cv2.findContours
 * and cv2.minAreaRect per mask on the CPU) and integrate_masks (segmentation/XMem_infer.py:256-261).  The rule is DESIGN.md
 * section 2h: integer arithmetic only, the result does not depend on the order the threads ran in.
 */
#define D2R_PROP_REC_WORDS 8u         /* area, components of the 5 x 5 dilation, dropping stage (0 kept, 1 disconnected, 2 large,
                                       * 3 subpart, 4 small), label, boundary pixels of the chosen component, ew, eh, dd */
#define D2R_PROP_MAX 1024u            /* proposals per call */
#define D2R_PROP_MAX_SIDE 8192u       /* width and height */

/* props_u8 host [m][h][w] (non-zero = set) in the proposer's order, inside_u8 (optional) host [h][w] (non-zero = inside the
 * scene bounds); labels_out host [h][w]: 0, or the label 1, 2, ... of the last surviving proposal that covers the pixel.
 * recs_out (optional) host [m][D2R_PROP_REC_WORDS]: every field is filled for every proposal, whatever stage dropped it.
 * inter_out (optional) host [m][m]: |P[i] & P[j]| for i < j among the proposals that passed stages 1 and 2, 0 elsewhere.
 * m = 0 gives an all-zero image.  Refused with D2R_ERR_INVALID and labels_out, recs_out, inter_out untouched: m above
 * D2R_PROP_MAX, a zero width or height or one above D2R_PROP_MAX_SIDE, more than 255 survivors; D2R_ERR_UNSUPPORTED: m * w * h
 * of 2^32 or more. */
D2R_API int d2r_proposals_labels(d2r_ctx *ctx, const uint8_t *props_u8, const uint8_t *inside_u8, uint32_t m, uint32_t w, uint32_t h,
                                 uint8_t *labels_out, uint32_t *recs_out, uint32_t *inter_out);

/* Device-event times of the context's last d2r_proposals_labels with m > 0: ms_out host [3] = upload, kernels, download, in
 * milliseconds. */
D2R_API int d2r_proposals_get_timing(d2r_ctx *ctx, double *ms_out);

/* ------------------------------------------------- first-frame labels carried through a scan by geometry (tracker="geometric")
 *
 * This package's own stand-in for the video-object-segmentation network (XMem) the reference tracks its first label image with; nothing
 * here stands where reference code stands.  A scan is a static scene seen from known poses with metric depth: a voxel grid over the
 * scene bounds holds one (label, count) pair per voxel.  Frame 0 votes its label image into the grid; every later frame, in order,
 * reads a label per pixel from the voxel its depth back-projects to (predict), grows the known labels into the unknown pixels along
 * depth-continuous 4-neighbour paths for `grow` Jacobi sweeps (fill), is written out with the unknown pixels as 0, and votes what it
 * holds into the grid (Boyer-Moore majority, one lane per voxel, no atomics).  fp32 arithmetic, one IEEE operation at a time.
 */
#define D2R_LABELTRACK_UNKNOWN 255u        /* inside the unit only: never in labels0, never in labels_out */
#define D2R_LABELTRACK_SWEEPS_PER_LAUNCH 8u /* the sweeps one fill launch runs: the unit of stats_out's last column */
#define D2R_LABELTRACK_MAX_PIXELS (1u << 21)
#define D2R_LABELTRACK_MAX_VOXELS (1ull << 31)
#define D2R_LABELTRACK_MAX_COORD (1 << 23)  /* |voxel coordinate| of the grid's faces: every one is an exact float */

typedef struct d2r_labeltrack_params {
    float voxel;              /* metres, finite, > 0; 0.004 by default in the Python layer */
    uint32_t band_voxels;     /* 1 .. 8: the grid's padding and the vote's depth band, in voxels; 2 */
    uint32_t tau_mm;          /* 0 .. 65535: the largest depth step a label crosses in the fill, millimetres; 10 */
    uint32_t grow;            /* 0 .. 4096: sweeps of the fill; 64 */
} d2r_labeltrack_params;

/* The grid d2r_labeltrack_scan lays over bounds (host [6]: xmin ymin zmin xmax ymax zmax): dims_out host [3] voxels along x, y, z,
 * lo_out host [3] the first voxel's coordinate per axis; vol_out of the scan holds dims[0] * dims[1] * dims[2] uint16.  Host only.
 * Refused with D2R_ERR_INVALID, outputs untouched: null arguments, a parameter outside its range, non-finite or inverted bounds,
 * a face beyond D2R_LABELTRACK_MAX_COORD voxels from the origin, more than D2R_LABELTRACK_MAX_VOXELS voxels. */
D2R_API int d2r_labeltrack_grid(const double *bounds, const d2r_labeltrack_params *params, uint32_t *dims_out, int32_t *lo_out);

/* d16 host [n][h][w] millimetres, cam_poses host [n][16] fp32 row-major camera-to-world (OpenCV), K host [4]: fx fy cx cy,
 * labels0 host [h][w] frame 0's labels (0 the background, 255 refused).  labels_out host [n][h][w]: frame 0's is labels0.
 * stats_out (optional) host [n][4]: pixels known after predict, pixels the fill labelled, pixels left unknown, fill launches (of
 * D2R_LABELTRACK_SWEEPS_PER_LAUNCH sweeps) in which a pixel changed; frame 0's row is w h, 0, 0, 0.  vol_out (optional) host
 * [dims z][dims y][dims x] uint16, label in the low byte and count in the high byte, after the last frame's vote; vol_dims_out and
 * vol_lo_out (optional) host [3] as d2r_labeltrack_grid gives them.  Refused with D2R_ERR_INVALID before any device work, outputs
 * untouched: what d2r_labeltrack_grid refuses, null arguments, n = 0, w h = 0 or above D2R_LABELTRACK_MAX_PIXELS, a non-rigid (R^T R = I
 * to 1e-5, last row 0 0 0 1) or non-finite pose, non-finite intrinsics or a zero focal length, a 255 in labels0.  All frames are
 * uploaded once; no host synchronisation between the frames.  Synchronous. */
D2R_API int d2r_labeltrack_scan(d2r_ctx *ctx, const double *bounds, const d2r_labeltrack_params *params, uint32_t n, uint32_t w, uint32_t h,
                                const double *K, const uint16_t *d16, const float *cam_poses, const uint8_t *labels0, uint8_t *labels_out,
                                uint32_t *stats_out, uint16_t *vol_out, uint32_t *vol_dims_out, int32_t *vol_lo_out);

/* Device-event times of the context's last d2r_labeltrack_scan: ms_out host [3] = upload, kernels, download, in milliseconds. */
D2R_API int d2r_labeltrack_get_timing(d2r_ctx *ctx, double *ms_out);

/* ------------------------------------------------- mask proposals from depth and the support plane (proposer="geometric")
 *
 * This package's own stand-in for the segmentation network (SAM's mask generator) the reference takes its mask proposals from, for
 * table-top scenes; nothing here stands where reference code stands.  A pixel of frame 0 with depth is back-projected in fp64
 * (section 2d) and is `inside` when its point lies in the bounds; its height is floor(1000 (up . p) + 0.5) millimetres.  The support
 * plane b* is the centre of the fullest window of window_mm height bins (ties to the lowest); a pixel is `above` when it is inside
 * at b* + h_min_mm or higher; two 4-neighbours are linked when both are above and their depths differ by tau_mm millimetres at the
 * most; the connected sets of at least min_area pixels, the max_props largest of them (area ties to the smaller first pixel),
 * numbered 1 .. M by their first pixel in raster order, are the proposals.  Integer atomics only: the result does not depend on
 * the order the threads ran in.
 */
#define D2R_GEOPROP_REC_WORDS 6u       /* root (raster index of the first pixel), area, i0, j0, i1, j1 (rows, columns, inclusive) */
#define D2R_GEOPROP_PLANE_WORDS 5u     /* b*, pixels in its window, inside pixels, above pixels, components before the selection */
#define D2R_GEOPROP_MAX_BINS (1u << 16)

typedef struct d2r_geoprop_params {
    uint32_t window_mm;       /* odd, 1 .. 65535: the height bins summed around a candidate plane; 5 by default in the Python layer */
    uint32_t h_min_mm;        /* 0 .. 65535: a pixel is above from b* + h_min_mm on; 6 */
    uint32_t tau_mm;          /* 0 .. 65535: the largest depth step between two linked neighbours, millimetres; 10 */
    uint32_t min_area;        /* pixels: smaller components are dropped; 200 */
    uint32_t max_props;       /* 1 .. D2R_PROP_MAX: the most proposals returned */
} d2r_geoprop_params;

/* bounds host [6]: xmin ymin zmin xmax ymax zmax; up host [3]: a unit vector (to 1e-6), the direction heights are measured along;
 * d16 host [h][w] millimetres; cam_pose host [16] fp32 row-major camera-to-world (OpenCV); K host [4]: fx fy cx cy.  labels_out host
 * [h][w]: 0 or the proposal's number; recs_out host [max_props][D2R_GEOPROP_REC_WORDS]: rows 0 .. M - 1 filled, the others zero;
 * *n_out = M; plane_out host [D2R_GEOPROP_PLANE_WORDS].  Without an inside pixel there is no plane: everything comes back zero, which
 * is a result, not a failure.  Refused with D2R_ERR_INVALID before any device work, outputs untouched: null arguments, w h = 0 or
 * above D2R_LABELTRACK_MAX_PIXELS, a non-rigid or non-finite pose, a focal length that is not finite and > 0, a non-finite principal
 * point, bounds that are not finite with min < max or span more than D2R_GEOPROP_MAX_BINS height bins, an up that is not of unit
 * length, a parameter outside its range.  Synchronous. */
D2R_API int d2r_geoprop_masks(d2r_ctx *ctx, const double *bounds, const double *up, const d2r_geoprop_params *params, uint32_t w, uint32_t h,
                              const double *K, const uint16_t *d16, const float *cam_pose, uint16_t *labels_out, uint32_t *recs_out,
                              uint32_t *n_out, int32_t *plane_out);

/* Device-event times of the context's last d2r_geoprop_masks: ms_out host [5] = upload; heights and histogram; plane choice, links,
 * labelling, statistics and the candidate list; selection, numbering and the label image; download, in milliseconds.  The second
 * and the third interval each hold one small copy to the host and the host's part of the rule. */
D2R_API int d2r_geoprop_get_timing(d2r_ctx *ctx, double *ms_out);

/* ------------------------------------------------- object names from the package's own CLIP towers (captioner="clip")
 *
 * This package's own stand-in for the captioning network (BLIP-2) and the language model's merging of the per-view captions
 * (reference caption.py:132-160); nothing here stands where reference code stands.  The thumbnails d2r_thumbs_fill left packed on
 * the device (they stay there until the context's next d2r_thumbs_plan) go through HF's CLIPImageProcessor (shortest side to S with
 * Pillow's antialiased bicubic, centre crop) in one launch whatever their sizes, through the vision tower, and are compared with the
 * embeddings of a closed vocabulary of names: cos[t][v] in fp32 by 64 partial sums joined by the xor butterfly, summed per object
 * over its thumbnails in record order; the k best classes per object by (score descending, index ascending) are the answer.
 */
#define D2R_CAPTION_MAX_K 8u
#define D2R_CAPTION_MAX_V 8192u       /* classes per call */
#define D2R_CAPTION_MAX_D 1024u       /* embedding width: a multiple of 64 */

/* Needs a d2r_thumbs_plan and a d2r_thumbs_fill on this context (or d2r_caption_load_packed).  embeds_out host [T][proj_dim], T the
 * accepted records of the plan in record order, L2-normalised; crops_u8_out (optional) host [T][S][S][3] the resized and cropped
 * images; pixel_values_out (optional) host [T][3][S][S] what the tower's patches were rounded from.  Refused with D2R_ERR_INVALID
 * before any device work, outputs untouched: null arguments, no filled plan on this context; D2R_ERR_UNSUPPORTED: a thumbnail whose
 * resized long side would pass 2^20 pixels or whose band does not fit in LDS. */
D2R_API int d2r_caption_embed(d2r_ctx *ctx, const d2r_clip *clip, float *embeds_out, uint8_t *crops_u8_out, float *pixel_values_out);

/* Parity hook, the scoring launch alone on host arrays: embeds host [T][D], obj_of host [T] the object 0 .. n_objs - 1 of every
 * thumbnail, non-decreasing; class_embeds host [V][D].  idx_out host [n_objs][k], score_out host [n_objs][k]; an object without a
 * thumbnail scores 0 for every class, and a score that is no number (a NaN embedding) ranks, and is reported, as minus infinity.  The
 * class embeddings are uploaded once per (V, D, contents).  Refused with D2R_ERR_INVALID
 * before any device work, outputs untouched: null arguments, V = 0 or above D2R_CAPTION_MAX_V, D no multiple of 64 or above
 * D2R_CAPTION_MAX_D, k outside 1 .. min(D2R_CAPTION_MAX_K, V), n_objs outside 1 .. 255, a class embedding that is not finite, an
 * obj_of that decreases or reaches n_objs. */
D2R_API int d2r_caption_vote(d2r_ctx *ctx, const float *embeds, const uint32_t *obj_of, uint32_t T, const float *class_embeds, uint32_t V,
                             uint32_t D, uint32_t n_objs, uint32_t k, uint32_t *idx_out, float *score_out);

/* The fused call: the context's thumbnails -> idx_out host [n_objs][k], score_out host [n_objs][k] for the objects 1 .. n_objs =
 * num_objs - 1 of the plan; nothing else crosses to the host.  Refused like the two calls above, when D is not the clip's proj_dim,
 * and when n_objs is not the number of objects the context's thumbnails are of (the outputs would not fit). */
D2R_API int d2r_caption_names(d2r_ctx *ctx, const d2r_clip *clip, const float *class_embeds, uint32_t V, uint32_t D, uint32_t n_objs,
                              uint32_t k, uint32_t *idx_out, float *score_out);

/* Parity hook: a packed buffer of thumbnails from the host in place of a plan and a fill, so that a test chooses the sizes.  recs
 * host [n_recs][5]: object 0 .. n_objs - 1 (non-decreasing), rows, cols, offset low, offset high; an image is rows x cols x 3 bytes
 * at its offset, a multiple of 4.  Refused with D2R_ERR_INVALID: null arguments, no record or object, a record outside the buffer,
 * rows or cols outside 1 .. 16384. */
D2R_API int d2r_caption_load_packed(d2r_ctx *ctx, const uint8_t *packed_u8, uint64_t total_bytes, const uint32_t *recs, uint32_t n_recs,
                                    uint32_t n_objs);

/* Device-event times of the context's last d2r_caption_embed / d2r_caption_vote / d2r_caption_names: ms_out host [5] = upload,
 * preprocess, tower, scoring, download, in milliseconds (a stage the call did not run is 0; the upload includes the class
 * embeddings when the call brought new ones). */
D2R_API int d2r_caption_get_timing(d2r_ctx *ctx, double *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* D2R_H */
