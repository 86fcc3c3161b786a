// Internal declarations shared by the HIP translation units of libd2r.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/d2r.h"
#include "d2r_shared.h"
#include "tsdf_sample.h"

class D2rJobPool;   // pngio.h
struct D2rPngBase;  // pngio.h

#define D2R_MAX_LEVELS 16
#define D2R_MAX_DEVICES 64              // per-device "kernel attribute already set" flags
#define D2R_GRID 128
#define D2R_DT 0.0016914558f           // sqrt(3)/1024
#define D2R_INV_DT (1.0f / D2R_DT)
// aabb_scale 2 (oracle/d2r_oracle.c "cone stepping"): t_{k+1} = t_k + max(dt, t_k/256) in closed form
#define D2R_CONE 0.00390625f
// D2R_T_LINEAR: the distance at which steps start to grow, dt_min / cone as in the per-step rule dt = max(dt_min, t * cone).  Newer
// instant-ngp revisions step in an analytic log space and switch at dt_min / log1p(cone) (~256.5 dt_min; lattices agree to ~0.2 % of a
// step).  The reference's pinned commit is unknown: if a real snapshot ever disagrees, change this line and oracle/d2r_oracle.c's twin.
#define D2R_T_LINEAR (D2R_DT * 256.0f)
#define D2R_N_WFRAG 24                 // MLP weight fragments (see nerf.hip)

struct LevelMeta {
    float scale;
    uint32_t res;
    uint32_t size;
    uint32_t offset;
    uint32_t hashed;
};

// One "slot" = the pair of hash-grid levels (2i, 2i+1) that the two lanes (l, l^32) of a lane
// pair evaluate.  Their tables are stored INTERLEAVED in HBM: entry e of level 2i+h lives at
// byte  slot_off + 8*e + 4*h, so a corner address is (index << 3) | (h << 2) plus an SGPR offset.
struct SlotMeta {
    float scale[2];
    uint32_t res[2];
    uint32_t size[2];
    uint32_t hashed[2];
    uint32_t mask8;      // (hash table size - 1) << 3 | 4   (hashed levels share one size)
    uint32_t off;        // byte offset of the slot's interleaved table
    // bounding-box-local dense brick of each level (served from LDS when the slot is bricked):
    // vertex (gx,gy,gz) at LDS word  bbase + gx + bnx*gy + bnxy*gz
    uint32_t bnx[2], bnxy[2];
    int32_t bbase[2];
};

struct NerfParams {
    const uint32_t *grid;      // interleaved slot tables, half2 entries
    uint32_t grid_bytes;
    uint32_t n_levels;         // 16 (F = 2: a slot is the level pair 2i, 2i+1) or 8 (F = 4: a slot is level i, its two
                               // "halves" the feature pairs (0,1) and (2,3) of the 8-byte entries) — either way entry e
                               // of half h lives at byte 8e + 4h of the slot table and network input 4*slot + 2h + f
    int32_t n_dense;           // leading dense HALF-levels (2 per level when F = 4; slot kinds follow from it), -1 = irregular
    SlotMeta slot[D2R_MAX_LEVELS / 2];
    uint32_t refill_min;       // free lanes in a wave before it pulls new rays from the queue
    uint32_t compact;          // 1: a wave with <= 32 rays left moves them to lanes 0..31 (tile 1 then costs nothing)
    uint32_t sort_log2;        // ray sort: 0 off, else log2 of the bins per axis of the occupied box (2: 4x4x4 ... 4: 16x16x16); the bin of a ray's first sample rides in bits 20.. of its queue entry's k
    uint32_t n_brick_slots;    // leading slots whose levels are de-hashed into LDS bricks (0 .. 5)
    uint32_t brick_words;      // total words of those bricks
    const uint32_t *brick_tab; // [brick_words] half2 entries, copied to LDS by every workgroup
    uint32_t n_gbrick_slots;   // further slots de-hashed into dense bricks kept in HBM (spatially coherent)
    uint32_t gbrick_bytes;
    const uint32_t *gbrick_tab;
    const uint64_t *bricks;    // [n_cascades][32^3] 4x4x4-cell occupancy bricks
    uint32_t aabb_scale;       // 1, or a power of two up to 128: log2 + 1 cascades, cone stepping, positions normalised to the box (k_*<.., CONE>)
    uint32_t n_casc;
    float side, inv_side;      // aabb_scale and its reciprocal as floats
    const uint4 *wfrag;        // [24][64] MFMA A-operand fragments of the MLPs, bf16
    const uint4 *wfrag16;      // the same fragments holding the snapshot's fp16 weights unrounded (option mlp_f16)
    float bbox_lo[3], bbox_hi[3];  // bounding box of occupied cells (+margin), unit-cube units
    // Testbed.render_aabb clipped to the model's box: in ngp coordinates (ray slab test) and in the unit cube of
    // the box (per-sample containment test); the whole box when none is set
    float raabb_lo[3], raabb_hi[3], rn_lo[3], rn_hi[3];
};

struct ViewParams {
    uint32_t W, H;
    float focal[2], center[2];
    float scale, inv_scale;
    float offset[3];
    float background[4];
    float min_transmittance, near_distance;
    uint32_t lens_mode;        // D2R_LENS_*: 1 = every ray's camera-space direction is undistorted (lens_undistort, nerf.hip)
    float lens[4];             // OpenCV k1, k2, p1, p2
    const float2 *lens_tab;    // [H][W] undistorted (x, y) of the camera-space direction per pixel (k_lens_table), nullptr = perspective
};

struct ClipParams;   // clip.hip

// masks.hip: what d2r_thumbs_plan leaves for d2r_thumbs_fill.  The frames stay in thumb_in.
struct D2rThumbPlan {
    bool valid = false;
    uint32_t n = 0, w = 0, h = 0, dilate_k = 0;
    size_t o_rgb = 0, o_mask = 0, o_oob = 0;     // segments of thumb_in
    uint64_t total = 0;                          // bytes of the packed thumbnails
    std::vector<uint32_t> recs;                  // [n_recs][D2R_THUMB_REC_WORDS]
};

// captions.hip: the packed thumbnails d2r_thumbs_fill (or the parity hook d2r_caption_load_packed) left in thumb_out, as
// d2r_caption_embed / d2r_caption_names read them.  A new plan, or anything else that writes thumb_out, clears `filled`.
struct D2rCaptionSrc {
    bool filled = false;
    uint32_t n_objs = 0;                         // objects 1 .. n_objs of the plan
    uint64_t total = 0;                          // bytes of the packed buffer
    std::vector<uint32_t> recs;                  // [T][5] in record order: object - 1, rows, cols, offset low, offset high
};

// ... the resize geometry and the coefficient tables of one (rows, cols, S, P), cut to the S positions the centre crop reads; a side
// that is S already has no tables.  Built on first use and kept by the context.
struct D2rCaptionTables {
    int ks_h = 0, ks_v = 0, need_h = 0, need_v = 0, left = 0, top = 0;
    int band_rows = 0;                           // the largest vertical support of a band of P output rows
    std::vector<int> bh, kh, bv, kv;             // bounds_h [S][2], kk_h [S][ks_h], bounds_v [S][2], kk_v [S][ks_v]
};

// Layer-0 reuse of background tokens inside d2r_render_score (clip.hip "layer-0 reuse"): the frame rectangles the candidates
// of the chunk touched, and the background's own pre-LayerNorm residual rows and layer-0 q / k / v rows (d2r_clip_layer0_background)
struct ClipL0Reuse {
    const void *rects;           // device int4 [n]: x0, y0, x1, y1 in frame pixels, inclusive (k_raygen_rect)
    uint32_t w, h;               // frame size
    const uint16_t *bg_hi;       // [d / 64][bg_rows][64] bf16
    const uint8_t *bg_lo;        // lo bytes, lo8_off(bg_rows, ..) layout
    const float2 *bg_ab;         // [bg_rows] (rstd, -rstd * mean)
    const uint16_t *bg_qkv;      // [3 d / 64][bg_rows][64] bf16
    uint32_t bg_rows;            // tokens per image, rounded up to a multiple of 256
    uint32_t *touched_out;       // device, optional: receives the chunk's touched-token count (render statistics)
};

struct d2r_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    // growable device workspaces (one per role so sizes are independent); a role with several segments lays them out with D2rStage
    using Buf = D2rBuf;
    Buf queue2, sort_counts;   // ray sort: the sorted queue, per-chunk bin counts / offsets
    Buf cams, queue, counters, frames, rgba, depth, poses, clipws[8], text, logits, pix;
    // host -> device uploads of small caller buffers on asynchronous entry points (text embeddings of d2r_render_score)
    // go through two library-owned pinned slots, so the caller's memory is consumed before the call returns whatever
    // the runtime does with pageable copies; an event per slot guards its reuse
    void *text_host[2] = {nullptr, nullptr};
    size_t text_host_cap[2] = {0, 0};
    hipEvent_t text_ev[2] = {nullptr, nullptr};
    uint32_t text_turn = 0;
    // background of the current view
    Buf bg_rgba, bg_depth, bg_u8;
    Buf pcd_mats, pcd_bg_keys, pcd_bg_frame, pcd_cols;   // pcd.hip: candidate matrices, background key buffer and colour frame, colour table of the current call
    Buf tv_mats, tv_bg_frame, tv_bg_depth, tv_depth;   // tsdfvis.hip: candidate matrices + frame rectangles, the background's ray-cast frame and depth image, the candidates' depth images (parity hook)
    D2rStageTimer tv_timer, tv_pass_timer;   // ... upload / background cast of the last call, and one pass's candidate cast; tv_cast_ms sums the passes (d2r_tsdfvis_get_timing)
    D2rStageTimer tv_dl_timer;   // ... one pass's copy of frames and depths to the host (parity hook); tv_dl_ms sums the passes
    double tv_cast_ms = 0.0, tv_dl_ms = 0.0;
    bool tv_pass_pending = false, tv_dl_pending = false;
    Buf ct_in, ct_ws;            // camtrack.hip: the uploaded depth + mask (one D2rStage), per-workgroup partial sums + the 29 sums
    D2rStageTimer ct_timer, ct_it_timer;   // ... upload of the last refine, and one iteration's kernels / download; ct_ms sums the iterations (d2r_camtrack_get_timing)
    double ct_ms[3] = {0.0, 0.0, 0.0};
    bool ct_timed = false;
    Buf lt_in, lt_ws;            // labeltrack.hip: the uploaded depth frames + first label image + per-frame matrices (one D2rStage), the two label planes + result frames + counters
    D2rStageTimer lt_timer;      // ... upload / kernels / download of the last d2r_labeltrack_scan (d2r_labeltrack_get_timing)
    Buf gp_in, gp_ws;            // geoprop.hip: the uploaded depth frame, height bins / histogram / link planes / union-find parents / statistics / candidates / label image (one D2rStage)
    D2rStageTimer gp_timer, gp_timer2;   // ... upload / heights / components, then selection / download of the last d2r_geoprop_masks (d2r_geoprop_get_timing)
    Buf mv_in, mv_recs, mv_queue, mv_shade, mv_keys, mv_out;   // meshvis.hip: uploaded inputs (seven segments of a D2rStage), triangle records, the large-triangle queue, shade bytes, mesh + cube key buffers, rgb + ids of the current call
    Buf mask_in, mask_out, mask_ws;   // masks.hip: uploaded frames + per-label slots (the segments of a D2rStage per entry point), result frames, union-find parents + component statistics of a pass
    Buf thumb_in, thumb_ws, thumb_out;   // masks.hip, object thumbnails: frames + noise + records (one D2rStage), statistics / labelling / blur workspace, the packed thumbnails
    D2rThumbPlan thumb_plan;     // ... the records of the last d2r_thumbs_plan
    D2rStageTimer thumb_timer[2];   // ... upload / kernels / download of the last plan and of the last fill (d2r_thumbs_get_timing adds them)
    D2rCaptionSrc cap_src;       // captions.hip: what thumb_out holds for the captioner
    Buf cap_tab, cap_emb, cap_ws, cap_cls;   // ... record descriptors + coefficient tables (one D2rStage), the thumbnails' embeddings, parity outputs / vote inputs and results (one D2rStage), the class embeddings
    uint64_t cap_cls_key[3] = {0, 0, 0};     // ... V, D and the FNV-1a hash of the class embeddings cap_cls holds
    bool cap_cls_valid = false;
    std::map<std::array<uint32_t, 4>, D2rCaptionTables> cap_sizes;   // ... tables per (rows, cols, S, P), host side
    D2rStageTimer cap_ev[4];     // ... a pass of preprocess + tower, the scoring, a pass's downloads, the class embeddings' upload
    double cap_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // ... upload, preprocess, tower, scoring, download of the last caption call (d2r_caption_get_timing)
    bool cap_timed = false;
    Buf prop_in, prop_ws, prop_out;   // proposals.hip: the uploaded proposals + scene mask, the packed planes / union-find parents / records / pair matrix (one D2rStage), the label image
    D2rStageTimer prop_timer;    // ... upload / kernels / download of the last d2r_proposals_labels (d2r_proposals_get_timing)
    D2rStageTimer mask_timer;    // ... upload / kernels / download of the last batch call (d2r_masks_get_timing)
    D2rStageTimer pcdb_timer;    // pcdbuild.hip: upload / kernels of the last d2r_pcd_build (d2r_pcd_build_get_timing)
    Buf lens_tab;                // undistorted camera-space directions of the current view's pixels (nerf.hip lens_table)
    float lens_key[10] = {};     // ... and the view (size, intrinsics, coefficients) it was computed for
    bool lens_key_valid = false;
    Buf rect_ws;                 // d2r_rectify_background_depth: source images, tap tables, outputs (one D2rStage)
    Buf rects;                   // per candidate of a pass: frame rectangle (x0, y0, x1, y1) its rays were generated in
    Buf bg_patches;              // CLIP patches of the background frame itself (one image)
    const void *bg_patches_for = nullptr;   // the d2r_clip they were computed with (nullptr = stale)
    Buf bg_l0, l0_a1, l0_q2, l0_misc;       // layer-0 reuse: the background's rows; gathered patch rows; compact q / k / v; count + list + pairs
    const void *bg_l0_for = nullptr;        // the d2r_clip bg_l0 was computed with (nullptr = stale)
    ClipL0Reuse bg_l0_desc{};               // pointers into bg_l0
    int64_t vit_fp8 = 0;         // vision tower: the Linear products of the blocks between the first and the last on the MX-scaled fp8 MFMA (clip.hip, "fp8 blocks")
    int64_t l0_reuse = 1;        // d2r_render_score: patch embedding + layer-0 QKV on the touched tokens only
    int64_t prep_reuse = 1;      // k_preprocess copies the background's patch rows for bands a candidate cannot have touched
    uint32_t bg_w = 0, bg_h = 0;
    d2r_render_stats stats{};
    // device geometry (hipDeviceProp_t / hipDeviceAttributeNumberOfXccs): persistent kernels launch one
    // workgroup per CU and map tiles to XCDs (one L2 each)
    int n_cu = 256, n_xcd = 8;
    // pose-shard communicator (comm.hip): an ncclComm_t, or null at world size 1
    void *comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    // the render-and-score pipeline (api.hip render_score_core): the render half of chunk i+1 runs on render_stream while
    // the ViT scores chunk i on `stream`; frames that leave the GPU go through copy_stream into two pinned buffers and
    // from there to the worker pool (PNG files, the caller's array)
    hipStream_t render_stream = nullptr, copy_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_prep[2] = {nullptr, nullptr}, ev_clip[2] = {nullptr, nullptr},
               ev_march[2] = {nullptr, nullptr}, ev_copy[2] = {nullptr, nullptr};
    Buf patches2, frames2;
    void *frame_host[2] = {nullptr, nullptr};
    size_t frame_host_cap[2] = {0, 0};
    D2rJobPool *pool = nullptr;
    std::shared_ptr<const D2rPngBase> png_base;     // the current background's scanlines, entropy-coded once for the frame files (reset by d2r_set_background)
    int64_t overlap = 0;        // 1: render half of chunk i+1 on render_stream under the ViT of chunk i (measured neutral: both sides fill whole CUs); 0: program order on `stream`
    int64_t debug_fail_chunk = -1;   // fault injection for the error path of render_score_core (tests/test_api_path.py)
    uint32_t last_chunks = 0;   // chunks of the last d2r_render_score (its per-chunk counters are behind counters+64)
    int64_t chunk = 4096;       // candidates per pass (capped per model/view by d2r_pass_size() in api.hip)
    uint32_t last_pass = 0;     // pass size the last d2r_render_score used (for its stats read-back)
    int64_t march_blocks = 0;  // 0 = auto
    int64_t ray_sort = 1;      // 1: the ray queue is sorted by the object region (Morton cell of the occupied box) a ray's first sample lies in before it is marched; 0: marched in generation order
    int64_t ray_sort_log2 = 4; // cells per axis = 2^this (1..4); measured 8^3 -> 16^3: another 6 %
    int64_t march_threads = 0; // threads per marcher workgroup: 0 = auto (768, or 512 when the HBM bricks exceed march_threads_auto_mib MiB), else 64 .. 768 in steps of 64
    int64_t march_threads_auto_mib = 64;   // apple 36 MB (issue-bound: 768 threads are 8 % faster), shelf 112 MB, 2.2x / 5x apple 394 / 89 MB (L2-miss-bound: 512 are 1-5 % faster)
    // read-backs (options march_threads_used, march_hbm_brick_bytes, march_lds_slots, march_hbm_brick_slots):
    int64_t last_march_threads = 0, last_march_gbrick_bytes = 0;   // the workgroup size / HBM-brick bytes of the last march launch
    int64_t last_march_nb = 0, last_march_ngb = 0;    // ... and the brick configuration it ran with
    int64_t refill_min = 64;   // measured on MI355X: a refill (queue + camera loads, ray setup, SH) costs several iterations,
                               // so a wave runs its 64 rays to the end (lane utilisation 0.79) rather than topping up at 16 free lanes (0.90)
    int64_t march_compact = 1; // marcher: compact a wave's last <= 32 rays into one tile (option "march_compact")
    int64_t ln_fold = 4;       // vision tower: 0 LayerNorm kernels + fp32 residual; LayerNorm folded into the GEMMs with 1 a split (hi + lo) bf16 residual, 2 a bf16 residual, 3 an fp32 residual + bf16 copy, 4 bf16 hi + one lo byte
    int64_t gemm_nsplit = 0;     // column sections of the persistent GEMM's tile order (XCD sets own column ranges): 0 = two where the XCDs and the column tiles divide evenly, 1 = none
    int64_t attn_rem = 1;          // attention: a remainder of at most this many query tiles (sequence = 8 g + r tiles) runs on workgroups of r waves instead of one more eight-wave group
    int64_t cls_last = 1;          // vision tower: run the last block on the class-token rows only (the head reads nothing else)
    int64_t mlp_f16 = 1;       // operand type of the NeRF MLPs' MFMAs: 1 (default since round 6) fp16 — the reference's operand type (tiny-cuda-nn), the snapshot's weights unrounded; 0 bf16 (north_star's wording).  Same MFMA rate; chosen by the distance table of tests/test_gpu_parity.py::test_render_distances_to_the_fp16_accumulation_emulation
    int64_t render_arith = 0;  // arithmetic of the field evaluation (nerf.hip eval_wave<…, ARITH>): 0 the specification (fp32 accumulation); 1 / 2 oracle/d2r_oracle.c's d2r_oracle_set_arith(1 / 2) restated — hash-grid corners summed in half (2: the fma form), half accumulators in both MLPs (one rounding per 16-wide k-step), half activations.  A validation mode: brick-free kernels, fp16 operands whatever mlp_f16 says
    int64_t use_bricks = 1;
    int64_t raygen_rect = 1;   // composite mode: generate rays only inside the projected occupied bbox
    int64_t gbrick_slots = 8;  // at most this many slots use HBM bricks
    int64_t brick_slots_total = 7;   // ... and none at or beyond this slot index: bricking the finest slot (levels 14-15) measured slower (cache misses)
    int64_t lds_slots_max = 5;       // d2r_nerf_create: at most this many leading slots as LDS bricks (experiments: the marcher's regimes)
    int64_t gbrick_max_mib = 512;    // d2r_nerf_create: a slot is HBM-bricked only while its brick stays below this size (512 = only the 512 MiB total bounds them: measured, a 5x apple renders 1.45x faster on its 100+ MiB bricks than on the 4 MiB hashed tables, profiles/r05_march_regimes.md)
    // optional per-kernel timing (HIP events on the launch stream), see d2r_get_timing
    int64_t timing = 0;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<std::pair<int, std::pair<size_t, size_t>>> ev_pairs;   // (kind, (begin, end))
    size_t timing_begin(int kind);          // returns pair index, records the begin event (kinds >= D2R_T_VIT_QKV only with "timing" 2)
    void timing_end(size_t pair);
};
enum { D2R_T_MARCH = 0, D2R_T_RAYGEN = 1, D2R_T_CLIP = 2, D2R_T_PREP = 3, D2R_T_SORT = 4,
       // "timing" 2: the vision tower's products, one pair of events per launch (full-size launches of the default schedule only:
       // layer 0's compact QKV under l0_reuse and the class-token-only last block stay inside D2R_T_CLIP's remainder)
       D2R_T_VIT_QKV = 5, D2R_T_VIT_ATTN = 6, D2R_T_VIT_OUT = 7, D2R_T_VIT_FC1 = 8, D2R_T_VIT_FC2 = 9, D2R_T_KINDS = 10 };

struct d2r_nerf {
    d2r_ctx *ctx;
    int device = 0;
    NerfParams P{};
    D2rDev<uint32_t> d_grid, d_brick_tab, d_gbrick_tab;
    D2rDev<uint64_t> d_bricks;
    D2rDev<uint4> d_wfrag;
};

// a coloured point cloud on a device: uploaded by d2r_pcd_create (pcd.hip) or built there by d2r_pcd_build (pcdbuild.hip)
struct d2r_pcd {
    int device = 0;
    uint32_t n = 0;
    D2rDev<float4> xyz;          // [n] (x, y, z, 0)
    D2rDev<uint32_t> rgb;        // [n] r | g << 8 | b << 16
};

// hipFuncSetAttribute once per (kernel instantiation, device), safe when different contexts are driven from
// different threads: one static instance per call site
struct PerDeviceOnce {
    std::once_flag flag[D2R_MAX_DEVICES];
    template <class F>
    void run(int device, F &&fn) { std::call_once(flag[device % D2R_MAX_DEVICES], fn); }
};

// tsdf.hip: a volume as its readers (tsdfvis.hip, camtrack.hip) see it: D2rTsdfDev of tsdf_sample.h, which kernels take by value
bool d2r_tsdf_has_colour(const d2r_tsdf *v);
int d2r_tsdf_device(const d2r_tsdf *v);
float d2r_tsdf_voxel(const d2r_tsdf *v);
int d2r_tsdf_dev(d2r_ctx *ctx, d2r_tsdf *v, D2rTsdfDev *out);     // reads the block flags back when frames arrived since the last call (synchronises); the cells are the box's (cells_of_box)

int d2r_pcd_check_view(d2r_ctx *ctx, const d2r_pcd_view *view);      // pcd.hip: the limits d2r_pcd_render holds a view to (meshvis.hip shares them)

// phys.hip: the host side the two physics pre-filters (hulls + GJK in phys.hip, points against the TSDF field in sdfphys.hip) share
int d2r_phys_orientations(d2r_ctx *, const d2r_phys_params *, uint32_t N, uint64_t *oris_out);      // checks N against sample_res -> orientations per position
std::vector<uint8_t> d2r_phys_orientation_mask(const d2r_phys_params *, const float *pose_batch, const uint8_t *valid_io, uint32_t oris);   // [oris] 0: duplicate orientation / not regraspable

// clip.hip: what captions.hip reaches of the vision tower (the tower entry itself, d2r_clip_forward, is declared where it is called)
struct d2r_clip;
uint32_t d2r_clip_patch_size(const d2r_clip *);
uint32_t d2r_clip_patch_stride(const d2r_clip *);      // bf16 elements per patch row of the tower's input (Kp_pad)
int d2r_clip_resample_coeffs(int in_size, int out_size, int first, int count, std::vector<int> &bounds, std::vector<int> &kk);   // Pillow's fixed-point bicubic tables as prep_tables builds them, for the output positions first .. first + count - 1 -> ksize

// api.hip: what the entry points that score frames share
struct d2r_clip;
uint32_t d2r_pass_size(const d2r_ctx *, const d2r_clip *clip, size_t px);      // candidates per pass: option "chunk" under the model's (clip, optional) and the ray queue's (px per frame, 0 = no rays) 32-bit bounds
uint32_t d2r_frame_pass_size(uint32_t per, size_t px);                        // ... bounded further when the frames of a pass leave the GPU
int d2r_upload_text(d2r_ctx *, const d2r_clip *, const float *text, uint32_t C);   // checks the caller's [C][proj] text embeddings and queues them into ctx->text through a pinned slot
// for each pass [c0, c0 + nc): fill(c0, nc) must leave nc frames [nc][h][w][3] in ctx->frames on ctx->stream
int d2r_score_frames_chunked(d2r_ctx *, const d2r_clip *, uint32_t n, uint32_t w, uint32_t h, int rot90, uint32_t C, float logit_scale,
                             const std::function<int(uint32_t c0, uint32_t nc)> &fill, float *logits_out, float *embeds_out /* optional */,
                             uint8_t *frames_out /* optional */);

// nerf.hip launchers
int d2r_launch_cameras_direct(d2r_ctx *, const ViewParams &, const float *cams_nerf_dev, uint32_t n,
                              float *cams_out);
int d2r_launch_cameras_virtual(d2r_ctx *, const ViewParams &, const float *obj_now16,
                               const float *cam16, const float *obj_poses_dev, uint32_t n,
                               float *cams_out);
int d2r_launch_render(d2r_ctx *, const d2r_nerf *, const ViewParams &, const float *cams_dev,
                      uint32_t n, bool composite, float *rgba_dev, float *depth_dev,
                      uint8_t *frames_dev, void *rects_dev = nullptr);     // a view with a lens comes with its table attached (d2r_lens_table)
int d2r_launch_bg_quantize(d2r_ctx *, uint32_t w, uint32_t h);
ViewParams d2r_view_params(const d2r_view *v);
int d2r_reserve_render(d2r_ctx *, size_t rays);    // ray queue (+ sorted copy and bin counts with the ray sort) for a pass of `rays` rays
int d2r_lens_table(d2r_ctx *, ViewParams &V);      // attaches the view's undistorted-direction table (built, and the stream synchronised, on a new view: call it before a chunk loop)
