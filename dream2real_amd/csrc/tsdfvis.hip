// tsdfvis.hip — the colour-TSDF visual model's ray caster (vis_backend "tsdf") and its fused render-and-score call.  This package's
// own third visual backend: nothing here stands where a stage of the reference stands.  The rule is DESIGN.md section 2i, restated
// in numpy by tests/tsdfvis_ref.py and held to it byte for byte; how a sample point meets a volume (its cell, the eight corners and
// the weight rule, the trilinear value) is tsdf_sample.h's, which camtrack.hip reads through too: every step is one IEEE fp32
// operation in a written order, nothing is contracted (the library is built with -ffp-contract=off), the divides are correctly rounded.
//
// A volume stays put and the ray moves: pixel (i, j) casts d_c = ((j - cx) / fx, (i - cy) / fy, 1), so the ray parameter is the
// camera depth whatever the volume, and the depth test between the two volumes compares it.
//   background pass (once per call): one lane per pixel marches the background volume -> a colour frame and a depth image
//   candidate pass: one workgroup per (candidate, 16 x 16 pixel tile), a wave on an 8 x 8 patch so that its lanes walk neighbouring
//   voxels; inside the candidate's rectangle a lane marches the movable volume and keeps its hit where it is strictly nearer
//   than the background's, elsewhere it copies the background pixel
// Samples are indexed by the integer s.  What is skipped is proven unobserved: indices whose point lies outside the box of the
// blocks any frame touched (a padded fp64 slab test per ray), cells whose own block no frame touched (one byte), pixels outside
// the box's projected rectangle (tsdfvis_rect.h).  No scratch, no LDS.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "d2r_internal.h"
#include "tsdfvis_rect.h"

namespace {

constexpr uint32_t TV_THREADS = 256;
constexpr int TV_TILE = 16;                  // a workgroup's pixel tile: 2 x 2 waves of 8 x 8 pixels
constexpr double TV_DEPTH_MAX = 3.0;         // the depth range of the frames the volumes were fused from (section 2c)
constexpr double TV_MAX_SAMPLES = 1048576.0; // 2^20 samples a ray: (float)s * step stays well inside a step of exact

struct TvMat { float m[12]; };               // rows 0..2 of the rigid transform camera -> volume frame, row-major

struct TvCam {
    float fx, fy, cx, cy, near, thr;
    int32_t W, H, S;                         // S samples a ray: s = 0 .. S - 1
};

__device__ __forceinline__ void tv_colour(const D2rTsdfDev &V, size_t base, const float (&f)[3], uint8_t (&rgb)[3])
{
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = V.col[ts_corner(V, base, k) * 3 + ch];
        const float c = floorf(ts_lerp3(t, f) + 0.5f);
        rgb[ch] = (uint8_t)(int)fminf(fmaxf(c, 0.f), 255.f);        // (fmaxf drops a NaN: 0)
    }
}

// pixel (i, j)'s ray through the volume V under M -> the first front-face hit: its camera depth and colour
__device__ __forceinline__ bool tv_cast(const D2rTsdfDev &V, const TvMat &M, const TvCam &c, int i, int j, float &t_hit, uint8_t (&rgb)[3])
{
    const float x = ((float)j - c.cx) / c.fx, y = ((float)i - c.cy) / c.fy;
    float o[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = M.m[4 * a + 3];
        d[a] = (M.m[4 * a] * x + M.m[4 * a + 1] * y) + M.m[4 * a + 2];
    }
    // The sample indices whose point can lie in the touched-block box: a slab test in fp64 over the box widened by two voxels and by
    // what an fp32 sample point can be off, the index range widened by two.  Everything outside is unobserved.
    const double step = (double)V.voxel, near = (double)c.near, t_end = near + (double)c.S * step;
    double t0 = near, t1 = t_end;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double slack = 2.0 * step + 4e-6 * (fabs((double)o[a]) + t_end * fabs((double)d[a]));
        const double L = ((double)V.clo[a]) * step - slack, H = ((double)V.chi[a] + 2.0) * step + slack;
        const double oa = (double)o[a], da = (double)d[a];
        if (fabs(da) > 0.0) {
            const double ta = (L - oa) / da, tb = (H - oa) / da;
            t0 = fmax(t0, fmin(ta, tb));
            t1 = fmin(t1, fmax(ta, tb));
        } else if (oa < L || oa > H) {
            return false;
        }
    }
    if (!(t0 <= t1)) return false;                                  // (NaN: a miss, as every sample of such a ray is unobserved)
    const int s0 = (int)fmax(floor((t0 - near) / step) - 2.0, 0.0), s1 = (int)fmin(ceil((t1 - near) / step) + 2.0, (double)(c.S - 1));

    bool prev_ok = false;
    float prev_v = 0.f;
    for (int s = s0; s <= s1; ++s) {
        const float t = c.near + (float)s * V.voxel;
        const float p[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        size_t base = 0;
        float f[3], v = 0.f;
        // (the two calls stand here and below, not behind one helper of this unit: behind one the compiler kept fewer loads in
        // flight, 52 VGPRs for 63, and the candidates' casts measured 5 % slower)
        const bool ok = ts_cell<true>(V, p, base, f) && ts_tsdf(V, base, f, c.thr, v);
        if (ok && prev_ok && prev_v > 0.f && v <= 0.f) {
            const float tp = c.near + (float)(s - 1) * V.voxel;
            t_hit = tp + (V.voxel * prev_v) / (prev_v - v);
            const float ph[3] = {o[0] + t_hit * d[0], o[1] + t_hit * d[1], o[2] + t_hit * d[2]};
            size_t bh = 0;
            float fh[3], vh;
            if (ts_cell<true>(V, ph, bh, fh) && ts_tsdf(V, bh, fh, c.thr, vh)) tv_colour(V, bh, fh, rgb);
            else tv_colour(V, base, f, rgb);
            return true;
        }
        prev_ok = ok;
        prev_v = v;
    }
    return false;
}

// BG: the background volume under mats[0] -> bg_frame [H][W][3], bg_depth [H][W] (+inf: no hit).
// else: blockIdx.y = candidate k: frames[k] (and depths[k] when given) = the background's pixel, or the movable volume's hit under
// mats[k] where the pixel lies in rects[k] and the hit is strictly nearer
template <bool BG>
__global__ __launch_bounds__(TV_THREADS) void k_tv_cast(D2rTsdfDev V, const TvMat *__restrict__ mats, const int4 *__restrict__ rects, TvCam c,
                                                        uint8_t *__restrict__ bg_frame, float *__restrict__ bg_depth,
                                                        uint8_t *__restrict__ frames, float *__restrict__ depths)
{
    const uint32_t tiles_x = ((uint32_t)c.W + TV_TILE - 1) / TV_TILE;
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int j = (int)(tx * TV_TILE + (wave & 1u) * 8u + (lane & 7u)), i = (int)(ty * TV_TILE + (wave >> 1) * 8u + (lane >> 3));
    if (i >= c.H || j >= c.W) return;
    const size_t p = (size_t)i * c.W + j;
    uint8_t rgb[3] = {0, 0, 0};
    float t = INFINITY;
    if (BG) {
        const TvMat M = mats[0];
        if (!tv_cast(V, M, c, i, j, t, rgb)) {
            t = INFINITY;
            rgb[0] = rgb[1] = rgb[2] = 0;
        }
        bg_frame[p * 3] = rgb[0];
        bg_frame[p * 3 + 1] = rgb[1];
        bg_frame[p * 3 + 2] = rgb[2];
        bg_depth[p] = t;
    } else {
        const uint32_t k = blockIdx.y;
        const int4 r = rects[k];
        t = bg_depth[p];
        rgb[0] = bg_frame[p * 3];
        rgb[1] = bg_frame[p * 3 + 1];
        rgb[2] = bg_frame[p * 3 + 2];
        if (j >= r.x && j <= r.z && i >= r.y && i <= r.w) {
            const TvMat M = mats[k];
            uint8_t mc[3];
            float tm;
            if (tv_cast(V, M, c, i, j, tm, mc) && tm < t) {
                t = tm;
                rgb[0] = mc[0];
                rgb[1] = mc[1];
                rgb[2] = mc[2];
            }
        }
        const size_t q = (size_t)k * (size_t)c.W * (size_t)c.H + p;
        frames[q * 3] = rgb[0];
        frames[q * 3 + 1] = rgb[1];
        frames[q * 3 + 2] = rgb[2];
        if (depths) depths[q] = t;
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct TvCall {
    TvCam cam{};
    D2rTsdfDev bg{}, mv{};                   // the cells of the touched-block box
    uint32_t K = 0;
    size_t o_mats = 0, o_rects = 0;          // segments of ctx->tv_mats: [1 + K] matrices (the background's first), [K] rectangles
};

// the refusals: pure host work, nothing on the device yet
int tv_check(d2r_ctx *ctx, const d2r_tsdf *bg, const d2r_tsdf *mv, const d2r_pcd_view *view, const float *cam_pose, const float *obj_pose_now,
             const float *obj_poses, uint32_t K, float thr)
{
    if (!ctx || !bg || !mv || !view || !cam_pose || !obj_pose_now || (K && !obj_poses)) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (int rc = d2r_pcd_check_view(ctx, view)) return rc;
    if (!(thr > 0.f) || !std::isfinite(thr)) return d2r_fail(ctx, D2R_ERR_INVALID, "TSDF ray caster: weight_threshold must be > 0");
    if (d2r_tsdf_device(bg) != ctx->device || d2r_tsdf_device(mv) != ctx->device)
        return d2r_fail(ctx, D2R_ERR_INVALID, "TSDF ray caster: a volume belongs to another device");
    if (!d2r_tsdf_has_colour(bg) || !d2r_tsdf_has_colour(mv))
        return d2r_fail(ctx, D2R_ERR_INVALID,
                        "TSDF ray caster: a volume holds no colour (its frames must come through d2r_tsdf_integrate_rgb)");
    if (!d2r_is_rigid(cam_pose) || !d2r_is_rigid(obj_pose_now))
        return d2r_fail(ctx, D2R_ERR_INVALID, "TSDF ray caster: cam_pose and obj_pose_now must be finite rigid transforms");
    for (uint32_t k = 0; k < K; ++k)
        if (!d2r_is_rigid(obj_poses + (size_t)k * 16))
            return d2r_fail(ctx, D2R_ERR_INVALID, "TSDF ray caster: candidate pose " + std::to_string(k) + " is not a finite rigid transform");
    for (const d2r_tsdf *vol : {bg, mv})
        if (ceil((TV_DEPTH_MAX - (double)view->near) / (double)d2r_tsdf_voxel(vol)) > TV_MAX_SAMPLES)
            return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "TSDF ray caster: a ray would take more than 2^20 samples at this voxel size");
    return D2R_OK;
}

int samples(double near, float voxel) { return (int)std::max(0.0, ceil((TV_DEPTH_MAX - near) / (double)voxel)); }

// matrices and rectangles to the device, the background's cast -> ctx->tv_bg_frame / ctx->tv_bg_depth
int tv_prepare(d2r_ctx *ctx, d2r_tsdf *bg, d2r_tsdf *mv, const d2r_pcd_view *view, const float *cam_pose, const float *obj_pose_now,
               const float *obj_poses, uint32_t K, float thr, TvCall &call)
{
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    D2rTsdfDev &Db = call.bg, &Dm = call.mv;
    int rc;
    if ((rc = d2r_tsdf_dev(ctx, bg, &Db)) || (rc = d2r_tsdf_dev(ctx, mv, &Dm))) return rc;
    call.K = K;
    call.cam = TvCam{view->fx, view->fy, view->cx, view->cy, view->near, thr, (int32_t)view->width, (int32_t)view->height, 0};
    const TvCam &c = call.cam;

    // M_k = (O inv(P_k)) cam_pose in fp64, rounded once; the true fp64 inverse of the rounded matrix projects the movable volume's box
    double C4[16], O4[16], Pi[16], T[16], M[16], Minv[16];
    d2r_load16(cam_pose, C4);
    d2r_load16(obj_pose_now, O4);
    std::vector<TvMat> mats(1 + (size_t)K);
    std::vector<TvRect> rects(std::max<uint32_t>(K, 1), TvRect{0, 0, -1, -1});
    d2r_round34(C4, mats[0].m);
    const double step = (double)Dm.voxel, t_end = (double)c.near + (double)samples(c.near, Dm.voxel) * step;
    const double xmax = std::max(fabs(0.0 - (double)c.cx), fabs((double)c.W - 1.0 - (double)c.cx)) / fabs((double)c.fx);
    const double ymax = std::max(fabs(0.0 - (double)c.cy), fabs((double)c.H - 1.0 - (double)c.cy)) / fabs((double)c.fy);
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = ((double)Dm.box_lo[a] - 1.0) * step;             // a sample's point lies in [box_lo, box_hi + 1) voxels to be observed
        hi[a] = ((double)Dm.box_hi[a] + 2.0) * step;
    }
    for (uint32_t k = 0; k < K; ++k) {
        d2r_rigid_inverse4(obj_poses + (size_t)k * 16, Pi);
        d2r_mul4(O4, Pi, T);
        d2r_mul4(T, C4, M);
        d2r_round34(M, mats[1 + k].m);
        tv_inverse34(mats[1 + k].m, Minv);
        // what an fp32 sample point o + t d can be off: a few ulps of |o| + t |d|
        const double omax = std::max(fabs(M[3]), std::max(fabs(M[7]), fabs(M[11])));
        const double slack = 4e-6 * (omax + t_end * (xmax + ymax + 1.0));
        rects[k] = tv_box_rect(Minv, lo, hi, slack, c.fx, c.fy, c.cx, c.cy, c.near, c.W, c.H);
    }

    const size_t px = (size_t)c.W * c.H;
    D2rStage st(ctx, ctx->tv_mats);
    call.o_mats = st.add(mats.size() * sizeof(TvMat));
    call.o_rects = st.add(rects.size() * sizeof(TvRect));
    if ((rc = st.reserve()) || (rc = d2r_reserve(ctx, ctx->tv_bg_frame, px * 3)) || (rc = d2r_reserve(ctx, ctx->tv_bg_depth, px * 4))) return rc;
    if ((rc = ctx->tv_timer.mark(ctx, 0))) return rc;
    if ((rc = st.upload(call.o_mats, mats.data(), mats.size() * sizeof(TvMat))) || (rc = st.upload(call.o_rects, rects.data(), rects.size() * sizeof(TvRect))))
        return rc;
    if ((rc = ctx->tv_timer.mark(ctx, 1))) return rc;
    const uint32_t tiles = (((uint32_t)c.W + TV_TILE - 1) / TV_TILE) * (((uint32_t)c.H + TV_TILE - 1) / TV_TILE);
    TvCam cb = c;
    cb.S = samples(c.near, Db.voxel);
    hipLaunchKernelGGL(k_tv_cast<true>, dim3(tiles), dim3(TV_THREADS), 0, ctx->stream, call.bg, st.at<const TvMat>(call.o_mats),
                       st.at<const int4>(call.o_rects), cb, (uint8_t *)ctx->tv_bg_frame.p, (float *)ctx->tv_bg_depth.p, (uint8_t *)nullptr,
                       (float *)nullptr);
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = ctx->tv_timer.mark(ctx, 2))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));     // `mats` and `rects` (pageable host memory) have been consumed
    call.cam.S = samples(c.near, Dm.voxel);
    ctx->tv_cast_ms = ctx->tv_dl_ms = 0.0;
    ctx->tv_pass_pending = ctx->tv_dl_pending = false;
    return D2R_OK;
}

// the previous pass's cast has finished (every pass ends in a stream synchronisation): its time joins the sum
int tv_collect(d2r_ctx *ctx)
{
    double ms = 0.0;
    if (ctx->tv_pass_pending) {
        ctx->tv_pass_timer.done();
        if (int rc = ctx->tv_pass_timer.read(ctx, &ms, 1, "")) return rc;
        ctx->tv_cast_ms += ms;
        ctx->tv_pass_pending = false;
    }
    if (ctx->tv_dl_pending) {
        ctx->tv_dl_timer.done();
        if (int rc = ctx->tv_dl_timer.read(ctx, &ms, 1, "")) return rc;
        ctx->tv_dl_ms += ms;
        ctx->tv_dl_pending = false;
    }
    return D2R_OK;
}

// candidates k0 .. k0 + nc - 1 -> ctx->frames [nc][H][W][3] (reserved by the caller for its largest pass), depths [nc][H][W] when given
int tv_candidates(d2r_ctx *ctx, const TvCall &call, uint32_t k0, uint32_t nc, float *depths)
{
    int rc;
    if ((rc = tv_collect(ctx)) || (rc = ctx->tv_pass_timer.mark(ctx, 0))) return rc;
    const TvCam &c = call.cam;
    const uint32_t tiles = (((uint32_t)c.W + TV_TILE - 1) / TV_TILE) * (((uint32_t)c.H + TV_TILE - 1) / TV_TILE);
    const TvMat *mats = (const TvMat *)((const char *)ctx->tv_mats.p + call.o_mats) + 1 + k0;
    const int4 *rects = (const int4 *)((const char *)ctx->tv_mats.p + call.o_rects) + k0;
    hipLaunchKernelGGL(k_tv_cast<false>, dim3(tiles, nc), dim3(TV_THREADS), 0, ctx->stream, call.mv, mats, rects, c, (uint8_t *)ctx->tv_bg_frame.p,
                       (float *)ctx->tv_bg_depth.p, (uint8_t *)ctx->frames.p, depths);
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = ctx->tv_pass_timer.mark(ctx, 1))) return rc;
    ctx->tv_pass_pending = true;
    return D2R_OK;
}

}  // namespace

extern "C" {

int d2r_tsdfvis_render(d2r_ctx *ctx, d2r_tsdf *bg, d2r_tsdf *movable, const d2r_pcd_view *view, const float *cam_pose, const float *obj_pose_now,
                       const float *obj_poses, uint32_t K, float weight_threshold, uint8_t *frames_out, float *depth_out)
{
    if (ctx && K && !frames_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null frames_out");
    int rc = tv_check(ctx, bg, movable, view, cam_pose, obj_pose_now, obj_poses, K, weight_threshold);
    if (rc || K == 0) return rc;
    TvCall call;
    if ((rc = tv_prepare(ctx, bg, movable, view, cam_pose, obj_pose_now, obj_poses, K, weight_threshold, call))) return rc;
    const size_t px = (size_t)call.cam.W * call.cam.H, fb = px * 3;
    const uint32_t per = std::min<uint32_t>(d2r_frame_pass_size(d2r_pass_size(ctx, nullptr, 0), px), 65535u);
    if ((rc = d2r_reserve(ctx, ctx->frames, (size_t)std::min(per, K) * fb))) return rc;
    if (depth_out && (rc = d2r_reserve(ctx, ctx->tv_depth, (size_t)std::min(per, K) * px * 4))) return rc;
    for (uint32_t k0 = 0; k0 < K; k0 += per) {
        const uint32_t nc = std::min(per, K - k0);
        if ((rc = tv_candidates(ctx, call, k0, nc, depth_out ? (float *)ctx->tv_depth.p : nullptr))) return rc;
        if ((rc = ctx->tv_dl_timer.mark(ctx, 0))) return rc;
        D2R_HIP(ctx, hipMemcpyAsync(frames_out + (size_t)k0 * fb, ctx->frames.p, (size_t)nc * fb, hipMemcpyDeviceToHost, ctx->stream));
        if (depth_out)
            D2R_HIP(ctx, hipMemcpyAsync(depth_out + (size_t)k0 * px, ctx->tv_depth.p, (size_t)nc * px * 4, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = ctx->tv_dl_timer.mark(ctx, 1))) return rc;
        ctx->tv_dl_pending = true;
        D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if ((rc = tv_collect(ctx))) return rc;
    ctx->tv_timer.done();
    return D2R_OK;
}

int d2r_tsdfvis_render_score_host(d2r_ctx *ctx, d2r_tsdf *bg, d2r_tsdf *movable, const d2r_clip *clip, const d2r_pcd_view *view,
                                  const float *cam_pose, const float *obj_pose_now, const float *obj_poses, uint32_t K, float weight_threshold,
                                  const float *text_embeds, uint32_t C, float logit_scale, float *logits_out, uint8_t *frames_out)
{
    if (!ctx || !clip || (K && !logits_out)) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    int rc = tv_check(ctx, bg, movable, view, cam_pose, obj_pose_now, obj_poses, K, weight_threshold);
    if (rc) return rc;
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = d2r_upload_text(ctx, clip, text_embeds, C)) || K == 0) return rc;
    if (d2r_pass_size(ctx, clip, 0) > 65535u)
        return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "TSDF ray caster: a pass holds more than 65535 candidates (option \"chunk\")");
    TvCall call;
    if ((rc = tv_prepare(ctx, bg, movable, view, cam_pose, obj_pose_now, obj_poses, K, weight_threshold, call))) return rc;
    auto fill = [&](uint32_t k0, uint32_t nc) { return tv_candidates(ctx, call, k0, nc, nullptr); };
    if ((rc = d2r_score_frames_chunked(ctx, clip, K, (uint32_t)call.cam.W, (uint32_t)call.cam.H, 1, C, logit_scale, fill, logits_out, nullptr, frames_out)))
        return rc;
    if ((rc = tv_collect(ctx))) return rc;
    ctx->tv_timer.done();
    return D2R_OK;
}

int d2r_tsdfvis_get_timing(d2r_ctx *ctx, double *ms_out)
{
    if (!ctx || !ms_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (int rc = ctx->tv_timer.read(ctx, ms_out, 2, "d2r_tsdfvis_get_timing: no ray-cast call with K > 0 has completed on this context")) return rc;
    ms_out[2] = ctx->tv_cast_ms;
    ms_out[3] = ctx->tv_dl_ms;
    return D2R_OK;
}

}  // extern "C"
