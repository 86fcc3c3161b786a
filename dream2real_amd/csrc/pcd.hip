// pcd.hip — the point-cloud ablation renderer (reference vision_3d/pcd_visual_model.py:98-155, `use_vis_pcds`) and its
// fused render-and-score call.  The render rule is DESIGN.md section 2: pinhole projection, square point sprites, nearest
// point wins with ties to the lower global index, the winning point's 8-bit colour unchanged, white where no point lands,
// then the reference's "all three channels > 220 -> black" rule.
//
// Visibility is a minimum over the 64-bit key (float_bits(z) << 32) | global_index (z > near > 0, so the float bits order
// like the depths): the result does not depend on the order in which points are splatted.
//   background pass (once per call): every background point splats its sprite into a [H][W] key buffer with a global u64
//   atomic min; the buffer is resolved into the background colour frame.
//   candidate pass (one workgroup per candidate): the workgroup transforms the movable points with its candidate's matrix,
//   reduces the frame rectangle their sprites cover, copies the background frame outside it, and walks the rectangle in
//   LDS tiles: background keys in, LDS u64 atomic min of the movable sprites, colour out.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "d2r_internal.h"

namespace {

constexpr uint32_t PCD_THREADS = 256;
constexpr uint32_t PCD_TILE_PX = 4096;       // LDS keys per tile: 32 KiB
constexpr uint64_t PCD_EMPTY = ~0ull;

struct PcdMat { float m[12]; };              // rows 0..2 of a rigid transform, row-major

struct PcdCam {
    float fx, fy, cx, cy, near, half;        // half = point_size / 2
    int32_t W, H, ps;                        // ps = point_size (sprite side in pixels)
};

// DESIGN.md section 2, "arithmetic": fp32, in this order, no contraction (the library is built with -ffp-contract=off),
// correctly rounded divide.  -> false when the point is culled (z <= near) or its sprite misses the frame; else the
// camera-space depth and the first column / row of the sprite.
__device__ __forceinline__ bool pcd_project(const PcdMat &M, float4 p, const PcdCam &c, float &z, int &j0, int &i0)
{
    const float *m = M.m;
    float x = ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3];
    float y = ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7];
    z = ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11];
    if (!(z > c.near)) return false;
    float u = (c.fx * x) / z + c.cx;
    float v = (c.fy * y) / z + c.cy;
    float a = ceilf(u - c.half), b = ceilf(v - c.half);
    // columns a .. a + ps - 1 meet 0 .. W - 1 (NaN and infinities fail both tests)
    if (!(a > (float)-c.ps && a < (float)c.W)) return false;
    if (!(b > (float)-c.ps && b < (float)c.H)) return false;
    j0 = (int)a;
    i0 = (int)b;
    return true;
}

__device__ __forceinline__ uint64_t pcd_key(float z, uint32_t idx)
{
    return ((uint64_t)__float_as_uint(z) << 32) | idx;
}

// key -> the frame's three bytes: the winning point's colour, white where no point landed, then black for any pixel whose
// three channels are all > 220 (reference pcd_visual_model.py:145-147)
// (cols: the background's colours followed by the movable cloud's, indexed by the global index)
__device__ __forceinline__ void pcd_store_colour(uint64_t key, const uint32_t *cols, uint8_t *px)
{
    uint32_t c = 0xffffffu;
    if (key != PCD_EMPTY) c = cols[(uint32_t)key];
    uint32_t r = c & 255u, g = (c >> 8) & 255u, b = (c >> 16) & 255u;
    if (r > 220u && g > 220u && b > 220u) r = g = b = 0;
    px[0] = (uint8_t)r;
    px[1] = (uint8_t)g;
    px[2] = (uint8_t)b;
}

__global__ __launch_bounds__(PCD_THREADS) void k_pcd_splat_bg(const float4 *__restrict__ xyz, uint32_t n, PcdMat M, PcdCam c,
                                                              unsigned long long *__restrict__ keys)
{
    uint32_t i = blockIdx.x * PCD_THREADS + threadIdx.x;
    if (i >= n) return;
    float z;
    int j0, i0;
    if (!pcd_project(M, xyz[i], c, z, j0, i0)) return;
    const unsigned long long key = pcd_key(z, i);
    const int r0 = max(i0, 0), r1 = min(i0 + c.ps - 1, c.H - 1);
    const int q0 = max(j0, 0), q1 = min(j0 + c.ps - 1, c.W - 1);
    for (int r = r0; r <= r1; ++r)
        for (int q = q0; q <= q1; ++q)
            atomicMin(&keys[(size_t)r * c.W + q], key);
}

__global__ __launch_bounds__(PCD_THREADS) void k_pcd_resolve_bg(const unsigned long long *__restrict__ keys, uint32_t npx,
                                                                const uint32_t *__restrict__ cols, uint8_t *__restrict__ frame)
{
    uint32_t p = blockIdx.x * PCD_THREADS + threadIdx.x;
    if (p >= npx) return;
    pcd_store_colour(keys[p], cols, frame + (size_t)p * 3);
}

// one workgroup per candidate k: frames[k] = background + the movable cloud moved by mats[k]
__global__ __launch_bounds__(PCD_THREADS) void k_pcd_candidates(const float4 *__restrict__ mv_xyz, uint32_t nm, uint32_t nb,
                                                                const uint32_t *__restrict__ cols,
                                                                const PcdMat *__restrict__ mats, PcdCam c,
                                                                const unsigned long long *__restrict__ bg_keys,
                                                                const uint8_t *__restrict__ bg_frame, uint8_t *__restrict__ frames)
{
    __shared__ unsigned long long tile[PCD_TILE_PX];
    __shared__ int rect[4];                  // x0, y0 (min), x1, y1 (max): the clipped pixels the sprites cover
    const uint32_t t = threadIdx.x;
    const PcdMat M = mats[blockIdx.x];
    const uint32_t npx = (uint32_t)c.W * (uint32_t)c.H;
    uint8_t *frame = frames + (size_t)blockIdx.x * npx * 3;

    if (t == 0) {
        rect[0] = c.W;
        rect[1] = c.H;
        rect[2] = -1;
        rect[3] = -1;
    }
    __syncthreads();
    int lx0 = c.W, ly0 = c.H, lx1 = -1, ly1 = -1;
    for (uint32_t i = t; i < nm; i += PCD_THREADS) {
        float z;
        int j0, i0;
        if (!pcd_project(M, mv_xyz[i], c, z, j0, i0)) continue;
        lx0 = min(lx0, max(j0, 0));
        ly0 = min(ly0, max(i0, 0));
        lx1 = max(lx1, min(j0 + c.ps - 1, c.W - 1));
        ly1 = max(ly1, min(i0 + c.ps - 1, c.H - 1));
    }
    if (lx1 >= 0) {
        atomicMin(&rect[0], lx0);
        atomicMin(&rect[1], ly0);
        atomicMax(&rect[2], lx1);
        atomicMax(&rect[3], ly1);
    }
    __syncthreads();
    const int x0 = rect[0], y0 = rect[1], x1 = rect[2], y1 = rect[3];

    // outside the rectangle the frame is the background frame
    for (uint32_t p = t; p < npx; p += PCD_THREADS) {
        const int i = (int)(p / (uint32_t)c.W), j = (int)(p - (uint32_t)i * (uint32_t)c.W);
        if (i >= y0 && i <= y1 && j >= x0 && j <= x1) continue;
        const uint8_t *s = bg_frame + (size_t)p * 3;
        uint8_t *d = frame + (size_t)p * 3;
        d[0] = s[0];
        d[1] = s[1];
        d[2] = s[2];
    }
    if (x1 < x0) return;                     // no movable point on screen (uniform over the workgroup)

    const int rw = x1 - x0 + 1, rh = y1 - y0 + 1;
    const int tw = min(rw, (int)PCD_TILE_PX), th = min(rh, (int)PCD_TILE_PX / tw);
    for (int ty = y0; ty <= y1; ty += th) {
        const int ch = min(th, y1 - ty + 1);
        for (int tx = x0; tx <= x1; tx += tw) {
            const int cw = min(tw, x1 - tx + 1);
            const int n = cw * ch;
            for (int q = (int)t; q < n; q += PCD_THREADS) {
                const int r = q / cw;
                tile[q] = bg_keys[(size_t)(ty + r) * c.W + tx + (q - r * cw)];
            }
            __syncthreads();
            for (uint32_t i = t; i < nm; i += PCD_THREADS) {
                float z;
                int j0, i0;
                if (!pcd_project(M, mv_xyz[i], c, z, j0, i0)) continue;
                const int r0 = max(i0, ty), r1 = min(i0 + c.ps - 1, ty + ch - 1);
                const int q0 = max(j0, tx), q1 = min(j0 + c.ps - 1, tx + cw - 1);
                if (r0 > r1 || q0 > q1) continue;
                const unsigned long long key = pcd_key(z, nb + i);
                for (int r = r0; r <= r1; ++r)
                    for (int q = q0; q <= q1; ++q)
                        atomicMin(&tile[(r - ty) * cw + (q - tx)], key);
            }
            __syncthreads();
            for (int q = (int)t; q < n; q += PCD_THREADS) {
                const int r = q / cw;
                pcd_store_colour(tile[q], cols, frame + ((size_t)(ty + r) * c.W + tx + (q - r * cw)) * 3);
            }
            __syncthreads();                 // the next tile overwrites the keys
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side

PcdMat to_mat34(const double T[16]) { PcdMat M; d2r_round34(T, M.m); return M; }

int check_view(d2r_ctx *ctx, const d2r_pcd_view *v, PcdCam &c)
{
    if (!v) return d2r_fail(ctx, D2R_ERR_INVALID, "null view");
    if (v->width == 0 || v->height == 0 || v->width > 16384 || v->height > 16384)
        return d2r_fail(ctx, D2R_ERR_INVALID, "point-cloud view: width and height must be 1 .. 16384");
    if (!(v->point_size >= 1.f && v->point_size <= 16.f) || v->point_size != floorf(v->point_size))
        return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "point-cloud view: point_size must be a whole number of pixels, 1 .. 16");
    if (!(v->near >= 0.f) || !std::isfinite(v->near) || !std::isfinite(v->fx) || !std::isfinite(v->fy) ||
        !std::isfinite(v->cx) || !std::isfinite(v->cy))
        return d2r_fail(ctx, D2R_ERR_INVALID, "point-cloud view: intrinsics and near must be finite, near >= 0");
    c = PcdCam{v->fx, v->fy, v->cx, v->cy, v->near, v->point_size * 0.5f, (int32_t)v->width, (int32_t)v->height,
               (int32_t)v->point_size};
    return D2R_OK;
}

// argument checks, candidate matrices and the colour table to the device, background pass -> ctx->pcd_bg_keys / ctx->pcd_bg_frame
int pcd_prepare(d2r_ctx *ctx, const d2r_pcd *bg, const d2r_pcd *mv, const d2r_pcd_view *view, const float *cam_pose,
                const float *obj_pose_now, const float *obj_poses, uint32_t K, PcdCam &c)
{
    if (!ctx || !bg || !mv || !cam_pose || !obj_pose_now || (K && !obj_poses))
        return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    int rc = check_view(ctx, view, c);
    if (rc) return rc;
    if (bg->device != ctx->device || mv->device != ctx->device)
        return d2r_fail(ctx, D2R_ERR_INVALID, "point clouds belong to another device");
    if ((uint64_t)bg->n + mv->n >= 0xffffffffull)
        return d2r_fail(ctx, D2R_ERR_INVALID, "background + movable points must stay below 2^32 - 1");
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    double Ci[16], Oi[16], P[16], T[16], M[16];
    d2r_rigid_inverse4(cam_pose, Ci);
    d2r_rigid_inverse4(obj_pose_now, Oi);
    std::vector<PcdMat> mats(std::max<uint32_t>(K, 1));
    for (uint32_t k = 0; k < K; ++k) {
        d2r_load16(obj_poses + (size_t)k * 16, P);
        d2r_mul4(Ci, P, T);
        d2r_mul4(T, Oi, M);
        mats[k] = to_mat34(M);
    }
    const size_t px = (size_t)c.W * c.H;
    if ((rc = d2r_reserve(ctx, ctx->pcd_mats, mats.size() * sizeof(PcdMat)))) return rc;
    if ((rc = d2r_reserve(ctx, ctx->pcd_bg_keys, px * 8))) return rc;
    if ((rc = d2r_reserve(ctx, ctx->pcd_bg_frame, px * 3))) return rc;
    if ((rc = d2r_reserve(ctx, ctx->pcd_cols, ((size_t)bg->n + mv->n) * 4 + 4))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(ctx->pcd_cols.p, bg->rgb.get(), (size_t)bg->n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync((uint32_t *)ctx->pcd_cols.p + bg->n, mv->rgb.get(), (size_t)mv->n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(ctx->pcd_mats.p, mats.data(), (size_t)K * sizeof(PcdMat), hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemsetAsync(ctx->pcd_bg_keys.p, 0xff, px * 8, ctx->stream));
    if (bg->n)
        hipLaunchKernelGGL(k_pcd_splat_bg, dim3((bg->n + PCD_THREADS - 1) / PCD_THREADS), dim3(PCD_THREADS), 0, ctx->stream,
                           bg->xyz.get(), bg->n, to_mat34(Ci), c, (unsigned long long *)ctx->pcd_bg_keys.p);
    hipLaunchKernelGGL(k_pcd_resolve_bg, dim3((uint32_t)((px + PCD_THREADS - 1) / PCD_THREADS)), dim3(PCD_THREADS), 0, ctx->stream,
                       (const unsigned long long *)ctx->pcd_bg_keys.p, (uint32_t)px, (const uint32_t *)ctx->pcd_cols.p,
                       (uint8_t *)ctx->pcd_bg_frame.p);
    D2R_HIP(ctx, hipGetLastError());
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));     // `mats` (pageable host memory) has been consumed
    return D2R_OK;
}

// candidates k0 .. k0 + nc - 1 -> ctx->frames [nc][H][W][3] (reserved by the caller for its largest pass)
int pcd_candidates(d2r_ctx *ctx, const d2r_pcd *bg, const d2r_pcd *mv, const PcdCam &c, uint32_t k0, uint32_t nc)
{
    hipLaunchKernelGGL(k_pcd_candidates, dim3(nc), dim3(PCD_THREADS), 0, ctx->stream, mv->xyz.get(), mv->n, bg->n, (const uint32_t *)ctx->pcd_cols.p,
                       (const PcdMat *)ctx->pcd_mats.p + k0, c, (const unsigned long long *)ctx->pcd_bg_keys.p,
                       (const uint8_t *)ctx->pcd_bg_frame.p, (uint8_t *)ctx->frames.p);
    D2R_HIP(ctx, hipGetLastError());
    return D2R_OK;
}

}  // namespace

int d2r_pcd_check_view(d2r_ctx *ctx, const d2r_pcd_view *view)
{
    PcdCam c;
    return check_view(ctx, view, c);
}

extern "C" {

int d2r_pcd_create(d2r_ctx *ctx, const float *xyz, const uint8_t *rgb, uint32_t n, d2r_pcd **out)
{
    if (!ctx || !out || (n && (!xyz || !rgb))) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (n >= 0xffffffffu) return d2r_fail(ctx, D2R_ERR_INVALID, "too many points");
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<float4> p(std::max<uint32_t>(n, 1), float4{0.f, 0.f, 0.f, 0.f});
    std::vector<uint32_t> col(std::max<uint32_t>(n, 1), 0u);
    for (uint32_t i = 0; i < n; ++i) {
        p[i] = float4{xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], 0.f};
        col[i] = d2r_pack_rgb(rgb + 3 * (size_t)i);
    }
    std::unique_ptr<d2r_pcd> m(new d2r_pcd);
    m->device = ctx->device;
    m->n = n;
    int rc;
    if ((rc = m->xyz.alloc(ctx, p.size() * sizeof(float4), "a point cloud")) || (rc = m->rgb.alloc(ctx, col.size() * 4, "a point cloud"))) return rc;
    D2R_HIP(ctx, hipMemcpy(m->xyz.get(), p.data(), p.size() * sizeof(float4), hipMemcpyHostToDevice));
    D2R_HIP(ctx, hipMemcpy(m->rgb.get(), col.data(), col.size() * 4, hipMemcpyHostToDevice));
    *out = m.release();
    return D2R_OK;
}

void d2r_pcd_destroy(d2r_pcd *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    delete m;
}

int d2r_pcd_render(d2r_ctx *ctx, const d2r_pcd *bg, const d2r_pcd *movable, const d2r_pcd_view *view, const float *cam_pose,
                   const float *obj_pose_now, const float *obj_poses, uint32_t K, uint8_t *frames_out)
{
    if (K && !frames_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null frames_out");
    PcdCam c;
    int rc = pcd_prepare(ctx, bg, movable, view, cam_pose, obj_pose_now, obj_poses, K, c);
    if (rc) return rc;
    const size_t fb = (size_t)c.W * c.H * 3;
    const uint32_t per = d2r_frame_pass_size(d2r_pass_size(ctx, nullptr, 0), (size_t)c.W * c.H);
    if ((rc = d2r_reserve(ctx, ctx->frames, (size_t)std::min(per, K) * fb))) return rc;
    for (uint32_t k0 = 0; k0 < K; k0 += per) {
        const uint32_t nc = std::min(per, K - k0);
        if ((rc = pcd_candidates(ctx, bg, movable, c, k0, nc))) return rc;
        D2R_HIP(ctx, hipMemcpyAsync(frames_out + (size_t)k0 * fb, ctx->frames.p, (size_t)nc * fb, hipMemcpyDeviceToHost, ctx->stream));
        D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return D2R_OK;
}

int d2r_pcd_render_score_host(d2r_ctx *ctx, const d2r_pcd *bg, const d2r_pcd *movable, const d2r_clip *clip,
                              const d2r_pcd_view *view, const float *cam_pose, const float *obj_pose_now, const float *obj_poses,
                              uint32_t K, const float *text_embeds, uint32_t C, float logit_scale, float *logits_out,
                              uint8_t *frames_out)
{
    if (!ctx || !clip || (K && !logits_out)) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    int rc = d2r_upload_text(ctx, clip, text_embeds, C);      // (the text is checked before the point clouds and the view, as ever)
    if (rc) return rc;
    PcdCam c;
    if ((rc = pcd_prepare(ctx, bg, movable, view, cam_pose, obj_pose_now, obj_poses, K, c))) return rc;
    auto fill = [&](uint32_t k0, uint32_t nc) { return pcd_candidates(ctx, bg, movable, c, k0, nc); };
    return d2r_score_frames_chunked(ctx, clip, K, (uint32_t)c.W, (uint32_t)c.H, 1, C, logit_scale, fill, logits_out, nullptr, frames_out);
}

}  // extern "C"
