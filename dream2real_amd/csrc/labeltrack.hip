// labeltrack.hip — the first frame's label image carried through a scan by geometry (tracker="geometric").  This package's own
// stand-in for the video-object-segmentation network the reference tracks its labels with; nothing here stands where reference code
// stands.  The rule is DESIGN.md section 2k, restated in numpy by tests/labeltrack_ref.py and held to it by equality of every byte;
// the grid and the refusals are labeltrack_grid.h's.  Every fp32 step is one IEEE operation in the written order (the library is built
// with -ffp-contract=off).
//   k_lt_predict  one lane per pixel: back-projection, one 2-byte gather from the (label, count) grid
//   k_lt_fill     one workgroup per 64 x 64 tile: the tile and a halo of 8 pixels (labels and depth) in LDS, up to 8 Jacobi sweeps
//                 there, the interior written back.  A label travels one pixel a sweep, so the interior is what 8 sweeps over the
//                 whole frame give.  ceil(grow / 8) launches ping-pong between two planes; a launch that finds the one before it
//                 changed nothing returns at once (the two planes are equal from then on)
//   k_lt_finish   one lane per pixel: unknown -> 0 into the result frame, the frame's counters
//   k_lt_vote     one lane per voxel, lanes along x, the whole grid once per frame: Boyer-Moore on one uint16 per voxel
// Ordinary vector stores; the only atomics are integer adds on the per-frame counters; no scratch.
#include <string.h>

#include <algorithm>
#include <vector>

#include "d2r_internal.h"
#include "labeltrack_grid.h"

namespace {

constexpr uint32_t LT_THREADS = 256;
constexpr int LT_TILE = 64, LT_HALO = (int)LT_SWEEPS, LT_SIDE = LT_TILE + 2 * LT_HALO;
constexpr uint32_t LT_STATS = 4;               // device counters per frame: known after predict, known after the fill, unused, launches that changed

struct LtFrame {
    float m[12];                               // cam_pose, rows 0..2
    float inv[12];                             // inv(cam_pose), rows 0..2: [R^T | -R^T t] composed in fp64, rounded to fp32
};

struct LtCam {
    float fx, fy, cx, cy;
    int32_t W, H;
};

__device__ __forceinline__ bool lt_depth_ok(float z) { return z > 0.f && z <= LT_DEPTH_MAX; }

__global__ __launch_bounds__(LT_THREADS) void k_lt_predict(LtGrid G, LtCam c, const LtFrame *__restrict__ fr, const uint16_t *__restrict__ depth,
                                                           const uint16_t *__restrict__ vol, uint8_t *__restrict__ plane, uint32_t *__restrict__ stats)
{
    const uint32_t p = blockIdx.x * LT_THREADS + threadIdx.x, px = (uint32_t)c.W * (uint32_t)c.H;
    uint32_t lab = LT_UNKNOWN;
    if (p < px) {
        const int i = (int)(p / (uint32_t)c.W), j = (int)(p - (uint32_t)i * (uint32_t)c.W);
        const float z = (float)depth[p] / 1000.0f;
        if (lt_depth_ok(z)) {
            const float xc = (((float)j - c.cx) / c.fx) * z, yc = (((float)i - c.cy) / c.fy) * z;
            bool ok = true;
            uint32_t g[3] = {0, 0, 0};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float pw = ((fr->m[4 * a] * xc + fr->m[4 * a + 1] * yc) + fr->m[4 * a + 2] * z) + fr->m[4 * a + 3];
                const float gf = floorf(pw / G.voxel + 0.5f);
                const bool in = gf >= (float)G.lo[a] && gf <= (float)(G.lo[a] + (int32_t)(G.n[a] - 1));      // (NaN fails)
                ok = ok && in;
                g[a] = in ? (uint32_t)((int32_t)gf - G.lo[a]) : 0u;
            }
            if (ok) {
                const uint32_t s = vol[((size_t)g[2] * G.n[1] + g[1]) * G.n[0] + g[0]];
                if (s >> 8) lab = s & 255u;
            }
        }
        plane[p] = (uint8_t)lab;
    }
    const unsigned long long known = __ballot(lab != LT_UNKNOWN);
    if ((threadIdx.x & 63u) == 0 && known) atomicAdd(&stats[0], (uint32_t)__popcll(known));
}

// what neighbour (rq, cq) offers the unknown pixel of depth dp (0 = no depth): its label when it gives, and the difference
__device__ __forceinline__ void lt_offer(const uint8_t (*lab)[LT_SIDE], const uint16_t (*dep)[LT_SIDE], int rq, int cq, uint32_t dp, uint32_t tau,
                                         uint32_t &best, uint32_t &v)
{
    if (rq < 0 || rq >= LT_SIDE || cq < 0 || cq >= LT_SIDE) return;
    const uint32_t lq = lab[rq][cq];
    if (lq == LT_UNKNOWN) return;
    uint32_t diff = 0;
    if (dp != 0) {
        const uint32_t dq = dep[rq][cq];
        if (dq == 0) return;
        diff = dp > dq ? dp - dq : dq - dp;
        if (diff > tau) return;
    }
    if (diff < best) {
        best = diff;
        v = lq;
    }
}

__global__ __launch_bounds__(LT_THREADS) void k_lt_fill(LtCam c, const uint16_t *__restrict__ depth, const uint8_t *__restrict__ src,
                                                        uint8_t *__restrict__ dst, uint32_t sweeps, uint32_t tau, const uint32_t *__restrict__ prev_chg,
                                                        uint32_t *__restrict__ chg)
{
    if (prev_chg && *prev_chg == 0) return;                  // the launch before changed nothing: dst equals src already
    __shared__ uint8_t lab[2][LT_SIDE][LT_SIDE];
    __shared__ uint16_t dep[LT_SIDE][LT_SIDE];               // millimetres where the depth is valid, else 0
    const int t = (int)threadIdx.x;
    const int tx0 = (int)blockIdx.x * LT_TILE - LT_HALO, ty0 = (int)blockIdx.y * LT_TILE - LT_HALO;
    for (int q = t; q < LT_SIDE * LT_SIDE; q += (int)LT_THREADS) {
        const int r = q / LT_SIDE, cc = q - r * LT_SIDE;
        const int gi = ty0 + r, gj = tx0 + cc;
        uint8_t l = (uint8_t)LT_UNKNOWN;
        uint16_t d = 0;
        if (gi >= 0 && gi < c.H && gj >= 0 && gj < c.W) {
            const size_t at = (size_t)gi * c.W + gj;
            l = src[at];
            const uint16_t raw = depth[at];
            if (lt_depth_ok((float)raw / 1000.0f)) d = raw;
        }
        lab[0][r][cc] = l;
        lab[1][r][cc] = l;                                   // cells outside the frame stay unknown in both
        dep[r][cc] = d;
    }
    __syncthreads();
    int cur = 0;
    for (uint32_t s = 0; s < sweeps; ++s) {
        for (int q = t; q < LT_SIDE * LT_SIDE; q += (int)LT_THREADS) {
            const int r = q / LT_SIDE, cc = q - r * LT_SIDE;
            const int gi = ty0 + r, gj = tx0 + cc;
            if (!(gi >= 0 && gi < c.H && gj >= 0 && gj < c.W)) continue;
            uint32_t v = lab[cur][r][cc];
            if (v == LT_UNKNOWN) {
                const uint32_t dp = dep[r][cc];
                uint32_t best = 0xffffffffu;
                lt_offer(lab[cur], dep, r - 1, cc, dp, tau, best, v);       // N, W, E, S: a tie goes to the earlier one
                lt_offer(lab[cur], dep, r, cc - 1, dp, tau, best, v);
                lt_offer(lab[cur], dep, r, cc + 1, dp, tau, best, v);
                lt_offer(lab[cur], dep, r + 1, cc, dp, tau, best, v);
            }
            lab[cur ^ 1][r][cc] = (uint8_t)v;
        }
        __syncthreads();
        cur ^= 1;
    }
    int changed = 0;
    for (int q = t; q < LT_TILE * LT_TILE; q += (int)LT_THREADS) {
        const int r = q / LT_TILE, cc = q - r * LT_TILE;
        const int gi = ty0 + LT_HALO + r, gj = tx0 + LT_HALO + cc;
        if (gi < c.H && gj < c.W) {
            const size_t at = (size_t)gi * c.W + gj;
            const uint8_t v = lab[cur][LT_HALO + r][LT_HALO + cc];
            changed |= v != src[at];
            dst[at] = v;
        }
    }
    if (__syncthreads_or(changed) && t == 0) *chg = 1u;
}

__global__ __launch_bounds__(LT_THREADS) void k_lt_finish(uint32_t px, const uint8_t *__restrict__ plane, uint8_t *__restrict__ out,
                                                          uint32_t *__restrict__ stats, const uint32_t *__restrict__ chg, uint32_t n_launch)
{
    const uint32_t p = blockIdx.x * LT_THREADS + threadIdx.x;
    bool is_known = false;
    if (p < px) {
        const uint8_t v = plane[p];
        is_known = v != LT_UNKNOWN;
        out[p] = is_known ? v : (uint8_t)0;
    }
    const unsigned long long known = __ballot(is_known);
    if ((threadIdx.x & 63u) == 0 && known) atomicAdd(&stats[1], (uint32_t)__popcll(known));
    if (p == 0) {
        uint32_t s = 0;
        for (uint32_t l = 0; l < n_launch; ++l) s += chg[l];
        stats[3] = s;
    }
}

__global__ __launch_bounds__(LT_THREADS) void k_lt_vote(LtGrid G, LtCam c, const LtFrame *__restrict__ fr, const uint16_t *__restrict__ depth,
                                                        const uint8_t *__restrict__ plane, uint16_t *__restrict__ vol)
{
    for (uint32_t idx = blockIdx.x * LT_THREADS + threadIdx.x; idx < G.n_vox; idx += gridDim.x * LT_THREADS) {
        const uint32_t row = idx / G.n[0], x = idx - row * G.n[0], z = row / G.n[1], y = row - z * G.n[1];
        const float px = (float)(G.lo[0] + (int32_t)x) * G.voxel, py = (float)(G.lo[1] + (int32_t)y) * G.voxel, pz = (float)(G.lo[2] + (int32_t)z) * G.voxel;
        const float xc = ((fr->inv[0] * px + fr->inv[1] * py) + fr->inv[2] * pz) + fr->inv[3];
        const float yc = ((fr->inv[4] * px + fr->inv[5] * py) + fr->inv[6] * pz) + fr->inv[7];
        const float zc = ((fr->inv[8] * px + fr->inv[9] * py) + fr->inv[10] * pz) + fr->inv[11];
        if (!(zc > 0.f)) continue;
        const float u = floorf(((c.fx * xc) / zc + c.cx) + 0.5f);
        const float v = floorf(((c.fy * yc) / zc + c.cy) + 0.5f);
        if (!(u >= 0.f && u < (float)c.W && v >= 0.f && v < (float)c.H)) continue;              // (NaN fails)
        const size_t at = (size_t)(int)v * c.W + (int)u;
        const float zp = (float)depth[at] / 1000.0f;
        if (!lt_depth_ok(zp) || !(fabsf(zp - zc) <= G.band)) continue;
        const uint32_t l = plane[at];
        if (l == LT_UNKNOWN) continue;
        const uint32_t s = vol[idx];
        uint32_t lab = s & 255u, cnt = s >> 8;
        if (cnt == 0) {
            lab = l;
            cnt = 1;
        } else if (lab == l) {
            cnt = min(cnt + 1u, 255u);
        } else {
            cnt -= 1;                            // at 0 the old label byte stays; the voxel counts as unknown
        }
        vol[idx] = (uint16_t)(lab | cnt << 8);
    }
}

}  // namespace

extern "C" {

int d2r_labeltrack_grid(const double *bounds, const d2r_labeltrack_params *params, uint32_t *dims_out, int32_t *lo_out)
{
    if (!dims_out || !lo_out) return d2r_fail(nullptr, D2R_ERR_INVALID, "null argument");
    LtGrid G;
    if (int rc = lt_grid(nullptr, bounds, params, &G)) return rc;
    for (int a = 0; a < 3; ++a) {
        dims_out[a] = G.n[a];
        lo_out[a] = G.lo[a];
    }
    return D2R_OK;
}

int d2r_labeltrack_scan(d2r_ctx *ctx, const double *bounds, const d2r_labeltrack_params *params, uint32_t n, uint32_t w, uint32_t h,
                        const double *K, const uint16_t *d16, const float *cam_poses, const uint8_t *labels0, uint8_t *labels_out,
                        uint32_t *stats_out, uint16_t *vol_out, uint32_t *vol_dims_out, int32_t *vol_lo_out)
{
    if (!ctx) return d2r_fail(nullptr, D2R_ERR_INVALID, "null argument");
    LtGrid G;
    int rc;
    if ((rc = lt_grid(ctx, bounds, params, &G)) || (rc = lt_check_frames(ctx, n, w, h, K, d16, cam_poses, labels0, labels_out))) return rc;
    D2R_HIP(ctx, hipSetDevice(ctx->device));

    const size_t px = (size_t)w * h;
    const uint32_t n_launch = (params->grow + LT_SWEEPS - 1) / LT_SWEEPS, per = LT_STATS + n_launch;
    std::vector<LtFrame> frames(n);
    for (uint32_t f = 0; f < n; ++f) {
        const float *T = cam_poses + (size_t)f * 16;
        double inv[12];
        d2r_rigid_inverse(T, inv);
        for (int i = 0; i < 12; ++i) {
            frames[f].m[i] = T[i];
            frames[f].inv[i] = (float)inv[i];
        }
    }
    const LtCam c{(float)K[0], (float)K[1], (float)K[2], (float)K[3], (int32_t)w, (int32_t)h};

    D2rDev<uint16_t> vol;
    D2rDrain drain{ctx->stream};
    if ((rc = vol.alloc(ctx, (size_t)G.n_vox * 2, "a label volume"))) return rc;
    D2rStage in(ctx, ctx->lt_in), ws(ctx, ctx->lt_ws);
    const size_t o_depth = in.add((size_t)n * px * 2), o_lab0 = in.add(px), o_fr = in.add((size_t)n * sizeof(LtFrame));
    const size_t o_a = ws.add(px), o_b = ws.add(px), o_out = ws.add((size_t)n * px), o_cnt = ws.add((size_t)n * per * 4);
    if ((rc = in.reserve()) || (rc = ws.reserve())) return rc;
    D2rStageTimer &timer = ctx->lt_timer;
    if ((rc = timer.mark(ctx, 0))) return rc;
    if ((rc = in.upload(o_depth, d16, (size_t)n * px * 2)) || (rc = in.upload(o_lab0, labels0, px)) ||
        (rc = in.upload(o_fr, frames.data(), (size_t)n * sizeof(LtFrame))))
        return rc;
    if ((rc = timer.mark(ctx, 1))) return rc;

    const uint16_t *depth = in.at<uint16_t>(o_depth);
    const LtFrame *fr = in.at<LtFrame>(o_fr);
    uint8_t *plane[2] = {ws.at<uint8_t>(o_a), ws.at<uint8_t>(o_b)}, *out = ws.at<uint8_t>(o_out);
    uint32_t *cnt = ws.at<uint32_t>(o_cnt);
    D2R_HIP(ctx, hipMemsetAsync(vol.get(), 0, (size_t)G.n_vox * 2, ctx->stream));
    D2R_HIP(ctx, hipMemsetAsync(cnt, 0, (size_t)n * per * 4, ctx->stream));
    const dim3 pix_grid((uint32_t)((px + LT_THREADS - 1) / LT_THREADS)), tile_grid((w + LT_TILE - 1) / LT_TILE, (h + LT_TILE - 1) / LT_TILE);
    const dim3 vox_grid(std::max(1u, std::min((G.n_vox + LT_THREADS - 1) / LT_THREADS, (uint32_t)ctx->n_cu * 8u)));
    for (uint32_t f = 0; f < n; ++f) {
        const uint16_t *df = depth + (size_t)f * px;
        uint32_t *stats = cnt + (size_t)f * per, *chg = stats + LT_STATS;
        int cur = 0;
        if (f == 0) {
            D2R_HIP(ctx, hipMemcpyAsync(plane[0], in.at<uint8_t>(o_lab0), px, hipMemcpyDeviceToDevice, ctx->stream));
            D2R_HIP(ctx, hipMemcpyAsync(out, in.at<uint8_t>(o_lab0), px, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            hipLaunchKernelGGL(k_lt_predict, pix_grid, dim3(LT_THREADS), 0, ctx->stream, G, c, fr + f, df, (const uint16_t *)vol.get(), plane[0], stats);
            for (uint32_t l = 0; l < n_launch; ++l) {
                const uint32_t sweeps = std::min(LT_SWEEPS, params->grow - l * LT_SWEEPS);
                hipLaunchKernelGGL(k_lt_fill, tile_grid, dim3(LT_THREADS), 0, ctx->stream, c, df, (const uint8_t *)plane[cur], plane[cur ^ 1], sweeps,
                                   params->tau_mm, l ? (const uint32_t *)(chg + l - 1) : (const uint32_t *)nullptr, chg + l);
                cur ^= 1;
            }
            hipLaunchKernelGGL(k_lt_finish, pix_grid, dim3(LT_THREADS), 0, ctx->stream, (uint32_t)px, (const uint8_t *)plane[cur], out + (size_t)f * px,
                               stats, (const uint32_t *)chg, n_launch);
        }
        hipLaunchKernelGGL(k_lt_vote, vox_grid, dim3(LT_THREADS), 0, ctx->stream, G, c, fr + f, df, (const uint8_t *)plane[cur], vol.get());
        D2R_HIP(ctx, hipGetLastError());
    }
    if ((rc = timer.mark(ctx, 2))) return rc;

    // results come back aside and reach the caller once the whole call has succeeded
    std::vector<uint8_t> h_out((size_t)n * px);
    std::vector<uint32_t> h_cnt(stats_out ? (size_t)n * per : 0);
    std::vector<uint16_t> h_vol(vol_out ? (size_t)G.n_vox : 0);
    D2R_HIP(ctx, hipMemcpyAsync(h_out.data(), out, h_out.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (stats_out) D2R_HIP(ctx, hipMemcpyAsync(h_cnt.data(), cnt, h_cnt.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (vol_out) D2R_HIP(ctx, hipMemcpyAsync(h_vol.data(), vol.get(), h_vol.size() * 2, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = timer.mark(ctx, 3))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(labels_out, h_out.data(), h_out.size());
    if (stats_out)
        for (uint32_t f = 0; f < n; ++f) {
            const uint32_t *s = h_cnt.data() + (size_t)f * per;
            uint32_t *o = stats_out + (size_t)f * 4;
            o[0] = f ? s[0] : (uint32_t)px;
            o[1] = f ? s[1] - s[0] : 0u;
            o[2] = f ? (uint32_t)px - s[1] : 0u;
            o[3] = f ? s[3] : 0u;
        }
    if (vol_out) memcpy(vol_out, h_vol.data(), h_vol.size() * 2);
    for (int a = 0; a < 3; ++a) {
        if (vol_dims_out) vol_dims_out[a] = G.n[a];
        if (vol_lo_out) vol_lo_out[a] = G.lo[a];
    }
    timer.done();
    return D2R_OK;
}

int d2r_labeltrack_get_timing(d2r_ctx *ctx, double *ms_out)
{
    if (!ctx || !ms_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    return ctx->lt_timer.read(ctx, ms_out, 3, "d2r_labeltrack_get_timing: no d2r_labeltrack_scan has completed on this context");
}

}  // extern "C"
