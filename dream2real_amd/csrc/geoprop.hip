// geoprop.hip — mask proposals from frame 0's depth and the support plane (proposer="geometric").  This package's own stand-in, on
// table-top scenes, for the segmentation network the reference takes its proposals from; nothing here stands where reference code
// stands.  The rule is DESIGN.md section 2l, restated in numpy by tests/geoprop_ref.py and held to it by equality of every byte; the
// refusals, the height bins of the bounds, the plane choice and the selection are geoprop_plane.h's, plain host code.  fp64 is one IEEE
// operation at a time in the written order (the library is built with -ffp-contract=off).
//   k_gp_height    one lane per pixel: section 2d's fp64 back-projection, the bounds test, the height bin; the histogram by one integer
//                  add per distinct bin of a wave (wave_each_root, masks_shared.h)
//   k_gp_links     one wave per word of 64 pixels: the above bit, "linked right" and "linked down" as three bit planes
//   k_label_tiles / k_label_seams / k_label_flatten   (masks_shared.h) the labeller over LinkSrc, connectivity 4: a 64 x 16 tile is three
//                  words a row, a pair of neighbours is joined by the link bit of its left or upper pixel
//   k_gp_stats     area and bounding box at the root: integer adds and maxima, one set per distinct root of a wave
//   k_gp_collect   the roots counted; those of area >= min_area appended to the candidate list (its order is the only thing that
//                  depends on the launch, and the host's selection sorts it away)
//   k_gp_number    proposal k + 1 written at its root
//   k_gp_paint     the uint16 label image: a pixel above the plane carries its root's number
// Ordinary vector stores; the atomics are integer adds and maxima; no scratch.
#include <string.h>

#include <algorithm>
#include <vector>

#include "d2r_internal.h"
#include "geoprop_plane.h"
#include "masks_shared.h"

namespace {

constexpr uint32_t GP_OWN = 5;                 // per root: area, max(W - 1 - j), max i, max j, the proposal's number
constexpr uint32_t GP_CNT = 4;                 // counters: above pixels, components, candidates, unused

struct GpCam {
    double fx, fy, cx, cy;
    double lo[3], hi[3], up[3];
    double bin_lo;                             // the first height bin, an integer
    float T[12];                               // cam_pose, rows 0..2
    uint32_t n_bins;
    int W, H;
};

__global__ __launch_bounds__(MK_THREADS) void k_gp_height(GpCam c, const uint16_t *__restrict__ depth, uint32_t *__restrict__ bins,
                                                          uint32_t *__restrict__ hist)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x, px = (uint32_t)c.W * (uint32_t)c.H;
    uint32_t idx = GP_NONE;
    if (g < px) {
        const int i = (int)(g / (uint32_t)c.W), j = (int)(g - (uint32_t)i * (uint32_t)c.W);
        const uint16_t d = depth[g];
        if (d > 0) {
            const double z = (double)((float)d / 1000.0f);
            const double x = ((double)j - c.cx) * z / c.fx, y = ((double)i - c.cy) * z / c.fy;
            const double p0 = (((double)c.T[0] * x + (double)c.T[1] * y) + (double)c.T[2] * z) + (double)c.T[3];
            const double p1 = (((double)c.T[4] * x + (double)c.T[5] * y) + (double)c.T[6] * z) + (double)c.T[7];
            const double p2 = (((double)c.T[8] * x + (double)c.T[9] * y) + (double)c.T[10] * z) + (double)c.T[11];
            if (p0 >= c.lo[0] && p0 <= c.hi[0] && p1 >= c.lo[1] && p1 <= c.hi[1] && p2 >= c.lo[2] && p2 <= c.hi[2]) {
                const double hb = floor(1000.0 * ((c.up[0] * p0 + c.up[1] * p1) + c.up[2] * p2) + 0.5) - c.bin_lo;
                idx = (uint32_t)fmin(fmax(hb, 0.0), (double)(c.n_bins - 1));
            }
        }
        bins[g] = idx;
    }
    wave_each_root(idx != GP_NONE, idx, [&](uint32_t b, unsigned long long members, bool leader) {
        if (leader) atomicAdd(&hist[b], (uint32_t)__popcll(members));
    });
}

__device__ __forceinline__ bool gp_above(uint32_t bin, uint32_t thr) { return bin != GP_NONE && bin >= thr; }

__global__ __launch_bounds__(MK_THREADS) void k_gp_links(const uint16_t *__restrict__ depth, const uint32_t *__restrict__ bins, int W, int H, int WW,
                                                         uint32_t thr, uint32_t tau, unsigned long long *__restrict__ A,
                                                         unsigned long long *__restrict__ R, unsigned long long *__restrict__ D,
                                                         uint32_t *__restrict__ cnt)
{
    WordLane p;
    if (!d2r_word_lane(H, WW, p)) return;
    bool a = false, r = false, dn = false;
    if (p.j < W) {
        const size_t g = (size_t)p.i * W + p.j;
        a = gp_above(bins[g], thr);
        if (a) {
            const uint32_t d = depth[g];
            if (p.j + 1 < W && gp_above(bins[g + 1], thr)) {
                const uint32_t q = depth[g + 1];
                r = (d > q ? d - q : q - d) <= tau;
            }
            if (p.i + 1 < H && gp_above(bins[g + W], thr)) {
                const uint32_t q = depth[g + W];
                dn = (d > q ? d - q : q - d) <= tau;
            }
        }
    }
    const unsigned long long m = word_pack(p, a, A);
    word_pack(p, r, R);
    word_pack(p, dn, D);
    if (p.lane == 0 && m) atomicAdd(&cnt[0], (uint32_t)__popcll(m));
}

// bit planes [H][WW] of one frame: the pixels above the plane, and for each whether it is linked to its right and to its lower
// neighbour.  The labeller's third source: `same`, `left` and `up` say whether a PAIR is linked, and it asks about 4-neighbours alone.
struct LinkSrc {
    static constexpr int CONN = 4;
    const unsigned long long *a, *r, *d;
    int W, H, WW;
    struct Tile {
        unsigned long long a[LB_TH], r[LB_TH], d[LB_TH];
    };
    __device__ void stage(Tile &t, uint32_t, int i0, int j0) const
    {
        const int q = (int)threadIdx.x;
        if (q < LB_TH) {
            const bool in = i0 + q < H;
            const size_t at = (size_t)(i0 + q) * WW + j0 / LB_TW;
            t.a[q] = in ? a[at] : 0ull;
            t.r[q] = in ? r[at] : 0ull;
            t.d[q] = in ? d[at] : 0ull;
        }
    }
    // n is q itself (is the pixel above), its left (q - 1, never across the tile's edge) or its upper neighbour (q - LB_TW)
    __device__ static bool same(const Tile &t, int q, int n)
    {
        const int rq = q / LB_TW, cq = q % LB_TW;
        if (n == q) return (t.a[rq] >> cq) & 1ull;
        if (n == q - 1) return (t.r[rq] >> (cq - 1)) & 1ull;
        return (t.d[rq - 1] >> cq) & 1ull;
    }
    __device__ uint8_t at(uint32_t, int i, int j) const { return plane_bit(a, WW, i, j); }
    __device__ bool left(uint32_t, uint8_t, int i, int j) const { return plane_bit(r, WW, i, j - 1); }
    __device__ bool up(uint32_t, uint8_t, int i, int j) const { return plane_bit(d, WW, i - 1, j); }
};

__device__ inline uint32_t wave_max(uint32_t v)
{
    for (int o = 32; o; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

__global__ __launch_bounds__(MK_THREADS) void k_gp_stats(const unsigned long long *__restrict__ A, int W, int H, int WW,
                                                         const uint32_t *__restrict__ parent, uint32_t *__restrict__ own)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    bool active = false;
    uint32_t root = GP_NONE, i = 0, j = 0;
    if (g < (uint32_t)W * (uint32_t)H) {
        i = g / (uint32_t)W;
        j = g - i * (uint32_t)W;
        active = plane_bit(A, WW, (int)i, (int)j);
        if (active) root = parent[g];
    }
    wave_each_root(active, root, [&](uint32_t r0, unsigned long long members, bool leader) {
        const bool mine = active && root == r0;
        const uint32_t mj0 = wave_max(mine ? (uint32_t)W - 1u - j : 0u), i1 = wave_max(mine ? i : 0u), j1 = wave_max(mine ? j : 0u);
        if (leader) {
            uint32_t *o = own + (size_t)r0 * GP_OWN;
            atomicAdd(&o[0], (uint32_t)__popcll(members));
            atomicMax(&o[1], mj0);
            atomicMax(&o[2], i1);
            atomicMax(&o[3], j1);
        }
    });
}

__global__ __launch_bounds__(MK_THREADS) void k_gp_collect(const unsigned long long *__restrict__ A, int W, int H, int WW,
                                                           const uint32_t *__restrict__ parent, const uint32_t *__restrict__ own, uint32_t min_area,
                                                           uint32_t cap, uint32_t *__restrict__ cand, uint32_t *__restrict__ cnt)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    bool is_root = false;
    if (g < (uint32_t)W * (uint32_t)H) {
        const uint32_t i = g / (uint32_t)W, j = g - i * (uint32_t)W;
        is_root = plane_bit(A, WW, (int)i, (int)j) && parent[g] == g;
    }
    const unsigned long long roots = __ballot(is_root);
    if ((threadIdx.x & 63u) == 0 && roots) atomicAdd(&cnt[1], (uint32_t)__popcll(roots));
    if (!is_root) return;
    const uint32_t *o = own + (size_t)g * GP_OWN;
    if (o[0] < min_area) return;
    const uint32_t slot = atomicAdd(&cnt[2], 1u);
    if (slot >= cap) return;                                   // (cannot happen: at most w h / min_area components are that large)
    uint32_t *c = cand + (size_t)slot * GP_REC_WORDS;
    c[0] = g;
    c[1] = o[0];
    c[2] = g / (uint32_t)W;                                    // the root is its component's first pixel in raster order
    c[3] = (uint32_t)W - 1u - o[1];
    c[4] = o[2];
    c[5] = o[3];
}

__global__ __launch_bounds__(MK_THREADS) void k_gp_number(const uint32_t *__restrict__ kept, uint32_t m, uint32_t *__restrict__ own)
{
    const uint32_t k = blockIdx.x * MK_THREADS + threadIdx.x;
    if (k < m) own[(size_t)kept[k] * GP_OWN + 4] = k + 1u;
}

__global__ __launch_bounds__(MK_THREADS) void k_gp_paint(const unsigned long long *__restrict__ A, int W, int H, int WW,
                                                         const uint32_t *__restrict__ parent, const uint32_t *__restrict__ own, uint16_t *__restrict__ out)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    if (g >= (uint32_t)W * (uint32_t)H) return;
    const uint32_t i = g / (uint32_t)W, j = g - i * (uint32_t)W;
    out[g] = plane_bit(A, WW, (int)i, (int)j) ? (uint16_t)own[(size_t)parent[g] * GP_OWN + 4] : (uint16_t)0;
}

}  // namespace

extern "C" {

int d2r_geoprop_masks(d2r_ctx *ctx, const double *bounds, const double *up, const d2r_geoprop_params *params, uint32_t w, uint32_t h,
                      const double *K, const uint16_t *d16, const float *cam_pose, uint16_t *labels_out, uint32_t *recs_out, uint32_t *n_out,
                      int32_t *plane_out)
{
    if (!ctx) return d2r_fail(nullptr, D2R_ERR_INVALID, "null argument");
    GpBins B;
    int rc;
    if ((rc = gp_check(ctx, bounds, up, params, w, h, K, d16, cam_pose, labels_out, recs_out, n_out, plane_out, &B))) return rc;
    D2R_HIP(ctx, hipSetDevice(ctx->device));

    const size_t px = (size_t)w * h, ww = (w + 63) / 64, words = (size_t)h * ww;
    const uint32_t cap = (uint32_t)(px / std::max(1u, params->min_area)) + 1u;
    GpCam c{};
    c.fx = K[0]; c.fy = K[1]; c.cx = K[2]; c.cy = K[3];
    for (int a = 0; a < 3; ++a) {
        c.lo[a] = bounds[a];
        c.hi[a] = bounds[3 + a];
        c.up[a] = up[a];
    }
    c.bin_lo = (double)B.lo;
    for (int k = 0; k < 12; ++k) c.T[k] = cam_pose[k];
    c.n_bins = B.n;
    c.W = (int)w;
    c.H = (int)h;

    D2rStage in(ctx, ctx->gp_in), ws(ctx, ctx->gp_ws);
    const size_t o_depth = in.add(px * 2);
    // the first two segments are cleared together: counters, histogram
    const size_t o_cnt = ws.add(GP_CNT * 4), o_hist = ws.add((size_t)B.n * 4);
    const size_t clear_end = ws.total();
    const size_t o_bins = ws.add(px * 4), o_a = ws.add(words * 8), o_r = ws.add(words * 8), o_d = ws.add(words * 8), o_parent = ws.add(px * 4),
                 o_own = ws.add(px * GP_OWN * 4), o_cand = ws.add((size_t)cap * GP_REC_WORDS * 4), o_kept = ws.add((size_t)params->max_props * 4),
                 o_out = ws.add(px * 2);
    if ((rc = in.reserve()) || (rc = ws.reserve())) return rc;
    D2rStageTimer &timer = ctx->gp_timer, &timer2 = ctx->gp_timer2;
    if ((rc = timer.mark(ctx, 0)) || (rc = in.upload(o_depth, d16, px * 2)) || (rc = timer.mark(ctx, 1))) return rc;

    const int W = (int)w, H = (int)h, WW = (int)ww;
    const uint16_t *depth = in.at<uint16_t>(o_depth);
    uint32_t *d_cnt = ws.at<uint32_t>(o_cnt), *d_hist = ws.at<uint32_t>(o_hist), *d_bins = ws.at<uint32_t>(o_bins), *d_parent = ws.at<uint32_t>(o_parent);
    uint32_t *d_own = ws.at<uint32_t>(o_own), *d_cand = ws.at<uint32_t>(o_cand), *d_kept = ws.at<uint32_t>(o_kept);
    unsigned long long *d_a = ws.at<unsigned long long>(o_a), *d_r = ws.at<unsigned long long>(o_r), *d_d = ws.at<unsigned long long>(o_d);
    uint16_t *d_out = ws.at<uint16_t>(o_out);
    const dim3 T(MK_THREADS);
    const uint32_t gw = (uint32_t)((words + 3) / 4), gpx = (uint32_t)((px + MK_THREADS - 1) / MK_THREADS);

    D2R_HIP(ctx, hipMemsetAsync(ws.at<char>(o_cnt), 0, clear_end - o_cnt, ctx->stream));
    hipLaunchKernelGGL(k_gp_height, dim3(gpx), T, 0, ctx->stream, c, depth, d_bins, d_hist);
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = timer.mark(ctx, 2))) return rc;
    std::vector<uint32_t> hist(B.n);
    D2R_HIP(ctx, hipMemcpyAsync(hist.data(), d_hist, (size_t)B.n * 4, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const GpPlane plane = gp_plane(hist.data(), B, params->window_mm);

    const LinkSrc src{d_a, d_r, d_d, W, H, WW};
    hipLaunchKernelGGL(k_gp_links, dim3(gw), T, 0, ctx->stream, depth, (const uint32_t *)d_bins, W, H, WW, gp_threshold(plane, B, params->h_min_mm),
                       params->tau_mm, d_a, d_r, d_d, d_cnt);
    label_components(ctx, src, 1, d_parent, d_own, GP_OWN * 4);
    hipLaunchKernelGGL(k_gp_stats, dim3(gpx), T, 0, ctx->stream, (const unsigned long long *)d_a, W, H, WW, (const uint32_t *)d_parent, d_own);
    hipLaunchKernelGGL(k_gp_collect, dim3(gpx), T, 0, ctx->stream, (const unsigned long long *)d_a, W, H, WW, (const uint32_t *)d_parent,
                       (const uint32_t *)d_own, params->min_area, cap, d_cand, d_cnt);
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = timer.mark(ctx, 3)) || (rc = timer2.mark(ctx, 0))) return rc;
    uint32_t cnt[GP_CNT] = {0, 0, 0, 0};
    D2R_HIP(ctx, hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint32_t> cand((size_t)std::min(cnt[2], cap) * GP_REC_WORDS);
    if (!cand.empty()) {
        D2R_HIP(ctx, hipMemcpyAsync(cand.data(), d_cand, cand.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    gp_select(cand, params->max_props);
    const uint32_t m = (uint32_t)(cand.size() / GP_REC_WORDS);
    std::vector<uint32_t> kept(m);
    for (uint32_t k = 0; k < m; ++k) kept[k] = cand[(size_t)k * GP_REC_WORDS];
    if (m) {
        if ((rc = ws.upload(o_kept, kept.data(), (size_t)m * 4))) return rc;
        hipLaunchKernelGGL(k_gp_number, dim3((m + MK_THREADS - 1) / MK_THREADS), T, 0, ctx->stream, (const uint32_t *)d_kept, m, d_own);
    }
    hipLaunchKernelGGL(k_gp_paint, dim3(gpx), T, 0, ctx->stream, (const unsigned long long *)d_a, W, H, WW, (const uint32_t *)d_parent,
                       (const uint32_t *)d_own, d_out);
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = timer2.mark(ctx, 1))) return rc;

    // the image comes back aside and reaches the caller once the whole call has succeeded
    std::vector<uint16_t> h_out(px);
    D2R_HIP(ctx, hipMemcpyAsync(h_out.data(), d_out, px * 2, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = timer2.mark(ctx, 2))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(labels_out, h_out.data(), px * 2);
    memset(recs_out, 0, (size_t)params->max_props * GP_REC_WORDS * 4);
    if (m) memcpy(recs_out, cand.data(), cand.size() * 4);
    *n_out = m;
    plane_out[0] = plane.bin;
    plane_out[1] = (int32_t)plane.count;
    plane_out[2] = (int32_t)plane.inside;
    plane_out[3] = (int32_t)cnt[0];
    plane_out[4] = (int32_t)cnt[1];
    timer.done();
    timer2.done();
    return D2R_OK;
}

int d2r_geoprop_get_timing(d2r_ctx *ctx, double *ms_out)
{
    if (!ctx || !ms_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    const char *untimed = "d2r_geoprop_get_timing: no d2r_geoprop_masks has completed on this context";
    if (int rc = ctx->gp_timer.read(ctx, ms_out, 3, untimed)) return rc;
    return ctx->gp_timer2.read(ctx, ms_out + 3, 2, untimed);
}

}  // extern "C"
