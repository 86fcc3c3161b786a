// pcdbuild.hip — the visual clouds of the point-cloud ablation built on the device (reference vision_3d/pcd_visual_model.py:18-95,
// once per (object, view) on the CPU through cv2.erode and Open3D).  The rule is DESIGN.md section 2b, bullet "Clouds", restated in
// numpy by pcd_visual_model.erode_rect / backproject / crop / voxel_down_sample and held to them bit for bit.  One call, all views,
// all requested labels; a segment is one (object, view) pair, numbered object-major.
//   k_pb_erode_rows / _cols  separable 15 x 15 erosion of the label image: window min label == window max label
//   k_pb_points<false>       per (segment, 256 pixels): survivors with depth inside the crop, counted (fp64 back-projection)
//   k_pb_points<true>        the same points again, written in (segment, pixel) order at the scanned offsets (d2r_block_scan)
//   k_pb_scan_*              exclusive scan of a long uint32 row: chunks of 4096 by d2r_block_scan_row, their totals, the add-back
//   k_pb_seg_bounds          per segment: min and max -> the voxel origin, and the largest voxel index (the key's width)
//   k_pb_keys                key = (segment, ix, iy, iz) packed to the width the call needs, value = point index
//   k_pb_hist / k_pb_scatter stable least-significant-digit radix sort, 8 bits a pass, tiles of 256: ranks inside a tile come from
//                            wave ballots, so equal keys keep their pixel order
//   k_pb_runs / k_pb_voxels  one lane per run of equal keys: fp64 sums from 0.0 in sorted (= pixel) order, mean, colour rounded half up
// Integer atomics only (LDS histogram, the largest index).  Every value is written by ordinary vector stores from C++.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "d2r_internal.h"

namespace {

constexpr uint32_t PB_THREADS = D2R_SCAN_THREADS;
constexpr uint32_t PB_SCAN_CHUNK = 4096;      // entries one workgroup scans
constexpr int PB_R = 7;                       // erosion: 15 x 15 window, rows i - 7 .. i + 7
constexpr uint32_t PB_AXIS_BITS = 21;

struct PbArgs {
    const uint8_t *rgb;          // [n][px][3]
    const uint16_t *depth;       // [n][px]
    const uint8_t *labels;       // [n][px]
    const uint8_t *keep;         // [n_views][px] 1 where the pixel survives the erosion of its own label
    const double *poses;         // [n][16]
    const uint32_t *views;       // [n_views] frame index
    const uint8_t *obj_ids;      // [n_objs]
    double fx, fy, cx, cy, lo[3], hi[3];
    uint32_t W, px, bpf, n_views;      // bpf: workgroups per frame
};

struct PbOut {
    float4 *xyz;
    uint32_t *rgb;
};

__global__ __launch_bounds__(PB_THREADS) void k_pb_erode_rows(const uint8_t *__restrict__ labels, const uint32_t *__restrict__ views, int W, uint32_t px,
                                                              uint16_t *__restrict__ rowmm)
{
    const uint32_t g = blockIdx.x * PB_THREADS + threadIdx.x;
    if (g >= px) return;
    const uint8_t *L = labels + (size_t)views[blockIdx.y] * px;
    const int i = (int)(g / (uint32_t)W), j = (int)(g - (uint32_t)i * (uint32_t)W);
    uint32_t mn = 255u, mx = 0u;
    for (int b = -PB_R; b <= PB_R; ++b) {
        const int jj = j + b;
        if (jj < 0 || jj >= W) continue;              // outside the frame counts as matching
        const uint32_t l = L[(size_t)i * W + jj];
        mn = min(mn, l);
        mx = max(mx, l);
    }
    rowmm[(size_t)blockIdx.y * px + g] = (uint16_t)(mn | mx << 8);
}

__global__ __launch_bounds__(PB_THREADS) void k_pb_erode_cols(const uint16_t *__restrict__ rowmm, int W, int H, uint32_t px, uint8_t *__restrict__ keep)
{
    const uint32_t g = blockIdx.x * PB_THREADS + threadIdx.x;
    if (g >= px) return;
    const uint16_t *R = rowmm + (size_t)blockIdx.y * px;
    const int i = (int)(g / (uint32_t)W), j = (int)(g - (uint32_t)i * (uint32_t)W);
    uint32_t mn = 255u, mx = 0u;
    for (int a = -PB_R; a <= PB_R; ++a) {
        const int ii = i + a;
        if (ii < 0 || ii >= H) continue;
        const uint32_t v = R[(size_t)ii * W + j];
        mn = min(mn, v & 255u);
        mx = max(mx, v >> 8);
    }
    keep[(size_t)blockIdx.y * px + g] = mn == mx ? 1 : 0;      // the window holds one label: the pixel's own
}

// pixel g of segment s: does it give a point of the segment's cloud, and which (fp64, DESIGN.md 2b: products and sums in this order)
__device__ __forceinline__ bool pb_point(const PbArgs &A, uint32_t s, uint32_t g, double &px_, double &py_, double &pz_, size_t &at)
{
    const uint32_t o = s / A.n_views, v = s - o * A.n_views, f = A.views[v];
    if (!A.keep[(size_t)v * A.px + g]) return false;
    at = (size_t)f * A.px + g;
    if (A.labels[at] != A.obj_ids[o]) return false;
    const uint16_t d = A.depth[at];
    if (!d) return false;
    const uint32_t i = g / A.W, j = g - i * A.W;
    const double *T = A.poses + (size_t)f * 16;
    const double z = (double)((float)d / 1000.0f);
    const double x = (((double)j - A.cx) * z) / A.fx, y = (((double)i - A.cy) * z) / A.fy;
    px_ = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    py_ = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    pz_ = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    return px_ >= A.lo[0] && px_ <= A.hi[0] && py_ >= A.lo[1] && py_ <= A.hi[1] && pz_ >= A.lo[2] && pz_ <= A.hi[2];
}

// workgroup blockIdx.x = s * bpf + b covers pixels b * 256 .. of segment s.  EMIT false: counts[blockIdx.x] = its points; true: counts
// holds the scanned offsets and the points are written behind them, in pixel order
template <bool EMIT>
__global__ __launch_bounds__(PB_THREADS) void k_pb_points(PbArgs A, uint32_t *__restrict__ counts, double *__restrict__ pts, uint32_t *__restrict__ col,
                                                          uint32_t *__restrict__ seg)
{
    const uint32_t s = blockIdx.x / A.bpf, g = (blockIdx.x - s * A.bpf) * PB_THREADS + threadIdx.x;
    double x = 0.0, y = 0.0, z = 0.0;
    size_t at = 0;
    const bool k = g < A.px && pb_point(A, s, g, x, y, z, at);
    if (!EMIT) {
        const uint32_t c = d2r_block_sum<uint32_t>(k ? 1u : 0u);
        if (threadIdx.x == 0) counts[blockIdx.x] = c;
    } else {
        const uint32_t off = d2r_block_scan<uint32_t>(k ? 1u : 0u, counts[blockIdx.x]);
        if (k) {
            pts[(size_t)off * 3] = x;
            pts[(size_t)off * 3 + 1] = y;
            pts[(size_t)off * 3 + 2] = z;
            col[off] = (uint32_t)A.rgb[at * 3] | (uint32_t)A.rgb[at * 3 + 1] << 8 | (uint32_t)A.rgb[at * 3 + 2] << 16;
            seg[off] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------ a long row's exclusive scan

__global__ __launch_bounds__(PB_THREADS) void k_pb_scan_chunks(uint32_t *__restrict__ data, uint32_t n, uint32_t *__restrict__ tops)
{
    const uint32_t lo = blockIdx.x * PB_SCAN_CHUNK;
    const uint32_t tot = d2r_block_scan_row<uint32_t>(data + lo, data + lo, min(PB_SCAN_CHUNK, n - lo));
    if (threadIdx.x == 0) tops[blockIdx.x] = tot;
}

__global__ __launch_bounds__(PB_THREADS) void k_pb_scan_tops(uint32_t *__restrict__ tops, uint32_t nchunks, uint32_t *__restrict__ total)
{
    const uint32_t tot = d2r_block_scan_row<uint32_t>(tops, tops, nchunks);
    if (threadIdx.x == 0) *total = tot;
}

__global__ __launch_bounds__(PB_THREADS) void k_pb_scan_add(uint32_t *__restrict__ data, uint32_t n, const uint32_t *__restrict__ tops)
{
    const uint32_t i = blockIdx.x * PB_THREADS + threadIdx.x;
    if (i < n) data[i] += tops[i / PB_SCAN_CHUNK];
}

// out[s] = offsets[s * stride] for s < count, out[count] = *total
__global__ __launch_bounds__(PB_THREADS) void k_pb_gather(const uint32_t *__restrict__ offsets, uint32_t stride, uint32_t count, const uint32_t *__restrict__ total,
                                                          uint32_t *__restrict__ out)
{
    const uint32_t s = blockIdx.x * PB_THREADS + threadIdx.x;
    if (s < count) out[s] = offsets[(size_t)s * stride];
    else if (s == count) out[s] = *total;
}

// ------------------------------------------------------------------------------------------------ clouds without voxels

__global__ __launch_bounds__(PB_THREADS) void k_pb_write_raw(const double *__restrict__ pts, const uint32_t *__restrict__ col, const uint32_t *__restrict__ seg,
                                                             const uint32_t *__restrict__ segstart, uint32_t M, uint32_t n_views, const PbOut *__restrict__ outs)
{
    const uint32_t i = blockIdx.x * PB_THREADS + threadIdx.x;
    if (i >= M) return;
    const uint32_t o = seg[i] / n_views, local = i - segstart[o * n_views];
    const PbOut out = outs[o];
    out.xyz[local] = make_float4((float)pts[(size_t)i * 3], (float)pts[(size_t)i * 3 + 1], (float)pts[(size_t)i * 3 + 2], 0.f);
    out.rgb[local] = col[i];
}

// ------------------------------------------------------------------------------------------------ voxel keys

__device__ __forceinline__ double pb_block_minmax(double v, bool want_max, double *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t s = PB_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const double a = red[threadIdx.x], b = red[threadIdx.x + s];
            red[threadIdx.x] = want_max ? (a > b ? a : b) : (a < b ? a : b);
        }
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// one workgroup per segment: origin = min - voxel / 2 per axis; the largest index of any segment per axis -> maxidx (zeroed before)
__global__ __launch_bounds__(PB_THREADS) void k_pb_seg_bounds(const double *__restrict__ pts, const uint32_t *__restrict__ segstart, double voxel,
                                                              double *__restrict__ origin, uint32_t *__restrict__ maxidx)
{
    __shared__ double red[PB_THREADS];
    const uint32_t s = blockIdx.x, lo = segstart[s], hi = segstart[s + 1];
    if (lo == hi) return;
    for (int a = 0; a < 3; ++a) {
        double mn = INFINITY, mx = -INFINITY;
        for (uint32_t i = lo + threadIdx.x; i < hi; i += PB_THREADS) {
            const double v = pts[(size_t)i * 3 + a];
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        mn = pb_block_minmax(mn, false, red);
        mx = pb_block_minmax(mx, true, red);
        if (threadIdx.x == 0) {
            const double o = mn - voxel * 0.5;
            origin[(size_t)s * 3 + a] = o;
            atomicMax(&maxidx[a], (uint32_t)floor((mx - o) / voxel));
        }
    }
}

__global__ __launch_bounds__(PB_THREADS) void k_pb_keys(const double *__restrict__ pts, const uint32_t *__restrict__ seg, const double *__restrict__ origin,
                                                        double voxel, uint32_t M, uint32_t by, uint32_t bz, uint32_t segshift,
                                                        unsigned long long *__restrict__ keys, uint32_t *__restrict__ idx)
{
    const uint32_t i = blockIdx.x * PB_THREADS + threadIdx.x;
    if (i >= M) return;
    const uint32_t s = seg[i];
    // every index is below 2^21 (the bounds were checked against it): through uint32, whose conversion is one instruction
    const unsigned long long ix = (uint32_t)floor((pts[(size_t)i * 3] - origin[(size_t)s * 3]) / voxel);
    const unsigned long long iy = (uint32_t)floor((pts[(size_t)i * 3 + 1] - origin[(size_t)s * 3 + 1]) / voxel);
    const unsigned long long iz = (uint32_t)floor((pts[(size_t)i * 3 + 2] - origin[(size_t)s * 3 + 2]) / voxel);
    unsigned long long k = (ix << (by + bz)) | (iy << bz) | iz;
    if (segshift < 64) k |= (unsigned long long)s << segshift;      // one segment and 63 index bits: nothing above them
    keys[i] = k;
    idx[i] = i;
}

// ------------------------------------------------------------------------------------------------ the sort

// hist[digit][tile]: how many keys of tile `blockIdx.x` (256 consecutive entries) carry the digit
__global__ __launch_bounds__(PB_THREADS) void k_pb_hist(const unsigned long long *__restrict__ keys, uint32_t M, uint32_t shift, uint32_t ntiles,
                                                        uint32_t *__restrict__ hist)
{
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * PB_THREADS + threadIdx.x;
    if (i < M) atomicAdd(&cnt[(uint32_t)(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}

// entry i goes to (scanned hist[digit][tile]) + the entries of the tile before it with its digit: waves in order, lanes in order
__global__ __launch_bounds__(PB_THREADS) void k_pb_scatter(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ idx, uint32_t M, uint32_t shift,
                                                           uint32_t ntiles, const uint32_t *__restrict__ hist, unsigned long long *__restrict__ keys_out,
                                                           uint32_t *__restrict__ idx_out)
{
    __shared__ uint32_t wcnt[PB_THREADS / 64][256];
    for (uint32_t q = threadIdx.x; q < (PB_THREADS / 64) * 256; q += PB_THREADS) (&wcnt[0][0])[q] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * PB_THREADS + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool valid = i < M;
    const unsigned long long key = valid ? keys[i] : 0ull;
    const uint32_t d = (uint32_t)(key >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long m = __ballot(valid && bit);
        peers &= bit ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wcnt[wave][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (!valid) return;
    uint32_t at = hist[(size_t)d * ntiles + blockIdx.x] + rank;
    for (uint32_t w = 0; w < wave; ++w) at += wcnt[w][d];
    keys_out[at] = key;
    idx_out[at] = idx[i];
}

// ------------------------------------------------------------------------------------------------ runs of equal keys

__global__ __launch_bounds__(PB_THREADS) void k_pb_heads(const unsigned long long *__restrict__ keys, uint32_t M, uint32_t *__restrict__ flags)
{
    const uint32_t i = blockIdx.x * PB_THREADS + threadIdx.x;
    if (i < M) flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// runstart[r] = first entry of run r (runid = the scanned head flags)
__global__ __launch_bounds__(PB_THREADS) void k_pb_runs(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ runid, uint32_t M,
                                                        uint32_t *__restrict__ runstart)
{
    const uint32_t i = blockIdx.x * PB_THREADS + threadIdx.x;
    if (i < M && (i == 0 || keys[i] != keys[i - 1])) runstart[runid[i]] = i;
}

// objrun[o] = the first run of object o's segments (the run count where none follows), objrun[n_objs] = the run count
__global__ __launch_bounds__(PB_THREADS) void k_pb_obj_runs(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ runid, uint32_t M,
                                                            const uint32_t *__restrict__ nruns, uint32_t segshift, uint32_t n_views, uint32_t n_objs,
                                                            uint32_t *__restrict__ objrun)
{
    const uint32_t o = blockIdx.x * PB_THREADS + threadIdx.x;
    if (o > n_objs) return;
    const unsigned long long first = (unsigned long long)o * n_views;
    uint32_t lo = 0, hi = M;                              // first entry whose segment is >= first
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const unsigned long long s = segshift < 64 ? keys[mid] >> segshift : 0ull;
        if (s < first) lo = mid + 1;
        else hi = mid;
    }
    objrun[o] = lo < M ? runid[lo] : *nruns;
}

// one lane per voxel: its points added one after another in sorted order, which within a key is pixel order (np.bincount's order)
__global__ __launch_bounds__(PB_THREADS) void k_pb_voxels(const double *__restrict__ pts, const uint32_t *__restrict__ col, const unsigned long long *__restrict__ keys,
                                                          const uint32_t *__restrict__ idx, const uint32_t *__restrict__ runstart, uint32_t R, uint32_t M,
                                                          uint32_t segshift, uint32_t n_views, const uint32_t *__restrict__ objrun,
                                                          const PbOut *__restrict__ outs)
{
    const uint32_t r = blockIdx.x * PB_THREADS + threadIdx.x;
    if (r >= R) return;
    const uint32_t lo = runstart[r], hi = r + 1 < R ? runstart[r + 1] : M;
    double sx = 0.0, sy = 0.0, sz = 0.0, sr = 0.0, sg = 0.0, sb = 0.0;
    for (uint32_t t = lo; t < hi; ++t) {
        const uint32_t p = idx[t], c = col[p];
        sx += pts[(size_t)p * 3];
        sy += pts[(size_t)p * 3 + 1];
        sz += pts[(size_t)p * 3 + 2];
        sr += (double)(c & 255u);
        sg += (double)((c >> 8) & 255u);
        sb += (double)((c >> 16) & 255u);
    }
    const double n = (double)(hi - lo);
    const uint32_t o = (uint32_t)((segshift < 64 ? keys[lo] >> segshift : 0ull) / n_views);
    const PbOut out = outs[o];
    const uint32_t local = r - objrun[o];
    out.xyz[local] = make_float4((float)(sx / n), (float)(sy / n), (float)(sz / n), 0.f);
    out.rgb[local] = (uint32_t)floor(sr / n + 0.5) | (uint32_t)floor(sg / n + 0.5) << 8 | (uint32_t)floor(sb / n + 0.5) << 16;
}

// ------------------------------------------------------------------------------------------------ host side

uint32_t pb_blocks(size_t n) { return (uint32_t)((n + PB_THREADS - 1) / PB_THREADS); }

uint32_t pb_bit_length(uint64_t v)
{
    uint32_t b = 0;
    while (v) {
        ++b;
        v >>= 1;
    }
    return b;
}

// data[0 .. n) -> its exclusive scan in place, the total in *total (device); tops holds ceil(n / 4096) entries
void pb_scan(d2r_ctx *ctx, uint32_t *data, uint32_t n, uint32_t *tops, uint32_t *total)
{
    const uint32_t nchunks = (n + PB_SCAN_CHUNK - 1) / PB_SCAN_CHUNK;
    hipLaunchKernelGGL(k_pb_scan_chunks, dim3(nchunks), dim3(PB_THREADS), 0, ctx->stream, data, n, tops);
    hipLaunchKernelGGL(k_pb_scan_tops, dim3(1), dim3(PB_THREADS), 0, ctx->stream, tops, nchunks, total);
    hipLaunchKernelGGL(k_pb_scan_add, dim3(pb_blocks(n)), dim3(PB_THREADS), 0, ctx->stream, data, n, (const uint32_t *)tops);
}

// everything d2r_pcd_build refuses before it touches the device
int pb_check(const uint8_t *rgb, const uint16_t *depth_u16, const uint8_t *labels, uint32_t n, uint32_t w, uint32_t h, const double *cam_poses,
             const double *K, const double *bounds, double voxel, const uint32_t *views, uint32_t n_views, const uint8_t *obj_ids, uint32_t n_objs)
{
    d2r_ctx *none = nullptr;
    if (!rgb || !depth_u16 || !labels || !cam_poses || !K || !bounds || !views || !obj_ids) return d2r_fail(none, D2R_ERR_INVALID, "pcd build: null argument");
    if (n == 0 || w == 0 || h == 0) return d2r_fail(none, D2R_ERR_INVALID, "pcd build: n, width and height must be at least 1");
    if (n_views == 0 || n_objs == 0) return d2r_fail(none, D2R_ERR_INVALID, "pcd build: at least one view and one object");
    for (uint32_t v = 0; v < n_views; ++v)
        if (views[v] >= n)
            return d2r_fail(none, D2R_ERR_INVALID, "pcd build: view index " + std::to_string(views[v]) + " with " + std::to_string(n) + " frames");
    bool seen[256] = {};
    for (uint32_t o = 0; o < n_objs; ++o) {
        if (seen[obj_ids[o]]) return d2r_fail(none, D2R_ERR_INVALID, "pcd build: object id " + std::to_string(obj_ids[o]) + " listed twice");
        seen[obj_ids[o]] = true;
    }
    if (!(voxel >= 0.0) || !std::isfinite(voxel)) return d2r_fail(none, D2R_ERR_INVALID, "pcd build: voxel must be finite and >= 0");
    if (int rc = d2r_check_cam(none, "pcd build", K, cam_poses, n)) return rc;
    for (int i = 0; i < 6; ++i)
        if (std::isnan(bounds[i])) return d2r_fail(none, D2R_ERR_INVALID, "pcd build: bounds must not be NaN");
    if (voxel > 0.0)
        for (int a = 0; a < 3; ++a)       // the cropped points lie inside the bounds: their extent is at most the bounds'
            if (!((bounds[3 + a] - bounds[a]) / voxel + 2.0 < (double)(1u << PB_AXIS_BITS)))
                return d2r_fail(none, D2R_ERR_INVALID, "pcd build: bounds / voxel needs more than 21 bits of voxel index on axis " + std::to_string(a));
    const uint64_t px = (uint64_t)w * h;
    if (px >= (1ull << 31) || px * n_views >= (1ull << 31)) return d2r_fail(none, D2R_ERR_UNSUPPORTED, "pcd build: views x pixels must stay below 2^31");
    if (n_views > 65535) return d2r_fail(none, D2R_ERR_UNSUPPORTED, "pcd build: at most 65535 views per call");
    if ((uint64_t)n_views * n_objs * ((px + PB_THREADS - 1) / PB_THREADS) >= (1ull << 31))
        return d2r_fail(none, D2R_ERR_UNSUPPORTED, "pcd build: objects x views x pixels / 256 must stay below 2^31");
    if ((uint64_t)n * px >= (1ull << 40)) return d2r_fail(none, D2R_ERR_UNSUPPORTED, "pcd build: the batch must have fewer than 2^40 pixels");
    return D2R_OK;
}

}  // namespace

extern "C" {

int d2r_pcd_build(d2r_ctx *ctx, const uint8_t *rgb, const uint16_t *depth_u16, const uint8_t *labels, uint32_t n, uint32_t w, uint32_t h,
                  const double *cam_poses, const double *K, const double *bounds, double voxel, const uint32_t *views, uint32_t n_views,
                  const uint8_t *obj_ids, uint32_t n_objs, d2r_pcd **out)
{
    if (!out) return d2r_fail(ctx, D2R_ERR_INVALID, "pcd build: null argument");
    for (uint32_t o = 0; o < n_objs; ++o) out[o] = nullptr;
    int rc = pb_check(rgb, depth_u16, labels, n, w, h, cam_poses, K, bounds, voxel, views, n_views, obj_ids, n_objs);
    if (rc) return d2r_fail(ctx, rc, d2r_last_error(nullptr));      // the message into the context too
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t px = w * h, bpf = pb_blocks(px), S = n_objs * n_views, nblk = S * bpf;
    const size_t tot = (size_t)n * px;

    D2rDev<uint8_t> d_rgb, d_labels, d_keep, d_ids;
    D2rDev<uint16_t> d_depth, d_rowmm;
    D2rDev<double> d_poses, d_pts, d_origin;
    D2rDev<uint32_t> d_views, d_counts, d_tops, d_small, d_segstart, d_col, d_seg, d_idx[2], d_hist, d_runid, d_runstart, d_objrun;
    D2rDev<unsigned long long> d_keys[2];
    D2rDev<PbOut> d_outs;
    std::vector<std::unique_ptr<d2r_pcd>> clouds;
    D2rDrain drain{ctx->stream};

    if ((rc = d_rgb.alloc(ctx, tot * 3, "pcd build frames")) || (rc = d_depth.alloc(ctx, tot * 2, "pcd build frames")) ||
        (rc = d_labels.alloc(ctx, tot, "pcd build frames")) || (rc = d_poses.alloc(ctx, (size_t)n * 128, "pcd build poses")) ||
        (rc = d_views.alloc(ctx, (size_t)n_views * 4, "pcd build views")) || (rc = d_ids.alloc(ctx, n_objs, "pcd build object ids")) ||
        (rc = d_rowmm.alloc(ctx, (size_t)n_views * px * 2, "pcd build erosion")) || (rc = d_keep.alloc(ctx, (size_t)n_views * px, "pcd build erosion")) ||
        (rc = d_counts.alloc(ctx, (size_t)nblk * 4, "pcd build counts")) ||
        (rc = d_tops.alloc(ctx, ((size_t)n_views * px / PB_SCAN_CHUNK + (size_t)nblk / PB_SCAN_CHUNK + 512) * 4, "pcd build scan totals")) ||
        (rc = d_small.alloc(ctx, 64, "pcd build counters")) || (rc = d_segstart.alloc(ctx, ((size_t)S + 1) * 4, "pcd build segments")))
        return rc;
    uint32_t *total = d_small.get(), *maxidx = d_small.get() + 1, *nruns = d_small.get() + 4;

    if ((rc = ctx->pcdb_timer.mark(ctx, 0))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(d_rgb.get(), rgb, tot * 3, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(d_depth.get(), depth_u16, tot * 2, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(d_labels.get(), labels, tot, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(d_poses.get(), cam_poses, (size_t)n * 128, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(d_views.get(), views, (size_t)n_views * 4, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(d_ids.get(), obj_ids, n_objs, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemsetAsync(d_small.get(), 0, 64, ctx->stream));
    if ((rc = ctx->pcdb_timer.mark(ctx, 1))) return rc;

    // erosion, then the points of every segment counted
    hipLaunchKernelGGL(k_pb_erode_rows, dim3(bpf, n_views), dim3(PB_THREADS), 0, ctx->stream, (const uint8_t *)d_labels.get(), (const uint32_t *)d_views.get(),
                       (int)w, px, d_rowmm.get());
    hipLaunchKernelGGL(k_pb_erode_cols, dim3(bpf, n_views), dim3(PB_THREADS), 0, ctx->stream, (const uint16_t *)d_rowmm.get(), (int)w, (int)h, px, d_keep.get());
    PbArgs A{d_rgb.get(), d_depth.get(), d_labels.get(), d_keep.get(), d_poses.get(), d_views.get(), d_ids.get(), K[0], K[4], K[2], K[5],
             {bounds[0], bounds[1], bounds[2]}, {bounds[3], bounds[4], bounds[5]}, w, px, bpf, n_views};
    hipLaunchKernelGGL(k_pb_points<false>, dim3(nblk), dim3(PB_THREADS), 0, ctx->stream, A, d_counts.get(), (double *)nullptr, (uint32_t *)nullptr,
                       (uint32_t *)nullptr);
    pb_scan(ctx, d_counts.get(), nblk, d_tops.get(), total);
    hipLaunchKernelGGL(k_pb_gather, dim3(pb_blocks((size_t)S + 1)), dim3(PB_THREADS), 0, ctx->stream, (const uint32_t *)d_counts.get(), bpf, S,
                       (const uint32_t *)total, d_segstart.get());
    D2R_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> segstart((size_t)S + 1);
    D2R_HIP(ctx, hipMemcpyAsync(segstart.data(), d_segstart.get(), segstart.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));       // counts: they size everything below
    const uint32_t M = segstart[S];

    std::vector<uint32_t> sizes(n_objs, 0u);
    std::vector<uint32_t> objrun((size_t)n_objs + 1, 0u);
    uint32_t R = 0, segshift = 0;
    const unsigned long long *sorted_keys = nullptr;
    const uint32_t *sorted_idx = nullptr;
    if (M) {
        if ((rc = d_pts.alloc(ctx, (size_t)M * 24, "pcd build points")) || (rc = d_col.alloc(ctx, (size_t)M * 4, "pcd build points")) ||
            (rc = d_seg.alloc(ctx, (size_t)M * 4, "pcd build points")))
            return rc;
        hipLaunchKernelGGL(k_pb_points<true>, dim3(nblk), dim3(PB_THREADS), 0, ctx->stream, A, d_counts.get(), d_pts.get(), d_col.get(), d_seg.get());
    }
    if (M && voxel == 0.0) {
        for (uint32_t o = 0; o < n_objs; ++o) sizes[o] = segstart[(size_t)(o + 1) * n_views] - segstart[(size_t)o * n_views];
    } else if (M) {
        const uint32_t ntiles = pb_blocks(M), nhist = ntiles * 256u;
        if ((rc = d_origin.alloc(ctx, (size_t)S * 24, "pcd build voxel origins")) || (rc = d_keys[0].alloc(ctx, (size_t)M * 8, "pcd build sort keys")) ||
            (rc = d_keys[1].alloc(ctx, (size_t)M * 8, "pcd build sort keys")) || (rc = d_idx[0].alloc(ctx, (size_t)M * 4, "pcd build sort values")) ||
            (rc = d_idx[1].alloc(ctx, (size_t)M * 4, "pcd build sort values")) || (rc = d_hist.alloc(ctx, (size_t)nhist * 4, "pcd build sort histogram")) ||
            (rc = d_runid.alloc(ctx, (size_t)M * 4, "pcd build runs")) || (rc = d_runstart.alloc(ctx, (size_t)M * 4, "pcd build runs")) ||
            (rc = d_objrun.alloc(ctx, ((size_t)n_objs + 1) * 4, "pcd build runs")))
            return rc;
        hipLaunchKernelGGL(k_pb_seg_bounds, dim3(S), dim3(PB_THREADS), 0, ctx->stream, (const double *)d_pts.get(), (const uint32_t *)d_segstart.get(), voxel,
                           d_origin.get(), maxidx);
        D2R_HIP(ctx, hipGetLastError());
        uint32_t mi[3];
        D2R_HIP(ctx, hipMemcpyAsync(mi, maxidx, 12, hipMemcpyDeviceToHost, ctx->stream));
        D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the largest voxel index: the key's width, so the sort's digit passes
        const uint32_t bx = pb_bit_length(mi[0]), by = pb_bit_length(mi[1]), bz = pb_bit_length(mi[2]), bs = pb_bit_length(S - 1);
        if (bx > PB_AXIS_BITS || by > PB_AXIS_BITS || bz > PB_AXIS_BITS || bx + by + bz + bs > 64)
            return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "pcd build: (segment, voxel index) needs more than 64 bits");
        segshift = bx + by + bz;
        const uint32_t bits = segshift + bs;
        hipLaunchKernelGGL(k_pb_keys, dim3(ntiles), dim3(PB_THREADS), 0, ctx->stream, (const double *)d_pts.get(), (const uint32_t *)d_seg.get(),
                           (const double *)d_origin.get(), voxel, M, by, bz, bs ? segshift : 64u, d_keys[0].get(), d_idx[0].get());
        if (!bs) segshift = 64;
        int cur = 0;
        for (uint32_t shift = 0; shift < bits; shift += 8) {
            hipLaunchKernelGGL(k_pb_hist, dim3(ntiles), dim3(PB_THREADS), 0, ctx->stream, (const unsigned long long *)d_keys[cur].get(), M, shift, ntiles,
                               d_hist.get());
            pb_scan(ctx, d_hist.get(), nhist, d_tops.get(), total);
            hipLaunchKernelGGL(k_pb_scatter, dim3(ntiles), dim3(PB_THREADS), 0, ctx->stream, (const unsigned long long *)d_keys[cur].get(),
                               (const uint32_t *)d_idx[cur].get(), M, shift, ntiles, (const uint32_t *)d_hist.get(), d_keys[cur ^ 1].get(), d_idx[cur ^ 1].get());
            cur ^= 1;
        }
        sorted_keys = d_keys[cur].get();
        sorted_idx = d_idx[cur].get();
        hipLaunchKernelGGL(k_pb_heads, dim3(ntiles), dim3(PB_THREADS), 0, ctx->stream, sorted_keys, M, d_runid.get());
        pb_scan(ctx, d_runid.get(), M, d_tops.get(), nruns);
        hipLaunchKernelGGL(k_pb_runs, dim3(ntiles), dim3(PB_THREADS), 0, ctx->stream, sorted_keys, (const uint32_t *)d_runid.get(), M, d_runstart.get());
        hipLaunchKernelGGL(k_pb_obj_runs, dim3(pb_blocks((size_t)n_objs + 1)), dim3(PB_THREADS), 0, ctx->stream, sorted_keys, (const uint32_t *)d_runid.get(), M,
                           (const uint32_t *)nruns, segshift, n_views, n_objs, d_objrun.get());
        D2R_HIP(ctx, hipGetLastError());
        D2R_HIP(ctx, hipMemcpyAsync(objrun.data(), d_objrun.get(), objrun.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));   // voxels per object: they size the clouds
        R = objrun[n_objs];
        for (uint32_t o = 0; o < n_objs; ++o) sizes[o] = objrun[o + 1] - objrun[o];
    }

    std::vector<PbOut> outs(n_objs);
    for (uint32_t o = 0; o < n_objs; ++o) {
        clouds.emplace_back(new d2r_pcd);
        d2r_pcd *m = clouds.back().get();
        m->device = ctx->device;
        m->n = sizes[o];
        if ((rc = m->xyz.alloc(ctx, (size_t)std::max(sizes[o], 1u) * sizeof(float4), "a point cloud")) ||
            (rc = m->rgb.alloc(ctx, (size_t)std::max(sizes[o], 1u) * 4, "a point cloud")))
            return rc;
        outs[o] = PbOut{m->xyz.get(), m->rgb.get()};
    }
    if (M) {
        if ((rc = d_outs.alloc(ctx, outs.size() * sizeof(PbOut), "pcd build outputs"))) return rc;
        D2R_HIP(ctx, hipMemcpyAsync(d_outs.get(), outs.data(), outs.size() * sizeof(PbOut), hipMemcpyHostToDevice, ctx->stream));
        if (voxel == 0.0)
            hipLaunchKernelGGL(k_pb_write_raw, dim3(pb_blocks(M)), dim3(PB_THREADS), 0, ctx->stream, (const double *)d_pts.get(), (const uint32_t *)d_col.get(),
                               (const uint32_t *)d_seg.get(), (const uint32_t *)d_segstart.get(), M, n_views, (const PbOut *)d_outs.get());
        else
            hipLaunchKernelGGL(k_pb_voxels, dim3(pb_blocks(R)), dim3(PB_THREADS), 0, ctx->stream, (const double *)d_pts.get(), (const uint32_t *)d_col.get(),
                               sorted_keys, sorted_idx, (const uint32_t *)d_runstart.get(), R, M, segshift, n_views, (const uint32_t *)d_objrun.get(),
                               (const PbOut *)d_outs.get());
        D2R_HIP(ctx, hipGetLastError());
    }
    if ((rc = ctx->pcdb_timer.mark(ctx, 2))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));       // `outs` (pageable host memory) has been consumed, the clouds are complete
    ctx->pcdb_timer.done();
    for (uint32_t o = 0; o < n_objs; ++o) out[o] = clouds[o].release();
    return D2R_OK;
}

int d2r_pcd_size(const d2r_pcd *pcd, uint32_t *n)
{
    if (!pcd || !n) return d2r_fail(nullptr, D2R_ERR_INVALID, "pcd size: null argument");
    *n = pcd->n;
    return D2R_OK;
}

int d2r_pcd_read(d2r_ctx *ctx, const d2r_pcd *pcd, float *xyz, uint8_t *rgb)
{
    if (!ctx || !pcd || (pcd->n && (!xyz || !rgb))) return d2r_fail(ctx, D2R_ERR_INVALID, "pcd read: null argument");
    if (pcd->device != ctx->device) return d2r_fail(ctx, D2R_ERR_INVALID, "pcd read: the point cloud belongs to another device");
    if (!pcd->n) return D2R_OK;
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<float4> p(pcd->n);
    std::vector<uint32_t> c(pcd->n);
    D2R_HIP(ctx, hipMemcpyAsync(p.data(), pcd->xyz.get(), p.size() * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(c.data(), pcd->rgb.get(), c.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < p.size(); ++i) {
        xyz[3 * i] = p[i].x;
        xyz[3 * i + 1] = p[i].y;
        xyz[3 * i + 2] = p[i].z;
        rgb[3 * i] = (uint8_t)(c[i] & 255u);
        rgb[3 * i + 1] = (uint8_t)((c[i] >> 8) & 255u);
        rgb[3 * i + 2] = (uint8_t)((c[i] >> 16) & 255u);
    }
    return D2R_OK;
}

int d2r_pcd_build_get_timing(d2r_ctx *ctx, double *ms_out)
{
    if (!ctx || !ms_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    return ctx->pcdb_timer.read(ctx, ms_out, 2, "pcd build timing: no d2r_pcd_build has completed on this context");
}

}  // extern "C"
