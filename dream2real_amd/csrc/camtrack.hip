// camtrack.hip — camera poses refined against a TSDF volume (cam_pose_refine "tsdf"): frame-to-model tracking on the signed distance
// field itself.  This package's own stand-in for the poses NeRF training optimises in the reference; nothing here stands where
// reference code stands.  The rule is DESIGN.md section 2j, restated in numpy by tests/camtrack_ref.py and held to it by integer
// equality; how a point meets the volume (its cell, the eight corners and the weight rule, the trilinear value and its gradient) is
// tsdf_sample.h's, which tsdfvis.hip reads through too.  Every fp32 step is one IEEE operation in the written order (the library is
// built with -ffp-contract=off), every term of the 29 sums is the exact fp64 product of two fp32 factors, scaled by 2^29, rounded to
// nearest even and added as a 64-bit integer, so the sums are the same bits whatever the order of the reduction.
//   k_ct_linearise  one lane per selected pixel (grid-stride, at most two workgroups a CU): back-projection, the cell's eight (tsdf,
//                   weight) corners (x-adjacent ones come fused: four 16-byte loads), the trilinear value and its analytic gradient,
//                   the gates, 29 integer accumulators in registers; at the end a wave reduction, four waves through LDS, one row of partials a workgroup
//   k_ct_reduce     one workgroup adds the rows up
// The 6 x 6 solve, the exponential and the loop run on the host in fp64 (camtrack_solve.h).  Ordinary vector stores, no atomics,
// no scratch.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "camtrack_solve.h"
#include "d2r_internal.h"

static_assert(CT_SUMS == D2R_CAMTRACK_SUMS && CT_SCALE_LOG2 == D2R_CAMTRACK_SCALE_LOG2, "camtrack_solve.h and d2r.h disagree");

namespace {

constexpr uint32_t CT_THREADS = 256;
constexpr uint32_t CT_ROW = 32;                // int64 slots per row of partials (29 used)
constexpr uint32_t CT_MAX_PIXELS = 1u << 21;   // w h, and so the contributing pixels: section 2j's overflow bound counts on it
constexpr float CT_DEPTH_MAX = 3.0f;           // section 2c's depth validity
// the gates that bound a term (section 2j): |n_a| <= 4, |p_w|_inf <= 8, |r| <= 1 -> |J_i| <= 64, every product <= 2^12
constexpr float CT_N_MAX = 4.0f, CT_P_MAX = 8.0f, CT_R_MAX = 1.0f;

struct CtCam {
    float fx, fy, cx, cy, thr;
    int32_t W, H;
    uint32_t stride, ws, n_sel;                // selected pixels: ws a row, n_sel in all
    float m[12];                               // cam_pose, rows 0..2
};

__device__ __forceinline__ long long ct_term(float a, float b)
{
    return __double2ll_rn(((double)a * (double)b) * CT_SCALE);       // the product is exact, the scaling is exact, one rounding
}

// selected pixel `idx` -> does it contribute; J = [n, p_w x n], r
__device__ __forceinline__ bool ct_pixel(const D2rTsdfDev &V, const CtCam &c, const uint16_t *__restrict__ depth, const uint8_t *__restrict__ mask,
                                         uint32_t idx, float (&J)[6], float &r)
{
    const uint32_t u = (idx % c.ws) * c.stride, v = (idx / c.ws) * c.stride;
    const size_t px = (size_t)v * (size_t)c.W + u;
    const float z = (float)depth[px] / 1000.0f;
    bool ok = mask[px] != 0 && z > 0.f && z <= CT_DEPTH_MAX;
    const float xc = (((float)u - c.cx) / c.fx) * z, yc = (((float)v - c.cy) / c.fy) * z;
    float p[3], f[3], t[8], g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = ((c.m[4 * a] * xc + c.m[4 * a + 1] * yc) + c.m[4 * a + 2] * z) + c.m[4 * a + 3];
        ok = ok && fabsf(p[a]) <= CT_P_MAX;                              // (NaN fails)
    }
    size_t base = 0;
    if (!ok || !ts_cell<false>(V, p, base, f) || !ts_corners(V, base, c.thr, t)) return false;
    const float phi = ts_lerp3_grad(t, f, g);
    r = phi * V.trunc;
    const float n0 = (g[0] * V.trunc) / V.voxel, n1 = (g[1] * V.trunc) / V.voxel, n2 = (g[2] * V.trunc) / V.voxel;
    if (!(fabsf(phi) < 1.0f && fabsf(r) <= CT_R_MAX && fabsf(n0) <= CT_N_MAX && fabsf(n1) <= CT_N_MAX && fabsf(n2) <= CT_N_MAX)) return false;
    J[0] = n0;
    J[1] = n1;
    J[2] = n2;
    J[3] = p[1] * n2 - p[2] * n1;
    J[4] = p[2] * n0 - p[0] * n2;
    J[5] = p[0] * n1 - p[1] * n0;
    return true;
}

// partials [gridDim.x][CT_ROW]: the sums over the pixels this workgroup visited
__global__ __launch_bounds__(CT_THREADS) void k_ct_linearise(D2rTsdfDev V, CtCam c, const uint16_t *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                             long long *__restrict__ partials)
{
    long long acc[CT_SUMS];
#pragma unroll
    for (int k = 0; k < CT_SUMS; ++k) acc[k] = 0;
    for (uint32_t idx = blockIdx.x * CT_THREADS + threadIdx.x; idx < c.n_sel; idx += gridDim.x * CT_THREADS) {
        float J[6], r;
        if (ct_pixel(V, c, depth, mask, idx, J, r)) {
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) acc[k++] += ct_term(J[i], J[j]);
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[21 + i] += ct_term(J[i], r);
            acc[27] += ct_term(r, r);
            acc[28] += 1;
        }
    }
    __shared__ long long part[CT_THREADS / 64][CT_ROW];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (int k = 0; k < CT_SUMS; ++k) {
        long long s = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < CT_SUMS) {
        long long s = 0;
#pragma unroll
        for (uint32_t wv = 0; wv < CT_THREADS / 64; ++wv) s += part[wv][threadIdx.x];
        partials[(size_t)blockIdx.x * CT_ROW + threadIdx.x] = s;
    }
}

// sums[k] = the k-th column of the n_rows rows of partials
__global__ __launch_bounds__(CT_THREADS) void k_ct_reduce(const long long *__restrict__ partials, uint32_t n_rows, long long *__restrict__ sums)
{
    __shared__ long long part[CT_THREADS / CT_ROW][CT_ROW];
    const uint32_t k = threadIdx.x % CT_ROW, g = threadIdx.x / CT_ROW;
    long long s = 0;
    if (k < CT_SUMS)
        for (uint32_t row = g; row < n_rows; row += CT_THREADS / CT_ROW) s += partials[(size_t)row * CT_ROW + k];
    part[g][k] = s;
    __syncthreads();
    if (threadIdx.x < CT_SUMS) {
        long long t = 0;
#pragma unroll
        for (uint32_t i = 0; i < CT_THREADS / CT_ROW; ++i) t += part[i][threadIdx.x];
        sums[threadIdx.x] = t;
    }
}

// ------------------------------------------------------------------------------------------------ host side

// the refusals: pure host work, nothing on the device yet
int ct_check(d2r_ctx *ctx, const d2r_tsdf *vol, const uint16_t *depth, const uint8_t *mask, uint32_t w, uint32_t h, const float *intrinsics,
             const float *pose, float thr, uint32_t stride)
{
    if (!ctx || !vol || !depth || !mask || !intrinsics || !pose) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (d2r_tsdf_device(vol) != ctx->device) return d2r_fail(ctx, D2R_ERR_INVALID, "camera tracking: the volume belongs to another device");
    if (!d2r_is_rigid(pose)) return d2r_fail(ctx, D2R_ERR_INVALID, "camera tracking: cam_pose must be a finite rigid transform");
    if (int rc = d2r_check_cam(ctx, "camera tracking", intrinsics, pose, 0)) return rc;       // (the pose is held to more, above)
    if (stride == 0) return d2r_fail(ctx, D2R_ERR_INVALID, "camera tracking: stride must be >= 1");
    if (w == 0 || h == 0 || (uint64_t)w * h > CT_MAX_PIXELS) return d2r_fail(ctx, D2R_ERR_INVALID, "camera tracking: a frame holds 1 .. 2^21 pixels");
    if (!(thr > 0.f) || !std::isfinite(thr)) return d2r_fail(ctx, D2R_ERR_INVALID, "camera tracking: weight_threshold must be > 0");
    return D2R_OK;
}

struct CtCall {
    D2rTsdfDev V{};                            // the cells of the whole grid: the block flags are not read
    CtCam c{};
    size_t o_depth = 0, o_mask = 0, o_part = 0, o_sums = 0;
    uint32_t grid = 0;
};

// depth and mask to the device, once per call
int ct_upload(d2r_ctx *ctx, d2r_tsdf *vol, const uint16_t *depth, const uint8_t *mask, uint32_t w, uint32_t h, const float *K, float thr,
              uint32_t stride, CtCall &call)
{
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = d2r_tsdf_dev(ctx, vol, &call.V))) return rc;
    call.V.cells_of_grid();
    CtCam &c = call.c;
    c.fx = K[0];
    c.fy = K[4];
    c.cx = K[2];
    c.cy = K[5];
    c.thr = thr;
    c.W = (int32_t)w;
    c.H = (int32_t)h;
    c.stride = stride;
    c.ws = (w + stride - 1) / stride;
    c.n_sel = c.ws * ((h + stride - 1) / stride);
    call.grid = std::max(1u, std::min((c.n_sel + CT_THREADS - 1) / CT_THREADS, (uint32_t)ctx->n_cu * 2u));
    const size_t px = (size_t)w * h;
    D2rStage in(ctx, ctx->ct_in), ws(ctx, ctx->ct_ws);
    call.o_depth = in.add(px * 2);
    call.o_mask = in.add(px);
    call.o_part = ws.add((size_t)call.grid * CT_ROW * 8);
    call.o_sums = ws.add(CT_ROW * 8);
    if ((rc = in.reserve()) || (rc = ws.reserve())) return rc;
    if ((rc = ctx->ct_timer.mark(ctx, 0))) return rc;
    if ((rc = in.upload(call.o_depth, depth, px * 2)) || (rc = in.upload(call.o_mask, mask, px))) return rc;
    if ((rc = ctx->ct_timer.mark(ctx, 1))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));                 // the caller's frame (pageable host memory) has been consumed
    return D2R_OK;
}

// one linearisation at `pose` -> sums (host); ms (optional) gains the kernels' and the download's device-event times
int ct_linearise(d2r_ctx *ctx, CtCall &call, const float *pose, int64_t *sums, double *ms)
{
    memcpy(call.c.m, pose, sizeof call.c.m);
    int rc;
    if ((rc = ctx->ct_it_timer.mark(ctx, 0))) return rc;
    char *in = (char *)ctx->ct_in.p, *ws = (char *)ctx->ct_ws.p;
    long long *part = (long long *)(ws + call.o_part), *dsums = (long long *)(ws + call.o_sums);
    hipLaunchKernelGGL(k_ct_linearise, dim3(call.grid), dim3(CT_THREADS), 0, ctx->stream, call.V, call.c, (const uint16_t *)(in + call.o_depth),
                       (const uint8_t *)(in + call.o_mask), part);
    hipLaunchKernelGGL(k_ct_reduce, dim3(1), dim3(CT_THREADS), 0, ctx->stream, (const long long *)part, call.grid, dsums);
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = ctx->ct_it_timer.mark(ctx, 1))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(sums, dsums, CT_SUMS * 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ctx->ct_it_timer.mark(ctx, 2))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ms) {
        double t[2];
        ctx->ct_it_timer.done();
        if ((rc = ctx->ct_it_timer.read(ctx, t, 2, ""))) return rc;
        ms[0] += t[0];
        ms[1] += t[1];
    }
    return D2R_OK;
}

}  // namespace

extern "C" {

int d2r_camtrack_system(d2r_ctx *ctx, d2r_tsdf *vol, const uint16_t *depth_u16, const uint8_t *mask_u8, uint32_t w, uint32_t h,
                        const float *intrinsics, const float *cam_pose, float weight_threshold, uint32_t stride, int64_t *sums_out)
{
    if (ctx && !sums_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    int rc = ct_check(ctx, vol, depth_u16, mask_u8, w, h, intrinsics, cam_pose, weight_threshold, stride);
    if (rc) return rc;
    CtCall call;
    if ((rc = ct_upload(ctx, vol, depth_u16, mask_u8, w, h, intrinsics, weight_threshold, stride, call))) return rc;
    int64_t sums[CT_SUMS];
    if ((rc = ct_linearise(ctx, call, cam_pose, sums, nullptr))) return rc;
    memcpy(sums_out, sums, sizeof sums);
    return D2R_OK;
}

int d2r_camtrack_refine(d2r_ctx *ctx, d2r_tsdf *vol, const uint16_t *depth_u16, const uint8_t *mask_u8, uint32_t w, uint32_t h,
                        const float *intrinsics, const float *cam_pose_in, const d2r_camtrack_params *params, float *cam_pose_out,
                        d2r_camtrack_report *report)
{
    if (ctx && (!params || !cam_pose_out || !report)) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    int rc = ct_check(ctx, vol, depth_u16, mask_u8, w, h, intrinsics, cam_pose_in, params ? params->weight_threshold : 0.f, params ? params->stride : 0);
    if (rc) return rc;
    if (params->max_iters == 0 || params->max_iters > D2R_CAMTRACK_MAX_ITERS)
        return d2r_fail(ctx, D2R_ERR_INVALID, "camera tracking: max_iters must be 1 .. 64");
    CtCall call;
    if ((rc = ct_upload(ctx, vol, depth_u16, mask_u8, w, h, intrinsics, params->weight_threshold, params->stride, call))) return rc;

    // the report is built aside and copied out once the call has succeeded
    static thread_local d2r_camtrack_report rep;
    memset(&rep, 0, sizeof rep);
    double T[12], ms[2] = {0.0, 0.0};
    for (int i = 0; i < 12; ++i) T[i] = (double)cam_pose_in[i];
    float out[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.f, 0.f, 0.f, 1.f};
    rep.status = D2R_CAMTRACK_MAX_ITERS_REACHED;
    bool keep_input = false;
    for (uint32_t it = 0; it < params->max_iters; ++it) {
        float *P = rep.poses[it];
        for (int i = 0; i < 12; ++i) P[i] = (float)T[i];
        P[12] = P[13] = P[14] = 0.f;
        P[15] = 1.f;
        int64_t *s = rep.sums[it];
        if ((rc = ct_linearise(ctx, call, P, s, ms))) return rc;
        rep.iters = it + 1;
        rep.pixels_last = (uint64_t)s[28];
        rep.rms_last = ct_rms(s);
        if (it == 0) {
            rep.pixels_first = rep.pixels_last;
            rep.rms_first = rep.rms_last;
        }
        if (s[28] < (int64_t)params->min_pixels) {
            rep.status = D2R_CAMTRACK_TOO_FEW;
            keep_input = true;
            break;
        }
        double xi[6], E[12];
        if (!ct_solve(s, xi)) {
            rep.status = D2R_CAMTRACK_DEGENERATE;
            break;
        }
        ct_exp(xi, E);
        ct_apply(E, T);
        const double nv = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]), nw = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
        if (nv < CT_CONVERGED && nw < CT_CONVERGED) {
            rep.status = D2R_CAMTRACK_CONVERGED;
            break;
        }
    }
    for (int i = 0; i < 12; ++i) out[i] = (float)T[i];
    memcpy(cam_pose_out, keep_input ? cam_pose_in : out, sizeof out);
    memcpy(report, &rep, sizeof rep);
    ctx->ct_timer.done();
    double up = 0.0;
    if ((rc = ctx->ct_timer.read(ctx, &up, 1, ""))) return rc;
    ctx->ct_ms[0] = up;
    ctx->ct_ms[1] = ms[0];
    ctx->ct_ms[2] = ms[1];
    ctx->ct_timed = true;
    return D2R_OK;
}

int d2r_camtrack_get_timing(d2r_ctx *ctx, double *ms_out)
{
    if (!ctx || !ms_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (!ctx->ct_timed) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_camtrack_get_timing: no d2r_camtrack_refine has completed on this context");
    for (int i = 0; i < 3; ++i) ms_out[i] = ctx->ct_ms[i];
    return D2R_OK;
}

}  // extern "C"
