// labeltrack_grid.h — the host side of DESIGN.md section 2k that needs nothing from HIP: the grid over the scene bounds and the
// refusals of d2r_labeltrack_scan.  Compiles under a plain host compiler (tests/labeltrack_host_main.cpp, which supplies d2r_fail).
#pragma once
#include <math.h>
#include <stdint.h>

#include "d2r_shared.h"

constexpr uint32_t LT_UNKNOWN = D2R_LABELTRACK_UNKNOWN;
constexpr uint32_t LT_SWEEPS = D2R_LABELTRACK_SWEEPS_PER_LAUNCH;   // sweeps per fill launch = the halo of a tile
constexpr float LT_DEPTH_MAX = 3.0f;                               // section 2c's depth validity

struct LtGrid {
    int32_t lo[3];          // the first voxel per axis: voxel g sits at (float)g * voxel
    uint32_t n[3];          // voxels per axis
    uint32_t n_vox;         // n[0] n[1] n[2] <= 2^31
    float voxel, band;      // band = (float)band_voxels * voxel
};

// the parameters' ranges, then per axis lo = floor((lo_b - band) / voxel), hi = ceil((hi_b + band) / voxel) in fp64 of the fp32
// values, n = hi - lo + 1
inline int lt_grid(d2r_ctx *ctx, const double *bounds, const d2r_labeltrack_params *p, LtGrid *g)
{
    if (!bounds || !p || !g) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (!(p->voxel > 0.f) || !std::isfinite(p->voxel)) return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: voxel must be finite and > 0");
    if (p->band_voxels < 1 || p->band_voxels > 8) return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: band_voxels must be 1 .. 8");
    if (p->tau_mm > 65535) return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: tau_mm must be 0 .. 65535");
    if (p->grow > 4096) return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: grow must be 0 .. 4096");
    LtGrid out{};
    out.voxel = p->voxel;
    out.band = (float)p->band_voxels * p->voxel;
    if (!std::isfinite(out.band)) return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: band_voxels * voxel is not finite");
    uint64_t total = 1;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(bounds[a]) || !std::isfinite(bounds[3 + a]) || !(bounds[a] <= bounds[3 + a]))
            return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: bounds must be finite with min <= max on every axis");
        const double lo = floor(((double)(float)bounds[a] - (double)out.band) / (double)out.voxel);
        const double hi = ceil(((double)(float)bounds[3 + a] + (double)out.band) / (double)out.voxel);
        if (!(fabs(lo) <= (double)D2R_LABELTRACK_MAX_COORD && fabs(hi) <= (double)D2R_LABELTRACK_MAX_COORD))       // (NaN fails)
            return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: the grid reaches beyond 2^23 voxels from the origin");
        out.lo[a] = (int32_t)lo;
        out.n[a] = (uint32_t)((int64_t)hi - (int64_t)lo + 1);
        total *= out.n[a];                       // each factor <= 2^24 + 1, checked after every one: no overflow
        if (total > D2R_LABELTRACK_MAX_VOXELS) return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: the grid holds more than 2^31 voxels");
    }
    out.n_vox = (uint32_t)total;
    *g = out;
    return D2R_OK;
}

// what d2r_labeltrack_scan refuses beyond the grid: K = fx fy cx cy
inline int lt_check_frames(d2r_ctx *ctx, uint32_t n, uint32_t w, uint32_t h, const double *K, const uint16_t *d16, const float *poses,
                           const uint8_t *labels0, const uint8_t *labels_out)
{
    if (!K || !d16 || !poses || !labels0 || !labels_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (n == 0) return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: no frames");
    if (w == 0 || h == 0 || (uint64_t)w * h > D2R_LABELTRACK_MAX_PIXELS) return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: a frame holds 1 .. 2^21 pixels");
    for (uint32_t f = 0; f < n; ++f)
        if (!d2r_is_rigid(poses + (size_t)f * 16))
            return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: cam_pose " + std::to_string(f) + " must be a finite rigid transform");
    const double K9[9] = {K[0], 0.0, K[2], 0.0, K[1], K[3], 0.0, 0.0, 1.0};
    if (int rc = d2r_check_cam(ctx, "label tracking", K9, poses, 0)) return rc;          // (the poses are held to more, above)
    if (!std::isfinite((float)K[0]) || !std::isfinite((float)K[1]) || (float)K[0] == 0.f || (float)K[1] == 0.f || !std::isfinite((float)K[2]) ||
        !std::isfinite((float)K[3]))
        return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: the intrinsics must be finite and the focal lengths non-zero in fp32");
    for (size_t i = 0; i < (size_t)w * h; ++i)
        if (labels0[i] == LT_UNKNOWN) return d2r_fail(ctx, D2R_ERR_INVALID, "label tracking: labels0 must not contain 255");
    return D2R_OK;
}
