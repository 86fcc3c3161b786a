// geoprop_plane.h — the host side of DESIGN.md section 2l that needs nothing from HIP: the refusals of d2r_geoprop_masks, the height
// bins of the scene bounds, the choice of the support plane from the histogram and the selection of the components that become
// proposals.  Compiles under a plain host compiler (tests/geoprop_host_main.cpp, which supplies d2r_fail).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "d2r_shared.h"

constexpr uint32_t GP_NONE = 0xffffffffu;                       // a pixel without a height bin: no depth, or outside the bounds
constexpr uint32_t GP_REC_WORDS = D2R_GEOPROP_REC_WORDS;        // root, area, i0, j0, i1, j1

// the height bins of the bounds: bin b holds the points whose height floor(1000 (up . p) + 0.5) is b, lo <= b < lo + n.  The
// box's lowest and highest corner along `up` are summed per axis in the order x, y, z and widened by a millimetre on either side
// (a point inside the bounds sums its three products in another grouping and may round across the face's bin); a bin outside is
// clamped into the range.
struct GpBins {
    int64_t lo;
    uint32_t n;             // 3 .. 2^16
};

struct GpPlane {
    int32_t bin;            // b*: the centre of the fullest window, millimetres along `up`; 0 without a plane
    uint32_t count;         // the inside pixels in the window_mm bins centred on b*
    uint32_t inside;        // the inside pixels; 0 = no plane
};

inline int gp_bins(d2r_ctx *ctx, const double *bounds, const double *up, GpBins *out)
{
    if (!bounds || !up || !out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(bounds[a]) || !std::isfinite(bounds[3 + a]) || !(bounds[a] < bounds[3 + a]))
            return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: bounds must be finite with min < max on every axis");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(up[a])) return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: up must be a unit vector (to 1e-6)");
    const double len = sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]);
    if (!(fabs(len - 1.0) <= 1e-6)) return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: up must be a unit vector (to 1e-6)");
    double m[3], M[3];
    for (int a = 0; a < 3; ++a) {
        const double p = up[a] * bounds[a], q = up[a] * bounds[3 + a];
        m[a] = std::min(p, q);
        M[a] = std::max(p, q);
    }
    const double lo = floor(1000.0 * ((m[0] + m[1]) + m[2]) + 0.5) - 1.0, hi = floor(1000.0 * ((M[0] + M[1]) + M[2]) + 0.5) + 1.0;
    if (!(fabs(lo) <= 1e9 && fabs(hi) <= 1e9) || hi - lo + 1.0 > (double)D2R_GEOPROP_MAX_BINS)
        return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: the bounds span more than 2^16 height bins of a millimetre");
    out->lo = (int64_t)lo;
    out->n = (uint32_t)((int64_t)hi - (int64_t)lo + 1);
    return D2R_OK;
}

// everything d2r_geoprop_masks refuses, before any device work: K = fx fy cx cy
inline int gp_check(d2r_ctx *ctx, const double *bounds, const double *up, const d2r_geoprop_params *p, uint32_t w, uint32_t h, const double *K,
                    const uint16_t *d16, const float *pose, const void *labels_out, const void *recs_out, const void *n_out, const void *plane_out,
                    GpBins *bins)
{
    if (!bounds || !up || !p || !K || !d16 || !pose || !labels_out || !recs_out || !n_out || !plane_out || !bins)
        return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (w == 0 || h == 0 || (uint64_t)w * h > D2R_LABELTRACK_MAX_PIXELS)
        return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: a frame holds 1 .. 2^21 pixels");
    if (!d2r_is_rigid(pose)) return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: cam_pose must be a finite rigid transform");
    if (!std::isfinite(K[0]) || !std::isfinite(K[1]) || !(K[0] > 0.0) || !(K[1] > 0.0))
        return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: the focal lengths must be finite and > 0");
    if (!std::isfinite(K[2]) || !std::isfinite(K[3])) return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: the principal point must be finite");
    if (p->window_mm < 1 || !(p->window_mm & 1u) || p->window_mm > 65535)
        return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: window_mm must be odd, 1 .. 65535");
    if (p->h_min_mm > 65535) return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: h_min_mm must be 0 .. 65535");
    if (p->tau_mm > 65535) return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: tau_mm must be 0 .. 65535");
    if (p->max_props < 1 || p->max_props > D2R_PROP_MAX)
        return d2r_fail(ctx, D2R_ERR_INVALID, "mask proposals: max_props must be 1 .. " + std::to_string(D2R_PROP_MAX));
    return gp_bins(ctx, bounds, up, bins);
}

// b* maximises the sum of the window_mm bins centred on it (bins outside the range count 0); ties go to the lowest bin
inline GpPlane gp_plane(const uint32_t *hist, const GpBins &bins, uint32_t window_mm)
{
    GpPlane out{0, 0, 0};
    const int64_t n = bins.n, half = window_mm / 2;
    uint64_t total = 0, sum = 0, best = 0;
    int64_t at = 0;
    for (int64_t b = 0; b < n; ++b) total += hist[b];
    if (total == 0) return out;
    for (int64_t b = 0; b <= std::min(half, n - 1); ++b) sum += hist[b];          // the window centred on bin 0
    for (int64_t b = 0; b < n; ++b) {
        if (sum > best) {
            best = sum;
            at = b;
        }
        if (b + half + 1 < n) sum += hist[b + half + 1];
        if (b - half >= 0) sum -= hist[b - half];
    }
    out.bin = (int32_t)(bins.lo + at);
    out.count = (uint32_t)best;
    out.inside = (uint32_t)total;
    return out;
}

// the first index a pixel's bin must reach to be above the plane: b* + h_min_mm - lo, GP_NONE - 1 when no bin can (GP_NONE marks
// a pixel without a bin and compares below it)
inline uint32_t gp_threshold(const GpPlane &pl, const GpBins &bins, uint32_t h_min_mm)
{
    if (pl.inside == 0) return GP_NONE - 1;
    const int64_t t = (int64_t)pl.bin + (int64_t)h_min_mm - bins.lo;
    return t >= (int64_t)bins.n ? GP_NONE - 1 : (uint32_t)std::max<int64_t>(t, 0);
}

// cand: n records of GP_REC_WORDS words (root, area, ...) in any order, every one of area >= min_area.  Keeps the max_props largest
// (area ties to the smaller root) and orders the kept ones by root: record k becomes proposal k + 1.
inline void gp_select(std::vector<uint32_t> &cand, uint32_t max_props)
{
    const size_t n = cand.size() / GP_REC_WORDS;
    std::vector<uint32_t> order(n);
    for (size_t k = 0; k < n; ++k) order[k] = (uint32_t)k;
    auto rec = [&](uint32_t k) { return cand.data() + (size_t)k * GP_REC_WORDS; };
    if (n > max_props) {
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return rec(a)[1] != rec(b)[1] ? rec(a)[1] > rec(b)[1] : rec(a)[0] < rec(b)[0];
        });
        order.resize(max_props);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rec(a)[0] < rec(b)[0]; });
    std::vector<uint32_t> out(order.size() * GP_REC_WORDS);
    for (size_t k = 0; k < order.size(); ++k) std::copy(rec(order[k]), rec(order[k]) + GP_REC_WORDS, out.begin() + k * GP_REC_WORDS);
    cand.swap(out);
}
