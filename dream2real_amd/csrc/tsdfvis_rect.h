// The host arithmetic of the colour-TSDF ray caster (tsdfvis.hip): a candidate's ray matrix, its inverse and the frame
// rectangle its movable volume can show in.  Pure fp64 arithmetic on the host; stands on its own with d2r_shared.h's 4x4 toolkit
// (tests/tsdfvis_host_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>

struct TvRect { int32_t x0, y0, x1, y1; };       // inclusive; x1 < x0: no pixel

// The poses are rigid to 1e-5 (d2r_is_rigid); the rectangle below does not lean on that tolerance: it is projected with the inverse
// of the very matrix the kernel marches with, however far the poses' origins lie.
//
// The fp64 inverse (row-major 4x4, last row 0 0 0 1) of the affine map whose rows 0..2 are the fp32 matrix m [3][4], by cofactors.
// This is the true inverse of the rounded matrix the kernel marches with, not a product of transposed inverses: the two differ by
// twice a pose's deviation from orthogonal times the distance to its origin, 18 mm for a pose scaled by 1 + 4.5e-6 two kilometres
// from the origin, which cut pixels off the rectangle.  A singular or non-finite m gives NaNs: tv_box_rect then takes the whole frame.
inline void tv_inverse34(const float m[12], double out[16])
{
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double co[3][3] = {{e * i - f * h, c * h - b * i, b * f - c * e}, {f * g - d * i, a * i - c * g, c * d - a * f}, {d * h - e * g, b * g - a * h, a * e - b * d}};
    const double det = (a * co[0][0] + b * co[1][0]) + c * co[2][0];
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) out[r * 4 + k] = co[r][k] / det;
        out[r * 4 + 3] = -((out[r * 4] * (double)m[3] + out[r * 4 + 1] * (double)m[7]) + out[r * 4 + 2] * (double)m[11]);
    }
    out[12] = out[13] = out[14] = 0.0;
    out[15] = 1.0;
}

// The pixels whose rays can meet the box [lo, hi] (metres, the volume's frame) when `to_cam` (rows 0..2 used) takes the volume's
// frame to the camera's: the bounds of the eight projected corners, widened by a pixel and clipped to the frame.  `slack` (metres)
// widens the box by what the kernel's fp32 sample points can be off.  A corner at or behind z = near, or anything not finite,
// gives the whole frame; a box with lo > hi on an axis gives no pixel.
inline TvRect tv_box_rect(const double to_cam[16], const double lo[3], const double hi[3], double slack, double fx, double fy, double cx,
                          double cy, double near, int32_t W, int32_t H)
{
    const TvRect whole{0, 0, W - 1, H - 1}, none{0, 0, -1, -1};
    for (int a = 0; a < 3; ++a)
        if (!(lo[a] <= hi[a])) return (lo[a] > hi[a]) ? none : whole;      // NaN: whole
    double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
    for (int k = 0; k < 8; ++k) {
        const double p[3] = {(k & 1) ? hi[0] + slack : lo[0] - slack, (k & 2) ? hi[1] + slack : lo[1] - slack,
                             (k & 4) ? hi[2] + slack : lo[2] - slack};
        double q[3];
        for (int r = 0; r < 3; ++r) q[r] = ((to_cam[r * 4] * p[0] + to_cam[r * 4 + 1] * p[1]) + to_cam[r * 4 + 2] * p[2]) + to_cam[r * 4 + 3];
        if (!(q[2] > near) || !(q[2] > 0.0)) return whole;
        const double u = fx * q[0] / q[2] + cx, v = fy * q[1] / q[2] + cy;
        if (!std::isfinite(u) || !std::isfinite(v)) return whole;
        umin = std::min(umin, u);
        umax = std::max(umax, u);
        vmin = std::min(vmin, v);
        vmax = std::max(vmax, v);
    }
    // (the clamps keep the conversions to int defined)
    const double x0 = std::max(floor(umin) - 1.0, 0.0), x1 = std::min(ceil(umax) + 1.0, (double)W - 1.0);
    const double y0 = std::max(floor(vmin) - 1.0, 0.0), y1 = std::min(ceil(vmax) + 1.0, (double)H - 1.0);
    if (x1 < x0 || y1 < y0) return none;
    return TvRect{(int32_t)x0, (int32_t)y0, (int32_t)x1, (int32_t)y1};
}
