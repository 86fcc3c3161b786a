// The host arithmetic of the camera-pose refinement (camtrack.hip): the 6 x 6 normal equations out of the 29
// integer sums, their LDL^T solve, the exponential of a twist and the pose update.  Pure fp64 on the host, every sum in a written
// order (tests/camtrack_ref.py restates it line by line); stands on its own.
#pragma once
#include <math.h>
#include <stdint.h>

constexpr int CT_SUMS = 29;                    // 21 upper triangle of J^T J (row-major, i <= j), 6 J^T r, sum r^2, count
constexpr int CT_SCALE_LOG2 = 29;              // S = 2^29: section 2j's derivation
constexpr double CT_SCALE = 536870912.0;
constexpr double CT_PIVOT_REL = 1e-6;          // a pivot <= this times the largest diagonal entry: degenerate (section 2j: three times the interpolant's own floor)
constexpr double CT_CONVERGED = 1e-5;          // |v| metres and |omega| radians

// -> false: degenerate (a pivot <= CT_PIVOT_REL max diag, or not finite).  xi = -A^-1 b, A = L D L^T.
// d_j = A_jj - sum_{k<j} L_jk^2 d_k; L_ij = (A_ij - sum_{k<j} L_ik L_jk d_k) / d_j, the sums over k ascending;
// L y = -b forward, z = y / d, L^T xi = z backward, the sums over the index ascending.
inline bool ct_solve(const int64_t sums[CT_SUMS], double xi[6])
{
    double A[6][6], b[6], L[6][6], d[6], y[6];
    int q = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++q) A[i][j] = A[j][i] = (double)sums[q] / CT_SCALE;
    for (int i = 0; i < 6; ++i) b[i] = (double)sums[21 + i] / CT_SCALE;
    double dmax = 0.0;
    for (int i = 0; i < 6; ++i) dmax = fmax(dmax, A[i][i]);
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
        for (int k = 0; k < j; ++k) s -= (L[j][k] * L[j][k]) * d[k];
        if (!(s > CT_PIVOT_REL * dmax)) return false;                // (NaN fails too)
        d[j] = s;
        for (int i = j + 1; i < 6; ++i) {
            double t = A[i][j];
            for (int k = 0; k < j; ++k) t -= (L[i][k] * L[j][k]) * d[k];
            L[i][j] = t / s;
        }
    }
    for (int i = 0; i < 6; ++i) {
        double t = -b[i];
        for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
        y[i] = t;
    }
    for (int i = 0; i < 6; ++i) y[i] = y[i] / d[i];
    for (int i = 5; i >= 0; --i) {
        double t = y[i];
        for (int k = i + 1; k < 6; ++k) t -= L[k][i] * xi[k];
        xi[i] = t;
    }
    return true;
}

// E (rows 0..2 of a rigid 4x4, row-major [3][4]) = exp(xi^), xi = (v, omega): R = I + a W + b W^2, t = (I + b W + c W^2) v with
// W = [omega]x, theta = |omega|, a = sin(theta) / theta, b = 2 sin^2(theta / 2) / theta^2, c = (theta - sin(theta)) / theta^3; below
// theta = 1e-4 the series a = 1 - theta^2 / 6, b = 1/2 - theta^2 / 24, c = 1/6 - theta^2 / 120 (their next terms are below 1e-18).
inline void ct_exp(const double xi[6], double E[12])
{
    const double wx = xi[3], wy = xi[4], wz = xi[5];
    const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
    double a, b, c;
    if (th < 1e-4) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
        c = 1.0 / 6.0 - th2 / 120.0;
    } else {
        const double s = sin(th), h = sin(0.5 * th);
        a = s / th;
        b = (2.0 * (h * h)) / th2;
        c = (th - s) / (th2 * th);
    }
    const double W[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
    double W2[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[i][j] = (W[i][0] * W[0][j] + W[i][1] * W[1][j]) + W[i][2] * W[2][j];
    for (int i = 0; i < 3; ++i) {
        double V[3];
        for (int j = 0; j < 3; ++j) {
            const double id = i == j ? 1.0 : 0.0;
            E[i * 4 + j] = (id + a * W[i][j]) + b * W2[i][j];
            V[j] = (id + b * W[i][j]) + c * W2[i][j];
        }
        E[i * 4 + 3] = (V[0] * xi[0] + V[1] * xi[1]) + V[2] * xi[2];
    }
}

// T <- exp(xi^) T for the rows 0..2 of T (row-major [3][4]): R' = E_R R, t' = E_R t + E_t, each sum left to right
inline void ct_apply(const double E[12], double T[12])
{
    double out[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j) out[i * 4 + j] = (E[i * 4] * T[j] + E[i * 4 + 1] * T[4 + j]) + E[i * 4 + 2] * T[8 + j];
        out[i * 4 + 3] += E[i * 4 + 3];
    }
    for (int i = 0; i < 12; ++i) T[i] = out[i];
}

inline double ct_rms(const int64_t sums[CT_SUMS])
{
    return sums[28] > 0 ? sqrt(((double)sums[27] / CT_SCALE) / (double)sums[28]) : 0.0;
}
