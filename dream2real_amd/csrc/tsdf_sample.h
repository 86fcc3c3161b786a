// How a point meets a fused TSDF volume: the one view of a volume that kernels take by value, the cell of a point, the load of the
// cell's eight corners with the weight rule, and the trilinear interpolant with and without its gradient.  The ray caster
// (tsdfvis.hip) and the camera tracker (camtrack.hip, section 2j) read a volume through this and nothing else,
// so the two rules cannot drift apart; the next reader of a volume includes it too.  tests/tsdf_ref.py restates it in numpy
// (cell, lerp3_grad) and both units' references build on that.
// Every step is one IEEE fp32 operation in the written order; the units that include it are built with -ffp-contract=off.
// Compiles for the device and, with nothing from HIP, under a plain host compiler (tests/tsdf_sample_host_main.cpp).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TS_FN __host__ __device__ __forceinline__
#define TS_UNROLL _Pragma("unroll")
#else
#define TS_FN inline
#define TS_UNROLL
#endif

// A voxel, (tsdf, weight) = s[0], s[1]: float2's layout, and like it a native vector of two floats, so that a voxel is read by one
// 8-byte load (a struct of two floats is taken apart into 4-byte loads).
typedef float TsVoxel __attribute__((vector_size(8)));

// tsdf.hip (d2r_tsdf_dev): a volume as its readers see it.  box: the voxels (global coordinates, inclusive) of the blocks any frame
// touched, lo > hi when there is none; every voxel outside it has weight 0.
struct D2rTsdfDev {
    const TsVoxel *vox;          // [nz][ny][nx]
    const float *col;            // [nz][ny][nx][3], nullptr for a volume without colour
    const uint8_t *ever;         // [nbz][nby][nbx] non-zero: some frame touched the block
    int32_t lo[3];               // global coordinate of voxel 0 per axis
    uint32_t nv[3], nb[3];
    int32_t box_lo[3], box_hi[3];
    float voxel, trunc;
    // A reader looks at a cell only when its lowest corner c (global voxel index) has clo <= c <= chi on every axis, and says
    // which cells those are: the ones whose eight corners lie in the touched-block box, or in the grid.  Either way c and c + 1
    // are voxels of the grid.  (|coordinates| <= 2^24 + 2^20: exact in fp32)
    float clo[3], chi[3];
    void cells_of_box()
    {
        for (int a = 0; a < 3; ++a) {
            clo[a] = (float)box_lo[a];
            chi[a] = (float)(box_hi[a] - 1);
        }
    }
    void cells_of_grid()
    {
        for (int a = 0; a < 3; ++a) {
            clo[a] = (float)lo[a];
            chi[a] = (float)(lo[a] + (int32_t)nv[a] - 2);
        }
    }
};

// The cell of the point p: base, the index of its lowest corner's voxel, and the fractions f.  -> false where the caller must not
// look: the corner outside clo .. chi on an axis, p not finite, or, with FLAGS, the cell's own block touched by no frame (every
// weight in it is 0).  f is written either way.
template <bool FLAGS>
TS_FN bool ts_cell(const D2rTsdfDev &V, const float (&p)[3], size_t &base, float (&f)[3])
{
    int q[3];
    bool in = true;
    TS_UNROLL
    for (int a = 0; a < 3; ++a) {
        const float g = p[a] / V.voxel, c = floorf(g);
        in = in && c >= V.clo[a] && c <= V.chi[a];                  // NaN and the infinities fail
        f[a] = g - c;
        q[a] = in ? (int)c - V.lo[a] : 0;
    }
    if (!in) return false;
    if (FLAGS && !V.ever[(((uint32_t)q[2] >> 4) * V.nb[1] + ((uint32_t)q[1] >> 4)) * V.nb[0] + ((uint32_t)q[0] >> 4)]) return false;
    base = ((size_t)q[2] * V.nv[1] + (size_t)q[1]) * V.nv[0] + (size_t)q[0];
    return true;
}

// corner k = x + 2 y + 4 z of the cell at `base`: its voxel's index
TS_FN size_t ts_corner(const D2rTsdfDev &V, size_t base, int k)
{
    return base + (size_t)(k & 1) + (size_t)((k >> 1) & 1) * V.nv[0] + (size_t)(k >> 2) * V.nv[0] * V.nv[1];
}

// t[k] = the tsdf of corner k, one 8-byte load a corner.  -> observed: the eight weights are >= thr.  (Written as four 16-byte loads
// of x-adjacent pairs this measured a quarter slower in the ray caster, docs/history/r26.md; where it pays, as in the tracker, the
// compiler fuses the pairs of this form by itself.)
TS_FN bool ts_corners(const D2rTsdfDev &V, size_t base, float thr, float (&t)[8])
{
    bool ok = true;
    TS_UNROLL
    for (int k = 0; k < 8; ++k) {
        const TsVoxel s = V.vox[ts_corner(V, base, k)];
        ok = ok && s[1] >= thr;                                     // (a NaN weight fails)
        t[k] = s[0];
    }
    return ok;
}

// The trilinear value of the corners t at the fractions f: along x, then y, then z, each step a + f (b - a).  g: the derivative of
// that interpolant by each fraction, in the same operations.
TS_FN float ts_lerp3_grad(const float (&t)[8], const float (&f)[3], float (&g)[3])
{
    const float e00 = t[1] - t[0], e10 = t[3] - t[2], e01 = t[5] - t[4], e11 = t[7] - t[6];
    const float x00 = t[0] + f[0] * e00, x10 = t[2] + f[0] * e10, x01 = t[4] + f[0] * e01, x11 = t[6] + f[0] * e11;
    const float d0 = x10 - x00, d1 = x11 - x01;
    const float y0 = x00 + f[1] * d0, y1 = x01 + f[1] * d1;
    g[2] = y1 - y0;
    g[1] = d0 + f[2] * (d1 - d0);
    const float ey0 = e00 + f[1] * (e10 - e00), ey1 = e01 + f[1] * (e11 - e01);
    g[0] = ey0 + f[2] * (ey1 - ey0);
    return y0 + f[2] * g[2];
}

// ... the value alone (the gradient's operations have no reader and are dropped)
TS_FN float ts_lerp3(const float (&t)[8], const float (&f)[3])
{
    float g[3];
    return ts_lerp3_grad(t, f, g);
}

// observed: the eight corners of the cell at `base` carry weight >= thr; val: the trilinear tsdf there, whatever the weights say
TS_FN bool ts_tsdf(const D2rTsdfDev &V, size_t base, const float (&f)[3], float thr, float &val)
{
    float t[8];
    const bool ok = ts_corners(V, base, thr, t);
    val = ts_lerp3(t, f);
    return ok;
}
