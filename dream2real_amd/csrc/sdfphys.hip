// sdfphys.hip — the physics pre-filter answered from the TSDF volumes themselves: points against a bit field (DESIGN.md
// section 2e).  The second backend of unsupcol_check beside phys.hip's hulls + GJK: no mesh, no convex parts.
//
// The static scene is one "touch" bit per voxel (tsdf.hip k_tsdf_touch_bits: observed and within the contact distance of the
// surface or behind it), the movable object the centres of its observed solid voxels.  A pose moves the points by
// T = pose inv(init_pose); "collides / is supported / is stable" become "any point lands on a set bit" under six probe
// translations (the pose, lowered along gravity, and the lowered pose pushed sideways four ways).
//   k_sdf_coarse   one bit per 16^3 block of the field: any bit set (the field is mostly free space and unobserved solid)
//   k_sdf_check    one wave per pose, a point per lane and step; the six probes share one rotation of the point; a wave leaves
//                  as soon as probe 0 hits (a collision decides) and stops evaluating probes whose answer it has
// Poses share nothing: no LDS, no atomics.  The bit field of a table-top scene is a few MB and stays in L2 / Infinity Cache,
// the coarse mask (2 - 64 KB) in L1 / L2.  Every value is written by ordinary vector stores from C++.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "d2r_internal.h"

#define D2R_SDF_MAX_VOXELS (1ull << 31)

struct SdfGrid {
    int32_t lo[3];          // first voxel per axis, global voxel coordinates (16 b0)
    uint32_t nv[3];         // voxels per axis
    uint32_t wpr;           // words per row: ceil(nx / 32)
    uint32_t ncb[3];        // 16^3 blocks per axis: ceil(nv / 16)
    float voxel;
};

struct d2r_sdfphys {
    d2r_ctx *ctx = nullptr;
    int device = 0;
    SdfGrid G{};
    D2rDev<uint32_t> d_words;       // [nz][ny][wpr] touch bits, all static grids ORed
    D2rDev<uint32_t> d_coarse;      // [ceil(blocks / 32)] bit (bz ncby + by) ncbx + bx
    D2rDev<float> d_pts;            // [3][n_points] x, y, z of the movable points (SoA), world frame at the initial pose
    uint32_t n_points = 0;
    D2rStageTimer timer;            // upload / kernel / download of the last check
};

struct SdfCheckParams {
    double inv[12];         // rows 0..2 of inv(init_pose) = [R^T | -R^T t]
    float table_z;
    float drop[3];          // unsup_thresh * gravity
    float perturb;
    int stability_check;
    uint32_t oris_per_pos;
};

namespace {

constexpr uint32_t SDF_THREADS = 256;        // 4 waves, one pose each

// coarse[w] bit k = any touch bit in block 32 w + k.  One wave per word of the mask: 32 blocks x 256 rows of 16 bits.
__global__ __launch_bounds__(SDF_THREADS) void k_sdf_coarse(const uint32_t *__restrict__ words, SdfGrid G, uint32_t n_blocks, uint32_t n_cwords,
                                                            uint32_t *__restrict__ coarse)
{
    const uint32_t cw = blockIdx.x * (SDF_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (cw >= n_cwords) return;
    uint32_t out = 0;
    for (uint32_t k = 0; k < 32; ++k) {
        const uint32_t cb = cw * 32u + k;
        if (cb >= n_blocks) break;
        const uint32_t bx = cb % G.ncb[0], by = (cb / G.ncb[0]) % G.ncb[1], bz = cb / (G.ncb[0] * G.ncb[1]);
        const uint32_t half = 0xffffu << (16u * (bx & 1u));             // the block's 16 voxels of its rows' word bx >> 1
        bool any = false;
        for (uint32_t r = lane; r < 256; r += 64) {
            const uint32_t y = by * 16u + (r & 15u), z = bz * 16u + (r >> 4);
            if (y < G.nv[1] && z < G.nv[2]) any = any || (words[((size_t)z * G.nv[1] + y) * G.wpr + (bx >> 1)] & half) != 0;
        }
        if (__ballot(any)) out |= 1u << k;
    }
    if (lane == 0) coarse[cw] = out;
}

// does the voxel (floorf'ed coordinates, still floats: huge and NaN values fail the range test and index nothing) carry a bit?
__device__ __forceinline__ bool sdf_touch(const SdfGrid &G, const float lo[3], const float hi[3], const uint32_t *__restrict__ words,
                                          const uint32_t *__restrict__ coarse, float fx, float fy, float fz)
{
    if (!(fx >= lo[0] && fx < hi[0] && fy >= lo[1] && fy < hi[1] && fz >= lo[2] && fz < hi[2])) return false;
    const uint32_t x = (uint32_t)((int32_t)fx - G.lo[0]), y = (uint32_t)((int32_t)fy - G.lo[1]), z = (uint32_t)((int32_t)fz - G.lo[2]);
    const uint32_t cb = ((z >> 4) * G.ncb[1] + (y >> 4)) * G.ncb[0] + (x >> 4);
    if (!((coarse[cb >> 5] >> (cb & 31u)) & 1u)) return false;
    return (words[((size_t)z * G.nv[1] + y) * G.wpr + (x >> 5)] >> (x & 31u)) & 1u;
}

__global__ __launch_bounds__(SDF_THREADS) void k_sdf_check(SdfCheckParams P, SdfGrid G, const float *__restrict__ poses, uint32_t n_poses,
                                                           const uint8_t *__restrict__ ori_mask, const uint32_t *__restrict__ words,
                                                           const uint32_t *__restrict__ coarse, const float *__restrict__ pts, uint32_t n_points,
                                                           uint8_t *__restrict__ valid)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pose = blockIdx.x * (SDF_THREADS / 64) + (threadIdx.x >> 6);
    if (pose >= n_poses) return;                             // everything below is uniform over the wave
    if (!valid[pose]) return;
    if (!ori_mask[pose % P.oris_per_pos]) {                  // duplicate orientation / not regraspable
        if (lane == 0) valid[pose] = 0;
        return;
    }
    // T = pose inv(init_pose), rows 0..2: fp64, each entry summed over l = 0 .. 3 in order (inv's last row is 0 0 0 1), rounded once
    const float *M = poses + (size_t)pose * 16;
    float T[12];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double last = j == 3 ? 1.0 : 0.0;
            T[i * 4 + j] = (float)((((double)M[i * 4 + 0] * P.inv[j] + (double)M[i * 4 + 1] * P.inv[4 + j]) + (double)M[i * 4 + 2] * P.inv[8 + j]) +
                                   (double)M[i * 4 + 3] * last);
        }
    // probe translations: 0 the pose, 1 lowered, 2 / 3 lowered and pushed along +x / -x, 4 / 5 along +y / -y.  Probes 4, 5 share
    // probe 1's x, probes 2, 3 its y, probes 2 .. 5 its z.
    const float t0x = T[3], t0y = T[7], t0z = T[11];
    const float t1x = t0x + P.drop[0], t1y = t0y + P.drop[1], t1z = t0z + P.drop[2];
    const float t2x = t1x + P.perturb, t3x = t1x + -P.perturb, t4y = t1y + P.perturb, t5y = t1y + -P.perturb;
    const bool below_table = M[11] < P.table_z;              // the sampled pose's own z (reference :332-333)
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = (float)G.lo[a];
        hi[a] = (float)(G.lo[a] + (int32_t)G.nv[a]);
    }
    // the probes whose answer can still change the verdict: below the table only the collision counts
    uint32_t need = below_table ? 1u : (P.stability_check ? 63u : 3u), hit = 0;
    const float *px = pts, *py = pts + n_points, *pz = pts + 2 * (size_t)n_points;
    const float v = G.voxel;
    for (uint32_t i0 = 0; i0 < n_points && !(hit & 1u); i0 += 64) {
        const uint32_t i = i0 + lane;
        uint32_t m = 0;
        if (i < n_points) {
            const float x = px[i], y = py[i], z = pz[i];
            const float rx = (T[0] * x + T[1] * y) + T[2] * z, ry = (T[4] * x + T[5] * y) + T[6] * z, rz = (T[8] * x + T[9] * y) + T[10] * z;
            m = sdf_touch(G, lo, hi, words, coarse, floorf((rx + t0x) / v + 0.5f), floorf((ry + t0y) / v + 0.5f), floorf((rz + t0z) / v + 0.5f)) ? 1u : 0u;
            if (need & 62u) {
                const float f1x = floorf((rx + t1x) / v + 0.5f), f1y = floorf((ry + t1y) / v + 0.5f), f1z = floorf((rz + t1z) / v + 0.5f);
                if (need & 2u) m |= sdf_touch(G, lo, hi, words, coarse, f1x, f1y, f1z) ? 2u : 0u;
                if (need & 4u) m |= sdf_touch(G, lo, hi, words, coarse, floorf((rx + t2x) / v + 0.5f), f1y, f1z) ? 4u : 0u;
                if (need & 8u) m |= sdf_touch(G, lo, hi, words, coarse, floorf((rx + t3x) / v + 0.5f), f1y, f1z) ? 8u : 0u;
                if (need & 16u) m |= sdf_touch(G, lo, hi, words, coarse, f1x, floorf((ry + t4y) / v + 0.5f), f1z) ? 16u : 0u;
                if (need & 32u) m |= sdf_touch(G, lo, hi, words, coarse, f1x, floorf((ry + t5y) / v + 0.5f), f1z) ? 32u : 0u;
            }
        }
        // wave votes: which probes any lane hit this step (need, hit and the loop condition stay uniform)
#pragma unroll
        for (uint32_t q = 0; q < 6; q++)
            if (__ballot((m >> q) & 1u)) hit |= 1u << q;
        need &= ~hit | 1u;
    }
    // the verdict (reference :308-370 with "any point touches" for pairwise_collision)
    bool ok = !(hit & 1u);
    if (ok && !below_table) {
        ok = (hit & 2u) != 0;
        if (ok && P.stability_check) ok = (hit & 60u) == 60u;
    }
    if (lane == 0) valid[pose] = ok ? 1 : 0;
}

}  // namespace

extern "C" {

int d2r_sdfphys_create(d2r_ctx *ctx, const int32_t *b0, const uint32_t *nv, float voxel, const uint32_t *words, uint32_t n_static_grids,
                       const float *points, uint32_t n_points, d2r_sdfphys **out)
{
    if (!ctx || !b0 || !nv || !words || !points || !out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n_static_grids == 0) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_sdfphys_create: at least one static grid is needed");
    if (n_points == 0) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_sdfphys_create: the movable object has no points");
    if (!(voxel > 0.f) || !std::isfinite(voxel)) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_sdfphys_create: voxel must be > 0");
    SdfGrid G{};
    G.voxel = voxel;
    double nvox = 1.0;
    for (int a = 0; a < 3; ++a) {
        // the range test of a point's voxel is made on floats: first and one-past-last voxel must be exact there
        if (nv[a] == 0 || nv[a] > (1u << 20) || b0[a] < -(1 << 19) || b0[a] > (1 << 19))
            return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_sdfphys_create: nv must be 1 .. 2^20 per axis and |b0| at most 2^19 blocks");
        G.lo[a] = b0[a] * 16;
        G.nv[a] = nv[a];
        G.ncb[a] = (nv[a] + 15u) / 16u;
        nvox *= (double)nv[a];
    }
    if (nvox > (double)D2R_SDF_MAX_VOXELS) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_sdfphys_create: a grid of more than 2^31 voxels is refused");
    G.wpr = (G.nv[0] + 31u) / 32u;
    const size_t n_words = (size_t)G.nv[2] * G.nv[1] * G.wpr;
    const uint32_t n_blocks = G.ncb[0] * G.ncb[1] * G.ncb[2], n_cwords = (n_blocks + 31u) / 32u;
    // several static objects: the OR of their grids (lazy_phys_mods = False).  Bits past nx in a row's last word are dropped.
    std::vector<uint32_t> field(words, words + n_words);
    for (uint32_t g = 1; g < n_static_grids; ++g)
        for (size_t i = 0; i < n_words; ++i) field[i] |= words[(size_t)g * n_words + i];
    if (G.nv[0] & 31u) {
        const uint32_t keep = (1u << (G.nv[0] & 31u)) - 1u;
        for (size_t r = 0; r < (size_t)G.nv[2] * G.nv[1]; ++r) field[r * G.wpr + G.wpr - 1] &= keep;
    }
    std::vector<float> soa((size_t)n_points * 3);
    for (uint32_t i = 0; i < n_points; ++i)
        for (int a = 0; a < 3; ++a) soa[(size_t)a * n_points + i] = points[(size_t)i * 3 + a];
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<d2r_sdfphys> h(new (std::nothrow) d2r_sdfphys());
    if (!h) return d2r_fail(ctx, D2R_ERR_MEMORY, "out of host memory");
    h->ctx = ctx;
    h->device = ctx->device;
    h->G = G;
    h->n_points = n_points;
    D2rDrain drain{ctx->stream};      // field and soa (host memory of this call) have been consumed, whichever return is taken
    int rc;
    if ((rc = h->d_words.alloc(ctx, n_words * 4, "the physics field")) || (rc = h->d_coarse.alloc(ctx, (size_t)n_cwords * 4, "the physics field")) ||
        (rc = h->d_pts.alloc(ctx, soa.size() * 4, "the physics field")))
        return rc;
    D2R_HIP(ctx, hipMemcpyAsync(h->d_words.get(), field.data(), n_words * 4, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(h->d_pts.get(), soa.data(), soa.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_sdf_coarse, dim3((n_cwords + 3) / 4), dim3(SDF_THREADS), 0, ctx->stream, (const uint32_t *)h->d_words.get(), G, n_blocks,
                       n_cwords, h->d_coarse.get());
    D2R_HIP(ctx, hipGetLastError());
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out = h.release();
    return D2R_OK;
}

void d2r_sdfphys_destroy(d2r_sdfphys *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

int d2r_sdfphys_check(d2r_ctx *ctx, d2r_sdfphys *h, const d2r_phys_params *prm, const float *pose_batch, uint32_t N, uint8_t *valid_io)
{
    if (!ctx || !h || !prm || !pose_batch || !valid_io) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    uint64_t oris = 1;
    if (int rc = d2r_phys_orientations(ctx, prm, N, &oris)) return rc;
    SdfCheckParams P;
    // init_pose must be rigid to 1e-3 for its inverse to be [R^T | -R^T t]
    // (not d2r_is_rigid: that one holds to 1e-5 and a finite translation, and would refuse poses this call has always taken)
    const float *I = prm->init_pose;
    double dev = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += (double)I[k * 4 + i] * (double)I[k * 4 + j];
            dev = std::max(dev, fabs(d - (i == j ? 1.0 : 0.0)));
        }
    if (!(dev <= 1e-3) || I[12] != 0.f || I[13] != 0.f || I[14] != 0.f || I[15] != 1.f)
        return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_sdfphys_check: init_pose must be a rigid transform");
    d2r_rigid_inverse(I, P.inv);
    P.table_z = prm->table_z;
    for (int i = 0; i < 3; i++) P.drop[i] = prm->unsup_thresh * prm->gravity[i];
    P.perturb = prm->perturb;
    P.stability_check = prm->stability_check;
    P.oris_per_pos = (uint32_t)oris;
    const std::vector<uint8_t> mask = d2r_phys_orientation_mask(prm, pose_batch, valid_io, (uint32_t)oris);
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = d2r_reserve(ctx, ctx->poses, (size_t)N * 64))) return rc;
    if ((rc = d2r_reserve(ctx, ctx->pix, (size_t)N + oris + 64))) return rc;
    uint8_t *d_valid = (uint8_t *)ctx->pix.p, *d_mask = d_valid + ((N + 63) / 64) * 64;
    if ((rc = h->timer.mark(ctx, 0))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(ctx->poses.p, pose_batch, (size_t)N * 64, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(d_valid, valid_io, N, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(d_mask, mask.data(), oris, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = h->timer.mark(ctx, 1))) return rc;
    hipLaunchKernelGGL(k_sdf_check, dim3((N + 3) / 4), dim3(SDF_THREADS), 0, ctx->stream, P, h->G, (const float *)ctx->poses.p, N,
                       (const uint8_t *)d_mask, (const uint32_t *)h->d_words.get(), (const uint32_t *)h->d_coarse.get(), (const float *)h->d_pts.get(), h->n_points,
                       d_valid);
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = h->timer.mark(ctx, 2))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(valid_io, d_valid, N, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = h->timer.mark(ctx, 3))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h->timer.done();
    return D2R_OK;
}

int d2r_sdfphys_get_timing(d2r_ctx *ctx, const d2r_sdfphys *h, double *ms_out)
{
    if (!ctx || !h || !ms_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    return h->timer.read(ctx, ms_out, 3, "d2r_sdfphys_get_timing: no check has run on this handle");
}

}  // extern "C"
