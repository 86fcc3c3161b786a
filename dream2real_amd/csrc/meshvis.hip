// meshvis.hip — the picture of the cost volume and of the best pose (reference vision_3d/geometry_utils.py:137-206 vis_cost_volume,
// dream2real.py:392-400 draw_geometries; both open Open3D windows there).  A triangle rasteriser held to the written rule of
// DESIGN.md section 2f byte for byte: every step is integer arithmetic or one IEEE operation, nothing is contracted.
//   set-up      one thread per triangle: its item's matrix, the fp32 projection of section 2b, the snap to 1/16 pixel, the drops, the
//               winding, 1 / z' per vertex in fp64, the clipped pixel box, the flat shade byte; boxes of more than MV_LARGE_PX pixels
//               are queued for the workgroup launch
//   rasterise   one thread per triangle walks its box (small), one workgroup per queued triangle strides over its box (large):
//               int64 edge functions, top-left fill rule, q = 1 / z interpolated in fp64, rounded to fp32, a u64 atomic max on
//               (bits(q) << 32) | (0xFFFFFFFF - triangle)
//   cubes       the same two launches over 12 triangles a cube; a sample counts where its q is above the mesh buffer's, and the
//               reduction is a maximum over (score << 32) | (0xFFFFFFFF - cube): a maximum-intensity projection, order-free
//   resolve     item colour x shade byte, viridis5(score) blended over it, background elsewhere; the ids image
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "d2r_internal.h"

namespace {

constexpr uint32_t MV_THREADS = 256;
constexpr int32_t MV_LARGE_PX = 1024;        // a clipped box of more pixels than this goes to the workgroup launch
constexpr uint32_t MV_LARGE_BLOCKS = 1024;   // workgroups of that launch (they stride over the queue)
constexpr float MV_UV_LIMIT = 131072.f;      // 2^17: |X|, |Y| <= 2^21, edge products < 2^45, all exact in int64 and in fp64

struct MvMat { float m[12]; };               // rows 0..2 of inv(cam_pose) item_mat, row-major

struct MvCam {
    float fx, fy, cx, cy, near;
    int32_t W, H;
};

enum { MV_DROPPED = 0, MV_SMALL = 1, MV_LARGE = 2 };

struct MvTri {
    int32_t X[3], Y[3];                      // snapped vertices, 1/16 pixel, wound so that A > 0
    int32_t bx0, by0, bx1, by1;              // pixel box (inclusive) clipped to the frame
    int32_t kind, pad;
    double q[3];                             // 1 / z' per vertex
    long long A;                             // doubled area in snapped units
};

// DESIGN.md section 2b's arithmetic (fp32, this order, no contraction, correctly rounded divide), then section 2f's snap.
// -> false when the vertex drops its triangle.  cam[] receives the camera-space point either way.
__device__ __forceinline__ bool mv_vertex(const MvMat &M, float px, float py, float pz, const MvCam &c, int32_t &X, int32_t &Y, double &q,
                                          float *cam)
{
    const float *m = M.m;
    const float x = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
    const float y = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
    const float z = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
    cam[0] = x;
    cam[1] = y;
    cam[2] = z;
    if (!(z > c.near)) return false;
    const float u = (c.fx * x) / z + c.cx;
    const float v = (c.fy * y) / z + c.cy;
    if (!(fabsf(u) < MV_UV_LIMIT && fabsf(v) < MV_UV_LIMIT)) return false;     // NaN and the infinities fail too
    X = (int32_t)rintf(16.f * u);
    Y = (int32_t)rintf(16.f * v);
    q = 1.0 / (double)z;
    return true;
}

// three world-space vertices -> the triangle's record; shade (optional) receives the flat shade byte
__device__ __forceinline__ void mv_setup(const MvMat &M, const float (&p)[3][3], const MvCam &c, MvTri &T, uint8_t *shade)
{
    float cam[3][3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = mv_vertex(M, p[k][0], p[k][1], p[k][2], c, T.X[k], T.Y[k], T.q[k], cam[k]) && ok;
    if (shade) {
        // 0.35 + 0.65 |n_z| / |n| in fp64, n = (p1 - p0) x (p2 - p0) in the camera frame; byte = floor(255 s + 0.5)
        const double ax = (double)cam[1][0] - (double)cam[0][0], ay = (double)cam[1][1] - (double)cam[0][1], az = (double)cam[1][2] - (double)cam[0][2];
        const double bx = (double)cam[2][0] - (double)cam[0][0], by = (double)cam[2][1] - (double)cam[0][1], bz = (double)cam[2][2] - (double)cam[0][2];
        const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);
        double r = 0.0;
        if (len > 0.0 && len < INFINITY) r = fabs(nz) / len;
        const double s = 0.35 + 0.65 * r;
        *shade = (uint8_t)(int)floor(s * 255.0 + 0.5);
    }
    T.kind = MV_DROPPED;
    T.pad = 0;
    T.bx0 = T.by0 = 0;
    T.bx1 = T.by1 = -1;
    T.A = 0;
    if (!ok) return;
    long long A = (long long)(T.X[1] - T.X[0]) * (long long)(T.Y[2] - T.Y[0]) - (long long)(T.Y[1] - T.Y[0]) * (long long)(T.X[2] - T.X[0]);
    if (A == 0) return;
    if (A < 0) {                             // the winding is normalised: swap vertices 1 and 2
        const int32_t tx = T.X[1], ty = T.Y[1];
        const double tq = T.q[1];
        T.X[1] = T.X[2]; T.Y[1] = T.Y[2]; T.q[1] = T.q[2];
        T.X[2] = tx; T.Y[2] = ty; T.q[2] = tq;
        A = -A;
    }
    T.A = A;
    // pixel j is sampled at 16 j + 8: the columns with min X <= 16 j + 8 <= max X (arithmetic shifts floor)
    const int32_t xmin = min(T.X[0], min(T.X[1], T.X[2])), xmax = max(T.X[0], max(T.X[1], T.X[2]));
    const int32_t ymin = min(T.Y[0], min(T.Y[1], T.Y[2])), ymax = max(T.Y[0], max(T.Y[1], T.Y[2]));
    T.bx0 = max((xmin + 7) >> 4, 0);
    T.bx1 = min((xmax - 8) >> 4, c.W - 1);
    T.by0 = max((ymin + 7) >> 4, 0);
    T.by1 = min((ymax - 8) >> 4, c.H - 1);
    if (T.bx1 < T.bx0 || T.by1 < T.by0) return;
    T.kind = (T.bx1 - T.bx0 + 1) * (T.by1 - T.by0 + 1) > MV_LARGE_PX ? MV_LARGE : MV_SMALL;
}

__device__ __forceinline__ void mv_finish(MvTri &T, uint32_t t, MvTri *recs, uint32_t *large, uint32_t *n_large)
{
    recs[t] = T;
    if (T.kind == MV_LARGE) large[atomicAdd(n_large, 1u)] = t;
}

__global__ __launch_bounds__(MV_THREADS) void k_mv_setup_mesh(const float *__restrict__ verts, const uint32_t *__restrict__ tris,
                                                              const uint32_t *__restrict__ tri_item, uint32_t nt,
                                                              const MvMat *__restrict__ mats, MvCam c, MvTri *__restrict__ recs,
                                                              uint8_t *__restrict__ shade, uint32_t *__restrict__ large,
                                                              uint32_t *__restrict__ n_large)
{
    const uint32_t t = blockIdx.x * MV_THREADS + threadIdx.x;
    if (t >= nt) return;
    float p[3][3];
    for (int k = 0; k < 3; ++k) {
        const size_t v = tris[(size_t)t * 3 + k];
        p[k][0] = verts[v * 3];
        p[k][1] = verts[v * 3 + 1];
        p[k][2] = verts[v * 3 + 2];
    }
    MvTri T;
    mv_setup(mats[tri_item[t]], p, c, T, shade + t);
    mv_finish(T, t, recs, large, n_large);
}

// corner b of a cube: bit 0 -> x, bit 1 -> y, bit 2 -> z (set = centre + half, clear = centre - half); triangle f of a cube
__constant__ uint8_t MV_CUBE_TRIS[12][3] = {{0, 1, 3}, {0, 3, 2}, {4, 6, 7}, {4, 7, 5}, {0, 4, 5}, {0, 5, 1},
                                            {2, 3, 7}, {2, 7, 6}, {0, 2, 6}, {0, 6, 4}, {1, 5, 7}, {1, 7, 3}};

__global__ __launch_bounds__(MV_THREADS) void k_mv_setup_cubes(const float4 *__restrict__ cubes, const uint32_t *__restrict__ scores,
                                                               uint32_t n_tris, MvMat M, MvCam c, MvTri *__restrict__ recs,
                                                               uint32_t *__restrict__ large, uint32_t *__restrict__ n_large)
{
    const uint32_t t = blockIdx.x * MV_THREADS + threadIdx.x;
    if (t >= n_tris) return;
    const uint32_t k = t / 12u, f = t - k * 12u;
    const float4 cube = cubes[k];
    float p[3][3];
    for (int a = 0; a < 3; ++a) {
        const uint32_t b = MV_CUBE_TRIS[f][a];
        p[a][0] = (b & 1u) ? cube.x + cube.w : cube.x - cube.w;
        p[a][1] = (b & 2u) ? cube.y + cube.w : cube.y - cube.w;
        p[a][2] = (b & 4u) ? cube.z + cube.w : cube.z - cube.w;
    }
    MvTri T;
    mv_setup(M, p, c, T, nullptr);
    if (scores[k] == 0u) T.kind = MV_DROPPED;
    mv_finish(T, t, recs, large, n_large);
}

// the edge a -> b of a triangle with A > 0 (interior: E > 0) owns the centres on it when it is a top edge (horizontal, interior
// below: dy == 0, dx > 0) or a left edge (dy < 0).  -> 0 for such an edge, -1 otherwise: a centre is covered iff E + bias >= 0
__device__ __forceinline__ long long mv_bias(int32_t dx, int32_t dy)
{
    return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
}

struct MvEdges {
    long long sx[3], sy[3], bias[3];         // E_k's step per column and per row (16 snapped units each), the fill-rule bias
    long long e00[3];                        // E_k at the centre of pixel (0, 0)
};

__device__ __forceinline__ void mv_edges(const MvTri &T, MvEdges &E)
{
    // E_0 belongs to the edge 1 -> 2 (the weight of vertex 0), E_1 to 2 -> 0, E_2 to 0 -> 1:
    // E(P) = dx (Py - ay) - dy (Px - ax)
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const int32_t dx = T.X[b] - T.X[a], dy = T.Y[b] - T.Y[a];
        E.e00[k] = (long long)dx * (long long)(8 - T.Y[a]) - (long long)dy * (long long)(8 - T.X[a]);
        E.sx[k] = -16ll * dy;
        E.sy[k] = 16ll * dx;
        E.bias[k] = mv_bias(dx, dy);
    }
}

// one sample: w[] are the three edge values at the centre of pixel p
template <bool CUBE>
__device__ __forceinline__ void mv_sample(const MvTri &T, const MvEdges &E, long long w0, long long w1, long long w2, size_t p, uint32_t low,
                                          uint32_t score, unsigned long long *__restrict__ mesh_keys,
                                          unsigned long long *__restrict__ cube_keys)
{
    if (((w0 + E.bias[0]) | (w1 + E.bias[1]) | (w2 + E.bias[2])) < 0) return;
    const double num = ((double)w0 * T.q[0] + (double)w1 * T.q[1]) + (double)w2 * T.q[2];
    const float q = (float)(num / (double)T.A);
    if (!CUBE) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(q) << 32) | low;
        if (key > mesh_keys[p]) atomicMax(&mesh_keys[p], key);      // (the read only spares atomics: keys never decrease)
    } else {
        const float mq = __uint_as_float((uint32_t)(mesh_keys[p] >> 32));
        if (!(q > mq)) return;
        const unsigned long long key = ((unsigned long long)score << 32) | low;
        if (key > cube_keys[p]) atomicMax(&cube_keys[p], key);
    }
}

// low word of a triangle's key, and the cube's score
template <bool CUBE>
__device__ __forceinline__ void mv_owner(uint32_t t, const uint32_t *__restrict__ scores, uint32_t &low, uint32_t &score)
{
    if (CUBE) {
        const uint32_t k = t / 12u;
        low = 0xffffffffu - k;
        score = scores[k];
    } else {
        low = 0xffffffffu - t;
        score = 0;
    }
}

template <bool CUBE>
__global__ __launch_bounds__(MV_THREADS) void k_mv_raster_small(const MvTri *__restrict__ recs, uint32_t n_tris,
                                                                const uint32_t *__restrict__ scores, int32_t W,
                                                                unsigned long long *__restrict__ mesh_keys,
                                                                unsigned long long *__restrict__ cube_keys)
{
    const uint32_t t = blockIdx.x * MV_THREADS + threadIdx.x;
    if (t >= n_tris) return;
    if (recs[t].kind != MV_SMALL) return;
    const MvTri T = recs[t];
    MvEdges E;
    mv_edges(T, E);
    uint32_t low, score;
    mv_owner<CUBE>(t, scores, low, score);
    for (int32_t i = T.by0; i <= T.by1; ++i) {
        long long w0 = E.e00[0] + E.sy[0] * i + E.sx[0] * T.bx0;
        long long w1 = E.e00[1] + E.sy[1] * i + E.sx[1] * T.bx0;
        long long w2 = E.e00[2] + E.sy[2] * i + E.sx[2] * T.bx0;
        for (int32_t j = T.bx0; j <= T.bx1; ++j) {
            mv_sample<CUBE>(T, E, w0, w1, w2, (size_t)i * W + j, low, score, mesh_keys, cube_keys);
            w0 += E.sx[0];
            w1 += E.sx[1];
            w2 += E.sx[2];
        }
    }
}

template <bool CUBE>
__global__ __launch_bounds__(MV_THREADS) void k_mv_raster_large(const MvTri *__restrict__ recs, const uint32_t *__restrict__ large,
                                                                const uint32_t *__restrict__ n_large,
                                                                const uint32_t *__restrict__ scores, int32_t W,
                                                                unsigned long long *__restrict__ mesh_keys,
                                                                unsigned long long *__restrict__ cube_keys)
{
    const uint32_t n = *n_large;
    for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
        const uint32_t t = large[e];
        const MvTri T = recs[t];
        MvEdges E;
        mv_edges(T, E);
        uint32_t low, score;
        mv_owner<CUBE>(t, scores, low, score);
        const uint32_t bw = (uint32_t)(T.bx1 - T.bx0 + 1), npx = bw * (uint32_t)(T.by1 - T.by0 + 1);
        for (uint32_t s = threadIdx.x; s < npx; s += MV_THREADS) {
            const uint32_t r = s / bw;
            const int32_t i = T.by0 + (int32_t)r, j = T.bx0 + (int32_t)(s - r * bw);
            mv_sample<CUBE>(T, E, E.e00[0] + E.sy[0] * i + E.sx[0] * j, E.e00[1] + E.sy[1] * i + E.sx[1] * j,
                            E.e00[2] + E.sy[2] * i + E.sx[2] * j, (size_t)i * W + j, low, score, mesh_keys, cube_keys);
        }
    }
}

// viridis5: integer piecewise-linear interpolation between five stops over 0 .. 65535, rounded to nearest
__device__ __forceinline__ uint32_t mv_viridis5(uint32_t score, int ch)
{
    const uint8_t stops[5][3] = {{68, 1, 84}, {59, 82, 139}, {33, 145, 140}, {94, 201, 98}, {253, 231, 37}};
    const uint32_t t = score * 4u;
    const uint32_t seg = min(t / 65535u, 3u), f = t - seg * 65535u;
    return ((uint32_t)stops[seg][ch] * (65535u - f) + (uint32_t)stops[seg + 1][ch] * f + 32767u) / 65535u;
}

__global__ __launch_bounds__(MV_THREADS) void k_mv_resolve(const unsigned long long *__restrict__ mesh_keys,
                                                           const unsigned long long *__restrict__ cube_keys, uint32_t npx,
                                                           const uint32_t *__restrict__ tri_item, const uint32_t *__restrict__ item_rgb,
                                                           const uint8_t *__restrict__ shade, uint32_t bg, uint8_t *__restrict__ rgb,
                                                           int32_t *__restrict__ ids)
{
    const uint32_t p = blockIdx.x * MV_THREADS + threadIdx.x;
    if (p >= npx) return;
    const unsigned long long mk = mesh_keys[p], ck = cube_keys[p];
    uint32_t c[3] = {bg & 255u, (bg >> 8) & 255u, (bg >> 16) & 255u};
    int32_t id = INT32_MIN;
    if (mk) {
        const uint32_t t = 0xffffffffu - (uint32_t)mk;
        const uint32_t col = item_rgb[tri_item[t]], s = shade[t];
        for (int ch = 0; ch < 3; ++ch) c[ch] = (((col >> (8 * ch)) & 255u) * s + 127u) / 255u;
        id = (int32_t)t;
    }
    if (ck) {
        const uint32_t score = (uint32_t)(ck >> 32);
        for (int ch = 0; ch < 3; ++ch) c[ch] = (c[ch] * (65535u - score) + mv_viridis5(score, ch) * score + 32767u) / 65535u;
        id = -1 - (int32_t)(0xffffffffu - (uint32_t)ck);
    }
    rgb[(size_t)p * 3] = (uint8_t)c[0];
    rgb[(size_t)p * 3 + 1] = (uint8_t)c[1];
    rgb[(size_t)p * 3 + 2] = (uint8_t)c[2];
    ids[p] = id;
}

}  // namespace

extern "C" int d2r_mesh_render(d2r_ctx *ctx, const d2r_pcd_view *view, const float *cam_pose, const float *verts, uint32_t nv,
                               const uint32_t *tris, const uint32_t *tri_item, uint32_t nt, const float *item_mats,
                               const uint8_t *item_rgb, uint32_t n_items, const float *cube_centres, const float *cube_half,
                               const uint16_t *cube_scores, uint32_t K, const uint8_t *background, uint8_t *rgb_out, int32_t *ids_out)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (!cam_pose || !background || !rgb_out) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_mesh_render: null cam_pose, background or rgb_out");
    if ((nv && !verts) || (nt && (!tris || !tri_item)) || (n_items && (!item_mats || !item_rgb)) ||
        (K && (!cube_centres || !cube_half || !cube_scores)))
        return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_mesh_render: a null array with a non-zero count");
    int rc = d2r_pcd_check_view(ctx, view);
    if (rc) return rc;
    if (nt > 0x7ffffffeu || K > 0x7ffffffeu / 12u)
        return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_mesh_render: triangles and 12 x cubes must each stay below 2^31 - 1");
    for (size_t i = 0; i < (size_t)nt * 3; ++i)
        if (tris[i] >= nv) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_mesh_render: a triangle references a vertex out of range");
    for (size_t t = 0; t < nt; ++t)
        if (tri_item[t] >= n_items) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_mesh_render: a tri_item entry is not below n_items");
    D2R_HIP(ctx, hipSetDevice(ctx->device));

    const MvCam c{view->fx, view->fy, view->cx, view->cy, view->near, (int32_t)view->width, (int32_t)view->height};
    // matrices: inv(cam_pose) item_mat in fp64, rounded once; the cubes live in the world frame: inv(cam_pose) alone
    double Ci[16], P[16], T[16];
    d2r_rigid_inverse4(cam_pose, Ci);
    MvMat cam_mat;
    d2r_round34(Ci, cam_mat.m);
    std::vector<MvMat> mats(std::max<uint32_t>(n_items, 1));
    std::vector<uint32_t> cols(std::max<uint32_t>(n_items, 1), 0u);
    for (uint32_t k = 0; k < n_items; ++k) {
        d2r_load16(item_mats + (size_t)k * 16, P);
        d2r_mul4(Ci, P, T);
        d2r_round34(T, mats[k].m);
        cols[k] = d2r_pack_rgb(item_rgb + 3 * (size_t)k);
    }
    std::vector<float4> cubes(std::max<uint32_t>(K, 1), float4{0.f, 0.f, 0.f, 0.f});
    std::vector<uint32_t> scores(std::max<uint32_t>(K, 1), 0u);
    for (uint32_t k = 0; k < K; ++k) {
        cubes[k] = float4{cube_centres[3 * (size_t)k], cube_centres[3 * (size_t)k + 1], cube_centres[3 * (size_t)k + 2], cube_half[k]};
        scores[k] = cube_scores[k];
    }
    const uint32_t bg = d2r_pack_rgb(background);

    // workspaces (owned by the context, grown and never shrunk): the inputs, the records and the queue, the two key buffers, the outputs
    const size_t px = (size_t)c.W * c.H, nct = (size_t)K * 12, nrec = std::max<size_t>(std::max<size_t>(nt, nct), 1);
    D2rStage in(ctx, ctx->mv_in);
    const size_t o_verts = in.add((size_t)nv * 12), o_tris = in.add((size_t)nt * 12), o_item = in.add((size_t)nt * 4),
                 o_mats = in.add(mats.size() * sizeof(MvMat)), o_cols = in.add(cols.size() * 4), o_cubes = in.add(cubes.size() * sizeof(float4)),
                 o_scores = in.add(scores.size() * 4);
    if ((rc = in.reserve())) return rc;
    if ((rc = d2r_reserve(ctx, ctx->mv_recs, nrec * sizeof(MvTri)))) return rc;
    if ((rc = d2r_reserve(ctx, ctx->mv_queue, 256 + nrec * 4))) return rc;
    if ((rc = d2r_reserve(ctx, ctx->mv_shade, std::max<size_t>(nt, 1)))) return rc;
    if ((rc = d2r_reserve(ctx, ctx->mv_keys, px * 16))) return rc;
    if ((rc = d2r_reserve(ctx, ctx->mv_out, px * 4 + px * 3))) return rc;
    hipStream_t st = ctx->stream;
    if (nv && (rc = in.upload(o_verts, verts, (size_t)nv * 12))) return rc;
    if (nt && ((rc = in.upload(o_tris, tris, (size_t)nt * 12)) || (rc = in.upload(o_item, tri_item, (size_t)nt * 4)))) return rc;
    if ((rc = in.upload(o_mats, mats.data(), mats.size() * sizeof(MvMat))) || (rc = in.upload(o_cols, cols.data(), cols.size() * 4))) return rc;
    if ((rc = in.upload(o_cubes, cubes.data(), cubes.size() * sizeof(float4))) || (rc = in.upload(o_scores, scores.data(), scores.size() * 4))) return rc;
    unsigned long long *mesh_keys = (unsigned long long *)ctx->mv_keys.p, *cube_keys = mesh_keys + px;
    D2R_HIP(ctx, hipMemsetAsync(mesh_keys, 0, px * 16, st));
    MvTri *recs = (MvTri *)ctx->mv_recs.p;
    uint32_t *n_large = (uint32_t *)ctx->mv_queue.p, *large = n_large + 64;
    const uint32_t *d_scores = in.at<const uint32_t>(o_scores);
    if (nt) {
        const dim3 grid((nt + MV_THREADS - 1) / MV_THREADS), block(MV_THREADS);
        D2R_HIP(ctx, hipMemsetAsync(n_large, 0, 4, st));
        hipLaunchKernelGGL(k_mv_setup_mesh, grid, block, 0, st, in.at<const float>(o_verts), in.at<const uint32_t>(o_tris),
                           in.at<const uint32_t>(o_item), nt, in.at<const MvMat>(o_mats), c, recs, (uint8_t *)ctx->mv_shade.p, large, n_large);
        hipLaunchKernelGGL(k_mv_raster_small<false>, grid, block, 0, st, (const MvTri *)recs, nt, d_scores, c.W, mesh_keys, cube_keys);
        hipLaunchKernelGGL(k_mv_raster_large<false>, dim3(MV_LARGE_BLOCKS), block, 0, st, (const MvTri *)recs, (const uint32_t *)large,
                           (const uint32_t *)n_large, d_scores, c.W, mesh_keys, cube_keys);
    }
    if (K) {
        const uint32_t n = (uint32_t)nct;
        const dim3 grid((n + MV_THREADS - 1) / MV_THREADS), block(MV_THREADS);
        D2R_HIP(ctx, hipMemsetAsync(n_large, 0, 4, st));
        hipLaunchKernelGGL(k_mv_setup_cubes, grid, block, 0, st, in.at<const float4>(o_cubes), d_scores, n, cam_mat, c, recs, large, n_large);
        hipLaunchKernelGGL(k_mv_raster_small<true>, grid, block, 0, st, (const MvTri *)recs, n, d_scores, c.W, mesh_keys, cube_keys);
        hipLaunchKernelGGL(k_mv_raster_large<true>, dim3(MV_LARGE_BLOCKS), block, 0, st, (const MvTri *)recs, (const uint32_t *)large,
                           (const uint32_t *)n_large, d_scores, c.W, mesh_keys, cube_keys);
    }
    int32_t *d_ids = (int32_t *)ctx->mv_out.p;
    uint8_t *d_rgb = (uint8_t *)(d_ids + px);
    hipLaunchKernelGGL(k_mv_resolve, dim3((uint32_t)((px + MV_THREADS - 1) / MV_THREADS)), dim3(MV_THREADS), 0, st,
                       (const unsigned long long *)mesh_keys, (const unsigned long long *)cube_keys, (uint32_t)px,
                       in.at<const uint32_t>(o_item), in.at<const uint32_t>(o_cols), (const uint8_t *)ctx->mv_shade.p, bg, d_rgb, d_ids);
    D2R_HIP(ctx, hipGetLastError());
    D2R_HIP(ctx, hipMemcpyAsync(rgb_out, d_rgb, px * 3, hipMemcpyDeviceToHost, st));
    if (ids_out) D2R_HIP(ctx, hipMemcpyAsync(ids_out, d_ids, px * 4, hipMemcpyDeviceToHost, st));
    D2R_HIP(ctx, hipStreamSynchronize(st));
    return D2R_OK;
}
