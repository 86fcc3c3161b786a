// tsdf.hip — TSDF fusion of masked RGB-D frames and surface extraction: the GPU side of get_phys_models' TSDF branch
// (reference vision_3d/physics_utils.py:58-115, Open3D's VoxelBlockGrid on the CPU).  The rule is DESIGN.md section 2c,
// restated in numpy by tests/tsdf_ref.py and held to it bit for bit.
//
// Storage is DENSE over scene_bounds padded by the truncation distance and rounded out to whole 16^3 blocks: voxel state
// (tsdf, weight) as float2 [nz][ny][nx], one stamp and one "ever active" byte per block.  The mesh is cropped to the bounds
// anyway, a 2 mm grid over a table-top scene (1 m x 1 m x 0.5 m) is 0.5 GB of state, and the device has 288 GB: no hash
// map, no allocation while frames arrive, neighbours of a cube are an index away.  Volumes over D2R_TSDF_MAX_VOXELS are
// refused.
//   k_erode        mask eroded by a k x k rectangle (separable minimum over an LDS tile), depth -> metres, invalid -> 0
//   k_mark_blocks  one lane per valid pixel walks its ray over [z - trunc, z + trunc] in voxel steps and stamps the blocks
//   k_integrate    one workgroup per block stamped this frame, lanes along x: the running average, frame by frame
//   k_fuse_rgb     the same body with colour (d2r_tsdf_integrate_rgb): three fp32 channels averaged at
//                  exactly the voxels the frame updates; k_tsdf_colours gathers them for the parity hook
//   k_mc_*         classify cubes, mark crossed edges, scan counts in (z, y, x) order, emit vertices, emit triangles
//   k_tsdf_touch_bits / k_tsdf_solid_*   the volume as the point-against-field physics backend reads it (DESIGN.md section 2e,
//                  sdfphys.hip): one "touch" bit per voxel, and the centres of the observed solid voxels in (z, y, x) order
// Every value is written by ordinary vector stores from C++.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "d2r_internal.h"
#include "mc_table.h"
#include "meshio.h"

#define D2R_TSDF_MAX_VOXELS (1ull << 31)     // 16 GiB of (tsdf, weight) + 6 B per voxel of extraction scratch
#define D2R_TSDF_BLOCK 16
#define D2R_TSDF_BLOCK_VOX 4096
#define D2R_TSDF_MAX_ERODE 32

struct TsdfGrid {
    int32_t b0[3];          // first block per axis, in global block coordinates (block b holds voxels 16 b .. 16 b + 15)
    uint32_t nb[3];         // blocks per axis
    uint32_t nv[3];         // voxels per axis
    float voxel, trunc;
};

struct TsdfCam {
    float fx, fy, cx, cy;
    int32_t W, H;
    float m[12];            // cam_pose, rows 0..2
    float inv[12];          // inv(cam_pose), rows 0..2: [R^T | -R^T t] composed in fp64, rounded to fp32
};

struct d2r_tsdf {
    d2r_ctx *ctx = nullptr;
    int device = 0;
    TsdfGrid G{};
    uint64_t n_vox = 0;
    uint32_t n_blocks = 0;
    D2rDev<float2> vox;             // [nz][ny][nx] (tsdf, weight)
    D2rDev<uint32_t> stamp;         // [n_blocks] 1 + index of the last frame that touched the block
    D2rDev<uint8_t> ever;           // [n_blocks]
    D2rDev<uint32_t> list;          // [n_blocks] blocks of the current frame (order does not matter: voxels are independent)
    D2rDev<uint32_t> counters;      // [0] length of list, [1] valid pixels of the frame, [2..3] vertex / triangle totals, [4] solid voxels
    uint32_t frame = 0;
    d2r_ctx::Buf depth_in, mask_in, zbuf;
    // colour (d2r_tsdf_integrate_rgb): allocated by the first rgb frame
    D2rDev<float> col;              // [nz][ny][nx][3]
    enum { FRAMES_NONE, FRAMES_PLAIN, FRAMES_RGB } frames = FRAMES_NONE;   // which of the two calls feeds this volume
    d2r_ctx::Buf rgb_in;
    // the touched-block box of d2r_tsdf_dev, as of frame box_frame
    uint32_t box_frame = 0xffffffffu;
    int32_t box_lo[3] = {}, box_hi[3] = {};
    ~d2r_tsdf()
    {
        for (void *p : {depth_in.p, mask_in.p, zbuf.p, rgb_in.p})
            if (p) (void)hipFree(p);
    }
    // the last extraction, kept for the fill call
    bool have = false;
    float key[9] = {};
    D2rMesh mesh;
};

namespace {

constexpr uint32_t TSDF_THREADS = D2R_SCAN_THREADS;
constexpr int ER_TW = 64, ER_TH = 32;        // output tile of k_erode
constexpr uint32_t MC_CHUNK = 4096;          // voxels per scan chunk: 256 threads x 16

__device__ const int8_t MC_TRI[256][16] = {D2R_MC_TABLE_ROWS};
// edge e of the cube at voxel v is the edge of voxel v + MC_EDGE_OFF[e] along axis MC_EDGE_AXIS[e] (0 x, 1 y, 2 z)
__device__ const uint8_t MC_EDGE_OFF[12][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 0}, {0, 0, 1}, {1, 0, 1},
                                               {0, 1, 1}, {0, 0, 1}, {0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}};
__device__ const uint8_t MC_EDGE_AXIS[12] = {0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2};

// ------------------------------------------------------------------------------------------------ frames in

// zbuf[i][j] = depth in metres where the eroded mask holds and 0 < z <= depth_max, else 0.  Erosion by a k x k rectangle of
// ones anchored at (k/2, k/2): rows i - k/2 .. i - k/2 + k - 1, columns likewise; outside the frame counts as set.
__global__ __launch_bounds__(TSDF_THREADS) void k_erode(const uint16_t *__restrict__ depth, const uint8_t *__restrict__ mask, int W, int H,
                                                        int k, float depth_max, float *__restrict__ zbuf, uint32_t *__restrict__ counters)
{
    __shared__ uint8_t m0[ER_TH + D2R_TSDF_MAX_ERODE - 1][ER_TW + D2R_TSDF_MAX_ERODE];
    __shared__ uint8_t m1[ER_TH + D2R_TSDF_MAX_ERODE - 1][ER_TW];
    const int t = (int)threadIdx.x, a = k / 2;
    const int tx0 = (int)blockIdx.x * ER_TW, ty0 = (int)blockIdx.y * ER_TH;
    const int rows = ER_TH + k - 1, cols = ER_TW + k - 1;
    for (int q = t; q < rows * cols; q += (int)TSDF_THREADS) {
        const int r = q / cols, c = q - r * cols;
        const int gi = ty0 + r - a, gj = tx0 + c - a;
        uint8_t v = 1;
        if (gi >= 0 && gi < H && gj >= 0 && gj < W) v = mask[(size_t)gi * W + gj] != 0;
        m0[r][c] = v;
    }
    __syncthreads();
    for (int q = t; q < rows * ER_TW; q += (int)TSDF_THREADS) {
        const int r = q / ER_TW, c = q - r * ER_TW;
        uint8_t v = 1;
        for (int d = 0; d < k; ++d) v &= m0[r][c + d];
        m1[r][c] = v;
    }
    __syncthreads();
    for (int q = t; q < ER_TH * ER_TW; q += (int)TSDF_THREADS) {
        const int r = q / ER_TW, c = q - r * ER_TW;
        const int i = ty0 + r, j = tx0 + c;
        float z = 0.f;
        if (i < H && j < W) {
            uint8_t v = 1;
            for (int d = 0; d < k; ++d) v &= m1[r + d][c];
            const float zz = (float)depth[(size_t)i * W + j] / 1000.0f;
            if (v && zz > 0.f && zz <= depth_max) z = zz;
            zbuf[(size_t)i * W + j] = z;
        }
        const unsigned long long any = __ballot(z > 0.f);
        if ((t & 63) == 0 && any) atomicAdd(&counters[1], (uint32_t)__popcll(any));
    }
}

// one lane per pixel: the blocks its ray crosses within the truncation band join the frame's list
__global__ __launch_bounds__(TSDF_THREADS) void k_mark_blocks(const float *__restrict__ zbuf, TsdfCam c, TsdfGrid G, int steps, uint32_t cur,
                                                              uint32_t *__restrict__ stamp, uint8_t *__restrict__ ever,
                                                              uint32_t *__restrict__ list, uint32_t *__restrict__ counters)
{
    const uint32_t p = blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (p >= (uint32_t)c.W * (uint32_t)c.H) return;
    const float z = zbuf[p];
    if (!(z > 0.f)) return;
    const int i = (int)(p / (uint32_t)c.W), j = (int)(p - (uint32_t)i * (uint32_t)c.W);
    const float xn = ((float)j - c.cx) / c.fx, yn = ((float)i - c.cy) / c.fy;
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = (float)(G.b0[a] * D2R_TSDF_BLOCK);
        hi[a] = (float)((G.b0[a] + (int32_t)G.nb[a]) * D2R_TSDF_BLOCK);
    }
    uint32_t last = 0xffffffffu;
    for (int s = 0; s <= 2 * steps; ++s) {
        const float d = (z - G.trunc) + (float)s * G.voxel;
        const float x = xn * d, y = yn * d;
        const float X = ((c.m[0] * x + c.m[1] * y) + c.m[2] * d) + c.m[3];
        const float Y = ((c.m[4] * x + c.m[5] * y) + c.m[6] * d) + c.m[7];
        const float Z = ((c.m[8] * x + c.m[9] * y) + c.m[10] * d) + c.m[11];
        const float gx = floorf(X / G.voxel), gy = floorf(Y / G.voxel), gz = floorf(Z / G.voxel);
        if (!(gx >= lo[0] && gx < hi[0] && gy >= lo[1] && gy < hi[1] && gz >= lo[2] && gz < hi[2])) continue;   // NaN fails too
        const uint32_t bx = (uint32_t)(((int)gx >> 4) - G.b0[0]), by = (uint32_t)(((int)gy >> 4) - G.b0[1]),
                       bz = (uint32_t)(((int)gz >> 4) - G.b0[2]);
        const uint32_t b = (bz * G.nb[1] + by) * G.nb[0] + bx;
        if (b == last) continue;
        last = b;
        if (stamp[b] != cur && atomicExch(&stamp[b], cur) != cur) {      // exactly one lane per block and frame gets here
            ever[b] = 1;
            list[atomicAdd(&counters[0], 1u)] = b;
        }
    }
}

// the running average of one frame over the blocks it stamped.  256 threads = one z-slice of a block: x = t & 15 along the
// lanes (neighbouring voxels read neighbouring pixels), y = t >> 4; a wave's 64 voxels are four 128-byte rows of state.
// RGB: the voxels whose tsdf is updated also average the pixel's colour, with the weight from before the increment
// (DESIGN.md section 2i); one launch per frame, so the average is order-exact without atomics.
template <bool RGB>
__device__ __forceinline__ void integrate_blocks(const float *__restrict__ zbuf, const TsdfCam &c, const TsdfGrid &G,
                                                 const uint32_t *__restrict__ list, const uint32_t *__restrict__ counters,
                                                 float2 *__restrict__ vox, const uint8_t *__restrict__ rgb, float *__restrict__ col)
{
    const uint32_t n = counters[0];
    const uint32_t x = threadIdx.x & 15u, y = threadIdx.x >> 4;
    for (uint32_t l = blockIdx.x; l < n; l += gridDim.x) {
        const uint32_t b = list[l];
        const uint32_t bx = b % G.nb[0], by = (b / G.nb[0]) % G.nb[1], bz = b / (G.nb[0] * G.nb[1]);
        const uint32_t lx = bx * D2R_TSDF_BLOCK + x, ly = by * D2R_TSDF_BLOCK + y;
        const float px = (float)(G.b0[0] * D2R_TSDF_BLOCK + (int32_t)(bx * D2R_TSDF_BLOCK + x)) * G.voxel;
        const float py = (float)(G.b0[1] * D2R_TSDF_BLOCK + (int32_t)(by * D2R_TSDF_BLOCK + y)) * G.voxel;
        for (uint32_t zz = 0; zz < D2R_TSDF_BLOCK; ++zz) {
            const uint32_t lz = bz * D2R_TSDF_BLOCK + zz;
            const float pz = (float)(G.b0[2] * D2R_TSDF_BLOCK + (int32_t)lz) * G.voxel;
            const float xc = ((c.inv[0] * px + c.inv[1] * py) + c.inv[2] * pz) + c.inv[3];
            const float yc = ((c.inv[4] * px + c.inv[5] * py) + c.inv[6] * pz) + c.inv[7];
            const float zc = ((c.inv[8] * px + c.inv[9] * py) + c.inv[10] * pz) + c.inv[11];
            if (!(zc > 0.f)) continue;
            const float u = floorf(((c.fx * xc) / zc + c.cx) + 0.5f);
            const float v = floorf(((c.fy * yc) / zc + c.cy) + 0.5f);
            if (!(u >= 0.f && u < (float)c.W && v >= 0.f && v < (float)c.H)) continue;
            const float zp = zbuf[(size_t)(int)v * c.W + (int)u];
            if (!(zp > 0.f)) continue;
            const float sdf = zp - zc;
            if (sdf < -G.trunc) continue;
            const float tt = fminf(sdf / G.trunc, 1.0f);
            float2 *s = vox + ((size_t)lz * G.nv[1] + ly) * G.nv[0] + lx;
            float2 sv = *s;
            if (RGB) {
                const uint8_t *pix = rgb + ((size_t)(int)v * c.W + (int)u) * 3;
                float *cv = col + (((size_t)lz * G.nv[1] + ly) * G.nv[0] + lx) * 3;
                for (int ch = 0; ch < 3; ++ch) cv[ch] = (sv.y * cv[ch] + (float)pix[ch]) / (sv.y + 1.0f);
            }
            sv.x = (sv.y * sv.x + tt) / (sv.y + 1.0f);
            sv.y = sv.y + 1.0f;
            *s = sv;
        }
    }
}

__global__ __launch_bounds__(TSDF_THREADS) void k_integrate(const float *__restrict__ zbuf, TsdfCam c, TsdfGrid G,
                                                            const uint32_t *__restrict__ list, const uint32_t *__restrict__ counters,
                                                            float2 *__restrict__ vox)
{
    integrate_blocks<false>(zbuf, c, G, list, counters, vox, nullptr, nullptr);
}

__global__ __launch_bounds__(TSDF_THREADS) void k_fuse_rgb(const float *__restrict__ zbuf, const uint8_t *__restrict__ rgb, TsdfCam c, TsdfGrid G,
                                                           const uint32_t *__restrict__ list, const uint32_t *__restrict__ counters,
                                                           float2 *__restrict__ vox, float *__restrict__ col)
{
    integrate_blocks<true>(zbuf, c, G, list, counters, vox, rgb, col);
}

// parity hook: the colours of the listed blocks, [n][16][16][16][3] in (z, y, x, channel) order
__global__ __launch_bounds__(TSDF_THREADS) void k_tsdf_colours(const float *__restrict__ col, TsdfGrid G, const uint32_t *__restrict__ blocks,
                                                                  float *__restrict__ out)
{
    const uint32_t b = blocks[blockIdx.x];
    const uint32_t bx = b % G.nb[0], by = (b / G.nb[0]) % G.nb[1], bz = b / (G.nb[0] * G.nb[1]);
    for (uint32_t q = threadIdx.x; q < D2R_TSDF_BLOCK_VOX * 3; q += TSDF_THREADS) {
        const uint32_t vx = q / 3u, ch = q - vx * 3u;
        const uint32_t x = vx & 15u, y = (vx >> 4) & 15u, z = vx >> 8;
        out[(size_t)blockIdx.x * D2R_TSDF_BLOCK_VOX * 3 + q] =
            col[(((size_t)(bz * D2R_TSDF_BLOCK + z) * G.nv[1] + by * D2R_TSDF_BLOCK + y) * G.nv[0] + bx * D2R_TSDF_BLOCK + x) * 3 + ch];
    }
}

// parity hook: the voxels of the listed blocks, [n][16][16][16] in (z, y, x) order
__global__ __launch_bounds__(TSDF_THREADS) void k_tsdf_gather(const float2 *__restrict__ vox, TsdfGrid G, const uint32_t *__restrict__ blocks,
                                                              float *__restrict__ tsdf, float *__restrict__ weight)
{
    const uint32_t b = blocks[blockIdx.x];
    const uint32_t bx = b % G.nb[0], by = (b / G.nb[0]) % G.nb[1], bz = b / (G.nb[0] * G.nb[1]);
    for (uint32_t q = threadIdx.x; q < D2R_TSDF_BLOCK_VOX; q += TSDF_THREADS) {
        const uint32_t x = q & 15u, y = (q >> 4) & 15u, z = q >> 8;
        const float2 s = vox[((size_t)(bz * D2R_TSDF_BLOCK + z) * G.nv[1] + by * D2R_TSDF_BLOCK + y) * G.nv[0] + bx * D2R_TSDF_BLOCK + x];
        tsdf[(size_t)blockIdx.x * D2R_TSDF_BLOCK_VOX + q] = s.x;
        weight[(size_t)blockIdx.x * D2R_TSDF_BLOCK_VOX + q] = s.y;
    }
}

// ------------------------------------------------------------------------------------------------ marching cubes

__device__ __forceinline__ void mc_xyz(uint64_t i, const TsdfGrid &G, uint32_t &x, uint32_t &y, uint32_t &z)
{
    x = (uint32_t)(i % G.nv[0]);
    const uint64_t r = i / G.nv[0];
    y = (uint32_t)(r % G.nv[1]);
    z = (uint32_t)(r / G.nv[1]);
}

__device__ __forceinline__ bool mc_block_ever(const uint8_t *ever, const TsdfGrid &G, uint32_t x, uint32_t y, uint32_t z)
{
    return ever[((z >> 4) * G.nb[1] + (y >> 4)) * G.nb[0] + (x >> 4)] != 0;
}

// cubecase[v] = the table row of the cube whose lowest corner is voxel v: 0 when a corner has weight < thr, the cube leaves
// the grid, or no triangle comes of it (rows 0 and 255)
__global__ __launch_bounds__(TSDF_THREADS) void k_mc_classify(const float2 *__restrict__ vox, const uint8_t *__restrict__ ever, TsdfGrid G,
                                                              uint64_t n_vox, float thr, uint8_t *__restrict__ cubecase)
{
    const uint64_t i = (uint64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (i >= n_vox) return;
    uint32_t x, y, z;
    mc_xyz(i, G, x, y, z);
    uint32_t idx = 0;
    if (x + 1 < G.nv[0] && y + 1 < G.nv[1] && z + 1 < G.nv[2] && mc_block_ever(ever, G, x, y, z)) {
        const size_t sx = 1, sy = G.nv[0], sz = (size_t)G.nv[0] * G.nv[1];
        const size_t off[8] = {0, sx, sx + sy, sy, sz, sz + sx, sz + sx + sy, sz + sy};
        bool ok = true;
        for (int k = 0; k < 8; ++k) {
            const float2 s = vox[i + off[k]];
            ok = ok && s.y >= thr;
            idx |= (s.x < 0.f ? 1u : 0u) << k;
        }
        if (!ok || idx == 255u) idx = 0;
    }
    cubecase[i] = (uint8_t)idx;
}

// ebits[v]: bit a = the edge from voxel v along axis a carries a vertex (its ends differ in sign and one of the four cubes
// around it is kept); bits 3..5 = triangles of the cube at v
__global__ __launch_bounds__(TSDF_THREADS) void k_mc_edges(const float2 *__restrict__ vox, const uint8_t *__restrict__ ever,
                                                           const uint8_t *__restrict__ cubecase, TsdfGrid G, uint64_t n_vox,
                                                           uint8_t *__restrict__ ebits)
{
    const uint64_t i = (uint64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (i >= n_vox) return;
    uint32_t x, y, z;
    mc_xyz(i, G, x, y, z);
    uint32_t bits = 0;
    if (mc_block_ever(ever, G, x, y, z)) {
        const uint32_t p[3] = {x, y, z};
        const size_t st[3] = {1, G.nv[0], (size_t)G.nv[0] * G.nv[1]};
        const float t0 = vox[i].x;
        for (int a = 0; a < 3; ++a) {
            if (p[a] + 1 >= G.nv[a]) continue;
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            bool kept = false;
            for (int db = 0; db < 2; ++db)
                for (int dc = 0; dc < 2; ++dc) {
                    if ((db && p[b] == 0) || (dc && p[c] == 0)) continue;
                    kept = kept || cubecase[i - db * st[b] - dc * st[c]] != 0;
                }
            if (!kept) continue;
            const float t1 = vox[i + st[a]].x;
            if ((t0 < 0.f) != (t1 < 0.f)) bits |= 1u << a;
        }
        const int8_t *row = MC_TRI[cubecase[i]];
        uint32_t nt = 0;
        while (nt < 5 && row[3 * nt] >= 0) ++nt;
        bits |= nt << 3;
    }
    ebits[i] = (uint8_t)bits;
}

__device__ __forceinline__ uint2 mc_counts16(const uint8_t *ebits, uint64_t first)
{
    const uint4 w = *reinterpret_cast<const uint4 *>(ebits + first);
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
    uint2 s = make_uint2(0, 0);
    for (int k = 0; k < 4; ++k) {
        s.x += (uint32_t)__popc(ws[k] & 0x07070707u);
        const uint32_t t = (ws[k] >> 3) & 0x07070707u;
        s.y += (t & 255u) + ((t >> 8) & 255u) + ((t >> 16) & 255u) + (t >> 24);
    }
    return s;
}

// (vertices, triangles) of each 4096-voxel chunk; the grid is whole blocks, so chunks are whole
__global__ __launch_bounds__(TSDF_THREADS) void k_mc_chunk_sums(const uint8_t *__restrict__ ebits, uint2 *__restrict__ chunk)
{
    const uint2 sum = d2r_block_sum(mc_counts16(ebits, (uint64_t)blockIdx.x * MC_CHUNK + threadIdx.x * 16u));
    if (threadIdx.x == 0) chunk[blockIdx.x] = sum;
}

// exclusive scan of the chunk sums in place (one workgroup); totals to counters[2..3]
__global__ __launch_bounds__(TSDF_THREADS) void k_mc_scan_chunks(uint2 *__restrict__ chunk, uint32_t nchunks, uint32_t *__restrict__ counters)
{
    const uint2 total = d2r_block_scan_row(chunk, chunk, nchunks);
    if (threadIdx.x == 0) {
        counters[2] = total.x;
        counters[3] = total.y;
    }
}

// TRIS = false: vbase[v] and the vertices of voxel v's edges, in (z, y, x, axis) order.  TRIS = true: the triangles of the
// cube at v, in (z, y, x, table) order, as indices into that vertex array.
template <bool TRIS>
__global__ __launch_bounds__(TSDF_THREADS) void k_mc_emit(const float2 *__restrict__ vox, const uint8_t *__restrict__ cubecase,
                                                          const uint8_t *__restrict__ ebits, const uint2 *__restrict__ chunk, TsdfGrid G,
                                                          uint32_t *__restrict__ vbase, float *__restrict__ verts, uint32_t n_verts,
                                                          uint32_t *__restrict__ tris, uint32_t n_tris)
{
    const uint64_t first = (uint64_t)blockIdx.x * MC_CHUNK + threadIdx.x * 16u;
    const uint2 both = mc_counts16(ebits, first);
    const uint32_t mine = TRIS ? both.y : both.x;
    uint32_t run = d2r_block_scan(mine, TRIS ? chunk[blockIdx.x].y : chunk[blockIdx.x].x);
    if (mine == 0) return;
    const size_t st[3] = {1, G.nv[0], (size_t)G.nv[0] * G.nv[1]};
    for (uint32_t k = 0; k < 16; ++k) {
        const uint64_t i = first + k;
        const uint32_t bits = ebits[i];
        if (!TRIS) {
            if (!(bits & 7u)) continue;
            vbase[i] = run;
            uint32_t p[3];
            mc_xyz(i, G, p[0], p[1], p[2]);
            float q[3];
            for (int a = 0; a < 3; ++a) q[a] = (float)(G.b0[a] * D2R_TSDF_BLOCK + (int32_t)p[a]) * G.voxel;
            const float t0 = vox[i].x;
            for (int a = 0; a < 3; ++a) {
                if (!(bits >> a & 1u)) continue;
                const float t1 = vox[i + st[a]].x;
                const float q1 = (float)(G.b0[a] * D2R_TSDF_BLOCK + (int32_t)p[a] + 1) * G.voxel;
                float o[3] = {q[0], q[1], q[2]};
                o[a] = q[a] + ((q1 - q[a]) * t0) / (t0 - t1);
                if (run < n_verts) {
                    verts[(size_t)run * 3 + 0] = o[0];
                    verts[(size_t)run * 3 + 1] = o[1];
                    verts[(size_t)run * 3 + 2] = o[2];
                }
                ++run;
            }
        } else {
            const uint32_t nt = bits >> 3;
            if (!nt) continue;
            const int8_t *row = MC_TRI[cubecase[i]];
            for (uint32_t t = 0; t < nt; ++t) {
                for (int c = 0; c < 3; ++c) {
                    const int e = row[3 * t + c];
                    const uint64_t j = i + MC_EDGE_OFF[e][0] * st[0] + MC_EDGE_OFF[e][1] * st[1] + MC_EDGE_OFF[e][2] * st[2];
                    const uint32_t a = MC_EDGE_AXIS[e];
                    const uint32_t vi = vbase[j] + (uint32_t)__popc(ebits[j] & ((1u << a) - 1u));
                    if (run < n_tris) tris[(size_t)run * 3 + c] = vi;
                }
                ++run;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ field and points (section 2e)

// touch[g] = w >= thr && tsdf * trunc <= contact, packed along x: bit x & 31 of word x >> 5, rows of wpr = ceil(nx / 32) words.
// One wave per 64 voxels of a row: its ballot is two words (the second only where the row still has one).
__global__ __launch_bounds__(TSDF_THREADS) void k_tsdf_touch_bits(const float2 *__restrict__ vox, TsdfGrid G, uint32_t wpr, uint32_t segs,
                                                                  uint64_t n_waves, float thr, float contact, uint32_t *__restrict__ words)
{
    const uint64_t wave = (uint64_t)blockIdx.x * (TSDF_THREADS / 64) + (threadIdx.x >> 6);
    if (wave >= n_waves) return;                                    // whole waves leave: the ballot below sees all 64 lanes
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t row = wave / segs;                               // z * ny + y
    const uint32_t seg = (uint32_t)(wave - row * segs), x = seg * 64u + lane;
    bool t = false;
    if (x < G.nv[0]) {
        const float2 s = vox[row * G.nv[0] + x];
        t = s.y >= thr && s.x * G.trunc <= contact;
    }
    const unsigned long long b = __ballot(t);
    if (lane == 0) words[row * wpr + 2u * seg] = (uint32_t)b;
    if (lane == 32 && 2u * seg + 1u < wpr) words[row * wpr + 2u * seg + 1u] = (uint32_t)(b >> 32);
}

// solid voxels (w >= thr && tsdf <= 0) of a 4096-voxel chunk: thread t looks at voxels s * 256 + t, s = 0 .. 15 (a wave reads
// 64 neighbours per step); bit s of the result
__device__ __forceinline__ uint32_t solid_mask16(const float2 *__restrict__ vox, uint64_t first, float thr)
{
    uint32_t m = 0;
#pragma unroll
    for (uint32_t s = 0; s < 16; ++s) {
        const float2 v = vox[first + s * TSDF_THREADS + threadIdx.x];
        m |= (v.y >= thr && v.x <= 0.f ? 1u : 0u) << s;
    }
    return m;
}

__global__ __launch_bounds__(TSDF_THREADS) void k_tsdf_solid_count(const float2 *__restrict__ vox, float thr, uint32_t *__restrict__ chunk)
{
    const uint32_t sum = d2r_block_sum((uint32_t)__popc(solid_mask16(vox, (uint64_t)blockIdx.x * MC_CHUNK, thr)));
    if (threadIdx.x == 0) chunk[blockIdx.x] = sum;
}

// exclusive scan of the chunk counts in place (one workgroup); the total to counters[4]
__global__ __launch_bounds__(TSDF_THREADS) void k_tsdf_solid_scan(uint32_t *__restrict__ chunk, uint32_t nchunks, uint32_t *__restrict__ counters)
{
    const uint32_t total = d2r_block_scan_row(chunk, chunk, nchunks);
    if (threadIdx.x == 0) counters[4] = total;
}

// the centres (float)g * voxel of the solid voxels, in voxel order: a chunk's 16 steps x 4 waves are 64 runs of 64 voxels
__global__ __launch_bounds__(TSDF_THREADS) void k_tsdf_solid_emit(const float2 *__restrict__ vox, const uint32_t *__restrict__ chunk, TsdfGrid G,
                                                                  float thr, float *__restrict__ xyz, uint32_t n_points)
{
    __shared__ uint32_t runs[16 * (TSDF_THREADS / 64)];
    const uint64_t first = (uint64_t)blockIdx.x * MC_CHUNK;
    const uint32_t mine = solid_mask16(vox, first, thr);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t s = 0; s < 16; ++s) {
        const unsigned long long b = __ballot((mine >> s) & 1u);
        if (lane == 0) runs[s * (TSDF_THREADS / 64) + wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = chunk[blockIdx.x];
        for (uint32_t i = 0; i < 16 * (TSDF_THREADS / 64); i++) {
            const uint32_t v = runs[i];
            runs[i] = run;
            run += v;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t s = 0; s < 16; ++s) {
        const unsigned long long b = __ballot((mine >> s) & 1u);
        const uint32_t at = runs[s * (TSDF_THREADS / 64) + wave] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (((mine >> s) & 1u) && at < n_points) {
            uint32_t px, py, pz;
            mc_xyz(first + s * TSDF_THREADS + threadIdx.x, G, px, py, pz);
            xyz[(size_t)at * 3 + 0] = (float)(G.b0[0] * D2R_TSDF_BLOCK + (int32_t)px) * G.voxel;
            xyz[(size_t)at * 3 + 1] = (float)(G.b0[1] * D2R_TSDF_BLOCK + (int32_t)py) * G.voxel;
            xyz[(size_t)at * 3 + 2] = (float)(G.b0[2] * D2R_TSDF_BLOCK + (int32_t)pz) * G.voxel;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side

int tsdf_fail(d2r_tsdf *v, int code, const std::string &msg) { return d2r_fail(v ? v->ctx : nullptr, code, msg); }

constexpr const char *TSDF_MEM = "a TSDF volume";

// the whole extraction on the device: raw vertices and triangles in canonical order to the host
int tsdf_extract_raw(d2r_tsdf *v, float thr, std::vector<float> &verts, std::vector<uint32_t> &tris)
{
    d2r_ctx *ctx = v->ctx;
    const uint64_t n = v->n_vox;
    const uint32_t nchunks = (uint32_t)(n / MC_CHUNK), nblk = (uint32_t)((n + TSDF_THREADS - 1) / TSDF_THREADS);
    D2rDev<uint8_t> cubecase, ebits;
    D2rDev<uint32_t> vbase, d_tris;
    D2rDev<uint2> chunk;
    D2rDev<float> d_verts;
    D2rDrain drain{ctx->stream};
    int r;
    if ((r = cubecase.alloc(ctx, n, TSDF_MEM)) || (r = ebits.alloc(ctx, n, TSDF_MEM)) || (r = vbase.alloc(ctx, n * 4, TSDF_MEM)) ||
        (r = chunk.alloc(ctx, (size_t)nchunks * 8, TSDF_MEM)))
        return r;
    hipLaunchKernelGGL(k_mc_classify, dim3(nblk), dim3(TSDF_THREADS), 0, ctx->stream, v->vox.get(), v->ever.get(), v->G, n, thr, cubecase.get());
    hipLaunchKernelGGL(k_mc_edges, dim3(nblk), dim3(TSDF_THREADS), 0, ctx->stream, v->vox.get(), v->ever.get(), cubecase.get(), v->G, n, ebits.get());
    hipLaunchKernelGGL(k_mc_chunk_sums, dim3(nchunks), dim3(TSDF_THREADS), 0, ctx->stream, ebits.get(), chunk.get());
    hipLaunchKernelGGL(k_mc_scan_chunks, dim3(1), dim3(TSDF_THREADS), 0, ctx->stream, chunk.get(), nchunks, v->counters.get());
    D2R_HIP(ctx, hipGetLastError());
    uint32_t tot[2] = {0, 0};
    D2R_HIP(ctx, hipMemcpyAsync(tot, v->counters.get() + 2, 8, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if ((uint64_t)tot[0] * 3 >= 0xffffffffull || (uint64_t)tot[1] * 3 >= 0xffffffffull)
        return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "TSDF surface has too many vertices for 32-bit indices");
    verts.resize((size_t)tot[0] * 3);
    tris.resize((size_t)tot[1] * 3);
    if (tot[0] == 0 || tot[1] == 0) {
        verts.clear();
        tris.clear();
        return D2R_OK;
    }
    if ((r = d_verts.alloc(ctx, verts.size() * 4, TSDF_MEM)) || (r = d_tris.alloc(ctx, tris.size() * 4, TSDF_MEM))) return r;
    hipLaunchKernelGGL(k_mc_emit<false>, dim3(nchunks), dim3(TSDF_THREADS), 0, ctx->stream, v->vox.get(), cubecase.get(), ebits.get(), chunk.get(), v->G,
                       vbase.get(), d_verts.get(), tot[0], d_tris.get(), tot[1]);
    hipLaunchKernelGGL(k_mc_emit<true>, dim3(nchunks), dim3(TSDF_THREADS), 0, ctx->stream, v->vox.get(), cubecase.get(), ebits.get(), chunk.get(), v->G,
                       vbase.get(), d_verts.get(), tot[0], d_tris.get(), tot[1]);
    D2R_HIP(ctx, hipGetLastError());
    D2R_HIP(ctx, hipMemcpyAsync(verts.data(), d_verts.get(), verts.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(tris.data(), d_tris.get(), tris.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return D2R_OK;
}

}  // namespace

extern "C" {

int d2r_tsdf_create(d2r_ctx *ctx, const float *bounds, float voxel, float trunc, d2r_tsdf **out)
{
    if (!ctx || !bounds || !out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!(voxel > 0.f) || !std::isfinite(voxel) || !(trunc >= voxel) || !std::isfinite(trunc))
        return d2r_fail(ctx, D2R_ERR_INVALID, "TSDF volume: voxel must be > 0 and trunc >= voxel");
    TsdfGrid G{};
    G.voxel = voxel;
    G.trunc = trunc;
    const double bs = (double)D2R_TSDF_BLOCK * (double)voxel;
    double nvox = 1.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = (double)bounds[a], hi = (double)bounds[3 + a];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi))
            return d2r_fail(ctx, D2R_ERR_INVALID, "TSDF volume: bounds must be finite with min < max on every axis");
        const double b0 = floor((lo - (double)trunc) / bs), b1 = floor((hi + (double)trunc) / bs);
        if (fabs(b0) > 1048576.0 || fabs(b1) > 1048576.0 || b1 - b0 + 1.0 > 65536.0)
            return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "TSDF volume: bounds are too far from the origin or too wide for this voxel size");
        G.b0[a] = (int32_t)b0;
        G.nb[a] = (uint32_t)(b1 - b0 + 1.0);
        G.nv[a] = G.nb[a] * D2R_TSDF_BLOCK;
        nvox *= (double)G.nv[a];
    }
    if (nvox > (double)D2R_TSDF_MAX_VOXELS) {
        char msg[320];
        snprintf(msg, sizeof msg,
                 "TSDF volume over the cap: scene_bounds padded by the truncation distance span %u x %u x %u voxels of %g m (%.1f GiB of "
                 "voxel state); the dense volume is capped at 2^31 voxels (16 GiB): shrink scene_bounds",
                 G.nv[0], G.nv[1], G.nv[2], (double)voxel, nvox * 8.0 / 1073741824.0);
        return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, msg);
    }
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<d2r_tsdf> v(new d2r_tsdf);
    v->ctx = ctx;
    v->device = ctx->device;
    v->G = G;
    v->n_vox = (uint64_t)G.nv[0] * G.nv[1] * G.nv[2];
    v->n_blocks = G.nb[0] * G.nb[1] * G.nb[2];
    int rc;
    if ((rc = v->vox.alloc(ctx, v->n_vox * sizeof(float2), TSDF_MEM, true)) || (rc = v->stamp.alloc(ctx, (size_t)v->n_blocks * 4, TSDF_MEM, true)) ||
        (rc = v->ever.alloc(ctx, v->n_blocks, TSDF_MEM, true)) || (rc = v->list.alloc(ctx, (size_t)v->n_blocks * 4, TSDF_MEM, true)) ||
        (rc = v->counters.alloc(ctx, 64, TSDF_MEM, true)))
        return rc;
    *out = v.release();
    return D2R_OK;
}

void d2r_tsdf_destroy(d2r_tsdf *v)
{
    if (!v) return;
    (void)hipSetDevice(v->device);
    delete v;
}

// one frame through either call: rgb_u8 == nullptr is d2r_tsdf_integrate
static int tsdf_integrate(d2r_tsdf *v, const uint16_t *depth_u16, const uint8_t *mask_u8, const uint8_t *rgb_u8, uint32_t w, uint32_t h,
                          const float *intrinsics, const float *cam_pose, uint32_t erode_k)
{
    d2r_ctx *ctx = v->ctx;
    if (w == 0 || h == 0 || w > 16384 || h > 16384) return d2r_fail(ctx, D2R_ERR_INVALID, "TSDF frame: width and height must be 1 .. 16384");
    if (erode_k < 1 || erode_k > D2R_TSDF_MAX_ERODE) return d2r_fail(ctx, D2R_ERR_INVALID, "TSDF frame: erode_k must be 1 .. 32");
    if (int rc = d2r_check_cam(ctx, "TSDF frame", intrinsics, cam_pose, 0)) return rc;
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(cam_pose[i])) return d2r_fail(ctx, D2R_ERR_INVALID, "TSDF frame: cam_pose must be finite");
    if (v->frame == 0xfffffffeu) return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "TSDF volume: too many frames");
    if (v->frames != d2r_tsdf::FRAMES_NONE && (v->frames == d2r_tsdf::FRAMES_RGB) != (rgb_u8 != nullptr))
        return d2r_fail(ctx, D2R_ERR_INVALID,
                        "TSDF volume: a frame through d2r_tsdf_integrate_rgb after d2r_tsdf_integrate (or the other way round) mixes the two "
                        "calls on one volume; its colours would average over fewer frames than its weights count");
    D2R_HIP(ctx, hipSetDevice(v->device));
    if (rgb_u8 && !v->col.get()) {
        if ((double)v->n_vox * 20.0 > (double)D2R_TSDF_MAX_VOXELS * 8.0) {
            char msg[320];
            snprintf(msg, sizeof msg,
                     "TSDF volume over the cap: %u x %u x %u voxels with colour are %.1f GiB of voxel state (20 bytes a voxel); the dense "
                     "volume is capped at 16 GiB: shrink scene_bounds",
                     v->G.nv[0], v->G.nv[1], v->G.nv[2], (double)v->n_vox * 20.0 / 1073741824.0);
            return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, msg);
        }
        if (int rc = v->col.alloc(ctx, v->n_vox * 12, TSDF_MEM, true)) return rc;
    }
    v->frames = rgb_u8 ? d2r_tsdf::FRAMES_RGB : d2r_tsdf::FRAMES_PLAIN;
    TsdfCam c{};
    c.fx = intrinsics[0];
    c.fy = intrinsics[4];
    c.cx = intrinsics[2];
    c.cy = intrinsics[5];
    c.W = (int32_t)w;
    c.H = (int32_t)h;
    memcpy(c.m, cam_pose, sizeof c.m);
    double inv[12];
    d2r_rigid_inverse(cam_pose, inv);
    for (int i = 0; i < 12; ++i) c.inv[i] = (float)inv[i];
    const size_t px = (size_t)w * h;
    int rc;
    if ((rc = d2r_reserve(ctx, v->depth_in, px * 2)) || (rc = d2r_reserve(ctx, v->mask_in, px)) || (rc = d2r_reserve(ctx, v->zbuf, px * 4))) return rc;
    if (rgb_u8) {
        if ((rc = d2r_reserve(ctx, v->rgb_in, px * 3))) return rc;
        D2R_HIP(ctx, hipMemcpyAsync(v->rgb_in.p, rgb_u8, px * 3, hipMemcpyHostToDevice, ctx->stream));
    }
    D2R_HIP(ctx, hipMemcpyAsync(v->depth_in.p, depth_u16, px * 2, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(v->mask_in.p, mask_u8, px, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipMemsetAsync(v->counters.get(), 0, 8, ctx->stream));
    const uint32_t cur = ++v->frame;
    const int steps = (int)lrint((double)v->G.trunc / (double)v->G.voxel);
    hipLaunchKernelGGL(k_erode, dim3((w + ER_TW - 1) / ER_TW, (h + ER_TH - 1) / ER_TH), dim3(TSDF_THREADS), 0, ctx->stream,
                       (const uint16_t *)v->depth_in.p, (const uint8_t *)v->mask_in.p, (int)w, (int)h, (int)erode_k, 3.0f, (float *)v->zbuf.p,
                       v->counters.get());
    hipLaunchKernelGGL(k_mark_blocks, dim3((uint32_t)((px + TSDF_THREADS - 1) / TSDF_THREADS)), dim3(TSDF_THREADS), 0, ctx->stream,
                       (const float *)v->zbuf.p, c, v->G, steps, cur, v->stamp.get(), v->ever.get(), v->list.get(), v->counters.get());
    const uint32_t grid = std::min<uint32_t>(v->n_blocks, (uint32_t)ctx->n_cu * 16u);
    if (rgb_u8)
        hipLaunchKernelGGL(k_fuse_rgb, dim3(grid), dim3(TSDF_THREADS), 0, ctx->stream, (const float *)v->zbuf.p, (const uint8_t *)v->rgb_in.p, c, v->G,
                           v->list.get(), v->counters.get(), v->vox.get(), v->col.get());
    else
        hipLaunchKernelGGL(k_integrate, dim3(grid), dim3(TSDF_THREADS), 0, ctx->stream, (const float *)v->zbuf.p, c, v->G, v->list.get(), v->counters.get(), v->vox.get());
    D2R_HIP(ctx, hipGetLastError());
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the caller's frame (pageable host memory) has been consumed
    v->have = false;
    return D2R_OK;
}

int d2r_tsdf_integrate(d2r_tsdf *v, const uint16_t *depth_u16, const uint8_t *mask_u8, uint32_t w, uint32_t h, const float *intrinsics,
                       const float *cam_pose, uint32_t erode_k)
{
    if (!v || !depth_u16 || !mask_u8 || !intrinsics || !cam_pose) return tsdf_fail(v, D2R_ERR_INVALID, "null argument");
    return tsdf_integrate(v, depth_u16, mask_u8, nullptr, w, h, intrinsics, cam_pose, erode_k);
}

int d2r_tsdf_integrate_rgb(d2r_tsdf *v, const uint16_t *depth_u16, const uint8_t *mask_u8, const uint8_t *rgb_u8, uint32_t w, uint32_t h,
                           const float *intrinsics, const float *cam_pose, uint32_t erode_k)
{
    if (!v || !depth_u16 || !mask_u8 || !rgb_u8 || !intrinsics || !cam_pose) return tsdf_fail(v, D2R_ERR_INVALID, "null argument");
    return tsdf_integrate(v, depth_u16, mask_u8, rgb_u8, w, h, intrinsics, cam_pose, erode_k);
}

int d2r_tsdf_read_colours(d2r_tsdf *v, uint32_t *n_blocks, float *colours)
{
    if (!v || !n_blocks) return tsdf_fail(v, D2R_ERR_INVALID, "null argument");
    d2r_ctx *ctx = v->ctx;
    if (!v->col.get())
        return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_tsdf_read_colours: the volume holds no colour (no frame came through d2r_tsdf_integrate_rgb)");
    D2R_HIP(ctx, hipSetDevice(v->device));
    std::vector<uint8_t> ever(v->n_blocks);
    D2R_HIP(ctx, hipMemcpyAsync(ever.data(), v->ever.get(), v->n_blocks, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint32_t> blocks;
    for (uint32_t b = 0; b < v->n_blocks; ++b)
        if (ever[b]) blocks.push_back(b);
    const uint32_t cap = *n_blocks;
    *n_blocks = (uint32_t)blocks.size();
    if (!colours || blocks.empty()) return D2R_OK;
    if (cap < blocks.size()) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_tsdf_read_colours: the buffer holds fewer blocks than are active");
    D2rDev<uint32_t> d_blocks;
    D2rDev<float> d_c;
    D2rDrain drain{ctx->stream};
    const size_t nb = blocks.size(), bytes = nb * D2R_TSDF_BLOCK_VOX * 12;
    int rc;
    if ((rc = d_blocks.alloc(ctx, nb * 4, TSDF_MEM)) || (rc = d_c.alloc(ctx, bytes, TSDF_MEM))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(d_blocks.get(), blocks.data(), nb * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_tsdf_colours, dim3((uint32_t)nb), dim3(TSDF_THREADS), 0, ctx->stream, v->col.get(), v->G, d_blocks.get(), d_c.get());
    D2R_HIP(ctx, hipGetLastError());
    D2R_HIP(ctx, hipMemcpyAsync(colours, d_c.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return D2R_OK;
}

int d2r_tsdf_read_voxels(d2r_tsdf *v, uint32_t *n_blocks, int32_t *block_coords, float *tsdf, float *weight)
{
    if (!v || !n_blocks) return tsdf_fail(v, D2R_ERR_INVALID, "null argument");
    d2r_ctx *ctx = v->ctx;
    D2R_HIP(ctx, hipSetDevice(v->device));
    std::vector<uint8_t> ever(v->n_blocks);
    D2R_HIP(ctx, hipMemcpyAsync(ever.data(), v->ever.get(), v->n_blocks, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint32_t> blocks;
    for (uint32_t b = 0; b < v->n_blocks; ++b)
        if (ever[b]) blocks.push_back(b);
    const uint32_t cap = *n_blocks;
    *n_blocks = (uint32_t)blocks.size();
    if (!block_coords && !tsdf && !weight) return D2R_OK;
    if (!block_coords || !tsdf || !weight) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_tsdf_read_voxels: give all three buffers or none");
    if (cap < blocks.size()) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_tsdf_read_voxels: buffers hold fewer blocks than are active");
    if (blocks.empty()) return D2R_OK;
    const TsdfGrid &G = v->G;
    for (size_t k = 0; k < blocks.size(); ++k) {
        const uint32_t b = blocks[k];
        block_coords[3 * k + 0] = G.b0[0] + (int32_t)(b % G.nb[0]);
        block_coords[3 * k + 1] = G.b0[1] + (int32_t)((b / G.nb[0]) % G.nb[1]);
        block_coords[3 * k + 2] = G.b0[2] + (int32_t)(b / (G.nb[0] * G.nb[1]));
    }
    D2rDev<uint32_t> d_blocks;
    D2rDev<float> d_t, d_w;
    D2rDrain drain{ctx->stream};
    const size_t nb = blocks.size(), bytes = nb * D2R_TSDF_BLOCK_VOX * 4;
    int rc;
    if ((rc = d_blocks.alloc(ctx, nb * 4, TSDF_MEM)) || (rc = d_t.alloc(ctx, bytes, TSDF_MEM)) || (rc = d_w.alloc(ctx, bytes, TSDF_MEM))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(d_blocks.get(), blocks.data(), nb * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_tsdf_gather, dim3((uint32_t)nb), dim3(TSDF_THREADS), 0, ctx->stream, v->vox.get(), G, d_blocks.get(), d_t.get(), d_w.get());
    D2R_HIP(ctx, hipGetLastError());
    D2R_HIP(ctx, hipMemcpyAsync(tsdf, d_t.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(weight, d_w.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return D2R_OK;
}

int d2r_tsdf_extract(d2r_tsdf *v, float weight_threshold, const float *crop, double cluster_keep, uint32_t *n_vertices, uint32_t *n_triangles,
                     float *vertices, uint32_t *triangles, int32_t *clusters, uint8_t *keep, double *centre)
{
    if (!v || !n_vertices || !n_triangles) return tsdf_fail(v, D2R_ERR_INVALID, "null argument");
    d2r_ctx *ctx = v->ctx;
    if (!(weight_threshold > 0.f) || !std::isfinite(weight_threshold))
        return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_tsdf_extract: weight_threshold must be > 0");
    if (!(cluster_keep >= 0.0 && cluster_keep <= 1.0)) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_tsdf_extract: cluster_keep must be 0 .. 1");
    float key[9] = {weight_threshold, (float)cluster_keep, crop ? 1.f : 0.f, 0, 0, 0, 0, 0, 0};
    if (crop) memcpy(key + 3, crop, 24);
    if (!v->have || memcmp(key, v->key, sizeof key) != 0) {
        D2R_HIP(ctx, hipSetDevice(v->device));
        std::vector<float> rv;
        std::vector<uint32_t> rt;
        int rc = tsdf_extract_raw(v, weight_threshold, rv, rt);
        if (rc) return rc;
        if (rt.empty())
            return d2r_fail(ctx, D2R_ERR_INVALID,
                            "TSDF volume holds no surface: the object was seen in no frame (no voxel reached the weight threshold inside a "
                            "sign change)");
        d2r_mesh_clean(rv.data(), rv.size() / 3, rt.data(), rt.size() / 3, crop, cluster_keep, v->mesh);
        if (v->mesh.tris.empty())
            return d2r_fail(ctx, D2R_ERR_INVALID, "TSDF surface lies wholly outside the crop box: no triangle survives");
        memcpy(v->key, key, sizeof key);
        v->have = true;
    }
    const D2rMesh &m = v->mesh;
    const uint32_t cap_v = *n_vertices, cap_t = *n_triangles;
    *n_vertices = (uint32_t)(m.verts.size() / 3);
    *n_triangles = (uint32_t)(m.tris.size() / 3);
    if (!vertices && !triangles && !clusters && !keep && !centre) return D2R_OK;
    if (cap_v < *n_vertices || cap_t < *n_triangles) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_tsdf_extract: buffers smaller than the mesh");
    if (vertices) memcpy(vertices, m.verts.data(), m.verts.size() * 4);
    if (triangles) memcpy(triangles, m.tris.data(), m.tris.size() * 4);
    if (clusters) memcpy(clusters, m.label.data(), m.label.size() * 4);
    if (keep) memcpy(keep, m.keep.data(), m.keep.size());
    if (centre) memcpy(centre, m.centre, 24);
    return D2R_OK;
}

int d2r_tsdf_grid(const d2r_tsdf *v, int32_t *b0, uint32_t *nv, float *voxel, float *trunc)
{
    if (!v || !b0 || !nv || !voxel || !trunc) return d2r_fail(v ? v->ctx : nullptr, D2R_ERR_INVALID, "null argument");
    for (int a = 0; a < 3; ++a) {
        b0[a] = v->G.b0[a];
        nv[a] = v->G.nv[a];
    }
    *voxel = v->G.voxel;
    *trunc = v->G.trunc;
    return D2R_OK;
}

int d2r_tsdf_touch_bits(d2r_tsdf *v, float weight_threshold, float contact, uint32_t *words_out)
{
    if (!v || !words_out) return tsdf_fail(v, D2R_ERR_INVALID, "null argument");
    d2r_ctx *ctx = v->ctx;
    if (!(weight_threshold > 0.f) || !std::isfinite(weight_threshold) || !std::isfinite(contact))
        return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_tsdf_touch_bits: weight_threshold must be > 0 and contact finite");
    D2R_HIP(ctx, hipSetDevice(v->device));
    const TsdfGrid &G = v->G;
    const uint32_t wpr = (G.nv[0] + 31u) / 32u, segs = (G.nv[0] + 63u) / 64u;
    const uint64_t rows = (uint64_t)G.nv[1] * G.nv[2], n_waves = rows * segs;
    const size_t bytes = (size_t)rows * wpr * 4;
    D2rDev<uint32_t> d_words;
    D2rDrain drain{ctx->stream};
    if (int rc = d_words.alloc(ctx, bytes, TSDF_MEM)) return rc;
    hipLaunchKernelGGL(k_tsdf_touch_bits, dim3((uint32_t)((n_waves + 3) / 4)), dim3(TSDF_THREADS), 0, ctx->stream, v->vox.get(), G, wpr, segs, n_waves,
                       weight_threshold, contact, d_words.get());
    D2R_HIP(ctx, hipGetLastError());
    D2R_HIP(ctx, hipMemcpyAsync(words_out, d_words.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return D2R_OK;
}

int d2r_tsdf_solid_points(d2r_tsdf *v, float weight_threshold, uint32_t *n_points, float *xyz)
{
    if (!v || !n_points) return tsdf_fail(v, D2R_ERR_INVALID, "null argument");
    d2r_ctx *ctx = v->ctx;
    if (!(weight_threshold > 0.f) || !std::isfinite(weight_threshold))
        return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_tsdf_solid_points: weight_threshold must be > 0");
    D2R_HIP(ctx, hipSetDevice(v->device));
    const uint32_t nchunks = (uint32_t)(v->n_vox / MC_CHUNK), cap = *n_points;
    D2rDev<uint32_t> chunk;
    D2rDev<float> d_xyz;
    D2rDrain drain{ctx->stream};
    int r;
    if ((r = chunk.alloc(ctx, (size_t)nchunks * 4, TSDF_MEM))) return r;
    hipLaunchKernelGGL(k_tsdf_solid_count, dim3(nchunks), dim3(TSDF_THREADS), 0, ctx->stream, v->vox.get(), weight_threshold, chunk.get());
    hipLaunchKernelGGL(k_tsdf_solid_scan, dim3(1), dim3(TSDF_THREADS), 0, ctx->stream, chunk.get(), nchunks, v->counters.get());
    D2R_HIP(ctx, hipGetLastError());
    uint32_t tot = 0;
    D2R_HIP(ctx, hipMemcpyAsync(&tot, v->counters.get() + 4, 4, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_points = tot;
    if (tot == 0)
        return d2r_fail(ctx, D2R_ERR_INVALID,
                        "TSDF volume holds no solid voxel: the object was seen in no frame (no voxel reached the weight threshold with "
                        "tsdf <= 0)");
    if (!xyz) return D2R_OK;
    if (cap < tot) return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_tsdf_solid_points: buffer smaller than the point set");
    if ((r = d_xyz.alloc(ctx, (size_t)tot * 12, TSDF_MEM))) return r;
    hipLaunchKernelGGL(k_tsdf_solid_emit, dim3(nchunks), dim3(TSDF_THREADS), 0, ctx->stream, v->vox.get(), chunk.get(), v->G, weight_threshold,
                       d_xyz.get(), tot);
    D2R_HIP(ctx, hipGetLastError());
    D2R_HIP(ctx, hipMemcpyAsync(xyz, d_xyz.get(), (size_t)tot * 12, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return D2R_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ the volume as its readers see it

bool d2r_tsdf_has_colour(const d2r_tsdf *v) { return v->col.get() != nullptr; }
int d2r_tsdf_device(const d2r_tsdf *v) { return v->device; }
float d2r_tsdf_voxel(const d2r_tsdf *v) { return v->G.voxel; }

int d2r_tsdf_dev(d2r_ctx *ctx, d2r_tsdf *v, D2rTsdfDev *out)
{
    const TsdfGrid &G = v->G;
    if (v->box_frame != v->frame) {
        std::vector<uint8_t> ever(v->n_blocks);
        D2R_HIP(ctx, hipMemcpyAsync(ever.data(), v->ever.get(), v->n_blocks, hipMemcpyDeviceToHost, ctx->stream));
        D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
        int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
        for (uint32_t b = 0; b < v->n_blocks; ++b) {
            if (!ever[b]) continue;
            const int32_t q[3] = {(int32_t)(b % G.nb[0]), (int32_t)((b / G.nb[0]) % G.nb[1]), (int32_t)(b / (G.nb[0] * G.nb[1]))};
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], q[a]);
                hi[a] = std::max(hi[a], q[a]);
            }
        }
        for (int a = 0; a < 3; ++a) {
            const bool none = lo[a] > hi[a];
            v->box_lo[a] = none ? 0 : (G.b0[a] + lo[a]) * D2R_TSDF_BLOCK;
            v->box_hi[a] = none ? -1 : (G.b0[a] + hi[a]) * D2R_TSDF_BLOCK + D2R_TSDF_BLOCK - 1;
        }
        v->box_frame = v->frame;
    }
    out->vox = (const TsVoxel *)v->vox.get();
    out->col = v->col.get();
    out->ever = v->ever.get();
    for (int a = 0; a < 3; ++a) {
        out->lo[a] = G.b0[a] * D2R_TSDF_BLOCK;
        out->nv[a] = G.nv[a];
        out->nb[a] = G.nb[a];
        out->box_lo[a] = v->box_lo[a];
        out->box_hi[a] = v->box_hi[a];
    }
    out->voxel = G.voxel;
    out->trunc = G.trunc;
    out->cells_of_box();
    return D2R_OK;
}
