// masks.hip — the mask geometry in front of build_scene_model: scene-bound masks from depth (reference data_loader.py:71-122,
// Open3D + two 50 x 50 cv2 morphology passes per frame on the CPU) and the connected-component pruning of label images
// (reference segmentation/XMem_infer.py:264-351, one cv2.connectedComponents per label per frame).  The rule is DESIGN.md
// section 2d, restated in numpy by tests/masks_ref.py and held to it bit for bit.
//   k_scene_bounds   one lane per pixel in fp64, the raw mask bit-packed: 64 pixels per uint64 through __ballot
//   k_morph          (masks_shared.h) dilation / erosion by a k x k rectangle on the packed words: log2(k) shift-and-OR (AND) steps along a row,
//                    the same doubling over the rows of an LDS tile of words
//   k_label_tiles    (masks_shared.h, over ByteSrc, as the next two) union-find over raster indices inside a 64 x 16 tile in LDS
//   k_label_seams    unions across tile borders, lock-free: find both roots, atomicMin the larger root's parent
//   k_label_flatten  every pixel points at its root = the smallest raster index of its component = the component's order key
//   k_comp_stats     area and (n, sum d, sum j d, sum i d) at the root's index: integer atomics, equal roots combined per wave
//                    (wave_each_root, masks_shared.h)
//   k_select_*       per label: component count, best distance (bit pattern of a non-negative double) or area, tie rule
//   k_prune_write    the pruned label image with the out-of-scene overwrite
//   k_mask_lut       out = lut[mask] | (oob != 0), optionally alpha = 255 (1 - out)
//   k_census         pixels per label per frame: one 256-bin LDS histogram per wave, 16 pixels per load, equal neighbours of a lane
//                    merged into one LDS add, the workgroup's bins flushed with integer atomics to the frame's row
// and the object thumbnails for captioning (reference caption.py:62-130; the rule is DESIGN.md section 2g, restated by tests/thumbs_ref.py):
//   k_thumb_init / k_thumb_obj_stats   area and bounding box of every label of every visited frame in one pass over the label images:
//                    four pixels per lane, equal neighbours merged, LDS integer atomics, non-empty slots flushed with integer atomics
//   k_thumb_complement   the 0 / 1 image of ~obj on frame 0 per object; the labelling above runs on it
//   k_thumb_comp_stats / k_thumb_container   pixels of label 0 and border pixels per component at its root, then the flag per object
//   k_thumb_pack     ~obj (or any 0 / 1 image) bit-packed, one wave per word
//   k_thumb_blur_rows / k_thumb_blur_cols   the separable 201-tap integer blur: bits -> u16 row sums -> the blur bit, packed again, in
//                    the rotated frame's layout where the frame is rotated; k_morph<false> dilates it
//   k_thumb_compose  every accepted thumbnail into one packed buffer: rotation, white or noise fill, crop
// The one-wave-per-word kernels (k_scene_bounds, k_thumb_pack) index and pack through d2r_word_lane / word_pack, single bits are read
// through plane_bit, the frames of a pass come from pass_items: all in masks_shared.h.
// Every value is written by ordinary vector stores from C++.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "d2r_internal.h"
#include "masks_shared.h"

namespace {

constexpr uint32_t CS_ITERS = 8, CS_SEGS = MK_THREADS * CS_ITERS;   // k_census: 16-byte segments per lane, per workgroup (32 KiB of pixels)
constexpr size_t MK_WS_BUDGET = (size_t)1 << 30;         // labelling workspace per pass of frames (D2R_MASKS_WS_BYTES overrides it)

struct MaskCam {
    double fx, fy, cx, cy;
};
struct MaskBox {
    double lo[3], hi[3];
};
struct MaskCentre {
    double c[3];
};
// per-root statistics: n, sum d, sum j d, sum i d over the pixels with d16 > 0 as uint64, then the area in the low half of word 4
constexpr int ST_WORDS = 5;

// ------------------------------------------------------------------------------------------------ scene bounds

__global__ __launch_bounds__(MK_THREADS) void k_scene_bounds(const uint16_t *__restrict__ depth, const float *__restrict__ poses, MaskCam c, MaskBox b,
                                                             int W, int H, int WW, unsigned long long *__restrict__ bits)
{
    const uint32_t f = blockIdx.y;
    WordLane p;
    if (!d2r_word_lane(H, WW, p)) return;
    const int i = p.i, j = p.j;
    bool set = false;
    if (j < W) {
        const uint16_t d = depth[(size_t)f * W * H + (size_t)i * W + j];
        const float *T = poses + (size_t)f * 16;
        const double z = (double)((float)d / 1000.0f);
        const double x = ((double)j - c.cx) * z / c.fx, y = ((double)i - c.cy) * z / c.fy;
        const double px = (((double)T[0] * x + (double)T[1] * y) + (double)T[2] * z) + (double)T[3];
        const double py = (((double)T[4] * x + (double)T[5] * y) + (double)T[6] * z) + (double)T[7];
        const double pz = (((double)T[8] * x + (double)T[9] * y) + (double)T[10] * z) + (double)T[11];
        set = d > 0 && pz > -0.40 && (px < b.lo[0] || px > b.hi[0] || py < b.lo[1] || py > b.hi[1] || pz < b.lo[2] || pz > b.hi[2]);
    }
    word_pack(p, set, bits + (size_t)f * H * WW);
}

// packed bits -> 0 / 255 bytes, eight pixels per lane
__global__ __launch_bounds__(MK_THREADS) void k_unpack(const unsigned long long *__restrict__ bits, int W, int H, int WW, uint8_t *__restrict__ out)
{
    const int W8 = (W + 7) / 8;
    const uint32_t q = blockIdx.x * MK_THREADS + threadIdx.x;
    if (q >= (uint32_t)H * (uint32_t)W8) return;
    const int i = (int)(q / (uint32_t)W8), j0 = (int)(q - (uint32_t)i * (uint32_t)W8) * 8;
    const unsigned long long word = bits[(size_t)blockIdx.y * H * WW + (size_t)i * WW + (j0 >> 6)];
    const uint32_t m = (uint32_t)(word >> (j0 & 63)) & 0xffu;
    uint8_t *dst = out + (size_t)blockIdx.y * W * H + (size_t)i * W + j0;
    if ((W & 7) == 0) {
        uint2 v;
        v.x = ((m & 1u) ? 0xffu : 0u) | ((m & 2u) ? 0xff00u : 0u) | ((m & 4u) ? 0xff0000u : 0u) | ((m & 8u) ? 0xff000000u : 0u);
        v.y = ((m & 16u) ? 0xffu : 0u) | ((m & 32u) ? 0xff00u : 0u) | ((m & 64u) ? 0xff0000u : 0u) | ((m & 128u) ? 0xff000000u : 0u);
        *reinterpret_cast<uint2 *>(dst) = v;
    } else {
        for (int e = 0; e < 8 && j0 + e < W; ++e) dst[e] = ((m >> e) & 1u) ? 255 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ labelling

__device__ inline unsigned long long wave_sum(unsigned long long v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// statistics at the root's index.  The lanes of a wave hold 64 consecutive pixels: those of equal root are summed in the wave and
// their first lane sends one set of atomics.  depth may be null (disconnected_prune: the area alone).
__global__ __launch_bounds__(MK_THREADS) void k_comp_stats(const uint8_t *__restrict__ mask, const uint16_t *__restrict__ depth, int W, int H,
                                                           const uint32_t *__restrict__ parent, unsigned long long *__restrict__ stats)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    const size_t base = (size_t)blockIdx.y * W * H;
    bool active = false;
    uint32_t root = NO_KEY;
    unsigned long long d = 0, jd = 0, id = 0;
    if (g < (uint32_t)W * (uint32_t)H && mask[base + g]) {
        active = true;
        root = parent[base + g];
        d = depth ? depth[base + g] : 0;
        const uint32_t i = g / (uint32_t)W, j = g - i * (uint32_t)W;
        jd = (unsigned long long)j * d;
        id = (unsigned long long)i * d;
    }
    wave_each_root(active, root, [&](uint32_t r0, unsigned long long members, bool leader) {
        const bool mine = active && root == r0;
        const unsigned long long n = (unsigned long long)__popcll(__ballot(mine && d > 0));
        const unsigned long long sd = wave_sum(mine ? d : 0ull), sjd = wave_sum(mine ? jd : 0ull), sid = wave_sum(mine ? id : 0ull);
        if (leader) {
            unsigned long long *st = stats + (base + r0) * ST_WORDS;
            if (n) {
                atomicAdd(&st[0], n);
                atomicAdd(&st[1], sd);
                atomicAdd(&st[2], sjd);
                atomicAdd(&st[3], sid);
            }
            atomicAdd(reinterpret_cast<uint32_t *>(&st[4]), (uint32_t)__popcll(members));
        }
    });
}

// ------------------------------------------------------------------------------------------------ selection

struct SelSlots {
    uint32_t *ncomp;                 // [n][256] components of the label
    uint32_t *key;                   // [n][256] duplicate: the kept root (NO_KEY none); disconnected: kept root + 1 (0 none)
    unsigned long long *best;        // [n][256] duplicate: smallest distance's bit pattern; disconnected: largest area
};

__global__ __launch_bounds__(MK_THREADS) void k_select_init(SelSlots S, uint32_t total, int mode)
{
    const uint32_t q = blockIdx.x * MK_THREADS + threadIdx.x;
    if (q >= total) return;
    S.ncomp[q] = 0;
    S.key[q] = mode == 0 ? NO_KEY : 0u;
    S.best[q] = mode == 0 ? ~0ull : 0ull;
}

// distance of the component's mean world point from the scene centre; false without a valid-depth pixel or at 10000 and beyond
__device__ inline bool comp_distance(const unsigned long long *st, const float *T, const MaskCam &c, const MaskCentre &ctr, double *out)
{
    if (st[0] == 0) return false;
    const double n = (double)st[0], sd = (double)st[1], sjd = (double)st[2], sid = (double)st[3];
    const double den = 1000.0 * n;
    const double z = sd / den, x = (sjd - c.cx * sd) / (den * c.fx), y = (sid - c.cy * sd) / (den * c.fy);
    const double dx = ((((double)T[0] * x + (double)T[1] * y) + (double)T[2] * z) + (double)T[3]) - ctr.c[0];
    const double dy = ((((double)T[4] * x + (double)T[5] * y) + (double)T[6] * z) + (double)T[7]) - ctr.c[1];
    const double dz = ((((double)T[8] * x + (double)T[9] * y) + (double)T[10] * z) + (double)T[11]) - ctr.c[2];
    const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
    *out = dist;
    return dist < 10000.0;
}

// PASS 0: count the label's components and reduce the best value; PASS 1: among the roots that hold it, the tie rule
template <int PASS>
__global__ __launch_bounds__(MK_THREADS) void k_select(const uint8_t *__restrict__ mask, int W, int H, const uint32_t *__restrict__ parent,
                                                       const unsigned long long *__restrict__ stats, const float *__restrict__ poses, MaskCam c,
                                                       MaskCentre ctr, uint32_t min_area, int mode, uint32_t frame0, SelSlots S)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    if (g >= (uint32_t)W * (uint32_t)H) return;
    const size_t base = (size_t)blockIdx.y * W * H;
    const uint8_t l = mask[base + g];
    if (!l || parent[base + g] != g) return;
    const uint32_t slot = (frame0 + blockIdx.y) * 256u + l;
    const unsigned long long *st = stats + (base + g) * ST_WORDS;
    const uint32_t area = (uint32_t)st[4];
    if (PASS == 0) atomicAdd(&S.ncomp[slot], 1u);
    if (area < min_area) return;
    unsigned long long v;
    if (mode == 0) {
        double dist;
        if (!comp_distance(st, poses + (size_t)(frame0 + blockIdx.y) * 16, c, ctr, &dist)) return;
        v = (unsigned long long)__double_as_longlong(dist);      // non-negative doubles order as their bit patterns
    } else {
        v = area;
    }
    if (PASS == 0) {
        if (mode == 0) atomicMin(&S.best[slot], v);
        else atomicMax(&S.best[slot], v);
    } else if (v == S.best[slot]) {
        if (mode == 0) atomicMin(&S.key[slot], g);               // duplicate_prune compares with <: the first component wins
        else atomicMax(&S.key[slot], g + 1u);                    // disconnected_prune compares with >=: the last one wins
    }
}

__global__ __launch_bounds__(MK_THREADS) void k_prune_write(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ oob, int W, int H,
                                                            const uint32_t *__restrict__ parent, int mode, uint32_t frame0, SelSlots S,
                                                            uint8_t *__restrict__ out)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    if (g >= (uint32_t)W * (uint32_t)H) return;
    const size_t base = (size_t)blockIdx.y * W * H;
    const uint8_t l = mask[base + g];
    uint8_t v = 0;
    if (l) {
        const uint32_t slot = (frame0 + blockIdx.y) * 256u + l, root = parent[base + g];
        const bool keep = S.ncomp[slot] <= 1u || (mode == 0 ? S.key[slot] == root : S.key[slot] == root + 1u);
        if (keep) v = l;
    }
    if (oob && oob[base + g] == 255) v = 255;
    out[base + g] = v;
}

__global__ __launch_bounds__(MK_THREADS) void k_mask_lut(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ oob, size_t total, const uint8_t *__restrict__ lut,
                                                         uint8_t *__restrict__ out, uint8_t *__restrict__ alpha)
{
    __shared__ uint8_t tab[256];
    tab[threadIdx.x] = lut[threadIdx.x] ? 1 : 0;
    __syncthreads();
    const size_t q = ((size_t)blockIdx.x * MK_THREADS + threadIdx.x) * 4;
    if (q >= total) return;
    if (q + 4 <= total) {
        const uint32_t m = *reinterpret_cast<const uint32_t *>(mask + q), ob = oob ? *reinterpret_cast<const uint32_t *>(oob + q) : 0u;
        uint32_t r = 0;
        for (int e = 0; e < 4; ++e) r |= (uint32_t)(tab[(m >> (8 * e)) & 0xffu] | (((ob >> (8 * e)) & 0xffu) ? 1u : 0u)) << (8 * e);
        *reinterpret_cast<uint32_t *>(out + q) = r;
        if (alpha) *reinterpret_cast<uint32_t *>(alpha + q) = (0x01010101u - r) * 255u;
    } else {
        for (size_t e = q; e < total; ++e) {
            const uint8_t r = tab[mask[e]] | ((oob && oob[e]) ? 1 : 0);
            out[e] = r;
            if (alpha) alpha[e] = (uint8_t)(255 * (1 - r));
        }
    }
}

// counts[f][l] += pixels of frame f with label l.  The batch is one byte range that starts 256-byte aligned; frame f is its bytes
// [f px, (f + 1) px), which begin and end anywhere.  The range is cut into the batch's aligned 16-byte segments: a segment inside
// the frame is one uint4 load, the (at most two) segments that straddle a frame's end are read byte by byte inside the frame only.
__global__ __launch_bounds__(MK_THREADS) void k_census(const uint8_t *__restrict__ mask, size_t px, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t hist[MK_THREADS / 64][256];
    const uint32_t t = threadIdx.x;
    for (uint32_t e = 0; e < MK_THREADS / 64; ++e) hist[e][t] = 0;
    __syncthreads();
    uint32_t *h = hist[t >> 6];
    const size_t lo = (size_t)blockIdx.y * px, hi = lo + px;
    const size_t seg1 = (hi + 15) / 16, first = lo / 16 + (size_t)blockIdx.x * CS_SEGS + t;
    for (uint32_t it = 0; it < CS_ITERS; ++it) {
        const size_t s = first + (size_t)it * MK_THREADS;
        if (s >= seg1) break;
        const size_t b = s * 16;
        if (b >= lo && b + 16 <= hi) {
            const uint4 v = *reinterpret_cast<const uint4 *>(mask + b);
            const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
            uint32_t cur = wd[0] & 0xffu, run = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t l = (wd[k >> 2] >> (8 * (k & 3))) & 0xffu;
                if (l == cur) {
                    ++run;
                } else {
                    atomicAdd(&h[cur], run);
                    cur = l;
                    run = 1;
                }
            }
            atomicAdd(&h[cur], run);
        } else {
            const size_t a = b < lo ? lo : b, z = b + 16 < hi ? b + 16 : hi;
            for (size_t e = a; e < z; ++e) atomicAdd(&h[mask[e]], 1u);
        }
    }
    __syncthreads();
    uint32_t sum = 0;
    for (uint32_t e = 0; e < MK_THREADS / 64; ++e) sum += hist[e][t];
    if (sum) atomicAdd(&counts[(size_t)blockIdx.y * 256 + t], sum);
}

// ------------------------------------------------------------------------------------------------ object thumbnails

constexpr int TH_R = 100, TH_TAPS = 2 * TH_R + 1;        // blur radius, taps
constexpr int TH_RS = 256;                               // k_thumb_blur_rows: pixels of a row per workgroup
constexpr int TH_CT = 64;                                // k_thumb_blur_cols: a tile is TH_CT columns x TH_CT rows (+ 2 TH_R rows of halo)
constexpr uint32_t TH_BLUR_BIT = 1u << 29;
constexpr int TH_SLOT = 5;                               // per (frame, label): area, min x, min y, max x, max y

// q[|t|], t = -100 .. 100: floor(2^15 g[t] / sum g + 1/2), g[t] = exp(-t^2 / (2 * 30.5^2)); their sum is 32767, so a row sum fits a
// uint16 and a column sum of row sums stays below 2^30
__constant__ uint16_t c_thumb_taps[TH_R + 1] = {
    429, 429, 428, 427, 425, 423, 421, 418, 415, 411, 407, 402, 397, 392, 386, 380, 374, 367, 360, 353, 346, 338, 331, 323, 315, 307,
    298, 290, 282, 273, 264, 256, 247, 239, 230, 222, 214, 206, 197, 189, 182, 174, 166, 159, 152, 144, 138, 131, 124, 118, 112, 106,
    100, 95,  89,  84,  80,  75,  70,  66,  62,  58,  54,  51,  47,  44,  41,  38,  36,  33,  31,  29,  26,  24,  23,  21,  19,  18,
    16,  15,  14,  13,  12,  11,  10,  9,   8,   7,   7,   6,   6,   5,   5,   4,   4,   3,   3,   3,   2,   2,   2};

// one accepted thumbnail.  row0 .. cols describe the crop in the (rotated, when D2R_THUMB_ROTATED) frame; bits_off is the first word
// of a container's dilated blur bits, rows of ceil(frame columns / 64) words in that same frame
struct ThumbRec {
    uint32_t frame, obj, flags, row0, col0, rows, cols, pad;
    unsigned long long off, bits_off;
};

// reflect-101 applied repeatedly: period 2 (n - 1); n = 1 reads index 0
__device__ inline int thumb_reflect(int p, int n)
{
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int m = p % period;
    if (m < 0) m += period;
    return m >= n ? period - m : m;
}

__global__ __launch_bounds__(MK_THREADS) void k_thumb_init(uint32_t *__restrict__ stats, uint32_t slots, uint32_t *__restrict__ flags)
{
    const uint32_t q = blockIdx.x * MK_THREADS + threadIdx.x;
    if (q < 256u) flags[q] = 0;
    if (q >= slots) return;
    uint32_t *s = stats + (size_t)q * TH_SLOT;
    s[0] = 0;
    s[1] = s[2] = NO_KEY;
    s[3] = s[4] = 0;
}

// stats[frame][label] over the pixels with oob == 0 and 1 <= label < num_objs.  A lane holds four consecutive pixels of a row and
// sends one set of LDS atomics per run of equal labels; the workgroup's non-empty slots go to the frame's row with integer atomics.
__global__ __launch_bounds__(MK_THREADS) void k_thumb_obj_stats(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ oob, int W, int H,
                                                                uint32_t num_objs, uint32_t *__restrict__ stats)
{
    __shared__ uint32_t s_area[256], s_x0[256], s_y0[256], s_x1[256], s_y1[256];
    const uint32_t t = threadIdx.x;
    s_area[t] = 0;
    s_x0[t] = s_y0[t] = NO_KEY;
    s_x1[t] = s_y1[t] = 0;
    __syncthreads();
    const uint32_t W4 = ((uint32_t)W + 3u) / 4u, q = blockIdx.x * MK_THREADS + t;
    if (q < (uint32_t)H * W4) {
        const uint32_t i = q / W4, j0 = (q - i * W4) * 4u;
        const size_t at = (size_t)blockIdx.y * W * H + (size_t)i * W + j0;
        uint32_t m4 = 0, o4 = 0;
        if ((W & 3) == 0) {
            m4 = *reinterpret_cast<const uint32_t *>(mask + at);
            o4 = *reinterpret_cast<const uint32_t *>(oob + at);
        } else {
            for (uint32_t e = 0; e < 4 && j0 + e < (uint32_t)W; ++e) {
                m4 |= (uint32_t)mask[at + e] << (8 * e);
                o4 |= (uint32_t)oob[at + e] << (8 * e);
            }
        }
        auto flush = [&](uint32_t l, uint32_t a, uint32_t b) {
            if (!l) return;
            atomicAdd(&s_area[l], b - a + 1u);
            atomicMin(&s_x0[l], a);
            atomicMax(&s_x1[l], b);
            atomicMin(&s_y0[l], i);
            atomicMax(&s_y1[l], i);
        };
        uint32_t cur = 0, start = j0;
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
            const uint32_t m = (m4 >> (8 * e)) & 0xffu, ob = (o4 >> (8 * e)) & 0xffu;
            const uint32_t l = (j0 + e < (uint32_t)W && ob == 0 && m < num_objs) ? m : 0u;       // label 0 is not an object here
            if (l != cur) {
                flush(cur, start, j0 + e - 1u);
                cur = l;
                start = j0 + e;
            }
        }
        flush(cur, start, j0 + 3u);      // a run that is still open ends inside the row: past it the label is 0
    }
    __syncthreads();
    if (s_area[t]) {
        uint32_t *s = stats + ((size_t)blockIdx.y * 256 + t) * TH_SLOT;
        atomicAdd(&s[0], s_area[t]);
        atomicMin(&s[1], s_x0[t]);
        atomicMin(&s[2], s_y0[t]);
        atomicMax(&s[3], s_x1[t]);
        atomicMax(&s[4], s_y1[t]);
    }
}

// out[o - obj0][g] = 1 where pixel g of the frame is not in object o (label o inside the scene), else 0
__global__ __launch_bounds__(MK_THREADS) void k_thumb_complement(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ oob, uint32_t px,
                                                                 uint32_t obj0, uint8_t *__restrict__ out)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    if (g >= px) return;
    out[(size_t)blockIdx.y * px + g] = (mask[g] == obj0 + blockIdx.y && oob[g] == 0) ? 0 : 1;
}

// at a component's root: stats word 0 += its pixels of label 0, word 1 += its pixels on the frame's border (k_label_flatten zeroed
// both, k_comp_stats without depth leaves them alone and puts the area into word 4).  Equal roots of a wave are combined first.
__global__ __launch_bounds__(MK_THREADS) void k_thumb_comp_stats(const uint8_t *__restrict__ comp, const uint8_t *__restrict__ mask, int W, int H,
                                                                 const uint32_t *__restrict__ parent, unsigned long long *__restrict__ stats)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    const size_t base = (size_t)blockIdx.y * W * H;
    bool active = false, zero = false, border = false;
    uint32_t root = NO_KEY;
    if (g < (uint32_t)W * (uint32_t)H && comp[base + g]) {
        active = true;
        root = parent[base + g];
        zero = mask[g] == 0;
        const uint32_t i = g / (uint32_t)W, j = g - i * (uint32_t)W;
        border = i == 0 || j == 0 || i == (uint32_t)H - 1u || j == (uint32_t)W - 1u;
    }
    wave_each_root(active, root, [&](uint32_t r0, unsigned long long, bool leader) {
        const bool mine = active && root == r0;
        const unsigned long long nz = (unsigned long long)__popcll(__ballot(mine && zero)), nb = (unsigned long long)__popcll(__ballot(mine && border));
        if (leader) {
            unsigned long long *st = stats + (base + r0) * ST_WORDS;
            if (nz) atomicAdd(&st[0], nz);
            if (nb) atomicAdd(&st[1], nb);
        }
    });
}

// one thread per root: area >= hole_area, 10 |comp & label 0| <= 7 area, no pixel on the border -> the object is a container
__global__ __launch_bounds__(MK_THREADS) void k_thumb_container(const uint8_t *__restrict__ comp, int W, int H, const uint32_t *__restrict__ parent,
                                                                const unsigned long long *__restrict__ stats, uint32_t hole_area, uint32_t obj0,
                                                                uint32_t *__restrict__ flags)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    if (g >= (uint32_t)W * (uint32_t)H) return;
    const size_t base = (size_t)blockIdx.y * W * H;
    if (!comp[base + g] || parent[base + g] != g) return;
    const unsigned long long *st = stats + (base + g) * ST_WORDS;
    const unsigned long long area = (uint32_t)st[4];
    if (area >= hole_area && 10ull * st[0] <= 7ull * area && st[1] == 0) atomicOr(&flags[obj0 + blockIdx.y], 1u);
}

// one wave per word of 64 pixels.  recs null: bit = src != 0 (one image); else slot blockIdx.y packs ~obj of its record's frame
__global__ __launch_bounds__(MK_THREADS) void k_thumb_pack(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ oob,
                                                           const ThumbRec *__restrict__ recs, int W, int H, int WW, unsigned long long *__restrict__ bits)
{
    WordLane p;
    if (!d2r_word_lane(H, WW, p)) return;
    bool set = false;
    if (p.j < W) {
        if (recs) {
            const size_t g = (size_t)recs[blockIdx.y].frame * W * H + (size_t)p.i * W + p.j;
            set = !(mask[g] == recs[blockIdx.y].obj && oob[g] == 0);
        } else {
            set = mask[(size_t)p.i * W + p.j] != 0;
        }
    }
    word_pack(p, set, bits + (size_t)blockIdx.y * H * WW);
}

// rowv(i, x) = sum_t q[t] b(i, reflect(x + t)): TH_RS pixels of one row per workgroup, their bits and the halo unpacked into LDS
__global__ __launch_bounds__(MK_THREADS) void k_thumb_blur_rows(const unsigned long long *__restrict__ bits, int W, int H, int WW,
                                                                uint16_t *__restrict__ rowv)
{
    __shared__ uint8_t seg[TH_RS + 2 * TH_R];
    const int t = (int)threadIdx.x, x0 = (int)blockIdx.x * TH_RS, i = (int)blockIdx.y;
    const unsigned long long *row = bits + (size_t)blockIdx.z * H * WW + (size_t)i * WW;
    for (int q = t; q < TH_RS + 2 * TH_R; q += (int)MK_THREADS) seg[q] = plane_bit(row, WW, 0, thumb_reflect(x0 - TH_R + q, W));
    __syncthreads();
    const int x = x0 + t;
    if (x >= W) return;
    uint32_t acc = 0;
    for (int k = 0; k < TH_TAPS; ++k) acc += (uint32_t)c_thumb_taps[k < TH_R ? TH_R - k : k - TH_R] * seg[t + k];
    rowv[(size_t)blockIdx.z * W * H + (size_t)i * W + x] = (uint16_t)acc;
}

// blur bit (y, x) = sum_t q[t] rowv(reflect(y + t), x) >= 2^29, packed: lanes along x, a wave's ballot is a row's word.  recs null or
// an unrotated record: rows of WW words.  A rotated record: the tile's 64 x 64 bits are transposed through LDS and written as the
// rotated frame's rows (row W - 1 - x, word y / 64) of HW words, so that the dilation runs in the rotated frame.
__global__ __launch_bounds__(MK_THREADS) void k_thumb_blur_cols(const uint16_t *__restrict__ rowv, int W, int H, int WW, int HW,
                                                                const ThumbRec *__restrict__ recs, unsigned long long *__restrict__ out)
{
    __shared__ uint16_t tile[TH_CT + 2 * TH_R][TH_CT];
    __shared__ unsigned long long rowbits[TH_CT];
    const int t = (int)threadIdx.x, x0 = (int)blockIdx.x * TH_CT, y0 = (int)blockIdx.y * TH_CT;
    const uint16_t *src = rowv + (size_t)blockIdx.z * W * H;
    for (int q = t; q < (TH_CT + 2 * TH_R) * TH_CT; q += (int)MK_THREADS) {
        const int r = q / TH_CT, c = q - r * TH_CT, x = x0 + c;
        tile[r][c] = x < W ? src[(size_t)thumb_reflect(y0 - TH_R + r, H) * W + x] : (uint16_t)0;
    }
    __syncthreads();
    const int c = t & 63, wv = t >> 6;
    for (int rr = 0; rr < TH_CT / 4; ++rr) {
        const int r = wv * (TH_CT / 4) + rr;
        uint32_t acc = 0;
        for (int k = 0; k < TH_TAPS; ++k) acc += (uint32_t)c_thumb_taps[k < TH_R ? TH_R - k : k - TH_R] * tile[r + k][c];
        const unsigned long long m = __ballot(y0 + r < H && x0 + c < W && acc >= TH_BLUR_BIT);
        if (c == 0) rowbits[r] = m;
    }
    __syncthreads();
    if (t >= TH_CT) return;
    const bool rot = recs && (recs[blockIdx.z].flags & D2R_THUMB_ROTATED);
    unsigned long long *o = out + (recs ? recs[blockIdx.z].bits_off : 0ull);
    if (!rot) {
        if (y0 + t < H) o[(size_t)(y0 + t) * WW + blockIdx.x] = rowbits[t];
    } else if (x0 + t < W) {
        unsigned long long word = 0;
        for (int y = 0; y < TH_CT; ++y) word |= ((rowbits[y] >> t) & 1ull) << y;
        o[(size_t)(W - 1 - (x0 + t)) * HW + blockIdx.y] = word;
    }
}

// thumbnail blockIdx.y, four pixels (twelve bytes) per lane.  Pixel (ti, tj) of the crop is pixel (row0 + ti, col0 + tj) of the
// record's frame, which reads unrotated memory at (y, x) = (rj, W - 1 - ri) when rotated.  Not a container: the frame where the
// object is, white elsewhere.  Container: the noise where the dilated blur bit is set, the frame elsewhere.
__global__ __launch_bounds__(MK_THREADS) void k_thumb_compose(const uint8_t *__restrict__ rgb, const uint8_t *__restrict__ mask,
                                                              const uint8_t *__restrict__ oob, const uint8_t *__restrict__ noise,
                                                              const ThumbRec *__restrict__ recs, int W, int H, int WW, int HW,
                                                              const unsigned long long *__restrict__ bits, uint8_t *__restrict__ out)
{
    const ThumbRec rec = recs[blockIdx.y];
    const uint32_t npx = rec.rows * rec.cols, p0 = (blockIdx.x * MK_THREADS + threadIdx.x) * 4u;
    if (p0 >= npx) return;
    const bool rot = rec.flags & D2R_THUMB_ROTATED, container = rec.flags & D2R_THUMB_CONTAINER;
    const size_t px = (size_t)W * H;
    uint32_t wd[3] = {0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t p = p0 + e;
        uint32_t r = 0, g = 0, b = 0;
        if (p < npx) {
            const uint32_t ti = p / rec.cols, ri = rec.row0 + ti, rj = rec.col0 + (p - ti * rec.cols);
            const uint32_t y = rot ? rj : ri, x = rot ? (uint32_t)W - 1u - ri : rj;
            const size_t at = (size_t)y * W + x, fat = (size_t)rec.frame * px + at;
            const uint8_t *src = rgb + fat * 3;
            bool white = false;
            if (container) {
                if (plane_bit(bits + rec.bits_off, rot ? HW : WW, (int)ri, (int)rj)) src = noise + at * 3;
            } else {
                white = !(mask[fat] == rec.obj && oob[fat] == 0);
            }
            r = white ? 255u : src[0];
            g = white ? 255u : src[1];
            b = white ? 255u : src[2];
        }
        wd[(3 * e) >> 2] |= r << (8 * ((3 * e) & 3));
        wd[(3 * e + 1) >> 2] |= g << (8 * ((3 * e + 1) & 3));
        wd[(3 * e + 2) >> 2] |= b << (8 * ((3 * e + 2) & 3));
    }
    uint8_t *dst = out + rec.off + (size_t)p0 * 3;      // rec.off and 3 p0 are multiples of 4
    if (p0 + 4 <= npx) {
        uint32_t *d4 = reinterpret_cast<uint32_t *>(dst);
        d4[0] = wd[0];
        d4[1] = wd[1];
        d4[2] = wd[2];
    } else {
        const uint32_t nb = (npx - p0) * 3u;
#pragma unroll
        for (uint32_t e = 0; e < 9; ++e)
            if (e < nb) dst[e] = (uint8_t)(wd[e >> 2] >> (8 * (e & 3)));
    }
}

// ------------------------------------------------------------------------------------------------ host side

int masks_check_frames(d2r_ctx *ctx, uint32_t n, uint32_t w, uint32_t h)
{
    if (n == 0 || w == 0 || h == 0) return d2r_fail(ctx, D2R_ERR_INVALID, "masks: n, width and height must be at least 1");
    if ((uint64_t)w * h >= (1ull << 31)) return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "masks: a frame must have fewer than 2^31 pixels");
    if (n > 65535) return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "masks: at most 65535 frames per call");
    if ((uint64_t)n * w * h >= (1ull << 40)) return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "masks: the batch must have fewer than 2^40 pixels");
    return D2R_OK;
}

// label, flatten and accumulate nf frames whose images start at mask / depth; parent and stats are the pass's workspace
void masks_label(d2r_ctx *ctx, const uint8_t *mask, const uint16_t *depth, uint32_t nf, uint32_t w, uint32_t h, uint32_t *parent,
                 unsigned long long *stats)
{
    label_components(ctx, ByteSrc{mask, (int)w, (int)h}, nf, parent, stats, 8 * ST_WORDS);
    hipLaunchKernelGGL(k_comp_stats, dim3((w * h + MK_THREADS - 1) / MK_THREADS, nf), dim3(MK_THREADS), 0, ctx->stream, mask, depth, (int)w, (int)h,
                       (const uint32_t *)parent, stats);
}

// frames per pass of d2r_masks_prune: 100 frames of 1280 x 720 go 26 per pass with the default budget
uint32_t masks_pass_frames(uint32_t n, size_t px)
{
    return pass_items("D2R_MASKS_WS_BYTES", MK_WS_BUDGET, n, px * (4 + 8 * ST_WORDS));
}

// blur bit of `slots` packed images (b0, rows of ww words) dilated by k x k into `dil`.  recs null: the images' own frame, one slot.
// Else slot s belongs to recs[s]; the first n_rot slots are rotated frames: their blur bits are written, and dilated, as rows of hw
// words (section 2g: with an even k the window is not symmetric, so the dilation has to run in the rotated frame).
void thumbs_blur_dilate(d2r_ctx *ctx, const unsigned long long *b0, uint16_t *rowv, unsigned long long *blur, unsigned long long *dil,
                        const ThumbRec *recs, uint32_t slots, uint32_t n_rot, uint32_t w, uint32_t h, uint32_t k)
{
    const uint32_t ww = (w + 63) / 64, hw = (h + 63) / 64;
    hipLaunchKernelGGL(k_thumb_blur_rows, dim3((w + TH_RS - 1) / TH_RS, h, slots), dim3(MK_THREADS), 0, ctx->stream, b0, (int)w, (int)h, (int)ww, rowv);
    hipLaunchKernelGGL(k_thumb_blur_cols, dim3(ww, hw, slots), dim3(MK_THREADS), 0, ctx->stream, (const uint16_t *)rowv, (int)w, (int)h, (int)ww,
                       (int)hw, recs, blur);
    if (n_rot)
        hipLaunchKernelGGL(k_morph<false>, dim3((hw + CL_TW - 1) / CL_TW, (w + CL_TR - 1) / CL_TR, n_rot), dim3(MK_THREADS), 0, ctx->stream,
                           (const unsigned long long *)blur, dil, (int)h, (int)w, (int)hw, (int)k);
    if (slots > n_rot) {
        const size_t first = (size_t)n_rot * w * hw;
        hipLaunchKernelGGL(k_morph<false>, dim3((ww + CL_TW - 1) / CL_TW, (h + CL_TR - 1) / CL_TR, slots - n_rot), dim3(MK_THREADS), 0, ctx->stream,
                           (const unsigned long long *)blur + first, dil + first, (int)w, (int)h, (int)ww, (int)k);
    }
}

}  // namespace

extern "C" {

int d2r_scene_bound_masks(d2r_ctx *ctx, const uint16_t *depth_u16, uint32_t n, uint32_t w, uint32_t h, const float *poses, const double *K,
                          const double *bounds, uint32_t window, uint8_t *out_u8, uint8_t *raw_out_u8)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (!depth_u16 || !poses || !K || !bounds || !out_u8) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (window < 1 || window > 64) return d2r_fail(ctx, D2R_ERR_INVALID, "scene-bound masks: window must be 1 .. 64");
    int rc;
    if ((rc = masks_check_frames(ctx, n, w, h)) || (rc = d2r_check_cam(ctx, "masks", K, poses, n))) return rc;
    for (int i = 0; i < 6; ++i)
        if (std::isnan(bounds[i])) return d2r_fail(ctx, D2R_ERR_INVALID, "scene-bound masks: bounds must not be NaN");
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)w * h, ww = (w + 63) / 64, words = (size_t)n * h * ww;
    D2rStage in(ctx, ctx->mask_in);
    const size_t o_depth = in.add(px * 2 * n), o_pose = in.add((size_t)n * 64), o_bits = in.add(2 * words * 8);
    if ((rc = in.reserve()) || (rc = d2r_reserve(ctx, ctx->mask_out, px * n))) return rc;
    const uint16_t *d_depth = in.at<uint16_t>(o_depth);
    const float *d_pose = in.at<float>(o_pose);
    unsigned long long *b0 = in.at<unsigned long long>(o_bits), *b1 = b0 + words;
    MaskCam c{K[0], K[4], K[2], K[5]};
    MaskBox b{{bounds[0], bounds[1], -100.0}, {bounds[3], bounds[4], bounds[5]}};       // the reference overwrites zmin (data_loader.py:84)
    if ((rc = ctx->mask_timer.mark(ctx, 0)) || (rc = in.upload(o_depth, depth_u16, px * 2 * n))) return rc;
    if ((rc = in.upload(o_pose, poses, (size_t)n * 64)) || (rc = ctx->mask_timer.mark(ctx, 1))) return rc;
    const uint32_t wpf = (uint32_t)(h * ww), W8 = (w + 7) / 8;
    const dim3 g_unpack((uint32_t)(((size_t)h * W8 + MK_THREADS - 1) / MK_THREADS), n);
    hipLaunchKernelGGL(k_scene_bounds, dim3((wpf + 3) / 4, n), dim3(MK_THREADS), 0, ctx->stream, d_depth, d_pose, c, b, (int)w, (int)h, (int)ww, b0);
    if (raw_out_u8) {
        hipLaunchKernelGGL(k_unpack, g_unpack, dim3(MK_THREADS), 0, ctx->stream, (const unsigned long long *)b0, (int)w, (int)h, (int)ww,
                           (uint8_t *)ctx->mask_out.p);
        D2R_HIP(ctx, hipMemcpyAsync(raw_out_u8, ctx->mask_out.p, px * n, hipMemcpyDeviceToHost, ctx->stream));
    }
    const dim3 g_morph((uint32_t)((ww + CL_TW - 1) / CL_TW), (h + CL_TR - 1) / CL_TR, n);
    hipLaunchKernelGGL(k_morph<false>, g_morph, dim3(MK_THREADS), 0, ctx->stream, (const unsigned long long *)b0, b1, (int)w, (int)h, (int)ww, (int)window);
    hipLaunchKernelGGL(k_morph<true>, g_morph, dim3(MK_THREADS), 0, ctx->stream, (const unsigned long long *)b1, b0, (int)w, (int)h, (int)ww, (int)window);
    hipLaunchKernelGGL(k_unpack, g_unpack, dim3(MK_THREADS), 0, ctx->stream, (const unsigned long long *)b0, (int)w, (int)h, (int)ww,
                       (uint8_t *)ctx->mask_out.p);
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = ctx->mask_timer.mark(ctx, 2))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(out_u8, ctx->mask_out.p, px * n, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ctx->mask_timer.mark(ctx, 3))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mask_timer.done();
    return D2R_OK;
}

int d2r_masks_prune(d2r_ctx *ctx, int mode, const uint8_t *masks_u8, const uint16_t *depth_u16, const uint8_t *oob_u8, uint32_t n, uint32_t w,
                    uint32_t h, const float *poses, const double *K, const double *centre, uint32_t min_area, uint8_t *out_u8)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (mode != 0 && mode != 1) return d2r_fail(ctx, D2R_ERR_INVALID, "masks prune: mode must be 0 (duplicate) or 1 (disconnected)");
    if (!masks_u8 || !out_u8 || (mode == 0 && (!depth_u16 || !poses || !K || !centre))) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    int rc;
    if ((rc = masks_check_frames(ctx, n, w, h))) return rc;
    MaskCam c{1.0, 1.0, 0.0, 0.0};
    MaskCentre ctr{{0.0, 0.0, 0.0}};
    if (mode == 0) {
        if ((rc = d2r_check_cam(ctx, "masks", K, poses, n))) return rc;
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(centre[i])) return d2r_fail(ctx, D2R_ERR_INVALID, "masks prune: scene centre must be finite");
        c = MaskCam{K[0], K[4], K[2], K[5]};
        ctr = MaskCentre{{centre[0], centre[1], centre[2]}};
    }
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)w * h, tot = px * n;
    const bool have_depth = mode == 0;
    D2rStage in(ctx, ctx->mask_in);      // a frame set the call goes without is a segment of 0 bytes
    const size_t o_mask = in.add(tot), o_depth = in.add(have_depth ? tot * 2 : 0), o_oob = in.add(oob_u8 ? tot : 0),
                 o_pose = in.add((size_t)n * 64), o_n = in.add((size_t)n * 1024), o_key = in.add((size_t)n * 1024),
                 o_best = in.add((size_t)n * 2048);
    const uint32_t per = masks_pass_frames(n, px);
    if ((rc = in.reserve()) || (rc = d2r_reserve(ctx, ctx->mask_out, tot)) ||
        (rc = d2r_reserve(ctx, ctx->mask_ws, (size_t)per * px * (4 + 8 * ST_WORDS))))
        return rc;
    const uint8_t *d_mask = in.at<uint8_t>(o_mask), *d_oob = oob_u8 ? in.at<uint8_t>(o_oob) : nullptr;
    const uint16_t *d_depth = have_depth ? in.at<uint16_t>(o_depth) : nullptr;
    const float *d_pose = in.at<float>(o_pose);
    SelSlots S{in.at<uint32_t>(o_n), in.at<uint32_t>(o_key), in.at<unsigned long long>(o_best)};
    unsigned long long *stats = (unsigned long long *)ctx->mask_ws.p;
    uint32_t *parent = (uint32_t *)((uint8_t *)ctx->mask_ws.p + (size_t)per * px * 8 * ST_WORDS);
    if ((rc = ctx->mask_timer.mark(ctx, 0)) || (rc = in.upload(o_mask, masks_u8, tot))) return rc;
    if (have_depth && ((rc = in.upload(o_depth, depth_u16, tot * 2)) || (rc = in.upload(o_pose, poses, (size_t)n * 64)))) return rc;
    if (oob_u8 && (rc = in.upload(o_oob, oob_u8, tot))) return rc;
    if ((rc = ctx->mask_timer.mark(ctx, 1))) return rc;
    hipLaunchKernelGGL(k_select_init, dim3((n * 256u + MK_THREADS - 1) / MK_THREADS), dim3(MK_THREADS), 0, ctx->stream, S, n * 256u, mode);
    const uint32_t gpx = (uint32_t)((px + MK_THREADS - 1) / MK_THREADS);
    for (uint32_t f0 = 0; f0 < n; f0 += per) {              // passes share the workspace; nothing waits in between
        const uint32_t nf = std::min(per, n - f0);
        const uint8_t *m = d_mask + (size_t)f0 * px;
        masks_label(ctx, m, d_depth ? d_depth + (size_t)f0 * px : nullptr, nf, w, h, parent, stats);
        hipLaunchKernelGGL(k_select<0>, dim3(gpx, nf), dim3(MK_THREADS), 0, ctx->stream, m, (int)w, (int)h, (const uint32_t *)parent,
                           (const unsigned long long *)stats, d_pose, c, ctr, min_area, mode, f0, S);
        hipLaunchKernelGGL(k_select<1>, dim3(gpx, nf), dim3(MK_THREADS), 0, ctx->stream, m, (int)w, (int)h, (const uint32_t *)parent,
                           (const unsigned long long *)stats, d_pose, c, ctr, min_area, mode, f0, S);
        hipLaunchKernelGGL(k_prune_write, dim3(gpx, nf), dim3(MK_THREADS), 0, ctx->stream, m, d_oob ? d_oob + (size_t)f0 * px : nullptr, (int)w, (int)h,
                           (const uint32_t *)parent, mode, f0, S, (uint8_t *)ctx->mask_out.p + (size_t)f0 * px);
    }
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = ctx->mask_timer.mark(ctx, 2))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(out_u8, ctx->mask_out.p, tot, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ctx->mask_timer.mark(ctx, 3))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mask_timer.done();
    return D2R_OK;
}

int d2r_masks_components(d2r_ctx *ctx, const uint8_t *mask_u8, const uint16_t *depth_u16, uint32_t w, uint32_t h, uint32_t *keys_out,
                         uint32_t *area_out, uint64_t *sums_out)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (!mask_u8 || !depth_u16 || !keys_out || !area_out || !sums_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    int rc;
    if ((rc = masks_check_frames(ctx, 1, w, h))) return rc;
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)w * h;
    D2rStage in(ctx, ctx->mask_in);
    const size_t o_mask = in.add(px), o_depth = in.add(px * 2);
    if ((rc = in.reserve()) || (rc = d2r_reserve(ctx, ctx->mask_ws, px * (4 + 8 * ST_WORDS)))) return rc;
    unsigned long long *stats = (unsigned long long *)ctx->mask_ws.p;
    uint32_t *parent = (uint32_t *)((uint8_t *)ctx->mask_ws.p + px * 8 * ST_WORDS);
    if ((rc = in.upload(o_mask, mask_u8, px)) || (rc = in.upload(o_depth, depth_u16, px * 2))) return rc;
    masks_label(ctx, in.at<uint8_t>(o_mask), in.at<uint16_t>(o_depth), 1, w, h, parent, stats);
    D2R_HIP(ctx, hipGetLastError());
    std::vector<unsigned long long> st(px * ST_WORDS);
    D2R_HIP(ctx, hipMemcpyAsync(keys_out, parent, px * 4, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(st.data(), stats, px * 8 * ST_WORDS, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t g = 0; g < px; ++g) {                       // only roots carry statistics; label 0 has no component
        const bool root = mask_u8[g] != 0 && keys_out[g] == (uint32_t)g;
        if (!mask_u8[g]) keys_out[g] = NO_KEY;
        area_out[g] = root ? (uint32_t)st[g * ST_WORDS + 4] : 0u;
        for (int e = 0; e < 4; ++e) sums_out[g * 4 + e] = root ? (uint64_t)st[g * ST_WORDS + e] : 0ull;
    }
    return D2R_OK;
}

int d2r_masks_lut(d2r_ctx *ctx, const uint8_t *masks_u8, const uint8_t *oob_u8, uint32_t n, uint32_t w, uint32_t h, const uint8_t *lut,
                  uint8_t *out_u8, uint8_t *alpha_out_u8)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (!masks_u8 || !lut || !out_u8) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    int rc;
    if ((rc = masks_check_frames(ctx, n, w, h))) return rc;
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    const size_t tot = (size_t)w * h * n;
    D2rStage in(ctx, ctx->mask_in), out(ctx, ctx->mask_out);
    const size_t o_mask = in.add(tot), o_oob = in.add(tot), o_lut = in.add(256), o_out = out.add(tot), o_alpha = out.add(tot);
    if ((rc = in.reserve()) || (rc = out.reserve())) return rc;
    if ((rc = in.upload(o_mask, masks_u8, tot)) || (oob_u8 && (rc = in.upload(o_oob, oob_u8, tot))) || (rc = in.upload(o_lut, lut, 256))) return rc;
    uint8_t *d_out = out.at<uint8_t>(o_out), *d_alpha = alpha_out_u8 ? out.at<uint8_t>(o_alpha) : nullptr;
    const size_t quads = (tot + 3) / 4;
    hipLaunchKernelGGL(k_mask_lut, dim3((uint32_t)((quads + MK_THREADS - 1) / MK_THREADS)), dim3(MK_THREADS), 0, ctx->stream,
                       in.at<const uint8_t>(o_mask), oob_u8 ? in.at<const uint8_t>(o_oob) : nullptr, tot, in.at<const uint8_t>(o_lut), d_out, d_alpha);
    D2R_HIP(ctx, hipGetLastError());
    D2R_HIP(ctx, hipMemcpyAsync(out_u8, d_out, tot, hipMemcpyDeviceToHost, ctx->stream));
    if (alpha_out_u8) D2R_HIP(ctx, hipMemcpyAsync(alpha_out_u8, d_alpha, tot, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return D2R_OK;
}

int d2r_masks_census(d2r_ctx *ctx, const uint8_t *masks_u8, uint32_t n, uint32_t w, uint32_t h, uint32_t *counts_out)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (!masks_u8 || !counts_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    int rc;
    if ((rc = masks_check_frames(ctx, n, w, h))) return rc;
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)w * h, tot = px * n, out_bytes = (size_t)n * 256 * sizeof(uint32_t);
    D2rStage in(ctx, ctx->mask_in);
    const size_t o_mask = in.add(tot);
    if ((rc = in.reserve()) || (rc = d2r_reserve(ctx, ctx->mask_out, out_bytes))) return rc;
    if ((rc = ctx->mask_timer.mark(ctx, 0)) || (rc = in.upload(o_mask, masks_u8, tot)) || (rc = ctx->mask_timer.mark(ctx, 1))) return rc;
    D2R_HIP(ctx, hipMemsetAsync(ctx->mask_out.p, 0, out_bytes, ctx->stream));
    const size_t segs = px / 16 + 2;                         // a frame overlaps at most this many aligned segments of the batch
    hipLaunchKernelGGL(k_census, dim3((uint32_t)((segs + CS_SEGS - 1) / CS_SEGS), n), dim3(MK_THREADS), 0, ctx->stream,
                       in.at<const uint8_t>(o_mask), px, (uint32_t *)ctx->mask_out.p);
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = ctx->mask_timer.mark(ctx, 2))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(counts_out, ctx->mask_out.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ctx->mask_timer.mark(ctx, 3))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mask_timer.done();
    return D2R_OK;
}

int d2r_masks_get_timing(d2r_ctx *ctx, double *ms_out)
{
    if (!ctx || !ms_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    return ctx->mask_timer.read(ctx, ms_out, 3, "masks timing: no batch call has run on this context");
}

int d2r_thumbs_plan(d2r_ctx *ctx, const uint8_t *rgbs, const uint8_t *masks_u8, const uint8_t *oob_u8, uint32_t n, uint32_t w, uint32_t h,
                    uint32_t num_objs, const uint32_t *params, uint32_t *recs_out, uint32_t *n_recs, uint64_t *total_bytes)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (!rgbs || !masks_u8 || !oob_u8 || !params || !n_recs || !total_bytes) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    const bool topdown = params[0] != 0, multi_view = params[1] != 0;
    const uint32_t single = params[2], min_area = params[3], hole_area = params[4], pad = params[5], dilate_k = params[6];
    int rc;
    if ((rc = masks_check_frames(ctx, n, w, h))) return rc;
    if (num_objs == 0 || num_objs > 255) return d2r_fail(ctx, D2R_ERR_INVALID, "thumbnails: num_objs must be 1 .. 255");
    if (dilate_k < 1 || dilate_k > 64) return d2r_fail(ctx, D2R_ERR_INVALID, "thumbnails: dilate_k must be 1 .. 64");
    if (single >= n) return d2r_fail(ctx, D2R_ERR_INVALID, "thumbnails: single_view_idx must be below the number of frames");
    const uint32_t nobj = num_objs - 1, nvis = multi_view ? n : 1u, f_first = multi_view ? 0u : single, count = nobj * nvis;
    if (recs_out && *n_recs < count) return d2r_fail(ctx, D2R_ERR_INVALID, "thumbnails: recs_out holds fewer records than the plan has");
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    ctx->thumb_plan.valid = false;
    ctx->cap_src.filled = false;
    const size_t px = (size_t)w * h, tot = px * n;
    const bool test0 = f_first == 0 && nobj > 0;            // the container test runs on frame 0 alone
    // objects per pass of the container test: a pixel costs masks_label's 44 bytes and one more for the complement image
    const uint32_t per = test0 ? masks_pass_frames(nobj, px + px / (4 + 8 * ST_WORDS) + 1) : 0u;
    D2rStage in(ctx, ctx->thumb_in), ws(ctx, ctx->thumb_ws);
    const size_t o_rgb = in.add(tot * 3), o_mask = in.add(tot), o_oob = in.add(tot);
    const size_t o_stats = ws.add((size_t)nvis * 256 * TH_SLOT * 4), o_flags = ws.add(256 * 4), o_comp = ws.add((size_t)per * px),
                 o_lstats = ws.add((size_t)per * px * 8 * ST_WORDS), o_parent = ws.add((size_t)per * px * 4);
    if ((rc = in.reserve()) || (rc = ws.reserve())) return rc;
    D2rStageTimer &timer = ctx->thumb_timer[0];
    if ((rc = timer.mark(ctx, 0)) || (rc = in.upload(o_rgb, rgbs, tot * 3)) || (rc = in.upload(o_mask, masks_u8, tot)) ||
        (rc = in.upload(o_oob, oob_u8, tot)) || (rc = timer.mark(ctx, 1)))
        return rc;
    const uint8_t *d_mask = in.at<uint8_t>(o_mask), *d_oob = in.at<uint8_t>(o_oob);
    uint32_t *d_stats = ws.at<uint32_t>(o_stats), *d_flags = ws.at<uint32_t>(o_flags);
    const uint32_t slots = nvis * 256u, gpx = (uint32_t)((px + MK_THREADS - 1) / MK_THREADS);
    hipLaunchKernelGGL(k_thumb_init, dim3((slots + MK_THREADS - 1) / MK_THREADS), dim3(MK_THREADS), 0, ctx->stream, d_stats, slots, d_flags);
    const uint32_t quads = h * ((w + 3) / 4);
    hipLaunchKernelGGL(k_thumb_obj_stats, dim3((quads + MK_THREADS - 1) / MK_THREADS, nvis), dim3(MK_THREADS), 0, ctx->stream,
                       d_mask + (size_t)f_first * px, d_oob + (size_t)f_first * px, (int)w, (int)h, num_objs, d_stats);
    if (test0) {
        uint8_t *comp = ws.at<uint8_t>(o_comp);
        unsigned long long *lstats = ws.at<unsigned long long>(o_lstats);
        uint32_t *parent = ws.at<uint32_t>(o_parent);
        for (uint32_t o0 = 1; o0 < num_objs; o0 += per) {        // passes of objects share the workspace; nothing waits in between
            const uint32_t no = std::min(per, num_objs - o0);
            hipLaunchKernelGGL(k_thumb_complement, dim3(gpx, no), dim3(MK_THREADS), 0, ctx->stream, d_mask, d_oob, (uint32_t)px, o0, comp);
            masks_label(ctx, comp, nullptr, no, w, h, parent, lstats);
            hipLaunchKernelGGL(k_thumb_comp_stats, dim3(gpx, no), dim3(MK_THREADS), 0, ctx->stream, (const uint8_t *)comp, d_mask, (int)w, (int)h,
                               (const uint32_t *)parent, lstats);
            hipLaunchKernelGGL(k_thumb_container, dim3(gpx, no), dim3(MK_THREADS), 0, ctx->stream, (const uint8_t *)comp, (int)w, (int)h,
                               (const uint32_t *)parent, (const unsigned long long *)lstats, hole_area, o0, d_flags);
        }
    }
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = timer.mark(ctx, 2))) return rc;
    std::vector<uint32_t> stats((size_t)slots * TH_SLOT), flags(256);
    D2R_HIP(ctx, hipMemcpyAsync(stats.data(), d_stats, stats.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(flags.data(), d_flags, 256 * 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = timer.mark(ctx, 3))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    timer.done();
    // the sequential acceptance rule (section 2g, "Per frame")
    std::vector<uint32_t> &recs = ctx->thumb_plan.recs;
    recs.assign((size_t)count * D2R_THUMB_REC_WORDS, 0u);
    uint64_t off = 0;
    size_t at = 0;
    for (uint32_t o = 1; o < num_objs; ++o) {
        uint32_t accepted = 0;
        bool container = false;
        for (uint32_t v = 0; v < nvis; ++v, at += D2R_THUMB_REC_WORDS) {
            const uint32_t f = f_first + v, *s = &stats[((size_t)v * 256 + o) * TH_SLOT];
            const bool rot = (f < 2 && !topdown) || (!multi_view && single > 0);
            const uint32_t area = s[0], fh = rot ? w : h, fw = rot ? h : w;          // the (rotated) frame's rows and columns
            uint32_t *r = &recs[at];
            r[0] = o;
            r[1] = f;
            r[2] = rot ? D2R_THUMB_ROTATED : 0u;
            r[3] = area;
            if (area == 0) {
                r[2] |= D2R_THUMB_SMALL;
                continue;
            }
            // rotated pixel (i, j) is unrotated (y, x) = (j, w - 1 - i)
            const uint32_t i0 = rot ? w - 1 - s[3] : s[2], i1 = rot ? w - 1 - s[1] : s[4], j0 = rot ? s[2] : s[1], j1 = rot ? s[4] : s[3];
            const bool edge = i0 == 0 || j0 == 0 || i1 == fh - 1 || j1 == fw - 1;
            if (edge) r[2] |= D2R_THUMB_EDGE;
            if (area < min_area) {
                r[2] |= D2R_THUMB_SMALL;
                continue;
            }
            if (edge && accepted >= 3 && !topdown) continue;
            if (f == 0) container = flags[o] != 0;
            if (container) {
                r[2] |= D2R_THUMB_CONTAINER;
                r[4] = r[5] = 0;
                r[6] = fh;
                r[7] = fw;
            } else {
                const uint64_t a0 = i0 > pad ? i0 - pad : 0, a1 = std::min<uint64_t>((uint64_t)i1 + pad, fh - 1);
                const uint64_t b0 = j0 > pad ? j0 - pad : 0, b1 = std::min<uint64_t>((uint64_t)j1 + pad, fw - 1);
                r[4] = (uint32_t)a0;
                r[5] = (uint32_t)b0;
                r[6] = (uint32_t)(a1 - a0 + 1);
                r[7] = (uint32_t)(b1 - b0 + 1);
            }
            r[2] |= D2R_THUMB_ACCEPTED;
            r[8] = (uint32_t)off;
            r[9] = (uint32_t)(off >> 32);
            off = (off + (uint64_t)r[6] * r[7] * 3 + 3) & ~(uint64_t)3;
            ++accepted;
        }
    }
    D2rThumbPlan &P = ctx->thumb_plan;
    P.n = n; P.w = w; P.h = h; P.dilate_k = dilate_k;
    P.o_rgb = o_rgb; P.o_mask = o_mask; P.o_oob = o_oob;
    P.total = off;
    P.valid = true;
    if (recs_out) memcpy(recs_out, recs.data(), recs.size() * 4);
    *n_recs = count;
    *total_bytes = off;
    return D2R_OK;
}

int d2r_thumbs_fill(d2r_ctx *ctx, const uint8_t *noise_u8, uint8_t *out_u8, uint64_t total_bytes)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    const D2rThumbPlan &P = ctx->thumb_plan;
    if (!P.valid) return d2r_fail(ctx, D2R_ERR_INVALID, "thumbnails: d2r_thumbs_fill needs a d2r_thumbs_plan on this context first");
    if (!noise_u8 || (!out_u8 && P.total)) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (total_bytes < P.total) return d2r_fail(ctx, D2R_ERR_INVALID, "thumbnails: total_bytes is smaller than the plan's total");
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t w = P.w, h = P.h, ww = (w + 63) / 64, hw = (h + 63) / 64;
    const size_t px = (size_t)w * h, rot_words = (size_t)w * hw, flat_words = (size_t)h * ww;
    // accepted records in plan order; container slots with the rotated frames first
    std::vector<ThumbRec> recs;
    std::vector<uint32_t> cont[2];
    uint32_t max_px = 0;
    for (size_t at = 0; at < P.recs.size(); at += D2R_THUMB_REC_WORDS) {
        const uint32_t *r = &P.recs[at];
        if (!(r[2] & D2R_THUMB_ACCEPTED)) continue;
        if (r[2] & D2R_THUMB_CONTAINER) cont[(r[2] & D2R_THUMB_ROTATED) ? 0 : 1].push_back((uint32_t)recs.size());
        recs.push_back(ThumbRec{r[1], r[0], r[2], r[4], r[5], r[6], r[7], 0u, (unsigned long long)r[8] | (unsigned long long)r[9] << 32, 0ull});
        max_px = std::max(max_px, r[6] * r[7]);
    }
    const uint32_t n_rot = (uint32_t)cont[0].size(), slots = n_rot + (uint32_t)cont[1].size();
    std::vector<ThumbRec> slot_recs;                        // slot s packs and blurs ~obj of slot_recs[s]
    for (int g = 0; g < 2; ++g)
        for (uint32_t idx : cont[g]) {
            const size_t s = slot_recs.size();
            recs[idx].bits_off = s < n_rot ? s * rot_words : n_rot * rot_words + (s - n_rot) * flat_words;
            slot_recs.push_back(recs[idx]);
        }
    const size_t bit_words = (size_t)n_rot * rot_words + (size_t)(slots - n_rot) * flat_words;
    D2rStage ws(ctx, ctx->thumb_ws);
    const size_t o_noise = ws.add(px * 3), o_recs = ws.add(recs.size() * sizeof(ThumbRec)), o_srecs = ws.add(slots * sizeof(ThumbRec)),
                 o_b0 = ws.add((size_t)slots * flat_words * 8), o_rowv = ws.add((size_t)slots * px * 2), o_blur = ws.add(bit_words * 8),
                 o_dil = ws.add(bit_words * 8);
    int rc;
    ctx->cap_src.filled = false;
    if ((rc = ws.reserve()) || (rc = d2r_reserve(ctx, ctx->thumb_out, (size_t)P.total))) return rc;
    D2rStageTimer &timer = ctx->thumb_timer[1];
    if ((rc = timer.mark(ctx, 0)) || (rc = ws.upload(o_noise, noise_u8, px * 3))) return rc;
    if (!recs.empty() && (rc = ws.upload(o_recs, recs.data(), recs.size() * sizeof(ThumbRec)))) return rc;
    if (slots && (rc = ws.upload(o_srecs, slot_recs.data(), slots * sizeof(ThumbRec)))) return rc;
    if ((rc = timer.mark(ctx, 1))) return rc;
    const uint8_t *d_rgb = (const uint8_t *)ctx->thumb_in.p + P.o_rgb, *d_mask = (const uint8_t *)ctx->thumb_in.p + P.o_mask,
                  *d_oob = (const uint8_t *)ctx->thumb_in.p + P.o_oob;
    if (slots) {
        hipLaunchKernelGGL(k_thumb_pack, dim3((uint32_t)((flat_words + 3) / 4), slots), dim3(MK_THREADS), 0, ctx->stream, d_mask, d_oob,
                           ws.at<const ThumbRec>(o_srecs), (int)w, (int)h, (int)ww, ws.at<unsigned long long>(o_b0));
        thumbs_blur_dilate(ctx, ws.at<unsigned long long>(o_b0), ws.at<uint16_t>(o_rowv), ws.at<unsigned long long>(o_blur),
                           ws.at<unsigned long long>(o_dil), ws.at<const ThumbRec>(o_srecs), slots, n_rot, w, h, P.dilate_k);
    }
    if (!recs.empty())
        hipLaunchKernelGGL(k_thumb_compose, dim3(((max_px + 3) / 4 + MK_THREADS - 1) / MK_THREADS, (uint32_t)recs.size()), dim3(MK_THREADS), 0,
                           ctx->stream, d_rgb, d_mask, d_oob, ws.at<const uint8_t>(o_noise), ws.at<const ThumbRec>(o_recs), (int)w, (int)h, (int)ww,
                           (int)hw, ws.at<const unsigned long long>(o_dil), (uint8_t *)ctx->thumb_out.p);
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = timer.mark(ctx, 2))) return rc;
    if (P.total) D2R_HIP(ctx, hipMemcpyAsync(out_u8, ctx->thumb_out.p, (size_t)P.total, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = timer.mark(ctx, 3))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));         // the host vectors above were read by then
    timer.done();
    // the packed thumbnails stay in thumb_out until the next plan: captions.hip reads them there
    D2rCaptionSrc &C = ctx->cap_src;
    C.recs.clear();
    for (const ThumbRec &r : recs) {
        const uint32_t five[5] = {r.obj - 1, r.rows, r.cols, (uint32_t)r.off, (uint32_t)(r.off >> 32)};
        C.recs.insert(C.recs.end(), five, five + 5);
    }
    C.n_objs = P.recs.empty() ? 0u : P.recs[P.recs.size() - D2R_THUMB_REC_WORDS];      // objects outermost: the last record's
    C.total = P.total;
    C.filled = true;
    return D2R_OK;
}

int d2r_thumbs_blur_bits(d2r_ctx *ctx, const uint8_t *bits_u8, uint32_t w, uint32_t h, uint32_t dilate_k, uint8_t *out_u8)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (!bits_u8 || !out_u8) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (dilate_k < 1 || dilate_k > 64) return d2r_fail(ctx, D2R_ERR_INVALID, "thumbnails: dilate_k must be 1 .. 64");
    int rc;
    if ((rc = masks_check_frames(ctx, 1, w, h))) return rc;
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t ww = (w + 63) / 64;
    const size_t px = (size_t)w * h, words = (size_t)h * ww;
    ctx->cap_src.filled = false;                             // thumb_out is about to hold this image
    D2rStage ws(ctx, ctx->thumb_ws);
    const size_t o_img = ws.add(px), o_b0 = ws.add(words * 8), o_rowv = ws.add(px * 2), o_blur = ws.add(words * 8), o_dil = ws.add(words * 8);
    if ((rc = ws.reserve()) || (rc = d2r_reserve(ctx, ctx->thumb_out, px)) || (rc = ws.upload(o_img, bits_u8, px))) return rc;
    hipLaunchKernelGGL(k_thumb_pack, dim3((uint32_t)((words + 3) / 4), 1), dim3(MK_THREADS), 0, ctx->stream, ws.at<const uint8_t>(o_img),
                       (const uint8_t *)nullptr, (const ThumbRec *)nullptr, (int)w, (int)h, (int)ww, ws.at<unsigned long long>(o_b0));
    thumbs_blur_dilate(ctx, ws.at<unsigned long long>(o_b0), ws.at<uint16_t>(o_rowv), ws.at<unsigned long long>(o_blur),
                       ws.at<unsigned long long>(o_dil), nullptr, 1, 0, w, h, dilate_k);
    hipLaunchKernelGGL(k_unpack, dim3((uint32_t)(((size_t)h * ((w + 7) / 8) + MK_THREADS - 1) / MK_THREADS), 1), dim3(MK_THREADS), 0, ctx->stream,
                       ws.at<const unsigned long long>(o_dil), (int)w, (int)h, (int)ww, (uint8_t *)ctx->thumb_out.p);
    D2R_HIP(ctx, hipGetLastError());
    D2R_HIP(ctx, hipMemcpyAsync(out_u8, ctx->thumb_out.p, px, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t e = 0; e < px; ++e) out_u8[e] &= 1;          // k_unpack writes 0 / 255
    return D2R_OK;
}

int d2r_thumbs_get_timing(d2r_ctx *ctx, double *ms_out)
{
    if (!ctx || !ms_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    double plan[3], fill[3];
    int rc;
    if ((rc = ctx->thumb_timer[0].read(ctx, plan, 3, "thumbnails timing: no d2r_thumbs_plan has run on this context")) ||
        (rc = ctx->thumb_timer[1].read(ctx, fill, 3, "thumbnails timing: no d2r_thumbs_fill has run on this context")))
        return rc;
    for (int k = 0; k < 3; ++k) ms_out[k] = plan[k] + fill[k];
    return D2R_OK;
}

}  // extern "C"
