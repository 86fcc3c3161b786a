// proposals.hip — mask proposals to the first frame's label image: the post-processing of the reference's Segmentor.segment
// (segmentation/sam_seg.py:80-115: scene-bound AND, the disconnected / large / subpart / small rules, each a cv2 call per mask on
// the CPU) and integrate_masks (segmentation/XMem_infer.py:256-261).  The rule is DESIGN.md section 2h, restated in numpy by
// tests/proposals_ref.py and held to it bit for bit.  Integer arithmetic only; every sum, maximum and flag is order-free.
//   k_prop_pack         M proposals -> rows of 64-bit words, AND with the scene mask, the area's popcount: one read of the bytes
//   k_morph<false>      (masks_shared.h) the 5 x 5 dilation of every plane of a pass
//   k_label_tiles / k_label_seams / k_label_flatten   (masks_shared.h) the labeller of masks.hip over BitSrc: a 64 x 16 tile is one
//                       word of 16 rows, straight from the bits; a root's boundary counter starts at zero
//   k_prop_roots        components of a dilated plane = its roots after tiles and seams
//   k_prop_boundary     boundary pixels (a set pixel with an unset 4-neighbour; outside the image reads unset) counted at their root
//                       (wave_each_root, masks_shared.h)
//   k_prop_best         the component with the most boundary pixels, ties to the lowest first pixel: one 64-bit atomicMax
//   k_prop_geometry     one workgroup per mask: the chosen component's leftmost / rightmost pixel per row, a monotone chain over them
//                       (serial), every hull edge's extents across the lanes, the smallest rectangle by an exact 128-bit compare
//   k_prop_prefilter    stages 1 and 2 and the ordered list of their survivors
//   k_prop_pairs        |P[i] & P[j]|: a workgroup per 8 x 8 tile of survivor pairs streams both groups' words through LDS once
//   k_prop_select       stages 3 and 4, the labels, the records (one workgroup: M^2 flag logic)
//   k_prop_compose      the label image: the highest label whose mask covers the pixel
// Every value is written by ordinary vector stores from C++.
#include <string.h>

#include <algorithm>

#include "d2r_internal.h"
#include "masks_shared.h"

namespace {

constexpr size_t PR_WS_BUDGET = (size_t)1 << 30;          // labelling workspace per pass of masks (D2R_PROPOSALS_WS_BYTES overrides it)
constexpr int PR_TILE = 8;                                // k_prop_pairs: masks per side of a tile of pairs
constexpr int PR_CHUNK = 128;                             // ... words of a mask per trip through LDS
constexpr uint32_t PR_NONE = 0xffffffffu;
constexpr int GEO_WORDS = 4;                              // per mask: boundary pixels of the chosen component, ew, eh, dd

// one wave per word of 64 pixels of proposal blockIdx.y; area[m] += the word's popcount
__global__ __launch_bounds__(MK_THREADS) void k_prop_pack(const uint8_t *__restrict__ props, const uint8_t *__restrict__ inside, int W, int H, int WW,
                                                          unsigned long long *__restrict__ bits, uint32_t *__restrict__ area)
{
    WordLane p;
    if (!d2r_word_lane(H, WW, p)) return;
    bool set = false;
    if (p.j < W) {
        const size_t at = (size_t)p.i * W + p.j;
        set = props[(size_t)blockIdx.y * W * H + at] != 0 && (!inside || inside[at] != 0);
    }
    const unsigned long long m = word_pack(p, set, bits + (size_t)blockIdx.y * H * WW);
    if (p.lane == 0 && m) atomicAdd(&area[blockIdx.y], (uint32_t)__popcll(m));
}

// ncomp[mask] += the plane's roots after k_label_tiles and k_label_seams (a wave's roots in one add)
__global__ __launch_bounds__(MK_THREADS) void k_prop_roots(const unsigned long long *__restrict__ bits, int W, int H, int WW,
                                                           uint32_t *__restrict__ parent, uint32_t *__restrict__ ncomp)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    bool is_root = false;
    if (g < (uint32_t)W * (uint32_t)H) {
        const int i = (int)(g / (uint32_t)W), j = (int)(g - (uint32_t)i * (uint32_t)W);
        if (plane_bit(bits + (size_t)blockIdx.y * H * WW, WW, i, j))
            is_root = __hip_atomic_load(&parent[(size_t)blockIdx.y * W * H + g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g;
    }
    const unsigned long long roots = __ballot(is_root);
    if (roots && (threadIdx.x & 63) == 0) atomicAdd(&ncomp[blockIdx.y], (uint32_t)__popcll(roots));
}

// one wave per word: the word's boundary bits from its four neighbours, counted at the pixels' roots (equal roots of a wave in one add)
__global__ __launch_bounds__(MK_THREADS) void k_prop_boundary(const unsigned long long *__restrict__ bits, int W, int H, int WW,
                                                              const uint32_t *__restrict__ parent, uint32_t *__restrict__ bcnt)
{
    WordLane p;
    if (!d2r_word_lane(H, WW, p)) return;
    const unsigned long long *b = bits + (size_t)blockIdx.y * H * WW;
    const unsigned long long v = b[p.word];
    if (!v) return;                                         // wave-uniform
    const unsigned long long up = p.i > 0 ? b[p.word - WW] : 0ull, down = p.i + 1 < H ? b[p.word + WW] : 0ull;
    const unsigned long long prev = p.w > 0 ? b[p.word - 1] : 0ull, next = p.w + 1 < WW ? b[p.word + 1] : 0ull;
    const unsigned long long lft = (v << 1) | (prev >> 63), rgt = (v >> 1) | (next << 63);      // bit j = the pixel at j - 1, at j + 1
    const unsigned long long edge = v & ~(up & down & lft & rgt);
    const size_t base = (size_t)blockIdx.y * W * H;
    const bool active = (edge >> p.lane) & 1ull;
    const uint32_t root = active ? parent[base + (size_t)p.i * W + p.j] : PR_NONE;
    wave_each_root(active, root, [&](uint32_t r0, unsigned long long members, bool leader) {
        if (leader) atomicAdd(&bcnt[base + r0], (uint32_t)__popcll(members));
    });
}

// best[mask] = max over its components of (boundary pixels << 32 | ~first pixel): the most boundary pixels, then the lowest raster index
__global__ __launch_bounds__(MK_THREADS) void k_prop_best(const unsigned long long *__restrict__ bits, int W, int H, int WW,
                                                          const uint32_t *__restrict__ parent, const uint32_t *__restrict__ bcnt,
                                                          unsigned long long *__restrict__ best)
{
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    if (g >= (uint32_t)W * (uint32_t)H) return;
    const int i = (int)(g / (uint32_t)W), j = (int)(g - (uint32_t)i * (uint32_t)W);
    const size_t base = (size_t)blockIdx.y * W * H;
    if (!plane_bit(bits + (size_t)blockIdx.y * H * WW, WW, i, j) || parent[base + g] != g) return;
    atomicMax(&best[blockIdx.y], (unsigned long long)bcnt[base + g] << 32 | (unsigned long long)(PR_NONE - g));
}

// a point is x | y << 16 (x, y < 8192)
__device__ inline int pt_x(uint32_t p) { return (int)(p & 0xffffu); }
__device__ inline int pt_y(uint32_t p) { return (int)(p >> 16); }
// (a - o) x (b - o): below 2^28 in magnitude
__device__ inline int pt_cross(uint32_t o, uint32_t a, uint32_t b)
{
    return (pt_x(a) - pt_x(o)) * (pt_y(b) - pt_y(o)) - (pt_y(a) - pt_y(o)) * (pt_x(b) - pt_x(o));
}

// ew1 eh1 / dd1 < ew2 eh2 / dd2, exactly: ew eh < 2^56 and dd < 2^28, the cross products compared as 128-bit integers
__device__ inline bool rect_less(uint32_t ew1, uint32_t eh1, uint32_t dd1, uint32_t ew2, uint32_t eh2, uint32_t dd2)
{
    const unsigned long long a1 = (unsigned long long)ew1 * eh1, a2 = (unsigned long long)ew2 * eh2;
    const unsigned long long h1 = __umul64hi(a1, (unsigned long long)dd2), l1 = a1 * dd2, h2 = __umul64hi(a2, (unsigned long long)dd1), l2 = a2 * dd1;
    return h1 < h2 || (h1 == h2 && l1 < l2);
}

// Workgroup blockIdx.x = one mask of the pass.  ext: [masks][H] row extents (left | right << 16, PR_NONE for a row without a pixel
// of the chosen component); hull: [masks][4 H + 2] points (each chain holds at most the 2 H row
// extents).  geo[mask] = boundary pixels, ew, eh, dd (zeros for an empty mask;
// ew = eh = dd = 0 for a hull of one or two vertices).
__global__ __launch_bounds__(MK_THREADS) void k_prop_geometry(const unsigned long long *__restrict__ bits, int W, int H, int WW,
                                                              const uint32_t *__restrict__ parent, const unsigned long long *__restrict__ best,
                                                              uint32_t *__restrict__ ext_ws, uint32_t *__restrict__ hull_ws, uint32_t *__restrict__ geo)
{
    __shared__ uint32_t s_n;
    __shared__ uint32_t s_k[MK_THREADS], s_ew[MK_THREADS], s_eh[MK_THREADS], s_dd[MK_THREADS];
    const int t = (int)threadIdx.x;
    const unsigned long long key = best[blockIdx.x];
    uint32_t *out = geo + (size_t)blockIdx.x * GEO_WORDS;
    if (key == 0) {                                         // an empty mask: no component
        if (t < GEO_WORDS) out[t] = 0;
        return;
    }
    const uint32_t root = PR_NONE - (uint32_t)key;
    const unsigned long long *b = bits + (size_t)blockIdx.x * H * WW;
    const uint32_t *par = parent + (size_t)blockIdx.x * W * H;
    uint32_t *ext = ext_ws + (size_t)blockIdx.x * H, *hull = hull_ws + (size_t)blockIdx.x * (4 * (size_t)H + 2);
    for (int i = t; i < H; i += (int)MK_THREADS) {
        int lo = -1, hi = -1;
        for (int w = 0; w < WW && lo < 0; ++w) {
            unsigned long long v = b[(size_t)i * WW + w];
            while (v) {
                const int j = w * 64 + __ffsll((long long)v) - 1;
                if (par[(size_t)i * W + j] == root) {
                    lo = j;
                    break;
                }
                v &= v - 1;
            }
        }
        for (int w = WW - 1; w >= 0 && lo >= 0 && hi < 0; --w) {
            unsigned long long v = b[(size_t)i * WW + w];
            while (v) {
                const int bit = 63 - __clzll((long long)v), j = w * 64 + bit;
                if (par[(size_t)i * W + j] == root) {
                    hi = j;
                    break;
                }
                v &= ~(1ull << bit);
            }
        }
        ext[i] = lo < 0 ? PR_NONE : (uint32_t)lo | (uint32_t)hi << 16;
    }
    __syncthreads();                                        // a workgroup's global writes are visible to it after the barrier
    if (t == 0) {
        // Andrew's monotone chain over the points in (y, x) order: a turn with cross <= 0 is popped, so the hull is strictly convex
        uint32_t n = 0, npts = 0;
        for (int i = 0; i < H; ++i) {
            const uint32_t e = ext[i];
            if (e == PR_NONE) continue;
            const uint32_t y = (uint32_t)i << 16, pl = (e & 0xffffu) | y, pr = (e >> 16) | y;
            for (int s = 0; s < (pl == pr ? 1 : 2); ++s) {
                const uint32_t p = s ? pr : pl;
                while (n >= 2 && pt_cross(hull[n - 2], hull[n - 1], p) <= 0) --n;
                hull[n++] = p;
                ++npts;
            }
        }
        if (npts > 1) {
            const uint32_t base = --n;                      // the first chain without its last point, which starts the second
            for (int i = H - 1; i >= 0; --i) {
                const uint32_t e = ext[i];
                if (e == PR_NONE) continue;
                const uint32_t y = (uint32_t)i << 16, pl = (e & 0xffffu) | y, pr = (e >> 16) | y;
                for (int s = 0; s < (pl == pr ? 1 : 2); ++s) {
                    const uint32_t p = s ? pl : pr;
                    while (n - base >= 2 && pt_cross(hull[n - 2], hull[n - 1], p) <= 0) --n;
                    hull[n++] = p;
                }
            }
            --n;                                            // ... and the second without its last, the hull's first vertex
        }
        s_n = n;
    }
    __syncthreads();
    const uint32_t n = s_n;
    if (n < 3) {
        if (t == 0) {
            out[0] = (uint32_t)(key >> 32);
            out[1] = out[2] = out[3] = 0;
        }
        return;
    }
    uint32_t bk = PR_NONE, bew = 0, beh = 0, bdd = 1;
    for (uint32_t k = (uint32_t)t; k < n; k += MK_THREADS) {
        const uint32_t a = hull[k], c = hull[k + 1 == n ? 0 : k + 1];
        const int dx = pt_x(c) - pt_x(a), dy = pt_y(c) - pt_y(a);
        int dmin = 0x7fffffff, dmax = -0x7fffffff, nmin = 0x7fffffff, nmax = -0x7fffffff;
        for (uint32_t v = 0; v < n; ++v) {
            const uint32_t p = hull[v];
            const int dp = dx * pt_x(p) + dy * pt_y(p), np = -dy * pt_x(p) + dx * pt_y(p);
            dmin = min(dmin, dp); dmax = max(dmax, dp);
            nmin = min(nmin, np); nmax = max(nmax, np);
        }
        const uint32_t ew = (uint32_t)(dmax - dmin), eh = (uint32_t)(nmax - nmin), dd = (uint32_t)(dx * dx + dy * dy);
        if (bk == PR_NONE || rect_less(ew, eh, dd, bew, beh, bdd)) {
            bk = k; bew = ew; beh = eh; bdd = dd;
        }
    }
    s_k[t] = bk; s_ew[t] = bew; s_eh[t] = beh; s_dd[t] = bdd;
    __syncthreads();
    if (t == 0) {                                           // the smallest area; among equals the first edge
        for (uint32_t q = 1; q < MK_THREADS; ++q) {
            if (s_k[q] == PR_NONE) continue;
            if (rect_less(s_ew[q], s_eh[q], s_dd[q], bew, beh, bdd) || (!rect_less(bew, beh, bdd, s_ew[q], s_eh[q], s_dd[q]) && s_k[q] < bk)) {
                bk = s_k[q]; bew = s_ew[q]; beh = s_eh[q]; bdd = s_dd[q];
            }
        }
        out[0] = (uint32_t)(key >> 32);
        out[1] = bew;
        out[2] = beh;
        out[3] = bdd;
    }
}

// stage12[m] = 1 unless the dilation has exactly one component, else 2 when 10 area > 3 H W, else 0; surv = the masks with 0, in
// order, *n_surv their number.  One workgroup.
__global__ __launch_bounds__(MK_THREADS) void k_prop_prefilter(const uint32_t *__restrict__ area, const uint32_t *__restrict__ ncomp, uint32_t M,
                                                               unsigned long long px, uint32_t *__restrict__ stage12, uint32_t *__restrict__ surv,
                                                               uint32_t *__restrict__ n_surv)
{
    __shared__ uint8_t st[D2R_PROP_MAX];
    for (uint32_t m = threadIdx.x; m < M; m += MK_THREADS) {
        const uint32_t s = ncomp[m] != 1u ? 1u : (10ull * area[m] > 3ull * px ? 2u : 0u);
        st[m] = (uint8_t)s;
        stage12[m] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t n = 0;
        for (uint32_t m = 0; m < M; ++m)
            if (!st[m]) surv[n++] = m;
        *n_surv = n;
    }
}

// inter[i][j] = |P[i] & P[j]| for the survivors surv[PR_TILE bx ..] x surv[PR_TILE by ..], i < j.  Wave s of the workgroup sums
// every fourth word of a chunk for all 64 pairs of the tile (lane = pair); the four partial sums meet in LDS.
__global__ __launch_bounds__(MK_THREADS) void k_prop_pairs(const unsigned long long *__restrict__ bits, size_t words, uint32_t M,
                                                           const uint32_t *__restrict__ surv, const uint32_t *__restrict__ n_surv,
                                                           uint32_t *__restrict__ inter)
{
    __shared__ unsigned long long A[PR_TILE][PR_CHUNK + 1], B[PR_TILE][PR_CHUNK + 1];
    __shared__ uint32_t ia[PR_TILE], ib[PR_TILE], acc[PR_TILE * PR_TILE];
    const uint32_t n2 = *n_surv, k0 = blockIdx.x * PR_TILE, l0 = blockIdx.y * PR_TILE;
    if (blockIdx.x > blockIdx.y || l0 >= n2) return;        // k0 <= l0
    const int t = (int)threadIdx.x;
    if (t < PR_TILE) {
        ia[t] = k0 + t < n2 ? surv[k0 + t] : PR_NONE;
        ib[t] = l0 + t < n2 ? surv[l0 + t] : PR_NONE;
    }
    if (t < PR_TILE * PR_TILE) acc[t] = 0;
    __syncthreads();
    const int pair = t & 63, pa = pair / PR_TILE, pb = pair - pa * PR_TILE, sub = t >> 6;
    uint32_t sum = 0;
    for (size_t c0 = 0; c0 < words; c0 += PR_CHUNK) {
        for (int q = t; q < PR_TILE * PR_CHUNK; q += (int)MK_THREADS) {
            const int r = q / PR_CHUNK, c = q - r * PR_CHUNK;
            const bool in = c0 + c < words;
            A[r][c] = in && ia[r] != PR_NONE ? bits[(size_t)ia[r] * words + c0 + c] : 0ull;
            B[r][c] = in && ib[r] != PR_NONE ? bits[(size_t)ib[r] * words + c0 + c] : 0ull;
        }
        __syncthreads();
        for (int c = sub; c < PR_CHUNK; c += (int)MK_THREADS / 64) sum += (uint32_t)__popcll(A[pa][c] & B[pb][c]);
        __syncthreads();
    }
    atomicAdd(&acc[pair], sum);
    __syncthreads();
    if (t < PR_TILE * PR_TILE && ia[pa] != PR_NONE && ib[pb] != PR_NONE && k0 + pa < l0 + pb) inter[(size_t)ia[pa] * M + ib[pb]] = acc[t];
}

// stage 3 (every pair of survivors marks its smaller mask, marked ones still mark), stage 4, labels in order, the records.
// status[0] = the number of survivors; lab2mask[l - 1] = the mask of label l <= 255.  One workgroup.
__global__ __launch_bounds__(MK_THREADS) void k_prop_select(const uint32_t *__restrict__ area, const uint32_t *__restrict__ ncomp,
                                                            const uint32_t *__restrict__ stage12, const uint32_t *__restrict__ surv,
                                                            const uint32_t *__restrict__ n_surv, const uint32_t *__restrict__ inter,
                                                            const uint32_t *__restrict__ geo, uint32_t M, uint32_t *__restrict__ recs,
                                                            uint32_t *__restrict__ lab2mask, uint32_t *__restrict__ status)
{
    __shared__ uint32_t marked[D2R_PROP_MAX], fin[D2R_PROP_MAX], lab[D2R_PROP_MAX];
    const uint32_t n2 = *n_surv;
    for (uint32_t m = threadIdx.x; m < M; m += MK_THREADS) marked[m] = 0;
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n2; k += MK_THREADS) {
        const uint32_t i = surv[k];
        const unsigned long long ai = area[i];
        for (uint32_t l = k + 1; l < n2; ++l) {
            const uint32_t j = surv[l];
            const unsigned long long aj = area[j], it10 = 10ull * inter[(size_t)i * M + j];
            if (it10 > ai || it10 > aj) atomicOr(&marked[ai < aj ? i : j], 1u);
        }
    }
    __syncthreads();
    for (uint32_t m = threadIdx.x; m < M; m += MK_THREADS) {
        uint32_t s = stage12[m];
        if (!s && marked[m]) s = 3;
        if (!s) {
            const uint32_t *g = geo + (size_t)m * GEO_WORDS;
            const unsigned long long side = min(g[1], g[2]);
            if (area[m] < 80u || !(side * side > 400ull * g[3])) s = 4;
        }
        fin[m] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t n = 0;
        for (uint32_t m = 0; m < M; ++m) {
            lab[m] = 0;
            if (fin[m]) continue;
            if (n < 255u) lab2mask[n] = m;
            lab[m] = ++n;
        }
        status[0] = n;
    }
    __syncthreads();
    for (uint32_t m = threadIdx.x; m < M; m += MK_THREADS) {
        uint32_t *r = recs + (size_t)m * D2R_PROP_REC_WORDS;
        const uint32_t *g = geo + (size_t)m * GEO_WORDS;
        r[0] = area[m];
        r[1] = ncomp[m];
        r[2] = fin[m];
        r[3] = lab[m];
        r[4] = g[0];
        r[5] = g[1];
        r[6] = g[2];
        r[7] = g[3];
    }
}

// one wave per word, a pixel per lane: labels from the highest down until every pixel of the word has one
__global__ __launch_bounds__(MK_THREADS) void k_prop_compose(const unsigned long long *__restrict__ bits, int W, int H, int WW,
                                                             const uint32_t *__restrict__ lab2mask, const uint32_t *__restrict__ status,
                                                             uint8_t *__restrict__ out)
{
    WordLane p;
    if (!d2r_word_lane(H, WW, p)) return;
    const uint32_t n = status[0];
    if (n > 255u) return;                                   // the call fails; nothing is read back
    const size_t words = (size_t)H * WW;
    unsigned long long open = (W - p.w * 64) >= 64 ? ~0ull : ((1ull << (W - p.w * 64)) - 1ull);      // pixels of the word without a label yet
    uint32_t label = 0;
    for (uint32_t l = n; l > 0 && open; --l) {
        const unsigned long long v = bits[(size_t)lab2mask[l - 1] * words + p.word] & open;
        if ((v >> p.lane) & 1ull) label = l;
        open &= ~v;
    }
    if (p.j < W) out[(size_t)p.i * W + p.j] = (uint8_t)label;
}

}  // namespace

extern "C" {

int d2r_proposals_labels(d2r_ctx *ctx, const uint8_t *props_u8, const uint8_t *inside_u8, uint32_t m, uint32_t w, uint32_t h, uint8_t *labels_out,
                         uint32_t *recs_out, uint32_t *inter_out)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (!labels_out || (m && !props_u8)) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (m > D2R_PROP_MAX) return d2r_fail(ctx, D2R_ERR_INVALID, "proposals: at most " + std::to_string(D2R_PROP_MAX) + " proposals per call");
    if (w == 0 || h == 0 || w > D2R_PROP_MAX_SIDE || h > D2R_PROP_MAX_SIDE)
        return d2r_fail(ctx, D2R_ERR_INVALID, "proposals: width and height must be 1 .. " + std::to_string(D2R_PROP_MAX_SIDE));
    const size_t px = (size_t)w * h;
    if ((uint64_t)m * px >= (1ull << 32)) return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "proposals: the proposals must have fewer than 2^32 pixels in all");
    if (m == 0) {
        memset(labels_out, 0, px);
        return D2R_OK;
    }
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ww = (w + 63) / 64, words = (size_t)h * ww;
    // masks per pass of the labelling: a pixel costs a parent and a boundary counter, a word its dilated plane
    const uint32_t per = pass_items("D2R_PROPOSALS_WS_BYTES", PR_WS_BUDGET, m, px * 8 + words * 8 + ((size_t)h * 5 + 2) * 4);
    D2rStage in(ctx, ctx->prop_in), ws(ctx, ctx->prop_ws);
    const size_t o_props = in.add((size_t)m * px), o_inside = in.add(inside_u8 ? px : 0);
    // the first four segments are cleared together: area, ncomp, best, inter
    const size_t o_area = ws.add((size_t)m * 4), o_ncomp = ws.add((size_t)m * 4), o_best = ws.add((size_t)m * 8), o_inter = ws.add((size_t)m * m * 4);
    const size_t clear_end = ws.total();
    const size_t o_bits = ws.add((size_t)m * words * 8), o_dil = ws.add((size_t)per * words * 8), o_parent = ws.add((size_t)per * px * 4),
                 o_bcnt = ws.add((size_t)per * px * 4), o_ext = ws.add((size_t)per * h * 4), o_hull = ws.add((size_t)per * (4 * (size_t)h + 2) * 4),
                 o_geo = ws.add((size_t)m * GEO_WORDS * 4), o_stage = ws.add((size_t)m * 4), o_surv = ws.add((size_t)m * 4), o_nsurv = ws.add(4),
                 o_recs = ws.add((size_t)m * D2R_PROP_REC_WORDS * 4), o_lab = ws.add(256 * 4), o_status = ws.add(4);
    int rc;
    if ((rc = in.reserve()) || (rc = ws.reserve()) || (rc = d2r_reserve(ctx, ctx->prop_out, px))) return rc;
    D2rStageTimer &timer = ctx->prop_timer;
    if ((rc = timer.mark(ctx, 0)) || (rc = in.upload(o_props, props_u8, (size_t)m * px))) return rc;
    if (inside_u8 && (rc = in.upload(o_inside, inside_u8, px))) return rc;
    if ((rc = timer.mark(ctx, 1))) return rc;
    const int W = (int)w, H = (int)h, WW = (int)ww;
    uint32_t *d_area = ws.at<uint32_t>(o_area), *d_ncomp = ws.at<uint32_t>(o_ncomp), *d_inter = ws.at<uint32_t>(o_inter);
    unsigned long long *d_best = ws.at<unsigned long long>(o_best), *d_bits = ws.at<unsigned long long>(o_bits), *d_dil = ws.at<unsigned long long>(o_dil);
    uint32_t *d_parent = ws.at<uint32_t>(o_parent), *d_bcnt = ws.at<uint32_t>(o_bcnt), *d_geo = ws.at<uint32_t>(o_geo);
    uint32_t *d_stage = ws.at<uint32_t>(o_stage), *d_surv = ws.at<uint32_t>(o_surv), *d_nsurv = ws.at<uint32_t>(o_nsurv);
    uint32_t *d_recs = ws.at<uint32_t>(o_recs), *d_lab = ws.at<uint32_t>(o_lab), *d_status = ws.at<uint32_t>(o_status);
    const dim3 T(MK_THREADS);
    const uint32_t gw = (uint32_t)((words + 3) / 4), gpx = (uint32_t)((px + MK_THREADS - 1) / MK_THREADS);
    D2R_HIP(ctx, hipMemsetAsync(ws.at<char>(o_area), 0, clear_end - o_area, ctx->stream));
    hipLaunchKernelGGL(k_prop_pack, dim3(gw, m), T, 0, ctx->stream, in.at<const uint8_t>(o_props),
                       inside_u8 ? in.at<const uint8_t>(o_inside) : (const uint8_t *)nullptr, W, H, WW, d_bits, d_area);
    for (uint32_t m0 = 0; m0 < m; m0 += per) {              // passes share the workspace; nothing waits in between
        const uint32_t nm = std::min(per, m - m0);
        const unsigned long long *raw = d_bits + (size_t)m0 * words;
        hipLaunchKernelGGL(k_morph<false>, dim3((uint32_t)((ww + CL_TW - 1) / CL_TW), (h + CL_TR - 1) / CL_TR, nm), T, 0, ctx->stream, raw, d_dil, W, H, WW, 5);
        label_unite(ctx, BitSrc{d_dil, W, H, WW}, nm, d_parent);
        hipLaunchKernelGGL(k_prop_roots, dim3(gpx, nm), T, 0, ctx->stream, (const unsigned long long *)d_dil, W, H, WW, d_parent, d_ncomp + m0);
        label_components(ctx, BitSrc{raw, W, H, WW}, nm, d_parent, d_bcnt, 4);
        hipLaunchKernelGGL(k_prop_boundary, dim3(gw, nm), T, 0, ctx->stream, raw, W, H, WW, (const uint32_t *)d_parent, d_bcnt);
        hipLaunchKernelGGL(k_prop_best, dim3(gpx, nm), T, 0, ctx->stream, raw, W, H, WW, (const uint32_t *)d_parent, (const uint32_t *)d_bcnt, d_best + m0);
        hipLaunchKernelGGL(k_prop_geometry, dim3(nm), T, 0, ctx->stream, raw, W, H, WW, (const uint32_t *)d_parent, (const unsigned long long *)(d_best + m0),
                           ws.at<uint32_t>(o_ext), ws.at<uint32_t>(o_hull), d_geo + (size_t)m0 * GEO_WORDS);
    }
    hipLaunchKernelGGL(k_prop_prefilter, dim3(1), T, 0, ctx->stream, (const uint32_t *)d_area, (const uint32_t *)d_ncomp, m, (unsigned long long)px, d_stage,
                       d_surv, d_nsurv);
    const uint32_t tiles = (m + PR_TILE - 1) / PR_TILE;
    hipLaunchKernelGGL(k_prop_pairs, dim3(tiles, tiles), T, 0, ctx->stream, (const unsigned long long *)d_bits, words, m, (const uint32_t *)d_surv,
                       (const uint32_t *)d_nsurv, d_inter);
    hipLaunchKernelGGL(k_prop_select, dim3(1), T, 0, ctx->stream, (const uint32_t *)d_area, (const uint32_t *)d_ncomp, (const uint32_t *)d_stage,
                       (const uint32_t *)d_surv, (const uint32_t *)d_nsurv, (const uint32_t *)d_inter, (const uint32_t *)d_geo, m, d_recs, d_lab, d_status);
    hipLaunchKernelGGL(k_prop_compose, dim3(gw), T, 0, ctx->stream, (const unsigned long long *)d_bits, W, H, WW, (const uint32_t *)d_lab,
                       (const uint32_t *)d_status, (uint8_t *)ctx->prop_out.p);
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = timer.mark(ctx, 2))) return rc;
    uint32_t survivors = 0;                                 // checked before anything reaches the caller's arrays
    D2R_HIP(ctx, hipMemcpyAsync(&survivors, d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (survivors > 255)
        return d2r_fail(ctx, D2R_ERR_INVALID, "proposals: " + std::to_string(survivors) + " proposals survive, a label image holds at most 255");
    D2R_HIP(ctx, hipMemcpyAsync(labels_out, ctx->prop_out.p, px, hipMemcpyDeviceToHost, ctx->stream));
    if (recs_out) D2R_HIP(ctx, hipMemcpyAsync(recs_out, d_recs, (size_t)m * D2R_PROP_REC_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (inter_out) D2R_HIP(ctx, hipMemcpyAsync(inter_out, d_inter, (size_t)m * m * 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = timer.mark(ctx, 3))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    timer.done();
    return D2R_OK;
}

int d2r_proposals_get_timing(d2r_ctx *ctx, double *ms_out)
{
    if (!ctx || !ms_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    return ctx->prop_timer.read(ctx, ms_out, 3, "proposals timing: no d2r_proposals_labels with proposals has run on this context");
}

}  // extern "C"
