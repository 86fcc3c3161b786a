// What the mask units (masks.hip, proposals.hip) share: the workgroup size, the one-wave-per-word indexing and ballot pack, the
// single-bit read, the bit-packed k x k morphology on rows of 64-bit words, the lock-free union-find, the
// component labeller over a pixel source (bytes or bits) with its launcher, the per-root wave loop and the workspace budget of a
// pass.  A piece moves here when the second unit needs it.  Comes after d2r_internal.h.
#pragma once
#include <stdlib.h>

#include <algorithm>

#include "d2r_internal.h"

namespace {

constexpr uint32_t MK_THREADS = 256;
constexpr int CL_TW = 4, CL_TR = 64, CL_ROWS = 128;      // k_morph: words x output rows of a tile, rows held (CL_TR + 63 <= CL_ROWS)
constexpr int LB_TW = 64, LB_TH = 16, LB_PX = LB_TW * LB_TH;   // k_label_tiles: tile of the per-tile labelling
constexpr uint32_t NO_KEY = 0xffffffffu;

// items per pass over a shared workspace: as many as fit the budget, at least one.  The environment variable lowers (or raises)
// the budget, so that a test can drive a small batch through several passes.
inline uint32_t pass_items(const char *env, size_t budget, size_t n, size_t bytes_per_item)
{
    if (const char *v = getenv(env)) {
        char *end = nullptr;
        const unsigned long long b = strtoull(v, &end, 10);
        if (end != v && *end == 0 && b > 0) budget = (size_t)b;
    }
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(n, budget / bytes_per_item));
}

// bit (i, j) of a plane of rows of WW words
__device__ inline bool plane_bit(const unsigned long long *__restrict__ bits, int WW, int i, int j)
{
    return (bits[(size_t)i * WW + (j >> 6)] >> (j & 63)) & 1ull;
}

// One wave per word of 64 pixels, four words per workgroup along blockIdx.x: the wave's word of an H x WW plane, its row i and
// word w of the row, the lane's pixel j = 64 w + lane (which may lie past the row's end).  False past the plane: wave-uniform.
struct WordLane {
    uint32_t word;
    int i, w, lane, j;
};
__device__ inline bool d2r_word_lane(int H, int WW, WordLane &p)
{
    p.word = blockIdx.x * (MK_THREADS / 64) + (threadIdx.x >> 6);
    if (p.word >= (uint32_t)H * (uint32_t)WW) return false;
    p.i = (int)(p.word / (uint32_t)WW);
    p.w = (int)(p.word - (uint32_t)p.i * (uint32_t)WW);
    p.lane = (int)(threadIdx.x & 63);
    p.j = p.w * 64 + p.lane;
    return true;
}
// the lanes' bits as the wave's word of `plane`, written by lane 0; every lane gets the word
__device__ inline unsigned long long word_pack(const WordLane &p, bool set, unsigned long long *__restrict__ plane)
{
    const unsigned long long m = __ballot(set);
    if (p.lane == 0) plane[p.word] = m;
    return m;
}

// x (192 bits, x[0] lowest) >>= s with `fill` shifted in at the top, 1 <= s <= 63
__device__ inline void shr192(const unsigned long long x[3], int s, unsigned long long fill, unsigned long long y[3])
{
    y[0] = (x[0] >> s) | (x[1] << (64 - s));
    y[1] = (x[1] >> s) | (x[2] << (64 - s));
    y[2] = (x[2] >> s) | (fill << (64 - s));
}

// dst(i, j) = OR (ERODE: AND) of src(i + a, j + b), a and b in [-k/2, -k/2 + k - 1], positions outside the frame ignored (they read
// as the operation's identity, the tail bits of a row's last word included).  A workgroup makes CL_TW words x CL_TR rows.
template <bool ERODE>
__global__ __launch_bounds__(MK_THREADS) void k_morph(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst, int W, int H,
                                                      int WW, int k)
{
    __shared__ unsigned long long buf[2][CL_ROWS][CL_TW];
    const unsigned long long ident = ERODE ? ~0ull : 0ull;
    const int t = (int)threadIdx.x, hh = k / 2;
    const int w0 = (int)blockIdx.x * CL_TW, i0 = (int)blockIdx.y * CL_TR;
    const unsigned long long *s = src + (size_t)blockIdx.z * H * WW;
    unsigned long long *o = dst + (size_t)blockIdx.z * H * WW;
    const unsigned long long tail = (W & 63) ? (~0ull << (W & 63)) : 0ull;      // the bits past the row's end in its last word
    auto ld = [&](int gi, int w) -> unsigned long long {
        if (gi < 0 || gi >= H || w < 0 || w >= WW) return ident;
        unsigned long long v = s[(size_t)gi * WW + w];
        if (w == WW - 1) v = ERODE ? (v | tail) : (v & ~tail);
        return v;
    };
    auto op = [](unsigned long long a, unsigned long long b) -> unsigned long long { return ERODE ? (a & b) : (a | b); };
    for (int q = t; q < CL_ROWS * CL_TW; q += (int)MK_THREADS) {
        const int r = q / CL_TW, cw = q - r * CL_TW, gi = i0 - hh + r, w = w0 + cw;
        unsigned long long v = ident;
        if (r < CL_TR + k - 1 && w < WW && gi >= 0 && gi < H) {
            unsigned long long x[3] = {ld(gi, w - 1), ld(gi, w), ld(gi, w + 1)}, y[3];
            // x(j) = op over src(j .. j + L - 1), L doubling up to k
            int L = 1;
            while (2 * L <= k) {
                shr192(x, L, ident, y);
                x[0] = op(x[0], y[0]); x[1] = op(x[1], y[1]); x[2] = op(x[2], y[2]);
                L *= 2;
            }
            if (k > L) {
                shr192(x, k - L, ident, y);
                x[0] = op(x[0], y[0]); x[1] = op(x[1], y[1]); x[2] = op(x[2], y[2]);
            }
            v = hh ? ((x[1] << hh) | (x[0] >> (64 - hh))) : x[1];       // the window starts k/2 to the left
        }
        buf[0][r][cw] = v;
    }
    __syncthreads();
    int cur = 0;
    auto step = [&](int sft) {
        for (int q = t; q < CL_ROWS * CL_TW; q += (int)MK_THREADS) {
            const int r = q / CL_TW, cw = q - r * CL_TW;
            const unsigned long long a = buf[cur][r][cw], bb = r + sft < CL_ROWS ? buf[cur][r + sft][cw] : ident;
            buf[cur ^ 1][r][cw] = op(a, bb);
        }
        __syncthreads();
        cur ^= 1;
    };
    int L = 1;
    while (2 * L <= k) {
        step(L);
        L *= 2;
    }
    if (k > L) step(k - L);
    for (int q = t; q < CL_TR * CL_TW; q += (int)MK_THREADS) {
        const int r = q / CL_TW, cw = q - r * CL_TW, gi = i0 + r, w = w0 + cw;
        if (gi < H && w < WW) {
            unsigned long long v = buf[cur][r][cw];       // tile row r = frame row gi - k/2: the window's first row
            if (w == WW - 1) v &= ~tail;
            o[(size_t)gi * WW + w] = v;
        }
    }
}

// Union-find where a link always goes from the larger index to the smaller: a root is the smallest index of its set whatever
// order the atomics ran in.  `par` is LDS or global memory that other lanes update with atomicMin while it is read.
template <int SCOPE>
__device__ inline uint32_t uf_find(uint32_t *par, uint32_t x)
{
    for (;;) {
        const uint32_t p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, SCOPE);
        if (p == x) return x;
        x = p;
    }
}

template <int SCOPE>
__device__ inline void uf_unite(uint32_t *par, uint32_t a, uint32_t b)
{
    for (;;) {
        a = uf_find<SCOPE>(par, a);
        b = uf_find<SCOPE>(par, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t s = a;
            a = b;
            b = s;
        }
        const uint32_t old = atomicMin(&par[a], b);       // a was a root: linked; else a's parent `old` < a still has to meet b
        if (old == a) return;
        a = old;
    }
}

// ------------------------------------------------------------------------------------------------ component labelling
// 8-connected components of equal non-zero label: parent[g] of a labelled pixel ends as the smallest raster index of its component
// (pixels of label 0 are left alone: every reader tests the label first).  A pixel source gives the tile staging in LDS with the
// "equal, non-zero label" test between two tile positions, and the label at (frame, i, j) from global memory.  Its CONN is 8, or 4
// for a source whose test is a link between a pixel and its left or upper neighbour (geoprop.hip's LinkSrc): the labeller then
// visits no diagonal, and `same`, `left` and `up` are asked about those two neighbours alone.

// byte label images [frames][H][W]: the value is the label
struct ByteSrc {
    static constexpr int CONN = 8;
    const uint8_t *img;
    int W, H;
    struct Tile {
        uint8_t lab[LB_PX];
    };
    __device__ void stage(Tile &t, uint32_t frame, int i0, int j0) const
    {
        for (int q = (int)threadIdx.x; q < LB_PX; q += (int)MK_THREADS) {
            const int r = q / LB_TW, c = q - r * LB_TW, i = i0 + r, j = j0 + c;
            t.lab[q] = (i < H && j < W) ? at(frame, i, j) : 0;
        }
    }
    __device__ static bool same(const Tile &t, int q, int n) { return t.lab[q] && t.lab[q] == t.lab[n]; }
    __device__ uint8_t at(uint32_t frame, int i, int j) const { return img[(size_t)frame * W * H + (size_t)i * W + j]; }
    // (i, j) of label l joins its left / upper neighbour
    __device__ bool left(uint32_t frame, uint8_t l, int i, int j) const { return at(frame, i, j - 1) == l; }
    __device__ bool up(uint32_t frame, uint8_t l, int i, int j) const { return at(frame, i - 1, j) == l; }
};

// bit planes [planes][H][WW], the tail bits of a row's last word 0: the value is 0 or 1, a tile is one word of LB_TH rows
struct BitSrc {
    static constexpr int CONN = 8;
    const unsigned long long *bits;
    int W, H, WW;
    struct Tile {
        unsigned long long row[LB_TH];
    };
    __device__ void stage(Tile &t, uint32_t frame, int i0, int j0) const
    {
        const int r = (int)threadIdx.x;
        if (r < LB_TH) t.row[r] = i0 + r < H ? bits[((size_t)frame * H + i0 + r) * WW + j0 / LB_TW] : 0ull;
    }
    __device__ static bool same(const Tile &t, int q, int n) { return (t.row[q / LB_TW] >> (q % LB_TW)) & (t.row[n / LB_TW] >> (n % LB_TW)) & 1ull; }
    __device__ uint8_t at(uint32_t frame, int i, int j) const { return plane_bit(bits + (size_t)frame * H * WW, WW, i, j); }
    __device__ bool left(uint32_t frame, uint8_t l, int i, int j) const { return at(frame, i, j - 1) == l; }
    __device__ bool up(uint32_t frame, uint8_t l, int i, int j) const { return at(frame, i - 1, j) == l; }
};

// parent[g] = raster index of the smallest pixel of g's component INSIDE its tile
template <class Src>
__global__ __launch_bounds__(MK_THREADS) void k_label_tiles(Src src, uint32_t *__restrict__ parent)
{
    __shared__ typename Src::Tile tile;
    __shared__ uint32_t par[LB_PX];
    const int t = (int)threadIdx.x, j0 = (int)blockIdx.x * LB_TW, i0 = (int)blockIdx.y * LB_TH;
    src.stage(tile, blockIdx.z, i0, j0);
    for (int q = t; q < LB_PX; q += (int)MK_THREADS) par[q] = (uint32_t)q;
    __syncthreads();
    for (int q = t; q < LB_PX; q += (int)MK_THREADS) {
        const int r = q / LB_TW, c = q - r * LB_TW;
        if (!Src::same(tile, q, q)) continue;
        if (c > 0 && Src::same(tile, q, q - 1)) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, (uint32_t)q, (uint32_t)(q - 1));
        if (r > 0) {
            if constexpr (Src::CONN == 8)
                if (c > 0 && Src::same(tile, q, q - LB_TW - 1)) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, (uint32_t)q, (uint32_t)(q - LB_TW - 1));
            if (Src::same(tile, q, q - LB_TW)) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, (uint32_t)q, (uint32_t)(q - LB_TW));
            if constexpr (Src::CONN == 8)
                if (c + 1 < LB_TW && Src::same(tile, q, q - LB_TW + 1)) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, (uint32_t)q, (uint32_t)(q - LB_TW + 1));
        }
    }
    __syncthreads();
    uint32_t *out = parent + (size_t)blockIdx.z * src.W * src.H;
    for (int q = t; q < LB_PX; q += (int)MK_THREADS) {
        const int r = q / LB_TW, c = q - r * LB_TW;
        if (!Src::same(tile, q, q)) continue;               // a labelled pixel lies inside the image
        const uint32_t root = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, (uint32_t)q);
        const int rr = (int)root / LB_TW, rc = (int)root - rr * LB_TW;
        out[(size_t)(i0 + r) * src.W + j0 + c] = (uint32_t)(i0 + rr) * (uint32_t)src.W + (uint32_t)(j0 + rc);
    }
}

// pixels on a tile border meet their W / NW / N / NE neighbours of equal label in the neighbouring tiles (CONN 4: W and N alone)
template <class Src>
__global__ __launch_bounds__(MK_THREADS) void k_label_seams(Src src, uint32_t *__restrict__ parent)
{
    const int W = src.W, H = src.H;
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x, f = blockIdx.y;
    if (g >= (uint32_t)W * (uint32_t)H) return;
    const int i = (int)(g / (uint32_t)W), j = (int)(g - (uint32_t)i * (uint32_t)W);
    const bool top = (i % LB_TH) == 0, left = (j % LB_TW) == 0, right = (j % LB_TW) == LB_TW - 1;
    if (!(top || left || right)) return;
    uint32_t *par = parent + (size_t)f * W * H;
    const uint8_t l = src.at(f, i, j);
    if (!l) return;
    if (left && j > 0 && src.left(f, l, i, j)) uf_unite<__HIP_MEMORY_SCOPE_AGENT>(par, g, g - 1);
    if (i > 0) {
        if constexpr (Src::CONN == 8)
            if ((top || left) && j > 0 && src.at(f, i - 1, j - 1) == l) uf_unite<__HIP_MEMORY_SCOPE_AGENT>(par, g, g - (uint32_t)W - 1);
        if (top && src.up(f, l, i, j)) uf_unite<__HIP_MEMORY_SCOPE_AGENT>(par, g, g - (uint32_t)W);
        if constexpr (Src::CONN == 8)
            if ((top || right) && j + 1 < W && src.at(f, i - 1, j + 1) == l) uf_unite<__HIP_MEMORY_SCOPE_AGENT>(par, g, g - (uint32_t)W + 1);
    }
}

// parent[g] = root; what a root owns (own_words 32-bit words per pixel of `owned`: its statistics, its counter) starts at zero.
// Writes race only with reads that accept any ancestor.
template <class Src>
__global__ __launch_bounds__(MK_THREADS) void k_label_flatten(Src src, uint32_t *__restrict__ parent, uint32_t *__restrict__ owned, uint32_t own_words)
{
    const int W = src.W, H = src.H;
    const uint32_t g = blockIdx.x * MK_THREADS + threadIdx.x;
    if (g >= (uint32_t)W * (uint32_t)H) return;
    const int i = (int)(g / (uint32_t)W), j = (int)(g - (uint32_t)i * (uint32_t)W);
    if (!src.at(blockIdx.y, i, j)) return;
    const size_t base = (size_t)blockIdx.y * W * H;
    uint32_t *par = parent + base;
    const uint32_t root = uf_find<__HIP_MEMORY_SCOPE_AGENT>(par, g);
    if (root != g) {
        par[g] = root;
    } else {
        uint32_t *own = owned + (base + g) * own_words;
        for (uint32_t e = 0; e < own_words; ++e) own[e] = 0u;
    }
}

// tiles, then seams, for nf images on the context's stream: every labelled pixel's parent chain ends at its component's root
template <class Src>
void label_unite(d2r_ctx *ctx, const Src &src, uint32_t nf, uint32_t *parent)
{
    const uint32_t w = (uint32_t)src.W, h = (uint32_t)src.H;
    hipLaunchKernelGGL(k_label_tiles<Src>, dim3((w + LB_TW - 1) / LB_TW, (h + LB_TH - 1) / LB_TH, nf), dim3(MK_THREADS), 0, ctx->stream, src, parent);
    hipLaunchKernelGGL(k_label_seams<Src>, dim3((w * h + MK_THREADS - 1) / MK_THREADS, nf), dim3(MK_THREADS), 0, ctx->stream, src, parent);
}

// ... and the flatten: parent[g] = root, what the roots own zeroed (own_bytes per pixel, a multiple of 4)
template <class Src>
void label_components(d2r_ctx *ctx, const Src &src, uint32_t nf, uint32_t *parent, void *owned, uint32_t own_bytes)
{
    label_unite(ctx, src, nf, parent);
    hipLaunchKernelGGL(k_label_flatten<Src>, dim3(((uint32_t)src.W * (uint32_t)src.H + MK_THREADS - 1) / MK_THREADS, nf), dim3(MK_THREADS), 0,
                       ctx->stream, src, parent, (uint32_t *)owned, own_bytes / 4);
}

// f(root, members, leader) once per distinct root among the wave's active lanes, wave-uniform: the ballot of the lanes that hold
// that root, and whether this lane is their first, the one that sends the atomics
template <class F>
__device__ inline void wave_each_root(bool active, uint32_t root, F f)
{
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t r0 = __shfl(root, leader);
        const unsigned long long members = __ballot(active && root == r0);
        f(r0, members, lane == leader);
        todo &= ~members;
    }
}

}  // namespace
