// What the mask units (masks.hip, proposals.hip) share on the device: the workgroup size, the bit-packed k x k morphology on
// rows of 64-bit words and the lock-free union-find of the component labellers.  A piece moves here when
// the second unit needs it.  Comes after d2r_internal.h.
#pragma once
#include "d2r_internal.h"

namespace {

constexpr uint32_t MK_THREADS = 256;
constexpr int CL_TW = 4, CL_TR = 64, CL_ROWS = 128;      // k_morph: words x output rows of a tile, rows held (CL_TR + 63 <= CL_ROWS)
constexpr int LB_TW = 64, LB_TH = 16, LB_PX = LB_TW * LB_TH;   // k_label_tiles: tile of the per-tile labelling
constexpr uint32_t NO_KEY = 0xffffffffu;

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

}  // namespace
