// captions.hip — zero-shot object names from the package's own CLIP towers (captioner="clip"), gfx950 only.
//
// Stands where the reference's BLIP-2 captions and their merging by the language model stand (caption.py:132-160); nothing here
// restates reference code.  The thumbnails are the ones d2r_thumbs_fill left packed in thumb_out:
//   k_caption_preprocess   HF CLIPImageProcessor on thumbnails of ragged sizes in one launch: per record a descriptor (offset, size,
//                          table offsets, crop), Pillow's antialiased bicubic in 22-bit fixed point (horizontal, then vertical, the
//                          uint8 intermediate in LDS), only the columns and rows the centre crop reads, normalised, written as bf16
//                          patches in the tower's input layout (and as fp32 pixel_values / the cropped uint8 image for parity)
//   k_caption_score        one workgroup per object: cos[t][v] by 64 lane partials and the xor butterfly, the sum over the object's
//                          thumbnails in record order, then the k best classes by (score descending, index ascending)
// The tower in between is clip.hip's d2r_clip_forward.
#include "d2r_internal.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>

// implemented in clip.hip
int d2r_clip_forward(d2r_ctx *, const d2r_clip *, const uint16_t *patches_dev, uint32_t n, const float *text_dev, uint32_t C, float logit_scale,
                     float *logits_dev, float *embeds_dev, const ClipL0Reuse *reuse);
size_t d2r_clip_patch_bytes(const d2r_clip *, uint32_t n);
uint32_t d2r_clip_image_size(const d2r_clip *);
uint32_t d2r_clip_proj_dim(const d2r_clip *);

#define CAP_PRECISION_BITS 22
constexpr uint32_t CAP_THREADS = 256, CAP_WAVES = CAP_THREADS / 64;
constexpr size_t CAP_LDS_MAX = 150 * 1024;          // the band of k_caption_preprocess, as k_preprocess's
constexpr uint32_t CAP_NONE = 0xffffffffu;

// one thumbnail.  The tables hold the S entries the crop reads, not the whole resized side: entry x of bounds_h / kk_h is column
// left + x of the resized image, entry y of bounds_v / kk_v is row top + y.
struct CapDesc {
    unsigned long long off;     // first byte in the packed buffer
    int iw, ih;                 // columns, rows
    int bh, kh, bv, kv;         // offsets into the arena, in ints: bounds_h [S][2] (xmin, count), kk_h [S][ks_h], bounds_v [S][2], kk_v [S][ks_v]
    int ks_h, ks_v;
    int need_h, need_v;         // 0: that side is S already (copy)
    int left, top;              // the crop in the resized image
};

__device__ __forceinline__ uint32_t cap_clip8(int v)
{
    v >>= CAP_PRECISION_BITS;
    return (uint32_t)min(max(v, 0), 255);
}

// grid (bands of P output rows, thumbnails); block 256.  Dynamic LDS: 3 planes of [S][ld] bytes, column-major as in k_preprocess;
// ld is the largest vertical support of a band over the whole batch.
__global__ __launch_bounds__(CAP_THREADS) void k_caption_preprocess(const uint8_t *__restrict__ packed, const CapDesc *__restrict__ descs,
                                                                    const int *__restrict__ arena, uint32_t S, uint32_t P, uint32_t ld,
                                                                    uint16_t *__restrict__ patches, uint32_t Kp_pad,
                                                                    float *__restrict__ pixel_values, uint8_t *__restrict__ crops)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t tmp[];
    const uint32_t img = blockIdx.y;
    const CapDesc d = descs[img];
    const uint32_t row0 = blockIdx.x * P, nrows = min(P, S - row0);
    const int *bnd_h = arena + d.bh, *kk_h = arena + d.kh, *bnd_v = arena + d.bv, *kk_v = arena + d.kv;
    const uint8_t *src = packed + d.off;
    int y_first, y_last;                                     // source rows this band reads: [y_first, y_last)
    if (d.need_v) {
        y_first = bnd_v[2 * row0];
        const uint32_t last = row0 + nrows - 1;
        y_last = bnd_v[2 * last] + bnd_v[2 * last + 1];
    } else {
        y_first = d.top + (int)row0;
        y_last = y_first + (int)nrows;
    }
    const uint32_t trows = (uint32_t)(y_last - y_first);     // <= ld by the host's choice of ld
    const uint32_t plane = S * ld;
    // pass 1: horizontal filter (or copy) of the crop's columns into LDS
    for (uint32_t i = threadIdx.x; i < trows * S; i += blockDim.x) {
        const uint32_t ty = i / S, tx = i - ty * S;
        const size_t rowb = (size_t)(y_first + (int)ty) * d.iw;
        uint32_t o0, o1, o2;
        if (d.need_h) {
            const int xmin = bnd_h[2 * tx], cnt = bnd_h[2 * tx + 1];
            const int *k = kk_h + (size_t)tx * d.ks_h;
            int s0 = 1 << (CAP_PRECISION_BITS - 1), s1 = s0, s2 = s0;
            for (int x = 0; x < cnt; x++) {
                const uint8_t *p = src + (rowb + xmin + x) * 3;
                const int kv = k[x];
                uint32_t px;                     // one unaligned 4-byte load per pixel as in k_preprocess: the 4th byte is unused, and behind
                __builtin_memcpy(&px, p, 4);     //  the buffer's last thumbnail lies d2r_reserve's slack (64 bytes at least)
                s0 += (int)(px & 0xffu) * kv;
                s1 += (int)((px >> 8) & 0xffu) * kv;
                s2 += (int)((px >> 16) & 0xffu) * kv;
            }
            o0 = cap_clip8(s0); o1 = cap_clip8(s1); o2 = cap_clip8(s2);
        } else {
            const uint8_t *p = src + (rowb + d.left + (int)tx) * 3;
            o0 = p[0]; o1 = p[1]; o2 = p[2];
        }
        uint8_t *q = tmp + tx * ld + ty;
        q[0] = (uint8_t)o0;
        q[plane] = (uint8_t)o1;
        q[2 * plane] = (uint8_t)o2;
    }
    __syncthreads();
    // pass 2: vertical filter, normalise, scatter patch-major
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
    const float stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    const uint32_t g = S / P;
    for (uint32_t i = threadIdx.x; i < nrows * S; i += blockDim.x) {
        const uint32_t ry = i / S, rx = i - ry * S, oy = row0 + ry;
        uint32_t q[3];
        const uint8_t *col = tmp + rx * ld;
        if (d.need_v) {
            const int ymin = bnd_v[2 * oy] - y_first, cnt = bnd_v[2 * oy + 1];
            const int *k = kk_v + (size_t)oy * d.ks_v;
            int s0 = 1 << (CAP_PRECISION_BITS - 1), s1 = s0, s2 = s0;
            for (int y = 0; y < cnt; y++) {
                const uint8_t *p = col + ymin + y;
                const int kv = k[y];
                s0 += p[0] * kv;
                s1 += p[plane] * kv;
                s2 += p[2 * plane] * kv;
            }
            q[0] = cap_clip8(s0); q[1] = cap_clip8(s1); q[2] = cap_clip8(s2);
        } else {
            q[0] = col[ry]; q[1] = col[plane + ry]; q[2] = col[2 * plane + ry];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float f = (float)((double)q[c] * (1.0 / 255.0));
            const float v = (f - mean[c]) / stdv[c];
            if (pixel_values) pixel_values[(((size_t)img * 3 + c) * S + oy) * S + rx] = v;
            if (crops) crops[(((size_t)img * S + oy) * S + rx) * 3 + c] = (uint8_t)q[c];
            const uint32_t pr = oy / P, pc = rx / P, iy = oy % P, ix = rx % P;
            const size_t rowi = (size_t)img * g * g + pr * g + pc;
            union { __bf16 b; uint16_t u; } cv;
            cv.b = (__bf16)v;
            patches[rowi * Kp_pad + (c * P + iy) * P + ix] = cv.u;
        }
    }
}

// (score, index) order of the answer: score descending, ties to the lower index; CAP_NONE = nothing yet
__device__ __forceinline__ bool cap_better(float s, uint32_t i, float bs, uint32_t bi)
{
    return i != CAP_NONE && (bi == CAP_NONE || s > bs || (s == bs && i < bi));
}

// grid (objects); block 256 = 4 waves.  Wave w takes the classes v = w, w + 4, ...: lane l holds c[v][l], c[v][l + 64], ... in registers,
// and for every thumbnail t of the object in record order adds img[t][k] c[v][k] over k = l, l + 64, ... ascending (a multiply, then an
// add: the unit is compiled with -ffp-contract=off, and the intrinsics say it again), joins the 64 partials by the xor butterfly 32 ..
// 1 and adds the cosine to the object's score.  The scores of all V classes meet in LDS; k rounds then each pick the best class behind
// the previous round's in the answer's order.  Dynamic LDS: V floats.
__global__ __launch_bounds__(CAP_THREADS) void k_caption_score(const float *__restrict__ emb, const uint32_t *__restrict__ obj_start,
                                                               const float *__restrict__ cls, uint32_t V, uint32_t D, uint32_t k,
                                                               uint32_t *__restrict__ idx_out, float *__restrict__ score_out)
{
    extern __shared__ __attribute__((aligned(16))) float s_score[];
    __shared__ float w_s[CAP_WAVES], prev_s;
    __shared__ uint32_t w_i[CAP_WAVES], prev_i;
    const uint32_t o = blockIdx.x, t0 = obj_start[o], t1 = obj_start[o + 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nj = D / 64;
    for (uint32_t v = wave; v < V; v += CAP_WAVES) {
        float c[16];
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) c[j] = j < nj ? cls[(size_t)v * D + lane + 64 * j] : 0.f;
        float s = 0.f;
        for (uint32_t t = t0; t < t1; t++) {
            const float *e = emb + (size_t)t * D + lane;
            float p = 0.f;
#pragma unroll
            for (uint32_t j = 0; j < 16; j++)
                if (j < nj) p = __fadd_rn(p, __fmul_rn(e[64 * j], c[j]));
#pragma unroll
            for (int x = 32; x > 0; x >>= 1) p = __fadd_rn(p, __shfl_xor(p, x));
            s = __fadd_rn(s, p);
        }
        if (lane == 0) s_score[v] = s == s ? s : -INFINITY;      // a score that is no number ranks as minus infinity (section 2m)
    }
    __syncthreads();
    for (uint32_t r = 0; r < k; r++) {
        const float ps = r ? prev_s : 0.f;
        const uint32_t pi = r ? prev_i : 0u;
        float bs = 0.f;
        uint32_t bi = CAP_NONE;
        for (uint32_t v = threadIdx.x; v < V; v += CAP_THREADS) {
            const float sc = s_score[v];
            const bool behind = r == 0 || sc < ps || (sc == ps && v > pi);
            if (behind && cap_better(sc, v, bs, bi)) { bs = sc; bi = v; }
        }
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) {
            const float os = __shfl_xor(bs, x);
            const uint32_t oi = __shfl_xor(bi, x);
            if (cap_better(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        if (lane == 0) { w_s[wave] = bs; w_i[wave] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (uint32_t w = 1; w < CAP_WAVES; w++)
                if (cap_better(w_s[w], w_i[w], bs, bi)) { bs = w_s[w]; bi = w_i[w]; }
            idx_out[(size_t)o * k + r] = bi;
            score_out[(size_t)o * k + r] = bs;
            prev_s = bs;
            prev_i = bi;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ host

namespace {

// the geometry and tables of one distinct (rows, cols), from the context's cache: HF get_resize_output_image_size(shortest_edge = S,
// default_to_square = False), and Pillow's coefficients (d2r_clip_resample_coeffs) for the S positions of the crop on every side that
// is resized
const D2rCaptionTables &caption_size_tables(d2r_ctx *ctx, uint32_t rows, uint32_t cols, uint32_t S, uint32_t P)
{
    const std::array<uint32_t, 4> key = {rows, cols, S, P};
    auto it = ctx->cap_sizes.find(key);
    if (it != ctx->cap_sizes.end()) return it->second;
    if (ctx->cap_sizes.size() >= 4096) ctx->cap_sizes.clear();       // a bound on the host memory, far above a scan's distinct sizes
    D2rCaptionTables z;
    const int iw = (int)cols, ih = (int)rows;
    const int short_e = std::min(iw, ih), long_e = std::max(iw, ih);
    const int new_long = (int)((double)S * long_e / short_e);
    const int rw = iw <= ih ? (int)S : new_long, rh = iw <= ih ? new_long : (int)S;
    z.need_h = rw != iw;
    z.need_v = rh != ih;
    z.left = (rw - (int)S) / 2;
    z.top = (rh - (int)S) / 2;
    if (z.need_h) z.ks_h = d2r_clip_resample_coeffs(iw, rw, z.left, (int)S, z.bh, z.kh);
    if (z.need_v) z.ks_v = d2r_clip_resample_coeffs(ih, rh, z.top, (int)S, z.bv, z.kv);
    z.band_rows = (int)P;
    if (z.need_v) {
        z.band_rows = 0;
        for (uint32_t r0 = 0; r0 < S; r0 += P) {
            const uint32_t last = std::min(r0 + P, S) - 1;
            z.band_rows = std::max(z.band_rows, z.bv[2 * last] + z.bv[2 * last + 1] - z.bv[2 * r0]);
        }
    }
    return ctx->cap_sizes.emplace(key, std::move(z)).first->second;
}

// what d2r_caption_vote and d2r_caption_names refuse about the classes, and the key the upload is cached by
int caption_check_classes(d2r_ctx *ctx, const float *class_embeds, uint32_t V, uint32_t D, uint32_t k, uint64_t *hash)
{
    if (V == 0) return d2r_fail(ctx, D2R_ERR_INVALID, "captions: V = 0: there must be a class to name an object by");
    if (V > D2R_CAPTION_MAX_V) return d2r_fail(ctx, D2R_ERR_INVALID, "captions: V is above D2R_CAPTION_MAX_V");
    if (D == 0 || D % 64 != 0 || D > D2R_CAPTION_MAX_D) return d2r_fail(ctx, D2R_ERR_INVALID, "captions: D must be a multiple of 64, at most D2R_CAPTION_MAX_D");
    if (k < 1 || k > std::min<uint32_t>(D2R_CAPTION_MAX_K, V)) return d2r_fail(ctx, D2R_ERR_INVALID, "captions: k must be 1 .. min(D2R_CAPTION_MAX_K, V)");
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < (size_t)V * D; ++i) {
        if (!std::isfinite(class_embeds[i])) return d2r_fail(ctx, D2R_ERR_INVALID, "captions: a class embedding is not finite");
        uint32_t bits;
        memcpy(&bits, &class_embeds[i], 4);
        h = (h ^ bits) * 1099511628211ull;
    }
    *hash = h;
    return D2R_OK;
}

int caption_upload_classes(d2r_ctx *ctx, const float *class_embeds, uint32_t V, uint32_t D, uint64_t hash)
{
    if (ctx->cap_cls_valid && ctx->cap_cls_key[0] == V && ctx->cap_cls_key[1] == D && ctx->cap_cls_key[2] == hash) return D2R_OK;
    ctx->cap_cls_valid = false;
    int rc;
    D2rStageTimer &ev = ctx->cap_ev[3];
    if ((rc = d2r_reserve(ctx, ctx->cap_cls, (size_t)V * D * 4)) || (rc = ev.mark(ctx, 0))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(ctx->cap_cls.p, class_embeds, (size_t)V * D * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = ev.mark(ctx, 1))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));         // the caller's array has been read; the key is only set on success
    ev.done();
    double ms[1];
    if ((rc = ev.read(ctx, ms, 1, ""))) return rc;
    ctx->cap_ms[0] += ms[0];                                 // counted as upload of the call that brought new classes
    ctx->cap_cls_key[0] = V;
    ctx->cap_cls_key[1] = D;
    ctx->cap_cls_key[2] = hash;
    ctx->cap_cls_valid = true;
    return D2R_OK;
}

int caption_check_source(d2r_ctx *ctx)
{
    if (!ctx->cap_src.filled)
        return d2r_fail(ctx, D2R_ERR_INVALID, "captions: no thumbnails on this context: d2r_thumbs_plan and d2r_thumbs_fill come first");
    return D2R_OK;
}

void caption_timing_reset(d2r_ctx *ctx)
{
    for (double &m : ctx->cap_ms) m = 0.0;
}

// preprocess + tower over the context's thumbnails, a pass of the tower at a time; the embeddings [T][D] stay in cap_emb.  crops_dev /
// pv_dev (optional) receive a pass's parity outputs, which `download(c0, nc)` then copies out.  The stream is idle on return.
int caption_embed_device(d2r_ctx *ctx, const d2r_clip *clip, uint8_t *crops_dev, float *pv_dev,
                         const std::function<int(uint32_t c0, uint32_t nc)> &download)
{
    const D2rCaptionSrc &src = ctx->cap_src;
    const uint32_t T = (uint32_t)(src.recs.size() / 5), S = d2r_clip_image_size(clip), P = d2r_clip_patch_size(clip), D = d2r_clip_proj_dim(clip);
    if (T == 0) return D2R_OK;
    if (S % P != 0) return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "captions: the image size is not a whole number of patches");
    std::vector<int> arena;
    std::vector<CapDesc> descs(T);
    std::map<std::pair<uint32_t, uint32_t>, CapDesc> sizes;      // this batch's distinct sizes, their tables appended to the arena once
    int ld = 0;
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t *r = &src.recs[(size_t)t * 5];
        if ((uint64_t)S * std::max(r[1], r[2]) / std::min(r[1], r[2]) > (1u << 20))
            return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "captions: a thumbnail is too elongated: its resized long side would pass 2^20 pixels");
        auto it = sizes.find({r[1], r[2]});
        if (it == sizes.end()) {
            const D2rCaptionTables &z = caption_size_tables(ctx, r[1], r[2], S, P);
            CapDesc d{};
            d.iw = (int)r[2];
            d.ih = (int)r[1];
            d.ks_h = z.ks_h; d.ks_v = z.ks_v; d.need_h = z.need_h; d.need_v = z.need_v; d.left = z.left; d.top = z.top;
            auto put = [&arena](const std::vector<int> &v) {
                const int at = (int)arena.size();
                arena.insert(arena.end(), v.begin(), v.end());
                return at;
            };
            d.bh = put(z.bh); d.kh = put(z.kh); d.bv = put(z.bv); d.kv = put(z.kv);
            it = sizes.emplace(std::make_pair(r[1], r[2]), d).first;
        }
        descs[t] = it->second;
        descs[t].off = (unsigned long long)r[3] | (unsigned long long)r[4] << 32;
        ld = std::max(ld, caption_size_tables(ctx, r[1], r[2], S, P).band_rows);
    }
    if (arena.empty()) arena.push_back(0);                   // a batch of S x S thumbnails has no table
    const size_t lds = (size_t)ld * S * 3;
    if (lds > CAP_LDS_MAX) return d2r_fail(ctx, D2R_ERR_UNSUPPORTED, "captions: a thumbnail's preprocess band does not fit in LDS");
    const uint32_t per = d2r_pass_size(ctx, clip, 0), cap = std::min(per, T);
    D2rStage tab(ctx, ctx->cap_tab);
    const size_t o_desc = tab.add(descs.size() * sizeof(CapDesc)), o_arena = tab.add(arena.size() * sizeof(int));
    int rc;
    if ((rc = tab.reserve()) || (rc = d2r_reserve(ctx, ctx->cap_emb, (size_t)T * D * 4)) ||
        (rc = d2r_reserve(ctx, ctx->clipws[6], d2r_clip_patch_bytes(clip, cap))) || (rc = d2r_reserve(ctx, ctx->text, (size_t)D * 4)))
        return rc;
    D2rDrain drain{ctx->stream};                             // descs and arena are read by the queued copies
    static PerDeviceOnce attr;
    attr.run(ctx->device, [] {
        (void)hipFuncSetAttribute((const void *)k_caption_preprocess, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CAP_LDS_MAX);
    });
    D2rStageTimer &ev = ctx->cap_ev[0], &ev_dl = ctx->cap_ev[2];
    for (uint32_t c0 = 0; c0 < T; c0 += per) {
        const uint32_t nc = std::min(per, T - c0);
        if ((rc = ev.mark(ctx, 0))) return rc;
        if (c0 == 0 && ((rc = tab.upload(o_desc, descs.data(), descs.size() * sizeof(CapDesc))) ||
                        (rc = tab.upload(o_arena, arena.data(), arena.size() * sizeof(int)))))
            return rc;
        if ((rc = ev.mark(ctx, 1))) return rc;
        hipLaunchKernelGGL(k_caption_preprocess, dim3(S / P, nc), dim3(CAP_THREADS), lds, ctx->stream, (const uint8_t *)ctx->thumb_out.p,
                           tab.at<const CapDesc>(o_desc) + c0, tab.at<const int>(o_arena), S, P, (uint32_t)ld, (uint16_t *)ctx->clipws[6].p,
                           d2r_clip_patch_stride(clip), pv_dev, crops_dev);
        D2R_HIP(ctx, hipGetLastError());
        if ((rc = ev.mark(ctx, 2))) return rc;
        if ((rc = d2r_clip_forward(ctx, clip, (const uint16_t *)ctx->clipws[6].p, nc, (const float *)ctx->text.p, 0, 1.0f, nullptr,
                                   (float *)ctx->cap_emb.p + (size_t)c0 * D, nullptr)))
            return rc;
        if ((rc = ev.mark(ctx, 3)) || (rc = ev_dl.mark(ctx, 0))) return rc;
        if (download && (rc = download(c0, nc))) return rc;
        if ((rc = ev_dl.mark(ctx, 1))) return rc;
        D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ev.done();
        ev_dl.done();
        double ms[3], dl[1];
        if ((rc = ev.read(ctx, ms, 3, "")) || (rc = ev_dl.read(ctx, dl, 1, ""))) return rc;
        ctx->cap_ms[0] += ms[0];
        ctx->cap_ms[1] += ms[1];
        ctx->cap_ms[2] += ms[2];
        ctx->cap_ms[4] += dl[0];
    }
    return D2R_OK;
}

// the scoring launch on device arrays; idx / scores [n_objs][k] to the host.  Synchronises.
int caption_score_device(d2r_ctx *ctx, const float *emb_dev, const std::vector<uint32_t> &obj_start, uint32_t V, uint32_t D, uint32_t k,
                         const float *embeds_host, uint32_t T, uint32_t *idx_out, float *score_out)
{
    const uint32_t n_objs = (uint32_t)obj_start.size() - 1;
    D2rStage ws(ctx, ctx->cap_ws);
    const size_t o_start = ws.add(obj_start.size() * 4), o_emb = ws.add(embeds_host ? (size_t)T * D * 4 : 0), o_idx = ws.add((size_t)n_objs * k * 4),
                 o_sc = ws.add((size_t)n_objs * k * 4);
    int rc;
    if ((rc = ws.reserve())) return rc;
    D2rDrain drain{ctx->stream};
    D2rStageTimer &ev = ctx->cap_ev[1];
    if ((rc = ev.mark(ctx, 0)) || (rc = ws.upload(o_start, obj_start.data(), obj_start.size() * 4))) return rc;
    if (embeds_host && T && (rc = ws.upload(o_emb, embeds_host, (size_t)T * D * 4))) return rc;
    if ((rc = ev.mark(ctx, 1))) return rc;
    hipLaunchKernelGGL(k_caption_score, dim3(n_objs), dim3(CAP_THREADS), (size_t)V * 4, ctx->stream, embeds_host ? ws.at<const float>(o_emb) : emb_dev,
                       ws.at<const uint32_t>(o_start), (const float *)ctx->cap_cls.p, V, D, k, ws.at<uint32_t>(o_idx), ws.at<float>(o_sc));
    D2R_HIP(ctx, hipGetLastError());
    if ((rc = ev.mark(ctx, 2))) return rc;
    // into the library's own arrays first: the caller's outputs are written only once the device work has succeeded
    std::vector<uint32_t> idx((size_t)n_objs * k);
    std::vector<float> sc((size_t)n_objs * k);
    D2R_HIP(ctx, hipMemcpyAsync(idx.data(), ws.at<uint32_t>(o_idx), idx.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    D2R_HIP(ctx, hipMemcpyAsync(sc.data(), ws.at<float>(o_sc), sc.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ev.mark(ctx, 3))) return rc;
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ev.done();
    double ms[3];
    if ((rc = ev.read(ctx, ms, 3, ""))) return rc;
    ctx->cap_ms[0] += ms[0];
    ctx->cap_ms[3] += ms[1];
    ctx->cap_ms[4] += ms[2];
    memcpy(idx_out, idx.data(), idx.size() * 4);
    memcpy(score_out, sc.data(), sc.size() * 4);
    return D2R_OK;
}

}  // namespace

extern "C" {

int d2r_caption_load_packed(d2r_ctx *ctx, const uint8_t *packed_u8, uint64_t total_bytes, const uint32_t *recs, uint32_t n_recs, uint32_t n_objs)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (!packed_u8 || !recs) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (n_recs == 0 || n_objs == 0) return d2r_fail(ctx, D2R_ERR_INVALID, "captions: d2r_caption_load_packed needs a record and an object");
    uint32_t prev = 0;
    for (uint32_t t = 0; t < n_recs; ++t) {
        const uint32_t *r = &recs[(size_t)t * 5];
        const uint64_t off = (uint64_t)r[3] | (uint64_t)r[4] << 32;
        if (r[0] >= n_objs || r[0] < prev) return d2r_fail(ctx, D2R_ERR_INVALID, "captions: the records' objects must be below n_objs and must not decrease");
        if (r[1] == 0 || r[2] == 0 || r[1] > 16384 || r[2] > 16384) return d2r_fail(ctx, D2R_ERR_INVALID, "captions: a record's rows and cols must be 1 .. 16384");
        if (off % 4 != 0 || off > total_bytes || (uint64_t)r[1] * r[2] * 3 > total_bytes - off)
            return d2r_fail(ctx, D2R_ERR_INVALID, "captions: a record's offset must be a multiple of 4 and its image must lie inside the packed buffer");
        prev = r[0];
    }
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    ctx->cap_src.filled = false;
    int rc;
    if ((rc = d2r_reserve(ctx, ctx->thumb_out, (size_t)total_bytes))) return rc;
    D2R_HIP(ctx, hipMemcpyAsync(ctx->thumb_out.p, packed_u8, (size_t)total_bytes, hipMemcpyHostToDevice, ctx->stream));
    D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->cap_src.recs.assign(recs, recs + (size_t)n_recs * 5);
    ctx->cap_src.n_objs = n_objs;
    ctx->cap_src.total = total_bytes;
    ctx->cap_src.filled = true;
    return D2R_OK;
}

int d2r_caption_embed(d2r_ctx *ctx, const d2r_clip *clip, float *embeds_out, uint8_t *crops_u8_out, float *pixel_values_out)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (!clip || !embeds_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    int rc;
    if ((rc = caption_check_source(ctx))) return rc;
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t T = (uint32_t)(ctx->cap_src.recs.size() / 5), S = d2r_clip_image_size(clip), D = d2r_clip_proj_dim(clip);
    const uint32_t cap = std::min(d2r_pass_size(ctx, clip, 0), T);
    const size_t crop_b = (size_t)S * S * 3, pv_b = crop_b * 4;
    D2rStage ws(ctx, ctx->cap_ws);
    const size_t o_crop = ws.add(crops_u8_out ? cap * crop_b : 0), o_pv = ws.add(pixel_values_out ? cap * pv_b : 0);
    if ((rc = ws.reserve())) return rc;
    caption_timing_reset(ctx);
    auto download = [&](uint32_t c0, uint32_t nc) {
        D2R_HIP(ctx, hipMemcpyAsync(embeds_out + (size_t)c0 * D, (const float *)ctx->cap_emb.p + (size_t)c0 * D, (size_t)nc * D * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (crops_u8_out) D2R_HIP(ctx, hipMemcpyAsync(crops_u8_out + c0 * crop_b, ws.at<uint8_t>(o_crop), nc * crop_b, hipMemcpyDeviceToHost, ctx->stream));
        if (pixel_values_out)
            D2R_HIP(ctx, hipMemcpyAsync((char *)pixel_values_out + c0 * pv_b, ws.at<char>(o_pv), nc * pv_b, hipMemcpyDeviceToHost, ctx->stream));
        return (int)D2R_OK;
    };
    if ((rc = caption_embed_device(ctx, clip, crops_u8_out ? ws.at<uint8_t>(o_crop) : nullptr, pixel_values_out ? ws.at<float>(o_pv) : nullptr, download)))
        return rc;
    ctx->cap_timed = true;
    return D2R_OK;
}

int d2r_caption_vote(d2r_ctx *ctx, const float *embeds, const uint32_t *obj_of, uint32_t T, const float *class_embeds, uint32_t V, uint32_t D,
                     uint32_t n_objs, uint32_t k, uint32_t *idx_out, float *score_out)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if ((T && (!embeds || !obj_of)) || !class_embeds || !idx_out || !score_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (n_objs == 0 || n_objs > 255) return d2r_fail(ctx, D2R_ERR_INVALID, "captions: n_objs must be 1 .. 255");
    int rc;
    uint64_t hash;
    if ((rc = caption_check_classes(ctx, class_embeds, V, D, k, &hash))) return rc;
    std::vector<uint32_t> start(n_objs + 1, 0u);
    for (uint32_t t = 0; t < T; ++t) {
        if (obj_of[t] >= n_objs || (t && obj_of[t] < obj_of[t - 1]))
            return d2r_fail(ctx, D2R_ERR_INVALID, "captions: obj_of must be below n_objs and non-decreasing (thumbnails in record order)");
        ++start[obj_of[t] + 1];
    }
    for (uint32_t o = 0; o < n_objs; ++o) start[o + 1] += start[o];
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    caption_timing_reset(ctx);
    if ((rc = caption_upload_classes(ctx, class_embeds, V, D, hash)) ||
        (rc = caption_score_device(ctx, nullptr, start, V, D, k, embeds, T, idx_out, score_out)))
        return rc;
    ctx->cap_timed = true;
    return D2R_OK;
}

int d2r_caption_names(d2r_ctx *ctx, const d2r_clip *clip, const float *class_embeds, uint32_t V, uint32_t D, uint32_t n_objs, uint32_t k,
                      uint32_t *idx_out, float *score_out)
{
    if (!ctx) return d2r_fail(ctx, D2R_ERR_INVALID, "null context");
    if (!clip || !class_embeds || !idx_out || !score_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    int rc;
    if ((rc = caption_check_source(ctx))) return rc;
    if (d2r_clip_proj_dim(clip) != D)
        return d2r_fail(ctx, D2R_ERR_INVALID, "captions: the class embeddings' D (" + std::to_string(D) + ") is not the clip's proj_dim (" +
                                                  std::to_string(d2r_clip_proj_dim(clip)) + ")");
    uint64_t hash;
    if ((rc = caption_check_classes(ctx, class_embeds, V, D, k, &hash))) return rc;
    const D2rCaptionSrc &src = ctx->cap_src;
    if (src.n_objs == 0 || src.n_objs > 255) return d2r_fail(ctx, D2R_ERR_INVALID, "captions: the plan holds no object");
    if (n_objs != src.n_objs)
        return d2r_fail(ctx, D2R_ERR_INVALID, "captions: n_objs is " + std::to_string(n_objs) + " but the context's thumbnails are of " +
                                                  std::to_string(src.n_objs) + " objects: idx_out and score_out would not fit");
    const uint32_t T = (uint32_t)(src.recs.size() / 5);
    std::vector<uint32_t> start(src.n_objs + 1, 0u);
    for (uint32_t t = 0; t < T; ++t) ++start[src.recs[(size_t)t * 5] + 1];
    for (uint32_t o = 0; o < src.n_objs; ++o) start[o + 1] += start[o];
    D2R_HIP(ctx, hipSetDevice(ctx->device));
    caption_timing_reset(ctx);
    if ((rc = caption_upload_classes(ctx, class_embeds, V, D, hash)) || (rc = caption_embed_device(ctx, clip, nullptr, nullptr, nullptr)) ||
        (rc = d2r_reserve(ctx, ctx->cap_emb, (size_t)std::max<uint32_t>(T, 1) * D * 4)) ||
        (rc = caption_score_device(ctx, (const float *)ctx->cap_emb.p, start, V, D, k, nullptr, T, idx_out, score_out)))
        return rc;
    ctx->cap_timed = true;
    return D2R_OK;
}

int d2r_caption_get_timing(d2r_ctx *ctx, double *ms_out)
{
    if (!ctx || !ms_out) return d2r_fail(ctx, D2R_ERR_INVALID, "null argument");
    if (!ctx->cap_timed) return d2r_fail(ctx, D2R_ERR_INVALID, "captions timing: no caption call has run on this context");
    for (int i = 0; i < 5; ++i) ms_out[i] = ctx->cap_ms[i];
    return D2R_OK;
}

}  // extern "C"
