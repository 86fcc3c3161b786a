// What the geometry units (pcd.hip, pcdbuild.hip, meshvis.hip, masks.hip, tsdf.hip, sdfphys.hip, phys.hip, rectify.hip, the ray sort of
// nerf.hip, d2r_nerf) share.  On the device: the single-workgroup scan and reduction.  On the host: an owner for device memory, the
// fp64 4x4 toolkit, the layout of a staging buffer and its binder, the stage timer, the camera refusals of a batch of frames.  A piece
// moves here when a second unit needs it.  Stands on its own (tests/shared_host_main.cpp) and comes with d2r_internal.h.  A plain
// host compiler (tests/tsdfvis_host_main.cpp) gets the parts that need nothing from HIP: the 4x4 toolkit, the layout, the refusals.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/d2r.h"

// a growable device workspace of a context (d2r_ctx::Buf): grown by d2r_reserve, never shrunk, freed with the context
struct D2rBuf { void *p = nullptr; size_t cap = 0; };

int d2r_fail(d2r_ctx *ctx, int code, const std::string &msg);      // api.hip
int d2r_reserve(d2r_ctx *ctx, D2rBuf &b, size_t bytes);            // api.hip

#if defined(__HIPCC__)
hipStream_t d2r_stream(const d2r_ctx *ctx);                        // api.hip: ctx->stream, for the code here that sees d2r_ctx incomplete

#define D2R_HIP(ctx, expr)                                                              \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return d2r_fail(ctx, D2R_ERR_DEVICE,                                        \
                            std::string(#expr) + ": " + hipGetErrorString(e_));         \
    } while (0)

// ------------------------------------------------------------------------------------------------ a. owned device memory

// One hipMalloc, freed when the owner goes: a temporary of an entry point may be live across any early return, a handle that holds
// its buffers this way is destroyed by `delete`.  Not a workspace: what grows and is reused stays D2rBuf / d2r_reserve (section d).
template <class T>
class D2rDev {
public:
    D2rDev() = default;
    D2rDev(D2rDev &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    D2rDev &operator=(D2rDev &&o) noexcept
    {
        std::swap(p_, o.p_);
        return *this;
    }
    ~D2rDev()
    {
        if (p_) (void)hipFree(p_);
    }
    // `what` names the buffer's purpose in the message of a failure ("a TSDF volume")
    int alloc(d2r_ctx *ctx, size_t bytes, const char *what, bool zero = false)
    {
        if (p_) (void)hipFree(p_);
        if (hipMalloc((void **)&p_, std::max<size_t>(bytes, 16)) != hipSuccess) {
            p_ = nullptr;
            return d2r_fail(ctx, D2R_ERR_MEMORY, std::string("hipMalloc failed for ") + what + " (" + std::to_string(bytes >> 20) + " MiB)");
        }
        if (zero && hipMemset(p_, 0, std::max<size_t>(bytes, 16)) != hipSuccess)
            return d2r_fail(ctx, D2R_ERR_DEVICE, std::string("hipMemset failed for ") + what);
        return D2R_OK;
    }
    T *get() const { return p_; }

private:
    T *p_ = nullptr;
};

// Declared after an entry point's temporaries, so destroyed before them: whichever return is taken, the work queued on them
// has finished before they are freed.
struct D2rDrain {
    hipStream_t stream;
    ~D2rDrain() { (void)hipStreamSynchronize(stream); }
};

// ------------------------------------------------------------------------------------------------ b. one workgroup's scan and sum

// For workgroups of D2R_SCAN_THREADS threads, over uint32_t or uint2 (component-wise).  The scan is the plain one: a partial per
// thread in LDS, thread 0 runs over the 256 partials serially, two barriers.
constexpr uint32_t D2R_SCAN_THREADS = 256;

__device__ __forceinline__ uint32_t d2r_scan_add(uint32_t a, uint32_t b) { return a + b; }
__device__ __forceinline__ uint2 d2r_scan_add(uint2 a, uint2 b) { return make_uint2(a.x + b.x, a.y + b.y); }

// exclusive scan of one value per thread, starting at `seed` (thread 0's is the one used) -> the sum of the lower threads' values;
// *total (optional) receives seed + every value in thread 0 and is left alone in the others
template <class T>
__device__ __forceinline__ T d2r_block_scan(T mine, T seed, T *total = nullptr)
{
    __shared__ T part[D2R_SCAN_THREADS];
    part[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        T run = seed;
        for (uint32_t i = 0; i < D2R_SCAN_THREADS; i++) {
            const T v = part[i];
            part[i] = run;
            run = d2r_scan_add(run, v);
        }
        if (total) *total = run;
    }
    __syncthreads();
    return part[threadIdx.x];
}

// out[i] = in[0] + .. + in[i - 1] for a row of n entries in global memory; in == out scans in place.  Thread t owns entries
// t * per .. t * per + per - 1, per = ceil(n / 256).  -> the row's total in thread 0, zero in the others
template <class T>
__device__ __forceinline__ T d2r_block_scan_row(const T *in, T *out, uint32_t n)
{
    const uint32_t per = (n + D2R_SCAN_THREADS - 1) / D2R_SCAN_THREADS, lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
    T sum = T(), total = T();
    for (uint32_t i = lo; i < hi; i++) sum = d2r_scan_add(sum, in[i]);
    T run = d2r_block_scan(sum, T(), &total);
    for (uint32_t i = lo; i < hi; i++) {
        const T v = in[i];
        out[i] = run;
        run = d2r_scan_add(run, v);
    }
    return total;
}

// the sum of one value per thread (tree in LDS), in every thread
template <class T>
__device__ __forceinline__ T d2r_block_sum(T mine)
{
    __shared__ T part[D2R_SCAN_THREADS];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t s = D2R_SCAN_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] = d2r_scan_add(part[threadIdx.x], part[threadIdx.x + s]);
        __syncthreads();
    }
    return part[0];
}
#endif      // __HIPCC__

// ------------------------------------------------------------------------------------------------ c. the fp64 4x4 toolkit

// rows 0..2 of inv(T) = [R^T | -R^T t] for a row-major rigid 4x4: fp64, the translation's three products summed left to right
// (DESIGN.md sections 2b, 2c, 2e).  Callers round, append the row 0 0 0 1 or test rigidity as they need.
inline void d2r_rigid_inverse(const float T[16], double out[12])
{
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out[i * 4 + j] = (double)T[j * 4 + i];
        out[i * 4 + 3] = -(((double)T[0 * 4 + i] * (double)T[3] + (double)T[1 * 4 + i] * (double)T[7]) + (double)T[2 * 4 + i] * (double)T[11]);
    }
}

// ... as a 4x4 for d2r_mul4
inline void d2r_rigid_inverse4(const float T[16], double out[16])
{
    d2r_rigid_inverse(T, out);
    out[12] = out[13] = out[14] = 0.0;
    out[15] = 1.0;
}

// C = A B, fp64, each entry summed over l = 0, 1, 2, 3 in that order (DESIGN.md sections 2b, 2f)
inline void d2r_mul4(const double A[16], const double B[16], double C[16])
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            C[i * 4 + j] = ((A[i * 4 + 0] * B[0 * 4 + j] + A[i * 4 + 1] * B[1 * 4 + j]) + A[i * 4 + 2] * B[2 * 4 + j]) + A[i * 4 + 3] * B[3 * 4 + j];
}

// rows 0..3 of a row-major 4x4: finite, R^T R = I to 1e-5, last row 0 0 0 1 (the ray caster's and the camera tracker's refusal).
// Their rules invert poses by transposition, so a pose that is off orthogonal by e moves what a kernel reads by about e times the
// distance to that pose's origin; that is the caller's to bound (rotations built in fp32 are off by about 1e-7).
inline bool d2r_is_rigid(const float T[16])
{
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(T[i])) return false;
    double dev = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += (double)T[k * 4 + i] * (double)T[k * 4 + j];
            dev = std::max(dev, fabs(d - (i == j ? 1.0 : 0.0)));
        }
    return dev <= 1e-5 && T[12] == 0.f && T[13] == 0.f && T[14] == 0.f && T[15] == 1.f;
}

// float[16] -> double[16]; rows 0..2 rounded once into the float[12] a kernel-side matrix struct (PcdMat, MvMat) holds
inline void d2r_load16(const float p[16], double out[16]) { for (int i = 0; i < 16; ++i) out[i] = (double)p[i]; }
inline void d2r_round34(const double T[16], float out[12]) { for (int i = 0; i < 12; ++i) out[i] = (float)T[i]; }

// three bytes -> r | g << 8 | b << 16, the colour word of the point clouds and the mesh renderer
inline uint32_t d2r_pack_rgb(const uint8_t rgb[3]) { return (uint32_t)rgb[0] | (uint32_t)rgb[1] << 8 | (uint32_t)rgb[2] << 16; }

// ------------------------------------------------------------------------------------------------ d. an entry point's staging and timing

// Segments of one buffer, packed in call order, each starting at a multiple of 256 bytes.  Pure arithmetic.
struct D2rLayout {
    size_t end = 0;
    size_t add(size_t bytes)      // -> the new segment's offset; a segment of 0 bytes takes no room
    {
        const size_t at = (end + 255) & ~(size_t)255;
        end = at + bytes;
        return at;
    }
    size_t total() const { return end; }      // the end of the last segment: the bytes to reserve
};

#if defined(__HIPCC__)
// A layout bound to the workspace it describes: add() the segments, reserve(), then at<T>() and upload() by offset.
class D2rStage : public D2rLayout {
public:
    D2rStage(d2r_ctx *ctx, D2rBuf &buf) : ctx_(ctx), buf_(buf) {}
    int reserve() { return d2r_reserve(ctx_, buf_, total()); }
    template <class T>
    T *at(size_t off) const { return (T *)((char *)buf_.p + off); }
    // queues host -> device on the context's stream; `src` must stay alive until the stream has run it
    int upload(size_t off, const void *src, size_t bytes) const
    {
        D2R_HIP(ctx_, hipMemcpyAsync(at<char>(off), src, bytes, hipMemcpyHostToDevice, d2r_stream(ctx_)));
        return D2R_OK;
    }

private:
    d2r_ctx *ctx_;
    D2rBuf &buf_;
};

// Up to four events on the context's stream: begin, after upload, after kernels, after download.  An entry point marks them as
// it goes and calls done() once the whole call has succeeded; a call that fails midway leaves the flag as it found it.  The
// owner (a context, a handle) is destroyed with its device current, and the events with it.
class D2rStageTimer {
public:
    D2rStageTimer() = default;
    D2rStageTimer(const D2rStageTimer &) = delete;
    D2rStageTimer &operator=(const D2rStageTimer &) = delete;
    ~D2rStageTimer()
    {
        for (hipEvent_t e : ev_)
            if (e) (void)hipEventDestroy(e);
    }
    int mark(d2r_ctx *ctx, int k)
    {
        if (!ev_[k]) D2R_HIP(ctx, hipEventCreate(&ev_[k]));
        D2R_HIP(ctx, hipEventRecord(ev_[k], d2r_stream(ctx)));
        return D2R_OK;
    }
    void done() { timed_ = true; }
    // ms_out[k] = milliseconds from mark k to mark k + 1, k < n_stages; refuses with `untimed` while no call has been done()
    int read(d2r_ctx *ctx, double *ms_out, int n_stages, const char *untimed) const
    {
        if (!timed_) return d2r_fail(ctx, D2R_ERR_INVALID, untimed);
        for (int k = 0; k < n_stages; ++k) {
            float ms = 0.f;
            D2R_HIP(ctx, hipEventElapsedTime(&ms, ev_[k], ev_[k + 1]));
            ms_out[k] = ms;
        }
        return D2R_OK;
    }

private:
    hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
    bool timed_ = false;
};
#endif      // __HIPCC__

// ------------------------------------------------------------------------------------------------ e. a frame batch's camera

// Every unit that takes a camera refuses alike, `unit` in front of the message: 3x3 intrinsics, n row-major 4x4 poses, each float
// or double.  A unit that holds its pose to more (tsdf.hip, camtrack.hip) passes n = 0 and says so itself.
template <class I, class P>
int d2r_check_cam(d2r_ctx *ctx, const char *unit, const I *K, const P *poses, uint32_t n)
{
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(K[i])) return d2r_fail(ctx, D2R_ERR_INVALID, std::string(unit) + ": intrinsics must be finite");
    if (K[0] == 0.0 || K[4] == 0.0) return d2r_fail(ctx, D2R_ERR_INVALID, std::string(unit) + ": focal lengths must not be 0");
    for (size_t i = 0; i < (size_t)n * 16; ++i)
        if (!std::isfinite(poses[i])) return d2r_fail(ctx, D2R_ERR_INVALID, std::string(unit) + ": poses must be finite");
    return D2R_OK;
}
