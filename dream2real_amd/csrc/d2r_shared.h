// What the geometry units (pcd.hip, tsdf.hip, sdfphys.hip, phys.hip, the ray sort of nerf.hip, d2r_nerf) share: an owner for
// device memory, the single-workgroup scan and reduction, the rigid inverse.  Nothing else belongs here.  Stands on its own and
// comes with d2r_internal.h, whose d2r_nerf owns its buffers through it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/d2r.h"

int d2r_fail(d2r_ctx *ctx, int code, const std::string &msg);      // api.hip

// ------------------------------------------------------------------------------------------------ a. owned device memory

// One hipMalloc, freed when the owner goes: a temporary of an entry point may be live across any early return, a handle that holds
// its buffers this way is destroyed by `delete`.  Not a workspace: what grows and is reused stays d2r_ctx::Buf / d2r_reserve.
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

// ------------------------------------------------------------------------------------------------ c. the rigid inverse

// rows 0..2 of inv(T) = [R^T | -R^T t] for a row-major rigid 4x4: fp64, the translation's three products summed left to right
// (DESIGN.md sections 2b, 2c, 2e).  Callers round, append the row 0 0 0 1 or test rigidity as they need.
inline void d2r_rigid_inverse(const float T[16], double out[12])
{
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out[i * 4 + j] = (double)T[j * 4 + i];
        out[i * 4 + 3] = -(((double)T[0 * 4 + i] * (double)T[3] + (double)T[1 * 4 + i] * (double)T[7]) + (double)T[2 * 4 + i] * (double)T[11]);
    }
}
