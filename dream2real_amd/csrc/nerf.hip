// nerf.hip — hash-grid NeRF ray marcher for gfx950 (MI355X), hand-written HIP.
//
// Replaces, for a whole batch of cameras at once, what the reference obtains from
// pyngp.Testbed.render() in Shade and Depth mode (reference
// reconstruction/combined_rendering.py:105,113,127,130) and the per-pixel compositing that
// follows it (:133-155).  The algorithm is specified by oracle/d2r_oracle.c; this file is
// an independent MI355X-first implementation of that specification:
//
//   k_cameras_*   per-candidate virtual camera (convert_virtual_pose, :250-263, fp64) and
//                 nerf_matrix_to_ngp
//   k_raygen      one lane per pixel: ray, unit-cube + occupied-bbox slab tests, brick DDA
//                 to the first occupied lattice sample; survivors are appended to a ray
//                 queue with ONE atomic per wave (64-bit ballot + prefix popcount)
//   k_march       persistent waves: each lane owns a ray; lanes that finish are refilled
//                 from the queue by ballot/prefix compaction.  Per iteration the wave
//                 evaluates 64 samples: lane pairs (l, l^32) split the 16 hash-grid levels
//                 of two samples so that every lane directly produces MFMA B-operand
//                 fragments (no LDS staging, no transposes); both MLPs run as
//                 v_mfma_f32_32x32x16_bf16 with weights as A-operands read from LDS, and
//                 each layer's C layout is consumed as the next layer's B operand through
//                 a pre-permuted weight fragment order.  Colour and depth are composited
//                 in the same pass; finished rays write the final pixel (parity mode:
//                 fp32 RGBA + depth; composite mode: depth test against the background,
//                 un-premultiply, sRGB, uint8, alpha threshold).
#include <algorithm>
#include <cstring>

#include "d2r_internal.h"
#include <type_traits>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
union Frag {
    bf16x8 v;
    f16x8 h;
    uint4 u;
};

// Operand type of the MLPs' MFMAs, fp32 accumulation either way.  F16 = true (option "mlp_f16" 1, the default since round 6): fp16 — the
// reference's OPERAND type (tiny-cuda-nn's fully fused MLPs hold weights and activations in __half; it also ACCUMULATES in half, which
// nothing here does): the snapshot's fp16 weights enter the MFMA exactly, features and activations keep 11 significant bits,
// v_mfma_f32_32x32x16_f16 runs at the bf16 rate.  Range: activations must stay below 65504, as in the reference.  F16 = false: bf16
// operands (north_star: "a small fused MLP as MFMA bf16 tiles"), 8 significant bits.
template <bool F16>
__device__ __forceinline__ uint32_t pack2(float a, float b)
{
    if constexpr (F16) {
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        union { f16x2 v; uint32_t u; } r;
        r.v[0] = (_Float16)a;         // v_cvt_pk_f16_f32 (round to nearest even)
        r.v[1] = (_Float16)b;
        return r.u;
    } else {
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        union { bf16x2 v; uint32_t u; } r;
        r.v[0] = (__bf16)a;
        r.v[1] = (__bf16)b;
        return r.u;
    }
}

__device__ __forceinline__ float srgb_to_linear(float x)
{
    return x <= 0.04045f ? x / 12.92f : powf((x + 0.055f) / 1.055f, 2.4f);
}
__device__ __forceinline__ float linear_to_srgb(float x)
{
    return x > 0.0031308f ? 1.055f * powf(x, (float)(1.0 / 2.4)) - 0.055f : 12.92f * x;
}
__device__ __forceinline__ uint32_t quant_u8(float x)
{
    float c = fminf(fmaxf(x, 0.f), 1.f);
    return (uint32_t)(c * 255.0f + 0.5f);
}

// ------------------------------------------------------------------ cameras

__device__ inline void inv4(const double *m, double *inv)
{
    // adjugate / determinant, general 4x4
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    double id = 1.0 / det;
    for (int i = 0; i < 16; i++) inv[i] *= id;
}

__device__ inline void mul4(const double *a, const double *b, double *c)
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int k = 0; k < 4; k++) s += a[i * 4 + k] * b[k * 4 + j];
            c[i * 4 + j] = s;
        }
}

// instant-ngp nerf_matrix_to_ngp (oracle: d2r_oracle_nerf_matrix_to_ngp); m: 3x4 row-major
__device__ inline void nerf_to_ngp(const float *m, const ViewParams &V, float *out)
{
    float r[3][4];
    for (int i = 0; i < 3; i++) {
        r[i][0] = m[i * 4 + 0];
        r[i][1] = -m[i * 4 + 1];
        r[i][2] = -m[i * 4 + 2];
        r[i][3] = m[i * 4 + 3] * V.scale + V.offset[i];
    }
    for (int c = 0; c < 4; c++) {
        out[0 * 4 + c] = r[1][c];
        out[1 * 4 + c] = r[2][c];
        out[2 * 4 + c] = r[0][c];
    }
}

__global__ void k_cameras_direct(ViewParams V, const float *__restrict__ cams_nerf, uint32_t n,
                                 float *__restrict__ cams_out)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float m[12], o[12];
    for (int j = 0; j < 12; j++) m[j] = cams_nerf[i * 12 + j];
    nerf_to_ngp(m, V, o);
    for (int j = 0; j < 12; j++) cams_out[i * 12 + j] = o[j];
}

struct Mat16 { float v[16]; };

// convert_virtual_pose (reference combined_rendering.py:250-263):
//   T_WC_2 = T_WO_1 @ (inv(T_WO_2) @ T_WO_1) @ (inv(T_WO_1) @ T_WC_1), fp64
__global__ void k_cameras_virtual(ViewParams V, Mat16 obj_now, Mat16 cam, const float *__restrict__ obj_poses,
                                  uint32_t n, float *__restrict__ cams_out)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double T1[16], T2[16], TC[16], I2[16], I1[16], A[16], B[16], C[16], R[16];
    for (int j = 0; j < 16; j++) {
        T1[j] = (double)obj_now.v[j];
        TC[j] = (double)cam.v[j];
        T2[j] = (double)obj_poses[(size_t)i * 16 + j];
    }
    inv4(T2, I2);
    inv4(T1, I1);
    mul4(I2, T1, A);   // T_O2_O1
    mul4(I1, TC, B);   // T_O1_C1
    mul4(T1, A, C);
    mul4(C, B, R);
    float m[12], o[12];
    for (int j = 0; j < 12; j++) m[j] = (float)R[j];   // np.matrix(cam)[:-1,:] -> float32 in pyngp
    nerf_to_ngp(m, V, o);
    for (int j = 0; j < 12; j++) cams_out[(size_t)i * 12 + j] = o[j];
}

#ifndef D2R_MARCH_PROF
#define D2R_MARCH_PROF 0              /* development: per-wave cycle stamps of the refill block, printed by a few waves */
#endif
#ifndef D2R_MARCH_ABLATE
#define D2R_MARCH_ABLATE 0            /* development: 1 no LDS-brick slots, 2 no global slots (HBM bricks / tables), 4 no MLPs, 8 no occupancy walk (fixed 16 samples per ray); wrong pixels, timing only */
#endif
#ifndef D2R_MARCH_RESERVE
#define D2R_MARCH_RESERVE 128          /* queue entries a wave reserves per atomic */
#endif

// --------------------------------------------------------------------- rays

struct Ray {
    float ox, oy, oz, dx, dy, dz;      // in the unit cube of the model's box (d is the unit direction / aabb_scale)
    float t0;                          // distance (world units) of lattice point 0
    uint32_t k_hi;
    uint32_t k1;                       // CONE only: last lattice point of the constant-step stretch, and its distance
    float t1;
};

// aabb_scale >= 2 (template parameter CONE): the lattice of a ray is the cone-stepping sequence
// t_{k+1} = t_k + max(dt, t_k / 256) in closed form -- t0 + k dt up to k1, t1 (1 + 1/256)^(k - k1) after it,
// the power as the fixed-order product of fp32 constants that oracle/d2r_oracle.c uses (same bits).
// (1 + 1/256)^n = hi[n >> 6] * lo[n & 63]: lo[i] = float(c^i), hi[j] = float(c^(64 j)), the powers accumulated in double by
// repeated multiplication — evaluated at COMPILE time here, by the same IEEE operations oracle/d2r_oracle.c runs at start-up
// (same bits).  The CONE kernels copy the 512 bytes into LDS: one multiply and two LDS reads per lattice point where the fixed-order
// product of twelve constants cost twelve selects and multiplies (round 5).
struct ConeTab { float lo[64], hi[64]; };
constexpr ConeTab make_cone_tab()
{
    ConeTab t{};
    double p = 1.0;
    for (int i = 0; i < 64; i++) {
        t.lo[i] = (float)p;
        p *= 1.00390625;
    }
    const double c64 = p;
    double q = 1.0;
    for (int j = 0; j < 64; j++) {
        t.hi[j] = (float)q;
        q *= c64;
    }
    return t;
}
__device__ const ConeTab d2r_cone_tab_dev = make_cone_tab();
__shared__ float d2r_cone_lds[128];          // [0, 64) lo, [64, 128) hi; only the CONE instantiations reference (and allocate) it
// every CONE kernel calls this once, before its first lattice_t (ends with a barrier)
__device__ __forceinline__ void cone_tab_to_lds()
{
    for (uint32_t i = threadIdx.x; i < 128; i += blockDim.x) d2r_cone_lds[i] = i < 64 ? d2r_cone_tab_dev.lo[i] : d2r_cone_tab_dev.hi[i - 64];
    __syncthreads();
}
__device__ __forceinline__ float cone_pow(uint32_t n)
{
    n = min(n, 4095u);
    return d2r_cone_lds[64 + (n >> 6)] * d2r_cone_lds[n & 63u];
}
template <bool CONE>
__device__ __forceinline__ float lattice_t(const Ray &r, uint32_t k)
{
    if (!CONE) return fmaf((float)k, D2R_DT, r.t0);
    return k <= r.k1 ? fmaf((float)k, D2R_DT, r.t0) : r.t1 * cone_pow(k - r.k1);
}
template <bool CONE>
__device__ __forceinline__ float lattice_dt(float t)
{
    return CONE ? fmaxf(D2R_DT, t * D2R_CONE) : D2R_DT;
}
// a lattice index at or below the one whose distance is t (conservative by `slack` points either way)
__device__ __forceinline__ float cone_index_of(const Ray &r, float t)
{
    if (t <= r.t1) return (t - r.t0) * D2R_INV_DT;
    return (float)r.k1 + __log2f(t / r.t1) * 177.79119873046875f;       // 1 / log2(1 + 1/256)
}

// The training view's lens (ViewParams.lens_mode == D2R_LENS_OPENCV; reference reconstruction/combined_rendering.py:98,116:
// set_camera_to_training_view makes the view's OpenCV lens the render lens).  Same float32 operation sequence as
// oracle/d2r_oracle.c lens_distortion_delta / lens_undistort (the library is built with -ffp-contract=off; the divisions are
// IEEE divisions): the offset the lens moves a pinhole direction (u, v, 1) by, and instant-ngp's Newton iteration on a
// central-difference Jacobian that inverts it for a pixel.  Three to four steps for the demo coefficients; the loop is per lane.
__device__ __forceinline__ void lens_delta(const float (&L)[4], float u, float v, float &du, float &dv)
{
    const float u2 = u * u, uv = u * v, v2 = v * v;
    const float r2 = u2 + v2;
    const float radial = L[0] * r2 + L[1] * r2 * r2;
    du = u * radial + 2.0f * L[2] * uv + L[3] * (r2 + 2.0f * u2);
    dv = v * radial + 2.0f * L[3] * uv + L[2] * (r2 + 2.0f * v2);
}
__device__ __forceinline__ void lens_undistort(const float (&L)[4], float &u, float &v)
{
    const float eps = 1.1920928955078125e-07f;
    const float x0 = u, y0 = v;
    float x = x0, y = y0;
    for (int it = 0; it < 100; it++) {
        const float s0 = fmaxf(eps, fabsf(1e-6f * x));
        const float s1 = fmaxf(eps, fabsf(1e-6f * y));
        float dx, dy, bx0, by0, fx0, fy0, bx1, by1, fx1, fy1;
        lens_delta(L, x, y, dx, dy);
        lens_delta(L, x - s0, y, bx0, by0);
        lens_delta(L, x + s0, y, fx0, fy0);
        lens_delta(L, x, y - s1, bx1, by1);
        lens_delta(L, x, y + s1, fx1, fy1);
        const float a = 1.0f + (fx0 - bx0) / (2.0f * s0);
        const float b = (fx1 - bx1) / (2.0f * s1);
        const float c = (fy0 - by0) / (2.0f * s0);
        const float d = 1.0f + (fy1 - by1) / (2.0f * s1);
        const float rx = x + dx - x0, ry = y + dy - y0;
        const float inv_det = 1.0f / (a * d - b * c);
        const float sx = (d * rx - b * ry) * inv_det;
        const float sy = (a * ry - c * rx) * inv_det;
        x -= sx;
        y -= sy;
        if (sx * sx + sy * sy < 1e-10f) break;
    }
    u = x;
    v = y;
}

// The undistorted direction depends on the pixel and the view only, not on the candidate: it is computed ONCE per view into a
// [H][W] float2 table (1.8 MB at 640x360, L2-resident) that make_ray reads — in the ray generators and again when the marcher
// rebuilds a ray at a refill — so the per-ray cost of the lens is one 8-byte load and the marcher's registers are untouched.
__global__ __launch_bounds__(256) void k_lens_table(ViewParams V, float2 *__restrict__ tab)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V.W * V.H) return;
    const uint32_t px = i % V.W, py = i / V.W;
    float u = ((float)px + 0.5f) / (float)V.W;
    float v = ((float)py + 0.5f) / (float)V.H;
    float dcx = (u - V.center[0]) * (float)V.W / V.focal[0];       // exactly make_ray's expressions
    float dcy = (v - V.center[1]) * (float)V.H / V.focal[1];
    lens_undistort(V.lens, dcx, dcy);
    tab[i] = make_float2(dcx, dcy);
}

// pixel -> ray, lattice origin and the [k_lo, k_hi] window in which occupied cells can lie.
// Same fma sequence as the oracle (d2r_oracle_render).
template <bool CONE>
__device__ __forceinline__ bool make_ray(const NerfParams &P, const ViewParams &V, const float *cam,
                                         uint32_t px, uint32_t py, Ray &r, uint32_t &k_lo)
{
    float u = ((float)px + 0.5f) / (float)V.W;
    float v = ((float)py + 0.5f) / (float)V.H;
    float dcx = (u - V.center[0]) * (float)V.W / V.focal[0];
    float dcy = (v - V.center[1]) * (float)V.H / V.focal[1];
    if (V.lens_tab) {                           // wave-uniform (a kernel argument): the view's undistorted directions, one per pixel (k_lens_table)
        const float2 t = V.lens_tab[py * V.W + px];
        dcx = t.x;
        dcy = t.y;
    }
    float d[3], o[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        d[i] = fmaf(cam[i * 4 + 2], 1.0f, fmaf(cam[i * 4 + 1], dcy, cam[i * 4 + 0] * dcx));
        o[i] = fmaf(d[i], V.near_distance, cam[i * 4 + 3]);
    }
    float inv_len = 1.0f / sqrtf(fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0])));
#pragma unroll
    for (int i = 0; i < 3; i++) d[i] *= inv_len;
    // the model's box (the unit cube, or (CONE) the cube of side 2 centred at 0.5) cropped to render_aabb
    float tmin = -INFINITY, tmax = INFINITY;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float inv = 1.0f / d[i];
        float t0 = (P.raabb_lo[i] - o[i]) * inv, t1 = (P.raabb_hi[i] - o[i]) * inv;
        tmin = fmaxf(tmin, fminf(t0, t1));
        tmax = fminf(tmax, fmaxf(t0, t1));
    }
    if (CONE) {
        // from here on in the unit cube of the box (side aabb_scale about 0.5); distances stay world distances
#pragma unroll
        for (int i = 0; i < 3; i++) {
            o[i] = fmaf(o[i] - 0.5f, P.inv_side, 0.5f);
            d[i] *= P.inv_side;
        }
    }
    float bmin = -INFINITY, bmax = INFINITY;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float inv = 1.0f / d[i];
        float b0 = (P.bbox_lo[i] - o[i]) * inv, b1 = (P.bbox_hi[i] - o[i]) * inv;
        bmin = fmaxf(bmin, fminf(b0, b1));
        bmax = fminf(bmax, fmaxf(b0, b1));
    }
    r.ox = o[0]; r.oy = o[1]; r.oz = o[2];
    r.dx = d[0]; r.dy = d[1]; r.dz = d[2];
    r.k1 = 0;
    r.t1 = 0.f;
    if (!(tmax >= tmin && tmax > 0.f)) return false;
    r.t0 = fmaxf(tmin, 0.0f) + 1e-6f;
    float hi = fminf(bmax, tmax);
    if (!(hi >= bmin) || hi < r.t0) return false;
    float lo = fmaxf(bmin, r.t0);
    if (CONE) {
        r.k1 = r.t0 >= D2R_T_LINEAR ? 0u : (uint32_t)ceilf((D2R_T_LINEAR - r.t0) * D2R_INV_DT);
        r.t1 = fmaf((float)r.k1, D2R_DT, r.t0);
        float kl = floorf(cone_index_of(r, lo)) - 2.0f;
        k_lo = kl > 0.f ? (uint32_t)kl : 0u;
        r.k_hi = (uint32_t)ceilf(cone_index_of(r, hi)) + 2u;
        return true;
    }
    float kl = floorf((lo - r.t0) * D2R_INV_DT) - 1.0f;
    k_lo = kl > 0.f ? (uint32_t)kl : 0u;
    r.k_hi = (uint32_t)ceilf((hi - r.t0) * D2R_INV_DT) + 1u;
    return true;
}

// Lattice point k of a ray: its distance, its position in the unit cube of the box, and the occupancy cell it falls into (cascade
// `mip`, cell (cx, cy, cz), cell size and origin of that cascade in box units).  inside = false: the point lies outside render_aabb.
struct OccCell {
    float t, px, py, pz, cell, corg;
    int mip, cx, cy, cz;
    bool inside;
};
template <bool CONE>
__device__ __forceinline__ OccCell occ_cell(const NerfParams &P, const Ray &r, uint32_t k)
{
    OccCell o;
    o.t = lattice_t<CONE>(r, k);
    const float px = fmaf(o.t, r.dx, r.ox), py = fmaf(o.t, r.dy, r.oy), pz = fmaf(o.t, r.dz, r.oz);
    o.px = px; o.py = py; o.pz = pz;
    o.inside = !(px < P.rn_lo[0] || px > P.rn_hi[0] || py < P.rn_lo[1] || py > P.rn_hi[1] || pz < P.rn_lo[2] || pz > P.rn_hi[2]);
    // occupancy cascade (CONE; n_casc = log2(aabb_scale) + 1 of them, cascade c the cube of side 2^c about 0.5 with
    // cells 2^c / 128): the smallest one that contains the sample, or a coarser one once the step has grown to
    // its cells (step * 256 >= 2^(c-1)) — instant-ngp's max(mip_from_pos, mip_from_dt) as believed
    int mip = 0;
    float qx = px, qy = py, qz = pz, cell = 1.0f / (float)D2R_GRID, corg = 0.f;
    if (CONE) {
        const float mxw = fmaxf(fmaxf(fabsf(px - 0.5f), fabsf(py - 0.5f)), fabsf(pz - 0.5f)) * P.side;   // world units
        const float dt256 = lattice_dt<CONE>(o.t) * 256.0f;
        const int top = (int)P.n_casc - 1;
        float half = 0.5f, step = 1.0f;
        for (int c = 1; c <= top; c++) {
            if (mxw >= half || dt256 >= step) mip = c;
            half *= 2.0f;
            step *= 2.0f;
        }
        if (mip != top) {
            // the sample in the unit cube of cascade `mip`: scale about the centre by aabb_scale / 2^mip
            const float sc = P.side / (float)(1 << mip);
            qx = fmaf(px - 0.5f, sc, 0.5f);
            qy = fmaf(py - 0.5f, sc, 0.5f);
            qz = fmaf(pz - 0.5f, sc, 0.5f);
            cell = 1.0f / ((float)D2R_GRID * sc);
            corg = 0.5f - 0.5f / sc;
        }
    }
    o.mip = mip; o.cell = cell; o.corg = corg;
    o.cx = min(max((int)(qx * (float)D2R_GRID), 0), D2R_GRID - 1);
    o.cy = min(max((int)(qy * (float)D2R_GRID), 0), D2R_GRID - 1);
    o.cz = min(max((int)(qz * (float)D2R_GRID), 0), D2R_GRID - 1);
    return o;
}
__device__ __forceinline__ const uint64_t *occ_word_ptr(const NerfParams &P, const OccCell &o)
{
    return P.bricks + ((size_t)o.mip * 32768 + (o.cx >> 2) + 32 * ((o.cy >> 2) + 32 * (o.cz >> 2)));
}

// Advance k to the next lattice sample t0+k*dt that lies in an occupied cell.
// Empty 4^3 bricks / empty cells are skipped conservatively (never past an untested
// lattice point that could be in another cell).  Returns false when the ray is finished.
template <bool CONE>
__device__ __forceinline__ bool next_sample(const NerfParams &P, const Ray &r, uint32_t &k, float &px,
                                            float &py, float &pz)
{
    // approximate reciprocals are enough: they only size the conservative skip below
    float ix = __builtin_amdgcn_rcpf(r.dx), iy = __builtin_amdgcn_rcpf(r.dy), iz = __builtin_amdgcn_rcpf(r.dz);
    while (k <= r.k_hi) {
        const OccCell o = occ_cell<CONE>(P, r, k);
        const float t = o.t;
        px = o.px; py = o.py; pz = o.pz;
        if (!o.inside) return false;
        const int mip = o.mip, cx = o.cx, cy = o.cy, cz = o.cz;
        const float cell = o.cell, corg = o.corg;
        const uint64_t w = *occ_word_ptr(P, o);
        uint32_t bit = (cx & 3) + 4 * (cy & 3) + 16 * (cz & 3);
        if ((w >> bit) & 1ull) return true;
        // skip: to the far face of the empty brick, or of the empty cell (box units: cell size `cell`, origin `corg`)
        int sh = (w == 0ull) ? 2 : 0;
        float cs = (float)(1 << sh) * cell;
        float lx = fmaf((float)((cx >> sh) << sh), cell, corg);
        float ly = fmaf((float)((cy >> sh) << sh), cell, corg);
        float lz = fmaf((float)((cz >> sh) << sh), cell, corg);
        float tx = ((r.dx > 0.f ? lx + cs : lx) - px) * ix;
        float ty = ((r.dy > 0.f ? ly + cs : ly) - py) * iy;
        float tz = ((r.dz > 0.f ? lz + cs : lz) - pz) * iz;
        float dist = fminf(fminf(tx, ty), tz);
        // whole steps that surely stay inside the skipped region: the steps only grow along the ray, so
        // sizing them by the step at the far end is conservative; and never across a distance at which
        // the cascade choice changes with the step size (t = 1, 2, 4, ...)
        int n;
        if (CONE) {
            if (mip != (int)P.n_casc - 1) {
                float tb = 1.0f;
                while (tb <= t) tb *= 2.0f;
                dist = fminf(dist, tb - t);
            }
            n = (int)floorf(dist / lattice_dt<CONE>(t + fmaxf(dist, 0.f)));
        } else {
            n = (int)floorf(dist * D2R_INV_DT);
        }
        k += (uint32_t)max(n, 1);
    }
    return false;
}

// ray sort: the bin (Morton order over 2^L x 2^L x 2^L cells of the occupied box) of a ray's first sample, as bits 20.. of the queue
// entry's k (k < 2^20 always: lattice points are at least dt_min = sqrt(3)/1024 apart and a ray crosses at most the box diagonal,
// sqrt(3) * aabb_scale <= sqrt(3) * 128, i.e. k <= 2^17 even without cone stepping)
#define D2R_SORT_SHIFT 20
__device__ __forceinline__ uint32_t sort_tag(const NerfParams &P, float x, float y, float z)
{
    if (P.sort_log2 == 0) return 0u;
    const uint32_t n1 = 1u << P.sort_log2;
    uint32_t c[3];
    const float p[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float u = (p[a] - P.bbox_lo[a]) / (P.bbox_hi[a] - P.bbox_lo[a]) * (float)n1;
        c[a] = min((uint32_t)fmaxf(u, 0.f), n1 - 1u);
    }
    uint32_t bin = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) bin |= (((c[0] >> b) & 1u) << (3 * b)) | (((c[1] >> b) & 1u) << (3 * b + 1)) | (((c[2] >> b) & 1u) << (3 * b + 2));
    return bin << D2R_SORT_SHIFT;
}

__device__ __forceinline__ void empty_pixel(const ViewParams &V, float *rgba)
{
    // no sample: C = 0, A = 0 -> background blend only
    rgba[0] = V.background[3] * V.background[0];
    rgba[1] = V.background[3] * V.background[1];
    rgba[2] = V.background[3] * V.background[2];
    rgba[3] = V.background[3];
}

// grid: (tiles of 16x16 pixels, n_cams); block 256 = 4 waves, each wave an 8x8 pixel tile
template <bool CONE>
__global__ __launch_bounds__(256) void k_raygen(NerfParams P, ViewParams V, const float *__restrict__ cams,
                                                uint2 *__restrict__ queue, uint32_t *__restrict__ qcount,
                                                float *__restrict__ rgba_out, float *__restrict__ depth_out)
{
    if (CONE) cone_tab_to_lds();
    const uint32_t tiles_x = (V.W + 15) / 16;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t px = (blockIdx.x % tiles_x) * 16 + (wave & 1) * 8 + (lane & 7);
    const uint32_t py = (blockIdx.x / tiles_x) * 16 + (wave >> 1) * 8 + (lane >> 3);
    const uint32_t cam_i = blockIdx.y;
    const bool inside = px < V.W && py < V.H;
    bool alive = false;
    uint32_t k = 0;
    if (inside) {
        float cam[12];
#pragma unroll
        for (int j = 0; j < 12; j++) cam[j] = cams[(size_t)cam_i * 12 + j];
        Ray r;
        if (make_ray<CONE>(P, V, cam, px, py, r, k)) {
            float x, y, z;
            alive = next_sample<CONE>(P, r, k, x, y, z);
            if (alive) k |= sort_tag(P, x, y, z);
        }
    }
    const uint32_t ray_id = cam_i * (V.W * V.H) + py * V.W + px;
    // wave-level compaction: one atomic per wave
    unsigned long long m = __ballot(alive);
    if (m) {
        uint32_t cnt = (uint32_t)__popcll(m), base = 0;
        if (lane == (uint32_t)__ffsll((long long)m) - 1) base = atomicAdd(qcount, cnt);
        base = __shfl(base, __ffsll((long long)m) - 1);
        if (alive) {
            uint32_t off = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            queue[base + off] = make_uint2(ray_id, k);
        }
    }
    if (inside && !alive && rgba_out) {
        float e[4];
        empty_pixel(V, e);
        *(float4 *)(rgba_out + (size_t)ray_id * 4) = make_float4(e[0], e[1], e[2], e[3]);
        depth_out[ray_id] = 0.f;
    }
}

// Composite mode (frames already hold the background): only pixels whose ray can reach the occupied
// bounding box need a ray.  All rays leave the camera centre, so with the eight box corners in front
// of the camera the box projects into the bounding rectangle of the projected corners; the block
// walks the 16x16 tiles of that rectangle (+2 px) instead of the whole frame.  A camera that is not a
// rigid transform, or a corner at or behind the camera plane, falls back to the full frame.
// grid: (n_cams, parts); block 256 = 4 waves, each wave an 8x8 pixel tile.
template <bool CONE>
__global__ __launch_bounds__(256) void k_raygen_rect(NerfParams P, ViewParams V, const float *__restrict__ cams,
                                                     uint2 *__restrict__ queue, uint32_t *__restrict__ qcount,
                                                     int4 *__restrict__ rects)
{
    if (CONE) cone_tab_to_lds();
    const uint32_t cam_i = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float cam[12];
#pragma unroll
    for (int j = 0; j < 12; j++) cam[j] = cams[(size_t)cam_i * 12 + j];
    int x0 = 0, y0 = 0, x1 = (int)V.W - 1, y1 = (int)V.H - 1;
    {
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = a; b < 3; b++) {
                const float dot = cam[a] * cam[b] + cam[4 + a] * cam[4 + b] + cam[8 + a] * cam[8 + b];
                ok = ok && fabsf(dot - (a == b ? 1.0f : 0.0f)) < 1e-3f;
            }
        // the box's corners in the camera's normalised plane (x / z, y / z): with every corner in front of the camera the
        // box's pinhole projection lies inside their bounding rectangle [u0, u1] x [v0, v1]
        float u0 = INFINITY, u1 = -INFINITY, v0 = INFINITY, v1 = -INFINITY;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            // box-unit corner -> world (CONE: the box is the cube of side 2 about 0.5)
            const float wx = (c & 1) ? P.bbox_hi[0] : P.bbox_lo[0], wy = (c & 2) ? P.bbox_hi[1] : P.bbox_lo[1];
            const float wz = (c & 4) ? P.bbox_hi[2] : P.bbox_lo[2];
            const float qx = (CONE ? fmaf(wx - 0.5f, P.side, 0.5f) : wx) - cam[3];
            const float qy = (CONE ? fmaf(wy - 0.5f, P.side, 0.5f) : wy) - cam[7];
            const float qz = (CONE ? fmaf(wz - 0.5f, P.side, 0.5f) : wz) - cam[11];
            const float cx = cam[0] * qx + cam[4] * qy + cam[8] * qz;      // R^T (p - t)
            const float cy = cam[1] * qx + cam[5] * qy + cam[9] * qz;
            const float cz = cam[2] * qx + cam[6] * qy + cam[10] * qz;
            ok = ok && cz > 1e-3f;                                          // false for NaN too
            const float un = cx / cz, vn = cy / cz;
            u0 = fminf(u0, un); u1 = fmaxf(u1, un);
            v0 = fminf(v0, vn); v1 = fmaxf(v1, vn);
        }
        ok = ok && u1 - u0 < 1e6f && v1 - v0 < 1e6f;                       // finite
        float margin = 2.f;                                                 // pixels
        if (ok && V.lens_mode == D2R_LENS_OPENCV) {
            // A pixel needs a ray when its UNDISTORTED direction falls into that rectangle, i.e. when its own (distorted) sensor
            // position lies in the image D(rect) of the rectangle under the forward lens map D(x) = x + delta(x).  D is a local
            // diffeomorphism on the rectangle (checked: det J > 0.1 on the boundary samples), so the outline of D(rect) is the
            // image of the rectangle's outline: lane l evaluates D at outline point l (16 per edge), the wave reduces the four
            // extremes, and what the outline can bulge by BETWEEN two samples (h^2 / 8 max|D''| for spacing h) widens the margin.
            const uint32_t e = lane >> 4;
            const float s_ = (float)(lane & 15u) * (1.0f / 15.0f);
            const float bu = e == 0 ? fmaf(s_, u1 - u0, u0) : e == 1 ? u1 : e == 2 ? fmaf(s_, u1 - u0, u0) : u0;
            const float bv = e == 0 ? v0 : e == 1 ? fmaf(s_, v1 - v0, v0) : e == 2 ? v1 : fmaf(s_, v1 - v0, v0);
            float du, dv;
            lens_delta(V.lens, bu, bv, du, dv);
            float lu0 = bu + du, lu1 = lu0, lv0 = bv + dv, lv1 = lv0;
            // Jacobian of D at the sample, analytically
            const float k1 = V.lens[0], k2 = V.lens[1], p1 = V.lens[2], p2 = V.lens[3];
            const float r2 = bu * bu + bv * bv;
            const float rad = k1 * r2 + k2 * r2 * r2, drad = 2.f * k1 + 4.f * k2 * r2;            // d rad / d (r^2) * 2
            const float jxx = 1.f + rad + bu * bu * drad + 2.f * p1 * bv + 6.f * p2 * bu;
            const float jxy = bu * bv * drad + 2.f * p1 * bu + 2.f * p2 * bv;
            const float jyy = 1.f + rad + bv * bv * drad + 2.f * p2 * bu + 6.f * p1 * bv;
            float detmin = jxx * jyy - jxy * jxy;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                lu0 = fminf(lu0, __shfl_xor(lu0, m)); lu1 = fmaxf(lu1, __shfl_xor(lu1, m));
                lv0 = fminf(lv0, __shfl_xor(lv0, m)); lv1 = fmaxf(lv1, __shfl_xor(lv1, m));
                detmin = fminf(detmin, __shfl_xor(detmin, m));
            }
            const float R = sqrtf(fmaxf(u0 * u0, u1 * u1) + fmaxf(v0 * v0, v1 * v1));
            const float d2max = 6.f * fabsf(k1) * R + 20.f * fabsf(k2) * R * R * R + 6.f * (fabsf(p1) + fabsf(p2));
            const float h = fmaxf(u1 - u0, v1 - v0) * (1.0f / 15.0f);
            margin += h * h * 0.125f * d2max * fmaxf(V.focal[0], V.focal[1]);
            ok = ok && detmin > 0.1f && margin < 1e6f;                      // false for NaN too
            u0 = lu0; u1 = lu1; v0 = lv0; v1 = lv1;
        }
        if (ok) {
            // pixel whose centre has the sensor position (u, v): c W + u f - 0.5
            const float pxmin = fmaf(u0, V.focal[0], V.center[0] * (float)V.W) - 0.5f, pxmax = fmaf(u1, V.focal[0], V.center[0] * (float)V.W) - 0.5f;
            const float pymin = fmaf(v0, V.focal[1], V.center[1] * (float)V.H) - 0.5f, pymax = fmaf(v1, V.focal[1], V.center[1] * (float)V.H) - 0.5f;
            const int mg = (int)ceilf(margin);
            x0 = max(x0, (int)floorf(fmaxf(pxmin, -4.f)) - mg);
            y0 = max(y0, (int)floorf(fmaxf(pymin, -4.f)) - mg);
            x1 = min(x1, (int)ceilf(fminf(pxmax, (float)V.W + 4.f)) + mg);
            y1 = min(y1, (int)ceilf(fminf(pymax, (float)V.H + 4.f)) + mg);
        }
    }
    if (x0 > x1 || y0 > y1) {                                               // the box is off screen
        if (rects && blockIdx.y == 0 && threadIdx.x == 0) rects[cam_i] = make_int4(1, 1, 0, 0);     // empty
        return;
    }
    const int tx0 = x0 >> 4, ty0 = y0 >> 4, ntx = (x1 >> 4) - tx0 + 1, nty = (y1 >> 4) - ty0 + 1;
    // the pixels this candidate's rays can write: the 16x16 tiles walked below (for the CLIP preprocess's fast path)
    if (rects && blockIdx.y == 0 && threadIdx.x == 0)
        rects[cam_i] = make_int4(tx0 * 16, ty0 * 16, min((int)V.W, (tx0 + ntx) * 16) - 1, min((int)V.H, (ty0 + nty) * 16) - 1);
    // live rays are collected in LDS and appended to the global queue with ONE atomic per flush: the
    // queue counter is a single address, and one atomic per wave (~10^6 per pass) was what bounded
    // the full-frame generator
    constexpr uint32_t CAP = 2048;
    __shared__ uint2 pending[CAP];
    __shared__ uint32_t n_pending, flush_base;
    if (threadIdx.x == 0) n_pending = 0;
    __syncthreads();
    auto flush = [&]() {                       // block-uniform call sites only
        __syncthreads();
        const uint32_t np_ = n_pending;
        if (threadIdx.x == 0 && np_) flush_base = atomicAdd(qcount, np_);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < np_; i += 256) queue[flush_base + i] = pending[i];
        __syncthreads();
        if (threadIdx.x == 0) n_pending = 0;
        __syncthreads();
    };
    uint32_t since_flush = 0;
    for (int t = (int)blockIdx.y; t < ntx * nty; t += (int)gridDim.y) {
        if (since_flush + 256 > CAP) {         // worst case every pixel of every tile so far is live
            flush();
            since_flush = 0;
        }
        since_flush += 256;
        const uint32_t px = (uint32_t)(tx0 + t % ntx) * 16 + (wave & 1) * 8 + (lane & 7);
        const uint32_t py = (uint32_t)(ty0 + t / ntx) * 16 + (wave >> 1) * 8 + (lane >> 3);
        bool alive = false;
        uint32_t k = 0;
        if (px < V.W && py < V.H) {
            Ray r;
            if (make_ray<CONE>(P, V, cam, px, py, r, k)) {
                float x, y, z;
                alive = next_sample<CONE>(P, r, k, x, y, z);
                if (alive) k |= sort_tag(P, x, y, z);
            }
        }
        const uint32_t ray_id = cam_i * (V.W * V.H) + py * V.W + px;
        unsigned long long m = __ballot(alive);
        if (m) {
            uint32_t cnt = (uint32_t)__popcll(m), base = 0;
            if (lane == (uint32_t)__ffsll((long long)m) - 1) base = atomicAdd(&n_pending, cnt);
            base = __shfl(base, __ffsll((long long)m) - 1);
            if (alive) {
                uint32_t off = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                pending[base + off] = make_uint2(ray_id, k);
            }
        }
    }
    flush();
}

// --------------------------------------------------------------- ray sort
//
// Where the bricks behind the LDS slots outgrow the L2s the marcher is bound by the L2-miss path: at any moment its ~3000 waves march
// rays of ~50 candidates through every part of the object.  All candidates render the SAME object, so the rays are marched in the
// order of the object region their first sample lies in (a stable counting sort of the queue on the tag k_raygen* left in the
// entries): the waves running at one time then read the bricks of a few neighbouring regions.  Three small passes over the queue
// (8 bytes per ray each): per-chunk bin counts, a scan per bin over the chunks + a scan over the bins, the scatter.  The order of
// the entries of one bin within a chunk is whatever the LDS atomics give: the frames do not depend on the order rays are marched in.
#define D2R_SORT_CHUNK 16384u        /* entries per block and pass: [bins][chunks] counters = 1 GB for the worst case of a configs[1] pass (every pixel a ray) */
#define D2R_SORT_BINS 4096u          /* 16 x 16 x 16 at most (ray_sort_log2 = 4) */
__global__ __launch_bounds__(256) void k_sort_count(const uint2 *__restrict__ queue, const uint32_t *__restrict__ qcount, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t hist[D2R_SORT_BINS];
    const uint32_t n = *qcount, nchunks = (n + D2R_SORT_CHUNK - 1) / D2R_SORT_CHUNK;
    for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        for (uint32_t i = threadIdx.x; i < D2R_SORT_BINS; i += 256) hist[i] = 0;
        __syncthreads();
        for (uint32_t i = c * D2R_SORT_CHUNK + threadIdx.x; i < min(n, (c + 1) * D2R_SORT_CHUNK); i += 256) atomicAdd(&hist[queue[i].y >> D2R_SORT_SHIFT], 1u);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < D2R_SORT_BINS; i += 256) counts[(size_t)i * nchunks + c] = hist[i];     // bin-major: the scan below reads rows
        __syncthreads();
    }
}
// one block per bin: exclusive scan of its row of chunk counts, the row's total to bin_total
__global__ __launch_bounds__(256) void k_sort_scan_rows(const uint32_t *__restrict__ qcount, uint32_t *__restrict__ counts, uint32_t *__restrict__ bin_total)
{
    const uint32_t n = *qcount, nchunks = (n + D2R_SORT_CHUNK - 1) / D2R_SORT_CHUNK;
    uint32_t *row = counts + (size_t)blockIdx.x * nchunks;
    const uint32_t total = d2r_block_scan_row(row, row, nchunks);
    if (threadIdx.x == 0) bin_total[blockIdx.x] = total;
}
// exclusive scan of the bin totals (one block)
__global__ __launch_bounds__(256) void k_sort_scan_bins(const uint32_t *__restrict__ bin_total, uint32_t *__restrict__ bin_base)
{
    d2r_block_scan_row(bin_total, bin_base, D2R_SORT_BINS);
}
__global__ __launch_bounds__(256) void k_sort_scatter(const uint2 *__restrict__ queue, const uint32_t *__restrict__ qcount, const uint32_t *__restrict__ counts,
                                                      const uint32_t *__restrict__ bin_base, uint2 *__restrict__ sorted)
{
    __shared__ uint32_t cursor[D2R_SORT_BINS];
    const uint32_t n = *qcount, nchunks = (n + D2R_SORT_CHUNK - 1) / D2R_SORT_CHUNK;
    for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        for (uint32_t i = threadIdx.x; i < D2R_SORT_BINS; i += 256) cursor[i] = bin_base[i] + counts[(size_t)i * nchunks + c];
        __syncthreads();
        for (uint32_t i = c * D2R_SORT_CHUNK + threadIdx.x; i < min(n, (c + 1) * D2R_SORT_CHUNK); i += 256) {
            const uint2 e = queue[i];
            sorted[atomicAdd(&cursor[e.y >> D2R_SORT_SHIFT], 1u)] = make_uint2(e.x, e.y & ((1u << D2R_SORT_SHIFT) - 1u));
        }
        __syncthreads();
    }
}

// ------------------------------------------------------- field evaluation

template <bool F16>
__device__ __forceinline__ f32x16 mfma(const uint4 &a, const uint4 &b, f32x16 c)
{
    Frag fa, fb;
    fa.u = a;
    fb.u = b;
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(fa.h, fb.h, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v, fb.v, c, 0, 0, 0);
}

enum { K_DENSE = 0, K_HASH = 1, K_MIXED = 2, K_BRICK = 3 };

// kind of slot i: the first NB slots are bricks (LDS, then NGB of them in HBM); otherwise
// dense/hashed/mixed from the number of leading dense levels ND (ND < 0: every slot mixed)
template <int NB, int ND>
__device__ __host__ constexpr int slot_kind(int i)
{
    return i < NB ? K_BRICK : (ND < 0 ? K_MIXED : (2 * i + 1 < ND ? K_DENSE : (2 * i >= ND ? K_HASH : K_MIXED)));
}

// Addresses + interpolation fractions of one slot (this lane's level of the pair) of one sample.
// One address op per corner; the slot table base rides in the SGPR soffset of the buffer load.
template <int KIND>
__device__ __forceinline__ void slot_addr(const NerfParams &P, int slot, bool hi, float x, float y, float z,
                                          uint32_t *off, float *w)
{
    const SlotMeta &m = P.slot[slot];
    const float scale = hi ? m.scale[1] : m.scale[0];
    float p0 = fmaf(scale, x, 0.5f), p1 = fmaf(scale, y, 0.5f), p2 = fmaf(scale, z, 0.5f);
    float f0 = floorf(p0), f1 = floorf(p1), f2 = floorf(p2);
    w[0] = p0 - f0;
    w[1] = p1 - f1;
    w[2] = p2 - f2;
    uint32_t gx = (uint32_t)(int)f0, gy = (uint32_t)(int)f1, gz = (uint32_t)(int)f2;
    const uint32_t h4 = hi ? 4u : 0u;
    if (KIND == K_BRICK) {
        // bounding-box-local dense brick in LDS: byte offset of corner (0,0,0), then +x, +y, +z strides.  (Measured and
        // dropped in round 4: v_fract_f32 + p - fract for the floor, and the vertex index formed in fp32 from brick-local
        // coordinates — 8 % fewer VALU instructions, but the extra per-lane loop invariants spill inside the march loop:
        // 26.3 -> 33.1 ms per launch.)
        const uint32_t nx = hi ? m.bnx[1] : m.bnx[0], nxy = hi ? m.bnxy[1] : m.bnxy[0];
        const int32_t base = hi ? m.bbase[1] : m.bbase[0];
        const uint32_t b = (uint32_t)((int32_t)(gx + nx * gy + nxy * gz) + base) << 2;
#pragma unroll
        for (int c = 0; c < 8; c++) off[c] = b + ((c & 1) ? 4u : 0u) + ((c & 2) ? nx << 2 : 0u) + ((c & 4) ? nxy << 2 : 0u);
    } else if (KIND == K_HASH) {
        // everything pre-shifted by 3: ((a<<3) ^ (b<<3)) & (mask<<3|4) == ((a^b)&mask)<<3 | h4
        const uint32_t x0 = (gx << 3) | h4, x1 = x0 + 8u;
        const uint32_t y0 = gy * (2654435761u << 3), y1 = y0 + (2654435761u << 3);
        const uint32_t z0 = gz * (805459861u << 3), z1 = z0 + (805459861u << 3);
        const uint32_t yz[4] = {y0 ^ z0, y1 ^ z0, y0 ^ z1, y1 ^ z1};
#pragma unroll
        for (int c = 0; c < 8; c++) off[c] = (((c & 1) ? x1 : x0) ^ yz[c >> 1]) & m.mask8;
    } else {
        const uint32_t res = hi ? m.res[1] : m.res[0];
        const uint32_t size = hi ? m.size[1] : m.size[0];
        const bool hashed = KIND == K_MIXED && ((hi ? m.hashed[1] : m.hashed[0]) != 0);
        const uint32_t my = hashed ? 2654435761u : res;
        const uint32_t mz = hashed ? 805459861u : res * res;
        const uint32_t y0 = gy * my, y1 = y0 + my, z0 = gz * mz, z1 = z0 + mz;
        const uint32_t yzd[4] = {y0 + z0, y1 + z0, y0 + z1, y1 + z1};
        const uint32_t yzh[4] = {y0 ^ z0, y1 ^ z0, y0 ^ z1, y1 ^ z1};
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const uint32_t a = gx + (c & 1);
            // dense: tiny-cuda-nn's idx % size (the index reaches `size` only on the far cube faces)
            uint32_t idx = a + yzd[c >> 1];
            idx = min(idx, idx - size);        // unsigned: idx - size wraps huge unless idx >= size
            if (KIND == K_MIXED) idx = hashed ? ((a ^ yzh[c >> 1]) & (size - 1u)) : idx;
            off[c] = (idx << 3) | h4;
        }
    }
}

// trilinear blend of the 8 corner entries, corner weights in the oracle's order ((wx*wy)*wz).
// v_fma_mix_f32 multiplies the fp32 weight with one half of the packed fp16 pair and accumulates
// in fp32 directly — no fp16->fp32 converts (hipcc does not form it with fp32 denormals on).
__device__ __forceinline__ void slot_blend(const uint32_t *raw, const float *w, float &o0, float &o1)
{
    // the twelve weight products of a level as six packed fp32 multiplies (v_pk_mul_f32: two products per issue slot,
    // the same roundings as the scalar multiplies: (wx * wy) * wz in the oracle's order)
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const float ux = 1.0f - w[0], uy = 1.0f - w[1], uz = 1.0f - w[2];
    const f32x2 wx = {ux, w[0]};
    const f32x2 xy01 = wx * (f32x2){uy, uy}, xy23 = wx * (f32x2){w[1], w[1]};
    const f32x2 c01 = xy01 * (f32x2){uz, uz}, c23 = xy23 * (f32x2){uz, uz}, c45 = xy01 * (f32x2){w[2], w[2]}, c67 = xy23 * (f32x2){w[2], w[2]};
    const float wcs[8] = {c01.x, c01.y, c23.x, c23.y, c45.x, c45.y, c67.x, c67.y};
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const float wc = wcs[c];
        asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[0,1,0]" : "+v"(a0) : "v"(wc), "v"(raw[c]));
        asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "+v"(a1) : "v"(wc), "v"(raw[c]));
    }
    o0 = a0;
    o1 = a1;
}

// fp32 operation, then ONE round-to-nearest-even conversion to half (subnormal halves kept: the kernels run with fp16 denormals on).
// The empty asm keeps the fp32 result in a register of its own (no instruction): without it hipcc fuses the convert into the operation
// — fptrunc(fma) becomes v_fma_mixlo_f16 — and that instruction rounds the exact result ONCE, to half, where the definition rounds
// to fp32 first: measured on MI355X, 2 .. 11 of 20 000 features off by one half ulp in the fma form (tests/test_render_arith_gpu.py
// test_grid_encoding_is_bit_exact).
__device__ __forceinline__ float rn16(float x)
{
    asm("" : "+v"(x));
    return (float)(_Float16)x;
}

// The same blend in tiny-cuda-nn's half arithmetic (option "render_arith" 1 / 2; oracle/d2r_oracle.c hashgrid_encode under
// d2r_oracle_set_arith, operation by operation): one accumulator per feature from 0, corners c = 0 .. 7 in that order (bit d of
// c chooses dimension d: the order of raw[] on every path), the fp32 weight built as ((1 wx) wy) wz,
//   ARITH 1: acc = rn16(acc + rn16(weight val))        ARITH 2: acc = rn16(fmaf(rn16(weight), val, acc))
// Held bit-exact against the oracle (test_grid_encoding_is_bit_exact).  A validation mode: scalar converts and adds, no packed tricks.
template <int ARITH>
__device__ __forceinline__ void slot_blend_half(const uint32_t *raw, const float *w, float &o0, float &o1)
{
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        float wc = 1.0f;
#pragma unroll
        for (int d = 0; d < 3; d++) wc *= (c & (1 << d)) ? w[d] : 1.0f - w[d];
        union { uint32_t u; f16x2 v; } e;
        e.u = raw[c];
        const float v0 = (float)e.v[0], v1 = (float)e.v[1];
        if constexpr (ARITH == 1) {
            a0 = rn16(a0 + rn16(wc * v0));
            a1 = rn16(a1 + rn16(wc * v1));
        } else {
            const float wh = rn16(wc);
            a0 = rn16(fmaf(wh, v0, a0));
            a1 = rn16(fmaf(wh, v1, a1));
        }
    }
    o0 = a0;
    o1 = a1;
}
template <int ARITH>
__device__ __forceinline__ void slot_blend_as(const uint32_t *raw, const float *w, float &o0, float &o1)
{
    if constexpr (ARITH == 0) slot_blend(raw, w, o0, o1);
    else slot_blend_half<ARITH>(raw, w, o0, o1);
}

// compile-time loop: f(std::integral_constant<int, B>{}), ..., f(std::integral_constant<int, E - 1>{})
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

// Global slots [S0, S0 + CNT) of one sample in three phases — all their addresses, then all their gathers issued
// back-to-back (memory-level parallelism is what bounds this kernel), then `under()` (work that needs no global data: the
// LDS-brick slots) while those are in flight, then the blends.  Slots below NB + NGB come from dense HBM bricks, where the two
// x-neighbour corners are adjacent words: ONE 8-byte gather per (y, z) pair halves the lane-gathers (the texture addresser's
// cost is per lane); the others from the slot tables (dense / hashed / mixed by ND).
template <int NB, int NGB, int ND, int S0, int CNT, int ARITH, class Under>
__device__ __forceinline__ void encode_batch(const NerfParams &P, const __amdgpu_buffer_rsrc_t &rs, const __amdgpu_buffer_rsrc_t &rsb,
                                             bool hi, float x, float y, float z, float *f, Under &&under)
{
    uint32_t off[CNT][8];
    float w[CNT][3];
    uint32_t raw[CNT][8];
    static_for<0, CNT>([&](auto j) {
        constexpr int I = S0 + decltype(j)::value;
        if constexpr (I < NB + NGB) slot_addr<K_BRICK>(P, I, hi, x, y, z, off[decltype(j)::value], w[decltype(j)::value]);
        else slot_addr<slot_kind<NB + NGB, ND>(I)>(P, I, hi, x, y, z, off[decltype(j)::value], w[decltype(j)::value]);
    });
    __builtin_amdgcn_sched_barrier(0);
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    static_for<0, CNT>([&](auto j) {
        constexpr int J = decltype(j)::value, I = S0 + J;
        if constexpr (I < NB + NGB) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsb, off[J][2 * q], 0, 0);
                raw[J][2 * q] = v[0];
                raw[J][2 * q + 1] = v[1];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 8; c++) raw[J][c] = __builtin_amdgcn_raw_buffer_load_b32(rs, off[J][c], P.slot[I].off, 0);
        }
    });
    __builtin_amdgcn_sched_barrier(0);
    under();
    static_for<0, CNT>([&](auto j) {
        constexpr int J = decltype(j)::value, I = S0 + J;
        slot_blend_as<ARITH>(raw[J], w[J], f[2 * I], f[2 * I + 1]);
    });
}

// global slots S0 .. 7 in batches: at most four slots per batch while they are bricks (4 address registers per slot survive
// into the load phase: the base and three strides are shared), at most three once table slots (eight independent
// addresses each, plus the dense / hashed index arithmetic) are among them
template <int NB, int NGB, int ND, int S0, int ARITH, class Under>
__device__ __forceinline__ void encode_from(const NerfParams &P, const __amdgpu_buffer_rsrc_t &rs, const __amdgpu_buffer_rsrc_t &rsb,
                                            bool hi, float x, float y, float z, float *f, Under &&under)
{
    constexpr int LEFT = 8 - S0;
    constexpr int BMAX = (S0 + 4 <= NB + NGB) ? 4 : 3;
    // split the remainder evenly over the batches it needs (5 -> 3 + 2, 8 -> 3 + 3 + 2 or 4 + 4)
    constexpr int NBATCH = (LEFT + BMAX - 1) / BMAX;
    constexpr int CNT = (LEFT + NBATCH - 1) / NBATCH;
    encode_batch<NB, NGB, ND, S0, CNT, ARITH>(P, rs, rsb, hi, x, y, z, f, under);
    if constexpr (LEFT > CNT) encode_from<NB, NGB, ND, S0 + CNT, ARITH>(P, rs, rsb, hi, x, y, z, f, [] {});
}

// All 8 slots of one sample.  f[2*i], f[2*i+1] = features of slot i (this lane's level of the pair).  Matches oracle
// hashgrid_encode().  NB slots from LDS bricks, the next NGB from HBM bricks, the rest from the hashed tables.
// The 8 - NB global slots go through encode_batch in batches of at most four (encode_from): a batch keeps up to 19
// registers per slot live (8 offsets, 3 fractions, 8 gathered words) across its three phases, and with 5 .. 8 slots in ONE
// batch the 168-register budget of three waves per SIMD spilled 6 .. 90 registers inside the march loop (round 5: the
// generic no-brick kernel had always run like that).
template <int NB, int NGB, int ND, bool F16, int ARITH = 0>
__device__ __forceinline__ void encode_sample(const NerfParams &P, const __amdgpu_buffer_rsrc_t &rs,
                                              const __amdgpu_buffer_rsrc_t &rsb,
                                              const uint8_t *__restrict__ lds_bricks, bool hi, float x, float y,
                                              float z, uint4 &p0, uint4 &p1)
{
    float f[16];
    constexpr int NG = 8 - NB;          // slots fetched from HBM (bricks first, then tables)
    auto lds_slots = [&]() {
#pragma unroll
        for (int i = 0; i < NB; i++) {
            uint32_t br[8];
            float bw[3];
            uint32_t bo[8];
            slot_addr<K_BRICK>(P, i, hi, x, y, z, bo, bw);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t *p = (const uint32_t *)(lds_bricks + bo[2 * j]);
                br[2 * j] = p[0];
                br[2 * j + 1] = p[1];
            }
            slot_blend_as<ARITH>(br, bw, f[2 * i], f[2 * i + 1]);
        }
    };
#if D2R_MARCH_ABLATE & 3
#pragma unroll
    for (int i = 0; i < 16; i++) f[i] = x + (float)i * y;
    if (!(D2R_MARCH_ABLATE & 1)) lds_slots();
    if constexpr (NG != 0)
        if (!(D2R_MARCH_ABLATE & 2)) encode_from<NB, NGB, ND, NB, ARITH>(P, rs, rsb, hi, x, y, z, f, [] {});
#else
    if constexpr (NG == 0) lds_slots();
    else encode_from<NB, NGB, ND, NB, ARITH>(P, rs, rsb, hi, x, y, z, f, lds_slots);
#endif
    // straight into the two bf16 B fragments of density layer 1 (k-step 0: slots 0..3, 1: slots 4..7)
    p0.x = pack2<F16>(f[0], f[1]); p0.y = pack2<F16>(f[2], f[3]); p0.z = pack2<F16>(f[4], f[5]); p0.w = pack2<F16>(f[6], f[7]);
    p1.x = pack2<F16>(f[8], f[9]); p1.y = pack2<F16>(f[10], f[11]); p1.z = pack2<F16>(f[12], f[13]); p1.w = pack2<F16>(f[14], f[15]);
}

__device__ __forceinline__ void sh16(float x, float y, float z, float *o)
{
    float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    o[0] = 0.28209479177387814f;
    o[1] = -0.48860251190291987f * y;
    o[2] = 0.48860251190291987f * z;
    o[3] = -0.48860251190291987f * x;
    o[4] = 1.0925484305920792f * xy;
    o[5] = -1.0925484305920792f * yz;
    o[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
    o[7] = -1.0925484305920792f * xz;
    o[8] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
    o[9] = 0.59004358992664352f * y * (-3.0f * x2 + y2);
    o[10] = 2.8906114426405538f * xy * z;
    o[11] = 0.45704579946446572f * y * (1.0f - 5.0f * z2);
    o[12] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
    o[13] = 0.45704579946446572f * x * (1.0f - 5.0f * z2);
    o[14] = 1.4453057213202769f * z * (x2 - y2);
    o[15] = 0.59004358992664352f * x * (-x2 + 3.0f * y2);
}

// ReLU on the raw bits: max as signed integers against 0 maps every negative float (sign bit
// set) to +0 and keeps the others — one v_max_i32, and none of the canonicalising v_max_f32
// hipcc puts in front of fmaxf() on MFMA results.
__device__ __forceinline__ float relu_bits(float x)
{
    return __int_as_float(max(__float_as_int(x), 0));
}

// relu + pack registers [r0, r0+8) of an accumulator as the next layer's B fragment
template <bool F16>
__device__ __forceinline__ uint4 relu_pack(const f32x16 &a, int r0)
{
    // pack first, then ReLU on the packed pairs (v_pk_max_i16 against 0: a negative bf16 has its sign bit set, i.e. is a
    // negative int16; rounding to bf16 never changes the sign): 96 packed maxes per wave iteration instead of 192 v_max_i32.
    // The conversion stays with the compiler: it reads MFMA results, and hipcc pads the MFMA -> VALU hazard only for
    // instructions it emits itself; the packed max (inline asm) reads an ordinary VALU result.
    // (fp16 has its sign bit in the same place: the same integer maximum)
    auto pm = [](float lo, float hi) {
        uint32_t t = pack2<F16>(lo, hi), r;
        asm("v_pk_max_i16 %0, %1, 0" : "=v"(r) : "v"(t));
        return r;
    };
    uint4 o;
    o.x = pm(a[r0 + 0], a[r0 + 1]);
    o.y = pm(a[r0 + 2], a[r0 + 3]);
    o.z = pm(a[r0 + 4], a[r0 + 5]);
    o.w = pm(a[r0 + 6], a[r0 + 7]);
    return o;
}

// One tile (32 samples: sample n lives in lanes n and n+32, which hold half of its features each)
// through both MLPs.  Returns raw density-net output 0 and colour-net outputs 0..2 in lanes 0..31.
// Scheduling fences between the layers keep hipcc from hoisting later layers' LDS weight reads
// above the current MFMA chain (that inflated the live register set past 3 waves/SIMD).
template <bool F16>
__device__ __forceinline__ void mlp_tile(const uint4 *__restrict__ sw, uint32_t lane, const uint4 &a0,
                                         const uint4 &a1, const uint4 &sh, float *out)
{
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // density layer 1: 64 x 32
    f32x16 h0 = mfma<F16>(sw[0 * 64 + lane], a0, zero), h1 = mfma<F16>(sw[2 * 64 + lane], a0, zero);
    h0 = mfma<F16>(sw[1 * 64 + lane], a1, h0);
    h1 = mfma<F16>(sw[3 * 64 + lane], a1, h1);
    uint4 p0 = relu_pack<F16>(h0, 0), p1 = relu_pack<F16>(h0, 8), p2 = relu_pack<F16>(h1, 0), p3 = relu_pack<F16>(h1, 8);
    __builtin_amdgcn_sched_barrier(0);
    // density layer 2: 16 (padded 32) x 64
    f32x16 dd = mfma<F16>(sw[4 * 64 + lane], p0, zero);
    dd = mfma<F16>(sw[5 * 64 + lane], p1, dd);
    dd = mfma<F16>(sw[6 * 64 + lane], p2, dd);
    dd = mfma<F16>(sw[7 * 64 + lane], p3, dd);
    out[0] = dd[0];
    // colour layer 1: 64 x 32, input = [density out (no activation) | SH]
    uint4 cd;
    cd.x = pack2<F16>(dd[0], dd[1]); cd.y = pack2<F16>(dd[2], dd[3]); cd.z = pack2<F16>(dd[4], dd[5]); cd.w = pack2<F16>(dd[6], dd[7]);
    __builtin_amdgcn_sched_barrier(0);
    h0 = mfma<F16>(sw[8 * 64 + lane], cd, zero);
    h1 = mfma<F16>(sw[10 * 64 + lane], cd, zero);
    h0 = mfma<F16>(sw[9 * 64 + lane], sh, h0);
    h1 = mfma<F16>(sw[11 * 64 + lane], sh, h1);
    p0 = relu_pack<F16>(h0, 0); p1 = relu_pack<F16>(h0, 8); p2 = relu_pack<F16>(h1, 0); p3 = relu_pack<F16>(h1, 8);
    __builtin_amdgcn_sched_barrier(0);
    // colour layer 2: 64 x 64
    h0 = mfma<F16>(sw[12 * 64 + lane], p0, zero);
    h1 = mfma<F16>(sw[16 * 64 + lane], p0, zero);
    h0 = mfma<F16>(sw[13 * 64 + lane], p1, h0);
    h1 = mfma<F16>(sw[17 * 64 + lane], p1, h1);
    h0 = mfma<F16>(sw[14 * 64 + lane], p2, h0);
    h1 = mfma<F16>(sw[18 * 64 + lane], p2, h1);
    h0 = mfma<F16>(sw[15 * 64 + lane], p3, h0);
    h1 = mfma<F16>(sw[19 * 64 + lane], p3, h1);
    p0 = relu_pack<F16>(h0, 0); p1 = relu_pack<F16>(h0, 8); p2 = relu_pack<F16>(h1, 0); p3 = relu_pack<F16>(h1, 8);
    __builtin_amdgcn_sched_barrier(0);
    // colour layer 3: 16 (padded 32) x 64
    dd = mfma<F16>(sw[20 * 64 + lane], p0, zero);
    dd = mfma<F16>(sw[21 * 64 + lane], p1, dd);
    dd = mfma<F16>(sw[22 * 64 + lane], p2, dd);
    dd = mfma<F16>(sw[23 * 64 + lane], p3, dd);
    out[1] = dd[0];
    out[2] = dd[1];
    out[3] = dd[2];
    __builtin_amdgcn_sched_barrier(0);
}

// One tile through both MLPs with HALF accumulators (option "render_arith" 1 / 2; oracle/d2r_oracle.c matvec_f16_halfacc / nerf_eval):
// one v_mfma_f32_32x32x16_f16 has K = 16, so one MFMA from a ZERO accumulator is one 16-wide k-step's sum of exact products (the
// oracle's `part`); a VALU add and a convert round it into the running half accumulator, acc = rn16(acc + part).  The fragment order
// puts inputs 16 s .. 16 s + 15 into k-step s (build_frag), the oracle's own grouping.  Inputs are halves already (grid features, SH
// rounded by pack2, the previous layer's half results, so relu_pack's conversion is exact), the activation acts on the half result,
// network outputs are halves.  The MFMA's order of the 16 products inside a k-step is not the oracle's fmaf chain: `part` can differ
// in its last fp32 bit and flip a half rounding that sits on a tie — held to a tolerance, not bit-exact.
__device__ __forceinline__ void mlp_tile_half(const uint4 *__restrict__ sw, uint32_t lane, const uint4 &a0, const uint4 &a1, const uint4 &sh, float *out)
{
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // one 32-output half of a layer: NK weight fragments from sw[W0], inputs x[0 .. NK)
    auto half_layer = [&](int W0, int NK, const uint4 *x) {
        f32x16 acc = zero;
#pragma unroll
        for (int i = 0; i < NK; i++) {
            const f32x16 part = mfma<true>(sw[(W0 + i) * 64 + lane], x[i], zero);
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = rn16(acc[r] + part[r]);
        }
        return acc;
    };
    uint4 x[4], p[4];
    f32x16 g;
    // density layer 1: 64 x 32
    x[0] = a0; x[1] = a1;
    g = half_layer(0, 2, x);
    p[0] = relu_pack<true>(g, 0); p[1] = relu_pack<true>(g, 8);
    g = half_layer(2, 2, x);
    p[2] = relu_pack<true>(g, 0); p[3] = relu_pack<true>(g, 8);
    __builtin_amdgcn_sched_barrier(0);
    // density layer 2: 16 (padded 32) x 64
    g = half_layer(4, 4, p);
    out[0] = g[0];
    // colour layer 1: 64 x 32, input = [density out (no activation) | SH]
    x[0].x = pack2<true>(g[0], g[1]); x[0].y = pack2<true>(g[2], g[3]); x[0].z = pack2<true>(g[4], g[5]); x[0].w = pack2<true>(g[6], g[7]);
    x[1] = sh;
    __builtin_amdgcn_sched_barrier(0);
    g = half_layer(8, 2, x);
    p[0] = relu_pack<true>(g, 0); p[1] = relu_pack<true>(g, 8);
    g = half_layer(10, 2, x);
    p[2] = relu_pack<true>(g, 0); p[3] = relu_pack<true>(g, 8);
    __builtin_amdgcn_sched_barrier(0);
    // colour layer 2: 64 x 64
    g = half_layer(12, 4, p);
    x[0] = relu_pack<true>(g, 0); x[1] = relu_pack<true>(g, 8);
    g = half_layer(16, 4, p);
    x[2] = relu_pack<true>(g, 0); x[3] = relu_pack<true>(g, 8);
    __builtin_amdgcn_sched_barrier(0);
    // colour layer 3: 16 (padded 32) x 64
    g = half_layer(20, 4, x);
    out[1] = g[0];
    out[2] = g[1];
    out[3] = g[2];
    __builtin_amdgcn_sched_barrier(0);
}

// SH fragments of the wave's ray directions: the colour net's second B fragment for tile 0
// (directions of lanes 0..31) and tile 1 (lanes 32..63); this lane holds coefficients
// 8hi..8hi+7.  Directions are per RAY, so k_march recomputes these only when it refills.
template <bool F16>
__device__ __forceinline__ void sh_fragments(uint32_t lane, float dx, float dy, float dz, uint4 &shfA, uint4 &shfB)
{
    const bool hi = lane >= 32;
    float qdx = __shfl_xor(dx, 32), qdy = __shfl_xor(dy, 32), qdz = __shfl_xor(dz, 32);
    float sa[16];
    sh16(hi ? qdx : dx, hi ? qdy : dy, hi ? qdz : dz, sa);
    shfA.x = pack2<F16>(hi ? sa[8] : sa[0], hi ? sa[9] : sa[1]);
    shfA.y = pack2<F16>(hi ? sa[10] : sa[2], hi ? sa[11] : sa[3]);
    shfA.z = pack2<F16>(hi ? sa[12] : sa[4], hi ? sa[13] : sa[5]);
    shfA.w = pack2<F16>(hi ? sa[14] : sa[6], hi ? sa[15] : sa[7]);
    sh16(hi ? dx : qdx, hi ? dy : qdy, hi ? dz : qdz, sa);
    shfB.x = pack2<F16>(hi ? sa[8] : sa[0], hi ? sa[9] : sa[1]);
    shfB.y = pack2<F16>(hi ? sa[10] : sa[2], hi ? sa[11] : sa[3]);
    shfB.z = pack2<F16>(hi ? sa[12] : sa[4], hi ? sa[13] : sa[5]);
    shfB.w = pack2<F16>(hi ? sa[14] : sa[6], hi ? sa[15] : sa[7]);
}

// Evaluate the wave's 64 samples (one per lane; `valid` marks lanes that have one).
// On return every valid lane holds sigma and the network rgb of ITS OWN sample.
// ARITH (option "render_arith"): 0 the specification, fp32 accumulation; 1 / 2 tiny-cuda-nn's half arithmetic as
// oracle/d2r_oracle.c emulates it (slot_blend_half, mlp_tile_half), fp16 operands only.
template <int NB, int NGB, int ND, bool F16, int ARITH = 0>
__device__ __forceinline__ void eval_wave(const NerfParams &P, const __amdgpu_buffer_rsrc_t &rs,
                                          const __amdgpu_buffer_rsrc_t &rsb, const uint4 *__restrict__ sw,
                                          const uint8_t *__restrict__ lds_bricks, uint32_t lane, bool valid, float x,
                                          float y, float z, const uint4 &shfA, const uint4 &shfB, float &sigma,
                                          float &r, float &g, float &b)
{
    const bool hi = lane >= 32;
    // partner lane (l ^ 32) owns the other sample of this lane's column
    float qx = __shfl_xor(x, 32), qy = __shfl_xor(y, 32), qz = __shfl_xor(z, 32);
    bool qvalid = __shfl_xor((int)valid, 32) != 0;
    // tile 0 = samples of lanes 0..31, tile 1 = samples of lanes 32..63
    float ax = hi ? qx : x, ay = hi ? qy : y, az = hi ? qz : z;      // tile-0 sample seen by this lane
    float bx = hi ? x : qx, by = hi ? y : qy, bz = hi ? z : qz;      // tile-1 sample
    bool av = hi ? qvalid : valid, bv = hi ? valid : qvalid;
    // this lane's levels: 2i + hi for every slot i (slots 0..3 -> k-step 0, 4..7 -> k-step 1);
    // the features go straight into bf16 fragments (8 registers per sample instead of 16 floats)
    uint4 fa0 = make_uint4(0, 0, 0, 0), fa1 = fa0, fb0 = fa0, fb1 = fa0;
    if (av) encode_sample<NB, NGB, ND, F16, ARITH>(P, rs, rsb, lds_bricks, hi, ax, ay, az, fa0, fa1);
    if (bv) encode_sample<NB, NGB, ND, F16, ARITH>(P, rs, rsb, lds_bricks, hi, bx, by, bz, fb0, fb1);
    float oa[4] = {0.f, 0.f, 0.f, 0.f}, ob[4] = {0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_sched_barrier(0);
    // a tile none of whose 32 samples exists (the tail of a wave's rays, compacted into tile 0 by k_march) costs nothing:
    // its features were skipped above (exec-masked), its MLP passes are skipped here (wave-uniform)
    const unsigned long long vm = __ballot(valid);
#if D2R_MARCH_ABLATE & 4
    oa[0] = __uint_as_float(fa0.x) * 1e-3f; oa[1] = __uint_as_float(fa0.y); oa[2] = __uint_as_float(fa1.x); oa[3] = __uint_as_float(fa1.y);
    ob[0] = __uint_as_float(fb0.x) * 1e-3f; ob[1] = __uint_as_float(fb0.y); ob[2] = __uint_as_float(fb1.x); ob[3] = __uint_as_float(fb1.y);
#else
    if constexpr (ARITH != 0) {
        static_assert(F16, "the half arithmetic has no bf16 form");
        if ((uint32_t)vm != 0u) mlp_tile_half(sw, lane, fa0, fa1, shfA, oa);
        if ((uint32_t)(vm >> 32) != 0u) mlp_tile_half(sw, lane, fb0, fb1, shfB, ob);
    } else {
    if ((uint32_t)vm != 0u) mlp_tile<F16>(sw, lane, fa0, fa1, shfA, oa);
    if ((uint32_t)(vm >> 32) != 0u) mlp_tile<F16>(sw, lane, fb0, fb1, shfB, ob);
    }
#endif
    // tile-1 results live in lanes 0..31; their owners are lanes 32..63
    float ts = __shfl_xor(ob[0], 32), tr = __shfl_xor(ob[1], 32), tg = __shfl_xor(ob[2], 32), tb = __shfl_xor(ob[3], 32);
    // sigma = exp(x), rgb = sigmoid(x) through the hardware exp2 / rcp (1-2 ulp)
    const float L2E = 1.4426950408889634f;
    sigma = __builtin_amdgcn_exp2f(L2E * (hi ? ts : oa[0]));
    r = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-L2E * (hi ? tr : oa[1])));
    g = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-L2E * (hi ? tg : oa[2])));
    b = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-L2E * (hi ? tb : oa[3])));
}

// field evaluation at arbitrary points (parity hook used by tests through d2r_eval_points)
template <int ND, bool F16, int ARITH = 0>
__global__ __launch_bounds__(256) void k_eval_points(NerfParams P, const float *__restrict__ xyz,
                                                     const float *__restrict__ dirs, uint32_t n,
                                                     float *__restrict__ out)
{
    __shared__ uint4 sw[D2R_N_WFRAG * 64];
    for (uint32_t i = threadIdx.x; i < D2R_N_WFRAG * 64; i += blockDim.x) sw[i] = (F16 ? P.wfrag16 : P.wfrag)[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)P.grid, 0, P.grid_bytes, 0x00020000);
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = i < n;
    float x = 0, y = 0, z = 0, dx = 0, dy = 0, dz = 1;
    if (valid) {
        x = xyz[3 * i]; y = xyz[3 * i + 1]; z = xyz[3 * i + 2];
        dx = dirs[3 * i]; dy = dirs[3 * i + 1]; dz = dirs[3 * i + 2];
    }
    float s, r, g, b;
    uint4 shfA, shfB;
    sh_fragments<F16>(lane, dx, dy, dz, shfA, shfB);
    eval_wave<0, 0, ND, F16, ARITH>(P, rs, rs, sw, nullptr, lane, valid, x, y, z, shfA, shfB, s, r, g, b);   // arbitrary points: no bricks
    if (valid) *(float4 *)(out + 4 * (size_t)i) = make_float4(s, r, g, b);
}

// ------------------------------------------------------------------ marcher

// 768 threads = 12 waves = 3 per SIMD (168 VGPRs): the sweet spot measured on MI355X; 512 leaves
// latency exposed, 1024 spills heavily.
#ifndef D2R_MARCH_THREADS
#define D2R_MARCH_THREADS 768
#endif
template <bool COMPOSITE, int NB, int NGB, int ND, bool CONE = false, bool F16 = false, int ARITH = 0>
__global__ __launch_bounds__(D2R_MARCH_THREADS) void k_march(NerfParams P, ViewParams V, const float *__restrict__ cams,
                                                  const uint2 *__restrict__ queue,
                                                  const uint32_t *__restrict__ qcount,
                                                  uint32_t *__restrict__ qhead, float *__restrict__ rgba_out,
                                                  float *__restrict__ depth_out,
                                                  const float *__restrict__ bg_depth,
                                                  uint8_t *__restrict__ frames,
                                                  unsigned long long *__restrict__ sample_counter)
{
    // one 8-wave workgroup per CU: [0, 24 KiB) MLP fragments, then the de-hashed level bricks
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint4 *sw = (uint4 *)smem;
    uint8_t *lds_bricks = smem + D2R_N_WFRAG * 64 * 16;
    for (uint32_t i = threadIdx.x; i < D2R_N_WFRAG * 64; i += blockDim.x) sw[i] = (F16 ? P.wfrag16 : P.wfrag)[i];
    if (NB > 0)
        for (uint32_t i = threadIdx.x; i < P.brick_words; i += blockDim.x) ((uint32_t *)lds_bricks)[i] = P.brick_tab[i];
    if (CONE) cone_tab_to_lds();
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n_q = *qcount;
    const uint32_t WH = V.W * V.H;
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)P.grid, 0, P.grid_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc((void *)P.gbrick_tab, 0, P.gbrick_bytes, 0x00020000);

    bool alive = false, exhausted = false;
    uint32_t res_lo = 0, res_hi = 0;           // wave-uniform: this wave's reserved range of queue entries
    Ray ray = {};
    uint32_t k = 0, ray_id = 0;
    float px = 0.f, py = 0.f, pz = 0.f;
    float C0 = 0.f, C1 = 0.f, C2 = 0.f, A = 0.f, Z = 0.f;
    // depth of a sample along the camera axis: z = fwd.(p - c) = t * (d.fwd) + (o - c).fwd
    float zslope = 0.f, zbase = 0.f;
    uint32_t nsamp = 0, niter = 0;
    uint4 shfA = make_uint4(0, 0, 0, 0), shfB = shfA;

#if D2R_MARCH_PROF
    long long prof_t0 = clock64(), prof_refill = 0;
    uint32_t prof_n = 0, prof_le32 = 0, prof_le16 = 0, prof_half = 0, prof_alive = 0;
#endif
    for (;;) {
        // ---- compaction (P.compact): once no more than 32 rays are left and some of them sit in lanes 32..63, the wave's rays move
        // to lanes 0 .. n-1 (ds_permute: a forward permutation, no LDS memory): tile 1 then holds no sample, its gathers and MLP
        // passes are skipped (eval_wave), and the free lanes are one contiguous block for the next refill.  Per-ray arithmetic
        // does not depend on the lane a ray sits in: the frames are bit-identical.
        bool sh_dirty = false;                 // wave-uniform
        if (P.compact) {
            const unsigned long long am = __ballot(alive);
            const uint32_t na = (uint32_t)__popcll(am);
            if (na != 0u && na <= 32u && (am >> 32) != 0ull) {
                const unsigned long long below = (1ull << lane) - 1ull;
                const uint32_t dest = alive ? (uint32_t)__popcll(am & below) : na + (uint32_t)__popcll(~am & below);
                const int d4 = (int)(dest << 2);
                auto mv = [&](float &v) { v = __int_as_float(__builtin_amdgcn_ds_permute(d4, __float_as_int(v))); };
                auto mvu = [&](uint32_t &v) { v = (uint32_t)__builtin_amdgcn_ds_permute(d4, (int)v); };
                mv(ray.ox); mv(ray.oy); mv(ray.oz); mv(ray.dx); mv(ray.dy); mv(ray.dz); mv(ray.t0); mvu(ray.k_hi);
                if (CONE) { mvu(ray.k1); mv(ray.t1); }
                mvu(k); mvu(ray_id); mv(px); mv(py); mv(pz);
                mv(C0); mv(C1); mv(C2); mv(A); mv(Z); mv(zslope); mv(zbase);
                alive = lane < na;
                sh_dirty = true;
            }
        }
        // ---- refill free lanes from the ray queue (ballot + prefix popcount, one atomic per wave)
        unsigned long long freem = __ballot(!alive);
        if ((!exhausted || res_lo < res_hi) && freem != 0ull && (__popcll(freem) >= (int)P.refill_min || freem == ~0ull)) {
#if D2R_MARCH_PROF
            const long long prof_a = clock64();
#endif
            const uint32_t nfree = (uint32_t)__popcll(freem);
            if (res_lo == res_hi) {
                // this wave's reservation is used up: take the next D2R_MARCH_RESERVE queue entries with
                // one atomic (the queue head is a single address; one atomic per refill was ~10^6 per pass)
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(qhead, (uint32_t)D2R_MARCH_RESERVE);
                base = __builtin_amdgcn_readfirstlane(base);
                res_lo = min(base, n_q);
                res_hi = min(base + (uint32_t)D2R_MARCH_RESERVE, n_q);
                if (base + D2R_MARCH_RESERVE >= n_q) exhausted = true;
            }
            const uint32_t take = min(nfree, res_hi - res_lo);
            const uint32_t first = res_lo;
            res_lo += take;
            if (!alive) {
                const uint32_t rank = (uint32_t)__popcll(freem & ((1ull << lane) - 1ull));
                const uint32_t idx = first + rank;
                if (rank < take) {
                    uint2 q = queue[idx];
                    ray_id = q.x;
                    k = q.y;
                    uint32_t cam_i = ray_id / WH, pix = ray_id - cam_i * WH;
                    float cam[12];
#pragma unroll
                    for (int j = 0; j < 12; j++) cam[j] = cams[(size_t)cam_i * 12 + j];
                    uint32_t klo;
                    make_ray<CONE>(P, V, cam, pix % V.W, pix / V.W, ray, klo);
                    float t = lattice_t<CONE>(ray, k);
                    px = fmaf(t, ray.dx, ray.ox);
                    py = fmaf(t, ray.dy, ray.oy);
                    pz = fmaf(t, ray.dz, ray.oz);
                    // world-space ray for the depth (CONE: the stored ray lives in the unit cube of the box)
                    const float wdx = CONE ? ray.dx * P.side : ray.dx, wdy = CONE ? ray.dy * P.side : ray.dy, wdz = CONE ? ray.dz * P.side : ray.dz;
                    const float wox = CONE ? fmaf(ray.ox - 0.5f, P.side, 0.5f) : ray.ox, woy = CONE ? fmaf(ray.oy - 0.5f, P.side, 0.5f) : ray.oy;
                    const float woz = CONE ? fmaf(ray.oz - 0.5f, P.side, 0.5f) : ray.oz;
                    zslope = (wdx * cam[2] + wdy * cam[6] + wdz * cam[10]) * V.inv_scale;
                    zbase = ((wox - cam[3]) * cam[2] + (woy - cam[7]) * cam[6] + (woz - cam[11]) * cam[10]) * V.inv_scale;
                    C0 = C1 = C2 = A = Z = 0.f;
                    alive = true;
                }
            }
            sh_dirty = true;
#if D2R_MARCH_PROF
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            prof_refill += clock64() - prof_a;
            prof_n++;
#endif
        }
        if (!__any(alive)) break;
        if (sh_dirty) {
            // ray directions changed in some lanes (refill) or moved between lanes (compaction): refresh the wave's SH
            // fragments (all lanes take part: a lane's fragment also carries its partner's direction)
            if (CONE) sh_fragments<F16>(lane, ray.dx * P.side, ray.dy * P.side, ray.dz * P.side, shfA, shfB);     // unit direction
            else sh_fragments<F16>(lane, ray.dx, ray.dy, ray.dz, shfA, shfB);
        }
        niter++;
#if D2R_MARCH_PROF
        {
            const unsigned long long am = __ballot(alive);
            const int na = __popcll(am);
            prof_le32 += na <= 32;
            prof_le16 += na <= 16;
            prof_half += (am >> 32) == 0ull || (am & 0xffffffffull) == 0ull;
            prof_alive += na;
        }
#endif

        // ---- evaluate this wave's samples
        float sigma, cr, cg, cb;
        eval_wave<NB, NGB, ND, F16, ARITH>(P, rs, rsb, sw, lds_bricks, lane, alive, px, py, pz, shfA, shfB, sigma, cr, cg, cb);

        // ---- composite + advance
        if (alive) {
            nsamp++;
            float T = 1.0f - A;
            const float tk = lattice_t<CONE>(ray, k);
            float alpha = 1.0f - expf(-sigma * lattice_dt<CONE>(tk));
            float wgt = alpha * T;
            float zz = fmaf(tk, zslope, zbase);
            C0 = fmaf(wgt, cr, C0);
            C1 = fmaf(wgt, cg, C1);
            C2 = fmaf(wgt, cb, C2);
            Z = fmaf(wgt, zz, Z);
            A += wgt;
            bool done = false;
            if (A > 1.0f - V.min_transmittance) {
                float ia = 1.0f / A;
                C0 *= ia; C1 *= ia; C2 *= ia; Z *= ia;
                A = 1.0f;
                done = true;
            } else {
                k++;
                done = !next_sample<CONE>(P, ray, k, px, py, pz);
            }
            if (done) {
                alive = false;
                // shade (sRGB-space accumulation -> linear, premultiplied) + background blend
                float o0 = fmaf((1.0f - A) * V.background[3], V.background[0], srgb_to_linear(C0));
                float o1 = fmaf((1.0f - A) * V.background[3], V.background[1], srgb_to_linear(C1));
                float o2 = fmaf((1.0f - A) * V.background[3], V.background[2], srgb_to_linear(C2));
                float oa = fmaf(1.0f - A, V.background[3], A);
                if (!COMPOSITE) {
                    *(float4 *)(rgba_out + (size_t)ray_id * 4) = make_float4(o0, o1, o2, oa);
                    depth_out[ray_id] = Z;
                } else {
                    // reference combined_rendering.py:134-153 for a pixel the fg ray reached
                    uint32_t pix = ray_id % WH;
                    float fd = Z < 0.05f ? 100.f : Z;
                    float bd = bg_depth[pix];
                    bd = bd < 0.05f ? 100.f : bd;
                    if (fd < bd) {
                        uint32_t qa = quant_u8(oa);
                        uint32_t q0 = 0, q1 = 0, q2 = 0;
                        if (qa >= 130) {
                            q0 = quant_u8(linear_to_srgb(oa != 0.f ? o0 / oa : 0.f));
                            q1 = quant_u8(linear_to_srgb(oa != 0.f ? o1 / oa : 0.f));
                            q2 = quant_u8(linear_to_srgb(oa != 0.f ? o2 / oa : 0.f));
                        }
                        uint8_t *dst = frames + (size_t)ray_id * 3;
                        dst[0] = (uint8_t)q0;
                        dst[1] = (uint8_t)q1;
                        dst[2] = (uint8_t)q2;
                    }
                }
            }
        }
    }
#if D2R_MARCH_PROF
    if (lane == 0 && (threadIdx.x >> 6) < 2 && blockIdx.x % 64 == 0)
        printf("prof block %u wave %u: cycles %lld refill %lld (%u refills) iterations %u alive<=32 %u alive<=16 %u half-dead %u lane-samples %u\n", blockIdx.x, threadIdx.x >> 6, clock64() - prof_t0, prof_refill, prof_n, niter, prof_le32, prof_le16, prof_half, prof_alive);
#endif
    // per-wave sample count -> global counter
    unsigned long long tot = nsamp;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    if (lane == 0 && tot) {
        atomicAdd(sample_counter, tot);
        atomicAdd(sample_counter + 1, (unsigned long long)niter);     // wave-iterations (64 sample slots each)
    }
}

// frames[c][pix] = bg_u8[pix] for every candidate (16-byte stores)
__global__ void k_frames_init(const uint4 *__restrict__ bg_u8, uint4 *__restrict__ frames, uint32_t n_vec,
                              uint32_t n_cams)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_vec) return;
    uint4 v = bg_u8[i];
    for (uint32_t c = blockIdx.y; c < n_cams; c += gridDim.y) frames[(size_t)c * n_vec + i] = v;
}

// same, for frame sizes whose byte count is not a multiple of 16 (unaligned frame starts)
__global__ void k_frames_init_bytes(const uint8_t *__restrict__ bg_u8, uint8_t *__restrict__ frames, uint32_t n_bytes,
                                    uint32_t n_cams)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_bytes) return;
    uint8_t v = bg_u8[i];
    for (uint32_t c = blockIdx.y; c < n_cams; c += gridDim.y) frames[(size_t)c * n_bytes + i] = v;
}

// background pixel as it appears in the composited frame when the fg does not win the depth
// test (reference combined_rendering.py:147-153 applied to bg_image)
__global__ void k_bg_quantize(const float *__restrict__ bg_rgba, uint8_t *__restrict__ out, uint32_t n)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 p = *(const float4 *)(bg_rgba + (size_t)i * 4);
    uint32_t qa = quant_u8(p.w), q0 = 0, q1 = 0, q2 = 0;
    if (qa >= 130) {
        q0 = quant_u8(linear_to_srgb(p.w != 0.f ? p.x / p.w : 0.f));
        q1 = quant_u8(linear_to_srgb(p.w != 0.f ? p.y / p.w : 0.f));
        q2 = quant_u8(linear_to_srgb(p.w != 0.f ? p.z / p.w : 0.f));
    }
    out[3 * (size_t)i + 0] = (uint8_t)q0;
    out[3 * (size_t)i + 1] = (uint8_t)q1;
    out[3 * (size_t)i + 2] = (uint8_t)q2;
}

// ---------------------------------------------------------------- launchers

ViewParams d2r_view_params(const d2r_view *v)
{
    ViewParams V;
    V.W = v->width;
    V.H = v->height;
    V.focal[0] = v->focal[0];
    V.focal[1] = v->focal[1];
    V.center[0] = v->center[0];
    V.center[1] = v->center[1];
    V.scale = v->scale;
    V.inv_scale = 1.0f / v->scale;
    for (int i = 0; i < 3; i++) V.offset[i] = v->offset[i];
    for (int i = 0; i < 4; i++) V.background[i] = v->background[i];
    V.min_transmittance = v->min_transmittance;
    V.near_distance = v->near_distance;
    V.lens_mode = v->lens_mode;
    for (int i = 0; i < 4; i++) V.lens[i] = v->lens_mode ? v->lens_params[i] : 0.f;
    V.lens_tab = nullptr;           // d2r_lens_table attaches the view's table
    return V;
}

int d2r_launch_cameras_direct(d2r_ctx *ctx, const ViewParams &V, const float *cams_nerf_dev, uint32_t n,
                              float *cams_out)
{
    hipLaunchKernelGGL(k_cameras_direct, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, V, cams_nerf_dev, n,
                       cams_out);
    D2R_HIP(ctx, hipGetLastError());
    return D2R_OK;
}

int d2r_launch_cameras_virtual(d2r_ctx *ctx, const ViewParams &V, const float *obj_now16, const float *cam16,
                               const float *obj_poses_dev, uint32_t n, float *cams_out)
{
    Mat16 a, b;
    for (int i = 0; i < 16; i++) {
        a.v[i] = obj_now16[i];
        b.v[i] = cam16[i];
    }
    hipLaunchKernelGGL(k_cameras_virtual, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, V, a, b,
                       obj_poses_dev, n, cams_out);
    D2R_HIP(ctx, hipGetLastError());
    return D2R_OK;
}

// counters layout: [0] queue count, [1] queue head, [2..3] 64-bit sample counter
// the [H][W] table of undistorted camera-space directions of a view with a lens: rebuilt only when the view's size, intrinsics
// or coefficients change (once per task in the path), then synchronised so that any stream of the context may read it.  Every
// caller of d2r_launch_render attaches it BEFORE its chunk loop (and before render_score_body forks its streams): a rebuild
// reserves memory and synchronises
int d2r_lens_table(d2r_ctx *ctx, ViewParams &V)
{
    V.lens_tab = nullptr;
    if (V.lens_mode != D2R_LENS_OPENCV) return D2R_OK;
    const float key[10] = {(float)V.W, (float)V.H, V.focal[0], V.focal[1], V.center[0], V.center[1], V.lens[0], V.lens[1], V.lens[2], V.lens[3]};
    const size_t px = (size_t)V.W * V.H;
    if (!ctx->lens_tab.p || !ctx->lens_key_valid || memcmp(key, ctx->lens_key, sizeof key) != 0) {
        ctx->lens_key_valid = false;
        int rc = d2r_reserve(ctx, ctx->lens_tab, px * sizeof(float2));
        if (rc) return rc;
        hipLaunchKernelGGL(k_lens_table, dim3((uint32_t)((px + 255) / 256)), dim3(256), 0, ctx->stream, V, (float2 *)ctx->lens_tab.p);
        D2R_HIP(ctx, hipGetLastError());
        D2R_HIP(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(ctx->lens_key, key, sizeof key);
        ctx->lens_key_valid = true;
    }
    V.lens_tab = (const float2 *)ctx->lens_tab.p;
    return D2R_OK;
}

// Every workspace a render pass over `rays` rays (worst case: every pixel of every candidate a ray) takes: the ray queue, and with
// the ray sort its second copy and the per-chunk bin counts.  render_score_core calls this ONCE before its chunk loop (ADVICE r05:
// a lazy reservation inside the loop ran under the stream swap of the overlapped pipeline), the single-pass entry points per launch.
int d2r_reserve_render(d2r_ctx *ctx, size_t rays)
{
    int rc;
    if ((rc = d2r_reserve(ctx, ctx->queue, rays * sizeof(uint2)))) return rc;
    if (ctx->ray_sort) {
        const size_t max_chunks = (rays + D2R_SORT_CHUNK - 1) / D2R_SORT_CHUNK;
        if ((rc = d2r_reserve(ctx, ctx->queue2, rays * sizeof(uint2)))) return rc;
        if ((rc = d2r_reserve(ctx, ctx->sort_counts, (max_chunks + 2) * D2R_SORT_BINS * 4))) return rc;
    }
    return D2R_OK;
}

int d2r_launch_render(d2r_ctx *ctx, const d2r_nerf *m, const ViewParams &V, const float *cams_dev, uint32_t n,
                      bool composite, float *rgba_dev, float *depth_dev, uint8_t *frames_dev, void *rects_dev)
{
    const size_t rays = (size_t)n * V.W * V.H;
    if (rays >= (1ull << 32)) return d2r_fail(ctx, D2R_ERR_INVALID, "too many rays in one pass");
    if (V.lens_mode == D2R_LENS_OPENCV && !V.lens_tab)
        return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_launch_render: a view with a lens arrived without its table (d2r_lens_table)");
    int rc;
    if ((rc = d2r_reserve_render(ctx, rays))) return rc;      // no-op when the caller sized the pass up front (render_score_core)
    if ((rc = d2r_reserve(ctx, ctx->counters, 64))) return rc;
    uint32_t *cnt = (uint32_t *)ctx->counters.p;
    D2R_HIP(ctx, hipMemsetAsync(cnt, 0, 32, ctx->stream));
    if (composite) {
        if (ctx->bg_w != V.W || ctx->bg_h != V.H || !ctx->bg_u8.p)
            return d2r_fail(ctx, D2R_ERR_INVALID, "d2r_set_background must be called for this view first");
        const uint32_t n_bytes = V.W * V.H * 3;
        if (n_bytes % 16 == 0) {
            const uint32_t n_vec = n_bytes / 16;
            hipLaunchKernelGGL(k_frames_init, dim3((n_vec + 255) / 256, n < 64 ? n : 64), dim3(256), 0, ctx->stream,
                               (const uint4 *)ctx->bg_u8.p, (uint4 *)frames_dev, n_vec, n);
        } else {
            hipLaunchKernelGGL(k_frames_init_bytes, dim3((n_bytes + 255) / 256, n < 64 ? n : 64), dim3(256), 0,
                               ctx->stream, (const uint8_t *)ctx->bg_u8.p, frames_dev, n_bytes, n);
        }
    }
    const uint32_t tiles = ((V.W + 15) / 16) * ((V.H + 15) / 16);
    // ray sort (see k_sort_count): rays marched in the order of the object region they enter
    const uint32_t sort_log2 = ctx->ray_sort ? (uint32_t)ctx->ray_sort_log2 : 0u;
    NerfParams PR = m->P;
    PR.sort_log2 = sort_log2;
    size_t tr = ctx->timing_begin(D2R_T_RAYGEN);
    const bool cone = m->P.aabb_scale >= 2;          // occupancy cascades + cone stepping
    if (composite && ctx->raygen_rect) {
        if (cone) hipLaunchKernelGGL(k_raygen_rect<true>, dim3(n, 4), dim3(256), 0, ctx->stream, PR, V, cams_dev, (uint2 *)ctx->queue.p, cnt, (int4 *)rects_dev);
        else hipLaunchKernelGGL(k_raygen_rect<false>, dim3(n, 4), dim3(256), 0, ctx->stream, PR, V, cams_dev, (uint2 *)ctx->queue.p, cnt, (int4 *)rects_dev);
    } else {
        if (cone)
            hipLaunchKernelGGL(k_raygen<true>, dim3(tiles, n), dim3(256), 0, ctx->stream, PR, V, cams_dev, (uint2 *)ctx->queue.p,
                               cnt, composite ? nullptr : rgba_dev, composite ? nullptr : depth_dev);
        else
            hipLaunchKernelGGL(k_raygen<false>, dim3(tiles, n), dim3(256), 0, ctx->stream, PR, V, cams_dev, (uint2 *)ctx->queue.p,
                               cnt, composite ? nullptr : rgba_dev, composite ? nullptr : depth_dev);
    }
    ctx->timing_end(tr);
    const uint2 *q = (const uint2 *)ctx->queue.p;
    if (sort_log2) {
        size_t ts = ctx->timing_begin(D2R_T_SORT);
        // counts: [bins][chunks] + [bins] bin totals + [bins] bin bases, sized for the worst case (every pixel of every candidate a ray)
        const size_t max_chunks = (rays + D2R_SORT_CHUNK - 1) / D2R_SORT_CHUNK;        // (reserved by d2r_reserve_render above)
        uint32_t *counts = (uint32_t *)ctx->sort_counts.p, *bin_total = counts + max_chunks * D2R_SORT_BINS, *bin_base = bin_total + D2R_SORT_BINS;
        const int sb = (int)std::min<size_t>(max_chunks, 4096);
        hipLaunchKernelGGL(k_sort_count, dim3(sb), dim3(256), 0, ctx->stream, q, cnt, counts);
        hipLaunchKernelGGL(k_sort_scan_rows, dim3(D2R_SORT_BINS), dim3(256), 0, ctx->stream, cnt, counts, bin_total);
        hipLaunchKernelGGL(k_sort_scan_bins, dim3(1), dim3(256), 0, ctx->stream, bin_total, bin_base);
        hipLaunchKernelGGL(k_sort_scatter, dim3(sb), dim3(256), 0, ctx->stream, q, cnt, counts, bin_base, (uint2 *)ctx->queue2.p);
        q = (const uint2 *)ctx->queue2.p;
        ctx->timing_end(ts);
    }
    size_t tm = ctx->timing_begin(D2R_T_MARCH);
    int blocks = ctx->march_blocks > 0 ? (int)ctx->march_blocks : ctx->n_cu;     // persistent: one per CU
    const float *bgd = (const float *)ctx->bg_depth.p;
    unsigned long long *sc = (unsigned long long *)(cnt + 2);
    // Brick configuration (NB leading slots from LDS, the next NGB from HBM bricks, the rest from the tables) -> one of the
    // instantiated kernels.  The HBM bricks were built for the model's own LDS count, so NB is that count or 0; NGB is
    // rounded DOWN to an instantiated value (using fewer HBM-brick slots than exist is always valid).
    const bool bricks_ok = ctx->use_bricks && m->P.n_dense == 5;
    uint32_t nb = bricks_ok ? m->P.n_brick_slots : 0;
    uint32_t ngb = 0;
    if (bricks_ok) {
        const uint32_t cap_total = (uint32_t)std::max<int64_t>(ctx->brick_slots_total, nb);
        ngb = std::min<uint32_t>(std::min<uint32_t>((uint32_t)ctx->gbrick_slots, m->P.n_gbrick_slots), cap_total - nb);
        // instantiated (NB, NGB): NB = 5: 0..3;  4: 0, 2, 3;  3: 3, 4;  2: 4, 5;  1: 5, 6;  0: 0, 6, 7  (HBM bricks through slot 5 or 6)
        bool none = false;
        switch (nb) {
            case 5: ngb = std::min(ngb, 3u); break;
            case 4: ngb = ngb >= 3 ? 3 : ngb >= 2 ? 2 : 0; break;
            case 3: case 2: case 1:
                if (ngb >= 7 - nb) ngb = 7 - nb;
                else if (ngb >= 6 - nb) ngb = 6 - nb;
                else none = true;             // LDS bricks alone are not instantiated for 1..3 slots (slots <= 5 always fit the HBM budget)
                break;
            default: ngb = ngb >= 7 ? 7 : ngb >= 6 ? 6 : 0; break;
        }
        if (none) nb = ngb = 0;
    }
    // "render_arith" 1 / 2: the brick-free generic table kernel (a validation mode: two instantiations per mode, not thirty-four)
    const int arith = (int)ctx->render_arith;
    if (arith) nb = ngb = 0;
    NerfParams PP = m->P;
    PP.refill_min = (uint32_t)ctx->refill_min;
    PP.compact = (uint32_t)ctx->march_compact;
    const size_t lds = (size_t)D2R_N_WFRAG * 64 * 16 + (nb ? (size_t)m->P.brick_words * 4 : 0);
    // waves per workgroup (= per CU): the kernels are compiled for D2R_MARCH_THREADS (three waves per SIMD); a launch may use fewer.
    // Auto: all of them — except WITHOUT the ray sort where the bricks behind the LDS slots are larger than the L2s can hold: there the
    // unsorted marcher is bound by the L2-miss path and two waves per SIMD thrash less (1-5 % faster; round 5, same-box A/B)
    uint32_t threads = D2R_MARCH_THREADS;
    if (ctx->march_threads > 0) threads = std::min<uint32_t>((uint32_t)ctx->march_threads, D2R_MARCH_THREADS);
    else if (!sort_log2 && ngb && m->P.gbrick_bytes > (size_t)ctx->march_threads_auto_mib << 20) threads = std::min<uint32_t>(512u, D2R_MARCH_THREADS);
#define D2R_MARCH_C(COMP, NB, NGB, ND, CONE)                            \
    do {                                                                \
        if (ctx->mlp_f16) D2R_MARCH_F(COMP, NB, NGB, ND, CONE, true, 0);   \
        else D2R_MARCH_F(COMP, NB, NGB, ND, CONE, false, 0);               \
    } while (0)
#define D2R_MARCH_F(COMP, NB, NGB, ND, CONE, F16, ARITH)                                                              \
    do {                                                                                                          \
        static PerDeviceOnce attr;                                                                                \
        attr.run(ctx->device, [] {                                                                                \
            (void)hipFuncSetAttribute((const void *)k_march<COMP, NB, NGB, ND, CONE, F16, ARITH>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (CONE ? 512 : 0)); /* the CONE kernels hold 512 B of static LDS (cone tables): static + dynamic <= 160 KiB */ \
        });                                                                                                       \
        hipLaunchKernelGGL((k_march<COMP, NB, NGB, ND, CONE, F16, ARITH>), dim3(blocks), dim3(threads), lds, ctx->stream, PP, V, cams_dev, q, \
                           cnt, cnt + 1, COMP ? nullptr : rgba_dev, COMP ? nullptr : depth_dev,                   \
                           COMP ? bgd : nullptr, COMP ? frames_dev : nullptr, sc);                                \
    } while (0)
    // compile-time slot kinds: the usual tables have 5 leading dense levels; anything else takes the generic instantiation
#define D2R_MARCH_CASE(COMP, CONE, NB, NGB) else if (nb == NB && ngb == NGB) D2R_MARCH_C(COMP, NB, NGB, 5, CONE);
#define D2R_MARCH_PICK(COMP, CONE)                                      \
    do {                                                                \
        if (m->P.n_dense != 5) D2R_MARCH_C(COMP, 0, 0, -1, CONE);       \
        D2R_MARCH_CASE(COMP, CONE, 5, 3) D2R_MARCH_CASE(COMP, CONE, 5, 2) D2R_MARCH_CASE(COMP, CONE, 5, 1) D2R_MARCH_CASE(COMP, CONE, 5, 0) \
        D2R_MARCH_CASE(COMP, CONE, 4, 3) D2R_MARCH_CASE(COMP, CONE, 4, 2) D2R_MARCH_CASE(COMP, CONE, 4, 0)                                  \
        D2R_MARCH_CASE(COMP, CONE, 3, 4) D2R_MARCH_CASE(COMP, CONE, 3, 3)                                                                   \
        D2R_MARCH_CASE(COMP, CONE, 2, 5) D2R_MARCH_CASE(COMP, CONE, 2, 4)                                                                   \
        D2R_MARCH_CASE(COMP, CONE, 1, 6) D2R_MARCH_CASE(COMP, CONE, 1, 5)                                                                   \
        D2R_MARCH_CASE(COMP, CONE, 0, 7) D2R_MARCH_CASE(COMP, CONE, 0, 6)                                                                   \
        else D2R_MARCH_C(COMP, 0, 0, 5, CONE);                          \
    } while (0)
    // "render_arith" 1 / 2 have one kernel per (COMP, CONE): the generic table kernel with fp16 operands
#define D2R_MARCH_HALF(COMP, CONE)                                      \
    do {                                                                \
        if (arith == 1) D2R_MARCH_F(COMP, 0, 0, -1, CONE, true, 1);     \
        else D2R_MARCH_F(COMP, 0, 0, -1, CONE, true, 2);                \
    } while (0)
#define D2R_MARCH_ANY(COMP, CONE)                                       \
    do {                                                                \
        if (arith) D2R_MARCH_HALF(COMP, CONE);                          \
        else D2R_MARCH_PICK(COMP, CONE);                                \
    } while (0)
    if (cone) {
        if (composite) D2R_MARCH_ANY(true, true);
        else D2R_MARCH_ANY(false, true);
    } else {
        if (composite) D2R_MARCH_ANY(true, false);
        else D2R_MARCH_ANY(false, false);
    }
#undef D2R_MARCH_ANY
#undef D2R_MARCH_HALF
    ctx->last_march_nb = nb;
    ctx->last_march_ngb = ngb;
    ctx->last_march_threads = threads;
    ctx->last_march_gbrick_bytes = ngb ? m->P.gbrick_bytes : 0;
#undef D2R_MARCH_CASE
#undef D2R_MARCH_PICK
#undef D2R_MARCH_C
#undef D2R_MARCH_F
    ctx->timing_end(tm);
    D2R_HIP(ctx, hipGetLastError());
    return D2R_OK;
}

int d2r_launch_bg_quantize(d2r_ctx *ctx, uint32_t w, uint32_t h)
{
    uint32_t n = w * h;
    hipLaunchKernelGGL(k_bg_quantize, dim3((n + 255) / 256), dim3(256), 0, ctx->stream,
                       (const float *)ctx->bg_rgba.p, (uint8_t *)ctx->bg_u8.p, n);
    D2R_HIP(ctx, hipGetLastError());
    return D2R_OK;
}

int d2r_launch_eval_points(d2r_ctx *ctx, const d2r_nerf *m, const float *xyz, const float *dirs, uint32_t n,
                           float *out)
{
    const dim3 g((n + 255) / 256), b(256);
    if (ctx->render_arith == 1) hipLaunchKernelGGL((k_eval_points<-1, true, 1>), g, b, 0, ctx->stream, m->P, xyz, dirs, n, out);
    else if (ctx->render_arith == 2) hipLaunchKernelGGL((k_eval_points<-1, true, 2>), g, b, 0, ctx->stream, m->P, xyz, dirs, n, out);
    else if (m->P.n_dense == 5) {
        if (ctx->mlp_f16) hipLaunchKernelGGL((k_eval_points<5, true>), g, b, 0, ctx->stream, m->P, xyz, dirs, n, out);
        else hipLaunchKernelGGL((k_eval_points<5, false>), g, b, 0, ctx->stream, m->P, xyz, dirs, n, out);
    } else {
        if (ctx->mlp_f16) hipLaunchKernelGGL((k_eval_points<-1, true>), g, b, 0, ctx->stream, m->P, xyz, dirs, n, out);
        else hipLaunchKernelGGL((k_eval_points<-1, false>), g, b, 0, ctx->stream, m->P, xyz, dirs, n, out);
    }
    D2R_HIP(ctx, hipGetLastError());
    return D2R_OK;
}
