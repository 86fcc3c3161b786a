// gjk_steps.cpp — counts the steps of phys.hip's GJK loop on the host.  A plain C++ copy of gjk_intersect and the simplex
// routines of dream2real_amd/csrc/phys.hip (fmaf where the kernel has it, support by a linear scan whose strict '>' is the
// kernel's lowest-index tie rule); the kernel itself carries no counters.  Close to the kernel, not bit-identical: hipcc
// contracts the plain a * b - c * d of cross() and of va, vb, vc into fused operations, this file is built without.  Nothing
// builds it or compares it with phys.hip: after a change to the kernel's simplex routines, copy them here again.
//   c++ -O2 -ffp-contract=off -o gjk_steps tools/gjk_steps.cpp && ./gjk_steps FILE
// FILE (text): na, nb, n_queries, margin2; na + nb vertices (x y z); per query 9 numbers R (row-major), 3 numbers t and the expected answer (1 contact, 0 apart).
// `python -m tests.phys_cases cap FILE [MARGIN]` writes the queries of the 1000-vertex case of tests/test_phys_shapes_gpu.py.
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <vector>
#define __device__
#define __forceinline__ inline
#define __restrict__

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 neg(V3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// ---- closest point to the origin on a simplex of 2 / 3 / 4 points (Ericson, Real-Time Collision Detection 5.1.2, 5.1.5,
// 5.1.6: Voronoi-region tests).  The simplex is reduced in place to the sub-simplex that carries the closest point; the
// functions return that point.  Wave-uniform: every lane runs the same scalar arithmetic.

__device__ V3 closest_segment(V3 *s, int &n)
{
    const V3 a = s[0], b = s[1], ab = b - a;
    const float t = dot(neg(a), ab), den = dot(ab, ab);
    if (t <= 0.f || den <= 0.f) { n = 1; return a; }
    if (t >= den) { s[0] = b; n = 1; return b; }
    const float u = t / den;
    return {fmaf(u, ab.x, a.x), fmaf(u, ab.y, a.y), fmaf(u, ab.z, a.z)};
}

__device__ V3 closest_triangle(V3 *s, int &n)
{
    const V3 a = s[0], b = s[1], c = s[2], ab = b - a, ac = c - a;
    const float d1 = dot(ab, neg(a)), d2 = dot(ac, neg(a));
    if (d1 <= 0.f && d2 <= 0.f) { n = 1; return a; }
    const float d3 = dot(ab, neg(b)), d4 = dot(ac, neg(b));
    if (d3 >= 0.f && d4 <= d3) { s[0] = b; n = 1; return b; }
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        const float v = d1 / (d1 - d3);
        n = 2;                                                     // edge ab: s[0], s[1] stay
        return {fmaf(v, ab.x, a.x), fmaf(v, ab.y, a.y), fmaf(v, ab.z, a.z)};
    }
    const float d5 = dot(ab, neg(c)), d6 = dot(ac, neg(c));
    if (d6 >= 0.f && d5 <= d6) { s[0] = c; n = 1; return c; }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
        const float w = d2 / (d2 - d6);
        s[1] = c; n = 2;                                           // edge ac
        return {fmaf(w, ac.x, a.x), fmaf(w, ac.y, a.y), fmaf(w, ac.z, a.z)};
    }
    const float va = d3 * d6 - d5 * d4;
    if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
        const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        const V3 bc = c - b;
        s[0] = b; s[1] = c; n = 2;                                 // edge bc
        return {fmaf(w, bc.x, b.x), fmaf(w, bc.y, b.y), fmaf(w, bc.z, b.z)};
    }
    const float sum = va + vb + vc;
    if (!(sum > 0.f) || !(sum < INFINITY)) {
        // degenerate (collinear / repeated points: flat hulls, duplicate vertices) — the interior formula would divide by zero and a NaN
        // direction would make every later comparison false.  The closest point then lies on one of the three edges.
        V3 best_s[2] = {a, b};
        int best_n = 2;
        V3 e[2] = {a, b};
        int en = 2;
        V3 q = closest_segment(e, en), best = q;
        best_s[0] = e[0]; best_s[1] = e[1]; best_n = en;
        float bq = dot(q, q);
        const V3 cand[2][2] = {{a, c}, {b, c}};
        for (int k = 0; k < 2; k++) {
            e[0] = cand[k][0]; e[1] = cand[k][1]; en = 2;
            q = closest_segment(e, en);
            const float qq = dot(q, q);
            if (qq < bq) { bq = qq; best = q; best_s[0] = e[0]; best_s[1] = e[1]; best_n = en; }
        }
        s[0] = best_s[0]; s[1] = best_s[1]; n = best_n;
        return best;
    }
    // interior: the foot of the perpendicular, n (a . n) / (n . n).  The barycentric form a + v ab + w ac carries a rounding
    // error of eps |a| in every component, sideways ones included; against a static shape metres wide (a table) and a gap of
    // millimetres that turns v by 1e-4 rad, the support point along -v is then a vertex already held, and the lower bound
    // v . w / |v| is off by 1e-4 m (round 14: 1000 extreme vertices 2 mm over a 2 m slab answered "apart" at 1.97 mm)
    const V3 nrm = cross(ab, ac);
    const float nn = dot(nrm, nrm);
    if (nn > 0.f && nn < INFINITY) {
        const float t = dot(a, nrm) / nn;
        return {t * nrm.x, t * nrm.y, t * nrm.z};
    }
    const float den = 1.f / sum, v = vb * den, w = vc * den;
    return {fmaf(w, ac.x, fmaf(v, ab.x, a.x)), fmaf(w, ac.y, fmaf(v, ab.y, a.y)), fmaf(w, ac.z, fmaf(v, ab.z, a.z))};
}

// false: the origin is inside the tetrahedron (the caller reports an intersection)
__device__ bool closest_tetrahedron(V3 *s, int &n, V3 &out)
{
    const V3 p[4] = {s[0], s[1], s[2], s[3]};
    const int face[4][4] = {{0, 1, 2, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {1, 3, 2, 0}};      // three face vertices, then the opposite one
    float best = INFINITY;
    bool outside_any = false;
    V3 bs[3];
    int bn = 0;
    for (int f = 0; f < 4; f++) {
        const V3 a = p[face[f][0]], b = p[face[f][1]], c = p[face[f][2]], d = p[face[f][3]];
        const V3 nrm = cross(b - a, c - a);
        const float sp = dot(neg(a), nrm), sd = dot(d - a, nrm);
        if (sp * sd < 0.f || sd == 0.f) {                          // the origin lies beyond this face (a flat tetrahedron counts as outside)
            outside_any = true;
            V3 t[3] = {a, b, c};
            int tn = 3;
            const V3 q = closest_triangle(t, tn);
            const float qq = dot(q, q);
            if (qq < best) {
                best = qq;
                out = q;
                bn = tn;
                bs[0] = t[0]; bs[1] = t[1]; bs[2] = t[2];
            }
        }
    }
    if (!outside_any) return false;
    n = bn;
    for (int i = 0; i < bn; i++) s[i] = bs[i];
    return true;
}

static V3 hull_support(const float *verts, uint32_t n, V3 d)
{
    float best = -INFINITY;
    uint32_t bi = 0;
    for (uint32_t i = 0; i < n; i++) {
        const float s = fmaf(verts[3 * i], d.x, fmaf(verts[3 * i + 1], d.y, verts[3 * i + 2] * d.z));
        if (s > best) { best = s; bi = i; }
    }
    return {verts[3 * bi], verts[3 * bi + 1], verts[3 * bi + 2]};
}

// gjk_intersect of phys.hip; *steps: support queries after the first, i.e. passes through the loop body
static bool gjk_intersect(const float *a, uint32_t na, const float R[9], V3 t, const float *b, uint32_t nb, float margin2, int *steps)
{
    auto support = [&](V3 d) -> V3 {
        const V3 dl = {fmaf(R[0], d.x, fmaf(R[3], d.y, R[6] * d.z)), fmaf(R[1], d.x, fmaf(R[4], d.y, R[7] * d.z)),
                       fmaf(R[2], d.x, fmaf(R[5], d.y, R[8] * d.z))};
        const V3 va = hull_support(a, na, dl);
        const V3 wa = {fmaf(R[0], va.x, fmaf(R[1], va.y, fmaf(R[2], va.z, t.x))),
                       fmaf(R[3], va.x, fmaf(R[4], va.y, fmaf(R[5], va.z, t.y))),
                       fmaf(R[6], va.x, fmaf(R[7], va.y, fmaf(R[8], va.z, t.z)))};
        const V3 vb = hull_support(b, nb, neg(d));
        return wa - vb;
    };
    const float m2 = margin2 * margin2;
    V3 s[4];
    int n = 1;
    s[0] = support({1.f, 0.f, 0.f});
    V3 v = s[0];
    for (int it = 0; it < 48; it++) {
        *steps = it + 1;
        const float vv = dot(v, v);
        if (!(vv == vv)) return true;
        if (vv <= m2 || vv < 1e-18f) return true;
        const V3 w = support(neg(v));
        const float vw = dot(v, w);
        if (vw > 0.f && vw * vw > m2 * vv) return false;
        if (vv - vw <= 1e-6f * vv) return false;
        for (int i = 0; i < n; i++)
            if (s[i].x == w.x && s[i].y == w.y && s[i].z == w.z) return false;
        s[n++] = w;
        if (n == 2) v = closest_segment(s, n);
        else if (n == 3) v = closest_triangle(s, n);
        else if (!closest_tetrahedron(s, n, v)) return true;
    }
    *steps = 49;                                                  // ran into the cap
    return dot(v, v) <= m2;
}

int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: gjk_steps FILE\n"); return 2; }
    unsigned na, nb, nq;
    float margin2;
    if (fscanf(f, "%u %u %u %f", &na, &nb, &nq, &margin2) != 4) return 2;
    std::vector<float> v(3 * (size_t)(na + nb));
    for (float &x : v)
        if (fscanf(f, "%f", &x) != 1) return 2;
    int worst = 0, wrong = 0, capped = 0;
    for (unsigned q = 0; q < nq; q++) {
        float R[9], t[3];
        int expect = 0;
        for (float &x : R) if (fscanf(f, "%f", &x) != 1) return 2;
        for (float &x : t) if (fscanf(f, "%f", &x) != 1) return 2;
        if (fscanf(f, "%d", &expect) != 1) return 2;
        int steps = 0;
        const bool hit = gjk_intersect(v.data(), na, R, {t[0], t[1], t[2]}, v.data() + 3 * (size_t)na, nb, margin2, &steps);
        printf("query %u: %s after %d steps%s%s\n", q, hit ? "contact" : "apart", steps, steps > 48 ? " (THE CAP)" : "",
               hit != (expect != 0) ? " WRONG" : "");
        worst = steps > worst ? steps : worst;
        wrong += hit != (expect != 0);
        capped += steps > 48;
    }
    printf("most steps: %d of 48; %d of %u queries ran into the cap; %d wrong answers\n", worst > 48 ? 48 : worst, capped, nq, wrong);
    fclose(f);
    return 0;
}
