// The ray caster's host arithmetic (dream2real_amd/csrc/tsdfvis_rect.h, d2r_shared.h's d2r_is_rigid) in a program of its own: tests/test_tsdfvis_host.py
// builds it with -fsanitize=address,undefined and runs it.  Prints "ok" when every check holds.
#include <stdio.h>

#include "../dream2real_amd/csrc/d2r_shared.h"
#include "../dream2real_amd/csrc/tsdfvis_rect.h"

static int failures = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            printf("line %d: %s\n", __LINE__, #cond);             \
            ++failures;                                           \
        }                                                         \
    } while (0)

static bool same(TvRect r, int x0, int y0, int x1, int y1) { return r.x0 == x0 && r.y0 == y0 && r.x1 == x1 && r.y1 == y1; }

// a candidate's rectangle as tv_prepare builds it: the box under the true inverse of the fp32 ray matrix m
static TvRect rect_of(const float m[12], const double lo[3], const double hi[3], double slack, double fx, double fy, double cx, double cy,
                      double near, int W, int H)
{
    double inv[16];
    tv_inverse34(m, inv);
    return tv_box_rect(inv, lo, hi, slack, fx, fy, cx, cy, near, W, H);
}

int main()
{
    float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(d2r_is_rigid(I));
    float T[16];
    for (int i = 0; i < 16; ++i) T[i] = I[i];
    T[0] = 1.01f;
    CHECK(!d2r_is_rigid(T));                  // scaled
    T[0] = 1.0f;
    T[3] = INFINITY;
    CHECK(!d2r_is_rigid(T));                  // not finite
    T[3] = 5.0f;
    T[15] = 2.0f;
    CHECK(!d2r_is_rigid(T));                  // last row
    T[15] = 1.0f;
    T[5] = T[10] = 0.0f;                     // a quarter turn about x
    T[6] = -1.0f;
    T[9] = 1.0f;
    CHECK(d2r_is_rigid(T));

    const double E[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const double fx = 100, fy = 100, cx = 50, cy = 40, near = 0.01;
    const int W = 100, H = 80;
    // a box in front of the camera: x 0 .. 0.1, y -0.1 .. 0, z 1 .. 2 -> u 50 .. 60, v 30 .. 40, a pixel wider
    double lo[3] = {0, -0.1, 1}, hi[3] = {0.1, 0, 2};
    CHECK(same(tv_box_rect(E, lo, hi, 0.0, fx, fy, cx, cy, near, W, H), 49, 29, 61, 41));
    // slack widens it
    TvRect r = tv_box_rect(E, lo, hi, 0.05, fx, fy, cx, cy, near, W, H);
    CHECK(r.x0 < 49 && r.x1 > 61 && r.y0 < 29 && r.y1 > 41);
    // clipped by each border
    double lo2[3] = {-2, -2, 1}, hi2[3] = {2, 2, 2};
    CHECK(same(tv_box_rect(E, lo2, hi2, 0.0, fx, fy, cx, cy, near, W, H), 0, 0, W - 1, H - 1));
    // wholly off screen: no pixel
    double lo3[3] = {5, 0, 1}, hi3[3] = {6, 0.1, 2};
    r = tv_box_rect(E, lo3, hi3, 0.0, fx, fy, cx, cy, near, W, H);
    CHECK(r.x1 < r.x0);
    // a corner at or behind the near plane: the whole frame
    double lo4[3] = {0, 0, 0.01}, hi4[3] = {0.1, 0.1, 2};
    CHECK(same(tv_box_rect(E, lo4, hi4, 0.0, fx, fy, cx, cy, near, W, H), 0, 0, W - 1, H - 1));
    double lo5[3] = {0, 0, -1}, hi5[3] = {0.1, 0.1, 2};
    CHECK(same(tv_box_rect(E, lo5, hi5, 0.0, fx, fy, cx, cy, 0.0, W, H), 0, 0, W - 1, H - 1));
    // an empty box: no pixel; not finite: the whole frame
    double lo6[3] = {0, 0, 1}, hi6[3] = {-0.003, 0.1, 2};
    r = tv_box_rect(E, lo6, hi6, 0.0, fx, fy, cx, cy, near, W, H);
    CHECK(r.x1 < r.x0);
    double lo7[3] = {0, NAN, 1};
    CHECK(same(tv_box_rect(E, lo7, hi, 0.0, fx, fy, cx, cy, near, W, H), 0, 0, W - 1, H - 1));
    CHECK(same(tv_box_rect(E, lo, hi, INFINITY, fx, fy, cx, cy, near, W, H), 0, 0, W - 1, H - 1));
    // a huge focal length: u runs from 50 (x = 0) to 1e307, clamped to the frame before the conversion to int
    CHECK(same(tv_box_rect(E, lo, hi, 0.0, 1e308, fy, cx, cy, near, W, H), 49, 29, W - 1, 41));
    // off by more than 1e-5 from orthogonal: refused (the rectangle and the rule invert by transposition)
    T[5] = 1e-4f;
    CHECK(!d2r_is_rigid(T));
    // a rotated transform: the camera looks back along -z from z = 3
    const double B[16] = {-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 3, 0, 0, 0, 1};
    CHECK(same(tv_box_rect(B, lo, hi, 0.0, fx, fy, cx, cy, near, W, H), 39, 29, 51, 41));
    // the inverse of a rigid matrix is its transposed inverse; of a singular or non-finite one, NaNs, and the whole frame
    {
        const float b[12] = {-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 3};
        double inv[16];
        tv_inverse34(b, inv);
        for (int i = 0; i < 16; ++i) CHECK(inv[i] == B[i]);
        const float z[12] = {1, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0};
        CHECK(same(rect_of(z, lo, hi, 0.0, fx, fy, cx, cy, near, W, H), 0, 0, W - 1, H - 1));
        const float n[12] = {1, 0, 0, NAN, 0, 1, 0, 0, 0, 0, 1, 0};
        CHECK(same(rect_of(n, lo, hi, 0.0, fx, fy, cx, cy, near, W, H), 0, 0, W - 1, H - 1));
    }
    // the rectangle inputs of tests/tsdfvis_edge_cases.py (the values tests/tsdfvis_ref.py's candidate_rect is given and gives)
    {   // E8: a rectangle of one pixel
        const float m[12] = {1.0, 0.0, 0.0, 0.19140625, 0.0, 1.0, 0.0, 0.2578125, 0.0, 0.0, 1.0, 0.0};
        const double lo[3] = {-0.06640625, -0.06640625, 0.18359375}, hi[3] = {0.06640625, 0.06640625, 0.31640625};
        CHECK(same(rect_of(m, lo, hi, 2.3031249999999997e-05, 24.0, 16.0, 8.0, 8.0, 0.0078125, 17, 17), 0, 0, 0, 0));
    }
    {   // E8: a rectangle that ends on column 15, a tile's last
        const float m[12] = {1.0, 0.0, 0.0, 0.0234375, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
        const double lo[3] = {-0.06640625, -0.06640625, 0.18359375}, hi[3] = {0.06640625, 0.06640625, 0.31640625};
        CHECK(same(rect_of(m, lo, hi, 2.209375e-05, 24.0, 16.0, 8.0, 8.0, 0.0078125, 17, 17), 0, 1, 15, 15));
    }
    {   // E8: a rectangle that starts on column 16, the next tile's first
        const float m[12] = {1.0, 0.0, 0.0, -0.19140625, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
        const double lo[3] = {-0.06640625, -0.06640625, 0.18359375}, hi[3] = {0.06640625, 0.06640625, 0.31640625};
        CHECK(same(rect_of(m, lo, hi, 2.2765625e-05, 24.0, 16.0, 8.0, 8.0, 0.0078125, 17, 17), 16, 1, 16, 15));
    }
    {   // E12: a pose scaled by 1 + 4.5e-6 two kilometres from the origin; the transposed inverses gave 30 .. 47 here
        const float m[12] = {0.9999954700469971, 0.0, 0.0, 2047.92822265625, 0.0, 0.9999954700469971, 0.0, -1023.995361328125, 0.0, 0.0, 0.9999954700469971, 511.7476806640625};
        const double lo[3] = {2047.93359375, -1024.06640625, 512.18359375}, hi[3] = {2048.06640625, -1023.93359375, 512.31640625};
        CHECK(same(rect_of(m, lo, hi, 0.008204744141757488, 512.0, 512.0, 24.0, 20.0, 0.0078125, 48, 40), 19, 0, 47, 39));
    }
    {   // E12: the same scaled the other way
        const float m[12] = {1.000004529953003, 0.0, 0.0, 2047.94677734375, 0.0, 1.000004529953003, 0.0, -1024.004638671875, 0.0, 0.0, 1.000004529953003, 511.7523193359375};
        const double lo[3] = {2047.93359375, -1024.06640625, 512.18359375}, hi[3] = {2048.06640625, -1023.93359375, 512.31640625};
        CHECK(same(rect_of(m, lo, hi, 0.008204818358242511, 512.0, 512.0, 24.0, 20.0, 0.0078125, 48, 40), 0, 0, 47, 39));
    }

    if (failures == 0) printf("ok\n");
    return failures != 0;
}
