// The ray caster's host arithmetic (dream2real_amd/csrc/tsdfvis_rect.h) in a program of its own: tests/test_tsdfvis_host.py
// builds it with -fsanitize=address,undefined and runs it.  Prints "ok" when every check holds.
#include <stdio.h>

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

int main()
{
    float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(tv_is_rigid(I));
    float T[16];
    for (int i = 0; i < 16; ++i) T[i] = I[i];
    T[0] = 1.01f;
    CHECK(!tv_is_rigid(T));                  // scaled
    T[0] = 1.0f;
    T[3] = INFINITY;
    CHECK(!tv_is_rigid(T));                  // not finite
    T[3] = 5.0f;
    T[15] = 2.0f;
    CHECK(!tv_is_rigid(T));                  // last row
    T[15] = 1.0f;
    T[5] = T[10] = 0.0f;                     // a quarter turn about x
    T[6] = -1.0f;
    T[9] = 1.0f;
    CHECK(tv_is_rigid(T));

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
    CHECK(!tv_is_rigid(T));
    // a rotated transform: the camera looks back along -z from z = 3
    const double B[16] = {-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 3, 0, 0, 0, 1};
    CHECK(same(tv_box_rect(B, lo, hi, 0.0, fx, fy, cx, cy, near, W, H), 39, 29, 51, 41));
    if (failures == 0) printf("ok\n");
    return failures != 0;
}
