// The pure host parts of dream2real_amd/csrc/d2r_shared.h, checked without the library and without a device: the staging layout,
// the fp64 4x4 product's summation order, the 4x4 rigid inverse, the colour packer.  Prints one line per failure, then "ok" or the
// number of failures; tests/test_shared_host.py builds and runs it.
#include <stdio.h>
#include <string.h>

#include "d2r_shared.h"

static int failures = 0;

#define CHECK(cond, ...)             \
    do {                             \
        if (!(cond)) {               \
            ++failures;              \
            printf("FAIL: ");        \
            printf(__VA_ARGS__);     \
            printf("\n");            \
        }                            \
    } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

static void check_layout()
{
    D2rLayout empty;
    CHECK(empty.total() == 0, "an empty layout has total %zu", empty.total());

    const size_t sizes[] = {0, 1, 255, 256, 257, ((size_t)1 << 32) + 1};
    const int n = (int)(sizeof sizes / sizeof sizes[0]);
    size_t off[6];
    D2rLayout L;
    for (int i = 0; i < n; ++i) off[i] = L.add(sizes[i]);
    for (int i = 0; i < n; ++i) {
        CHECK(off[i] % 256 == 0, "segment %d starts at %zu, no multiple of 256", i, off[i]);
        if (i) CHECK(off[i] >= off[i - 1], "segment %d starts at %zu, before segment %d at %zu", i, off[i], i - 1, off[i - 1]);
        if (i) CHECK(off[i - 1] + sizes[i - 1] <= off[i], "segment %d ends at %zu, past the start %zu of the next", i - 1, off[i - 1] + sizes[i - 1], off[i]);
    }
    CHECK(L.total() == off[n - 1] + sizes[n - 1], "total %zu is not the end %zu of the last segment", L.total(), off[n - 1] + sizes[n - 1]);

    // a, then nothing, then b: b lies where it lies without the empty segment, give or take the alignment
    D2rLayout with, without;
    with.add(300);
    const size_t hole = with.add(0), b_with = with.add(77);
    without.add(300);
    const size_t b_without = without.add(77);
    CHECK(hole % 256 == 0 && hole >= 300, "an empty segment at %zu", hole);
    CHECK(b_with >= b_without && b_with - b_without <= 256, "an empty segment moved its successor from %zu to %zu", b_without, b_with);
}

static void check_mul4()
{
    // Column j of B is 2^j in every row, so entry (i, j) is 2^j times the sum of row i of A in the order taken.  One ulp of 1e16
    // is 2: row 0 gives 1 left to right (the first 1 is absorbed, the last survives) and 0 right to left; row 1 gives 4 and 5,
    // row 3 gives 1.001 and 2.  Row 2 is ordinary numbers.
    const double big = 1e16;
    double A[16], B[16], C[16];
    const double rows[4][4] = {{big, 1.0, -big, 1.0}, {1.0, big, 3.0, -big}, {0.1, 0.2, 0.3, 0.4}, {-big, big, 1.0, 1e-3}};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            A[i * 4 + j] = rows[i][j];
            B[i * 4 + j] = (double)(1 << j);
        }
    d2r_mul4(A, B, C);
    int order_matters = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const double a0 = A[i * 4 + 0], a1 = A[i * 4 + 1], a2 = A[i * 4 + 2], a3 = A[i * 4 + 3];
            const double b0 = B[0 * 4 + j], b1 = B[1 * 4 + j], b2 = B[2 * 4 + j], b3 = B[3 * 4 + j];
            volatile double ltr = ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3;
            volatile double rtl = a0 * b0 + (a1 * b1 + (a2 * b2 + a3 * b3));
            CHECK(same_bits(C[i * 4 + j], ltr), "product entry (%d, %d) is %.17g, left to right gives %.17g", i, j, C[i * 4 + j], (double)ltr);
            if (!same_bits(ltr, rtl)) ++order_matters;
        }
    CHECK(order_matters >= 12, "the inputs tell the summation orders apart in %d entries only, not in rows 0, 1 and 3", order_matters);
    CHECK(same_bits(C[0], 1.0) && same_bits(C[4], 4.0), "rows 0 and 1 sum to %.17g and %.17g left to right, not to 1 and 4", C[0], C[4]);
}

static void check_rigid_inverse()
{
    // Rz(cos 0.6, sin 0.8) Rx(cos 0.28, sin 0.96), orthonormal in the reals and to a float's rounding here, and a translation
    const float T[16] = {0.6f, -0.224f, 0.768f, 0.25f, 0.8f, 0.168f, -0.576f, -1.5f, 0.f, 0.96f, 0.28f, 3.125f, 0.f, 0.f, 0.f, 1.f};
    double r12[12], r16[16];
    d2r_rigid_inverse(T, r12);
    for (int i = 0; i < 16; ++i) r16[i] = -7.0;
    d2r_rigid_inverse4(T, r16);
    for (int i = 0; i < 12; ++i) CHECK(same_bits(r16[i], r12[i]), "4x4 inverse entry %d is %.17g, the 3x4 form has %.17g", i, r16[i], r12[i]);
    CHECK(same_bits(r16[12], 0.0) && same_bits(r16[13], 0.0) && same_bits(r16[14], 0.0) && same_bits(r16[15], 1.0),
          "the 4x4 inverse ends in %g %g %g %g", r16[12], r16[13], r16[14], r16[15]);
    double P[16], I[16];
    d2r_load16(T, P);
    for (int i = 0; i < 16; ++i) CHECK(same_bits(P[i], (double)T[i]), "load16 entry %d", i);
    d2r_mul4(r16, P, I);
    for (int i = 0; i < 16; ++i) CHECK(fabs(I[i] - (i % 5 == 0 ? 1.0 : 0.0)) < 1e-6, "inverse x pose entry %d is %.9g", i, I[i]);
    float m[12];
    d2r_round34(r16, m);
    for (int i = 0; i < 12; ++i) CHECK(m[i] == (float)r16[i], "round34 entry %d", i);
}

static void check_packer()
{
    const uint8_t triples[3][3] = {{0, 0, 0}, {255, 255, 255}, {18, 200, 7}};
    for (const auto &t : triples) {
        const uint32_t v = d2r_pack_rgb(t);
        CHECK((v & 255u) == t[0] && ((v >> 8) & 255u) == t[1] && ((v >> 16) & 255u) == t[2] && (v >> 24) == 0u,
              "(%u, %u, %u) packs to %#x", (unsigned)t[0], (unsigned)t[1], (unsigned)t[2], (unsigned)v);
    }
}

int main()
{
    check_layout();
    check_mul4();
    check_rigid_inverse();
    check_packer();
    if (failures) printf("%d failures\n", failures);
    else printf("ok\n");
    return failures ? 1 : 0;
}
