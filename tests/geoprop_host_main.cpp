// csrc/geoprop_plane.h in a program of its own: tests/test_geoprop_host.py builds it with -fsanitize=address,undefined and runs it.
//   geoprop_host refusals                            runs every refusal, prints "ok" when each one refuses with a message
//   geoprop_host planes                              the plane choice on hand-made histograms and the selection, prints "ok"
//   geoprop_host bins <b0> .. <b5> <u0> <u1> <u2>    prints "rc lo n" (rc alone when refused)
//   geoprop_host plane <lo> <window> <h0> <h1> ..    prints "bin count inside"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "../dream2real_amd/csrc/geoprop_plane.h"

static std::string g_msg;
int d2r_fail(d2r_ctx *, int code, const std::string &msg)
{
    g_msg = msg;
    return code;
}

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("line %d: %s (last message: %s)\n", __LINE__, #cond, g_msg.c_str()); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static int refused(int rc, const char *word)
{
    const bool ok = rc == D2R_ERR_INVALID && g_msg.find(word) != std::string::npos;
    if (!ok) printf("expected a refusal naming '%s', got rc %d and '%s'\n", word, rc, g_msg.c_str());
    g_msg.clear();
    return ok;
}

static int refusals()
{
    const double bounds[6] = {-0.09, -0.09, -0.03, 0.09, 0.09, 0.08}, up[3] = {0.0, 0.0, 1.0}, K[4] = {380.0, 380.0, 2.0, 1.0};
    const d2r_geoprop_params good = {5, 6, 10, 200, 255};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const uint32_t w = 5, h = 3;
    std::vector<uint16_t> d16(w * h, 300), labels(w * h, 0);
    std::vector<uint32_t> recs(255 * GP_REC_WORDS, 0);
    uint32_t n = 0;
    int32_t plane[D2R_GEOPROP_PLANE_WORDS] = {0, 0, 0, 0, 0};
    float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    GpBins bins;
    memset(&bins, 0x5a, sizeof bins);
    const GpBins untouched = bins;
    struct Args {
        const double *bounds, *up;
        const d2r_geoprop_params *p;
        uint32_t w, h;
        const double *K;
        const uint16_t *d16;
        const float *pose;
        const void *labels, *recs, *n, *plane;
        GpBins *bins;
    };
    const Args ok{bounds, up, &good, w, h, K, d16.data(), pose, labels.data(), recs.data(), &n, plane, &bins};
    auto check = [](const Args &a) { return gp_check(nullptr, a.bounds, a.up, a.p, a.w, a.h, a.K, a.d16, a.pose, a.labels, a.recs, a.n, a.plane, a.bins); };
    Args a = ok;
#define REFUSED(change, word) \
    a = ok;                   \
    change;                   \
    CHECK(refused(check(a), word))
    REFUSED(a.bounds = nullptr, "null");
    REFUSED(a.up = nullptr, "null");
    REFUSED(a.p = nullptr, "null");
    REFUSED(a.K = nullptr, "null");
    REFUSED(a.d16 = nullptr, "null");
    REFUSED(a.pose = nullptr, "null");
    REFUSED(a.labels = nullptr, "null");
    REFUSED(a.recs = nullptr, "null");
    REFUSED(a.n = nullptr, "null");
    REFUSED(a.plane = nullptr, "null");
    REFUSED(a.bins = nullptr, "null");
    REFUSED(a.w = 0, "pixels");
    REFUSED(a.h = 0, "pixels");
    REFUSED((a.w = 2048, a.h = 1025), "pixels");             // refused before anything is read
    float bad[16];
    memcpy(bad, pose, sizeof bad);
    bad[0] = 1.5f;
    REFUSED(a.pose = bad, "rigid");
    memcpy(bad, pose, sizeof bad);
    bad[3] = std::numeric_limits<float>::quiet_NaN();
    REFUSED(a.pose = bad, "rigid");
    memcpy(bad, pose, sizeof bad);
    bad[12] = 0.1f;
    REFUSED(a.pose = bad, "rigid");
    double Kb[4];
    for (double v : {0.0, -380.0, nan, inf}) {
        for (int k = 0; k < 2; ++k) {
            memcpy(Kb, K, sizeof Kb);
            Kb[k] = v;
            REFUSED(a.K = Kb, "focal");
        }
    }
    for (double v : {nan, inf}) {
        memcpy(Kb, K, sizeof Kb);
        Kb[3] = v;
        REFUSED(a.K = Kb, "principal");
    }
    double b2[6];
    memcpy(b2, bounds, sizeof b2);
    b2[4] = nan;
    REFUSED(a.bounds = b2, "bounds");
    memcpy(b2, bounds, sizeof b2);
    b2[0] = 0.09;                                              // min = max
    REFUSED(a.bounds = b2, "bounds");
    b2[0] = 0.1;                                               // min > max
    REFUSED(a.bounds = b2, "bounds");
    memcpy(b2, bounds, sizeof b2);
    b2[5] = 65.6;                                              // 65 630 + 3 bins
    REFUSED(a.bounds = b2, "2^16");
    b2[5] = 1e30;
    REFUSED(a.bounds = b2, "2^16");
    double u2[3] = {0.0, 0.0, 1.00001};
    REFUSED(a.up = u2, "unit");
    u2[2] = 0.0;
    REFUSED(a.up = u2, "unit");
    u2[2] = nan;
    REFUSED(a.up = u2, "unit");
    d2r_geoprop_params p = good;
    for (uint32_t v : {0u, 2u, 4u, 65536u, 65537u}) {
        p = good;
        p.window_mm = v;
        REFUSED(a.p = &p, "window_mm");
    }
    p = good;
    p.h_min_mm = 65536;
    REFUSED(a.p = &p, "h_min_mm");
    p = good;
    p.tau_mm = 65536;
    REFUSED(a.p = &p, "tau_mm");
    for (uint32_t v : {0u, D2R_PROP_MAX + 1u}) {
        p = good;
        p.max_props = v;
        REFUSED(a.p = &p, "max_props");
    }
    CHECK(memcmp(&bins, &untouched, sizeof bins) == 0);
    CHECK(check(ok) == D2R_OK && bins.lo == -31 && bins.n == 113);        // -30 - 1 .. 80 + 1
    p = good;                                                  // the ends of the ranges pass
    p.window_mm = 65535;
    p.h_min_mm = 65535;
    p.tau_mm = 65535;
    p.min_area = 0xffffffffu;
    p.max_props = D2R_PROP_MAX;
    a = ok;
    a.p = &p;
    CHECK(check(a) == D2R_OK);
    p = {1, 0, 0, 0, 1};
    CHECK(check(a) == D2R_OK);
    const double tilted[3] = {0.6, 0.0, 0.8};                  // a unit vector off the axes: the lowest and the highest corner per axis
    a = ok;
    a.up = tilted;
    CHECK(check(a) == D2R_OK && bins.lo == -79 && bins.n == 199);         // 0.6 (-0.09) + 0.8 (-0.03) = -0.078, 0.054 + 0.064 = 0.118: -79 .. 119
    b2[0] = -0.09, b2[1] = -0.09, b2[2] = 0.0, b2[3] = 0.09, b2[4] = 0.09, b2[5] = 65.533;
    a = ok;
    a.bounds = b2;
    CHECK(check(a) == D2R_OK && bins.n == D2R_GEOPROP_MAX_BINS);          // -1 .. 65 534: exactly 2^16 bins pass
    printf("ok\n");
    return 0;
}

static int planes()
{
    auto choose = [](std::vector<uint32_t> hist, int64_t lo, uint32_t window) {
        const GpBins b{lo, (uint32_t)hist.size()};
        return gp_plane(hist.data(), b, window);
    };
    GpPlane pl = choose({0, 0, 0, 0}, -2, 5);
    CHECK(pl.bin == 0 && pl.count == 0 && pl.inside == 0);                 // no pixel inside: no plane
    pl = choose({7}, 12, 5);                                               // a single bin
    CHECK(pl.bin == 12 && pl.count == 7 && pl.inside == 7);
    pl = choose({7}, 12, 1);
    CHECK(pl.bin == 12 && pl.count == 7 && pl.inside == 7);
    pl = choose({0, 0, 0, 9, 0, 0, 0, 0}, 10, 5);                          // one full bin: the windows centred on 11 .. 15 tie, the lowest wins
    CHECK(pl.bin == 11 && pl.count == 9 && pl.inside == 9);
    pl = choose({0, 0, 0, 9, 0, 0, 0, 0}, 10, 1);
    CHECK(pl.bin == 13 && pl.count == 9);
    pl = choose({5, 0, 0, 0, 0, 0, 0, 5}, 0, 3);                           // two equal planes: the lower
    CHECK(pl.bin == 0 && pl.count == 5 && pl.inside == 10);
    pl = choose({5, 0, 0, 0, 0, 0, 0, 6}, 0, 3);                           // the window at the upper end of the range
    CHECK(pl.bin == 6 && pl.count == 6 && pl.inside == 11);
    pl = choose({1, 2, 3, 4, 5, 6, 7, 8}, 0, 3);                           // ... clipped there: 7 + 8 against 6 + 7 + 8 centred one lower
    CHECK(pl.bin == 6 && pl.count == 21);
    pl = choose({8, 7, 6, 5, 4, 3, 2, 1}, -4, 3);                          // the window at the lower end: 8 + 7 against 8 + 7 + 6
    CHECK(pl.bin == -3 && pl.count == 21);
    pl = choose({9, 1, 0, 1, 1, 1, 1, 1}, -4, 3);                          // ... clipped there and tied with the one above it
    CHECK(pl.bin == -4 && pl.count == 10);
    pl = choose({1, 1, 1}, 0, 65535);                                      // a window wider than the range: every bin ties
    CHECK(pl.bin == 0 && pl.count == 3);
    pl = choose({2, 3, 2, 0, 0, 1, 4, 1}, 100, 3);
    CHECK(pl.bin == 101 && pl.count == 7 && pl.inside == 13);

    const GpBins b{-31, 113};
    GpPlane at{2, 10, 10};
    CHECK(gp_threshold(at, b, 6) == 39);                                   // 2 + 6 + 31
    CHECK(gp_threshold(at, b, 79) == 112 && gp_threshold(at, b, 80) == GP_NONE - 1 && gp_threshold(at, b, 65535) == GP_NONE - 1);
    at.inside = 0;
    CHECK(gp_threshold(at, b, 0) == GP_NONE - 1);
    at = {-31, 1, 1};
    CHECK(gp_threshold(at, b, 0) == 0);

    // selection: the largest stay, an area tie goes to the smaller root, the kept ones are ordered by root
    auto recs = [](std::initializer_list<std::pair<uint32_t, uint32_t>> ra) {
        std::vector<uint32_t> v;
        for (auto &p : ra) {
            const uint32_t r[GP_REC_WORDS] = {p.first, p.second, 1, 2, 3, 4};
            v.insert(v.end(), r, r + GP_REC_WORDS);
        }
        return v;
    };
    auto roots = [](const std::vector<uint32_t> &v) {
        std::vector<uint32_t> r;
        for (size_t k = 0; k < v.size(); k += GP_REC_WORDS) r.push_back(v[k]);
        return r;
    };
    std::vector<uint32_t> c = recs({{90, 20}, {10, 20}, {70, 30}, {50, 20}, {30, 10}});
    gp_select(c, 3);
    CHECK((roots(c) == std::vector<uint32_t>{10, 50, 70}) && c[1] == 20 && c[5] == 4);
    c = recs({{90, 20}, {10, 20}, {70, 30}});
    gp_select(c, 3);
    CHECK((roots(c) == std::vector<uint32_t>{10, 70, 90}));
    c = recs({{90, 20}, {10, 20}, {70, 30}});
    gp_select(c, 1);
    CHECK((roots(c) == std::vector<uint32_t>{70}));
    c.clear();
    gp_select(c, 4);
    CHECK(c.empty());
    printf("ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "refusals")) return refusals();
    if (argc == 2 && !strcmp(argv[1], "planes")) return planes();
    if (argc == 11 && !strcmp(argv[1], "bins")) {
        double b[6], u[3];
        for (int i = 0; i < 6; ++i) b[i] = strtod(argv[2 + i], nullptr);
        for (int i = 0; i < 3; ++i) u[i] = strtod(argv[8 + i], nullptr);
        GpBins bins;
        const int rc = gp_bins(nullptr, b, u, &bins);
        if (rc) {
            printf("%d\n", rc);
            return 0;
        }
        printf("0 %lld %u\n", (long long)bins.lo, bins.n);
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "plane")) {
        std::vector<uint32_t> hist;
        for (int i = 4; i < argc; ++i) hist.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
        const GpBins bins{strtoll(argv[2], nullptr, 10), (uint32_t)hist.size()};
        const GpPlane pl = gp_plane(hist.data(), bins, (uint32_t)strtoul(argv[3], nullptr, 10));
        printf("%d %u %u\n", pl.bin, pl.count, pl.inside);
        return 0;
    }
    fprintf(stderr, "usage: geoprop_host refusals | planes | bins <b0> .. <b5> <u0> <u1> <u2> | plane <lo> <window> <h0> ..\n");
    return 2;
}
