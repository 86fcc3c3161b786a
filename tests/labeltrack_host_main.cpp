// csrc/labeltrack_grid.h in a program of its own: tests/test_labeltrack_host.py builds it with -fsanitize=address,undefined and runs it.
//   labeltrack_host grid <voxel> <band_voxels> <b0> .. <b5>   prints "rc lo0 lo1 lo2 n0 n1 n2 n_vox" (rc alone when refused)
//   labeltrack_host refusals                                    runs every refusal, prints "ok" when each one refuses with a message
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "../dream2real_amd/csrc/labeltrack_grid.h"

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
    const double bounds[6] = {-0.09, -0.09, -0.03, 0.09, 0.09, 0.08};
    const d2r_labeltrack_params good = {0.004f, 2, 10, 64};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    LtGrid g;
    memset(&g, 0x5a, sizeof g);
    const LtGrid untouched = g;
    CHECK(refused(lt_grid(nullptr, nullptr, &good, &g), "null"));
    CHECK(refused(lt_grid(nullptr, bounds, nullptr, &g), "null"));
    CHECK(refused(lt_grid(nullptr, bounds, &good, nullptr), "null"));
    d2r_labeltrack_params p = good;
    for (float v : {0.f, -0.004f, nan, inf}) {
        p = good;
        p.voxel = v;
        CHECK(refused(lt_grid(nullptr, bounds, &p, &g), "voxel"));
    }
    for (uint32_t b : {0u, 9u, 0xffffffffu}) {
        p = good;
        p.band_voxels = b;
        CHECK(refused(lt_grid(nullptr, bounds, &p, &g), "band_voxels"));
    }
    p = good;
    p.tau_mm = 65536;
    CHECK(refused(lt_grid(nullptr, bounds, &p, &g), "tau_mm"));
    p = good;
    p.grow = 4097;
    CHECK(refused(lt_grid(nullptr, bounds, &p, &g), "grow"));
    p = good;
    p.voxel = 1e-5f;                                           // 18000 x 18000 x 11000 voxels
    CHECK(refused(lt_grid(nullptr, bounds, &p, &g), "2^31"));
    p.voxel = 3e-38f;                                          // the quotient is beyond every integer type
    CHECK(refused(lt_grid(nullptr, bounds, &p, &g), "2^23"));
    double b2[6];
    memcpy(b2, bounds, sizeof b2);
    b2[4] = (double)nan;
    CHECK(refused(lt_grid(nullptr, b2, &good, &g), "bounds"));
    memcpy(b2, bounds, sizeof b2);
    b2[0] = 0.1;                                               // min > max
    CHECK(refused(lt_grid(nullptr, b2, &good, &g), "bounds"));
    memcpy(b2, bounds, sizeof b2);
    b2[3] = 1e5;
    CHECK(refused(lt_grid(nullptr, b2, &good, &g), "2^23"));
    CHECK(memcmp(&g, &untouched, sizeof g) == 0);
    p = good;                                                  // the ends of the ranges pass
    p.band_voxels = 8;
    p.tau_mm = 65535;
    p.grow = 4096;
    CHECK(lt_grid(nullptr, bounds, &p, &g) == D2R_OK && g.band == 8.f * 0.004f);
    p.band_voxels = 1;
    p.tau_mm = 0;
    p.grow = 0;
    CHECK(lt_grid(nullptr, bounds, &p, &g) == D2R_OK && g.n_vox == g.n[0] * g.n[1] * g.n[2]);

    const uint32_t w = 5, h = 3, n = 2;
    const double K[4] = {380.0, 380.0, 2.0, 1.0};
    std::vector<uint16_t> d16(n * w * h, 300);
    std::vector<uint8_t> labels0(w * h, 1), out(n * w * h, 0);
    std::vector<float> poses(n * 16, 0.f);
    for (uint32_t f = 0; f < n; ++f) poses[f * 16] = poses[f * 16 + 5] = poses[f * 16 + 10] = poses[f * 16 + 15] = 1.f;
    auto frames = [&](uint32_t nn, uint32_t ww, uint32_t hh, const double *k, const uint16_t *d, const float *ps, const uint8_t *l, const uint8_t *o) {
        return lt_check_frames(nullptr, nn, ww, hh, k, d, ps, l, o);
    };
    CHECK(frames(n, w, h, K, d16.data(), poses.data(), labels0.data(), out.data()) == D2R_OK);
    CHECK(refused(frames(n, w, h, nullptr, d16.data(), poses.data(), labels0.data(), out.data()), "null"));
    CHECK(refused(frames(n, w, h, K, nullptr, poses.data(), labels0.data(), out.data()), "null"));
    CHECK(refused(frames(n, w, h, K, d16.data(), nullptr, labels0.data(), out.data()), "null"));
    CHECK(refused(frames(n, w, h, K, d16.data(), poses.data(), nullptr, out.data()), "null"));
    CHECK(refused(frames(n, w, h, K, d16.data(), poses.data(), labels0.data(), nullptr), "null"));
    CHECK(refused(frames(0, w, h, K, d16.data(), poses.data(), labels0.data(), out.data()), "no frames"));
    CHECK(refused(frames(n, 0, h, K, d16.data(), poses.data(), labels0.data(), out.data()), "pixels"));
    CHECK(refused(frames(n, w, 0, K, d16.data(), poses.data(), labels0.data(), out.data()), "pixels"));
    CHECK(refused(frames(n, 2048, 1025, K, d16.data(), poses.data(), labels0.data(), out.data()), "pixels"));   // refused before anything is read
    std::vector<float> bad = poses;
    bad[16] = 1.5f;
    CHECK(refused(frames(n, w, h, K, d16.data(), bad.data(), labels0.data(), out.data()), "cam_pose 1"));
    bad = poses;
    bad[3] = nan;
    CHECK(refused(frames(n, w, h, K, d16.data(), bad.data(), labels0.data(), out.data()), "cam_pose 0"));
    bad = poses;
    bad[16 + 12] = 0.1f;
    CHECK(refused(frames(n, w, h, K, d16.data(), bad.data(), labels0.data(), out.data()), "cam_pose 1"));
    double Kb[4] = {0.0, 380.0, 2.0, 1.0};
    CHECK(refused(frames(n, w, h, Kb, d16.data(), poses.data(), labels0.data(), out.data()), "focal"));
    Kb[0] = 380.0;
    Kb[1] = (double)inf;
    CHECK(refused(frames(n, w, h, Kb, d16.data(), poses.data(), labels0.data(), out.data()), "finite"));
    Kb[1] = 380.0;
    Kb[3] = (double)nan;
    CHECK(refused(frames(n, w, h, Kb, d16.data(), poses.data(), labels0.data(), out.data()), "finite"));
    Kb[3] = 1.0;
    Kb[0] = 1e-60;                                             // not zero in fp64, zero in the fp32 the kernels divide by
    CHECK(refused(frames(n, w, h, Kb, d16.data(), poses.data(), labels0.data(), out.data()), "fp32"));
    labels0[w * h - 1] = 255;
    CHECK(refused(frames(n, w, h, K, d16.data(), poses.data(), labels0.data(), out.data()), "255"));
    labels0[w * h - 1] = 254;
    CHECK(frames(n, w, h, K, d16.data(), poses.data(), labels0.data(), out.data()) == D2R_OK);
    printf("ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "refusals")) return refusals();
    if (argc == 10 && !strcmp(argv[1], "grid")) {
        d2r_labeltrack_params p = {strtof(argv[2], nullptr), (uint32_t)strtoul(argv[3], nullptr, 10), 10, 64};
        double b[6];
        for (int i = 0; i < 6; ++i) b[i] = strtod(argv[4 + i], nullptr);
        LtGrid g;
        const int rc = lt_grid(nullptr, b, &p, &g);
        if (rc) {
            printf("%d\n", rc);
            return 0;
        }
        printf("0 %d %d %d %u %u %u %u\n", g.lo[0], g.lo[1], g.lo[2], g.n[0], g.n[1], g.n[2], g.n_vox);
        return 0;
    }
    fprintf(stderr, "usage: labeltrack_host grid <voxel> <band_voxels> <b0> .. <b5> | refusals\n");
    return 2;
}
