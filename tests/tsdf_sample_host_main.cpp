// How a point meets a TSDF volume (dream2real_amd/csrc/tsdf_sample.h) in a program of its own: tests/test_tsdfvis_host.py builds it
// with -fsanitize=address,undefined -ffp-contract=off, hands it a volume and points, and compares what it writes with the numpy
// restatements bit for bit.
//   in:  int32 nv[3], nb[3], lo[3], n_points, n_modes; float voxel, thr; (tsdf, weight) float [nz][ny][nx][2]; uint8 ever[nbz nby nbx];
//        per mode int32 flags, float clo[3], chi[3]; float p[n_points][3]
//   out: per mode, per point: int32 in (ts_cell), int32 observed (ts_corners), int64 base, float f[3], value, g[3]
//        (base, value and g are 0 where the cell is refused: nothing may be read there)
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../dream2real_amd/csrc/tsdf_sample.h"

template <class T>
static bool get(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool put(FILE *f, const T *p, size_t n) { return fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t h[11];
    float s[2];
    if (!get(in, h, 11) || !get(in, s, 2)) return 3;
    D2rTsdfDev V{};
    size_t n_vox = 1, n_blocks = 1;
    for (int a = 0; a < 3; ++a) {
        V.nv[a] = (uint32_t)h[a];
        V.nb[a] = (uint32_t)h[3 + a];
        V.lo[a] = h[6 + a];
        n_vox *= V.nv[a];
        n_blocks *= V.nb[a];
    }
    const int n_points = h[9], n_modes = h[10];
    V.voxel = s[0];
    const float thr = s[1];
    // exactly as many voxels as the grid holds: a read past the last one is the address sanitizer's to report
    std::vector<TsVoxel> vox(n_vox);
    std::vector<uint8_t> ever(n_blocks);
    std::vector<int32_t> flags(n_modes);
    std::vector<float> box((size_t)n_modes * 6), pts((size_t)n_points * 3);
    if (!get(in, (float *)vox.data(), n_vox * 2) || !get(in, ever.data(), n_blocks)) return 3;
    for (int m = 0; m < n_modes; ++m)
        if (!get(in, &flags[m], 1) || !get(in, &box[(size_t)m * 6], 6)) return 3;
    if (!get(in, pts.data(), pts.size())) return 3;
    V.vox = vox.data();
    V.ever = ever.data();
    for (int m = 0; m < n_modes; ++m) {
        memcpy(V.clo, &box[(size_t)m * 6], 12);
        memcpy(V.chi, &box[(size_t)m * 6 + 3], 12);
        for (int i = 0; i < n_points; ++i) {
            const float p[3] = {pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2]};
            size_t base = 0;
            float f[3], t[8], g[3] = {0.f, 0.f, 0.f}, val = 0.f;
            const bool cell = flags[m] ? ts_cell<true>(V, p, base, f) : ts_cell<false>(V, p, base, f);
            bool obs = false;
            if (cell) {
                obs = ts_corners(V, base, thr, t);
                val = ts_lerp3_grad(t, f, g);
                const float alone = ts_lerp3(t, f);
                if (memcmp(&val, &alone, 4) != 0) return 4;                               // the value alone is the same value
            }
            const int32_t b[2] = {cell, obs};
            const int64_t q = (int64_t)base;
            if (!put(out, b, 2) || !put(out, &q, 1) || !put(out, f, 3) || !put(out, &val, 1) || !put(out, g, 3)) return 5;
        }
    }
    if (fclose(out) != 0) return 5;
    fclose(in);
    printf("ok\n");
    return 0;
}
