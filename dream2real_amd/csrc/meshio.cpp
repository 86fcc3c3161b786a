// meshio.cpp — what follows the marching cubes on the host (reference vision_3d/physics_utils.py:102-115, 175-176; DESIGN.md
// section 2c "clean-up" and "files"): the inclusive crop to scene_bounds, connected triangle clusters and the removal of the
// small ones, the centre of the vertex array, and mesh_concave_{id}.obj.  None of it is hot: one pass each over a mesh of
// some 10^5 triangles.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "d2r_internal.h"
#include <algorithm>

#include "meshio.h"

void d2r_mesh_clean(const float *verts, size_t nv, const uint32_t *tris, size_t nt, const float *crop, double keep_frac, D2rMesh &out)
{
    out = D2rMesh();
    std::vector<uint8_t> inside(nv, 1);
    if (crop)
        for (size_t i = 0; i < nv; ++i)
            for (int a = 0; a < 3; ++a)
                if (!(verts[3 * i + a] >= crop[a] && verts[3 * i + a] <= crop[3 + a])) inside[i] = 0;
    std::vector<uint8_t> used(nv, 0);
    std::vector<uint8_t> tkeep(nt, 0);
    for (size_t t = 0; t < nt; ++t) {
        const uint32_t *q = tris + 3 * t;
        if (inside[q[0]] && inside[q[1]] && inside[q[2]]) {
            tkeep[t] = 1;
            used[q[0]] = used[q[1]] = used[q[2]] = 1;
        }
    }
    std::vector<uint32_t> remap(nv, 0xffffffffu);
    for (size_t i = 0; i < nv; ++i)
        if (used[i]) {
            remap[i] = (uint32_t)(out.verts.size() / 3);
            out.verts.insert(out.verts.end(), verts + 3 * i, verts + 3 * i + 3);
        }
    for (size_t t = 0; t < nt; ++t)
        if (tkeep[t])
            for (int c = 0; c < 3; ++c) out.tris.push_back(remap[tris[3 * t + c]]);
    const size_t mv = out.verts.size() / 3, mt = out.tris.size() / 3;
    // clusters: union-find over vertices
    std::vector<uint32_t> parent(mv);
    for (size_t i = 0; i < mv; ++i) parent[i] = (uint32_t)i;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    };
    for (size_t t = 0; t < mt; ++t) {
        const uint32_t a = find(out.tris[3 * t]), b = find(out.tris[3 * t + 1]);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
        const uint32_t a2 = find(out.tris[3 * t]), c = find(out.tris[3 * t + 2]);
        if (a2 != c) parent[std::max(a2, c)] = std::min(a2, c);
    }
    std::vector<int32_t> of_root(mv, -1);
    std::vector<uint64_t> size;
    out.label.resize(mt);
    for (size_t t = 0; t < mt; ++t) {
        const uint32_t r = find(out.tris[3 * t]);
        if (of_root[r] < 0) {
            of_root[r] = (int32_t)size.size();
            size.push_back(0);
        }
        out.label[t] = of_root[r];
        ++size[(size_t)of_root[r]];
    }
    out.n_clusters = (uint32_t)size.size();
    uint64_t largest = 0;
    for (uint64_t s : size) largest = std::max(largest, s);
    const double threshold = keep_frac * (double)largest;
    out.keep.resize(mt);
    for (size_t t = 0; t < mt; ++t) out.keep[t] = !((double)size[(size_t)out.label[t]] < threshold);
    double s[3] = {0, 0, 0};
    for (size_t i = 0; i < mv; ++i)
        for (int a = 0; a < 3; ++a) s[a] += (double)out.verts[3 * i + a];
    for (int a = 0; a < 3; ++a) out.centre[a] = mv ? s[a] / (double)mv : 0.0;
}

// "v %f %f %f" per vertex, then "f %u %u %u" (1-based) per kept triangle
extern "C" int d2r_obj_write(const char *path, const float *vertices, uint32_t n_vertices, const uint32_t *triangles, uint32_t n_triangles,
                             const uint8_t *keep)
{
    if (!path || (n_vertices && !vertices) || (n_triangles && !triangles)) return d2r_fail(nullptr, D2R_ERR_INVALID, "null argument");
    for (size_t i = 0; i < (size_t)n_triangles * 3; ++i)
        if (triangles[i] >= n_vertices) return d2r_fail(nullptr, D2R_ERR_INVALID, "d2r_obj_write: a triangle references a vertex out of range");
    FILE *f = fopen(path, "wb");
    if (!f) return d2r_fail(nullptr, D2R_ERR_INVALID, std::string("cannot open ") + path + " for writing");
    std::string s;
    s.reserve((size_t)n_vertices * 40 + (size_t)n_triangles * 30);
    char line[160];
    for (size_t i = 0; i < n_vertices; ++i) {
        const int n = snprintf(line, sizeof line, "v %f %f %f\n", (double)vertices[3 * i], (double)vertices[3 * i + 1], (double)vertices[3 * i + 2]);
        s.append(line, (size_t)n);
    }
    for (size_t t = 0; t < n_triangles; ++t) {
        if (keep && !keep[t]) continue;
        const int n = snprintf(line, sizeof line, "f %u %u %u\n", triangles[3 * t] + 1, triangles[3 * t + 1] + 1, triangles[3 * t + 2] + 1);
        s.append(line, (size_t)n);
    }
    const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
    if (fclose(f) != 0 || !ok) return d2r_fail(nullptr, D2R_ERR_INVALID, std::string("short write to ") + path);
    return D2R_OK;
}

// `v` and `f` lines of a Wavefront .obj; see include/d2r.h.  A number is read as fp64 (strtod) and rounded to fp32.
extern "C" int d2r_obj_read(const char *path, uint32_t *n_vertices, uint32_t *n_triangles, float *vertices, uint32_t *triangles)
{
    if (!path || !n_vertices || !n_triangles) return d2r_fail(nullptr, D2R_ERR_INVALID, "null argument");
    FILE *f = fopen(path, "rb");
    if (!f) return d2r_fail(nullptr, D2R_ERR_INVALID, std::string("cannot open ") + path + " for reading");
    std::string s;
    char chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) s.append(chunk, got);
    const bool read_ok = !ferror(f);
    fclose(f);
    if (!read_ok) return d2r_fail(nullptr, D2R_ERR_INVALID, std::string("cannot read ") + path);
    const uint64_t cap_v = vertices ? *n_vertices : 0, cap_t = triangles ? *n_triangles : 0;
    uint64_t nv = 0, nt = 0, line_no = 0;
    auto bad = [&](const char *what) {
        return d2r_fail(nullptr, D2R_ERR_INVALID, std::string(path) + ", line " + std::to_string(line_no) + ": " + what);
    };
    const char *p = s.c_str(), *end = p + s.size();          // (c_str: NUL-terminated, so strtod and strtol stop at the end)
    while (p < end) {
        ++line_no;
        const char *eol = (const char *)memchr(p, '\n', (size_t)(end - p));
        if (!eol) eol = end;
        const char *q = p;
        while (q < eol && (*q == ' ' || *q == '\t')) ++q;
        if (q + 1 < eol && q[0] == 'v' && (q[1] == ' ' || q[1] == '\t')) {
            q += 2;
            double xyz[3];
            for (int a = 0; a < 3; ++a) {
                char *e;
                xyz[a] = strtod(q, &e);
                if (e == q || e > eol) return bad("a vertex needs three numbers");
                q = e;
            }
            if (nv >= 0xffffffffull) return bad("too many vertices");
            if (vertices) {
                if (nv >= cap_v) return bad("more vertices than the buffer holds");
                for (int a = 0; a < 3; ++a) vertices[3 * nv + a] = (float)xyz[a];
            }
            ++nv;
        } else if (q + 1 < eol && q[0] == 'f' && (q[1] == ' ' || q[1] == '\t')) {
            q += 2;
            uint32_t first = 0, prev = 0;
            int corners = 0;
            for (;;) {
                while (q < eol && (*q == ' ' || *q == '\t' || *q == '\r')) ++q;
                if (q >= eol) break;
                char *e;
                const long long idx = strtoll(q, &e, 10);
                if (e == q || e > eol) return bad("a face corner is not an index");
                q = e;
                while (q < eol && *q != ' ' && *q != '\t' && *q != '\r') ++q;      // the /vt/vn parts
                const long long v = idx > 0 ? idx - 1 : (long long)nv + idx;
                if (idx == 0 || v < 0 || v >= (long long)nv) return bad("a face index is out of range");
                if (corners == 0) first = (uint32_t)v;
                if (corners >= 2) {
                    if (nt >= 0xffffffffull) return bad("too many triangles");
                    if (triangles) {
                        if (nt >= cap_t) return bad("more triangles than the buffer holds");
                        triangles[3 * nt] = first;
                        triangles[3 * nt + 1] = prev;
                        triangles[3 * nt + 2] = (uint32_t)v;
                    }
                    ++nt;
                }
                prev = (uint32_t)v;
                ++corners;
            }
            if (corners < 3) return bad("a face needs three corners");
        }
        p = eol + 1;
    }
    *n_vertices = (uint32_t)nv;
    *n_triangles = (uint32_t)nt;
    return D2R_OK;
}
