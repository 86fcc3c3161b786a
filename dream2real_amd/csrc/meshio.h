// meshio.h — host-side clean-up of an extracted triangle mesh and the Wavefront .obj writer (meshio.cpp)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

struct D2rMesh {
    std::vector<float> verts;        // [nv][3]
    std::vector<uint32_t> tris;      // [nt][3], every triangle that survived the crop
    std::vector<int32_t> label;      // [nt] connected cluster, numbered by first appearance
    std::vector<uint8_t> keep;       // [nt] 0 = in a cluster smaller than keep_frac * the largest
    double centre[3] = {0, 0, 0};    // mean of verts, summed in order in fp64
    uint32_t n_clusters = 0;
};

// crop (6 floats: min xyz, max xyz, inclusive; nullptr = none) -> triangles with all three vertices inside, vertices that
// no surviving triangle references dropped, order kept; clusters by shared vertices; keep mask; centre
void d2r_mesh_clean(const float *verts, size_t nv, const uint32_t *tris, size_t nt, const float *crop, double keep_frac, D2rMesh &out);
