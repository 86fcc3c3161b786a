"""numpy restatement of the TSDF rule — the oracle of tests/test_tsdf_*.py.

The product does not import this module and this module imports nothing from the product.  Every step is fp32 in the
written order (numpy does not contract), so the GPU's blocks, voxels, vertices, triangles, centre and .obj bytes can be
compared bit for bit.
  grid       blocks of 16^3 voxels; voxel g sits at g * voxel; the dense grid spans blocks floor((min - trunc) / (16 voxel))
             .. floor((max + trunc) / (16 voxel)) per axis (fp64 of the fp32 bounds, voxel and trunc)
  mask       eroded by a k x k rectangle anchored at (k // 2, k // 2), outside the frame counts as set
  depth      z = u16 / 1000, valid when the eroded mask holds and 0 < z <= 3
  blocks     per valid pixel, d = (z - trunc) + s voxel for s = 0 .. 2 trunc / voxel; x = ((j - cx) / fx) d, y = ((i - cy) / fy) d;
             world = ((m0 x + m1 y) + m2 d) + m3 per row of cam_pose; voxel floor(world / voxel); block = voxel >> 4
  integrate  voxels of THIS frame's blocks: camera point through inv(cam_pose) = [R^T | -R^T t] (fp64, rounded to fp32), z_cam > 0,
             u = floor(((fx x) / z + cx) + 0.5), v likewise, inside the frame, pixel valid, sdf = z_pixel - z_cam >= -trunc,
             t = min(sdf / trunc, 1), tsdf = (w tsdf + t) / (w + 1), w = w + 1
  surface    cubes with all eight weights >= threshold; inside = tsdf < 0; Bourke's numbering and table; vertex
             p0 + ((p1 - p0) t0) / (t0 - t1); vertices by (z, y, x, axis), triangles by (z, y, x, table order)
  clean-up   inclusive crop (triangle survives when its three vertices do; unreferenced vertices dropped); clusters by shared
             vertices; clusters below 0.02 of the largest dropped, vertices stay; centre = sequential fp64 mean of the vertices
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
BLOCK = 16
DEPTH_MAX = f32(3.0)

# corner c of a cube at (dx, dy, dz); edge e between corners EDGE_CORNERS[e]; edge e = the edge of voxel v + EDGE_OFF[e] along EDGE_AXIS[e]
CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGE_CORNERS = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
EDGE_OFF = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (0, 0, 1), (0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]
EDGE_AXIS = [0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2]

# the 256-case triangle table (Lorensen & Cline; Paul Bourke's numbering), edge triples per case
TRI_TABLE = [
    (),
    (0, 8, 3,),
    (0, 1, 9,),
    (1, 8, 3, 9, 8, 1,),
    (1, 2, 10,),
    (0, 8, 3, 1, 2, 10,),
    (9, 2, 10, 0, 2, 9,),
    (2, 8, 3, 2, 10, 8, 10, 9, 8,),
    (3, 11, 2,),
    (0, 11, 2, 8, 11, 0,),
    (1, 9, 0, 2, 3, 11,),
    (1, 11, 2, 1, 9, 11, 9, 8, 11,),
    (3, 10, 1, 11, 10, 3,),
    (0, 10, 1, 0, 8, 10, 8, 11, 10,),
    (3, 9, 0, 3, 11, 9, 11, 10, 9,),
    (9, 8, 10, 10, 8, 11,),
    (4, 7, 8,),
    (4, 3, 0, 7, 3, 4,),
    (0, 1, 9, 8, 4, 7,),
    (4, 1, 9, 4, 7, 1, 7, 3, 1,),
    (1, 2, 10, 8, 4, 7,),
    (3, 4, 7, 3, 0, 4, 1, 2, 10,),
    (9, 2, 10, 9, 0, 2, 8, 4, 7,),
    (2, 10, 9, 2, 9, 7, 2, 7, 3, 7, 9, 4,),
    (8, 4, 7, 3, 11, 2,),
    (11, 4, 7, 11, 2, 4, 2, 0, 4,),
    (9, 0, 1, 8, 4, 7, 2, 3, 11,),
    (4, 7, 11, 9, 4, 11, 9, 11, 2, 9, 2, 1,),
    (3, 10, 1, 3, 11, 10, 7, 8, 4,),
    (1, 11, 10, 1, 4, 11, 1, 0, 4, 7, 11, 4,),
    (4, 7, 8, 9, 0, 11, 9, 11, 10, 11, 0, 3,),
    (4, 7, 11, 4, 11, 9, 9, 11, 10,),
    (9, 5, 4,),
    (9, 5, 4, 0, 8, 3,),
    (0, 5, 4, 1, 5, 0,),
    (8, 5, 4, 8, 3, 5, 3, 1, 5,),
    (1, 2, 10, 9, 5, 4,),
    (3, 0, 8, 1, 2, 10, 4, 9, 5,),
    (5, 2, 10, 5, 4, 2, 4, 0, 2,),
    (2, 10, 5, 3, 2, 5, 3, 5, 4, 3, 4, 8,),
    (9, 5, 4, 2, 3, 11,),
    (0, 11, 2, 0, 8, 11, 4, 9, 5,),
    (0, 5, 4, 0, 1, 5, 2, 3, 11,),
    (2, 1, 5, 2, 5, 8, 2, 8, 11, 4, 8, 5,),
    (10, 3, 11, 10, 1, 3, 9, 5, 4,),
    (4, 9, 5, 0, 8, 1, 8, 10, 1, 8, 11, 10,),
    (5, 4, 0, 5, 0, 11, 5, 11, 10, 11, 0, 3,),
    (5, 4, 8, 5, 8, 10, 10, 8, 11,),
    (9, 7, 8, 5, 7, 9,),
    (9, 3, 0, 9, 5, 3, 5, 7, 3,),
    (0, 7, 8, 0, 1, 7, 1, 5, 7,),
    (1, 5, 3, 3, 5, 7,),
    (9, 7, 8, 9, 5, 7, 10, 1, 2,),
    (10, 1, 2, 9, 5, 0, 5, 3, 0, 5, 7, 3,),
    (8, 0, 2, 8, 2, 5, 8, 5, 7, 10, 5, 2,),
    (2, 10, 5, 2, 5, 3, 3, 5, 7,),
    (7, 9, 5, 7, 8, 9, 3, 11, 2,),
    (9, 5, 7, 9, 7, 2, 9, 2, 0, 2, 7, 11,),
    (2, 3, 11, 0, 1, 8, 1, 7, 8, 1, 5, 7,),
    (11, 2, 1, 11, 1, 7, 7, 1, 5,),
    (9, 5, 8, 8, 5, 7, 10, 1, 3, 10, 3, 11,),
    (5, 7, 0, 5, 0, 9, 7, 11, 0, 1, 0, 10, 11, 10, 0,),
    (11, 10, 0, 11, 0, 3, 10, 5, 0, 8, 0, 7, 5, 7, 0,),
    (11, 10, 5, 7, 11, 5,),
    (10, 6, 5,),
    (0, 8, 3, 5, 10, 6,),
    (9, 0, 1, 5, 10, 6,),
    (1, 8, 3, 1, 9, 8, 5, 10, 6,),
    (1, 6, 5, 2, 6, 1,),
    (1, 6, 5, 1, 2, 6, 3, 0, 8,),
    (9, 6, 5, 9, 0, 6, 0, 2, 6,),
    (5, 9, 8, 5, 8, 2, 5, 2, 6, 3, 2, 8,),
    (2, 3, 11, 10, 6, 5,),
    (11, 0, 8, 11, 2, 0, 10, 6, 5,),
    (0, 1, 9, 2, 3, 11, 5, 10, 6,),
    (5, 10, 6, 1, 9, 2, 9, 11, 2, 9, 8, 11,),
    (6, 3, 11, 6, 5, 3, 5, 1, 3,),
    (0, 8, 11, 0, 11, 5, 0, 5, 1, 5, 11, 6,),
    (3, 11, 6, 0, 3, 6, 0, 6, 5, 0, 5, 9,),
    (6, 5, 9, 6, 9, 11, 11, 9, 8,),
    (5, 10, 6, 4, 7, 8,),
    (4, 3, 0, 4, 7, 3, 6, 5, 10,),
    (1, 9, 0, 5, 10, 6, 8, 4, 7,),
    (10, 6, 5, 1, 9, 7, 1, 7, 3, 7, 9, 4,),
    (6, 1, 2, 6, 5, 1, 4, 7, 8,),
    (1, 2, 5, 5, 2, 6, 3, 0, 4, 3, 4, 7,),
    (8, 4, 7, 9, 0, 5, 0, 6, 5, 0, 2, 6,),
    (7, 3, 9, 7, 9, 4, 3, 2, 9, 5, 9, 6, 2, 6, 9,),
    (3, 11, 2, 7, 8, 4, 10, 6, 5,),
    (5, 10, 6, 4, 7, 2, 4, 2, 0, 2, 7, 11,),
    (0, 1, 9, 4, 7, 8, 2, 3, 11, 5, 10, 6,),
    (9, 2, 1, 9, 11, 2, 9, 4, 11, 7, 11, 4, 5, 10, 6,),
    (8, 4, 7, 3, 11, 5, 3, 5, 1, 5, 11, 6,),
    (5, 1, 11, 5, 11, 6, 1, 0, 11, 7, 11, 4, 0, 4, 11,),
    (0, 5, 9, 0, 6, 5, 0, 3, 6, 11, 6, 3, 8, 4, 7,),
    (6, 5, 9, 6, 9, 11, 4, 7, 9, 7, 11, 9,),
    (10, 4, 9, 6, 4, 10,),
    (4, 10, 6, 4, 9, 10, 0, 8, 3,),
    (10, 0, 1, 10, 6, 0, 6, 4, 0,),
    (8, 3, 1, 8, 1, 6, 8, 6, 4, 6, 1, 10,),
    (1, 4, 9, 1, 2, 4, 2, 6, 4,),
    (3, 0, 8, 1, 2, 9, 2, 4, 9, 2, 6, 4,),
    (0, 2, 4, 4, 2, 6,),
    (8, 3, 2, 8, 2, 4, 4, 2, 6,),
    (10, 4, 9, 10, 6, 4, 11, 2, 3,),
    (0, 8, 2, 2, 8, 11, 4, 9, 10, 4, 10, 6,),
    (3, 11, 2, 0, 1, 6, 0, 6, 4, 6, 1, 10,),
    (6, 4, 1, 6, 1, 10, 4, 8, 1, 2, 1, 11, 8, 11, 1,),
    (9, 6, 4, 9, 3, 6, 9, 1, 3, 11, 6, 3,),
    (8, 11, 1, 8, 1, 0, 11, 6, 1, 9, 1, 4, 6, 4, 1,),
    (3, 11, 6, 3, 6, 0, 0, 6, 4,),
    (6, 4, 8, 11, 6, 8,),
    (7, 10, 6, 7, 8, 10, 8, 9, 10,),
    (0, 7, 3, 0, 10, 7, 0, 9, 10, 6, 7, 10,),
    (10, 6, 7, 1, 10, 7, 1, 7, 8, 1, 8, 0,),
    (10, 6, 7, 10, 7, 1, 1, 7, 3,),
    (1, 2, 6, 1, 6, 8, 1, 8, 9, 8, 6, 7,),
    (2, 6, 9, 2, 9, 1, 6, 7, 9, 0, 9, 3, 7, 3, 9,),
    (7, 8, 0, 7, 0, 6, 6, 0, 2,),
    (7, 3, 2, 6, 7, 2,),
    (2, 3, 11, 10, 6, 8, 10, 8, 9, 8, 6, 7,),
    (2, 0, 7, 2, 7, 11, 0, 9, 7, 6, 7, 10, 9, 10, 7,),
    (1, 8, 0, 1, 7, 8, 1, 10, 7, 6, 7, 10, 2, 3, 11,),
    (11, 2, 1, 11, 1, 7, 10, 6, 1, 6, 7, 1,),
    (8, 9, 6, 8, 6, 7, 9, 1, 6, 11, 6, 3, 1, 3, 6,),
    (0, 9, 1, 11, 6, 7,),
    (7, 8, 0, 7, 0, 6, 3, 11, 0, 11, 6, 0,),
    (7, 11, 6,),
    (7, 6, 11,),
    (3, 0, 8, 11, 7, 6,),
    (0, 1, 9, 11, 7, 6,),
    (8, 1, 9, 8, 3, 1, 11, 7, 6,),
    (10, 1, 2, 6, 11, 7,),
    (1, 2, 10, 3, 0, 8, 6, 11, 7,),
    (2, 9, 0, 2, 10, 9, 6, 11, 7,),
    (6, 11, 7, 2, 10, 3, 10, 8, 3, 10, 9, 8,),
    (7, 2, 3, 6, 2, 7,),
    (7, 0, 8, 7, 6, 0, 6, 2, 0,),
    (2, 7, 6, 2, 3, 7, 0, 1, 9,),
    (1, 6, 2, 1, 8, 6, 1, 9, 8, 8, 7, 6,),
    (10, 7, 6, 10, 1, 7, 1, 3, 7,),
    (10, 7, 6, 1, 7, 10, 1, 8, 7, 1, 0, 8,),
    (0, 3, 7, 0, 7, 10, 0, 10, 9, 6, 10, 7,),
    (7, 6, 10, 7, 10, 8, 8, 10, 9,),
    (6, 8, 4, 11, 8, 6,),
    (3, 6, 11, 3, 0, 6, 0, 4, 6,),
    (8, 6, 11, 8, 4, 6, 9, 0, 1,),
    (9, 4, 6, 9, 6, 3, 9, 3, 1, 11, 3, 6,),
    (6, 8, 4, 6, 11, 8, 2, 10, 1,),
    (1, 2, 10, 3, 0, 11, 0, 6, 11, 0, 4, 6,),
    (4, 11, 8, 4, 6, 11, 0, 2, 9, 2, 10, 9,),
    (10, 9, 3, 10, 3, 2, 9, 4, 3, 11, 3, 6, 4, 6, 3,),
    (8, 2, 3, 8, 4, 2, 4, 6, 2,),
    (0, 4, 2, 4, 6, 2,),
    (1, 9, 0, 2, 3, 4, 2, 4, 6, 4, 3, 8,),
    (1, 9, 4, 1, 4, 2, 2, 4, 6,),
    (8, 1, 3, 8, 6, 1, 8, 4, 6, 6, 10, 1,),
    (10, 1, 0, 10, 0, 6, 6, 0, 4,),
    (4, 6, 3, 4, 3, 8, 6, 10, 3, 0, 3, 9, 10, 9, 3,),
    (10, 9, 4, 6, 10, 4,),
    (4, 9, 5, 7, 6, 11,),
    (0, 8, 3, 4, 9, 5, 11, 7, 6,),
    (5, 0, 1, 5, 4, 0, 7, 6, 11,),
    (11, 7, 6, 8, 3, 4, 3, 5, 4, 3, 1, 5,),
    (9, 5, 4, 10, 1, 2, 7, 6, 11,),
    (6, 11, 7, 1, 2, 10, 0, 8, 3, 4, 9, 5,),
    (7, 6, 11, 5, 4, 10, 4, 2, 10, 4, 0, 2,),
    (3, 4, 8, 3, 5, 4, 3, 2, 5, 10, 5, 2, 11, 7, 6,),
    (7, 2, 3, 7, 6, 2, 5, 4, 9,),
    (9, 5, 4, 0, 8, 6, 0, 6, 2, 6, 8, 7,),
    (3, 6, 2, 3, 7, 6, 1, 5, 0, 5, 4, 0,),
    (6, 2, 8, 6, 8, 7, 2, 1, 8, 4, 8, 5, 1, 5, 8,),
    (9, 5, 4, 10, 1, 6, 1, 7, 6, 1, 3, 7,),
    (1, 6, 10, 1, 7, 6, 1, 0, 7, 8, 7, 0, 9, 5, 4,),
    (4, 0, 10, 4, 10, 5, 0, 3, 10, 6, 10, 7, 3, 7, 10,),
    (7, 6, 10, 7, 10, 8, 5, 4, 10, 4, 8, 10,),
    (6, 9, 5, 6, 11, 9, 11, 8, 9,),
    (3, 6, 11, 0, 6, 3, 0, 5, 6, 0, 9, 5,),
    (0, 11, 8, 0, 5, 11, 0, 1, 5, 5, 6, 11,),
    (6, 11, 3, 6, 3, 5, 5, 3, 1,),
    (1, 2, 10, 9, 5, 11, 9, 11, 8, 11, 5, 6,),
    (0, 11, 3, 0, 6, 11, 0, 9, 6, 5, 6, 9, 1, 2, 10,),
    (11, 8, 5, 11, 5, 6, 8, 0, 5, 10, 5, 2, 0, 2, 5,),
    (6, 11, 3, 6, 3, 5, 2, 10, 3, 10, 5, 3,),
    (5, 8, 9, 5, 2, 8, 5, 6, 2, 3, 8, 2,),
    (9, 5, 6, 9, 6, 0, 0, 6, 2,),
    (1, 5, 8, 1, 8, 0, 5, 6, 8, 3, 8, 2, 6, 2, 8,),
    (1, 5, 6, 2, 1, 6,),
    (1, 3, 6, 1, 6, 10, 3, 8, 6, 5, 6, 9, 8, 9, 6,),
    (10, 1, 0, 10, 0, 6, 9, 5, 0, 5, 6, 0,),
    (0, 3, 8, 5, 6, 10,),
    (10, 5, 6,),
    (11, 5, 10, 7, 5, 11,),
    (11, 5, 10, 11, 7, 5, 8, 3, 0,),
    (5, 11, 7, 5, 10, 11, 1, 9, 0,),
    (10, 7, 5, 10, 11, 7, 9, 8, 1, 8, 3, 1,),
    (11, 1, 2, 11, 7, 1, 7, 5, 1,),
    (0, 8, 3, 1, 2, 7, 1, 7, 5, 7, 2, 11,),
    (9, 7, 5, 9, 2, 7, 9, 0, 2, 2, 11, 7,),
    (7, 5, 2, 7, 2, 11, 5, 9, 2, 3, 2, 8, 9, 8, 2,),
    (2, 5, 10, 2, 3, 5, 3, 7, 5,),
    (8, 2, 0, 8, 5, 2, 8, 7, 5, 10, 2, 5,),
    (9, 0, 1, 5, 10, 3, 5, 3, 7, 3, 10, 2,),
    (9, 8, 2, 9, 2, 1, 8, 7, 2, 10, 2, 5, 7, 5, 2,),
    (1, 3, 5, 3, 7, 5,),
    (0, 8, 7, 0, 7, 1, 1, 7, 5,),
    (9, 0, 3, 9, 3, 5, 5, 3, 7,),
    (9, 8, 7, 5, 9, 7,),
    (5, 8, 4, 5, 10, 8, 10, 11, 8,),
    (5, 0, 4, 5, 11, 0, 5, 10, 11, 11, 3, 0,),
    (0, 1, 9, 8, 4, 10, 8, 10, 11, 10, 4, 5,),
    (10, 11, 4, 10, 4, 5, 11, 3, 4, 9, 4, 1, 3, 1, 4,),
    (2, 5, 1, 2, 8, 5, 2, 11, 8, 4, 5, 8,),
    (0, 4, 11, 0, 11, 3, 4, 5, 11, 2, 11, 1, 5, 1, 11,),
    (0, 2, 5, 0, 5, 9, 2, 11, 5, 4, 5, 8, 11, 8, 5,),
    (9, 4, 5, 2, 11, 3,),
    (2, 5, 10, 3, 5, 2, 3, 4, 5, 3, 8, 4,),
    (5, 10, 2, 5, 2, 4, 4, 2, 0,),
    (3, 10, 2, 3, 5, 10, 3, 8, 5, 4, 5, 8, 0, 1, 9,),
    (5, 10, 2, 5, 2, 4, 1, 9, 2, 9, 4, 2,),
    (8, 4, 5, 8, 5, 3, 3, 5, 1,),
    (0, 4, 5, 1, 0, 5,),
    (8, 4, 5, 8, 5, 3, 9, 0, 5, 0, 3, 5,),
    (9, 4, 5,),
    (4, 11, 7, 4, 9, 11, 9, 10, 11,),
    (0, 8, 3, 4, 9, 7, 9, 11, 7, 9, 10, 11,),
    (1, 10, 11, 1, 11, 4, 1, 4, 0, 7, 4, 11,),
    (3, 1, 4, 3, 4, 8, 1, 10, 4, 7, 4, 11, 10, 11, 4,),
    (4, 11, 7, 9, 11, 4, 9, 2, 11, 9, 1, 2,),
    (9, 7, 4, 9, 11, 7, 9, 1, 11, 2, 11, 1, 0, 8, 3,),
    (11, 7, 4, 11, 4, 2, 2, 4, 0,),
    (11, 7, 4, 11, 4, 2, 8, 3, 4, 3, 2, 4,),
    (2, 9, 10, 2, 7, 9, 2, 3, 7, 7, 4, 9,),
    (9, 10, 7, 9, 7, 4, 10, 2, 7, 8, 7, 0, 2, 0, 7,),
    (3, 7, 10, 3, 10, 2, 7, 4, 10, 1, 10, 0, 4, 0, 10,),
    (1, 10, 2, 8, 7, 4,),
    (4, 9, 1, 4, 1, 7, 7, 1, 3,),
    (4, 9, 1, 4, 1, 7, 0, 8, 1, 8, 7, 1,),
    (4, 0, 3, 7, 4, 3,),
    (4, 8, 7,),
    (9, 10, 8, 10, 11, 8,),
    (3, 0, 9, 3, 9, 11, 11, 9, 10,),
    (0, 1, 10, 0, 10, 8, 8, 10, 11,),
    (3, 1, 10, 11, 3, 10,),
    (1, 2, 11, 1, 11, 9, 9, 11, 8,),
    (3, 0, 9, 3, 9, 11, 1, 2, 9, 2, 11, 9,),
    (0, 2, 11, 8, 0, 11,),
    (3, 2, 11,),
    (2, 3, 8, 2, 8, 10, 10, 8, 9,),
    (9, 10, 2, 0, 9, 2,),
    (2, 3, 8, 2, 8, 10, 0, 1, 8, 1, 10, 8,),
    (1, 10, 2,),
    (1, 3, 8, 9, 1, 8,),
    (0, 9, 1,),
    (0, 3, 8,),
    (),
]


# Wrong rules, one name each: Volume(..., rules={name}) restates the rule with that one departure, so that a test can show that its
# cases tell the two apart (tests/test_tsdf_edges_host.py).  ("swap_row", r) is given to Volume.triangles() directly.
WRONG_RULES = ("anchor_low", "border_unset", "z_lt_3", "sdf_le", "zc_ge_0", "rint", "steps_floor", "inside_le", "seven_of_eight",
               "other_end", "inv_fp32")


def erode(mask, k: int, anchor=None, border=True):
    """cv2.erode(mask, ones((k, k))) with cv2's anchor (k // 2, k // 2) and border rule, written as a direct window minimum.
    `anchor` and `border` (what a pixel outside the frame counts as) are the rule's; other values restate wrong rules."""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    a = k // 2 if anchor is None else anchor
    p = np.full((H + k - 1, W + k - 1), bool(border))
    p[a:a + H, a:a + W] = m
    out = np.ones((H, W), bool)
    for di in range(k):
        for dj in range(k):
            out &= p[di:di + H, dj:dj + W]
    return out


def rigid_inverse34(T, dtype=np.float64):
    T = np.asarray(T, np.float32).astype(dtype).reshape(4, 4)
    out = np.zeros((3, 4), dtype)
    for i in range(3):
        for j in range(3):
            out[i, j] = T[j, i]
        out[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    return out.astype(np.float32)


# ---------------------------------------------------------------------------------------------------- a point meets a volume
# csrc/tsdf_sample.h restated; tests/tsdfvis_ref.py and tests/camtrack_ref.py build on these two.

def cell(p, voxel, clo, chi):
    """ts_cell's arithmetic: p float32 [n,3], voxel float32, clo / chi int [3] (global voxel indices, x y z) -> (inside bool [n,3]: per
    axis clo <= c <= chi, NaN and the infinities fail; c float32 [n,3] = floor(p / voxel); fractions float32 [n,3] = p / voxel - c)."""
    with np.errstate(all="ignore"):
        g = np.asarray(p, np.float32) / f32(voxel)
        c = np.floor(g)
        fr = (g - c).astype(np.float32)
        inside = np.stack([(c[:, a] >= f32(clo[a])) & (c[:, a] <= f32(chi[a])) for a in range(3)], 1)
    return inside, c, fr


def lerp3_grad(t, fr):
    """ts_lerp3_grad: t the eight corners (k = x + 2 y + 4 z; [n] each, or [n,ch]), fr float32 [n,3] -> (value, (gx, gy, gz)): along
    x, then y, then z, each step a + f (b - a); the gradient is the derivative of that interpolant by each fraction."""
    f0, f1, f2 = (fr[:, a] if t[0].ndim == 1 else fr[:, a:a + 1] for a in range(3))
    with np.errstate(all="ignore"):
        e00, e10, e01, e11 = t[1] - t[0], t[3] - t[2], t[5] - t[4], t[7] - t[6]
        x00, x10, x01, x11 = t[0] + f0 * e00, t[2] + f0 * e10, t[4] + f0 * e01, t[6] + f0 * e11
        d0, d1 = x10 - x00, x11 - x01
        y0, y1 = x00 + f1 * d0, x01 + f1 * d1
        gz = y1 - y0
        gy = d0 + f2 * (d1 - d0)
        ey0, ey1 = e00 + f1 * (e10 - e00), e01 + f1 * (e11 - e01)
        gx = ey0 + f2 * (ey1 - ey0)
        return y0 + f2 * gz, (gx, gy, gz)


def lerp3(t, fr):
    return lerp3_grad(t, fr)[0]


class Volume:
    def __init__(self, bounds, voxel=0.002, trunc=None, rules=(), probe=False):
        """rules: names from WRONG_RULES (default: the rule as written).  probe: record in self.probe what the rule touches on
        its way: per frame the pixels a voxel update read and the number of blocks stamped, band samples that left the grid per
        face, camera depths met in stamped blocks, and the marching cubes' per-cube table rows."""
        self.rules = frozenset(rules)
        assert self.rules <= set(WRONG_RULES), self.rules
        self.probe = dict(pixels_read=[], frame_blocks=[], steps_outside=np.zeros((3, 2), np.int64), zc_nonpositive=0, zc_zero=0, zc_tiny=0) if probe else None
        self.voxel = f32(voxel)
        self.trunc = f32(8) * self.voxel if trunc is None else f32(trunc)
        b = np.asarray(bounds, np.float64).reshape(2, 3).astype(np.float32).astype(np.float64)
        bs = BLOCK * float(self.voxel)
        self.b0 = np.floor((b[0] - float(self.trunc)) / bs).astype(np.int64)
        b1 = np.floor((b[1] + float(self.trunc)) / bs).astype(np.int64)
        self.nb = b1 - self.b0 + 1                       # blocks per axis (x, y, z)
        self.nv = self.nb * BLOCK
        nx, ny, nz = (int(v) for v in self.nv)
        self.tsdf = np.zeros((nz, ny, nx), np.float32)
        self.w = np.zeros((nz, ny, nx), np.float32)
        self.ever = np.zeros((int(self.nb[2]), int(self.nb[1]), int(self.nb[0])), bool)
        self.steps = int(round(float(self.trunc) / float(self.voxel)))
        if "steps_floor" in self.rules:
            self.steps = int(np.floor(float(self.trunc) / float(self.voxel)))
        self.frames_used = 0

    # ------------------------------------------------------------------------------------------------ frames
    def valid_depth(self, depth_u16, mask, erode_k):
        z = np.asarray(depth_u16, np.uint16).astype(np.float32) / f32(1000)
        eroded = erode(mask, erode_k, (erode_k - 1) // 2 if "anchor_low" in self.rules else None, "border_unset" not in self.rules)
        ok = eroded & (z > 0) & ((z < DEPTH_MAX) if "z_lt_3" in self.rules else (z <= DEPTH_MAX))
        return np.where(ok, z, f32(0)).astype(np.float32)

    def frame_blocks(self, zbuf, intrinsics, cam_pose):
        """-> bool [nbz, nby, nbx]: the blocks of this frame."""
        K = np.asarray(intrinsics, np.float64).reshape(3, 3).astype(np.float32)
        M = np.asarray(cam_pose, np.float64).reshape(4, 4).astype(np.float32)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        ii, jj = np.nonzero(zbuf > 0)
        z = zbuf[ii, jj]
        xn = (jj.astype(np.float32) - cx) / fx
        yn = (ii.astype(np.float32) - cy) / fy
        out = np.zeros(self.ever.shape, bool)
        lo = self.b0 * BLOCK
        hi = (self.b0 + self.nb) * BLOCK
        for s in range(2 * self.steps + 1):
            d = (z - self.trunc) + f32(s) * self.voxel
            x, y = xn * d, yn * d
            g = [np.floor((((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * d) + M[r, 3]) / self.voxel) for r in range(3)]
            ok = np.ones(len(z), bool)
            for a in range(3):
                ok &= (g[a] >= lo[a]) & (g[a] < hi[a])
                if self.probe is not None:
                    self.probe["steps_outside"][a] += [int((g[a] < lo[a]).sum()), int((g[a] >= hi[a]).sum())]
            b = [(g[a][ok].astype(np.int64) >> 4) - self.b0[a] for a in range(3)]
            out[b[2], b[1], b[0]] = True
        return out

    def integrate(self, depth_u16, mask, intrinsics, cam_pose, erode_k):
        zbuf = self.valid_depth(depth_u16, mask, erode_k)
        if not (zbuf > 0).any():
            return False                                   # the reference's `except RuntimeError: pass`
        self.frames_used += 1
        H, W = zbuf.shape
        blocks = self.frame_blocks(zbuf, intrinsics, cam_pose)
        self.ever |= blocks
        K = np.asarray(intrinsics, np.float64).reshape(3, 3).astype(np.float32)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        Mi = rigid_inverse34(np.asarray(cam_pose, np.float64).reshape(4, 4).astype(np.float32), np.float32 if "inv_fp32" in self.rules else np.float64)
        bz, by, bx = np.nonzero(blocks)
        if self.probe is not None:
            self.probe["frame_blocks"].append(len(bz))
            self.probe["pixels_read"].append(np.zeros((H, W), bool))
        o = np.arange(BLOCK)
        for k0 in range(0, len(bz), 512):
            sl = slice(k0, k0 + 512)
            lz = (bz[sl, None] * BLOCK + o)[:, :, None, None]          # local voxel indices, [n,16,1,1] etc.
            ly = (by[sl, None] * BLOCK + o)[:, None, :, None]
            lx = (bx[sl, None] * BLOCK + o)[:, None, None, :]
            lz, ly, lx = np.broadcast_arrays(lz, ly, lx)
            px = (lx + self.b0[0] * BLOCK).astype(np.float32) * self.voxel
            py = (ly + self.b0[1] * BLOCK).astype(np.float32) * self.voxel
            pz = (lz + self.b0[2] * BLOCK).astype(np.float32) * self.voxel
            xc, yc, zc = (((Mi[r, 0] * px + Mi[r, 1] * py) + Mi[r, 2] * pz) + Mi[r, 3] for r in range(3))
            ok = (zc >= 0) if "zc_ge_0" in self.rules else (zc > 0)
            if self.probe is not None:
                self.probe["zc_nonpositive"] += int((zc <= 0).sum())
                self.probe["zc_zero"] += int((zc == 0).sum())
                self.probe["zc_tiny"] += int(((zc > 0) & (zc < self.voxel / f32(4))).sum())
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                if "rint" in self.rules:
                    u, v = np.rint((fx * xc) / zc + cx), np.rint((fy * yc) / zc + cy)
                else:
                    u = np.floor(((fx * xc) / zc + cx) + f32(0.5))
                    v = np.floor(((fy * yc) / zc + cy) + f32(0.5))
            ok &= (u >= 0) & (u < f32(W)) & (v >= 0) & (v < f32(H))
            ui = np.where(ok, u, 0).astype(np.int64)
            vi = np.where(ok, v, 0).astype(np.int64)
            zp = zbuf[vi, ui]
            ok &= zp > 0
            sdf = zp - zc
            ok &= ~((sdf <= -self.trunc) if "sdf_le" in self.rules else (sdf < -self.trunc))
            if self.probe is not None:
                self.probe["pixels_read"][-1][vi[ok], ui[ok]] = True
            t = np.minimum(sdf / self.trunc, f32(1))
            iz, iy, ix = lz[ok], ly[ok], lx[ok]
            w0, t0 = self.w[iz, iy, ix], self.tsdf[iz, iy, ix]
            self.tsdf[iz, iy, ix] = (w0 * t0 + t[ok]) / (w0 + f32(1))
            self.w[iz, iy, ix] = w0 + f32(1)
        return True

    def active_blocks(self):
        """-> int64 [n,3] global block coordinates (x, y, z) in (z, y, x) order."""
        bz, by, bx = np.nonzero(self.ever)
        return np.stack([bx + self.b0[0], by + self.b0[1], bz + self.b0[2]], 1)

    def block_voxels(self):
        """-> (tsdf, w) float32 [n,16,16,16] of the active blocks, indexed [z][y][x]."""
        bz, by, bx = np.nonzero(self.ever)
        T = np.stack([self.tsdf[z * 16:z * 16 + 16, y * 16:y * 16 + 16, x * 16:x * 16 + 16] for z, y, x in zip(bz, by, bx)]) if len(bz) else np.zeros((0, 16, 16, 16), np.float32)
        Wt = np.stack([self.w[z * 16:z * 16 + 16, y * 16:y * 16 + 16, x * 16:x * 16 + 16] for z, y, x in zip(bz, by, bx)]) if len(bz) else np.zeros((0, 16, 16, 16), np.float32)
        return T, Wt

    # ------------------------------------------------------------------------------------------------ surface
    def marching_cubes(self, weight_threshold=3.0):
        """-> (vertices float32 [nv,3], triangles int64 [nt,3]) in canonical order."""
        T, Wt = self.tsdf, self.w
        nz, ny, nx = T.shape
        enough = Wt >= f32(weight_threshold)
        inside = (T <= 0) if "inside_le" in self.rules else (T < 0)
        sl = lambda d, n: slice(d, n - 1 + d)
        passed = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
        case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
        for c, (dx, dy, dz) in enumerate(CORNERS):
            s = (sl(dz, nz), sl(dy, ny), sl(dx, nx))
            passed += enough[s]
            case |= inside[s].astype(np.int64) << c
        case[passed < (7 if "seven_of_eight" in self.rules else 8)] = 0
        case[case == 255] = 0
        cube = np.zeros((nz, ny, nx), np.int64)
        cube[:-1, :-1, :-1] = case
        # edge (v, axis) carries a vertex when its ends differ in sign and one of the four cubes around it is kept
        present = np.zeros((nz, ny, nx, 3), bool)
        kept = cube != 0
        for a in range(3):
            ax = 2 - a                                     # array axis of coordinate a (arrays are [z][y][x])
            near = kept.copy()
            for other in (b for b in range(3) if b != a):
                sh = np.zeros_like(near)
                dst = [slice(None)] * 3
                src = [slice(None)] * 3
                dst[2 - other] = slice(1, None)
                src[2 - other] = slice(0, -1)
                sh[tuple(dst)] = near[tuple(src)]
                near = near | sh
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[ax] = slice(0, -1)
            hi[ax] = slice(1, None)
            cross = np.zeros((nz, ny, nx), bool)
            cross[tuple(lo)] = inside[tuple(lo)] != inside[tuple(hi)]
            present[..., a] = cross & near
        flat = present.reshape(-1)
        vid = np.cumsum(flat) - 1                          # (z, y, x, axis) order
        vid = vid.reshape(nz, ny, nx, 3)
        z, y, x, a = np.nonzero(present)
        g = [x, y, z]
        p0 = [(g[k] + self.b0[k] * BLOCK).astype(np.float32) * self.voxel for k in range(3)]
        n = [x + (a == 0), y + (a == 1), z + (a == 2)]
        t0, t1 = T[z, y, x], T[n[2], n[1], n[0]]
        verts = np.stack(p0, 1)
        for k in range(3):
            m = a == k
            q1 = (g[k][m] + 1 + self.b0[k] * BLOCK).astype(np.float32) * self.voxel
            with np.errstate(invalid="ignore", divide="ignore"):
                if "other_end" in self.rules:
                    verts[m, k] = q1 + ((p0[k][m] - q1) * t1[m]) / (t1[m] - t0[m])
                else:
                    verts[m, k] = p0[k][m] + ((q1 - p0[k][m]) * t0[m]) / (t0[m] - t1[m])
        if self.probe is not None:
            self.probe["cube"], self.probe["vid"] = cube, vid
        return verts.astype(np.float32), self.triangles(cube, vid)

    @staticmethod
    def triangles(cube, vid, swap_row=None):
        """The triangles of the cubes `cube` (table row per voxel, 0: none) as indices `vid` [nz, ny, nx, 3] of their edges' vertices.
        swap_row: a wrong table, that row's first triangle with its first two indices exchanged."""
        tris = []
        cz, cy, cx = np.nonzero(cube)
        for zz, yy, xx in zip(cz, cy, cx):
            row = TRI_TABLE[cube[zz, yy, xx]]
            if cube[zz, yy, xx] == swap_row:
                row = (row[1], row[0]) + row[2:]
            for k in range(0, len(row), 3):
                tris.append([vid[zz + EDGE_OFF[e][2], yy + EDGE_OFF[e][1], xx + EDGE_OFF[e][0], EDGE_AXIS[e]] for e in row[k:k + 3]])
        return np.asarray(tris, np.int64).reshape(-1, 3)


def clean(verts, tris, crop=None, keep_frac=0.02):
    """-> dict(vertices, triangles, clusters, keep, centre) as d2r_tsdf_extract returns them."""
    verts = np.asarray(verts, np.float32)
    tris = np.asarray(tris, np.int64)
    inside = np.ones(len(verts), bool)
    if crop is not None:
        c = np.asarray(crop, np.float64).reshape(2, 3).astype(np.float32)
        inside = np.all((verts >= c[0]) & (verts <= c[1]), axis=1)
    tk = inside[tris].all(axis=1)
    tris = tris[tk]
    used = np.zeros(len(verts), bool)
    used[tris.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    verts = verts[used]
    tris = remap[tris]
    parent = np.arange(len(verts))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b, c in tris:
        for p, q in ((a, b), (a, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    roots = np.array([find(t[0]) for t in tris], np.int64)
    labels = np.zeros(len(tris), np.int64)
    seen = {}
    for k, r in enumerate(roots):
        labels[k] = seen.setdefault(int(r), len(seen))
    sizes = np.bincount(labels, minlength=len(seen))
    keep = ~(sizes[labels].astype(np.float64) < keep_frac * float(sizes.max())) if len(tris) else np.zeros(0, bool)
    centre = np.add.accumulate(verts.astype(np.float64), axis=0)[-1] / len(verts) if len(verts) else np.zeros(3)
    return dict(vertices=verts, triangles=tris, clusters=labels, keep=keep, centre=centre)


def obj_bytes(verts, tris, keep=None) -> bytes:
    lines = ["v %f %f %f\n" % (float(v[0]), float(v[1]), float(v[2])) for v in verts]
    lines += ["f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1) for k, t in enumerate(tris) if keep is None or keep[k]]
    return "".join(lines).encode()


def fuse(depths, cam_poses, intrinsics, masks, obj_id, bounds, frame_range=None):
    """The per-object loop of get_phys_models' TSDF branch: -> (Volume, raw vertices, raw triangles, cleaned dict)."""
    vol = Volume(bounds)
    for f in (range(len(depths)) if frame_range is None else frame_range):
        u16 = (np.asarray(depths[f]) * 1000).astype(np.uint16)
        vol.integrate(u16, np.asarray(masks[f]) == obj_id, intrinsics, cam_poses[f], 20 if obj_id == 0 else 8)
    v, t = vol.marching_cubes(3.0)
    return vol, v, t, (clean(v, t, bounds, 0.02) if len(t) else None)
