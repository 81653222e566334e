// ls_scene_tris.h -- the committed scene as one flat list of triangles, which ls_scene_grid, ls_scene_distance_grid and
// ls_sample_surface run over.  Host: scene_tris_prepare (ls_internal.h; ls_gather.cpp) brings the gathers'
// per-geomID table up to date and, next to it, tri_first[0 .. n_table]: where each geomID's triangles start in the flat index (a
// free id: none; a quad geometry: 2 n_elems), the total n_tris behind them -- uploaded only when they differ from what the device
// holds, whichever query asks first after a commit.  Device, below: the geometry of a flat index, and a triangle's three vertices
// through the frame's transform (xform_vertex) and the call's.
#pragma once

#include <stdint.h>

#include "ls_kernels.h"

#if defined(__HIPCC__)
#include "ls_device.h"

namespace ls {

// the geometry whose slice of the flat index holds i < n_tris: the last one with tri_first[gid] <= i (tri_first[0] = 0,
// tri_first[n_table] = n_tris > i)
__device__ __forceinline__ uint32_t scene_geom_of(const uint32_t *__restrict__ tri_first, uint32_t n_table, uint32_t i)
{
    uint32_t lo = 0u, hi = n_table;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tri_first[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// a sensor-frame vertex in the call's frame: ls_cloud_to_world's products and sums in its order
__device__ __forceinline__ void scene_vertex_to_grid(const float *m, float &x, float &y, float &z)
{
    const float a = x, b = y, c = z;
    x = ((m[0] * a + m[1] * b) + m[2] * c) + m[3];
    y = ((m[4] * a + m[5] * b) + m[6] * c) + m[7];
    z = ((m[8] * a + m[9] * b) + m[10] * c) + m[11];
}

// Triangle `tri` of geometry ge (both in range of the table) in the sensor's frame, or with has_xf through xf (row-major 3 x 4) in
// the call's.  The three indices are checked against the vertex count before an address is formed from them.  false: no such
// geometry or an index out of range
__device__ __forceinline__ bool scene_tri_vertices(bool has_xf, const float *xf, const AttrGeom &ge, uint32_t tri, V3 &a, V3 &b, V3 &c)
{
    if (ge.verts == nullptr) return false;
    const uint32_t i0 = ge.idx[3 * (size_t)tri], i1 = ge.idx[3 * (size_t)tri + 1], i2 = ge.idx[3 * (size_t)tri + 2];
    if (!(i0 < ge.n_verts && i1 < ge.n_verts && i2 < ge.n_verts)) return false;
    a = xform_vertex(ge.m, ge.verts + (size_t)i0 * ge.stride);
    b = xform_vertex(ge.m, ge.verts + (size_t)i1 * ge.stride);
    c = xform_vertex(ge.m, ge.verts + (size_t)i2 * ge.stride);
    if (has_xf) {
        scene_vertex_to_grid(xf, a.x, a.y, a.z);
        scene_vertex_to_grid(xf, b.x, b.y, b.z);
        scene_vertex_to_grid(xf, c.x, c.y, c.z);
    }
    return true;
}

}  // namespace ls
#endif
