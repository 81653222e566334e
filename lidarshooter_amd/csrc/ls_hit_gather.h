// ls_hit_gather.h -- what the gathers over hit records share (device only): k_hit_attributes (ls_attr.hip), k_returns_eval
// (ls_returns.hip), k_hit_attributes_moving + k_returns_eval_moving (ls_attr_moving.hip).  A gather kernel reads: bounds, ray
// (sensor_ray_dir, moving_rays), test (record_on_triangle), and what that kernel does with the result.  The packs of the scan
// frames (ls_sweep.hip, ls_beam.hip) rebuild their points from the same direction.
#pragma once

#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_hit_attr.h"
#include "ls_motion.h"

namespace ls {
namespace {

// LidarDevice.cpp:310-316: d = (sin(theta)cos(phi), sin(theta)sin(phi), cos(theta)) of channel v < V and column h < H
__device__ __forceinline__ void sensor_dir(const SensorTables &tb, uint32_t v, uint32_t h, float *d)
{
    const float st = tb.sin_theta[v], ctv = tb.cos_theta[v];
    const float2 cs = tb.cs_phi[h];
    d[0] = st * cs.x; d[1] = st * cs.y; d[2] = ctv;
}

// the same for ray < V * H of the full raster, with its split into channel and column
__device__ __forceinline__ void sensor_ray_dir(const SensorTables &tb, uint32_t ray, float *d, uint32_t *v, uint32_t *h)
{
    *v = ray / tb.H;
    *h = ray - *v * tb.H;
    sensor_dir(tb, *v, *h, d);
}

// and for q < V * naz of the shard, ascending in the ray index: h is the column of the full raster
__device__ __forceinline__ void shard_ray_dir(const SensorTables &tb, uint32_t q, float *d, uint32_t *v, uint32_t *h)
{
    *v = q / tb.naz;
    *h = tb.az0 + (q - *v * tb.naz);
    sensor_dir(tb, *v, *h, d);
}

// The validity test: whether the ray (o, d) meets the triangle hit.prim names in g -- through the frame's own transform
// (xform_vertex: the bits of k_transform), by hit_attributes_on_triangle (ls_hit_attr.h) -- with t bit-equal to hit.t; a quad tries
// its two triangles in order.  The caller has checked hit.geom and hit.prim < g.n_elems; the three vertex indices are checked
// here, before an address is formed from them.  true: *k the triangle inside the geometry, *t and r9 the test's results.
__device__ __forceinline__ bool record_on_triangle(const AttrGeom &g, uint4 hit, const float *o, const float *d, uint32_t *k, float *t, float *r9)
{
    const uint32_t halves = g.quad ? 2u : 1u;
    bool valid = false;
    for (uint32_t c = 0; c < halves && !valid; ++c) {
        const uint32_t tri = g.quad ? 2u * hit.z + c : hit.z;
        const uint32_t *ix = g.idx + 3 * (size_t)tri;
        const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
        if (i0 >= g.n_verts || i1 >= g.n_verts || i2 >= g.n_verts) continue;
        const V3 a = xform_vertex(g.m, g.verts + (size_t)i0 * g.stride);
        const V3 b = xform_vertex(g.m, g.verts + (size_t)i1 * g.stride);
        const V3 cc = xform_vertex(g.m, g.verts + (size_t)i2 * g.stride);
        const float v0[3] = {a.x, a.y, a.z}, v1[3] = {b.x, b.y, b.z}, v2[3] = {cc.x, cc.y, cc.z};
        if (hit_attributes_on_triangle(o, d, v0, v1, v2, t, r9) && __float_as_uint(*t) == hit.w) {
            *k = tri;
            valid = true;
        }
    }
    return valid;
}

// The ray column h cast with the nominal direction d -- sweep_ray through pose[h], or (0, d) without a pose table --, and the ray
// a geometry with the motion table tab saw -- motion_ray through tab[h], or the cast ray without a table.  p, q: the two records
// as loaded (written only where there is a table), for sweep_point and motion_normal.  false: the seen ray fails
// motion_ray_usable, the walk skipped the geometry there.
__device__ __forceinline__ bool moving_rays(const float *pose, const float *tab, uint32_t h, const float *d, float *p, float *q, float *cast,
                                            float *seen)
{
    cast[0] = 0.f; cast[1] = 0.f; cast[2] = 0.f; cast[3] = 0.f;
    cast[4] = d[0]; cast[5] = d[1]; cast[6] = d[2]; cast[7] = kSweepTmax;
    if (pose) {
        load_pose(pose, h, table_aligned16(pose), p);
        sweep_ray(p, d[0], d[1], d[2], cast);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) seen[j] = cast[j];
    if (!tab) return true;
    load_pose(tab, h, table_aligned16(tab), q);
    motion_ray(q, cast, seen);
    return motion_ray_usable(seen);
}

}  // namespace
}  // namespace ls
