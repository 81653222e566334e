// ls_attr.hip -- k_hit_attributes: surface attributes of hit records (ls_hit_attributes, include/lidarshooter_hip.h;
// DESIGN.md 3.3.3): per ls_hit the unit geometric normal, the incidence cosine, Embree's barycentrics, the triangle inside
// the geometry (which half of a quad), the hit point.
//
// No hierarchy, no walk: a gather, one lane per record.  Per lane 16 bytes of hit, the ray (two 16-byte loads of the caller's
// record, or the handle's factor-table entries for a sensor ray), the geometry's entry of the per-geomID table (AttrGeom, 128
// bytes; lanes of a wave mostly share it: frame hits come in ray order), three indices, three vertex records of the
// geometry's stride -- then the frame's own transform (xform_vertex: the bits of k_transform) and hit_attributes_on_triangle
// (ls_hit_attr.h, the arithmetic ls_debug_hit_attributes_on_triangle runs on the host), and three 16-byte stores.
// A record is valid when the exact test from the ray's origin passes on the named triangle with t bit-equal to hit.t; a quad
// tries its two triangles in order.  Every index is checked against its bound before an address is formed from it: the
// ray, the geometry id and the element here, the three vertex indices in record_on_triangle (ls_hit_gather.h, the test all four
// gathers run; the sensor ray's direction: sensor_ray_dir, there too).  Anything else: flags = 0, zeros, the ray index echoed.
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_hit_attr.h"
#include "ls_hit_gather.h"

namespace ls {

namespace {

__global__ __launch_bounds__(kBlock) void k_hit_attributes(const uint4 *__restrict__ hits, const uint32_t *__restrict__ d_count, uint32_t n,
                                                           const float4 *__restrict__ rays, uint32_t n_rays, SensorTables tb,
                                                           const AttrGeom *__restrict__ table, uint32_t n_table, uint4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t count = d_count ? min(n, *d_count) : n;
    if (i >= count) return;
    const uint4 h = hits[i];   // (ray, geom, prim, t bits)
    const uint32_t ray_bound = rays ? n_rays : tb.V * tb.H;
    float res[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t tri = 0, flags = 0;
    if (h.x < ray_bound && h.y < n_table) {
        const AttrGeom &g = table[h.y];
        if (g.verts && h.z < g.n_elems) {
            float o[3] = {0.f, 0.f, 0.f}, d[3];
            if (rays) {
                const float4 r0 = rays[2 * (size_t)h.x], r1 = rays[2 * (size_t)h.x + 1];
                o[0] = r0.x; o[1] = r0.y; o[2] = r0.z;
                d[0] = r1.x; d[1] = r1.y; d[2] = r1.z;
            } else {
                uint32_t v, hh;
                sensor_ray_dir(tb, h.x, d, &v, &hh);
            }
            float t, r9[9];
            if (record_on_triangle(g, h, o, d, &tri, &t, r9)) {
#pragma unroll
                for (int j = 0; j < 9; ++j) res[j] = r9[j];
                if (!rays) {   // a sensor ray: xyz = t * dir with no sum, the bits of k_pack (EmbreeTracer.cpp:341-345)
                    res[6] = t * d[0]; res[7] = t * d[1]; res[8] = t * d[2];
                }
                flags = 1u;
            }
        }
    }
    uint4 *dst = out + 3 * (size_t)i;
    dst[0] = make_uint4(__float_as_uint(res[0]), __float_as_uint(res[1]), __float_as_uint(res[2]), __float_as_uint(res[3]));
    dst[1] = make_uint4(__float_as_uint(res[4]), __float_as_uint(res[5]), tri, flags);
    dst[2] = make_uint4(__float_as_uint(res[6]), __float_as_uint(res[7]), __float_as_uint(res[8]), h.x);
}

}  // namespace

void launch_hit_attributes(hipStream_t s, const void *hits, const uint32_t *d_count, uint32_t n, const void *rays, uint32_t n_rays,
                           const SensorTables &tb, const AttrGeom *table, uint32_t n_table, void *out)
{
    if (!n) return;
    hipLaunchKernelGGL(k_hit_attributes, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, static_cast<const uint4 *>(hits), d_count, n,
                       static_cast<const float4 *>(rays), n_rays, tb, table, n_table, static_cast<uint4 *>(out));
}

}  // namespace ls
