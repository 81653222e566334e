// ls_velocity.hip -- k_hit_velocities: the surface velocity, the velocity of the sensor's origin and the Doppler range rate at the
// hit records of a frame (ls_hit_velocities, include/lidarshooter_hip.h), one more gather in the family of
// k_hit_attributes_moving (ls_attr_moving.hip) with which it shares the direction, the rays and the validity test (ls_hit_gather.h):
// the valid bit of a record is the one ls_hit_attributes_moving gives it for the same tables, because the same code decides it.
//
// No hierarchy, no walk, no LDS: one lane per record.  The lane rebuilds the ray its column cast and the ray its geometry saw
// (moving_rays), runs the exact test (record_on_triangle), and on a valid record evaluates the rigid-body velocity field of the
// geometry's twist at the hit point and of the sensor's twist at the sensor's origin (hit_velocity, ls_velocity.h: the host compiles
// the same sequence as ls_debug_hit_velocity).
// Every index is checked against its bound before an address is formed from it: the ray (hence the channel and the column, which
// every table of H records covers), the geometry id against the length the three per-geomID arrays share, the element, the three
// vertex indices.  Per record: what k_hit_attributes_moving reads -- 16 bytes of hit, 16 of factor tables, 128 of AttrGeom, 48 of
// pose and 48 of motion record, 12 of indices, three vertex records --, 16 bytes of table pointers instead of 8, and 24 bytes of
// twist record for the geometry and 24 for the sensor, read as dwords (the tables are 4-byte aligned and a record is no multiple of
// 16 bytes; consecutive lanes read consecutive columns); 32 bytes written, and 4 more with d_radial.
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_hit_attr.h"
#include "ls_hit_gather.h"
#include "ls_motion.h"
#include "ls_velocity.h"

namespace ls {

namespace {

// the 6 floats of column h's twist record
__device__ __forceinline__ void load_twist(const float *__restrict__ table, uint32_t h, float *tw)
{
    const float *src = table + 6 * (size_t)h;
#pragma unroll
    for (int k = 0; k < 6; ++k) tw[k] = src[k];
}

__global__ __launch_bounds__(kBlock) void k_hit_velocities(const uint4 *__restrict__ hits, const uint32_t *__restrict__ d_count, uint32_t n,
                                                           SensorTables tb, const AttrGeom *__restrict__ table,
                                                           const float *const *__restrict__ motion, const float *const *__restrict__ twist,
                                                           uint32_t n_table, const float *__restrict__ pose,
                                                           const float *__restrict__ sensor_twist, uint4 *__restrict__ out,
                                                           uint32_t *__restrict__ radial)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t count = d_count ? min(n, *d_count) : n;
    if (i >= count) return;
    const uint4 h = hits[i];   // (ray, geom, prim, t bits)
    float res[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t flags = 0;
    if (h.x < tb.V * tb.H && h.y < n_table) {
        const AttrGeom &g = table[h.y];
        if (g.verts && h.z < g.n_elems) {
            uint32_t v, hh, tri;
            float d[3], p[12], q[12], cast[8], seen[8], t, r9[9];
            sensor_ray_dir(tb, h.x, d, &v, &hh);
            if (moving_rays(pose, motion[h.y], hh, d, p, q, cast, seen) && record_on_triangle(g, h, seen, seen + 4, &tri, &t, r9)) {
                const float *gtab = twist[h.y];
                float gt[6], st[6];
                if (gtab) load_twist(gtab, hh, gt);
                if (sensor_twist) load_twist(sensor_twist, hh, st);
                hit_velocity(cast, t, sensor_twist != nullptr, st, gtab != nullptr, gt, res);
                flags = 1u;
            }
        }
    }
    if (out) {
        uint4 *dst = out + 2 * (size_t)i;
        dst[0] = make_uint4(__float_as_uint(res[0]), __float_as_uint(res[1]), __float_as_uint(res[2]), __float_as_uint(res[3]));
        dst[1] = make_uint4(__float_as_uint(res[4]), __float_as_uint(res[5]), __float_as_uint(res[6]), flags);
    }
    if (radial) radial[i] = flags ? __float_as_uint(res[3]) : 0x7FC00000u;   // an invalid record: the canonical quiet NaN
}

}  // namespace

void launch_hit_velocities(hipStream_t s, const void *hits, const uint32_t *d_count, uint32_t n, const SensorTables &tb, const AttrGeom *table,
                           const float *const *motion, const float *const *twist, uint32_t n_table, const float *pose, const float *sensor_twist,
                           void *out, float *radial)
{
    if (!n) return;
    hipLaunchKernelGGL(k_hit_velocities, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, static_cast<const uint4 *>(hits), d_count, n, tb, table,
                       motion, twist, n_table, pose, sensor_twist, static_cast<uint4 *>(out), reinterpret_cast<uint32_t *>(radial));
}

}  // namespace ls
