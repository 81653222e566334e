// ls_attr_moving.hip -- k_hit_attributes_moving + k_returns_eval_moving: surface attributes and sensor returns for the hit records
// of a frame whose sensor and geometries move during the turn (ls_hit_attributes_moving / ls_apply_return_model_moving,
// include/lidarshooter_hip.h), siblings of k_hit_attributes (ls_attr.hip) and k_returns_eval (ls_returns.hip)
// with which they share the direction, the validity test (ls_hit_gather.h) and the count of kept records (ls_pack.h); the two
// kernels here share moving_rays (ls_hit_gather.h), the three steps below.
//
// No hierarchy, no walk: one lane per record.  What a record of ls_trace_scene_sweep_moving lacks for the exact test is the ray ITS
// geometry saw, and the lane rebuilds it from what the frame was traced with (moving_rays): the nominal d of ray hit.ray, column h =
// hit.ray % H; the ray the column cast, (o, d'); the ray geometry hit.geom saw, (o_g, d_g), where the per-geomID pointer array names
// a table for it; a record whose ray fails motion_ray_usable is invalid (the walk skipped the geometry there).
// Then the validity test (record_on_triangle) with (o_g, d_g) -- the per-geomID AttrGeom entry, three indices, three vertex records,
// the frame's transform, hit_attributes_on_triangle with t bit-equal to hit.t, a quad's two halves in order --; the normal of a moving
// geometry goes back into the sensor frame through motion_normal (ls_motion.h); the point is t * d with the nominal d (the frame's
// points32 bits) or, deskewed under a pose table, sweep_point(pose[h], d, t) (the deskewed frame's).
// Every index is checked against its bound before an address is formed from it: the ray (hence the channel and the column, which
// every table of H records covers), the geometry id against the length both per-geomID arrays share, the element, the three vertex
// indices.  Per record: 16 bytes of hit, 16 of factor tables, 128 of AttrGeom and 8 of table pointer (lanes of a wave mostly share
// them: frame records come in ray order), 48 of pose and 48 of motion record (consecutive lanes read consecutive columns), 12 of
// indices, three vertex records; 48 bytes written (k_returns_eval_moving: 32 parked).
// k_returns_eval_moving parks what k_returns_eval parks; the compaction is k_returns_pack itself (launch_returns_pack, ls_returns.hip).
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_hit_attr.h"
#include "ls_hit_gather.h"
#include "ls_motion.h"
#include "ls_pack.h"
#include "ls_return_model.h"

namespace ls {

namespace {

__global__ __launch_bounds__(kBlock) void k_hit_attributes_moving(const uint4 *__restrict__ hits, const uint32_t *__restrict__ d_count, uint32_t n,
                                                                  SensorTables tb, const AttrGeom *__restrict__ table,
                                                                  const float *const *__restrict__ motion, uint32_t n_table,
                                                                  const float *__restrict__ pose, uint32_t deskew, uint4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t count = d_count ? min(n, *d_count) : n;
    if (i >= count) return;
    const uint4 h = hits[i];   // (ray, geom, prim, t bits)
    float res[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t tri = 0, flags = 0;
    if (h.x < tb.V * tb.H && h.y < n_table) {
        const AttrGeom &g = table[h.y];
        if (g.verts && h.z < g.n_elems) {
            uint32_t v, hh;
            float d[3], p[12], q[12], cast[8], seen[8], t, r9[9];
            sensor_ray_dir(tb, h.x, d, &v, &hh);
            const float *tab = motion[h.y];
            if (moving_rays(pose, tab, hh, d, p, q, cast, seen) && record_on_triangle(g, h, seen, seen + 4, &tri, &t, r9)) {
#pragma unroll
                for (int j = 0; j < 9; ++j) res[j] = r9[j];
                if (tab) motion_normal(q, r9, res);   // the normal the geometry carries, back in the sensor frame
                if (pose && deskew) {                 // the deskewed frame's point: o_h + t d' per axis
                    sweep_point(p, d[0], d[1], d[2], t, res + 6);
                } else {   // what the sensor reports: xyz = t * dir with no sum, the bits of k_sweep_pack (EmbreeTracer.cpp:341-345)
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

__global__ __launch_bounds__(kBlock) void k_returns_eval_moving(const uint4 *__restrict__ hits, const uint32_t *__restrict__ d_count, uint32_t n,
                                                                SensorTables tb, const AttrGeom *__restrict__ table,
                                                                const float *const *__restrict__ motion, uint32_t n_table,
                                                                const float *__restrict__ pose, uint32_t deskew, ls_return_model model,
                                                                uint32_t frame_index, const float *__restrict__ refl, uint32_t n_refl,
                                                                float4 *__restrict__ park_point, uint4 *__restrict__ park_hit,
                                                                uint32_t *__restrict__ block_counts)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t count = d_count ? min(n, *d_count) : n;
    bool keep = false;
    if (i < count) {
        const uint4 h = hits[i];   // (ray, geom, prim, t bits)
        float tp = 0.f, I = 0.f, px = 0.f, py = 0.f, pz = 0.f;
        if (h.x < tb.V * tb.H && h.y < n_table) {
            const AttrGeom &g = table[h.y];
            if (g.verts && h.z < g.n_elems) {
                const float rho = refl && h.y < n_refl ? refl[h.y] : 1.0f;
                // the ray the column cast -- the sensor ranges along it --, then the ray the record's geometry saw
                uint32_t v, hh, tri;
                float d[3], p[12], q[12], cast[8], seen[8], t, r9[9];
                sensor_ray_dir(tb, h.x, d, &v, &hh);
                if (moving_rays(pose, motion[h.y], hh, d, p, q, cast, seen) && record_on_triangle(g, h, seen, seen + 4, &tri, &t, r9)) {
                    const float cos_inc = r9[3];   // (a rotation keeps it: the incidence on the geometry where it was committed)
                    const float len = sqrtf((cast[4] * cast[4] + cast[5] * cast[5]) + cast[6] * cast[6]);
                    keep = return_model_eval(model, h.x, frame_index, __uint_as_float(h.w), len, cos_inc, rho, &tp, &I);
                    if (pose && deskew) {
                        px = cast[0] + tp * cast[4]; py = cast[1] + tp * cast[5]; pz = cast[2] + tp * cast[6];
                    } else {   // what the sensor reports: xyz = t' * dir with no sum, the bits of k_sweep_pack (EmbreeTracer.cpp:341-345)
                        px = tp * d[0]; py = tp * d[1]; pz = tp * d[2];
                    }
                }
            }
        }
        park_hit[i] = make_uint4(h.x, h.y, h.z, keep ? __float_as_uint(tp) : 0u);
        if (keep) park_point[i] = make_float4(px, py, pz, I);
    }
    block_count_store((uint32_t)__popcll(__ballot(keep)), block_counts);
}

}  // namespace

void launch_hit_attributes_moving(hipStream_t s, const void *hits, const uint32_t *d_count, uint32_t n, const SensorTables &tb, const AttrGeom *table,
                                  const float *const *motion, uint32_t n_table, const float *pose, bool deskew, void *out)
{
    if (!n) return;
    hipLaunchKernelGGL(k_hit_attributes_moving, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, static_cast<const uint4 *>(hits), d_count, n, tb,
                       table, motion, n_table, pose, deskew ? 1u : 0u, static_cast<uint4 *>(out));
}

void launch_returns_eval_moving(hipStream_t s, const void *hits, const uint32_t *d_count, uint32_t n, const SensorTables &tb, const AttrGeom *table,
                                const float *const *motion, uint32_t n_table, const float *pose, bool deskew, const ls_return_model &model,
                                uint32_t frame_index, const float *refl, uint32_t n_refl, void *park, uint32_t *block_counts)
{
    if (!n) return;
    const ParkHalves pk = park_halves(park, n);
    hipLaunchKernelGGL(k_returns_eval_moving, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, static_cast<const uint4 *>(hits), d_count, n, tb,
                       table, motion, n_table, pose, deskew ? 1u : 0u, model, frame_index, refl, n_refl, pk.point, pk.hit, block_counts);
}

}  // namespace ls
