// ls_attr_moving.hip -- k_hit_attributes_moving + k_returns_eval_moving: surface attributes and sensor returns for the hit records
// of a frame whose sensor and geometries move during the turn (ls_hit_attributes_moving / ls_apply_return_model_moving,
// include/lidarshooter_hip.h), siblings of k_hit_attributes (ls_attr.hip) and k_returns_eval (ls_returns.hip)
// whose gather they copy the way k_trace_rays_moving copies k_trace_rays' walk.
//
// No hierarchy, no walk: one lane per record.  What a record of ls_trace_scene_sweep_moving lacks for the exact test is the ray ITS
// geometry saw, and the lane rebuilds it from what the frame was traced with:
//   * the nominal d of ray hit.ray from the factor tables (the products k_hit_attributes forms), column h = hit.ray % H;
//   * the ray the column cast: sweep_ray(pose[h], d) -> (o, d') (ls_sweep.h), or (0, d) without a pose table;
//   * the ray geometry hit.geom saw: motion_ray(table[h], ray) -> (o_g, d_g) (ls_motion.h) where the per-geomID pointer array names a
//     table for it, else (o, d'); a record whose ray fails motion_ray_usable is invalid (the walk skipped the geometry there).
// Then k_hit_attributes' validity test with (o_g, d_g) -- the per-geomID AttrGeom entry, three indices, three vertex records, the
// frame's transform, hit_attributes_on_triangle with t bit-equal to hit.t, a quad's two halves in order --; the normal of a moving
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
#include "ls_motion.h"
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
            // LidarDevice.cpp:310-316: d = (sin(theta)cos(phi), sin(theta)sin(phi), cos(theta)), the products the trace kernels form
            const uint32_t v = h.x / tb.H, hh = h.x - v * tb.H;
            const float st = tb.sin_theta[v];
            const float2 cs = tb.cs_phi[hh];
            const float d[3] = {st * cs.x, st * cs.y, tb.cos_theta[v]};
            // the ray the column cast, then the ray the record's geometry saw
            float ray[8] = {0.f, 0.f, 0.f, 0.f, d[0], d[1], d[2], kSweepTmax};
            float p[12], q[12];
            if (pose) {
                load_pose(pose, hh, ((uintptr_t)pose & 15u) == 0u, p);
                sweep_ray(p, d[0], d[1], d[2], ray);
            }
            const float *tab = motion[h.y];
            bool usable = true;
            if (tab) {
                load_pose(tab, hh, ((uintptr_t)tab & 15u) == 0u, q);
                float rg[8];
                motion_ray(q, ray, rg);
                usable = motion_ray_usable(rg);
#pragma unroll
                for (int j = 0; j < 8; ++j) ray[j] = rg[j];
            }
            const float *o_g = ray, *d_g = ray + 4;
            const uint32_t halves = g.quad ? 2u : 1u;
            for (uint32_t c = 0; c < halves && !flags && usable; ++c) {
                const uint32_t k = g.quad ? 2u * h.z + c : h.z;
                const uint32_t *ix = g.idx + 3 * (size_t)k;
                const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
                if (i0 >= g.n_verts || i1 >= g.n_verts || i2 >= g.n_verts) continue;
                const V3 a = xform_vertex(g.m, g.verts + (size_t)i0 * g.stride);
                const V3 b = xform_vertex(g.m, g.verts + (size_t)i1 * g.stride);
                const V3 cc = xform_vertex(g.m, g.verts + (size_t)i2 * g.stride);
                const float v0[3] = {a.x, a.y, a.z}, v1[3] = {b.x, b.y, b.z}, v2[3] = {cc.x, cc.y, cc.z};
                float t, r9[9];
                if (hit_attributes_on_triangle(o_g, d_g, v0, v1, v2, &t, r9) && __float_as_uint(t) == h.w) {
#pragma unroll
                    for (int j = 0; j < 9; ++j) res[j] = r9[j];
                    if (tab) motion_normal(q, r9, res);   // the normal the geometry carries, back in the sensor frame
                    if (pose && deskew) {                 // the deskewed frame's point: o_h + t d' per axis
                        sweep_point(p, d[0], d[1], d[2], t, res + 6);
                    } else {   // what the sensor reports: xyz = t * dir with no sum, the bits of k_sweep_pack (EmbreeTracer.cpp:341-345)
                        res[6] = t * d[0]; res[7] = t * d[1]; res[8] = t * d[2];
                    }
                    tri = k;
                    flags = 1u;
                }
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
    __shared__ uint32_t s_cnt[kBlock / 64];
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
                // LidarDevice.cpp:310-316: d = (sin(theta)cos(phi), sin(theta)sin(phi), cos(theta)), the products the trace kernels form
                const uint32_t v = h.x / tb.H, hh = h.x - v * tb.H;
                const float st = tb.sin_theta[v];
                const float2 cs = tb.cs_phi[hh];
                const float d[3] = {st * cs.x, st * cs.y, tb.cos_theta[v]};
                // the ray the column cast -- the sensor ranges along it --, then the ray the record's geometry saw
                float cast[8] = {0.f, 0.f, 0.f, 0.f, d[0], d[1], d[2], kSweepTmax};
                if (pose) {
                    float p[12];
                    load_pose(pose, hh, ((uintptr_t)pose & 15u) == 0u, p);
                    sweep_ray(p, d[0], d[1], d[2], cast);
                }
                float seen[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) seen[j] = cast[j];
                const float *tab = motion[h.y];
                bool usable = true;
                if (tab) {
                    float q[12];
                    load_pose(tab, hh, ((uintptr_t)tab & 15u) == 0u, q);
                    motion_ray(q, cast, seen);
                    usable = motion_ray_usable(seen);
                }
                const float *o_g = seen, *d_g = seen + 4;
                const uint32_t halves = g.quad ? 2u : 1u;
                bool valid = false;
                float cos_inc = 0.f;
                for (uint32_t c = 0; c < halves && !valid && usable; ++c) {
                    const uint32_t k = g.quad ? 2u * h.z + c : h.z;
                    const uint32_t *ix = g.idx + 3 * (size_t)k;
                    const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
                    if (i0 >= g.n_verts || i1 >= g.n_verts || i2 >= g.n_verts) continue;
                    const V3 a = xform_vertex(g.m, g.verts + (size_t)i0 * g.stride);
                    const V3 b = xform_vertex(g.m, g.verts + (size_t)i1 * g.stride);
                    const V3 cc = xform_vertex(g.m, g.verts + (size_t)i2 * g.stride);
                    const float v0[3] = {a.x, a.y, a.z}, v1[3] = {b.x, b.y, b.z}, v2[3] = {cc.x, cc.y, cc.z};
                    float t, r9[9];
                    if (hit_attributes_on_triangle(o_g, d_g, v0, v1, v2, &t, r9) && __float_as_uint(t) == h.w) {
                        cos_inc = r9[3];   // (a rotation keeps it: the incidence on the geometry where it was committed)
                        valid = true;
                    }
                }
                if (valid) {
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
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
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
    float4 *park_point = static_cast<float4 *>(park);
    uint4 *park_hit = reinterpret_cast<uint4 *>(park_point + n);
    hipLaunchKernelGGL(k_returns_eval_moving, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, static_cast<const uint4 *>(hits), d_count, n, tb,
                       table, motion, n_table, pose, deskew ? 1u : 0u, model, frame_index, refl, n_refl, park_point, park_hit, block_counts);
}

}  // namespace ls
