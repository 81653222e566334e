// ls_sweep.hip -- k_sweep_rays, k_sweep_count + k_sweep_pack: the two passes ls_trace_scene_sweep (include/lidarshooter_hip.h;
// DESIGN.md 3.3.5) puts around the ray queries' walk (k_trace_rays, ls_rays.hip), which it runs unchanged.
//
// k_sweep_rays, one lane per ray of the shard: the nominal direction from the factor tables (the products the frame kernels and
// k_raygen_aos form), carried through the pose of its azimuth column (ls_sweep.h: the arithmetic ls_debug_sweep_ray runs on the
// host) into a 32-byte lidarshooter::Ray record -- at the shard-local index q = v * naz + (h - az0), ascending in the global
// ray index, which is what the walk reads; and, when asked, at the global index r = v * H + h of the caller's buffer.  A wave
// is 64 consecutive columns of ONE ring: the ring's two table entries are the same in every lane, the wave's poses are 3 KB
// of contiguous memory read once, its records 2 KB of contiguous memory written once.  No transcendental: the table's
// rotations were made on the host.
// k_sweep_count + k_sweep_pack, one lane per ray of the shard: the ordered pack (ls_pack.h: block_count_store, counts_before,
// pack_wave_base) over the walk's dense ls_hit records (geom != 0xFFFFFFFF: a hit), a ballot bit per lane: point and record go
// to the hit's rank among the shard's hits, ascending ray index.  The point is rebuilt from the factor tables (shard_ray_dir,
// ls_hit_gather.h); the pose is read only under LS_SWEEP_DESKEW.
// Bytes per ray: 48 pose + 32 written (+ 32 for d_rays_out); 16 read twice; per hit 48 written (+ 48 pose when deskewing).
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_sweep.h"
#include "ls_pack.h"
#include "ls_hit_gather.h"

namespace ls {

namespace {

constexpr uint32_t kSweepRows = kBlock / 64;   // rings per workgroup of k_sweep_rays: one per wave

__global__ __launch_bounds__(kBlock) void k_sweep_rays(SensorTables tb, const float *__restrict__ pose, uint32_t aligned16,
                                                       float4 *__restrict__ rays, float4 *__restrict__ rays_out)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t v = blockIdx.y * kSweepRows + w, c = blockIdx.x * 64u + lane;
    if (v >= tb.V || c >= tb.naz) return;
    const uint32_t h = tb.az0 + c;   // < H: the shard lies inside the raster (ls_tracer_set_shard)
    float p[12], d[3], r[8];
    load_pose(pose, h, aligned16 != 0u, p);
    sensor_dir(tb, v, h, d);
    sweep_ray(p, d[0], d[1], d[2], r);
    const float4 r0 = make_float4(r[0], r[1], r[2], r[3]), r1 = make_float4(r[4], r[5], r[6], r[7]);
    const size_t q = (size_t)v * tb.naz + c;
    rays[2 * q] = r0;
    rays[2 * q + 1] = r1;
    if (rays_out) {
        const size_t g = (size_t)v * tb.H + h;
        rays_out[2 * g] = r0;
        rays_out[2 * g + 1] = r1;
    }
}

// hits per 256 consecutive dense records (feeds the ordered pack)
__global__ __launch_bounds__(kBlock) void k_sweep_count(const uint4 *__restrict__ dense, uint32_t nq, uint32_t *__restrict__ block_counts)
{
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    const bool hit = q < nq && dense[q].y != kInvalid;
    block_count_store((uint32_t)__popcll(__ballot(hit)), block_counts);
}

__global__ __launch_bounds__(kBlock) void k_sweep_pack(SensorTables tb, const uint4 *__restrict__ dense, const uint32_t *__restrict__ block_counts,
                                                       const float *__restrict__ pose, uint32_t aligned16, uint32_t deskew,
                                                       float4 *__restrict__ points, uint4 *__restrict__ hits, uint32_t *__restrict__ n_points)
{
    const uint32_t nq = tb.V * tb.naz;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    // the record, the ray's table entries and the counts of the workgroups before this one: all requested up front
    uint4 rec = make_uint4(0u, kInvalid, kInvalid, 0u);
    if (q < nq) rec = dense[q];
    uint32_t v, h;
    float d[3];
    shard_ray_dir(tb, q < nq ? q : 0u, d, &v, &h);
    const uint32_t acc = counts_before(block_counts, blockIdx.x);
    const bool hit = rec.y != kInvalid;
    const unsigned long long m = __ballot(hit);
    const uint32_t base = pack_wave_base(acc, (uint32_t)__popcll(m), 0u, blockIdx.x == gridDim.x - 1, n_points);
    if (!hit) return;
    const uint32_t dst = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));   // < the shard's rays <= the caller's capacity
    const float t = __uint_as_float(rec.w);
    if (points) {
        float xyz[3];
        if (deskew) {
            float p[12];
            load_pose(pose, h, aligned16 != 0u, p);
            sweep_point(p, d[0], d[1], d[2], t, xyz);
        } else {   // what the moving sensor reports: xyz = t * dir with no sum, the frame's bits (k_pack)
            xyz[0] = t * d[0]; xyz[1] = t * d[1]; xyz[2] = t * d[2];
        }
        points[2 * (size_t)dst] = make_float4(xyz[0], xyz[1], xyz[2], 0.0f);
        points[2 * (size_t)dst + 1] = make_float4(64.0f, __int_as_float((int)v), 0.0f, 0.0f);
    }
    if (hits) hits[dst] = make_uint4(v * tb.H + h, rec.y, rec.z, rec.w);
}

}  // namespace

size_t sweep_block_count(uint32_t nq) { return ((size_t)nq + kBlock - 1) / kBlock; }

void launch_sweep_rays(hipStream_t s, const SensorTables &tb, const float *pose, void *rays, void *rays_out)
{
    const dim3 grid((tb.naz + 63u) / 64u, (tb.V + kSweepRows - 1u) / kSweepRows);
    hipLaunchKernelGGL(k_sweep_rays, grid, dim3(kBlock), 0, s, tb, pose, table_aligned16(pose), static_cast<float4 *>(rays),
                       static_cast<float4 *>(rays_out));
}

void launch_sweep_pack(hipStream_t s, const SensorTables &tb, const void *dense, uint32_t *block_counts, const float *pose, bool deskew,
                       void *points32, void *hits, uint32_t *n_points)
{
    const uint32_t nq = tb.V * tb.naz;
    const dim3 grid((uint32_t)sweep_block_count(nq));
    hipLaunchKernelGGL(k_sweep_count, grid, dim3(kBlock), 0, s, static_cast<const uint4 *>(dense), nq, block_counts);
    hipLaunchKernelGGL(k_sweep_pack, grid, dim3(kBlock), 0, s, tb, static_cast<const uint4 *>(dense), block_counts, pose,
                       table_aligned16(pose), deskew ? 1u : 0u, static_cast<float4 *>(points32), static_cast<uint4 *>(hits), n_points);
}

}  // namespace ls
