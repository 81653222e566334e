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
// k_sweep_count + k_sweep_pack, one lane per ray of the shard: the ordered pack of a frame (k_rowcount + k_pack,
// ls_kernels.hip) over the walk's dense ls_hit records (geom != 0xFFFFFFFF: a hit) -- the hits of every 256 rays counted, then
// each workgroup adds up the counts of the workgroups before it, ranks its own hits by ballot / mbcnt inside the wave and a
// four-entry prefix across its waves, and writes point and record at that position: ascending ray index, no atomic append, no
// workgroup waiting for another.  The point is rebuilt from the factor tables; the pose is read only under LS_SWEEP_DESKEW.
// Bytes per ray: 48 pose + 32 written (+ 32 for d_rays_out); 16 read twice; per hit 48 written (+ 48 pose when deskewing).
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_sweep.h"

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
    float p[12], r[8];
    load_pose(pose, h, aligned16 != 0u, p);
    const float st = tb.sin_theta[v], ctv = tb.cos_theta[v];
    const float2 cs = tb.cs_phi[h];
    sweep_ray(p, st * cs.x, st * cs.y, ctv, r);
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
    __shared__ uint32_t s_cnt[kBlock / 64];
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    const bool hit = q < nq && dense[q].y != kInvalid;
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(kBlock) void k_sweep_pack(SensorTables tb, const uint4 *__restrict__ dense, const uint32_t *__restrict__ block_counts,
                                                       const float *__restrict__ pose, uint32_t aligned16, uint32_t deskew,
                                                       float4 *__restrict__ points, uint4 *__restrict__ hits, uint32_t *__restrict__ n_points)
{
    __shared__ uint32_t s_part[kBlock / 64];
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t nq = tb.V * tb.naz;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    // the record, the ray's table entries and the counts of the workgroups before this one: all requested up front
    uint4 rec = make_uint4(0u, kInvalid, kInvalid, 0u);
    if (q < nq) rec = dense[q];
    const uint32_t qq = q < nq ? q : 0u;
    const uint32_t v = qq / tb.naz, h = tb.az0 + (qq - v * tb.naz);
    const float st = tb.sin_theta[v], ctv = tb.cos_theta[v];
    const float2 cs = tb.cs_phi[h];
    uint32_t acc = 0;
    constexpr uint32_t kCountsAhead = 8;
    for (uint32_t r0 = threadIdx.x; r0 < blockIdx.x; r0 += kCountsAhead * kBlock) {
        uint32_t c[kCountsAhead];
#pragma unroll
        for (uint32_t k = 0; k < kCountsAhead; ++k) c[k] = r0 + k * kBlock < blockIdx.x ? block_counts[r0 + k * kBlock] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < kCountsAhead; ++k) acc += c[k];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    const bool hit = rec.y != kInvalid;
    const unsigned long long m = __ballot(hit);
    if (lane == 0) { s_part[w] = acc; s_wave[w] = (uint32_t)__popcll(m); }
    __syncthreads();
    uint32_t base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (uint32_t k = 0; k < w; ++k) base += s_wave[k];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_points = base + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (!hit) return;
    const uint32_t dst = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));   // < the shard's rays <= the caller's capacity
    const float t = __uint_as_float(rec.w);
    if (points) {
        const float dx = st * cs.x, dy = st * cs.y;
        float xyz[3];
        if (deskew) {
            float p[12];
            load_pose(pose, h, aligned16 != 0u, p);
            sweep_point(p, dx, dy, ctv, t, xyz);
        } else {   // what the moving sensor reports: xyz = t * dir with no sum, the frame's bits (k_pack)
            xyz[0] = t * dx; xyz[1] = t * dy; xyz[2] = t * ctv;
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
    hipLaunchKernelGGL(k_sweep_rays, grid, dim3(kBlock), 0, s, tb, pose, ((uintptr_t)pose & 15u) ? 0u : 1u, static_cast<float4 *>(rays),
                       static_cast<float4 *>(rays_out));
}

void launch_sweep_pack(hipStream_t s, const SensorTables &tb, const void *dense, uint32_t *block_counts, const float *pose, bool deskew,
                       void *points32, void *hits, uint32_t *n_points)
{
    const uint32_t nq = tb.V * tb.naz;
    const dim3 grid((uint32_t)sweep_block_count(nq));
    hipLaunchKernelGGL(k_sweep_count, grid, dim3(kBlock), 0, s, static_cast<const uint4 *>(dense), nq, block_counts);
    hipLaunchKernelGGL(k_sweep_pack, grid, dim3(kBlock), 0, s, tb, static_cast<const uint4 *>(dense), block_counts, pose,
                       ((uintptr_t)pose & 15u) ? 0u : 1u, deskew ? 1u : 0u, static_cast<float4 *>(points32), static_cast<uint4 *>(hits), n_points);
}

}  // namespace ls
