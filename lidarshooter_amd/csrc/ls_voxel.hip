// ls_voxel.hip -- the kernels of ls_occupancy_grid (include/lidarshooter_hip.h): per cell of a voxel grid the
// number of rays that crossed it before their return or before they ran out of range, the number of returns that fell in it and
// the lowest geomID among those.
//
//   k_voxel_clear   the grid to zero / 0xFFFFFFFF (unless the call accumulates) and the per-ray keys to ~0;
//   k_voxel_ends    one lane per hit record: a record that counts sends (t bits << 32) | geom to its ray's key by atomicMin;
//   k_voxel_carve   one lane per ray: the span the ray carves, its occupied cell, and the walk (ls_voxel.h) over the cells of the
//                   span, one cell per trip of a wave-uniform loop.
//
// Every value written is an integer sum or an integer minimum: the grid is the same bytes whatever the order of the records and
// whatever the order in which waves arrive.  The outputs are the atomics' targets; there is no finish pass.
#include "ls_voxel.h"
#include "ls_device.h"
#include "ls_hit_gather.h"

namespace ls {

namespace {

__global__ __launch_bounds__(kBlock) void k_voxel_clear(uint2 *__restrict__ counts, uint32_t *__restrict__ geom, uint32_t n_cells,
                                                        unsigned long long *__restrict__ keys, uint32_t n_keys)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n_cells) {
        counts[i] = make_uint2(0u, 0u);
        if (geom) geom[i] = kInvalid;
    }
    if (i < n_keys) keys[i] = ~0ull;
}

// whether a caller's ray is one k_trace_rays walks (k_label_reduce's test)
__device__ __forceinline__ bool voxel_walkable(const float4 &r0, const float4 &r1)
{
    return isfinite(r0.x) && isfinite(r0.y) && isfinite(r0.z) && isfinite(r1.x) && isfinite(r1.y) && isfinite(r1.z) &&
           (r1.x != 0.f || r1.y != 0.f || r1.z != 0.f) && r0.w <= r1.w;
}

// k_label_reduce's counting rule: the geomID names a geometry of the table, the element and the ray are in range, t is finite and
// >= 0 and, for a caller ray, the ray is walkable.  Every index is checked before an address is formed from it.  t >= 0: its bits
// order as t does (a -0 counts as +0).
__global__ __launch_bounds__(kBlock) void k_voxel_ends(const uint4 *__restrict__ hits, const uint32_t *__restrict__ d_count, uint32_t n,
                                                       const float4 *__restrict__ rays, uint32_t ray_bound, uint32_t own_rays,
                                                       const AttrGeom *__restrict__ table, uint32_t n_table,
                                                       unsigned long long *__restrict__ keys)
{
    const uint32_t count = d_count ? min(n, *d_count) : n;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint4 hit = hits[i];
    const float t = __uint_as_float(hit.w);
    if (!(hit.y < n_table && hit.x < ray_bound && t >= 0.0f && t < INFINITY)) return;
    const AttrGeom &g = table[hit.y];
    if (g.verts == nullptr || hit.z >= g.n_elems) return;
    if (!own_rays && !voxel_walkable(rays[2 * (size_t)hit.x], rays[2 * (size_t)hit.x + 1])) return;
    atomicMin(&keys[hit.x], ((unsigned long long)(hit.w & 0x7FFFFFFFu) << 32) | hit.y);
}

// The cost of the carve is its atomic traffic, and that traffic is least evenly spread where it is densest: every ray of a frame
// crosses the sensor's own cell, and the 64 lanes of a wave -- adjacent azimuths of one channel from one origin -- stand in the
// same cell for most of the trips near it.  AGGREGATE: a lane that marks a cell is the head of a run when the lane below it marks
// another cell or none; one ballot of the heads and one of the marking lanes give each head the length of its run, and only heads
// add -- the run's length at once.  The plain form adds one per marking lane.  The sums are the same.
template <bool AGGREGATE>
__global__ __launch_bounds__(kBlock) void k_voxel_carve(VoxelGrid g, const float4 *__restrict__ rays, uint32_t ray_bound, uint32_t own_rays,
                                                        SensorTables tb, const unsigned long long *__restrict__ keys,
                                                        uint32_t *__restrict__ counts, uint32_t *__restrict__ geom)
{
    const uint32_t ray = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    VoxelWalk w;
    w.live = false;
    uint32_t occ = kVoxelNone;
    if (ray < ray_bound) {
        float o[3] = {0.f, 0.f, 0.f}, d[3];
        float tmin = 0.f, tmax = INFINITY;
        bool ok = true;
        if (own_rays) {
            uint32_t v, h;
            sensor_ray_dir(tb, ray, d, &v, &h);
        } else {
            const float4 r0 = rays[2 * (size_t)ray], r1 = rays[2 * (size_t)ray + 1];
            ok = voxel_walkable(r0, r1);
            o[0] = r0.x; o[1] = r0.y; o[2] = r0.z; tmin = r0.w;
            d[0] = r1.x; d[1] = r1.y; d[2] = r1.z; tmax = r1.w;
        }
        if (ok) {
            if (g.has_xf) voxel_ray_to_grid(g.xf, o, d);
            const unsigned long long key = keys[ray];
            const bool has_t = key != ~0ull;
            const float t = __uint_as_float((uint32_t)(key >> 32));
            float t0, t1;
            bool marks;
            const bool carve = voxel_span(g, tmin, tmax, has_t, t, &t0, &t1, &marks);
            if (marks) occ = voxel_occupied_cell(g, o, d, t, own_rays && !g.has_xf);
            if (occ != kVoxelNone) {   // (below n_cells by voxel_cell_of's compares)
                atomicAdd(&counts[2 * (size_t)occ + 1], 1u);
                if (geom) atomicMin(&geom[occ], (uint32_t)key);
            }
            if (carve) voxel_walk_begin(g, o, d, t0, t1, w);
        }
    }
    // one cell per trip; the wave goes on while any lane walks.  A cell index is in range by construction of the walk.
    while (__ballot(w.live) != 0ull) {
        const uint32_t at = w.live ? voxel_index(g, w) : kVoxelNone;
        const uint32_t mark = at != occ ? at : kVoxelNone;   // (a lane that does not walk: kVoxelNone either way)
        if (AGGREGATE) {
            const uint32_t below = (uint32_t)__shfl_up((int)mark, 1);
            const bool marking = mark != kVoxelNone;
            const bool head = marking && (lane == 0u || below != mark);
            const unsigned long long heads = __ballot(head), marks = __ballot(marking);
            if (head) {
                // the run ends before the next head or the next lane that marks nothing
                const unsigned long long stop = (heads | ~marks) & ~((2ull << lane) - 1ull);
                const uint32_t end = stop ? (uint32_t)__ffsll((long long)stop) - 1u : 64u;
                atomicAdd(&counts[2 * (size_t)mark], end - lane);
            }
        } else {
            if (mark != kVoxelNone) atomicAdd(&counts[2 * (size_t)mark], 1u);
        }
        if (w.live) voxel_walk_next(g, w);
    }
}

}  // namespace

void launch_voxel_clear(hipStream_t s, const VoxelGrid &g, void *counts, uint32_t *geom, unsigned long long *keys, uint32_t n_keys)
{
    const uint32_t n_cells = (g.flags & LS_OCC_ACCUMULATE) ? 0u : g.n[0] * g.n[1] * g.n[2];
    const uint32_t n = max(n_cells, n_keys);
    if (!n) return;
    hipLaunchKernelGGL(k_voxel_clear, dim3((uint32_t)(((unsigned long long)n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       static_cast<uint2 *>(counts), geom, n_cells, keys, n_keys);
}

void launch_voxel_ends(hipStream_t s, const void *hits, const uint32_t *d_count, uint32_t n, const void *rays, uint32_t n_rays, bool own_rays,
                       const SensorTables &tb, const AttrGeom *table, uint32_t n_table, unsigned long long *keys)
{
    const uint32_t ray_bound = own_rays ? tb.V * tb.H : n_rays;
    if (!n || !ray_bound) return;
    hipLaunchKernelGGL(k_voxel_ends, dim3((uint32_t)(((unsigned long long)n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       static_cast<const uint4 *>(hits), d_count, n, static_cast<const float4 *>(rays), ray_bound, own_rays ? 1u : 0u, table,
                       n_table, keys);
}

void launch_voxel_carve(hipStream_t s, const VoxelGrid &g, const void *rays, uint32_t n_rays, bool own_rays, const SensorTables &tb,
                        const unsigned long long *keys, void *counts, uint32_t *geom, bool aggregate)
{
    const uint32_t ray_bound = own_rays ? tb.V * tb.H : n_rays;
    if (!ray_bound) return;
    const dim3 grid((uint32_t)(((unsigned long long)ray_bound + kBlock - 1) / kBlock));
    if (aggregate)
        hipLaunchKernelGGL(k_voxel_carve<true>, grid, dim3(kBlock), 0, s, g, static_cast<const float4 *>(rays), ray_bound, own_rays ? 1u : 0u, tb,
                           keys, static_cast<uint32_t *>(counts), geom);
    else
        hipLaunchKernelGGL(k_voxel_carve<false>, grid, dim3(kBlock), 0, s, g, static_cast<const float4 *>(rays), ray_bound, own_rays ? 1u : 0u, tb,
                           keys, static_cast<uint32_t *>(counts), geom);
}

}  // namespace ls
