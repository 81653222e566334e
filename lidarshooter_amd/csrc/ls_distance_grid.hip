// ls_distance_grid.hip -- the kernels of ls_scene_distance_grid (include/lidarshooter_hip.h): per cell of a voxel
// grid the distance from its centre to the nearest triangle of the committed scene within a truncation distance, and the lowest
// geomID among the triangles that attain it.
//
//   k_distance_grid_clear   every record to {0xFFFFFFFF, +inf} (unless the call accumulates) and the queue's count word to zero;
//   k_distance_grid_small   one WAVE per triangle of the scene's flat index: the triangle, its vertices (ls_scene_tris.h)
//                           and its widened, clamped cell range (ls_distance_grid.h) are uniform
//                           over the wave; a range of at most `small` cells is worked off by the wave, its 64 lanes striding over
//                           the cells; a larger one is appended to a queue -- one atomicAdd per wave;
//   k_distance_grid_big     the queued triangles, on k_scene_grid_big's fixed launch: one to 32 blocks per entry, as many as the
//                           launch has for each, stride over the range's chunks of 256 cells, a lane per cell.
//
// Every cell of a triangle's range gets the same point-triangle sequence whichever kernel reaches it (dist_cell): there is no
// tile- or box-level rejection.  A counting pair sends (bits(dist) << 32) | geomID to its cell by a 64-bit atomicMin: every value is a
// minimum, so the grid is the same bytes whatever the order of the triangles and of the waves.  Every loop bound comes from the
// clamped integer range, at most 2^27 cells; the big launch is a fixed grid whatever the queue holds; no workgroup waits for
// another: a launch ends whatever the vertices hold.
#include "ls_distance_grid.h"
#include "ls_scene_tris.h"

namespace ls {

namespace {

__global__ __launch_bounds__(kBlock) void k_distance_grid_clear(unsigned long long *__restrict__ cells, uint32_t n_cells,
                                                                uint32_t *__restrict__ queue_count)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;   // two records (cells is 16-byte aligned)
    if (i == 0u) *queue_count = 0u;
    if (2u * i + 1u < n_cells)
        reinterpret_cast<ulonglong2 *>(cells)[i] = make_ulonglong2(kDistGridRest, kDistGridRest);
    else if (2u * i < n_cells)
        cells[2u * i] = kDistGridRest;
}

// Triangle `tri` of geometry ge (both in range of the table) in the grid's frame (scene_tri_vertices).  false: no such geometry,
// an index out of range, a non-finite vertex or a band outside the grid
__device__ __forceinline__ bool dist_tri_load(const DistGrid &g, const AttrGeom &ge, uint32_t tri, DistTri &t, SceneRange &r)
{
    V3 a, b, c;
    if (!scene_tri_vertices(g.has_xf != 0u, g.xf, ge, tri, a, b, c)) return false;
    return dist_tri_setup(g, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, t, r);
}

// one (triangle, cell) pair; the cell lies in the triangle's clamped range, so its index is below nx ny nz.  The word only ever
// decreases, so what a pre-read returns is the word or an older, larger value: skipping the atomic when it is already <= key is
// right whenever it is taken
__device__ __forceinline__ void dist_send(const DistGrid &g, const DistTri &t, uint32_t geom, bool preread, int cx, int cy, int cz,
                                          unsigned long long *__restrict__ cells)
{
    float dist;
    if (!dist_cell(t, g.trunc, g.cell, cx, cy, cz, &dist)) return;
    const unsigned long long key = dist_key(__float_as_uint(dist), geom);
    unsigned long long *at = &cells[dist_cell_index(g, cx, cy, cz)];
    if (preread && __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;
    atomicMin(at, key);
}

__global__ __launch_bounds__(kBlock) void k_distance_grid_small(DistGrid g, const AttrGeom *__restrict__ table, uint32_t n_table,
                                                                const uint32_t *__restrict__ tri_first, uint32_t n_tris,
                                                                const uint8_t *__restrict__ select, uint32_t n_select, uint32_t small,
                                                                uint32_t preread, unsigned long long *__restrict__ cells,
                                                                uint32_t *__restrict__ queue_count, uint2 *__restrict__ queue)
{
    // the wave's triangle: the same in every lane, and said so, so that the search, the loads and the set-up are scalar work
    const uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)));
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= n_tris) return;
    const uint32_t gid = scene_geom_of(tri_first, n_table, i), tri = i - tri_first[gid];
    if (!(gid >= n_select || select[gid] != 0)) return;
    DistTri t;
    SceneRange r;
    if (!dist_tri_load(g, table[gid], tri, t, r)) return;
    const uint32_t n = scene_range_cells(r);   // (at most 2^27)
    if (n > small) {
        if (lane == 0u) {
            const uint32_t slot = atomicAdd(queue_count, 1u);   // (below n_tris: a triangle is queued once)
            if (slot < n_tris) queue[slot] = make_uint2(gid, tri);
        }
        return;
    }
    const uint32_t wx = (uint32_t)(r.hix - r.lox + 1), wxy = wx * (uint32_t)(r.hiy - r.loy + 1);
    for (uint32_t k = lane; k < n; k += 64u) {   // at most ceil(small / 64) trips; no two lanes of a trip meet in a cell
        const uint32_t z = k / wxy, rest = k - z * wxy, y = rest / wx, x = rest - y * wx;
        dist_send(g, t, gid, preread != 0u, r.lox + (int)x, r.loy + (int)y, r.loz + (int)z, cells);
    }
}

// The launch is kDistGridBigX x kDistGridBigY blocks whatever the queue holds; how they share the queue is decided on the device,
// the same way in every block, from the count word: `per` blocks work on one entry -- a power of two, as many as the launch has
// for each entry, at most kDistGridBigY -- and stride over the range's chunks of 256 consecutive cells (the small kernel's cell
// order), a lane per cell.  Two ground triangles under a 2048 x 2048 grid get 32 blocks each and every block of the chip has work;
// a dense mesh under a wide band (a million queued triangles of a few thousand cells each) gets a block per entry, so that the
// triangle's load is not repeated by blocks that find no chunk left (EXPERIMENTS.md E24).
static_assert(kDistGridChunk == (uint32_t)kBlock && (kDistGridBigY & (kDistGridBigY - 1u)) == 0u, "a lane per cell of a chunk; per divides the launch");
__global__ __launch_bounds__(kBlock) void k_distance_grid_big(DistGrid g, const AttrGeom *__restrict__ table, uint32_t n_table, uint32_t n_tris,
                                                              uint32_t preread, unsigned long long *__restrict__ cells,
                                                              const uint32_t *__restrict__ queue_count, const uint2 *__restrict__ queue)
{
    const uint32_t n = min(*queue_count, n_tris);
    const uint32_t blocks = gridDim.x * gridDim.y, b = blockIdx.y * gridDim.x + blockIdx.x;
    uint32_t per = 1u;
    while (per < gridDim.y && (unsigned long long)n * (2u * per) <= blocks) per *= 2u;   // (gridDim.y is a power of two: per divides blocks)
    const uint32_t groups = blocks / per, group = b / per, sub = b % per;
    for (uint32_t e = group; e < n; e += groups) {
        const uint2 item = queue[e];
        if (item.x >= n_table) continue;   // (k_distance_grid_small queued it from this table)
        const AttrGeom &ge = table[item.x];
        if (item.y >= (ge.quad ? 2u * ge.n_elems : ge.n_elems)) continue;
        DistTri t;
        SceneRange r;
        if (!dist_tri_load(g, ge, item.y, t, r)) continue;
        const uint32_t n_cells = scene_range_cells(r);   // (at most 2^27)
        const uint32_t wx = (uint32_t)(r.hix - r.lox + 1), wxy = wx * (uint32_t)(r.hiy - r.loy + 1);
        const uint32_t chunks = (n_cells + kDistGridChunk - 1u) / kDistGridChunk;
        for (uint32_t chunk = sub; chunk < chunks; chunk += per) {
            const uint32_t k = chunk * kDistGridChunk + threadIdx.x;
            if (k < n_cells) {
                const uint32_t z = k / wxy, rest = k - z * wxy, y = rest / wx, x = rest - y * wx;
                dist_send(g, t, item.x, preread != 0u, r.lox + (int)x, r.loy + (int)y, r.loz + (int)z, cells);
            }
        }
    }
}

}  // namespace

void launch_distance_grid_clear(hipStream_t s, const DistGrid &g, unsigned long long *cells, uint32_t *queue_count)
{
    const uint32_t n_cells = (g.flags & LS_DIST_GRID_ACCUMULATE) ? 0u : g.n[0] * g.n[1] * g.n[2];
    const uint32_t lanes = max((n_cells + 1u) / 2u, 1u);
    hipLaunchKernelGGL(k_distance_grid_clear, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, s, cells, n_cells, queue_count);
}

void launch_distance_grid_small(hipStream_t s, const DistGrid &g, const AttrGeom *table, uint32_t n_table, const uint32_t *tri_first,
                                uint32_t n_tris, const uint8_t *select, uint32_t n_select, uint32_t small, bool preread, unsigned long long *cells,
                                uint32_t *queue_count, uint2 *queue)
{
    if (!n_tris || !n_table) return;
    constexpr uint32_t per_block = kBlock / 64;   // a wave per triangle
    const dim3 grid((uint32_t)(((unsigned long long)n_tris + per_block - 1) / per_block));
    hipLaunchKernelGGL(k_distance_grid_small, grid, dim3(kBlock), 0, s, g, table, n_table, tri_first, n_tris, select, n_select, small,
                       preread ? 1u : 0u, cells, queue_count, queue);
}

void launch_distance_grid_big(hipStream_t s, const DistGrid &g, const AttrGeom *table, uint32_t n_table, uint32_t n_tris, bool preread,
                              unsigned long long *cells, const uint32_t *queue_count, const uint2 *queue)
{
    if (!n_tris || !n_table) return;
    hipLaunchKernelGGL(k_distance_grid_big, dim3(min(n_tris, kDistGridBigX), kDistGridBigY), dim3(kBlock), 0, s, g, table, n_table, n_tris,
                       preread ? 1u : 0u, cells, queue_count, queue);
}

}  // namespace ls
