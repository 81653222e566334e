// ls_scene_grid.hip -- the kernels of ls_scene_grid (include/lidarshooter_hip.h): per cell of a voxel grid the
// number of triangles of the committed scene that overlap it and the lowest geomID among them.
//
//   k_scene_grid_clear   the grid to zero / 0xFFFFFFFF (unless the call accumulates) and the queue's count word to zero;
//   k_scene_grid_small   one lane per triangle of the scene's flat index: its vertices (ls_scene_tris.h), the clamped cell
//                        range (ls_scene_grid.h); a range of at most `small` cells is tested by the lane itself, a
//                        larger one is appended to a queue -- one ballot and one atomicAdd per wave;
//   k_scene_grid_big     the queued triangles: blockIdx.x strides over the queue, blockIdx.y over the triangle's tiles of 8 x 8 x 8
//                        cells, the lanes of the block over the cells of a tile, so that one ground triangle under a 2048 x 2048
//                        grid is spread over the chip.
//
// Every cell of a triangle's range gets the same 13-axis test whichever kernel reaches it (scene_cell_overlaps): there is no
// tile-level rejection.  Every value written is an integer sum or an integer minimum: the grid is the same bytes whatever the
// order of the triangles and of the waves.  Every loop bound comes from the clamped integer range, at most 2^27 cells: a launch
// ends whatever the vertices hold.
#include "ls_scene_grid.h"
#include "ls_scene_tris.h"

namespace ls {

namespace {

__global__ __launch_bounds__(kBlock) void k_scene_grid_clear(uint4 *__restrict__ counts, uint32_t *__restrict__ geom, uint32_t n_cells,
                                                             uint32_t *__restrict__ queue_count)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;   // four cells (counts is 16-byte aligned)
    if (i == 0u) *queue_count = 0u;
    if (4u * i + 3u < n_cells) {
        counts[i] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        uint32_t *c = reinterpret_cast<uint32_t *>(counts);
        for (uint32_t k = 4u * i; k < n_cells; ++k) c[k] = 0u;   // (at most three)
    }
    if (geom)
        for (uint32_t k = 4u * i; k < n_cells && k < 4u * i + 4u; ++k) geom[k] = kInvalid;
}

// Triangle `tri` of geometry ge (both in range of the table) in the grid's frame (scene_tri_vertices).  false: no such geometry,
// an index out of range, a non-finite vertex or a triangle outside the grid
__device__ __forceinline__ bool scene_tri_load(const SceneGrid &g, const AttrGeom &ge, uint32_t tri, SceneTri &t, SceneRange &r)
{
    V3 a, b, c;
    if (!scene_tri_vertices(g.has_xf != 0u, g.xf, ge, tri, a, b, c)) return false;
    return scene_tri_setup(g, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, t, r);
}

// Dense meshes put many tiny adjacent triangles into one cell, and the lanes of a wave are adjacent triangles of one geometry.
// AGGREGATE (k_voxel_carve's run-of-lanes form): a lane that marks a cell is the head of a run when the lane below it marks another
// cell or none; only heads add -- the run's length at once -- and send the geomID: the flat triangle index ascends with the geomID,
// so the head's is the lowest of its run.  The plain form adds one per marking lane.  The sums and the minima are the same.
template <bool AGGREGATE>
__global__ __launch_bounds__(kBlock) void k_scene_grid_small(SceneGrid g, const AttrGeom *__restrict__ table, uint32_t n_table,
                                                             const uint32_t *__restrict__ tri_first, uint32_t n_tris,
                                                             const uint8_t *__restrict__ select, uint32_t n_select, uint32_t small,
                                                             uint32_t *__restrict__ counts, uint32_t *__restrict__ geom,
                                                             uint32_t *__restrict__ queue_count, uint2 *__restrict__ queue)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    SceneTri t;
    SceneRange r;
    uint32_t gid = 0u, tri = 0u, cells = 0u;   // cells = 0: this lane has no triangle
    if (i < n_tris) {
        gid = scene_geom_of(tri_first, n_table, i);
        tri = i - tri_first[gid];
        const bool selected = gid >= n_select || select[gid] != 0;
        if (selected && scene_tri_load(g, table[gid], tri, t, r)) cells = scene_range_cells(r);
    }
    // the larger ranges go to the queue: the wave's first such lane takes as many slots as there are, each lane its own among them
    const bool big = cells > small;
    const unsigned long long bigs = __ballot(big);
    if (bigs != 0ull) {
        const uint32_t first = (uint32_t)__ffsll((long long)bigs) - 1u;
        uint32_t base = 0u;
        if (lane == first) base = atomicAdd(queue_count, (uint32_t)__popcll(bigs));
        base = (uint32_t)__shfl((int)base, (int)first);
        if (big) queue[base + (uint32_t)__popcll(bigs & ((1ull << lane) - 1ull))] = make_uint2(gid, tri);   // (below n_tris: a triangle is queued once)
    }
    const uint32_t mine = big ? 0u : cells;   // at most `small` trips
    const uint32_t wx = cells ? (uint32_t)(r.hix - r.lox + 1) : 1u, wy = cells ? (uint32_t)(r.hiy - r.loy + 1) : 1u;
    if (AGGREGATE) {
        // one cell per trip; the wave goes on while any lane has cells left
        for (uint32_t k = 0u; __ballot(k < mine) != 0ull; ++k) {
            uint32_t mark = kInvalid;
            if (k < mine) {
                const uint32_t x = k % wx, y = (k / wx) % wy, z = k / (wx * wy);
                const int cx = r.lox + (int)x, cy = r.loy + (int)y, cz = r.loz + (int)z;
                if (scene_cell_overlaps(t, cx, cy, cz)) mark = scene_cell_index(g, cx, cy, cz);
            }
            const uint32_t below = (uint32_t)__shfl_up((int)mark, 1);
            const bool marking = mark != kInvalid;
            const bool head = marking && (lane == 0u || below != mark);
            const unsigned long long heads = __ballot(head), marks = __ballot(marking);
            if (head) {
                // the run ends before the next head or the next lane that marks nothing
                const unsigned long long stop = (heads | ~marks) & ~((2ull << lane) - 1ull);
                const uint32_t end = stop ? (uint32_t)__ffsll((long long)stop) - 1u : 64u;
                atomicAdd(&counts[mark], end - lane);
                if (geom) atomicMin(&geom[mark], gid);
            }
        }
    } else {
        for (uint32_t k = 0u; k < mine; ++k) {
            const uint32_t x = k % wx, y = (k / wx) % wy, z = k / (wx * wy);
            const int cx = r.lox + (int)x, cy = r.loy + (int)y, cz = r.loz + (int)z;
            if (scene_cell_overlaps(t, cx, cy, cz)) {
                const uint32_t at = scene_cell_index(g, cx, cy, cz);   // (in range: the range is clamped to the grid)
                atomicAdd(&counts[at], 1u);
                if (geom) atomicMin(&geom[at], gid);
            }
        }
    }
}

// The launch is kSceneGridBigX x kSceneGridBigY blocks whatever the queue holds, and every block of a row repeats its triangle's
// load and set-up: right for few triangles of many tiles each.  A queue of thousands of one-tile triangles pays for it (EXPERIMENTS.md
// E22: 141 us at a threshold of 8 over SYN-1M); whoever lowers the threshold should give such entries a row of one block.
__global__ __launch_bounds__(kBlock) void k_scene_grid_big(SceneGrid g, const AttrGeom *__restrict__ table, uint32_t n_table, uint32_t n_tris,
                                                           uint32_t *__restrict__ counts, uint32_t *__restrict__ geom,
                                                           const uint32_t *__restrict__ queue_count, const uint2 *__restrict__ queue)
{
    const uint32_t n = min(*queue_count, n_tris);
    for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
        const uint2 item = queue[e];
        if (item.x >= n_table) continue;   // (k_scene_grid_small queued it from this table)
        const AttrGeom &ge = table[item.x];
        if (item.y >= (ge.quad ? 2u * ge.n_elems : ge.n_elems)) continue;
        SceneTri t;
        SceneRange r;
        if (!scene_tri_load(g, ge, item.y, t, r)) continue;
        const uint32_t tx = ((uint32_t)(r.hix - r.lox) / kSceneGridTile) + 1u, ty = ((uint32_t)(r.hiy - r.loy) / kSceneGridTile) + 1u,
                       tz = ((uint32_t)(r.hiz - r.loz) / kSceneGridTile) + 1u;
        const uint32_t tiles = tx * ty * tz;   // (at most 2^27 / 512 + the ragged ones: well below 2^32)
        for (uint32_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
            const int bx = r.lox + (int)((tile % tx) * kSceneGridTile), by = r.loy + (int)(((tile / tx) % ty) * kSceneGridTile),
                      bz = r.loz + (int)((tile / (tx * ty)) * kSceneGridTile);
            for (uint32_t c = threadIdx.x; c < kSceneGridTile * kSceneGridTile * kSceneGridTile; c += kBlock) {
                const int cx = bx + (int)(c & 7u), cy = by + (int)((c >> 3) & 7u), cz = bz + (int)(c >> 6);
                if (cx <= r.hix && cy <= r.hiy && cz <= r.hiz && scene_cell_overlaps(t, cx, cy, cz)) {
                    const uint32_t at = scene_cell_index(g, cx, cy, cz);
                    atomicAdd(&counts[at], 1u);
                    if (geom) atomicMin(&geom[at], item.x);
                }
            }
        }
    }
}

}  // namespace

void launch_scene_grid_clear(hipStream_t s, const SceneGrid &g, uint32_t *counts, uint32_t *geom, uint32_t *queue_count)
{
    const uint32_t n_cells = (g.flags & LS_SCENE_GRID_ACCUMULATE) ? 0u : g.n[0] * g.n[1] * g.n[2];
    const uint32_t lanes = max((n_cells + 3u) / 4u, 1u);
    hipLaunchKernelGGL(k_scene_grid_clear, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, s, reinterpret_cast<uint4 *>(counts), geom, n_cells,
                       queue_count);
}

void launch_scene_grid_small(hipStream_t s, const SceneGrid &g, const AttrGeom *table, uint32_t n_table, const uint32_t *tri_first, uint32_t n_tris,
                             const uint8_t *select, uint32_t n_select, uint32_t small, bool aggregate, uint32_t *counts, uint32_t *geom,
                             uint32_t *queue_count, uint2 *queue)
{
    if (!n_tris || !n_table) return;
    const dim3 grid((uint32_t)(((unsigned long long)n_tris + kBlock - 1) / kBlock));
    if (aggregate)
        hipLaunchKernelGGL(k_scene_grid_small<true>, grid, dim3(kBlock), 0, s, g, table, n_table, tri_first, n_tris, select, n_select, small, counts,
                           geom, queue_count, queue);
    else
        hipLaunchKernelGGL(k_scene_grid_small<false>, grid, dim3(kBlock), 0, s, g, table, n_table, tri_first, n_tris, select, n_select, small, counts,
                           geom, queue_count, queue);
}

void launch_scene_grid_big(hipStream_t s, const SceneGrid &g, const AttrGeom *table, uint32_t n_table, uint32_t n_tris, uint32_t *counts,
                           uint32_t *geom, const uint32_t *queue_count, const uint2 *queue)
{
    if (!n_tris || !n_table) return;
    hipLaunchKernelGGL(k_scene_grid_big, dim3(min(n_tris, kSceneGridBigX), kSceneGridBigY), dim3(kBlock), 0, s, g, table, n_table, n_tris, counts,
                       geom, queue_count, queue);
}

}  // namespace ls
