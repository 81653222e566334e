// ls_distance_grid.h -- the arithmetic of ls_scene_distance_grid (include/lidarshooter_hip.h) that the kernels
// (k_distance_grid_small, k_distance_grid_big: ls_distance_grid.hip) and the host (ls_debug_distance_grid_triangle, ls_debug.cpp; the
// descriptor's check) both compile: ONE float32 operation sequence per triangle and per cell, and what ls_distance_grid.hip gives
// the host code of the call (ls_distance_grid_host.cpp).
//
// Everything is float32 and every operation rounds once (the library is compiled with -ffp-contract=off).  Per triangle, v_k its
// three vertices in the grid's frame:
//   1. q_k = v_k - origin per axis; a triangle with a non-finite q is skipped;
//   2. per axis a: lo_a = floorf((min_k q_k[a] - trunc) / cell), hi_a = floorf((max_k q_k[a] + trunc) / cell), compared as floats
//      before any cast: the triangle is skipped if hi_a < 0 or lo_a >= n_a, otherwise both are clamped to [0, n_a - 1];
//   3. per cell c of that range: ctr_a = ((float)c_a + 0.5f) * cell (scene_cell_overlaps' centre), closest_on_triangle(ctr, q_0, q_1,
//      q_2) of ls_closest.h as it stands gives d2; the pair counts iff d2 is finite and dist = sqrtf(d2) <= trunc.
// A triangle without area never counts (closest_on_triangle skips it) -- unlike ls_scene_grid, where a segment marks cells.
// The kernels call closest_on_triangle through its pointers: the arrays it reads are locals of the inlined caller, which the
// compiler keeps in registers (no scratch: DESIGN.md 3.3.16 has the resource lines).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lidarshooter_hip.h"
#include "ls_closest.h"
#include "ls_grid_box.h"
#include "ls_kernels.h"
#include "ls_scene_grid.h"

#if defined(__HIPCC__)
#define LS_DGRID_HD __host__ __device__ __forceinline__
#else
#define LS_DGRID_HD inline
#endif

namespace ls {

constexpr uint32_t kDistGridFlags = LS_DIST_GRID_ACCUMULATE;
constexpr float kDistGridMaxBand = 32.0f;                         // trunc <= 32 cells: the work per triangle stays bounded
constexpr unsigned long long kDistGridRest = 0x7F800000FFFFFFFFull;   // {0xFFFFFFFF, +inf}: no surface within trunc
constexpr uint32_t kDistGridChunk = 256;   // k_distance_grid_big: a chunk is 256 consecutive cells of a range, a lane each (= kBlock)
constexpr uint32_t kDistGridBigX = 256;    // ... its launch, k_scene_grid_big's: 256 x 32 blocks at most, one to 32 of them per queued triangle
constexpr uint32_t kDistGridBigY = 32;     // (a power of two)

// the descriptor as the kernels take it, with the call's transform next to it
struct DistGrid {
    float origin[3], cell;
    uint32_t n[3], flags;
    float trunc;
    uint32_t has_xf, pad[2];
    float xf[12];   // sensor -> grid, row-major 3 x 4 (read only with has_xf)
};

// What the call refuses of a descriptor and a transform (nullptr: none), in the header's order, as two steps -- the device entry
// point's alignment test stands between them: the message of an LS_ERR_INVALID_ARGUMENT, then that of an LS_ERR_OUT_OF_RANGE
inline const char *dist_grid_args_invalid(const ls_distance_grid_desc &g, const float *xf)
{
    if ((g.flags & ~kDistGridFlags) || g.reserved[0] || g.reserved[1] || g.reserved[2]) return "unknown flags or non-zero reserved words";
    if (const char *why = grid_box_invalid(g.origin, g.cell, xf)) return why;
    if (!isfinite(g.trunc) || !(g.trunc >= 0.0f)) return "trunc is not finite or negative";
    return nullptr;
}

inline const char *dist_grid_out_of_range(const ls_distance_grid_desc &g)
{
    if (const char *why = grid_box_out_of_range(g.origin, g.dims, g.cell)) return why;
    if (g.trunc > kDistGridMaxBand * g.cell) return "trunc above 32 cells";
    return nullptr;
}

inline DistGrid dist_grid(const ls_distance_grid_desc &g, const float *sensor_to_grid3x4)
{
    DistGrid v{};
    grid_set_box(v, g, sensor_to_grid3x4);
    v.flags = g.flags; v.trunc = g.trunc;
    return v;
}

// a triangle as the cells' test reads it: the vertices relative to the grid's corner
struct DistTri {
    float q0[3], q1[3], q2[3];
};

// one axis of step 2; false: the triangle's band lies outside the grid along it
LS_DGRID_HD bool dist_axis_range(float a, float b, float c, float trunc, float cell, uint32_t n, int *lo, int *hi)
{
    const float l = floorf((fminf(fminf(a, b), c) - trunc) / cell), u = floorf((fmaxf(fmaxf(a, b), c) + trunc) / cell);
    if (u < 0.0f || l >= (float)n) return false;
    *lo = (int)fminf(fmaxf(l, 0.0f), (float)(n - 1u));
    *hi = (int)fminf(fmaxf(u, 0.0f), (float)(n - 1u));
    return true;
}

// steps 1 and 2.  v: the nine coordinates in the grid's frame.  false: skipped
LS_DGRID_HD bool dist_tri_setup(const DistGrid &g, float v0x, float v0y, float v0z, float v1x, float v1y, float v1z, float v2x, float v2y,
                                float v2z, DistTri &t, SceneRange &r)
{
    t.q0[0] = v0x - g.origin[0]; t.q0[1] = v0y - g.origin[1]; t.q0[2] = v0z - g.origin[2];
    t.q1[0] = v1x - g.origin[0]; t.q1[1] = v1y - g.origin[1]; t.q1[2] = v1z - g.origin[2];
    t.q2[0] = v2x - g.origin[0]; t.q2[1] = v2y - g.origin[1]; t.q2[2] = v2z - g.origin[2];
    if (!(isfinite(t.q0[0]) && isfinite(t.q0[1]) && isfinite(t.q0[2]) && isfinite(t.q1[0]) && isfinite(t.q1[1]) && isfinite(t.q1[2]) &&
          isfinite(t.q2[0]) && isfinite(t.q2[1]) && isfinite(t.q2[2])))
        return false;
    if (!dist_axis_range(t.q0[0], t.q1[0], t.q2[0], g.trunc, g.cell, g.n[0], &r.lox, &r.hix)) return false;
    if (!dist_axis_range(t.q0[1], t.q1[1], t.q2[1], g.trunc, g.cell, g.n[1], &r.loy, &r.hiy)) return false;
    return dist_axis_range(t.q0[2], t.q1[2], t.q2[2], g.trunc, g.cell, g.n[2], &r.loz, &r.hiz);
}

// step 3: whether cell (cx, cy, cz) counts for the triangle, and with which distance
LS_DGRID_HD bool dist_cell(const DistTri &t, float trunc, float cell, int cx, int cy, int cz, float *dist)
{
    const float p[3] = {((float)cx + 0.5f) * cell, ((float)cy + 0.5f) * cell, ((float)cz + 0.5f) * cell};
    float q[3], d2;
    closest_on_triangle(p, t.q0, t.q1, t.q2, q, &d2);
    if (!isfinite(d2)) return false;
    *dist = sqrtf(d2);
    return *dist <= trunc;
}

LS_DGRID_HD uint32_t dist_cell_index(const DistGrid &g, int cx, int cy, int cz) { return grid_cell_index(g.n, cx, cy, cz); }

// step 4: what a counting pair sends to its cell.  dist >= 0: its bits ascend with it
LS_DGRID_HD unsigned long long dist_key(uint32_t dist_bits, uint32_t geom) { return ((unsigned long long)dist_bits << 32) | geom; }

// ---- the launches of ls_distance_grid.hip ------------------------------------------------------------------------------------------

// every record to kDistGridRest unless LS_DIST_GRID_ACCUMULATE is set, and the queue's count word to zero
void launch_distance_grid_clear(hipStream_t s, const DistGrid &g, unsigned long long *cells, uint32_t *queue_count);
// one wave per triangle of the table (tri_first[geom] .. tri_first[geom + 1], n_table + 1 words; n_tris = tri_first[n_table]); a
// geometry whose select byte is 0 is left out.  A range of at most `small` cells is tested by the wave, its lanes striding over the
// cells; a larger one is appended to queue (8 bytes per triangle of the scene behind the count word).  preread: a lane reads the
// cell's word first and sends nothing when it is already <= its key (the same bytes either way)
void launch_distance_grid_small(hipStream_t s, const DistGrid &g, const AttrGeom *table, uint32_t n_table, const uint32_t *tri_first,
                                uint32_t n_tris, const uint8_t *select, uint32_t n_select, uint32_t small, bool preread, unsigned long long *cells,
                                uint32_t *queue_count, uint2 *queue);
// the queued triangles, one to 32 blocks per triangle over its range's chunks of 256 cells; the count is read on the device
void launch_distance_grid_big(hipStream_t s, const DistGrid &g, const AttrGeom *table, uint32_t n_table, uint32_t n_tris, bool preread,
                              unsigned long long *cells, const uint32_t *queue_count, const uint2 *queue);

}  // namespace ls
