// ls_scene_grid.h -- the arithmetic of ls_scene_grid (include/lidarshooter_hip.h) that the kernels
// (k_scene_grid_small, k_scene_grid_big: ls_scene_grid.hip) and the host (ls_debug_scene_grid_triangle, ls_debug.cpp; the
// descriptor's check) both compile: ONE float32 operation sequence per triangle and per cell, and what ls_scene_grid.hip gives
// the host code of the call (ls_scene_grid_host.cpp).
//
// Everything is float32 and every operation rounds once (the library is compiled with -ffp-contract=off).  Per triangle, v_k its
// three vertices in the grid's frame:
//   1. q_k = v_k - origin per axis; a triangle with a non-finite q is skipped;
//   2. per axis a: lo_a = floorf(min_k q_k[a] / cell), hi_a = floorf(max_k q_k[a] / cell), compared as floats before any cast:
//      the triangle is skipped if hi_a < 0 or lo_a >= n_a, otherwise both are clamped to [0, n_a - 1];
//   3. per cell c of that range: ctr_a = ((float)c_a + 0.5f) * cell, h = 0.5f * cell, p_k = q_k - ctr; the edges come from q, not
//      from p: e0 = q1 - q0, e1 = q2 - q1, e2 = q0 - q2;
//   4. the cell overlaps unless one of 13 axes separates:
//      the 3 box axes: min_k p_k[a] > h or max_k p_k[a] < -h;
//      the 9 axes unit_i x e_j: for i = x the projection of vertex k is (e_y * p_k.z) - (e_z * p_k.y) and r = h * (|e_z| + |e_y|);
//      for i = y it is (e_z * p_k.x) - (e_x * p_k.z) and r = h * (|e_x| + |e_z|); for i = z it is (e_x * p_k.y) - (e_y * p_k.x) and
//      r = h * (|e_y| + |e_x|); all three vertices are projected; the axis separates if min > r or max < -r;
//      the plane axis: n = cross(e0, e1) as products and differences, d = ((n.x * p_0.x) + (n.y * p_0.y)) + (n.z * p_0.z),
//      r = h * ((|n.x| + |n.y|) + |n.z|); it separates if d > r or d < -r.
// "min > r" is written as "every one of the three > r" and "max < -r" as "every one of the three < -r": with finite values the
// same, and a NaN (a product that overflowed twice) never separates.  The box is closed, but the range is floorf's: a triangle
// that ends on a cell's face plane reaches the cell above the plane and touches it, one that begins on it does not reach the cell
// below.  A segment or a point needs no special case: its cross axes are zero and never separate.
// The edges, the normal and the ten radii do not depend on the cell: they are made once per triangle (scene_tri_setup).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lidarshooter_hip.h"
#include "ls_grid_box.h"
#include "ls_kernels.h"

#if defined(__HIPCC__)
#define LS_SGRID_HD __host__ __device__ __forceinline__
#else
#define LS_SGRID_HD inline
#endif

namespace ls {

constexpr uint32_t kSceneGridFlags = LS_SCENE_GRID_ACCUMULATE;
constexpr uint32_t kSceneGridTile = 8;      // k_scene_grid_big: a tile is 8 x 8 x 8 cells
constexpr uint32_t kSceneGridBigX = 256;    // ... its launch: blockIdx.x strides over the queue, blockIdx.y over a triangle's tiles
constexpr uint32_t kSceneGridBigY = 32;

// the descriptor as the kernels take it, with the call's transform next to it
struct SceneGrid {
    float origin[3], cell;
    uint32_t n[3], flags;
    uint32_t has_xf, pad[3];
    float xf[12];   // sensor -> grid, row-major 3 x 4 (read only with has_xf)
};

// What the call refuses of a descriptor and a transform (nullptr: none), in the header's order, as two steps -- the device entry
// point's alignment test stands between them: the message of an LS_ERR_INVALID_ARGUMENT, then that of an LS_ERR_OUT_OF_RANGE
inline const char *scene_grid_args_invalid(const ls_scene_grid_desc &g, const float *xf)
{
    if (g.flags & ~kSceneGridFlags) return "unknown flags";
    return grid_box_invalid(g.origin, g.cell, xf);
}

inline const char *scene_grid_out_of_range(const ls_scene_grid_desc &g) { return grid_box_out_of_range(g.origin, g.dims, g.cell); }

inline SceneGrid scene_grid(const ls_scene_grid_desc &g, const float *sensor_to_grid3x4)
{
    SceneGrid v{};
    grid_set_box(v, g, sensor_to_grid3x4);
    v.flags = g.flags;
    return v;
}

// a triangle as the cells' test reads it: named scalars, so that the device keeps them in registers
struct SceneTri {
    float q0x, q0y, q0z, q1x, q1y, q1z, q2x, q2y, q2z;   // the vertices relative to the grid's corner
    float e0x, e0y, e0z, e1x, e1y, e1z, e2x, e2y, e2z;   // q1 - q0, q2 - q1, q0 - q2
    float nx, ny, nz;                                    // cross(e0, e1)
    float rx0, ry0, rz0, rx1, ry1, rz1, rx2, ry2, rz2;   // the radius of axis unit_i x e_j: r<i><j>
    float rn, h, cell;
};

// the clamped cell range of a triangle, inclusive
struct SceneRange {
    int lox, hix, loy, hiy, loz, hiz;
};

LS_SGRID_HD uint32_t scene_range_cells(const SceneRange &r)
{
    return (uint32_t)(r.hix - r.lox + 1) * (uint32_t)(r.hiy - r.loy + 1) * (uint32_t)(r.hiz - r.loz + 1);   // (at most 2^27)
}

// one axis of step 2; false: the triangle lies outside the grid along it
LS_SGRID_HD bool scene_axis_range(float a, float b, float c, float cell, uint32_t n, int *lo, int *hi)
{
    const float l = floorf(fminf(fminf(a, b), c) / cell), u = floorf(fmaxf(fmaxf(a, b), c) / cell);
    if (u < 0.0f || l >= (float)n) return false;
    *lo = (int)fminf(fmaxf(l, 0.0f), (float)(n - 1u));
    *hi = (int)fminf(fmaxf(u, 0.0f), (float)(n - 1u));
    return true;
}

// steps 1 and 2 and what step 4 needs of the triangle alone.  v: the nine coordinates in the grid's frame.  false: skipped
LS_SGRID_HD bool scene_tri_setup(const SceneGrid &g, float v0x, float v0y, float v0z, float v1x, float v1y, float v1z, float v2x, float v2y,
                                 float v2z, SceneTri &t, SceneRange &r)
{
    t.q0x = v0x - g.origin[0]; t.q0y = v0y - g.origin[1]; t.q0z = v0z - g.origin[2];
    t.q1x = v1x - g.origin[0]; t.q1y = v1y - g.origin[1]; t.q1z = v1z - g.origin[2];
    t.q2x = v2x - g.origin[0]; t.q2y = v2y - g.origin[1]; t.q2z = v2z - g.origin[2];
    if (!(isfinite(t.q0x) && isfinite(t.q0y) && isfinite(t.q0z) && isfinite(t.q1x) && isfinite(t.q1y) && isfinite(t.q1z) && isfinite(t.q2x) &&
          isfinite(t.q2y) && isfinite(t.q2z)))
        return false;
    if (!scene_axis_range(t.q0x, t.q1x, t.q2x, g.cell, g.n[0], &r.lox, &r.hix)) return false;
    if (!scene_axis_range(t.q0y, t.q1y, t.q2y, g.cell, g.n[1], &r.loy, &r.hiy)) return false;
    if (!scene_axis_range(t.q0z, t.q1z, t.q2z, g.cell, g.n[2], &r.loz, &r.hiz)) return false;
    t.cell = g.cell;
    t.h = 0.5f * g.cell;
    t.e0x = t.q1x - t.q0x; t.e0y = t.q1y - t.q0y; t.e0z = t.q1z - t.q0z;
    t.e1x = t.q2x - t.q1x; t.e1y = t.q2y - t.q1y; t.e1z = t.q2z - t.q1z;
    t.e2x = t.q0x - t.q2x; t.e2y = t.q0y - t.q2y; t.e2z = t.q0z - t.q2z;
    t.rx0 = t.h * (fabsf(t.e0z) + fabsf(t.e0y)); t.ry0 = t.h * (fabsf(t.e0x) + fabsf(t.e0z)); t.rz0 = t.h * (fabsf(t.e0y) + fabsf(t.e0x));
    t.rx1 = t.h * (fabsf(t.e1z) + fabsf(t.e1y)); t.ry1 = t.h * (fabsf(t.e1x) + fabsf(t.e1z)); t.rz1 = t.h * (fabsf(t.e1y) + fabsf(t.e1x));
    t.rx2 = t.h * (fabsf(t.e2z) + fabsf(t.e2y)); t.ry2 = t.h * (fabsf(t.e2x) + fabsf(t.e2z)); t.rz2 = t.h * (fabsf(t.e2y) + fabsf(t.e2x));
    t.nx = (t.e0y * t.e1z) - (t.e0z * t.e1y);
    t.ny = (t.e0z * t.e1x) - (t.e0x * t.e1z);
    t.nz = (t.e0x * t.e1y) - (t.e0y * t.e1x);
    t.rn = t.h * ((fabsf(t.nx) + fabsf(t.ny)) + fabsf(t.nz));
    return true;
}

// whether the interval spanned by a, b, c lies wholly beyond [-r, r]: no NaN makes it true
LS_SGRID_HD bool scene_separates(float a, float b, float c, float r)
{
    const float m = -r;
    return (a > r && b > r && c > r) || (a < m && b < m && c < m);
}

// the three axes unit_x x e, unit_y x e, unit_z x e of one edge e against the vertices p_k
LS_SGRID_HD bool scene_edge_separates(float ex, float ey, float ez, float rx, float ry, float rz, float p0x, float p0y, float p0z, float p1x,
                                      float p1y, float p1z, float p2x, float p2y, float p2z)
{
    if (scene_separates((ey * p0z) - (ez * p0y), (ey * p1z) - (ez * p1y), (ey * p2z) - (ez * p2y), rx)) return true;
    if (scene_separates((ez * p0x) - (ex * p0z), (ez * p1x) - (ex * p1z), (ez * p2x) - (ex * p2z), ry)) return true;
    return scene_separates((ex * p0y) - (ey * p0x), (ex * p1y) - (ey * p1x), (ex * p2y) - (ey * p2x), rz);
}

// steps 3 and 4: whether the triangle overlaps cell (cx, cy, cz)
LS_SGRID_HD bool scene_cell_overlaps(const SceneTri &t, int cx, int cy, int cz)
{
    const float ctrx = ((float)cx + 0.5f) * t.cell, ctry = ((float)cy + 0.5f) * t.cell, ctrz = ((float)cz + 0.5f) * t.cell;
    const float p0x = t.q0x - ctrx, p0y = t.q0y - ctry, p0z = t.q0z - ctrz;
    const float p1x = t.q1x - ctrx, p1y = t.q1y - ctry, p1z = t.q1z - ctrz;
    const float p2x = t.q2x - ctrx, p2y = t.q2y - ctry, p2z = t.q2z - ctrz;
    if (scene_separates(p0x, p1x, p2x, t.h) || scene_separates(p0y, p1y, p2y, t.h) || scene_separates(p0z, p1z, p2z, t.h)) return false;
    if (scene_edge_separates(t.e0x, t.e0y, t.e0z, t.rx0, t.ry0, t.rz0, p0x, p0y, p0z, p1x, p1y, p1z, p2x, p2y, p2z)) return false;
    if (scene_edge_separates(t.e1x, t.e1y, t.e1z, t.rx1, t.ry1, t.rz1, p0x, p0y, p0z, p1x, p1y, p1z, p2x, p2y, p2z)) return false;
    if (scene_edge_separates(t.e2x, t.e2y, t.e2z, t.rx2, t.ry2, t.rz2, p0x, p0y, p0z, p1x, p1y, p1z, p2x, p2y, p2z)) return false;
    const float d = ((t.nx * p0x) + (t.ny * p0y)) + (t.nz * p0z);
    return !(d > t.rn || d < -t.rn);
}

LS_SGRID_HD uint32_t scene_cell_index(const SceneGrid &g, int cx, int cy, int cz) { return grid_cell_index(g.n, cx, cy, cz); }

// ---- the launches of ls_scene_grid.hip ---------------------------------------------------------------------------------------------

// every count to zero and every geom word (nullptr: none) to 0xFFFFFFFF unless LS_SCENE_GRID_ACCUMULATE is set, and the queue's
// count word to zero
void launch_scene_grid_clear(hipStream_t s, const SceneGrid &g, uint32_t *counts, uint32_t *geom, uint32_t *queue_count);
// one lane per triangle of the table (tri_first[geom] .. tri_first[geom + 1], n_table + 1 words; n_tris = tri_first[n_table]); a
// geometry whose select byte is 0 is left out.  A range of at most `small` cells is tested by the lane, a larger one appended to
// queue (8 bytes per triangle of the scene behind the count word).  aggregate: a wave adds one atomic per run of adjacent lanes
// that mark the same cell (the same bytes either way)
void launch_scene_grid_small(hipStream_t s, const SceneGrid &g, const AttrGeom *table, uint32_t n_table, const uint32_t *tri_first, uint32_t n_tris,
                             const uint8_t *select, uint32_t n_select, uint32_t small, bool aggregate, uint32_t *counts, uint32_t *geom,
                             uint32_t *queue_count, uint2 *queue);
// the queued triangles, a block per (triangle, tile of 8 x 8 x 8 cells); the count is read on the device
void launch_scene_grid_big(hipStream_t s, const SceneGrid &g, const AttrGeom *table, uint32_t n_table, uint32_t n_tris, uint32_t *counts,
                           uint32_t *geom, const uint32_t *queue_count, const uint2 *queue);

}  // namespace ls
