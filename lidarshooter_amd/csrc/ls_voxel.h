// ls_voxel.h -- the arithmetic of ls_occupancy_grid (include/lidarshooter_hip.h) that the kernel (k_voxel_carve,
// ls_voxel.hip) and the host (ls_debug_voxel_walk, ls_debug.cpp; the descriptor's check) both compile: ONE float32 operation
// sequence per ray -- the affine, the span a ray carves, its occupied cell and the walk over the cells of that span -- and what
// ls_voxel.hip gives the host code of the call (ls_voxel_host.cpp).
//
// Everything is float32 and every operation rounds once (the library is compiled with -ffp-contract=off).  fminf / fmaxf return
// the other operand for a NaN; every compare that lets the walk go on is written so that a NaN ends it.
//
// The walk has no reciprocal and no accumulated boundary: the parameter at which the ray leaves cell c along axis a is recomputed
// from c by one product, one difference and one division, so a walk of 2048 cells ends where a walk of 2 cells would.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lidarshooter_hip.h"
#include "ls_grid_box.h"
#include "ls_kernels.h"

#if defined(__HIPCC__)
#define LS_VOXEL_HD __host__ __device__ __forceinline__
#else
#define LS_VOXEL_HD inline
#endif

namespace ls {

constexpr uint32_t kVoxelFlags = LS_OCC_CARVE_MISSES | LS_OCC_ACCUMULATE;

// the descriptor as the kernels take it, with the call's transform next to it
struct VoxelGrid {
    float origin[3], cell;
    uint32_t n[3], flags;
    float min_range, max_range;
    uint32_t has_xf, pad;
    float xf[12];   // sensor -> grid, row-major 3 x 4 (read only with has_xf)
};

// What the call refuses of a descriptor and a transform (nullptr: none), in the header's order, as two steps -- the device entry
// point's alignment test stands between them.  voxel_args_invalid: the message of an LS_ERR_INVALID_ARGUMENT, or nullptr;
// voxel_grid_out_of_range: that of an LS_ERR_OUT_OF_RANGE.  The box's share of both is ls_grid_box.h's.
inline const char *voxel_args_invalid(const ls_occupancy_grid_desc &g, const float *xf)
{
    if ((g.flags & ~kVoxelFlags) || g.reserved[0] || g.reserved[1]) return "unknown flags or non-zero reserved words";
    if (const char *why = grid_box_invalid(g.origin, g.cell, xf)) return why;
    if (!isfinite(g.min_range) || !(g.min_range >= 0.0f)) return "min_range is not finite or negative";
    if (!isfinite(g.max_range) || !(g.max_range >= g.min_range)) return "max_range is not finite or below min_range";
    return nullptr;
}

inline const char *voxel_grid_out_of_range(const ls_occupancy_grid_desc &g) { return grid_box_out_of_range(g.origin, g.dims, g.cell); }

inline VoxelGrid voxel_grid(const ls_occupancy_grid_desc &g, const float *sensor_to_grid3x4)
{
    VoxelGrid v{};
    grid_set_box(v, g, sensor_to_grid3x4);
    v.flags = g.flags; v.min_range = g.min_range; v.max_range = g.max_range;
    return v;
}

// the ray in the grid's frame: ls_cloud_to_world's products and sums in its order, the direction without the translation
LS_VOXEL_HD void voxel_ray_to_grid(const float *m, float *o, float *d)
{
    const float ox = o[0], oy = o[1], oz = o[2], dx = d[0], dy = d[1], dz = d[2];
    o[0] = ((m[0] * ox + m[1] * oy) + m[2] * oz) + m[3];
    o[1] = ((m[4] * ox + m[5] * oy) + m[6] * oz) + m[7];
    o[2] = ((m[8] * ox + m[9] * oy) + m[10] * oz) + m[11];
    d[0] = (m[0] * dx + m[1] * dy) + m[2] * dz;
    d[1] = (m[4] * dx + m[5] * dy) + m[6] * dz;
    d[2] = (m[8] * dx + m[9] * dy) + m[10] * dz;
}

// one ray of the table in the header: has_t, t: its deciding record.  -> whether anything is carved, and on [*t0, *t1]; *occ: whether
// the record's point may mark a cell.  tmin <= tmax of a walkable ray; the grid's ranges are finite, so *t1 is
LS_VOXEL_HD bool voxel_span(const VoxelGrid &g, float tmin, float tmax, bool has_t, float t, float *t0, float *t1, bool *occ)
{
    *occ = false;
    *t0 = fmaxf(tmin, g.min_range);
    *t1 = fminf(tmax, g.max_range);
    if (!has_t) return (g.flags & LS_OCC_CARVE_MISSES) != 0u;
    if (t < g.min_range) return false;   // blocked in the blind zone
    if (t <= g.max_range) {
        *t1 = t;
        *occ = true;
    }
    return true;
}

constexpr uint32_t kVoxelNone = 0xFFFFFFFFu;

// the cell of the point p, or kVoxelNone outside the grid: floorf((p - origin) / cell) per axis, compared as floats before any cast
LS_VOXEL_HD uint32_t voxel_cell_of(const VoxelGrid &g, float px, float py, float pz)
{
    const float fx = floorf((px - g.origin[0]) / g.cell), fy = floorf((py - g.origin[1]) / g.cell), fz = floorf((pz - g.origin[2]) / g.cell);
    if (!(fx >= 0.0f && fx < (float)g.n[0] && fy >= 0.0f && fy < (float)g.n[1] && fz >= 0.0f && fz < (float)g.n[2])) return kVoxelNone;
    const uint32_t cz = (uint32_t)fz, cy = (uint32_t)fy, cx = (uint32_t)fx;
    return grid_cell_index(g.n, (int)cx, (int)cy, (int)cz);
}

// the record's point: one product and one sum per axis; a handle's own ray without a transform starts at the origin and has no sum
// (the bits of the frame's points32)
LS_VOXEL_HD uint32_t voxel_occupied_cell(const VoxelGrid &g, const float *o, const float *d, float t, bool no_sum)
{
    const float px = no_sum ? t * d[0] : o[0] + t * d[0];
    const float py = no_sum ? t * d[1] : o[1] + t * d[1];
    const float pz = no_sum ? t * d[2] : o[2] + t * d[2];
    return voxel_cell_of(g, px, py, pz);
}

// the walk's state: named scalars, so that the device keeps them in registers
struct VoxelWalk {
    float q0, q1, q2, d0, d1, d2;   // origin relative to the grid's corner, direction
    float b0, b1, b2;               // the parameter at which the ray leaves the current cell along each axis (+inf: never)
    float t_out;
    int c0, c1, c2;
    uint32_t left;                  // trips the walk may still take (the hard cap: nx + ny + nz)
    bool live;                      // (c0, c1, c2) is a cell to visit
};

LS_VOXEL_HD float voxel_boundary(int c, float q, float d, float cell) { return ((float)(c + (d > 0.0f ? 1 : 0)) * cell - q) / d; }

LS_VOXEL_HD uint32_t voxel_index(const VoxelGrid &g, const VoxelWalk &w) { return grid_cell_index(g.n, w.c0, w.c1, w.c2); }

// clip [t0, t1] of the ray (o, d) against the grid and find its first cell; w.live = false: no cells
LS_VOXEL_HD void voxel_walk_begin(const VoxelGrid &g, const float *o, const float *d, float t0, float t1, VoxelWalk &w)
{
    w.q0 = o[0] - g.origin[0]; w.q1 = o[1] - g.origin[1]; w.q2 = o[2] - g.origin[2];
    w.d0 = d[0]; w.d1 = d[1]; w.d2 = d[2];
    w.b0 = w.b1 = w.b2 = INFINITY;
    w.c0 = w.c1 = w.c2 = 0;
    w.left = g.n[0] + g.n[1] + g.n[2];
    const float E0 = (float)g.n[0] * g.cell, E1 = (float)g.n[1] * g.cell, E2 = (float)g.n[2] * g.cell;
    float t_in = t0, t_out = t1;
    bool ok = true;
    auto slab = [&](float q, float dd, float E) {
        if (dd == 0.0f) {
            if (!(q >= 0.0f && q < E)) ok = false;
            return;
        }
        const float ta = (0.0f - q) / dd, tb = (E - q) / dd;
        t_in = fmaxf(t_in, fminf(ta, tb));
        t_out = fminf(t_out, fmaxf(ta, tb));
    };
    slab(w.q0, w.d0, E0);
    slab(w.q1, w.d1, E1);
    slab(w.q2, w.d2, E2);
    w.t_out = t_out;
    w.live = ok && t_in <= t_out;
    if (!w.live) return;
    auto first = [&](float q, float dd, uint32_t n) {
        const float e = q + t_in * dd;
        float f = floorf(e / g.cell);
        f = fminf(fmaxf(f, 0.0f), (float)(n - 1u));
        return (int)f;
    };
    w.c0 = first(w.q0, w.d0, g.n[0]);
    w.c1 = first(w.q1, w.d1, g.n[1]);
    w.c2 = first(w.q2, w.d2, g.n[2]);
    if (w.d0 != 0.0f) w.b0 = voxel_boundary(w.c0, w.q0, w.d0, g.cell);
    if (w.d1 != 0.0f) w.b1 = voxel_boundary(w.c1, w.q1, w.d1, g.cell);
    if (w.d2 != 0.0f) w.b2 = voxel_boundary(w.c2, w.q2, w.d2, g.cell);
}

// from the cell just visited to the next one; w.live = false: the walk is over.  Ties go to x, then y, then z
LS_VOXEL_HD void voxel_walk_next(const VoxelGrid &g, VoxelWalk &w)
{
    int a = 0;
    float b = w.b0;
    if (w.b1 < b) { a = 1; b = w.b1; }
    if (w.b2 < b) { a = 2; b = w.b2; }
    if (!(b <= w.t_out) || --w.left == 0u) { w.live = false; return; }
    if (a == 0) {
        w.c0 += w.d0 > 0.0f ? 1 : -1;
        if (w.c0 < 0 || w.c0 >= (int)g.n[0]) { w.live = false; return; }
        w.b0 = voxel_boundary(w.c0, w.q0, w.d0, g.cell);
    } else if (a == 1) {
        w.c1 += w.d1 > 0.0f ? 1 : -1;
        if (w.c1 < 0 || w.c1 >= (int)g.n[1]) { w.live = false; return; }
        w.b1 = voxel_boundary(w.c1, w.q1, w.d1, g.cell);
    } else {
        w.c2 += w.d2 > 0.0f ? 1 : -1;
        if (w.c2 < 0 || w.c2 >= (int)g.n[2]) { w.live = false; return; }
        w.b2 = voxel_boundary(w.c2, w.q2, w.d2, g.cell);
    }
}

// ---- the launches of ls_voxel.hip --------------------------------------------------------------------------------------------------

// every cell's {n_free, n_occ} to zero and its geom word (nullptr: none) to 0xFFFFFFFF unless LS_OCC_ACCUMULATE is set, and the
// n_keys per-ray keys to ~0
void launch_voxel_clear(hipStream_t s, const VoxelGrid &g, void *counts, uint32_t *geom, unsigned long long *keys, uint32_t n_keys);
// over n ls_hit records (min(n, *d_count) with a device count): a record that counts -- ls_object_labels' rule -- sends
// (t bits << 32) | geom to its ray's key by atomicMin: the smallest t, then the lowest geomID.  own_rays: hit.ray indexes the
// handle's full raster (tb); otherwise the n_rays 32-byte caller rays.  table, n_table: launch_hit_attributes'.
void launch_voxel_ends(hipStream_t s, const void *hits, const uint32_t *d_count, uint32_t n, const void *rays, uint32_t n_rays, bool own_rays,
                       const SensorTables &tb, const AttrGeom *table, uint32_t n_table, unsigned long long *keys);
// one lane per ray: the span, the occupied cell and the walk; integer atomics into counts and geom.  aggregate: a wave adds one
// atomic per run of adjacent lanes that stand in the same cell (the same bytes either way)
void launch_voxel_carve(hipStream_t s, const VoxelGrid &g, const void *rays, uint32_t n_rays, bool own_rays, const SensorTables &tb,
                        const unsigned long long *keys, void *counts, uint32_t *geom, bool aggregate);

}  // namespace ls
