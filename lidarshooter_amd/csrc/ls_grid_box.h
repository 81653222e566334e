// ls_grid_box.h -- what ls_occupancy_grid, ls_scene_grid and ls_scene_distance_grid mean by "a grid" (DESIGN.md 3.3.14): an origin,
// a cell edge, three dimensions and the call's optional transform into its frame.  What every descriptor's check refuses of them,
// the limits, the index of a cell, and how the descriptor's box reaches the struct the kernels take -- compiled by the kernels, by
// the host code of the calls and by ls_debug.cpp.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LS_GRID_HD __host__ __device__ __forceinline__
#else
#define LS_GRID_HD inline
#endif

namespace ls {

constexpr uint32_t kVoxelMaxDim = 2048;          // cells per axis
constexpr uint32_t kVoxelMaxCells = 1u << 27;    // cells of a grid

// the origin, the transform (nullptr: none) and the cell edge, in the headers' order: the message of an LS_ERR_INVALID_ARGUMENT, or
// nullptr
inline const char *grid_box_invalid(const float origin[3], float cell, const float *xf)
{
    if (!isfinite(origin[0]) || !isfinite(origin[1]) || !isfinite(origin[2])) return "the grid's origin is not finite";
    for (int k = 0; xf && k < 12; ++k)
        if (!isfinite(xf[k])) return "sensor_to_grid is not finite";
    if (!isfinite(cell) || !(cell > 0.0f)) return "the cell edge is not a finite positive number";
    return nullptr;
}

// the dimensions and the upper corner of a box that passed grid_box_invalid: the message of an LS_ERR_OUT_OF_RANGE, or nullptr
inline const char *grid_box_out_of_range(const float origin[3], const uint32_t dims[3], float cell)
{
    unsigned long long cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] == 0 || dims[a] > kVoxelMaxDim) return "a grid dimension of 0 or above 2048";
        cells *= dims[a];
    }
    if (cells > kVoxelMaxCells) return "more than 2^27 cells";
    for (int a = 0; a < 3; ++a)
        if (!isfinite(origin[a] + (float)dims[a] * cell)) return "the grid's upper corner is not finite";
    return nullptr;
}

// cell (cx, cy, cz) of a grid of n cells per axis, x fastest (in range: below 2^27)
LS_GRID_HD uint32_t grid_cell_index(const uint32_t n[3], int cx, int cy, int cz) { return ((uint32_t)cz * n[1] + (uint32_t)cy) * n[0] + (uint32_t)cx; }

inline size_t grid_cells(const uint32_t dims[3]) { return (size_t)dims[0] * dims[1] * dims[2]; }

// the call's transform in a kernel-side struct (has_xf, xf[12]); zeros without one
template <typename Args>
inline void grid_set_xf(Args &v, const float *xf3x4)
{
    v.has_xf = xf3x4 ? 1u : 0u;
    for (int k = 0; k < 12; ++k) v.xf[k] = xf3x4 ? xf3x4[k] : 0.0f;
}

// a descriptor's box (origin, dims, cell) and the call's transform in a kernel-side struct (origin, n, cell; has_xf, xf)
template <typename Grid, typename Desc>
inline void grid_set_box(Grid &v, const Desc &g, const float *xf3x4)
{
    for (int a = 0; a < 3; ++a) { v.origin[a] = g.origin[a]; v.n[a] = g.dims[a]; }
    v.cell = g.cell;
    grid_set_xf(v, xf3x4);
}

}  // namespace ls
