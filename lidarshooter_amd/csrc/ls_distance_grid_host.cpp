// ls_distance_grid_host.cpp -- ls_scene_distance_grid, its host-memory variant and the descriptor's check: per cell of a voxel grid
// the distance from its centre to the nearest surface of the committed scene within a truncation distance, and whose it is
// (ls_distance_grid.hip; the arithmetic is ls_distance_grid.h).  The scene is the flat triangle index (scene_tris_prepare;
// ls_scene_tris.h); the call's place among what the handle issues is that of every query (query_enter / query_leave).  No hierarchy
// is touched and LS_INFO_RAY_QUERY_BUILT is left as it is.
#include "ls_internal.h"
#include "ls_distance_grid.h"

namespace lsi {

namespace {

// A triangle whose widened range holds more cells than this goes to k_distance_grid_big's queue; below it one wave works the range
// off, 64 cells a trip.  The queue is for the few triangles of a very large range (a ground triangle under a fine grid), not for a
// dense mesh under a wide band: 82 trips at most per wave, and EXPERIMENTS.md E24 measured what a lower threshold costs SYN-1M.  A
// lane reads a cell's word before it sends its key and sends nothing when the word is already as small: below the plain form by
// more than the spreads at both bands measured there.  The same bytes whatever the two say.  An EXPERIMENTAL build reads the knobs at
// every call, so that tools/distance_grid_cost.py can alternate the forms in one process.
constexpr int kDistGridSmall = 5247;
constexpr int kDistGridPreread = 1;

// what the device entry point and the host-memory variant (any alignment) refuse, in this order
int dist_grid_check(ls_tracer *tr, const ls_distance_grid_desc *grid, const float *xf, const uint8_t *select, uint32_t n_select, const void *cells,
                    bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!grid) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null grid descriptor");
    if (!cells) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null cells");
    if (n_select && !select) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null select with n_select > 0");
    if (const char *why = ls::dist_grid_args_invalid(*grid, xf)) return fail(tr, LS_ERR_INVALID_ARGUMENT, why);
    if (!host && misaligned(cells, 16)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "cells must be 16-byte aligned");
    if (const char *why = ls::dist_grid_out_of_range(*grid)) return fail(tr, LS_ERR_OUT_OF_RANGE, why);
    return uncommitted(tr);
}

int dist_grid_issue(ls_tracer *tr, hipStream_t s, const ls::DistGrid &g, const uint8_t *d_select, uint32_t n_select, void *d_cells)
{
    const ls_tracer::HitAttr &a = tr->ha;
    int rc;
    uint32_t n_table, n_tris, *count;
    uint2 *queue;
    if ((rc = scene_tris_prepare(tr, s, 0xFFFFFFFFull, "more than 2^32 triangles", &n_table, &n_tris))) return rc;
    if ((rc = scene_queue_ensure(tr, tr->rq.dist_queue, n_tris, &count, &queue))) return rc;
    unsigned long long *cells = static_cast<unsigned long long *>(d_cells);
    const int small = tune_int("LS_DIST_GRID_SMALL", kDistGridSmall);
    const bool preread = tune_int("LS_DIST_GRID_PREREAD", kDistGridPreread) != 0;
    ls::launch_distance_grid_clear(s, g, cells, count);
    if (tune_int("LS_DIST_GRID_CLEAR_ONLY", 0)) return LS_OK;   // (the cost tool's floor: the clear alone)
    ls::launch_distance_grid_small(s, g, a.table.dev.p, n_table, a.tri_first.dev.p, n_tris, d_select, n_select, small < 0 ? 0u : (uint32_t)small,
                                   preread, cells, count, queue);
    ls::launch_distance_grid_big(s, g, a.table.dev.p, n_table, n_tris, preread, cells, count, queue);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

}  // namespace

}  // namespace lsi

using namespace lsi;

extern "C" {

int ls_scene_distance_grid_check(const ls_distance_grid_desc *grid)
{
    if (!grid) return LS_ERR_INVALID_ARGUMENT;
    if (ls::dist_grid_args_invalid(*grid, nullptr)) return LS_ERR_INVALID_ARGUMENT;
    return ls::dist_grid_out_of_range(*grid) ? LS_ERR_OUT_OF_RANGE : LS_OK;
}

int ls_scene_distance_grid(ls_tracer *tr, void *hip_stream, const ls_distance_grid_desc *grid, const float *sensor_to_grid3x4,
                           const uint8_t *d_select, uint32_t n_select, void *d_cells)
{
    LS_ENTER(tr);
    const hipStream_t s = stream_of(tr, hip_stream);
    if (const int rc = dist_grid_check(tr, grid, sensor_to_grid3x4, d_select, n_select, d_cells, false)) return rc;
    const ls::DistGrid g = ls::dist_grid(*grid, sensor_to_grid3x4);
    return query_run(tr, s, [&] { return dist_grid_issue(tr, s, g, d_select, n_select, d_cells); });
}

int ls_scene_distance_grid_host(ls_tracer *tr, const ls_distance_grid_desc *grid, const float *sensor_to_grid3x4, const uint8_t *select,
                                uint32_t n_select, void *cells)
{
    LS_ENTER(tr);
    int rc;
    if ((rc = dist_grid_check(tr, grid, sensor_to_grid3x4, select, n_select, cells, true))) return rc;
    const hipStream_t s = tr->stream;
    if ((rc = query_enter(tr, s))) return rc;
    Staging st;
    const int p_select = st.in(select, n_select);
    // an accumulating call goes on from what the caller's array holds: it travels both ways
    const int p_cells = st.inout(cells, ls::grid_cells(grid->dims), 8, (grid->flags & LS_DIST_GRID_ACCUMULATE) != 0u);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    const ls::DistGrid g = ls::dist_grid(*grid, sensor_to_grid3x4);
    if ((rc = dist_grid_issue(tr, s, g, io.dev<const uint8_t>(p_select), n_select, io.dev(p_cells)))) return rc;
    return io.fetch(tr);
}

}  // extern "C"
