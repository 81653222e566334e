// ls_scene_grid_host.cpp -- ls_scene_grid, its host-memory variant and the descriptor's check: per cell of a voxel grid the triangles
// of the committed scene that overlap it and the lowest geomID among them (ls_scene_grid.hip; the arithmetic is ls_scene_grid.h).
// The scene is the flat triangle index (scene_tris_prepare; ls_scene_tris.h); the call's place among what the handle issues is that
// of every query (query_enter / query_leave).  No hierarchy is touched and LS_INFO_RAY_QUERY_BUILT is left as it is.
#include "ls_internal.h"
#include "ls_scene_grid.h"

namespace lsi {

namespace {

// A triangle whose range holds more cells than this goes to k_scene_grid_big's queue, and the small path's atomics are plain or
// aggregated per run of lanes: the same bytes whatever the two say.  What ships is what EXPERIMENTS.md E22 measured: the aggregated
// atomics (198 us against 244 us per call over SYN-1M, spreads of 10 us), and a threshold of 64 -- 8 queues dense meshes' triangles
// for nothing (385 us), 64 and 512 cost the same there and where every triangle is queued, and without the queue a scene of 11 m
// triangles under 5 cm cells takes 575 ms instead of 0.23.  An EXPERIMENTAL build reads the knobs at every call, so that
// tools/scene_grid_cost.py can alternate the forms in one process.
constexpr int kSceneGridSmall = 64;
constexpr int kSceneGridAggregate = 1;

// what the device entry point and the host-memory variant (any alignment) refuse, in this order
int scene_grid_check(ls_tracer *tr, const ls_scene_grid_desc *grid, const float *xf, const uint8_t *select, uint32_t n_select, const void *counts,
                     const void *geom, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!grid) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null grid descriptor");
    if (!counts) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null counts");
    if (n_select && !select) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null select with n_select > 0");
    if (const char *why = ls::scene_grid_args_invalid(*grid, xf)) return fail(tr, LS_ERR_INVALID_ARGUMENT, why);
    if (!host && (misaligned(counts, 16) || misaligned(geom, 4)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "counts must be 16-byte aligned, geom 4-byte aligned");
    if (const char *why = ls::scene_grid_out_of_range(*grid)) return fail(tr, LS_ERR_OUT_OF_RANGE, why);
    return uncommitted(tr);
}

int scene_grid_issue(ls_tracer *tr, hipStream_t s, const ls::SceneGrid &g, const uint8_t *d_select, uint32_t n_select, void *d_counts, void *d_geom)
{
    const ls_tracer::HitAttr &a = tr->ha;
    int rc;
    uint32_t n_table, n_tris, *count;
    uint2 *queue;
    if ((rc = scene_tris_prepare(tr, s, 0xFFFFFFFFull, "more than 2^32 triangles", &n_table, &n_tris))) return rc;
    if ((rc = scene_queue_ensure(tr, tr->rq.scene_queue, n_tris, &count, &queue))) return rc;
    uint32_t *counts = static_cast<uint32_t *>(d_counts), *geom = static_cast<uint32_t *>(d_geom);
    const int small = tune_int("LS_SCENE_GRID_SMALL", kSceneGridSmall);
    ls::launch_scene_grid_clear(s, g, counts, geom, count);
    if (tune_int("LS_SCENE_GRID_CLEAR_ONLY", 0)) return LS_OK;   // (the cost tool's floor: the clear alone)
    ls::launch_scene_grid_small(s, g, a.table.dev.p, n_table, a.tri_first.dev.p, n_tris, d_select, n_select, small < 0 ? 0u : (uint32_t)small,
                                tune_int("LS_SCENE_GRID_AGGREGATE", kSceneGridAggregate) != 0, counts, geom, count, queue);
    ls::launch_scene_grid_big(s, g, a.table.dev.p, n_table, n_tris, counts, geom, count, queue);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

}  // namespace

}  // namespace lsi

using namespace lsi;

extern "C" {

int ls_scene_grid_check(const ls_scene_grid_desc *grid)
{
    if (!grid) return LS_ERR_INVALID_ARGUMENT;
    if (ls::scene_grid_args_invalid(*grid, nullptr)) return LS_ERR_INVALID_ARGUMENT;
    return ls::scene_grid_out_of_range(*grid) ? LS_ERR_OUT_OF_RANGE : LS_OK;
}

int ls_scene_grid(ls_tracer *tr, void *hip_stream, const ls_scene_grid_desc *grid, const float *sensor_to_grid3x4, const uint8_t *d_select,
                  uint32_t n_select, void *d_counts, void *d_geom)
{
    LS_ENTER(tr);
    const hipStream_t s = stream_of(tr, hip_stream);
    if (const int rc = scene_grid_check(tr, grid, sensor_to_grid3x4, d_select, n_select, d_counts, d_geom, false)) return rc;
    const ls::SceneGrid g = ls::scene_grid(*grid, sensor_to_grid3x4);
    return query_run(tr, s, [&] { return scene_grid_issue(tr, s, g, d_select, n_select, d_counts, d_geom); });
}

int ls_scene_grid_host(ls_tracer *tr, const ls_scene_grid_desc *grid, const float *sensor_to_grid3x4, const uint8_t *select, uint32_t n_select,
                       void *counts, void *geom)
{
    LS_ENTER(tr);
    int rc;
    if ((rc = scene_grid_check(tr, grid, sensor_to_grid3x4, select, n_select, counts, geom, true))) return rc;
    const hipStream_t s = tr->stream;
    if ((rc = query_enter(tr, s))) return rc;
    const size_t cells = ls::grid_cells(grid->dims);
    const bool acc = (grid->flags & LS_SCENE_GRID_ACCUMULATE) != 0u;
    Staging st;
    const int p_select = st.in(select, n_select);
    // an accumulating call goes on from what the caller's arrays hold: they travel both ways
    const int p_counts = st.inout(counts, cells, 4, acc), p_geom = st.inout(geom, cells, 4, acc);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    const ls::SceneGrid g = ls::scene_grid(*grid, sensor_to_grid3x4);
    if ((rc = scene_grid_issue(tr, s, g, io.dev<const uint8_t>(p_select), n_select, io.dev(p_counts), io.dev(p_geom)))) return rc;
    return io.fetch(tr);
}

}  // extern "C"
