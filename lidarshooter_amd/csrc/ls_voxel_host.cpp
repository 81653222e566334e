// ls_voxel_host.cpp -- ls_occupancy_grid, its host-memory variant and the descriptor's check: per cell of a voxel grid the rays that
// crossed it, the returns that fell in it and the lowest geomID among those (ls_voxel.hip; the arithmetic is ls_voxel.h).  The
// records' table is the gathers' (tables_prepare, ls_gather.cpp); the call's place among what the handle issues is that of every
// query (query_enter / query_leave).  No hierarchy is touched and LS_INFO_RAY_QUERY_BUILT is left as it is.
#include "ls_internal.h"
#include "ls_voxel.h"

namespace lsi {

namespace {

// The carve's two forms give the same bytes (ls_voxel.hip).  The wave-aggregated one ships: EXPERIMENTS.md E21.  An EXPERIMENTAL
// build reads the knob at every call, so that tools/occupancy_cost.py can alternate the forms in one process.
constexpr int kVoxelAggregate = 1;

// what the device entry point and the host-memory variant (any alignment) refuse, in this order
int voxel_check(ls_tracer *tr, const ls_occupancy_grid_desc *grid, const float *xf, const void *rays, uint32_t n_rays, const void *hits,
                const uint32_t *count, uint32_t n, const void *counts, const void *geom, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!grid) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null grid descriptor");
    if (!counts) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null count records");
    if (n && !hits) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records with n > 0");
    if (const char *why = ls::voxel_args_invalid(*grid, xf)) return fail(tr, LS_ERR_INVALID_ARGUMENT, why);
    if (!host && (misaligned16(rays, hits, counts) || misaligned(geom, 4) || misaligned(count, 4)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "rays, hit records and count records must be 16-byte aligned, geom and the count word 4-byte aligned");
    if (const char *why = ls::voxel_grid_out_of_range(*grid)) return fail(tr, LS_ERR_OUT_OF_RANGE, why);
    if (n > kMaxQueryRecords || (rays && n_rays > kMaxQueryRecords)) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records or rays in one call");
    return uncommitted(tr);
}

// own_rays: the handle's sensor rays (d_rays is not read); otherwise n_rays caller rays, which may be none
int voxel_issue(ls_tracer *tr, hipStream_t s, const ls::VoxelGrid &g, const void *d_rays, uint32_t n_rays, bool own_rays, const void *d_hits,
                const uint32_t *d_count, uint32_t n, void *d_counts, void *d_geom)
{
    ls_tracer::RayQuery &q = tr->rq;
    int rc;
    if ((rc = tables_prepare(tr, s, nullptr))) return rc;
    const ls_tracer::HitAttr &a = tr->ha;
    const uint32_t n_table = (uint32_t)a.table.current.size();
    ls::SensorTables tb = tables(tr);
    tb.az0 = 0;   // the full raster whatever the shard: hit.ray is the global ray index
    tb.naz = tb.H;
    const uint32_t ray_bound = own_rays ? tb.V * tb.H : n_rays;
    if ((rc = ensure(tr, q.voxel_keys, (size_t)ray_bound))) return rc;
    ls::launch_voxel_clear(s, g, d_counts, static_cast<uint32_t *>(d_geom), q.voxel_keys.p, ray_bound);
    ls::launch_voxel_ends(s, d_hits, d_count, n, d_rays, n_rays, own_rays, tb, a.table.dev.p, n_table, q.voxel_keys.p);
    ls::launch_voxel_carve(s, g, d_rays, n_rays, own_rays, tb, q.voxel_keys.p, d_counts, static_cast<uint32_t *>(d_geom),
                           tune_int("LS_VOXEL_AGGREGATE", kVoxelAggregate) != 0);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

}  // namespace

}  // namespace lsi

using namespace lsi;

extern "C" {

int ls_occupancy_grid_check(const ls_occupancy_grid_desc *grid)
{
    if (!grid) return LS_ERR_INVALID_ARGUMENT;
    if (ls::voxel_args_invalid(*grid, nullptr)) return LS_ERR_INVALID_ARGUMENT;
    return ls::voxel_grid_out_of_range(*grid) ? LS_ERR_OUT_OF_RANGE : LS_OK;
}

int ls_occupancy_grid(ls_tracer *tr, void *hip_stream, const ls_occupancy_grid_desc *grid, const float *sensor_to_grid3x4, const void *d_rays,
                      uint32_t n_rays, const void *d_hits, const uint32_t *d_count, uint32_t n, void *d_counts, void *d_geom)
{
    LS_ENTER(tr);
    const hipStream_t s = stream_of(tr, hip_stream);
    if (const int rc = voxel_check(tr, grid, sensor_to_grid3x4, d_rays, n_rays, d_hits, d_count, n, d_counts, d_geom, false)) return rc;
    const ls::VoxelGrid g = ls::voxel_grid(*grid, sensor_to_grid3x4);
    return query_run(tr, s, [&] { return voxel_issue(tr, s, g, d_rays, n_rays, d_rays == nullptr, d_hits, d_count, n, d_counts, d_geom); });
}

int ls_occupancy_grid_host(ls_tracer *tr, const ls_occupancy_grid_desc *grid, const float *sensor_to_grid3x4, const void *rays, uint32_t n_rays,
                           const void *hits, uint32_t n, void *counts, void *geom)
{
    LS_ENTER(tr);
    int rc;
    if ((rc = voxel_check(tr, grid, sensor_to_grid3x4, rays, n_rays, hits, nullptr, n, counts, geom, true))) return rc;
    const hipStream_t s = tr->stream;
    if ((rc = query_enter(tr, s))) return rc;
    const size_t cells = ls::grid_cells(grid->dims);
    const bool acc = (grid->flags & LS_OCC_ACCUMULATE) != 0u;
    Staging st;
    const int p_hits = st.in(hits, (size_t)n * 16), p_rays = st.in(rays, (size_t)n_rays * 32);
    // an accumulating call goes on from what the caller's arrays hold: they travel both ways
    const int p_counts = st.inout(counts, cells, 8, acc), p_geom = st.inout(geom, cells, 4, acc);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    const ls::VoxelGrid g = ls::voxel_grid(*grid, sensor_to_grid3x4);
    if ((rc = voxel_issue(tr, s, g, io.dev(p_rays), n_rays, rays == nullptr, io.dev(p_hits), nullptr, n, io.dev(p_counts), io.dev(p_geom)))) return rc;
    return io.fetch(tr);
}

}  // extern "C"
