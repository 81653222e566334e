// ls_debug.cpp -- include/lidarshooter_hip_debug.h: views into the handle for tests/ and bench.py (dense per-ray results,
// the exhaustive device checker, the committed scene and BVH arrays).  Not part of the drop-in surface.
#include "../../include/lidarshooter_hip_debug.h"
#include "ls_internal.h"
#include "ls_closest.h"
#include "ls_hit_attr.h"
#include "ls_return_model.h"
#include "ls_sweep.h"
#include "ls_motion.h"
#include "ls_velocity.h"
#include "ls_beam.h"
#include "ls_cloud_format.h"
#include "ls_voxel.h"
#include "ls_scene_grid.h"
#include "ls_distance_grid.h"
#include "ls_surface_sample.h"
#include "ls_cloud_nearest.h"

#include <algorithm>
#include <vector>

using namespace lsi;

namespace {
// layout entry and registry entry of a committed geometry
int find_committed(ls_tracer *tr, uint32_t geom_id, size_t *slot, Geometry **ge)
{
    if (!tr->committed) return fail(tr, LS_ERR_NOT_COMMITTED, "scene not committed");
    size_t i = 0;
    while (i < tr->slot_geom_ids.size() && (uint32_t)tr->slot_geom_ids[i] != geom_id) ++i;
    if (i >= tr->slot_geom_ids.size() || i >= tr->layout.size()) return fail(tr, LS_ERR_UNKNOWN_GEOMETRY, "no such geometry in the committed scene");
    *slot = i;
    return committed_geometry(tr, i, ge);
}

template <typename T>
struct Scratch {   // device memory of one call
    T *p = nullptr;
    ~Scratch() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(n, 1) * sizeof(T)); }
};
}  // namespace

extern "C" {

int ls_debug_dense_hits(ls_tracer *tr, float *t, uint32_t *gid)
{
    LS_ENTER(tr);
    if (!t || !gid) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null output");
    const uint32_t n = shard_rays(tr);
    if (!tr->traced) {
        for (uint32_t q = 0; q < n; ++q) { t[q] = -1.0f; gid[q] = ls::kInvalid; }
        return LS_OK;
    }
    {
        const int rc = flush_pipeline(tr);
        if (rc) return rc;
    }
    if (tr->traced_projection) {
        // the projection engine keeps no dense arrays: rebuild them from the frame's hit records
        ls::launch_dense_from_hits(tr->stream, tables(tr), tr->last_d_hits, tr->last_d_n, geom_table(tr), tr->hit_t.p, tr->hit_gid.p);
        LS_HIP(hipGetLastError());
    }
    LS_HIP(hipStreamSynchronize(tr->stream));
    LS_HIP(hipMemcpy(t, tr->hit_t.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    LS_HIP(hipMemcpy(gid, tr->hit_gid.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LS_OK;
}

int ls_debug_trace_bruteforce(ls_tracer *tr, float *t, uint32_t *gid)
{
    LS_ENTER(tr);
    if (!t || !gid) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null output");
    if (!tr->committed) return fail(tr, LS_ERR_NOT_COMMITTED, "scene not committed");
    if (!tr->scene_materialized) { const int rc = materialize_scene(tr, false); if (rc) return rc; }
    const uint32_t n = shard_rays(tr);
    float *dt = nullptr;
    uint32_t *dg = nullptr;
    LS_HIP(hipMalloc(reinterpret_cast<void **>(&dt), (size_t)n * 4));
    LS_HIP(hipMalloc(reinterpret_cast<void **>(&dg), (size_t)n * 4));
    ls::launch_bruteforce(tr->stream, tables(tr), tr->verts.p, tr->tris.p, tr->n_tris, dt, dg);
    hipError_t e = hipStreamSynchronize(tr->stream);
    if (e == hipSuccess) e = hipMemcpy(t, dt, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(gid, dg, (size_t)n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(dt);
    (void)hipFree(dg);
    if (e != hipSuccess) return fail(tr, LS_ERR_HIP, hipGetErrorString(e));
    return LS_OK;
}

int ls_debug_scene_size(ls_tracer *tr, uint32_t *n_verts, uint32_t *n_tris, uint32_t *n_node_slots, uint32_t *leaf_size)
{
    LS_ENTER(tr);
    if (!tr->committed) return fail(tr, LS_ERR_NOT_COMMITTED, "scene not committed");
    if (n_verts) *n_verts = tr->n_verts;
    if (n_tris) *n_tris = tr->n_tris;
    if (n_node_slots) *n_node_slots = tr->n_slots;
    if (leaf_size) *leaf_size = tr->committed_leaf_size;
    return LS_OK;
}

int ls_debug_download_scene(ls_tracer *tr, float *verts_xyz, uint32_t *tri_idx)
{
    LS_ENTER(tr);
    if (!tr->committed) return fail(tr, LS_ERR_NOT_COMMITTED, "scene not committed");
    if (!tr->scene_materialized) { const int rc = materialize_scene(tr, false); if (rc) return rc; }
    LS_HIP(hipStreamSynchronize(tr->stream));
    if (verts_xyz) LS_HIP(hipMemcpy(verts_xyz, tr->verts.p, (size_t)tr->n_verts * 12, hipMemcpyDeviceToHost));
    if (tri_idx) LS_HIP(hipMemcpy(tri_idx, tr->tris.p, (size_t)tr->n_tris * 12, hipMemcpyDeviceToHost));
    return LS_OK;
}

int ls_debug_download_bvh(ls_tracer *tr, void *nodes, void *tri_records)
{
    LS_ENTER(tr);
    if (!tr->committed || !tr->bvh_built) return fail(tr, LS_ERR_NOT_COMMITTED, "no BVH: commit with LS_OPT_ENGINE = 1");
    if (tr->bvh_inst) return fail(tr, LS_ERR_NOT_COMMITTED, "the debug view shows the classic hierarchy: commit with LS_OPT_BVH_INSTANCED = 0");
    LS_HIP(hipStreamSynchronize(tr->stream));
    if (nodes) LS_HIP(hipMemcpy(nodes, tr->nodes.p, (size_t)tr->n_slots * sizeof(ls::FatNode), hipMemcpyDeviceToHost));
    if (tri_records) LS_HIP(hipMemcpy(tri_records, tr->records.p, (size_t)tr->n_tris * sizeof(ls::TriRecord), hipMemcpyDeviceToHost));
    return LS_OK;
}

int ls_debug_download_hierarchy(ls_tracer *tr, uint32_t geom_id, uint32_t *n_leaves, uint32_t *leaf_size, void *nodes64, void *wide128,
                                void *records48)
{
    LS_ENTER(tr);
    if (!tr->committed || !tr->bvh_built || !tr->bvh_inst || !tr->inst_valid)
        return fail(tr, LS_ERR_NOT_COMMITTED, "no instanced hierarchies: commit with LS_OPT_ENGINE = 1 and LS_OPT_BVH_INSTANCED = 1");
    size_t i = 0;
    while (i < tr->slot_geom_ids.size() && (uint32_t)tr->slot_geom_ids[i] != geom_id) ++i;
    if (i >= tr->slot_geom_ids.size() || i >= tr->inst_layout.size()) return fail(tr, LS_ERR_UNKNOWN_GEOMETRY, "no such geometry in the committed scene");
    Geometry *ge = nullptr;
    {
        const int rc = committed_geometry(tr, i, &ge);
        if (rc) return rc;
    }
    const ls_tracer::InstSlot &sl = tr->inst_layout[i];
    if (n_leaves) *n_leaves = sl.n_leaves;
    if (leaf_size) *leaf_size = tr->inst_leaf_size;
    if (!nodes64 && !wide128 && !records48) return LS_OK;
    if (wide128 && sl.n_leaves > 1u && (!tr->wide_valid || !sl.wide_made))
        return fail(tr, LS_ERR_NOT_COMMITTED, "the four-wide twins of this hierarchy have not been made");
    {
        const int rc = flush_pipeline(tr);
        if (rc) return rc;
    }
    LS_HIP(hipStreamSynchronize(tr->stream));
    const size_t n_nodes = sl.n_leaves ? sl.n_leaves - 1u : 0u;
    if (nodes64 && n_nodes) LS_HIP(hipMemcpy(nodes64, tr->nodes.p + sl.node_first, n_nodes * sizeof(ls::FatNode), hipMemcpyDeviceToHost));
    if (wide128 && n_nodes) LS_HIP(hipMemcpy(wide128, tr->wide_nodes.p + sl.node_first, n_nodes * sizeof(ls::WideNode), hipMemcpyDeviceToHost));
    if (records48) LS_HIP(hipMemcpy(records48, tr->records.p + sl.rec_first, (size_t)ge->n_tris * sizeof(ls::TriRecord), hipMemcpyDeviceToHost));
    return LS_OK;
}

int ls_debug_sort_pairs(ls_tracer *tr, uint32_t *keys, uint32_t *vals, uint32_t n)
{
    LS_ENTER(tr);
    if ((!keys || !vals) && n) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null argument");
    if (!n) return LS_OK;
    uint32_t *d = nullptr;
    void *temp = nullptr;
    const size_t tb = ls::sort_temp_bytes(n);
    LS_HIP(hipMalloc(reinterpret_cast<void **>(&d), (size_t)n * 16));
    hipError_t e = hipMalloc(&temp, tb);
    if (e == hipSuccess) e = hipMemcpy(d, keys, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, vals, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        e = ls::launch_sort(tr->stream, temp, tb, d, d + 2 * (size_t)n, d + n, d + 3 * (size_t)n, n) ? hipStreamSynchronize(tr->stream)
                                                                                                       : hipErrorInvalidValue;
    }
    if (e == hipSuccess) e = hipMemcpy(keys, d + 2 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(vals, d + 3 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    (void)hipFree(temp);
    if (e != hipSuccess) return fail(tr, LS_ERR_HIP, hipGetErrorString(e));
    return LS_OK;
}

int ls_debug_closest_on_triangle(const float p[3], const float v0[3], const float v1[3], const float v2[3], float q[3], float *d2)
{
    if (!p || !v0 || !v1 || !v2 || !q || !d2) return LS_ERR_INVALID_ARGUMENT;
    ls::closest_on_triangle(p, v0, v1, v2, q, d2);
    return LS_OK;
}

int ls_debug_hit_attributes_on_triangle(const float o[3], const float d[3], const float v0[3], const float v1[3], const float v2[3], float *t,
                                        float out9[9])
{
    if (!o || !d || !v0 || !v1 || !v2 || !t || !out9) return LS_ERR_INVALID_ARGUMENT;
    return ls::hit_attributes_on_triangle(o, d, v0, v1, v2, t, out9) ? 1 : 0;
}

int ls_debug_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    if (!ctr || !key || !out) return LS_ERR_INVALID_ARGUMENT;
    ls::philox4x32_10(ctr, key, out);
    return LS_OK;
}

int ls_debug_return_model(const ls_return_model *m, uint32_t ray, uint32_t frame_index, float t, float len, float cos_inc, float rho, float *t_out,
                          float *intensity)
{
    if (!t_out || !intensity || ls::return_model_invalid(m)) return LS_ERR_INVALID_ARGUMENT;
    return ls::return_model_eval(*m, ray, frame_index, t, len, cos_inc, rho, t_out, intensity) ? 1 : 0;
}

int ls_debug_sweep_ray(const float d[3], const float pose12[12], float ray8[8])
{
    if (!d || !pose12 || !ray8) return LS_ERR_INVALID_ARGUMENT;
    ls::sweep_ray(pose12, d[0], d[1], d[2], ray8);
    return LS_OK;
}

int ls_debug_motion_ray(const float ray8_in[8], const float motion12[12], float ray8_out[8])
{
    if (!ray8_in || !motion12 || !ray8_out) return LS_ERR_INVALID_ARGUMENT;
    ls::motion_ray(motion12, ray8_in, ray8_out);
    return LS_OK;
}

int ls_debug_motion_normal(const float n3[3], const float motion12[12], float out3[3])
{
    if (!n3 || !motion12 || !out3) return LS_ERR_INVALID_ARGUMENT;
    ls::motion_normal(motion12, n3, out3);
    return LS_OK;
}

// hit_velocity: what a lane of k_hit_velocities does for a valid record
int ls_debug_hit_velocity(const float cast8[8], float t, const float sensor_twist6[6], const float geom_twist6[6], float out8[8])
{
    if (!cast8 || !out8) return LS_ERR_INVALID_ARGUMENT;
    float res[7];
    ls::hit_velocity(cast8, t, sensor_twist6 != nullptr, sensor_twist6, geom_twist6 != nullptr, geom_twist6, res);
    const uint32_t valid = 1u;
    std::memcpy(out8, res, sizeof(res));
    std::memcpy(out8 + 7, &valid, 4);
    return LS_OK;
}

int ls_debug_beam_ray(float sin_theta, float cos_theta, float cos_phi, float sin_phi, const float abk[3], float ray8[8])
{
    if (!abk || !ray8) return LS_ERR_INVALID_ARGUMENT;
    ls::beam_ray(sin_theta, cos_theta, cos_phi, sin_phi, abk[0], abk[1], ray8);
    return LS_OK;
}

// what a group of k_beam_reduce's lanes does, position by position: the keys in ascending order, the ballot masks, beam_select
int ls_debug_beam_echoes(const ls_beam_model *model, const float *r, const uint8_t *hit, uint32_t *out, uint32_t *n_out)
{
    if (!model || !r || !hit || !out || !n_out) return LS_ERR_INVALID_ARGUMENT;
    const uint32_t S = model->n_samples;
    if (S < 1u || S > ls::kBeamMaxSamples || !model->returns || (model->returns & ~(uint32_t)(LS_BEAM_FIRST | LS_BEAM_LAST | LS_BEAM_STRONGEST)) ||
        model->min_count < 1u || model->min_count > S || !(model->echo_separation >= 0.0f))
        return LS_ERR_INVALID_ARGUMENT;
    unsigned long long key[ls::kBeamMaxSamples];
    for (uint32_t s = 0; s < S; ++s) key[s] = hit[s] ? ls::beam_key(r[s], s) : ls::kBeamMiss;
    std::sort(key, key + S);
    unsigned long long starts = 0;
    uint32_t n_hits = 0;
    for (uint32_t j = 0; j < S; ++j) {
        if (ls::beam_starts_echo(j ? key[j - 1] : 0ull, key[j], j, model->echo_separation)) starts |= 1ull << j;
        if (key[j] != ls::kBeamMiss) ++n_hits;
    }
    const ls::BeamReturns ret = ls::beam_select(starts, n_hits, model->min_count, model->returns);
    const uint32_t n = ret.n, w[3] = {ret.w0, ret.w1, ret.w2};
    for (uint32_t i = 0; i < n; ++i) {
        const unsigned long long sel = key[ls::beam_word_where(w[i])];
        out[2 * i] = (uint32_t)(sel >> 8);
        out[2 * i + 1] = ls::beam_word(w[i] & 7u, ls::beam_word_count(w[i]), ls::beam_key_sample(sel));
    }
    *n_out = n;
    return LS_OK;
}

int ls_debug_beam_model_check(const ls_beam_model *model, uint32_t shard_rays, uint32_t capacity)
{
    int status = LS_OK;
    return ls::beam_model_invalid(model, shard_rays, capacity, &status) ? status : LS_OK;
}

// beam_ray, then sweep_ray on its direction: what a lane of k_beam_sweep_rays does
int ls_debug_beam_sweep_ray(float sin_theta, float cos_theta, float cos_phi, float sin_phi, const float abk[3], const float pose12[12], float ray8[8])
{
    if (!abk || !pose12 || !ray8) return LS_ERR_INVALID_ARGUMENT;
    float b[8];
    ls::beam_ray(sin_theta, cos_theta, cos_phi, sin_phi, abk[0], abk[1], b);
    ls::sweep_ray(pose12, b[4], b[5], b[6], ray8);
    return LS_OK;
}

// what a group of k_beam_reduce_weighted's lanes does, position by position: the keys in ascending order, the start mask, the prefix
// sums of the weights, the strength of every echo, the detectable ones and the strongest, beam_select_weighted
int ls_debug_beam_echoes_weighted(const ls_beam_model *model, const uint32_t *weights, uint32_t min_weight, const float *r, const uint8_t *hit,
                                  uint32_t *out, uint32_t *n_out)
{
    if (!model || !r || !hit || !out || !n_out) return LS_ERR_INVALID_ARGUMENT;
    const uint32_t S = model->n_samples;
    if (S < 1u || S > ls::kBeamMaxSamples || !model->returns || (model->returns & ~(uint32_t)(LS_BEAM_FIRST | LS_BEAM_LAST | LS_BEAM_STRONGEST)) ||
        model->min_count < 1u || model->min_count > S || !(model->echo_separation >= 0.0f) || ls::beam_weights_invalid(weights, S))
        return LS_ERR_INVALID_ARGUMENT;
    uint32_t w_total = 0;
    const ls::BeamWeights wts = ls::beam_weights_by_value(weights, S, &w_total);
    unsigned long long key[ls::kBeamMaxSamples];
    for (uint32_t s = 0; s < S; ++s) key[s] = hit[s] ? ls::beam_key(r[s], s) : ls::kBeamMiss;
    std::sort(key, key + S);
    unsigned long long starts = 0, detectable = 0;
    uint32_t n_hits = 0, upto[ls::kBeamMaxSamples], W[ls::kBeamMaxSamples], best = 0;
    for (uint32_t j = 0; j < S; ++j) {
        if (ls::beam_starts_echo(j ? key[j - 1] : 0ull, key[j], j, model->echo_separation)) starts |= 1ull << j;
        if (key[j] != ls::kBeamMiss) ++n_hits;
        upto[j] = (j ? upto[j - 1] : 0u) + (key[j] != ls::kBeamMiss ? (uint32_t)wts.w[ls::beam_key_sample(key[j])] : 0u);
    }
    for (uint32_t j = 0; j < S; ++j) {
        W[j] = 0;
        if (!((starts >> j) & 1ull)) continue;
        const uint32_t end = ls::beam_echo_end(starts, n_hits, j);
        W[j] = upto[end - 1] - (j ? upto[j - 1] : 0u);
        if (!ls::beam_detectable(end - j, W[j], model->min_count, min_weight)) continue;
        detectable |= 1ull << j;
        best = std::max(best, ls::beam_strength(W[j], j));
    }
    const ls::BeamReturns ret = ls::beam_select_weighted(starts, n_hits, detectable, ls::beam_strength_where(best), model->returns);
    const uint32_t n = ret.n, w[3] = {ret.w0, ret.w1, ret.w2};
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t at = ls::beam_word_where(w[i]);
        out[3 * i] = (uint32_t)(key[at] >> 8);
        out[3 * i + 1] = ls::beam_word(w[i] & 7u, ls::beam_word_count(w[i]), ls::beam_key_sample(key[at]));
        out[3 * i + 2] = W[at];
    }
    *n_out = n;
    return LS_OK;
}

int ls_debug_beam_sweep_check(const ls_beam_model *model, const uint32_t *weights, uint32_t shard_rays, uint32_t capacity)
{
    int status = LS_OK;
    if (ls::beam_model_invalid(model, shard_rays, capacity, &status)) return status;
    return ls::beam_weights_invalid(weights, model->n_samples) ? LS_ERR_INVALID_ARGUMENT : LS_OK;
}

// cloud_sources, then cloud_format_record: what a lane of k_format_cloud does for its record, or for the miss cell of cell_ray
int ls_debug_voxel_walk(const ls_occupancy_grid_desc *grid, const float *sensor_to_grid3x4, const float ray32[8], float t_end,
                        uint32_t *cells_out, uint32_t capacity, uint32_t *n_cells, uint32_t *occupied_cell_out)
{
    if (!grid || !ray32 || !n_cells || !occupied_cell_out || (capacity && !cells_out)) return LS_ERR_INVALID_ARGUMENT;
    if (ls::voxel_args_invalid(*grid, sensor_to_grid3x4) || ls::voxel_grid_out_of_range(*grid)) return LS_ERR_INVALID_ARGUMENT;
    const ls::VoxelGrid g = ls::voxel_grid(*grid, sensor_to_grid3x4);
    *n_cells = 0;
    *occupied_cell_out = ls::kVoxelNone;
    float o[3] = {ray32[0], ray32[1], ray32[2]}, d[3] = {ray32[4], ray32[5], ray32[6]};
    const float tmin = ray32[3], tmax = ray32[7];
    // (k_voxel_carve's test of a caller's ray)
    if (!(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]) && std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]) &&
          (d[0] != 0.f || d[1] != 0.f || d[2] != 0.f) && tmin <= tmax))
        return LS_OK;
    if (g.has_xf) ls::voxel_ray_to_grid(g.xf, o, d);
    float t0, t1;
    bool marks;
    const bool carve = ls::voxel_span(g, tmin, tmax, !std::isnan(t_end), t_end, &t0, &t1, &marks);
    if (marks) *occupied_cell_out = ls::voxel_occupied_cell(g, o, d, t_end, false);
    if (!carve) return LS_OK;
    ls::VoxelWalk w;
    for (ls::voxel_walk_begin(g, o, d, t0, t1, w); w.live; ls::voxel_walk_next(g, w)) {
        if (*n_cells < capacity) cells_out[*n_cells] = ls::voxel_index(g, w);
        ++*n_cells;
    }
    return *n_cells > capacity ? LS_ERR_OUT_OF_RANGE : LS_OK;
}

int ls_debug_scene_grid_triangle(const ls_scene_grid_desc *grid, const float tri9[9], uint32_t *cells_out, uint32_t capacity, uint32_t *n_cells)
{
    if (!grid || !tri9 || !n_cells || (capacity && !cells_out)) return LS_ERR_INVALID_ARGUMENT;
    if (ls_scene_grid_check(grid) != LS_OK) return LS_ERR_INVALID_ARGUMENT;
    const ls::SceneGrid g = ls::scene_grid(*grid, nullptr);
    *n_cells = 0;
    ls::SceneTri t;
    ls::SceneRange r;
    if (!ls::scene_tri_setup(g, tri9[0], tri9[1], tri9[2], tri9[3], tri9[4], tri9[5], tri9[6], tri9[7], tri9[8], t, r)) return LS_OK;
    for (int cz = r.loz; cz <= r.hiz; ++cz)
        for (int cy = r.loy; cy <= r.hiy; ++cy)
            for (int cx = r.lox; cx <= r.hix; ++cx)
                if (ls::scene_cell_overlaps(t, cx, cy, cz)) {
                    if (*n_cells < capacity) cells_out[*n_cells] = ls::scene_cell_index(g, cx, cy, cz);
                    ++*n_cells;
                }
    return *n_cells > capacity ? LS_ERR_OUT_OF_RANGE : LS_OK;
}

int ls_debug_scene_grid_queued(ls_tracer *tr, uint32_t *n_queued)
{
    LS_ENTER(tr);
    if (!n_queued) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null output");
    *n_queued = 0;
    if (!tr->rq.scene_queue.p) return LS_OK;
    LS_HIP(hipStreamSynchronize(tr->stream));
    LS_HIP(hipMemcpy(n_queued, tr->rq.scene_queue.p, 4, hipMemcpyDeviceToHost));
    return LS_OK;
}

int ls_debug_distance_grid_triangle(const ls_distance_grid_desc *grid, const float tri9[9], uint32_t *cells_out, float *dist_out, uint32_t capacity,
                                    uint32_t *n_cells)
{
    if (!grid || !tri9 || !n_cells || (capacity && (!cells_out || !dist_out))) return LS_ERR_INVALID_ARGUMENT;
    if (ls_scene_distance_grid_check(grid) != LS_OK) return LS_ERR_INVALID_ARGUMENT;
    const ls::DistGrid g = ls::dist_grid(*grid, nullptr);
    *n_cells = 0;
    ls::DistTri t;
    ls::SceneRange r;
    if (!ls::dist_tri_setup(g, tri9[0], tri9[1], tri9[2], tri9[3], tri9[4], tri9[5], tri9[6], tri9[7], tri9[8], t, r)) return LS_OK;
    for (int cz = r.loz; cz <= r.hiz; ++cz)
        for (int cy = r.loy; cy <= r.hiy; ++cy)
            for (int cx = r.lox; cx <= r.hix; ++cx) {
                float dist;
                if (!ls::dist_cell(t, g.trunc, g.cell, cx, cy, cz, &dist)) continue;
                if (*n_cells < capacity) {
                    cells_out[*n_cells] = ls::dist_cell_index(g, cx, cy, cz);
                    dist_out[*n_cells] = dist;
                }
                ++*n_cells;
            }
    return *n_cells > capacity ? LS_ERR_OUT_OF_RANGE : LS_OK;
}

int ls_debug_distance_grid_queued(ls_tracer *tr, uint32_t *n_queued)
{
    LS_ENTER(tr);
    if (!n_queued) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null output");
    *n_queued = 0;
    if (!tr->rq.dist_queue.p) return LS_OK;
    LS_HIP(hipStreamSynchronize(tr->stream));
    LS_HIP(hipMemcpy(n_queued, tr->rq.dist_queue.p, 4, hipMemcpyDeviceToHost));
    return LS_OK;
}

int ls_debug_surface_weights(const float *tris9, uint32_t n, float *area_out, uint64_t *weight_out, uint64_t *prefix_out, void *info_out)
{
    if (n && !tris9) return LS_ERR_INVALID_ARGUMENT;
    std::vector<float> area(n);
    uint32_t top = 0u;
    float normal[3];
    for (uint32_t i = 0; i < n; ++i) {
        area[i] = ls::surface_tri_area(tris9 + 9 * (size_t)i, normal);
        uint32_t bits;
        std::memcpy(&bits, &area[i], 4);
        top = std::max(top, bits);
    }
    const int e = ls::surface_exponent(top);
    uint64_t sum = 0;
    uint32_t weighted = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t w = ls::surface_weight(area[i], e);
        if (area_out) area_out[i] = area[i];
        if (weight_out) weight_out[i] = w;
        if (prefix_out) prefix_out[i] = sum;
        sum += w;
        weighted += w != 0;
    }
    if (prefix_out) prefix_out[n] = sum;
    if (info_out) {
        const int32_t e32 = e;
        std::memcpy(info_out, &sum, 8);
        std::memcpy(static_cast<uint8_t *>(info_out) + 8, &e32, 4);
        std::memcpy(static_cast<uint8_t *>(info_out) + 12, &weighted, 4);
    }
    return LS_OK;
}

int ls_debug_surface_pick(const uint64_t *prefix, uint32_t n, uint64_t r64, uint32_t *tri_out)
{
    if (!prefix || !tri_out) return LS_ERR_INVALID_ARGUMENT;
    const uint64_t W = prefix[n];
    *tri_out = W ? ls::surface_bisect(prefix, 0u, n, ls::surface_mulhi(r64, W)) : 0xFFFFFFFFu;
    return LS_OK;
}

int ls_debug_surface_point(const float tri9[9], uint32_t x2, uint32_t x3, float out9[9])
{
    if (!tri9 || !out9) return LS_ERR_INVALID_ARGUMENT;
    ls::surface_tri_area(tri9, out9 + 3);
    ls::surface_bary(x2, x3, &out9[6], &out9[7], &out9[8]);
    ls::surface_point(tri9, out9[6], out9[7], out9[8], out9);
    return LS_OK;
}

int ls_debug_cloud_cell(float radius, const float *xyz, uint32_t n, int32_t *cell_out, uint8_t *takes_part_out)
{
    if (n && (!xyz || !cell_out || !takes_part_out)) return LS_ERR_INVALID_ARGUMENT;
    ls_cloud_nearest_desc desc{};
    desc.radius = radius;
    desc.cloud_stride = desc.query_stride = 12;
    if (ls::cloud_nearest_args_invalid(desc, nullptr)) return LS_ERR_INVALID_ARGUMENT;
    const ls::CloudNearest d = ls::cloud_nearest(desc, nullptr);
    for (size_t i = 0; i < n; ++i) {
        const float *p = xyz + 3 * i;
        const bool part = ls::cloud_takes_part(d.D, p[0], p[1], p[2]);
        takes_part_out[i] = part ? 1 : 0;
        for (int a = 0; a < 3; ++a) cell_out[3 * i + a] = part ? ls::cloud_cell(d.h, p[a]) : 0;
    }
    return LS_OK;
}

uint32_t ls_debug_cloud_bucket(const int32_t cell[3], uint32_t log2_buckets)
{
    if (!cell || log2_buckets < ls::kCloudMinLog2 || log2_buckets > ls::kCloudMaxLog2) return 0xFFFFFFFFu;
    return ls::cloud_bucket(cell[0], cell[1], cell[2], (1u << log2_buckets) - 1u);
}

int ls_debug_format_record(const ls_cloud_format *fmt, const void *point32, const ls_hit *hit, uint32_t echo_word, float col_time_value,
                           float chan_time_value, uint32_t V, uint32_t H, uint32_t cell_ray, void *out_bytes)
{
    if (!out_bytes || ls_cloud_format_check(fmt) != LS_OK) return LS_ERR_INVALID_ARGUMENT;
    uint32_t p8[8], h4[4] = {cell_ray, 0u, 0u, 0u};
    if (point32) std::memcpy(p8, point32, 32);
    if (hit) std::memcpy(h4, hit, 16);
    const ls::CloudSources src = ls::cloud_sources(point32 ? p8 : nullptr, h4, !hit, echo_word, col_time_value, chan_time_value, V, H);
    ls::cloud_format_record(*fmt, src, static_cast<uint8_t *>(out_bytes));
    return LS_OK;
}

static_assert(sizeof(ls::BandMap) == 32, "map8 is the BandMap, word for word");

int ls_debug_band_map_fit(const float *tan_up, uint32_t V, float map8[8])
{
    if (!tan_up || !V || !map8) return LS_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < V; ++i)
        if (std::isnan(tan_up[i]) || (i && tan_up[i] < tan_up[i - 1])) return LS_ERR_INVALID_ARGUMENT;
    const ls::BandMap bm = ls::band_map_fit(tan_up, V);
    std::memcpy(map8, &bm, sizeof(bm));
    return LS_OK;
}

int ls_debug_band_guess(const float map8[8], uint32_t V, float t, uint32_t *start)
{
    if (!map8 || !start) return LS_ERR_INVALID_ARGUMENT;
    ls::BandMap bm;
    std::memcpy(&bm, map8, sizeof(bm));
    *start = ls::band_guess(bm, V, t);
    return LS_OK;
}

int ls_debug_tracer_band_map(const ls_tracer *tr, float map8[8])
{
    if (!tr || !map8) return LS_ERR_INVALID_ARGUMENT;
    std::memcpy(map8, &tr->band, sizeof(tr->band));
    return LS_OK;
}

// ---- group culling ---------------------------------------------------------------------------------------------------
static_assert(LS_DEBUG_CULL_LUT == ls::kCullVariantLut && LS_DEBUG_CULL_LDS == ls::kCullVariantLds && LS_DEBUG_CULL_SECTOR == ls::kCullVariantSector &&
              LS_DEBUG_CULL_COUNT == ls::kCullVariantCount, "the header's bits are launch_cull's");
int ls_debug_force_group_cull(ls_tracer *tr, int on)
{
    LS_ENTER(tr);
    const int rc = flush_pipeline(tr);
    if (rc) return rc;
    tr->debug_force_cull = on ? 1 : 0;   // (the culling data is made by the next commit: prepare_blocks)
    return LS_OK;
}

int ls_debug_download_cull(ls_tracer *tr, uint32_t geom_id, uint32_t *n_tris, uint32_t *perm, float *group_boxes, float *block_boxes)
{
    LS_ENTER(tr);
    size_t slot = 0;
    Geometry *ge = nullptr;
    int rc = find_committed(tr, geom_id, &slot, &ge);
    if (rc) return rc;
    if (!use_projection(tr) || !cull_enabled(tr, *ge) || !cull_size_ok(tr, ge->n_tris) || !ge->d_perm || !ge->d_boxes || ge->order_stale || ge->bounds_stale)
        return fail(tr, LS_ERR_NOT_COMMITTED, "this geometry has no current culling data (projection engine, LS_OPT_BLOCK_CULL, commit after the last upload)");
    if (n_tris) *n_tris = ge->n_tris;
    if (!perm && !group_boxes && !block_boxes) return LS_OK;
    if ((rc = flush_pipeline(tr))) return rc;
    LS_HIP(hipStreamSynchronize(tr->stream));
    const size_t groups = (ge->n_tris + ls::kCullGroup - 1) / ls::kCullGroup, blocks = ls::project_box_entries(ge->n_tris) - groups;
    if (perm) LS_HIP(hipMemcpy(perm, ge->d_perm, (size_t)ge->n_tris * 4, hipMemcpyDeviceToHost));
    if (group_boxes) LS_HIP(hipMemcpy(group_boxes, ge->d_boxes, groups * 32, hipMemcpyDeviceToHost));
    if (block_boxes) LS_HIP(hipMemcpy(block_boxes, ge->d_boxes + 2 * groups, blocks * 32, hipMemcpyDeviceToHost));
    return LS_OK;
}

int ls_debug_cull_survivors(ls_tracer *tr, uint32_t geom_id, uint32_t *out, uint32_t cap, uint32_t *n, uint32_t *variant)
{
    LS_ENTER(tr);
    if (!n || (!out && cap)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null output");
    size_t slot = 0;
    Geometry *ge = nullptr;
    int rc = find_committed(tr, geom_id, &slot, &ge);
    if (rc) return rc;
    if (!use_projection(tr)) return fail(tr, LS_ERR_NOT_COMMITTED, "group culling belongs to the projection engine (LS_OPT_ENGINE = 2)");
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open: its launches are recorded, not run");
    if ((rc = flush_pipeline(tr))) return rc;
    std::vector<ls::GeomSource> srcs;
    bool any_culled = false;
    if ((rc = project_sources(tr, srcs, any_culled))) return rc;
    const ls::ProjectParams pp = project_params(tr);
    const uint32_t groups = (ge->n_tris + ls::kCullGroup - 1) / ls::kCullGroup;
    ls::CullProbe probe;
    std::memset(&probe, 0, sizeof(probe));
    uint32_t at = ls::kGeomsPerLaunch;
    if (any_culled && shard_rays(tr) && ls::launch_cull_probe(tr->stream, pp, srcs.data(), (uint32_t)srcs.size(), nullptr, nullptr, nullptr, probe))
        for (uint32_t i = 0; i < probe.n; ++i)
            if (probe.src_index[i] == (uint32_t)slot) at = i;
    if (at == (uint32_t)ls::kGeomsPerLaunch) {
        // the frame projects every triangle of this geometry: no bounds, or more culled geometries than one launch takes
        *n = groups;
        if (variant) *variant = LS_DEBUG_CULL_UNCULLED;
        if (cap < groups) return fail(tr, LS_ERR_OUT_OF_RANGE, "more surviving groups than the output holds");
        for (uint32_t g = 0; g < groups; ++g) out[g] = g;
        return LS_OK;
    }
    Scratch<uint32_t> list, counts;
    Scratch<unsigned long long> stats;
    constexpr size_t kCountWords = (size_t)ls::kCullCounters * 16;
    LS_HIP(list.alloc(probe.entries));
    LS_HIP(counts.alloc(kCountWords));
    LS_HIP(stats.alloc(4));
    LS_HIP(hipMemsetAsync(counts.p, 0, kCountWords * 4, tr->stream));
    LS_HIP(hipMemsetAsync(stats.p, 0, 32, tr->stream));
    // (the frame's own counters, survivor lists, statistics and hint word are not touched: everything lands in this call's scratch)
    if (!ls::launch_cull_probe(tr->stream, pp, srcs.data(), (uint32_t)srcs.size(), list.p, counts.p, tr->opt_count ? stats.p : nullptr, probe))
        return fail(tr, LS_ERR_HIP, "the cull pass could not be laid out twice the same way");
    LS_HIP(hipGetLastError());
    LS_HIP(hipStreamSynchronize(tr->stream));
    std::vector<uint32_t> h_counts(kCountWords), found;
    LS_HIP(hipMemcpy(h_counts.data(), counts.p, kCountWords * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> seg(probe.seg_cap[at]);
    for (uint32_t s = 0; s < ls::kCullSegs; ++s) {
        const uint32_t c = h_counts[((size_t)at * ls::kCullSegs + s) * 16];
        if (c > probe.seg_cap[at]) return fail(tr, LS_ERR_OUT_OF_RANGE, "a survivor segment holds more than its capacity");
        if (!c) continue;
        LS_HIP(hipMemcpy(seg.data(), list.p + probe.list_first[at] + (size_t)s * probe.seg_cap[at], (size_t)c * 4, hipMemcpyDeviceToHost));
        found.insert(found.end(), seg.begin(), seg.begin() + c);
    }
    std::sort(found.begin(), found.end());
    *n = (uint32_t)found.size();
    if (variant) *variant = probe.variant;
    if (found.size() > cap) return fail(tr, LS_ERR_OUT_OF_RANGE, "more surviving groups than the output holds");
    std::copy(found.begin(), found.end(), out);
    return LS_OK;
}

int ls_debug_cull_tables(ls_tracer *tr, float *tan_up, float *tan_dn, uint32_t *chan_perm, int *lut_ok)
{
    LS_ENTER(tr);
    const size_t V = tr->V, at = 2 * V + 2 * (size_t)tr->H;
    if (tr->host_tables.size() < at + 3 * V) return fail(tr, LS_ERR_NOT_COMMITTED, "the handle has no sensor tables");
    if (tan_up) std::memcpy(tan_up, tr->host_tables.data() + at, V * 4);
    if (tan_dn) std::memcpy(tan_dn, tr->host_tables.data() + at + V, V * 4);
    if (chan_perm) std::memcpy(chan_perm, tr->host_tables.data() + at + 2 * V, V * 4);
    if (lut_ok) *lut_ok = tr->lut_ok ? 1 : 0;
    return LS_OK;
}

int ls_debug_chan_query(ls_tracer *tr, const float *tan_lo_hi, uint32_t n, uint8_t *lut_search)
{
    LS_ENTER(tr);
    if (!n) return LS_OK;
    if (!tan_lo_hi || !lut_search) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null argument");
    if (!use_projection(tr)) return fail(tr, LS_ERR_NOT_COMMITTED, "group culling belongs to the projection engine (LS_OPT_ENGINE = 2)");
    Scratch<float> q;
    Scratch<uint8_t> a;
    LS_HIP(q.alloc(2 * (size_t)n));
    LS_HIP(a.alloc(2 * (size_t)n));
    LS_HIP(hipMemcpy(q.p, tan_lo_hi, (size_t)n * 8, hipMemcpyHostToDevice));
    ls::launch_chan_query(tr->stream, project_params(tr), q.p, n, a.p);
    LS_HIP(hipGetLastError());
    LS_HIP(hipStreamSynchronize(tr->stream));
    LS_HIP(hipMemcpy(lut_search, a.p, (size_t)n * 2, hipMemcpyDeviceToHost));
    return LS_OK;
}

}  // extern "C"

int ls_debug_expand_hits(void *dst_points32, const void *hits8, uint32_t n, const float *sin_theta, const float *cos_theta,
                         const float *cs_phi, uint32_t V, uint32_t H)
{
    if (!n) return LS_OK;
    if (!dst_points32 || !hits8 || !sin_theta || !cos_theta || !cs_phi || !V || !H) return LS_ERR_INVALID_ARGUMENT;
    lsi::expand_hits_range(static_cast<uint8_t *>(dst_points32), static_cast<const uint8_t *>(hits8), n, sin_theta, cos_theta, cs_phi, V, H);
    return LS_OK;
}

