// ls_rays.cpp -- ls_trace_rays / ls_trace_rays_host: closest hits of caller-supplied rays against the committed scene;
// ls_occluded_rays / ls_occluded_rays_host: whether each ray hits anything (the same query set and walk, stopping at a hit);
// ls_closest_points / ls_closest_points_host: the nearest surface point to each caller point (the same query set, a
// distance-ordered walk: ls_points.hip);
// ls_hit_attributes / ls_hit_attributes_host: surface attributes of hit records (no hierarchy: a gather, ls_attr.hip; at the end);
// ls_apply_return_model / ls_apply_return_model_host: sensor returns from hit records (the same gather, a model on top of it and
// an ordered compaction: ls_returns.hip; after them).
// ls_trace_scene_sweep / ls_trace_scene_sweep_host: a frame whose sensor moves during the turn -- the shard's rays through per-column
// poses, the closest-hit walk over them, an ordered pack (ls_sweep.hip; at the end); ls_sweep_poses_constant_twist: a pose table.
// ls_trace_scene_beams / ls_trace_scene_beams_host: a frame of diverging beams -- S sub-rays per ray of the shard, the same walk over
// them, the echoes of every beam and an ordered pack of the selected returns (ls_beam.hip; after the sweep);
// ls_beam_pattern_rings: a sample pattern.
//
// The query set (ls_tracer::RayQuery) is a hierarchy set of its own -- one hierarchy per geometry, built by the kernels of
// the instanced commit (hier_layout / hier_build, ls_commit.cpp) into buffers nothing in the frame path reads or writes,
// its sort scratch included, so that no later commit or frame can leave it stale keys, and frames issued after a query on
// other streams may overlap it.  It is built lazily: the first query after a commit builds what the set lacks.
//   * mesh space when the geometry's mesh -> sensor map has a usable inverse (inst_inverse): a pose change costs nothing;
//   * the SENSOR frame otherwise (a singular pose -- a mesh scaled to zero to hide it -- or a scale ratio above 10^3):
//     identity direction map, rebuilt when its pose changes.
// What a slot was built from (vertex / index upload, mode, pose) is kept per slot: a query after a commit that changed only
// poses builds nothing; new vertices refit that geometry (its sorted order is kept in the set's own keys), new indices rebuild it.
#include "ls_internal.h"
#include "ls_return_model.h"
#include "ls_beam.h"

#include <algorithm>
#include <cmath>

namespace lsi {

namespace {

constexpr uint32_t kMaxRayLaunches = (uint32_t)ls::kMaxGeoms / (uint32_t)ls::kGeomsPerLaunch;

bool same_floats(const float *a, const float *b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }

// the registry's geometry of layout entry i, provided it still is what the last commit laid out (every query's check)
int committed_geometry(ls_tracer *tr, size_t i, Geometry **out)
{
    auto it = tr->geoms.find(tr->layout[i].name);
    if (it == tr->geoms.end()) return fail(tr, LS_ERR_NOT_COMMITTED, "geometry removed since the last commit");
    Geometry &ge = it->second;
    if (ge.id != tr->slot_geom_ids[i] || ge.n_tris != tr->slot_tri_first[i + 1] - tr->slot_tri_first[i] || !ge.has_verts || !ge.has_idx)
        return fail(tr, LS_ERR_NOT_COMMITTED, "the geometries changed since the last commit");
    *out = &ge;
    return LS_OK;
}

// the query set brought up to date with the committed layout and the geometries' current data (stream-ordered on s)
int ray_query_prepare(ls_tracer *tr, hipStream_t s, std::vector<Geometry *> &order, std::vector<bool> &sensor_frame)
{
    ls_tracer::RayQuery &q = tr->rq;
    const size_t n = tr->layout.size();
    order.assign(n, nullptr);
    sensor_frame.assign(n, false);
    std::vector<int> ids(n);
    std::vector<uint32_t> firsts(2 * n);   // where every geometry's vertices and triangles start in the layout
    for (size_t i = 0; i < n; ++i) {
        int rc0;
        if ((rc0 = committed_geometry(tr, i, &order[i]))) return rc0;
        Geometry &ge = *order[i];
        ids[i] = ge.id;
        firsts[2 * i] = tr->layout[i].vfirst;
        firsts[2 * i + 1] = tr->layout[i].tfirst;
        double minv[9], o[3], cond;
        sensor_frame[i] = !inst_inverse(tr, ge, minv, o, &cond);
    }
    const uint32_t g = tr->committed_leaf_size;
    HierSet hs{&q.records, &q.nodes, &q.wide_nodes, &q.range_boxes, &q.slots, &q.verts, &q.keys_a, &q.keys_b, &q.vals_b, &q.sort_temp, nullptr};
    int rc;
    const bool fresh = q.layout_ids != ids || q.layout_firsts != firsts || q.leaf != g || q.slots.size() != n;
    if (fresh) {
        uint32_t nodes = 0;
        if ((rc = hier_layout(tr, hs, order, g, &nodes))) return rc;
        q.built.assign(n, ls_tracer::RayQuerySlot());
        q.layout_ids = ids;
        q.layout_firsts = firsts;
        q.leaf = g;
    }
    std::vector<uint8_t> todo(n, 0);   // 1 build, 2 refit
    long count = 0;
    uint32_t biggest = 0;
    for (size_t i = 0; i < n; ++i) {
        const Geometry &ge = *order[i];
        const ls_tracer::RayQuerySlot &b = q.built[i];
        const bool sf = sensor_frame[i];
        bool same = b.valid && b.geom_id == ge.id && b.idx_gen == ge.idx_gen && b.sensor_frame == sf;
        if (same && b.vert_gen == ge.vert_gen && (!sf || (same_floats(b.affine, ge.affine, 12) && same_floats(b.rinv, tr->rinv, 9) &&
                                                         same_floats(b.t, tr->t, 3))))
            continue;
        todo[i] = same ? 2 : 1;   // (same order, same topology: the vertices moved -- a refit)
        ++count;
        biggest = std::max(biggest, ge.n_tris);
    }
    q.last_built = count;
    if (!count) return LS_OK;
    if ((rc = ensure(tr, q.verts, (size_t)tr->n_verts * 3))) return rc;
    if ((rc = ensure(tr, q.keys_a, tr->n_tris))) return rc;
    if ((rc = ensure(tr, q.keys_b, tr->n_tris))) return rc;
    if ((rc = ensure(tr, q.vals_b, tr->n_tris))) return rc;
    if ((rc = ensure(tr, q.sort_temp, ls::sort_temp_bytes(biggest)))) return rc;
    if (!q.d_maxabs) LS_HIP(hipMalloc(reinterpret_cast<void **>(&q.d_maxabs), ls::kMaxGeoms * 4));
    LS_HIP(hipMemsetAsync(q.d_maxabs, 0, n * 4, s));
    hs.d_maxabs = q.d_maxabs;
    static const float kIdA[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, kIdR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kZero[3] = {0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        if (!todo[i]) continue;
        const Geometry &ge = *order[i];
        const bool sf = sensor_frame[i];
        // mesh space: the vertices as uploaded; sensor frame: through the frame's own transform (the bits of k_transform)
        if ((rc = hier_build(tr, hs, s, i, ge, tr->layout[i].vfirst, tr->layout[i].tfirst, sf ? ge.affine : kIdA, sf ? tr->rinv : kIdR,
                             sf ? tr->t : kZero, g, todo[i] == 2, true)))
            return rc;
    }
    LS_HIP(hipGetLastError());
    // the extent of every rebuilt hierarchy (its box widening is scaled by it)
    std::vector<uint32_t> bits(n, 0u);
    LS_HIP(hipMemcpyAsync(bits.data(), q.d_maxabs, n * 4, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i) {
        if (!todo[i]) continue;
        const Geometry &ge = *order[i];
        ls_tracer::RayQuerySlot &b = q.built[i];
        b.valid = true;
        b.geom_id = ge.id;
        b.vert_gen = ge.vert_gen;
        b.idx_gen = ge.idx_gen;
        b.sensor_frame = sensor_frame[i];
        std::memcpy(b.affine, ge.affine, sizeof(b.affine));
        std::memcpy(b.rinv, tr->rinv, sizeof(b.rinv));
        std::memcpy(b.t, tr->t, sizeof(b.t));
        std::memcpy(&b.maxabs, &bits[i], 4);
    }
    return LS_OK;
}

// the launch descriptor of layout entry i for this query
void ray_geom(const ls_tracer *tr, size_t i, const Geometry &ge, bool sensor_frame, ls::RayGeom &rg)
{
    const ls_tracer::RayQuery &q = tr->rq;
    const ls_tracer::InstSlot &sl = q.slots[i];
    std::memset(static_cast<void *>(&rg), 0, sizeof(rg));
    rg.node_first = sl.node_first;
    rg.rec_first = sl.rec_first;
    rg.n_leaves = sl.n_leaves;
    rg.n_tris = ge.n_tris;
    rg.gid_first = tr->layout[i].tfirst;
    rg.geom_id = (uint32_t)ge.id;
    rg.prim_shift = ge.quad ? 1u : 0u;
    std::memcpy(rg.m.a, ge.affine, sizeof(rg.m.a));
    std::memcpy(rg.m.rinv, tr->rinv, sizeof(rg.m.rinv));
    std::memcpy(rg.m.t, tr->t, sizeof(rg.m.t));
    const float maxabs = q.built[i].maxabs;
    double minv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0}, cond = 1.0;
    if (sensor_frame) {
        rg.xform = 0;
    } else {
        inst_inverse(tr, ge, minv, o, &cond);
        static const float kIdentity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        rg.xform = std::memcmp(ge.affine, kIdentity, sizeof(kIdentity)) == 0 ? 2 : 1;
    }
    float omax = 0.0f, row = 0.0f;
    for (int k = 0; k < 3; ++k) { rg.o[k] = (float)o[k]; omax = std::max(omax, std::fabs(rg.o[k])); }
    for (int k = 0; k < 9; ++k) rg.minv[k] = (float)minv[k];
    for (int r = 0; r < 3; ++r) row = std::max(row, std::fabs(rg.minv[3 * r]) + std::fabs(rg.minv[3 * r + 1]) + std::fabs(rg.minv[3 * r + 2]));
    // The frame's widening (ls_trace.cpp) for a ray from the sensor origin -- the rounding of o and of minv * d along the way to
    // any box, times the conditioning of the map, a factor of ten in hand -- plus what a ray origin o_r adds: o_m = minv * o_r
    // + o rounds by a few ulps of ||minv|| |o_r| + |o|, and the way to a box grows by as much ("Ray queries").
    const float c = 4e-6f * (float)std::max(1.0, cond);
    rg.eps = c * (omax + 2.0f * maxabs);
    rg.eps_o = 2.0f * c * row;
}


// The largest eigenvalue of the symmetric 3 x 3 matrix S (row-major), closed form.
double sym3_lambda_max(const double *S)
{
    const double p1 = S[1] * S[1] + S[2] * S[2] + S[5] * S[5];
    const double qm = (S[0] + S[4] + S[8]) / 3.0;
    if (p1 == 0.0) return std::max(S[0], std::max(S[4], S[8]));
    const double a = S[0] - qm, b = S[4] - qm, c = S[8] - qm;
    const double p = std::sqrt((a * a + b * b + c * c + 2.0 * p1) / 6.0);
    const double B[9] = {a / p, S[1] / p, S[2] / p, S[1] / p, b / p, S[5] / p, S[2] / p, S[5] / p, c / p};
    const double det = B[0] * (B[4] * B[8] - B[5] * B[7]) - B[1] * (B[3] * B[8] - B[5] * B[6]) + B[2] * (B[3] * B[7] - B[4] * B[6]);
    const double r = std::min(1.0, std::max(-1.0, det / 2.0));
    return qm + 2.0 * p * std::cos(std::acos(r) / 3.0);
}

// ls_closest_points: the margins that make "s2 * (squared distance of p_m to a box widened by e0 + e1 |p|inf)" a lower bound of
// the float32 d2 closest_on_triangle gives for every triangle below the box:
//   * the ray query's own widening (rg.eps, rg.eps_o: the rounding of p_m = minv p + o and of the corners' way through the
//     frame's transform, in the hierarchy's units);
//   * delta = 8e-6 (|p|inf + W) in the sensor frame, W >= every intermediate of the corners' transform: the exact test's own
//     rounding (its q is a point of the triangle up to a few ulps of the coordinates, d2 = |p - q|^2 from that q) and the
//     corners' rounding where translations cancel -- carried into the hierarchy's units by 1 / s;
//   * s <= sigma_min of the linear part of hierarchy space -> sensor frame: 1 / ||minv||_2 in double, six digits kept in hand.
void point_margins(const ls_tracer *tr, size_t i, const Geometry &ge, bool sensor_frame, const ls::RayGeom &rg, ls::PointMargins &pm, size_t k)
{
    const double maxabs = tr->rq.built[i].maxabs;
    double s = 1.0, W = maxabs;
    if (!sensor_frame) {
        double minv[9], o[3], cond, S[9];
        inst_inverse(tr, ge, minv, o, &cond);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) S[3 * r + c] = minv[r] * minv[c] + minv[3 + r] * minv[3 + c] + minv[6 + r] * minv[6 + c];
        s = (1.0 - 1e-6) / std::sqrt(sym3_lambda_max(S));
        double arow = 0.0, rrow = 0.0, amax = 0.0, tmax = 0.0;
        for (int r = 0; r < 3; ++r) {
            arow = std::max(arow, std::fabs((double)ge.affine[4 * r]) + std::fabs((double)ge.affine[4 * r + 1]) + std::fabs((double)ge.affine[4 * r + 2]));
            rrow = std::max(rrow, std::fabs((double)tr->rinv[3 * r]) + std::fabs((double)tr->rinv[3 * r + 1]) + std::fabs((double)tr->rinv[3 * r + 2]));
            amax = std::max(amax, std::fabs((double)ge.affine[4 * r + 3]));
            tmax = std::max(tmax, std::fabs((double)tr->t[r]));
        }
        W = std::max(1.0, rrow) * (arow * maxabs + amax + tmax);
    }
    const double kd = 8e-6;
    // rounded up (e0, e1) and down (s2): a float conversion moves a value by less than 6e-8 of itself
    pm.e0[k] = (float)(((double)rg.eps + kd * W / s) * (1.0 + 1e-6));
    pm.e1[k] = (float)(((double)rg.eps_o + kd / s) * (1.0 + 1e-6));
    pm.s2[k] = (float)(s * s * (1.0 - 1e-6));
}

}  // namespace

void ray_query_release(ls_tracer *tr)
{
    ls_tracer::RayQuery &q = tr->rq;
    if (q.ev_done) (void)hipEventSynchronize(q.ev_done);
    release(q.records); release(q.nodes); release(q.wide_nodes); release(q.range_boxes); release(q.verts);
    release(q.keys_a); release(q.keys_b); release(q.vals_b); release(q.sort_temp); release(q.spill); release(q.io);
    release(q.sweep_rays); release(q.sweep_hits); release(q.sweep_counts);
    release(q.beam_rays); release(q.beam_hits); release(q.beam_blocks); release(q.beam_counts);
    if (q.d_maxabs) (void)hipFree(q.d_maxabs);
    if (q.d_counters) (void)hipFree(q.d_counters);
    if (q.ev_ready) (void)hipEventDestroy(q.ev_ready);
    if (q.ev_done) (void)hipEventDestroy(q.ev_done);
    q.d_maxabs = q.d_counters = nullptr;
    q.ev_ready = q.ev_done = nullptr;
}

namespace {

// the queries: what one launch over a geometry batch runs, what it reads per query and what it writes per result
struct RayQueryKind {
    void (*launch)(hipStream_t, uint32_t, const void *, uint32_t, const ls::RayBatch &, const ls::PointMargins &, const ls::WideNode *,
                   const ls::TriRecord *, uint32_t, void *, uint32_t *, uint32_t *);
    size_t in_bytes;    // per query: a 32-byte ray or a 16-byte point (16-byte aligned)
    size_t out_bytes;   // per result: an ls_hit, one byte, or an ls_closest record
    size_t out_align;   // 16, or 1 (any address)
    bool points;        // the launch takes PointMargins (ls_closest_points)
    const char *misaligned;
};
void launch_closest_hits(hipStream_t s, uint32_t blocks, const void *in, uint32_t n, const ls::RayBatch &batch, const ls::PointMargins &,
                         const ls::WideNode *wide, const ls::TriRecord *records, uint32_t leaf, void *out, uint32_t *counter, uint32_t *spill)
{
    ls::launch_trace_rays(s, blocks, in, n, batch, wide, records, leaf, out, counter, spill);
}
void launch_any_hits(hipStream_t s, uint32_t blocks, const void *in, uint32_t n, const ls::RayBatch &batch, const ls::PointMargins &,
                     const ls::WideNode *wide, const ls::TriRecord *records, uint32_t leaf, void *out, uint32_t *counter, uint32_t *spill)
{
    ls::launch_occluded_rays(s, blocks, in, n, batch, wide, records, leaf, out, counter, spill);
}
const RayQueryKind kClosest = {launch_closest_hits, 32, 16, 16, false, "rays and hit records must be 16-byte aligned"};
const RayQueryKind kOccluded = {launch_any_hits, 32, 1, 1, false, "rays must be 16-byte aligned"};
const RayQueryKind kNearest = {ls::launch_closest_points, 16, 32, 16, true, "points and result records must be 16-byte aligned"};

// What every query on the hierarchies does around and in its walk (ls_trace_rays and its siblings; ls_trace_scene_sweep, which
// puts a pass of its own on either side of the walk):
//   query_enter  after everything already issued on the handle -- its frames in flight, its mesh copies -- on stream s;
//   query_walk   the query set brought up to date, the counters, one launch per batch of kGeomsPerLaunch geometries;
//   query_leave  what the handle issues next (mesh copies, commits, the next query) comes after this query; frames of the
//                three-stream rotation that need none of that do not wait for it.
int query_enter(ls_tracer *tr, hipStream_t s)
{
    ls_tracer::RayQuery &q = tr->rq;
    int rc;
    if ((rc = flush_pipeline(tr))) return rc;
    if (!q.ev_ready) LS_HIP(hipEventCreateWithFlags(&q.ev_ready, hipEventDisableTiming));
    if (!q.ev_done) LS_HIP(hipEventCreateWithFlags(&q.ev_done, hipEventDisableTiming));
    if (s != tr->stream) {
        LS_HIP(hipEventRecord(q.ev_ready, tr->stream));
        LS_HIP(hipStreamWaitEvent(s, q.ev_ready, 0));
    }
    return LS_OK;
}

int query_walk(ls_tracer *tr, hipStream_t s, const void *d_rays, uint32_t n, void *d_out, const RayQueryKind &kind)
{
    ls_tracer::RayQuery &q = tr->rq;
    int rc;
    std::vector<Geometry *> order;
    std::vector<bool> sensor_frame;
    if ((rc = ray_query_prepare(tr, s, order, sensor_frame))) return rc;
    if ((rc = ensure(tr, q.spill, ls::trace_spill_bytes(tr->trace_blocks) / 4))) return rc;
    if (!q.d_counters) LS_HIP(hipMalloc(reinterpret_cast<void **>(&q.d_counters), kMaxRayLaunches * 4));
    const uint32_t launches = (uint32_t)((order.size() + ls::kGeomsPerLaunch - 1) / ls::kGeomsPerLaunch);
    LS_HIP(hipMemsetAsync(q.d_counters, 0, (size_t)launches * 4, s));
    // geometries in ascending geomID batches of kGeomsPerLaunch: each launch starts from what the ones before found
    for (uint32_t b = 0; b < launches; ++b) {
        ls::RayBatch batch;
        std::memset(static_cast<void *>(&batch), 0, sizeof(batch));
        const size_t first = (size_t)b * ls::kGeomsPerLaunch, last = std::min(order.size(), first + ls::kGeomsPerLaunch);
        batch.n = (uint32_t)(last - first);
        batch.first = b == 0 ? 1u : 0u;
        ls::PointMargins pm;
        std::memset(static_cast<void *>(&pm), 0, sizeof(pm));
        pm.last = b + 1 == launches ? 1u : 0u;
        for (size_t i = first; i < last; ++i) {
            ray_geom(tr, i, *order[i], sensor_frame[i], batch.g[i - first]);
            if (kind.points) point_margins(tr, i, *order[i], sensor_frame[i], batch.g[i - first], pm, i - first);
        }
        kind.launch(s, tr->trace_blocks, d_rays, n, batch, pm, q.wide_nodes.p, q.records.p, q.leaf, d_out, q.d_counters + b, q.spill.p);
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}

int query_leave(ls_tracer *tr, hipStream_t s)
{
    ls_tracer::RayQuery &q = tr->rq;
    if (s != tr->stream) {
        LS_HIP(hipEventRecord(q.ev_done, s));
        LS_HIP(hipStreamWaitEvent(tr->stream, q.ev_done, 0));
    }
    return LS_OK;
}

int rays_locked(ls_tracer *tr, hipStream_t s, const void *d_rays, uint32_t n, void *d_out, const RayQueryKind &kind)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (n && (!d_rays || !d_out)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null rays or output");
    if (((uintptr_t)d_rays & 15u) || ((uintptr_t)d_out & (kind.out_align - 1u))) return fail(tr, LS_ERR_INVALID_ARGUMENT, kind.misaligned);
    if (n > 0xFFF00000u) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many rays in one call");
    tr->rq.last_built = 0;
    if (!tr->committed || tr->n_tris == 0) return -1;   // as ls_trace_scene; nothing is written
    if (!n) return LS_OK;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    if ((rc = query_walk(tr, s, d_rays, n, d_out, kind))) return rc;
    return query_leave(tr, s);
}

// the host-memory variant: rays and results staged in q.io, on the handle's stream; returns when out is filled
int rays_host_locked(ls_tracer *tr, const void *rays, uint32_t n, void *out, const RayQueryKind &kind)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (n && (!rays || !out)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null rays or output");
    if (n > 0xFFF00000u) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many rays in one call");
    tr->rq.last_built = 0;
    if (!tr->committed || tr->n_tris == 0) return -1;   // (before n = 0: the same answer as the device entry point)
    if (!n) return LS_OK;
    ls_tracer::RayQuery &q = tr->rq;
    hipStream_t s = tr->stream;
    int rc;
    if ((rc = flush_pipeline(tr))) return rc;
    if ((rc = ensure(tr, q.io, (size_t)n * (kind.in_bytes + kind.out_bytes)))) return rc;   // (a growing buffer: the frame path's frames in flight never read it)
    uint8_t *d_rays = q.io.p, *d_out = q.io.p + (size_t)n * kind.in_bytes;
    LS_HIP(hipMemcpyAsync(d_rays, rays, (size_t)n * kind.in_bytes, hipMemcpyHostToDevice, s));
    if ((rc = rays_locked(tr, s, d_rays, n, d_out, kind))) return rc;
    LS_HIP(hipMemcpyAsync(out, d_out, (size_t)n * kind.out_bytes, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    return LS_OK;
}

// ---- ls_hit_attributes: no hierarchy, a gather over hit records (ls_attr.hip) -------------------------------------------

// the table k_hit_attributes reads, one entry per geomID up to the highest committed one (free ids stay zero), from the committed
// layout and the geometries' current buffers and poses (committed_geometry's checks); uploaded on s when it differs from what
// the device holds
int attr_table_prepare(ls_tracer *tr, hipStream_t s)
{
    ls_tracer::HitAttr &a = tr->ha;
    const size_t n = tr->layout.size();
    int max_id = -1;
    for (size_t i = 0; i < n; ++i) max_id = std::max(max_id, tr->slot_geom_ids[i]);
    std::vector<ls::AttrGeom> tab((size_t)(max_id + 1));
    if (!tab.empty()) std::memset(static_cast<void *>(tab.data()), 0, tab.size() * sizeof(ls::AttrGeom));
    for (size_t i = 0; i < n; ++i) {
        Geometry *gp = nullptr;
        int rc0;
        if ((rc0 = committed_geometry(tr, i, &gp))) return rc0;
        const Geometry &ge = *gp;
        ls::AttrGeom &e = tab[(size_t)ge.id];
        e.verts = static_cast<const uint8_t *>(ge.raw());
        e.idx = ge.idx();
        e.stride = ge.stride;
        e.n_elems = ge.n_elems;
        e.n_verts = ge.n_verts;
        e.quad = ge.quad ? 1u : 0u;
        std::memcpy(e.m.a, ge.affine, sizeof(e.m.a));
        std::memcpy(e.m.rinv, tr->rinv, sizeof(e.m.rinv));
        std::memcpy(e.m.t, tr->t, sizeof(e.m.t));
    }
    const size_t bytes = tab.size() * sizeof(ls::AttrGeom);
    if (tab.size() == a.current.size() && (!bytes || std::memcmp(tab.data(), a.current.data(), bytes) == 0)) return LS_OK;
    a.current.clear();   // (whatever fails from here on, the next call refreshes: ensure may give the table another buffer)
    int rc;
    if ((rc = ensure(tr, a.table, tab.size()))) return rc;
    if (!a.ev_stage) LS_HIP(hipEventCreateWithFlags(&a.ev_stage, hipEventDisableTiming));
    LS_HIP(hipEventSynchronize(a.ev_stage));   // (the copy of an earlier refresh may still be reading the staging buffer)
    if (a.stage_cap < tab.size()) {
        if (a.h_stage) LS_HIP(hipHostFree(a.h_stage));
        a.h_stage = nullptr;
        a.stage_cap = 0;
        LS_HIP(hipHostMalloc(reinterpret_cast<void **>(&a.h_stage), bytes + bytes / 8, hipHostMallocDefault));
        a.stage_cap = (bytes + bytes / 8) / sizeof(ls::AttrGeom);
    }
    std::memcpy(static_cast<void *>(a.h_stage), tab.data(), bytes);
    LS_HIP(hipMemcpyAsync(a.table.p, a.h_stage, bytes, hipMemcpyHostToDevice, s));
    LS_HIP(hipEventRecord(a.ev_stage, s));
    a.current.swap(tab);
    return LS_OK;
}

// argument checks, return codes and stream order of rays_locked; LS_INFO_RAY_QUERY_BUILT is left as it is
int attr_locked(ls_tracer *tr, hipStream_t s, const void *d_rays, uint32_t n_rays, const void *d_hits, const uint32_t *d_count, uint32_t n,
                void *d_out)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (n && (!d_hits || !d_out)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records or output");
    if (((uintptr_t)d_rays & 15u) || ((uintptr_t)d_hits & 15u) || ((uintptr_t)d_out & 15u) || ((uintptr_t)d_count & 3u))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "rays, hit records and attribute records must be 16-byte aligned, the count 4-byte aligned");
    if (n > 0xFFF00000u) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records in one call");
    if (!tr->committed || tr->n_tris == 0) return -1;   // as ls_trace_scene; nothing is written
    if (!n) return LS_OK;
    int rc;
    // after everything already issued on the handle: its frames in flight (whose hit records these may be), its mesh copies
    if ((rc = flush_pipeline(tr))) return rc;
    ls_tracer::RayQuery &q = tr->rq;
    if (!q.ev_ready) LS_HIP(hipEventCreateWithFlags(&q.ev_ready, hipEventDisableTiming));
    if (!q.ev_done) LS_HIP(hipEventCreateWithFlags(&q.ev_done, hipEventDisableTiming));
    if (s != tr->stream) {
        LS_HIP(hipEventRecord(q.ev_ready, tr->stream));
        LS_HIP(hipStreamWaitEvent(s, q.ev_ready, 0));
    }
    if ((rc = attr_table_prepare(tr, s))) return rc;
    ls::launch_hit_attributes(s, d_hits, d_count, n, d_rays, n_rays, tables(tr), tr->ha.table.p, (uint32_t)tr->ha.current.size(), d_out);
    LS_HIP(hipGetLastError());
    if (s != tr->stream) {
        LS_HIP(hipEventRecord(q.ev_done, s));
        LS_HIP(hipStreamWaitEvent(tr->stream, q.ev_done, 0));
    }
    return LS_OK;
}

// the host-memory variant: hit records, rays and results staged in q.io, on the handle's stream; returns when out is filled
int attr_host_locked(ls_tracer *tr, const void *rays, uint32_t n_rays, const void *hits, uint32_t n, void *out)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (n && (!hits || !out)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records or output");
    if (n > 0xFFF00000u || (rays && n_rays > 0xFFF00000u)) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many records in one call");
    if (!tr->committed || tr->n_tris == 0) return -1;   // (before n = 0: the same answer as the device entry point)
    if (!n) return LS_OK;
    ls_tracer::RayQuery &q = tr->rq;
    hipStream_t s = tr->stream;
    int rc;
    if ((rc = flush_pipeline(tr))) return rc;
    const size_t hit_bytes = (size_t)n * 16, ray_bytes = rays ? (size_t)n_rays * 32 : 0, out_bytes = (size_t)n * 48;
    if ((rc = ensure(tr, q.io, hit_bytes + ray_bytes + out_bytes))) return rc;
    uint8_t *d_hits = q.io.p, *d_rays = q.io.p + hit_bytes, *d_out = d_rays + ray_bytes;
    LS_HIP(hipMemcpyAsync(d_hits, hits, hit_bytes, hipMemcpyHostToDevice, s));
    if (ray_bytes) LS_HIP(hipMemcpyAsync(d_rays, rays, ray_bytes, hipMemcpyHostToDevice, s));
    if ((rc = attr_locked(tr, s, rays ? d_rays : nullptr, n_rays, d_hits, nullptr, n, d_out))) return rc;
    LS_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    return LS_OK;
}

// ---- ls_apply_return_model: the gather again, the return model on top, an ordered compaction (ls_returns.hip) ---------------

// argument checks, return codes and stream order of attr_locked (the model itself was checked before the handle was entered)
int returns_locked(ls_tracer *tr, hipStream_t s, const ls_return_model *model, uint32_t frame_index, const void *d_rays, uint32_t n_rays,
                   const void *d_hits, const uint32_t *d_count, uint32_t n, const float *d_refl, uint32_t n_refl, void *d_points32,
                   void *d_hits_out, uint32_t *d_n_out)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!d_n_out || (n && !d_hits)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records or count output");
    if (((uintptr_t)d_rays & 15u) || ((uintptr_t)d_hits & 15u) || ((uintptr_t)d_points32 & 15u) || ((uintptr_t)d_hits_out & 15u) ||
        ((uintptr_t)d_count & 3u) || ((uintptr_t)d_n_out & 3u) || ((uintptr_t)d_refl & 3u))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "rays, hit records and points must be 16-byte aligned, counts and reflectivities 4-byte aligned");
    if (n > 0xFFF00000u) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records in one call");
    if (!tr->committed || tr->n_tris == 0) return -1;   // as ls_trace_scene; nothing is written
    int rc;
    if ((rc = flush_pipeline(tr))) return rc;
    ls_tracer::RayQuery &q = tr->rq;
    ls_tracer::HitAttr &a = tr->ha;
    if (!q.ev_ready) LS_HIP(hipEventCreateWithFlags(&q.ev_ready, hipEventDisableTiming));
    if (!q.ev_done) LS_HIP(hipEventCreateWithFlags(&q.ev_done, hipEventDisableTiming));
    if (s != tr->stream) {
        LS_HIP(hipEventRecord(q.ev_ready, tr->stream));
        LS_HIP(hipStreamWaitEvent(s, q.ev_ready, 0));
    }
    if (!n) {
        LS_HIP(hipMemsetAsync(d_n_out, 0, 4, s));   // no record: no return
    } else {
        if ((rc = attr_table_prepare(tr, s))) return rc;
        if ((rc = ensure(tr, a.park, 2 * (size_t)n))) return rc;
        if ((rc = ensure(tr, a.block_counts, ls::returns_block_count(n)))) return rc;
        ls::launch_returns(s, d_hits, d_count, n, d_rays, n_rays, tables(tr), a.table.p, (uint32_t)a.current.size(), *model, frame_index,
                           n_refl ? d_refl : nullptr, n_refl, a.park.p, a.block_counts.p, d_points32, d_hits_out, d_n_out);
        LS_HIP(hipGetLastError());
    }
    if (s != tr->stream) {
        LS_HIP(hipEventRecord(q.ev_done, s));
        LS_HIP(hipStreamWaitEvent(tr->stream, q.ev_done, 0));
    }
    return LS_OK;
}

// the host-memory variant: inputs and results staged in q.io, on the handle's stream; the count comes back first, then as many
// records; returns when the outputs are filled
int returns_host_locked(ls_tracer *tr, const ls_return_model *model, uint32_t frame_index, const void *rays, uint32_t n_rays, const void *hits,
                        uint32_t n, const float *refl, uint32_t n_refl, void *points32, void *hits_out, uint32_t *n_out)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!n_out || (n && !hits)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records or count output");
    if (n > 0xFFF00000u || (rays && n_rays > 0xFFF00000u)) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many records in one call");
    if (!tr->committed || tr->n_tris == 0) return -1;   // (before n = 0: the same answer as the device entry point)
    if (!n) {
        *n_out = 0;
        return LS_OK;
    }
    ls_tracer::RayQuery &q = tr->rq;
    hipStream_t s = tr->stream;
    int rc;
    if ((rc = flush_pipeline(tr))) return rc;
    const size_t hit_bytes = (size_t)n * 16, ray_bytes = rays ? (size_t)n_rays * 32 : 0, point_bytes = points32 ? (size_t)n * 32 : 0,
                 out_bytes = hits_out ? hit_bytes : 0, refl_bytes = ((size_t)n_refl * 4 + 15) & ~(size_t)15;
    if ((rc = ensure(tr, q.io, hit_bytes + ray_bytes + point_bytes + out_bytes + refl_bytes + 16))) return rc;
    uint8_t *d_hits = q.io.p, *d_rays = d_hits + hit_bytes, *d_points = d_rays + ray_bytes, *d_out = d_points + point_bytes,
            *d_refl = d_out + out_bytes, *d_n = d_refl + refl_bytes;
    LS_HIP(hipMemcpyAsync(d_hits, hits, hit_bytes, hipMemcpyHostToDevice, s));
    if (ray_bytes) LS_HIP(hipMemcpyAsync(d_rays, rays, ray_bytes, hipMemcpyHostToDevice, s));
    if (n_refl) LS_HIP(hipMemcpyAsync(d_refl, refl, (size_t)n_refl * 4, hipMemcpyHostToDevice, s));
    if ((rc = returns_locked(tr, s, model, frame_index, rays ? d_rays : nullptr, n_rays, d_hits, nullptr, n, reinterpret_cast<const float *>(d_refl),
                             n_refl, points32 ? d_points : nullptr, hits_out ? d_out : nullptr, reinterpret_cast<uint32_t *>(d_n))))
        return rc;
    uint32_t kept = 0;
    LS_HIP(hipMemcpyAsync(&kept, d_n, 4, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    if (kept > n) return fail(tr, LS_ERR_HIP, "ls_apply_return_model: more returns than records");
    if (kept && points32) LS_HIP(hipMemcpyAsync(points32, d_points, (size_t)kept * 32, hipMemcpyDeviceToHost, s));
    if (kept && hits_out) LS_HIP(hipMemcpyAsync(hits_out, d_out, (size_t)kept * 16, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    *n_out = kept;
    return LS_OK;
}

// ---- ls_trace_scene_sweep: a frame whose sensor moves during the turn (ls_sweep.hip around the ray queries' walk) ----------

// argument checks first (none of them needs a commit), then the return codes, stream order and hierarchies of rays_locked
int sweep_locked(ls_tracer *tr, hipStream_t s, const float *d_col_pose, uint32_t n_cols, uint32_t flags, void *d_points32, void *d_hits,
                 uint32_t *d_n_points, uint32_t capacity, void *d_rays_out)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!d_col_pose || !d_n_points) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null pose table or count output");
    if (n_cols != tr->H) return fail(tr, LS_ERR_INVALID_ARGUMENT, "one pose per azimuth column of the full raster (LS_INFO_AZIMUTH_COUNT)");
    if (flags & ~(uint32_t)LS_SWEEP_DESKEW) return fail(tr, LS_ERR_INVALID_ARGUMENT, "unknown sweep flags");
    if (((uintptr_t)d_col_pose & 3u) || ((uintptr_t)d_n_points & 3u) || ((uintptr_t)d_points32 & 15u) || ((uintptr_t)d_hits & 15u) ||
        ((uintptr_t)d_rays_out & 15u))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "points, hit records and rays must be 16-byte aligned, the poses and the count 4-byte aligned");
    const uint32_t nq = shard_rays(tr);
    if (capacity < nq) return fail(tr, LS_ERR_INVALID_ARGUMENT, "capacity below the shard's ray count");
    if (nq > 0xFFF00000u) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many rays in one call");
    ls_tracer::RayQuery &q = tr->rq;
    q.last_built = 0;
    if (!tr->committed || tr->n_tris == 0) return -1;   // as ls_trace_scene; nothing is written, the count included
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    if ((rc = ensure(tr, q.sweep_rays, (size_t)nq * 32))) return rc;
    if ((rc = ensure(tr, q.sweep_hits, (size_t)nq * 16))) return rc;
    if ((rc = ensure(tr, q.sweep_counts, ls::sweep_block_count(nq)))) return rc;
    const ls::SensorTables tb = tables(tr);
    ls::launch_sweep_rays(s, tb, d_col_pose, q.sweep_rays.p, d_rays_out);
    if ((rc = query_walk(tr, s, q.sweep_rays.p, nq, q.sweep_hits.p, kClosest))) return rc;
    ls::launch_sweep_pack(s, tb, q.sweep_hits.p, q.sweep_counts.p, d_col_pose, (flags & LS_SWEEP_DESKEW) != 0, d_points32, d_hits, d_n_points);
    LS_HIP(hipGetLastError());
    return query_leave(tr, s);
}

// the host-memory variant: the poses, the outputs and the optional ray records staged in q.io, on the handle's stream; the count
// comes back first, then as many records; of rays_out only the shard's columns are written
int sweep_host_locked(ls_tracer *tr, const float *col_pose, uint32_t n_cols, uint32_t flags, void *points32, void *hits, uint32_t *n_points,
                      uint32_t capacity, void *rays_out)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!col_pose || !n_points) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null pose table or count output");
    if (n_cols != tr->H) return fail(tr, LS_ERR_INVALID_ARGUMENT, "one pose per azimuth column of the full raster (LS_INFO_AZIMUTH_COUNT)");
    if (flags & ~(uint32_t)LS_SWEEP_DESKEW) return fail(tr, LS_ERR_INVALID_ARGUMENT, "unknown sweep flags");
    const uint32_t nq = shard_rays(tr);
    if (capacity < nq) return fail(tr, LS_ERR_INVALID_ARGUMENT, "capacity below the shard's ray count");
    if (nq > 0xFFF00000u) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many rays in one call");
    tr->rq.last_built = 0;
    if (!tr->committed || tr->n_tris == 0) return -1;
    ls_tracer::RayQuery &q = tr->rq;
    hipStream_t s = tr->stream;
    int rc;
    if ((rc = flush_pipeline(tr))) return rc;
    const size_t point_bytes = points32 ? (size_t)nq * 32 : 0, hit_bytes = hits ? (size_t)nq * 16 : 0, row_bytes = (size_t)tr->H * 32,
                 ray_bytes = rays_out ? (size_t)tr->V * row_bytes : 0, pose_bytes = (size_t)n_cols * 48;
    if ((rc = ensure(tr, q.io, point_bytes + hit_bytes + ray_bytes + pose_bytes + 16))) return rc;
    uint8_t *d_points = q.io.p, *d_hits = d_points + point_bytes, *d_rays = d_hits + hit_bytes, *d_pose = d_rays + ray_bytes,
            *d_n = d_pose + pose_bytes;
    LS_HIP(hipMemcpyAsync(d_pose, col_pose, pose_bytes, hipMemcpyHostToDevice, s));
    if ((rc = sweep_locked(tr, s, reinterpret_cast<const float *>(d_pose), n_cols, flags, points32 ? d_points : nullptr, hits ? d_hits : nullptr,
                           reinterpret_cast<uint32_t *>(d_n), nq, rays_out ? d_rays : nullptr)))
        return rc;
    uint32_t count = 0;
    LS_HIP(hipMemcpyAsync(&count, d_n, 4, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    if (count > nq) return fail(tr, LS_ERR_HIP, "ls_trace_scene_sweep: more points than rays");
    if (count && points32) LS_HIP(hipMemcpyAsync(points32, d_points, (size_t)count * 32, hipMemcpyDeviceToHost, s));
    if (count && hits) LS_HIP(hipMemcpyAsync(hits, d_hits, (size_t)count * 16, hipMemcpyDeviceToHost, s));
    if (rays_out)   // V rows of the shard's naz records, at their place in the rows of H
        LS_HIP(hipMemcpy2DAsync(static_cast<uint8_t *>(rays_out) + (size_t)tr->az0 * 32, row_bytes, d_rays + (size_t)tr->az0 * 32, row_bytes,
                                (size_t)tr->naz * 32, tr->V, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    *n_points = count;
    return LS_OK;
}

// ---- ls_trace_scene_beams: diverging beams with multi-echo returns (ls_beam.hip around the ray queries' walk) --------------

// what both entry points refuse before any device call: an open frame graph, a NULL count, the model, the capacity, the size
int beams_check(ls_tracer *tr, const ls_beam_model *model, const void *n_points, uint32_t capacity)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!n_points) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null count output");
    int status = LS_OK;
    if (const char *why = ls::beam_model_invalid(model, shard_rays(tr), capacity, &status)) return fail(tr, status, why);
    return LS_OK;
}

uint32_t beam_returns(const ls_beam_model *model) { return (uint32_t)__builtin_popcount(model->returns); }

// (beams_check passed) the return codes, stream order and hierarchies of sweep_locked
int beams_locked(ls_tracer *tr, hipStream_t s, const ls_beam_model *model, void *d_points32, void *d_hits, uint32_t *d_echo, uint32_t *d_n_points,
                 uint32_t capacity)
{
    ls_tracer::RayQuery &q = tr->rq;
    q.last_built = 0;
    if (!tr->committed || tr->n_tris == 0) return -1;   // as ls_trace_scene; nothing is written, the count included
    const uint32_t nq = shard_rays(tr), S = model->n_samples, n = nq * S;   // n <= 2^27
    ls::BeamPattern pat;   // the caller's pattern, read here and now: it travels in the kernel arguments
    std::memset(static_cast<void *>(&pat), 0, sizeof(pat));
    for (uint32_t k = 0; k < S; ++k) {
        pat.a[k] = model->pattern[3 * k];
        pat.b[k] = model->pattern[3 * k + 1];
        pat.k[k] = model->pattern[3 * k + 2];
    }
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    if ((rc = ensure(tr, q.beam_rays, (size_t)n * 32))) return rc;
    if ((rc = ensure(tr, q.beam_hits, (size_t)n * 16))) return rc;
    if ((rc = ensure(tr, q.beam_blocks, 3 * (size_t)nq))) return rc;
    if ((rc = ensure(tr, q.beam_counts, (size_t)nq + ls::beam_block_count(nq)))) return rc;
    const ls::SensorTables tb = tables(tr);
    ls::launch_beam_rays(s, tb, pat, S, q.beam_rays.p);
    if ((rc = query_walk(tr, s, q.beam_rays.p, n, q.beam_hits.p, kClosest))) return rc;
    ls::launch_beam_pack(s, tb, pat, S, model->echo_separation, model->min_count, model->returns, q.beam_hits.p, q.beam_blocks.p, q.beam_counts.p,
                         q.beam_counts.p + nq, d_points32, d_hits, d_echo, d_n_points, capacity);
    LS_HIP(hipGetLastError());
    return query_leave(tr, s);
}

// the host-memory variant: the outputs staged in q.io, on the handle's stream; the count comes back first, then as many records
int beams_host_locked(ls_tracer *tr, const ls_beam_model *model, void *points32, void *hits, uint32_t *echo, uint32_t *n_points)
{
    tr->rq.last_built = 0;
    if (!tr->committed || tr->n_tris == 0) return -1;
    ls_tracer::RayQuery &q = tr->rq;
    hipStream_t s = tr->stream;
    int rc;
    if ((rc = flush_pipeline(tr))) return rc;
    const size_t cap = (size_t)beam_returns(model) * shard_rays(tr);   // <= 3 * 2^27
    const size_t point_bytes = points32 ? cap * 32 : 0, hit_bytes = hits ? cap * 16 : 0, echo_bytes = echo ? (cap * 4 + 15) & ~(size_t)15 : 0;
    if ((rc = ensure(tr, q.io, point_bytes + hit_bytes + echo_bytes + 16))) return rc;
    uint8_t *d_points = q.io.p, *d_hits = d_points + point_bytes, *d_echo = d_hits + hit_bytes, *d_n = d_echo + echo_bytes;
    if ((rc = beams_locked(tr, s, model, points32 ? d_points : nullptr, hits ? d_hits : nullptr, echo ? reinterpret_cast<uint32_t *>(d_echo) : nullptr,
                           reinterpret_cast<uint32_t *>(d_n), (uint32_t)cap)))
        return rc;
    uint32_t count = 0;
    LS_HIP(hipMemcpyAsync(&count, d_n, 4, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    if (count > cap) return fail(tr, LS_ERR_HIP, "ls_trace_scene_beams: more returns than the beams can give");
    if (count && points32) LS_HIP(hipMemcpyAsync(points32, d_points, (size_t)count * 32, hipMemcpyDeviceToHost, s));
    if (count && hits) LS_HIP(hipMemcpyAsync(hits, d_hits, (size_t)count * 16, hipMemcpyDeviceToHost, s));
    if (count && echo) LS_HIP(hipMemcpyAsync(echo, d_echo, (size_t)count * 4, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    *n_points = count;
    return LS_OK;
}

}  // namespace

void hit_attr_release(ls_tracer *tr)
{
    ls_tracer::HitAttr &a = tr->ha;
    if (a.ev_stage) { (void)hipEventSynchronize(a.ev_stage); (void)hipEventDestroy(a.ev_stage); }
    if (a.h_stage) (void)hipHostFree(a.h_stage);
    release(a.table); release(a.park); release(a.block_counts);
    a.ev_stage = nullptr;
    a.h_stage = nullptr;
    a.stage_cap = 0;
    a.current.clear();
}

}  // namespace lsi

using namespace lsi;

extern "C" {

int ls_trace_rays(ls_tracer *tr, void *hip_stream, const void *d_rays, uint32_t n, void *d_out)
{
    LS_ENTER(tr);
    return rays_locked(tr, hip_stream ? static_cast<hipStream_t>(hip_stream) : tr->stream, d_rays, n, d_out, kClosest);
}

int ls_trace_rays_host(ls_tracer *tr, const void *rays, uint32_t n, void *out)
{
    LS_ENTER(tr);
    return rays_host_locked(tr, rays, n, out, kClosest);
}

int ls_occluded_rays(ls_tracer *tr, void *hip_stream, const void *d_rays, uint32_t n, void *d_out)
{
    LS_ENTER(tr);
    return rays_locked(tr, hip_stream ? static_cast<hipStream_t>(hip_stream) : tr->stream, d_rays, n, d_out, kOccluded);
}

int ls_occluded_rays_host(ls_tracer *tr, const void *rays, uint32_t n, void *out)
{
    LS_ENTER(tr);
    return rays_host_locked(tr, rays, n, out, kOccluded);
}

int ls_closest_points(ls_tracer *tr, void *hip_stream, const void *d_points, uint32_t n, void *d_out)
{
    LS_ENTER(tr);
    return rays_locked(tr, hip_stream ? static_cast<hipStream_t>(hip_stream) : tr->stream, d_points, n, d_out, kNearest);
}

int ls_closest_points_host(ls_tracer *tr, const void *points, uint32_t n, void *out)
{
    LS_ENTER(tr);
    return rays_host_locked(tr, points, n, out, kNearest);
}

int ls_hit_attributes(ls_tracer *tr, void *hip_stream, const void *d_rays, uint32_t n_rays, const void *d_hits, const uint32_t *d_count, uint32_t n,
                      void *d_out)
{
    LS_ENTER(tr);
    return attr_locked(tr, hip_stream ? static_cast<hipStream_t>(hip_stream) : tr->stream, d_rays, n_rays, d_hits, d_count, n, d_out);
}

int ls_hit_attributes_host(ls_tracer *tr, const void *rays, uint32_t n_rays, const void *hits, uint32_t n, void *out)
{
    LS_ENTER(tr);
    return attr_host_locked(tr, rays, n_rays, hits, n, out);
}

// the model and the reflectivity arguments are checked before anything touches the device (the handle's included)
#define LS_RETURN_MODEL_CHECK(tr, model, refl, n_refl)                                                                   \
    if (!(tr)) return LS_ERR_INVALID_ARGUMENT;                                                                           \
    if (const char *why_ = (n_refl) && !(refl) ? "null reflectivities" : ls::return_model_invalid(model)) {              \
        std::lock_guard<std::mutex> lock_((tr)->mu);                                                                     \
        return lsi::fail((tr), LS_ERR_INVALID_ARGUMENT, why_);                                                           \
    }

int ls_apply_return_model(ls_tracer *tr, void *hip_stream, const ls_return_model *model, uint32_t frame_index, const void *d_rays, uint32_t n_rays,
                          const void *d_hits, const uint32_t *d_count, uint32_t n, const float *d_reflectivity, uint32_t n_reflectivity,
                          void *d_points32, void *d_hits_out, uint32_t *d_n_out)
{
    LS_RETURN_MODEL_CHECK(tr, model, d_reflectivity, n_reflectivity)
    LS_ENTER(tr);
    return returns_locked(tr, hip_stream ? static_cast<hipStream_t>(hip_stream) : tr->stream, model, frame_index, d_rays, n_rays, d_hits, d_count, n,
                          d_reflectivity, n_reflectivity, d_points32, d_hits_out, d_n_out);
}

int ls_apply_return_model_host(ls_tracer *tr, const ls_return_model *model, uint32_t frame_index, const void *rays, uint32_t n_rays,
                               const void *hits, uint32_t n, const float *reflectivity, uint32_t n_reflectivity, void *points32, void *hits_out,
                               uint32_t *n_out)
{
    LS_RETURN_MODEL_CHECK(tr, model, reflectivity, n_reflectivity)
    LS_ENTER(tr);
    return returns_host_locked(tr, model, frame_index, rays, n_rays, hits, n, reflectivity, n_reflectivity, points32, hits_out, n_out);
}

int ls_trace_scene_sweep(ls_tracer *tr, void *hip_stream, const float *d_col_pose, uint32_t n_cols, uint32_t flags, void *d_points32, void *d_hits,
                         uint32_t *d_n_points, uint32_t capacity, void *d_rays_out)
{
    LS_ENTER(tr);
    return sweep_locked(tr, hip_stream ? static_cast<hipStream_t>(hip_stream) : tr->stream, d_col_pose, n_cols, flags, d_points32, d_hits, d_n_points,
                        capacity, d_rays_out);
}

int ls_trace_scene_sweep_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols, uint32_t flags, void *points32, void *hits, uint32_t *n_points,
                              uint32_t capacity, void *rays_out)
{
    LS_ENTER(tr);
    return sweep_host_locked(tr, col_pose, n_cols, flags, points32, hits, n_points, capacity, rays_out);
}

// the refusals come before anything touches the device (the handle's included): LS_ENTER with beams_check in front of hipSetDevice
#define LS_ENTER_BEAMS(tr, model, n_points, capacity, misaligned)                                                        \
    if (!(tr)) return LS_ERR_INVALID_ARGUMENT;                                                                           \
    std::lock_guard<std::mutex> lock_((tr)->mu);                                                                         \
    if (const int refused_ = beams_check((tr), (model), (n_points), (capacity))) return refused_;                        \
    if (misaligned)                                                                                                      \
        return lsi::fail((tr), LS_ERR_INVALID_ARGUMENT,                                                                  \
                         "points and hit records must be 16-byte aligned, the echo words and the count 4-byte aligned"); \
    lsi::SinkScope sink_scope_(tr);                                                                                      \
    if (hipSetDevice((tr)->device) != hipSuccess) return lsi::fail((tr), LS_ERR_HIP, "hipSetDevice failed")

int ls_trace_scene_beams(ls_tracer *tr, void *hip_stream, const ls_beam_model *model, void *d_points32, void *d_hits, uint32_t *d_echo,
                         uint32_t *d_n_points, uint32_t capacity)
{
    LS_ENTER_BEAMS(tr, model, d_n_points, capacity,
                   ((uintptr_t)d_points32 & 15u) || ((uintptr_t)d_hits & 15u) || ((uintptr_t)d_echo & 3u) || ((uintptr_t)d_n_points & 3u));
    return beams_locked(tr, hip_stream ? static_cast<hipStream_t>(hip_stream) : tr->stream, model, d_points32, d_hits, d_echo, d_n_points, capacity);
}

int ls_trace_scene_beams_host(ls_tracer *tr, const ls_beam_model *model, void *points32, void *hits, uint32_t *echo, uint32_t *n_points,
                              uint32_t capacity)
{
    LS_ENTER_BEAMS(tr, model, n_points, capacity, false);   // (host memory: any alignment)
    return beams_host_locked(tr, model, points32, hits, echo, n_points);
}

// host only: the centre sample, then ring after ring; double throughout, one rounding per entry (k from the rounded a and b)
int ls_beam_pattern_rings(float half_angle_az, float half_angle_el, uint32_t n_rings, uint32_t per_ring, float *pattern)
{
    if (!pattern || !std::isfinite(half_angle_az) || !std::isfinite(half_angle_el)) return LS_ERR_INVALID_ARGUMENT;
    if ((unsigned long long)n_rings * per_ring + 1ull > ls::kBeamMaxSamples) return LS_ERR_INVALID_ARGUMENT;
    pattern[0] = 0.0f;
    pattern[1] = 0.0f;
    pattern[2] = 1.0f;
    float *p = pattern + 3;
    for (uint32_t j = 1; j <= n_rings; ++j)
        for (uint32_t i = 0; i < per_ring; ++i, p += 3) {
            const double rho = (double)j / (double)n_rings, phi = 2.0 * M_PI * ((double)i + 0.5 * (double)(j - 1)) / (double)per_ring;
            p[0] = (float)((double)half_angle_az * rho * std::cos(phi));
            p[1] = (float)((double)half_angle_el * rho * std::sin(phi));
            const double a = p[0], b = p[1];
            p[2] = (float)std::sqrt(1.0 + (a * a + b * b));
        }
    return LS_OK;
}

// host only: tau_h = t0 + h dt; R_h = Rodrigues' rotation by ang_vel * tau_h, o_h = lin_vel * tau_h; double throughout, one rounding
int ls_sweep_poses_constant_twist(const float lin_vel[3], const float ang_vel[3], double t0, double dt, uint32_t n_cols, float *col_pose)
{
    if (!lin_vel || !ang_vel || (n_cols && !col_pose)) return LS_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(t0) || !std::isfinite(dt)) return LS_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(lin_vel[k]) || !std::isfinite(ang_vel[k])) return LS_ERR_INVALID_ARGUMENT;
    const double w[3] = {ang_vel[0], ang_vel[1], ang_vel[2]};
    const double wn = std::sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    for (uint32_t h = 0; h < n_cols; ++h) {
        const double tau = t0 + (double)h * dt, angle = wn * tau;
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        if (angle != 0.0) {
            const double k[3] = {w[0] / wn, w[1] / wn, w[2] / wn}, sn = std::sin(angle), c1 = 1.0 - std::cos(angle);
            // R = I + sin(a) K + (1 - cos(a)) K^2, K the cross-product matrix of the unit axis k
            const double K[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    const double K2 = k[i] * k[j] - (i == j ? 1.0 : 0.0);   // (k k^T - I: |k| = 1)
                    R[3 * i + j] = (i == j ? 1.0 : 0.0) + sn * K[3 * i + j] + c1 * K2;
                }
        }
        float *p = col_pose + 12 * (size_t)h;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) p[4 * i + j] = (float)R[3 * i + j];
            p[4 * i + 3] = (float)((double)lin_vel[i] * tau);
        }
    }
    return LS_OK;
}

}  // extern "C"
