// ls_query.cpp -- the queries on the hierarchies and their host-memory variants: ls_trace_rays (closest hits of caller-supplied rays
// against the committed scene), ls_occluded_rays (whether each ray hits anything: the same walk, stopping at a hit) and
// ls_closest_points (the nearest surface point to each caller point: a distance-ordered walk, ls_points.hip); and what every query
// entry point shares (ls_gather.cpp, ls_scan.cpp, ls_cloud.cpp): the stream hand-over and the walk (query_enter / query_walk /
// query_leave), the host-memory variants' staging and read-back (Staging / Staged), stream_of.
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
#include "ls_labels.h"

#include <algorithm>
#include <cmath>

namespace lsi {

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

namespace {

constexpr uint32_t kMaxRayLaunches = (uint32_t)ls::kMaxGeoms / (uint32_t)ls::kGeomsPerLaunch;

bool same_floats(const float *a, const float *b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }

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
    release(q.cloud_map); release(q.label_acc); release(q.label_rays); release(q.voxel_keys); release(q.scene_queue); release(q.dist_queue);
    release(q.surface_area); release(q.surface_prefix); release(q.cloud_words); release(q.cloud_sorted); release(q.cloud_range);
    if (q.d_maxabs) (void)hipFree(q.d_maxabs);
    if (q.d_counters) (void)hipFree(q.d_counters);
    if (q.ev_ready) (void)hipEventDestroy(q.ev_ready);
    if (q.ev_done) (void)hipEventDestroy(q.ev_done);
    q.d_maxabs = q.d_counters = nullptr;
    q.ev_ready = q.ev_done = nullptr;
}

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

namespace {

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

}  // namespace

const RayQueryKind &closest_hits() { return kClosest; }

// What every query on the hierarchies does around and in its walk (ls_trace_rays and its siblings; the frames of
// ls_scan.cpp, which put a pass of their own on either side of the walk; the gathers of ls_gather.cpp, which have no walk):
//   query_enter  after everything already issued on the handle -- its frames in flight, its mesh copies -- on stream s (the one
//                flush_pipeline of a call);
//   query_walk   the query set brought up to date, the counters, one launch per batch of kGeomsPerLaunch geometries (motion: one
//                table pointer per layout entry, nullptr for a geometry at rest -- the closest-hit walk of ls_moving.hip over
//                the shard's sweep records instead of the kind's own);
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

int query_walk(ls_tracer *tr, hipStream_t s, const void *d_rays, uint32_t n, void *d_out, const RayQueryKind &kind, const float *const *motion)
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
        if (motion) {   // the sweep's records against geometries in motion: the tables follow their geometries into the batch
            ls::MotionBatch mb;
            std::memset(static_cast<void *>(&mb), 0, sizeof(mb));
            for (size_t i = first; i < last; ++i) mb.table[i - first] = motion[i];
            mb.az0 = tr->az0;
            mb.naz = tr->naz;
            ls::launch_trace_rays_moving(s, tr->trace_blocks, d_rays, n, batch, mb, q.wide_nodes.p, q.records.p, q.leaf, d_out, q.d_counters + b,
                                         q.spill.p);
            continue;
        }
        kind.launch(s, tr->trace_blocks, d_rays, n, batch, pm, q.wide_nodes.p, q.records.p, q.leaf, d_out, q.d_counters + b, q.spill.p);
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// ls_object_labels' footprint: query_walk's preparation and batches around k_label_footprint (ls_labels.hip).  The counts go to the
// call's accumulators, nothing to a per-ray output, and no launch starts from what another one left.
int query_footprint(ls_tracer *tr, hipStream_t s, const void *d_rays, uint32_t n, bool own_rays, uint32_t n_labels, void *d_acc)
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
    for (uint32_t b = 0; b < launches; ++b) {
        ls::RayBatch batch;
        std::memset(static_cast<void *>(&batch), 0, sizeof(batch));
        const size_t first = (size_t)b * ls::kGeomsPerLaunch, last = std::min(order.size(), first + ls::kGeomsPerLaunch);
        batch.n = (uint32_t)(last - first);
        batch.first = 1u;
        for (size_t i = first; i < last; ++i) {
            ls::RayGeom &rg = batch.g[i - first];
            ray_geom(tr, i, *order[i], sensor_frame[i], rg);
            if (rg.geom_id >= n_labels) rg.n_leaves = 0;   // no record for it: counted nowhere, and no accumulator to add to
        }
        ls::launch_label_footprint(s, tr->trace_blocks, d_rays, n, own_rays, batch, q.wide_nodes.p, q.records.p, q.leaf,
                                   static_cast<ls::LabelAcc *>(d_acc), q.d_counters + b, q.spill.p);
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

hipStream_t stream_of(const ls_tracer *tr, void *hip_stream) { return hip_stream ? static_cast<hipStream_t>(hip_stream) : tr->stream; }

int Staging::commit(ls_tracer *tr, hipStream_t s, Staged &io)
{
    DevBuf<uint8_t> &buf = tr->rq.io;
    if (const int rc = ensure(tr, buf, total)) return rc;
    io.base = buf.p;
    io.pieces.swap(pieces);
    for (const StagePiece &p : io.pieces)
        if (p.copy_in && p.bytes) LS_HIP(hipMemcpyAsync(io.base + p.at, p.host, p.bytes, hipMemcpyHostToDevice, s));
    return LS_OK;
}

int Staged::fetch(ls_tracer *tr) const
{
    const hipStream_t s = tr->stream;
    for (const StagePiece &p : pieces)
        if (p.record && p.bytes) LS_HIP(hipMemcpyAsync(p.host, base + p.at, p.bytes, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    return LS_OK;
}

int Staged::fetch_counted(ls_tracer *tr, int count_piece, size_t limit, const char *overflow, uint32_t *n_out, const StridedRows *strided) const
{
    const hipStream_t s = tr->stream;
    uint32_t count = 0;
    LS_HIP(hipMemcpyAsync(&count, dev(count_piece), 4, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    if (count > limit) return fail(tr, LS_ERR_HIP, overflow);
    for (const StagePiece &p : pieces)
        if (p.record && p.bytes && count) LS_HIP(hipMemcpyAsync(p.host, base + p.at, (size_t)count * p.record, hipMemcpyDeviceToHost, s));
    if (strided && strided->dst)
        LS_HIP(hipMemcpy2DAsync(static_cast<uint8_t *>(strided->dst) + strided->first, strided->pitch, dev(strided->piece) + strided->first,
                                strided->pitch, strided->bytes, strided->rows, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    *n_out = count;
    return LS_OK;
}

namespace {

// what the device entry point of a kind and its host-memory variant (any alignment) refuse, in this order
int rays_check(ls_tracer *tr, const void *in, uint32_t n, const void *out, const RayQueryKind &kind, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (n && (!in || !out)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null rays or output");
    if (!host && (misaligned(in, 16) || misaligned(out, kind.out_align))) return fail(tr, LS_ERR_INVALID_ARGUMENT, kind.misaligned);
    if (n > kMaxQueryRecords) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many rays in one call");
    tr->rq.last_built = 0;
    return uncommitted(tr);   // (before n = 0: the same answer whatever n)
}

int rays_device(ls_tracer *tr, void *hip_stream, const void *d_in, uint32_t n, void *d_out, const RayQueryKind &kind)
{
    const hipStream_t s = stream_of(tr, hip_stream);
    int rc;
    if ((rc = rays_check(tr, d_in, n, d_out, kind, false)) || !n) return rc;
    return query_run(tr, s, [&] { return query_walk(tr, s, d_in, n, d_out, kind); });
}

// the host-memory variant: queries and results staged in q.io, on the handle's stream; returns when out is filled
int rays_host(ls_tracer *tr, const void *in, uint32_t n, void *out, const RayQueryKind &kind)
{
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = rays_check(tr, in, n, out, kind, true)) || !n) return rc;
    if ((rc = query_enter(tr, s))) return rc;
    Staging st;
    const int p_in = st.in(in, (size_t)n * kind.in_bytes), p_out = st.out(out, n, kind.out_bytes);
    Staged io;
    if ((rc = st.commit(tr, s, io)) || (rc = query_walk(tr, s, io.dev(p_in), n, io.dev(p_out), kind))) return rc;
    return io.fetch(tr);
}

}  // namespace

}  // namespace lsi

using namespace lsi;

extern "C" {

int ls_trace_rays(ls_tracer *tr, void *hip_stream, const void *d_rays, uint32_t n, void *d_out)
{
    LS_ENTER(tr);
    return rays_device(tr, hip_stream, d_rays, n, d_out, kClosest);
}

int ls_trace_rays_host(ls_tracer *tr, const void *rays, uint32_t n, void *out)
{
    LS_ENTER(tr);
    return rays_host(tr, rays, n, out, kClosest);
}

int ls_occluded_rays(ls_tracer *tr, void *hip_stream, const void *d_rays, uint32_t n, void *d_out)
{
    LS_ENTER(tr);
    return rays_device(tr, hip_stream, d_rays, n, d_out, kOccluded);
}

int ls_occluded_rays_host(ls_tracer *tr, const void *rays, uint32_t n, void *out)
{
    LS_ENTER(tr);
    return rays_host(tr, rays, n, out, kOccluded);
}

int ls_closest_points(ls_tracer *tr, void *hip_stream, const void *d_points, uint32_t n, void *d_out)
{
    LS_ENTER(tr);
    return rays_device(tr, hip_stream, d_points, n, d_out, kNearest);
}

int ls_closest_points_host(ls_tracer *tr, const void *points, uint32_t n, void *out)
{
    LS_ENTER(tr);
    return rays_host(tr, points, n, out, kNearest);
}

}  // extern "C"
