// ls_gather.cpp -- what needs no hierarchy, a gather over hit records: ls_hit_attributes (surface attributes of the records,
// ls_attr.hip) and ls_apply_return_model (sensor returns from them: the same gather, a model on top of it and an ordered compaction,
// ls_returns.hip), each with its host-memory variant; and the two again for the records of ls_trace_scene_sweep_moving, whose
// geometries each saw a ray of their own (ls_hit_attributes_moving, ls_apply_return_model_moving: ls_attr_moving.hip, with a
// motion-table pointer per geomID next to the gather's table).  Their place among what the handle issues is that of the queries on the
// hierarchies (query_enter / query_leave, ls_query.cpp); LS_INFO_RAY_QUERY_BUILT is left as it is.
#include "ls_internal.h"
#include "ls_return_model.h"

#include <algorithm>

namespace lsi {

namespace {

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


// ---- ls_hit_attributes --------------------------------------------------------------------------------------------------------

// what the device entry point and the host-memory variant (any alignment; the ray count is checked too) refuse, in this order
int attr_check(ls_tracer *tr, const void *rays, uint32_t n_rays, const void *hits, const uint32_t *count, uint32_t n, const void *out, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (n && (!hits || !out)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records or output");
    if (!host && (misaligned16(rays, hits, out) || misaligned(count, 4)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "rays, hit records and attribute records must be 16-byte aligned, the count 4-byte aligned");
    if (n > kMaxQueryRecords || (host && rays && n_rays > kMaxQueryRecords)) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records in one call");
    return uncommitted(tr);   // (before n = 0: the same answer whatever n)
}

int attr_issue(ls_tracer *tr, hipStream_t s, const void *d_rays, uint32_t n_rays, const void *d_hits, const uint32_t *d_count, uint32_t n, void *d_out)
{
    int rc;
    if ((rc = attr_table_prepare(tr, s))) return rc;
    ls::launch_hit_attributes(s, d_hits, d_count, n, d_rays, n_rays, tables(tr), tr->ha.table.p, (uint32_t)tr->ha.current.size(), d_out);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// ---- ls_apply_return_model ----------------------------------------------------------------------------------------------------

// what both entry points refuse, in this order: the model and the reflectivities first, before anything touches the device
int returns_check(ls_tracer *tr, const ls_return_model *model, const void *rays, uint32_t n_rays, const void *hits, const uint32_t *count, uint32_t n,
                  const float *refl, uint32_t n_refl, const void *points32, const void *hits_out, const uint32_t *n_out, bool host)
{
    if (const char *why = n_refl && !refl ? "null reflectivities" : ls::return_model_invalid(model)) return fail(tr, LS_ERR_INVALID_ARGUMENT, why);
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!n_out || (n && !hits)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records or count output");
    if (!host && (misaligned16(rays, hits, points32, hits_out) || misaligned(count, 4) || misaligned(n_out, 4) || misaligned(refl, 4)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "rays, hit records and points must be 16-byte aligned, counts and reflectivities 4-byte aligned");
    if (n > kMaxQueryRecords || (host && rays && n_rays > kMaxQueryRecords)) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records in one call");
    return uncommitted(tr);
}

int returns_issue(ls_tracer *tr, hipStream_t s, const ls_return_model *model, uint32_t frame_index, const void *d_rays, uint32_t n_rays,
                  const void *d_hits, const uint32_t *d_count, uint32_t n, const float *d_refl, uint32_t n_refl, void *d_points32, void *d_hits_out,
                  uint32_t *d_n_out)
{
    ls_tracer::HitAttr &a = tr->ha;
    int rc;
    if (!n) {
        LS_HIP(hipMemsetAsync(d_n_out, 0, 4, s));   // no record: no return
        return LS_OK;
    }
    if ((rc = attr_table_prepare(tr, s))) return rc;
    if ((rc = ensure(tr, a.park, 2 * (size_t)n))) return rc;
    if ((rc = ensure(tr, a.block_counts, ls::returns_block_count(n)))) return rc;
    ls::launch_returns(s, d_hits, d_count, n, d_rays, n_rays, tables(tr), a.table.p, (uint32_t)a.current.size(), *model, frame_index,
                       n_refl ? d_refl : nullptr, n_refl, a.park.p, a.block_counts.p, d_points32, d_hits_out, d_n_out);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// ---- ls_hit_attributes_moving / ls_apply_return_model_moving ------------------------------------------------------------------

// what the four entry points refuse after their own NULL checks, in this order: ls_trace_scene_sweep_moving's pose table, flags and
// motions; misaligned device pointers (p16: records and points, p4: words and reflectivities; the tables 4 bytes); too many records;
// the commit state; a motion for a geometry that is not in the committed scene.  On LS_OK by_id[g] is the motion table of geomID g
// (nullptr: at rest), as long as the table attr_table_prepare makes
int moving_args_check(ls_tracer *tr, const float *col_pose, uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags,
                      uint32_t n, std::initializer_list<const void *> p16, std::initializer_list<const void *> p4, bool host,
                      std::vector<const float *> &by_id)
{
    if (const int rc = motion_args_check(tr, col_pose, n_cols, motions, n_motions, flags)) return rc;
    if (!host) {
        bool bad = misaligned(col_pose, 4);
        for (const void *p : p16) bad = bad || misaligned(p, 16);
        for (const void *p : p4) bad = bad || misaligned(p, 4);
        for (uint32_t k = 0; k < n_motions; ++k) bad = bad || misaligned(motions[k].col_motion, 4);
        if (bad)
            return fail(tr, LS_ERR_INVALID_ARGUMENT,
                        "hit records, attribute records and points must be 16-byte aligned, the counts, the poses, the motion tables and the "
                        "reflectivities 4-byte aligned");
    }
    if (n > kMaxQueryRecords) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records in one call");
    if (const int rc = uncommitted(tr)) return rc;   // (before n = 0: the same answer whatever n)
    int max_id = -1;
    for (const int id : tr->slot_geom_ids) max_id = std::max(max_id, id);
    by_id.assign((size_t)(max_id + 1), nullptr);
    for (uint32_t k = 0; k < n_motions; ++k) {
        if (std::find(tr->slot_geom_ids.begin(), tr->slot_geom_ids.end(), (int)motions[k].geom) == tr->slot_geom_ids.end() ||
            motions[k].geom >= by_id.size())
            return fail(tr, LS_ERR_UNKNOWN_GEOMETRY, "a motion names a geometry that is not in the committed scene");
        by_id[motions[k].geom] = motions[k].col_motion;
    }
    return LS_OK;
}

int attr_moving_check(ls_tracer *tr, const float *col_pose, uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags,
                      const void *hits, const uint32_t *count, uint32_t n, const void *out, bool host, std::vector<const float *> &by_id)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (n && (!hits || !out)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records or output");
    return moving_args_check(tr, col_pose, n_cols, motions, n_motions, flags, n, {hits, out}, {count}, host, by_id);
}

// the model and the reflectivities first, as ls_apply_return_model
int returns_moving_check(ls_tracer *tr, const ls_return_model *model, const float *col_pose, uint32_t n_cols, const ls_geometry_motion *motions,
                         uint32_t n_motions, uint32_t flags, const void *hits, const uint32_t *count, uint32_t n, const float *refl, uint32_t n_refl,
                         const void *points32, const void *hits_out, const uint32_t *n_out, bool host, std::vector<const float *> &by_id)
{
    if (const char *why = n_refl && !refl ? "null reflectivities" : ls::return_model_invalid(model)) return fail(tr, LS_ERR_INVALID_ARGUMENT, why);
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!n_out || (n && !hits)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records or count output");
    return moving_args_check(tr, col_pose, n_cols, motions, n_motions, flags, n, {hits, points32, hits_out}, {count, n_out, refl}, host, by_id);
}

// the pointer array k_hit_attributes_moving reads next to the AttrGeom table, one entry per geomID (by_id, cut or padded to that
// table's length: the kernels check a geomID against one bound); uploaded on s when it differs from what the device holds
int motion_table_prepare(ls_tracer *tr, hipStream_t s, std::vector<const float *> &by_id)
{
    ls_tracer::HitAttr &a = tr->ha;
    by_id.resize(a.current.size(), nullptr);
    if (by_id == a.motion_current && a.motion.p) return LS_OK;
    a.motion_current.clear();   // (whatever fails from here on, the next call refreshes)
    const size_t bytes = by_id.size() * sizeof(const float *);
    int rc;
    if ((rc = ensure(tr, a.motion, by_id.size()))) return rc;
    if (!a.ev_motion_stage) LS_HIP(hipEventCreateWithFlags(&a.ev_motion_stage, hipEventDisableTiming));
    LS_HIP(hipEventSynchronize(a.ev_motion_stage));   // (the copy of an earlier refresh may still be reading the staging buffer)
    if (a.motion_stage_cap < by_id.size()) {
        if (a.h_motion_stage) LS_HIP(hipHostFree(a.h_motion_stage));
        a.h_motion_stage = nullptr;
        a.motion_stage_cap = 0;
        LS_HIP(hipHostMalloc(reinterpret_cast<void **>(&a.h_motion_stage), bytes + bytes / 8, hipHostMallocDefault));
        a.motion_stage_cap = (bytes + bytes / 8) / sizeof(const float *);
    }
    std::memcpy(static_cast<void *>(a.h_motion_stage), by_id.data(), bytes);
    LS_HIP(hipMemcpyAsync(a.motion.p, a.h_motion_stage, bytes, hipMemcpyHostToDevice, s));
    LS_HIP(hipEventRecord(a.ev_motion_stage, s));
    a.motion_current = by_id;
    return LS_OK;
}

int attr_moving_issue(ls_tracer *tr, hipStream_t s, const float *d_col_pose, std::vector<const float *> &by_id, uint32_t flags, const void *d_hits,
                      const uint32_t *d_count, uint32_t n, void *d_out)
{
    int rc;
    if ((rc = attr_table_prepare(tr, s)) || (rc = motion_table_prepare(tr, s, by_id))) return rc;
    ls::launch_hit_attributes_moving(s, d_hits, d_count, n, tables(tr), tr->ha.table.p, tr->ha.motion.p, (uint32_t)tr->ha.current.size(), d_col_pose,
                                     (flags & LS_SWEEP_DESKEW) != 0, d_out);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

int returns_moving_issue(ls_tracer *tr, hipStream_t s, const ls_return_model *model, uint32_t frame_index, const float *d_col_pose,
                         std::vector<const float *> &by_id, uint32_t flags, const void *d_hits, const uint32_t *d_count, uint32_t n,
                         const float *d_refl, uint32_t n_refl, void *d_points32, void *d_hits_out, uint32_t *d_n_out)
{
    ls_tracer::HitAttr &a = tr->ha;
    int rc;
    if (!n) {
        LS_HIP(hipMemsetAsync(d_n_out, 0, 4, s));   // no record: no return
        return LS_OK;
    }
    if ((rc = attr_table_prepare(tr, s)) || (rc = motion_table_prepare(tr, s, by_id))) return rc;
    if ((rc = ensure(tr, a.park, 2 * (size_t)n))) return rc;
    if ((rc = ensure(tr, a.block_counts, ls::returns_block_count(n)))) return rc;
    const ls::SensorTables tb = tables(tr);
    ls::launch_returns_eval_moving(s, d_hits, d_count, n, tb, a.table.p, a.motion.p, (uint32_t)a.current.size(), d_col_pose,
                                   (flags & LS_SWEEP_DESKEW) != 0, *model, frame_index, n_refl ? d_refl : nullptr, n_refl, a.park.p, a.block_counts.p);
    ls::launch_returns_pack(s, a.park.p, a.block_counts.p, d_count, n, tb.H, d_points32, d_hits_out, d_n_out);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// the host-memory variants' tables in q.io: the pose table at at_pose, the named geometries' tables behind at_motion (48 H bytes
// each: every table starts 16-byte aligned); by_id then names the device copies
int stage_tables(ls_tracer *tr, hipStream_t s, uint8_t *base, size_t at_pose, size_t at_motion, const float *col_pose, uint32_t n_cols,
                 std::vector<const float *> &by_id)
{
    const size_t table_bytes = (size_t)tr->H * 48;
    if (col_pose) LS_HIP(hipMemcpyAsync(base + at_pose, col_pose, (size_t)n_cols * 48, hipMemcpyHostToDevice, s));
    size_t staged = 0;
    for (const float *&t : by_id) {
        if (!t) continue;
        uint8_t *dst = base + at_motion + staged++ * table_bytes;
        LS_HIP(hipMemcpyAsync(dst, t, table_bytes, hipMemcpyHostToDevice, s));
        t = reinterpret_cast<const float *>(dst);
    }
    return LS_OK;
}

}  // namespace

void hit_attr_release(ls_tracer *tr)
{
    ls_tracer::HitAttr &a = tr->ha;
    if (a.ev_stage) { (void)hipEventSynchronize(a.ev_stage); (void)hipEventDestroy(a.ev_stage); }
    if (a.h_stage) (void)hipHostFree(a.h_stage);
    if (a.ev_motion_stage) { (void)hipEventSynchronize(a.ev_motion_stage); (void)hipEventDestroy(a.ev_motion_stage); }
    if (a.h_motion_stage) (void)hipHostFree(a.h_motion_stage);
    release(a.table); release(a.park); release(a.block_counts); release(a.motion);
    a.ev_stage = nullptr;
    a.h_stage = nullptr;
    a.stage_cap = 0;
    a.current.clear();
    a.ev_motion_stage = nullptr;
    a.h_motion_stage = nullptr;
    a.motion_stage_cap = 0;
    a.motion_current.clear();
}

}  // namespace lsi

using namespace lsi;

extern "C" {

int ls_hit_attributes(ls_tracer *tr, void *hip_stream, const void *d_rays, uint32_t n_rays, const void *d_hits, const uint32_t *d_count, uint32_t n,
                      void *d_out)
{
    LS_ENTER(tr);
    const hipStream_t s = stream_of(tr, hip_stream);
    int rc;
    if ((rc = attr_check(tr, d_rays, n_rays, d_hits, d_count, n, d_out, false)) || !n) return rc;
    if ((rc = query_enter(tr, s)) || (rc = attr_issue(tr, s, d_rays, n_rays, d_hits, d_count, n, d_out))) return rc;
    return query_leave(tr, s);
}

// hit records, rays and results staged in q.io, on the handle's stream; returns when out is filled
int ls_hit_attributes_host(ls_tracer *tr, const void *rays, uint32_t n_rays, const void *hits, uint32_t n, void *out)
{
    LS_ENTER(tr);
    DevBuf<uint8_t> &buf = tr->rq.io;
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = attr_check(tr, rays, n_rays, hits, nullptr, n, out, true)) || !n) return rc;
    if ((rc = query_enter(tr, s))) return rc;
    IoPlan io;
    const size_t ray_bytes = rays ? (size_t)n_rays * 32 : 0;
    const size_t at_hits = io.add((size_t)n * 16), at_rays = io.add(ray_bytes), at_out = io.add((size_t)n * 48);
    if ((rc = ensure(tr, buf, io.total()))) return rc;
    LS_HIP(hipMemcpyAsync(buf.p + at_hits, hits, (size_t)n * 16, hipMemcpyHostToDevice, s));
    if (ray_bytes) LS_HIP(hipMemcpyAsync(buf.p + at_rays, rays, ray_bytes, hipMemcpyHostToDevice, s));
    if ((rc = attr_issue(tr, s, rays ? buf.p + at_rays : nullptr, n_rays, buf.p + at_hits, nullptr, n, buf.p + at_out))) return rc;
    LS_HIP(hipMemcpyAsync(out, buf.p + at_out, (size_t)n * 48, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    return LS_OK;
}

int ls_apply_return_model(ls_tracer *tr, void *hip_stream, const ls_return_model *model, uint32_t frame_index, const void *d_rays, uint32_t n_rays,
                          const void *d_hits, const uint32_t *d_count, uint32_t n, const float *d_reflectivity, uint32_t n_reflectivity,
                          void *d_points32, void *d_hits_out, uint32_t *d_n_out)
{
    LS_ENTER_CHECKED(tr, returns_check(tr, model, d_rays, n_rays, d_hits, d_count, n, d_reflectivity, n_reflectivity, d_points32, d_hits_out, d_n_out,
                                       false));
    const hipStream_t s = stream_of(tr, hip_stream);
    int rc;
    if ((rc = query_enter(tr, s)) || (rc = returns_issue(tr, s, model, frame_index, d_rays, n_rays, d_hits, d_count, n, d_reflectivity, n_reflectivity,
                                                         d_points32, d_hits_out, d_n_out)))
        return rc;
    return query_leave(tr, s);
}

// inputs and results staged in q.io, on the handle's stream; the count comes back first, then as many records
int ls_apply_return_model_host(ls_tracer *tr, const ls_return_model *model, uint32_t frame_index, const void *rays, uint32_t n_rays,
                               const void *hits, uint32_t n, const float *reflectivity, uint32_t n_reflectivity, void *points32, void *hits_out,
                               uint32_t *n_out)
{
    LS_ENTER_CHECKED(tr, returns_check(tr, model, rays, n_rays, hits, nullptr, n, reflectivity, n_reflectivity, points32, hits_out, n_out, true));
    if (!n) {
        *n_out = 0;
        return LS_OK;
    }
    DevBuf<uint8_t> &buf = tr->rq.io;
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    IoPlan io;
    const size_t ray_bytes = rays ? (size_t)n_rays * 32 : 0;
    const size_t at_hits = io.add((size_t)n * 16), at_rays = io.add(ray_bytes), at_points = io.add(points32 ? (size_t)n * 32 : 0),
                 at_out = io.add(hits_out ? (size_t)n * 16 : 0), at_refl = io.add((size_t)n_reflectivity * 4), at_n = io.add(4);
    if ((rc = ensure(tr, buf, io.total()))) return rc;
    LS_HIP(hipMemcpyAsync(buf.p + at_hits, hits, (size_t)n * 16, hipMemcpyHostToDevice, s));
    if (ray_bytes) LS_HIP(hipMemcpyAsync(buf.p + at_rays, rays, ray_bytes, hipMemcpyHostToDevice, s));
    if (n_reflectivity) LS_HIP(hipMemcpyAsync(buf.p + at_refl, reflectivity, (size_t)n_reflectivity * 4, hipMemcpyHostToDevice, s));
    if ((rc = returns_issue(tr, s, model, frame_index, rays ? buf.p + at_rays : nullptr, n_rays, buf.p + at_hits, nullptr, n,
                            reinterpret_cast<const float *>(buf.p + at_refl), n_reflectivity, points32 ? buf.p + at_points : nullptr,
                            hits_out ? buf.p + at_out : nullptr, reinterpret_cast<uint32_t *>(buf.p + at_n))))
        return rc;
    return fetch_counted(tr, buf.p + at_n, n, "ls_apply_return_model: more returns than records",
                         {{points32, buf.p + at_points, 32}, {hits_out, buf.p + at_out, 16}}, n_out);
}

int ls_hit_attributes_moving(ls_tracer *tr, void *hip_stream, const float *d_col_pose, uint32_t n_cols, const ls_geometry_motion *motions,
                             uint32_t n_motions, uint32_t flags, const void *d_hits, const uint32_t *d_count, uint32_t n, void *d_out)
{
    std::vector<const float *> by_id;
    LS_ENTER_CHECKED(tr, attr_moving_check(tr, d_col_pose, n_cols, motions, n_motions, flags, d_hits, d_count, n, d_out, false, by_id));
    if (!n) return LS_OK;
    const hipStream_t s = stream_of(tr, hip_stream);
    int rc;
    if ((rc = query_enter(tr, s)) || (rc = attr_moving_issue(tr, s, d_col_pose, by_id, flags, d_hits, d_count, n, d_out))) return rc;
    return query_leave(tr, s);
}

// hit records, the tables and the results staged in q.io, on the handle's stream; returns when out is filled
int ls_hit_attributes_moving_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions,
                                  uint32_t flags, const void *hits, uint32_t n, void *out)
{
    std::vector<const float *> by_id;
    LS_ENTER_CHECKED(tr, attr_moving_check(tr, col_pose, n_cols, motions, n_motions, flags, hits, nullptr, n, out, true, by_id));
    if (!n) return LS_OK;
    DevBuf<uint8_t> &buf = tr->rq.io;
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    IoPlan io;
    const size_t at_hits = io.add((size_t)n * 16), at_out = io.add((size_t)n * 48), at_pose = io.add((size_t)n_cols * 48),
                 at_motion = io.add((size_t)n_motions * tr->H * 48);
    if ((rc = ensure(tr, buf, io.total()))) return rc;
    LS_HIP(hipMemcpyAsync(buf.p + at_hits, hits, (size_t)n * 16, hipMemcpyHostToDevice, s));
    if ((rc = stage_tables(tr, s, buf.p, at_pose, at_motion, col_pose, n_cols, by_id))) return rc;
    if ((rc = attr_moving_issue(tr, s, col_pose ? reinterpret_cast<const float *>(buf.p + at_pose) : nullptr, by_id, flags, buf.p + at_hits, nullptr, n,
                                buf.p + at_out)))
        return rc;
    LS_HIP(hipMemcpyAsync(out, buf.p + at_out, (size_t)n * 48, hipMemcpyDeviceToHost, s));
    LS_HIP(hipStreamSynchronize(s));
    return LS_OK;
}

int ls_apply_return_model_moving(ls_tracer *tr, void *hip_stream, const ls_return_model *model, uint32_t frame_index, const float *d_col_pose,
                                 uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags, const void *d_hits,
                                 const uint32_t *d_count, uint32_t n, const float *d_reflectivity, uint32_t n_reflectivity, void *d_points32,
                                 void *d_hits_out, uint32_t *d_n_out)
{
    std::vector<const float *> by_id;
    LS_ENTER_CHECKED(tr, returns_moving_check(tr, model, d_col_pose, n_cols, motions, n_motions, flags, d_hits, d_count, n, d_reflectivity,
                                              n_reflectivity, d_points32, d_hits_out, d_n_out, false, by_id));
    const hipStream_t s = stream_of(tr, hip_stream);
    int rc;
    if ((rc = query_enter(tr, s)) || (rc = returns_moving_issue(tr, s, model, frame_index, d_col_pose, by_id, flags, d_hits, d_count, n, d_reflectivity,
                                                                n_reflectivity, d_points32, d_hits_out, d_n_out)))
        return rc;
    return query_leave(tr, s);
}

// inputs, tables and results staged in q.io, on the handle's stream; the count comes back first, then as many records
int ls_apply_return_model_moving_host(ls_tracer *tr, const ls_return_model *model, uint32_t frame_index, const float *col_pose, uint32_t n_cols,
                                      const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags, const void *hits, uint32_t n,
                                      const float *reflectivity, uint32_t n_reflectivity, void *points32, void *hits_out, uint32_t *n_out)
{
    std::vector<const float *> by_id;
    LS_ENTER_CHECKED(tr, returns_moving_check(tr, model, col_pose, n_cols, motions, n_motions, flags, hits, nullptr, n, reflectivity, n_reflectivity,
                                              points32, hits_out, n_out, true, by_id));
    if (!n) {
        *n_out = 0;
        return LS_OK;
    }
    DevBuf<uint8_t> &buf = tr->rq.io;
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    IoPlan io;
    const size_t at_hits = io.add((size_t)n * 16), at_points = io.add(points32 ? (size_t)n * 32 : 0), at_out = io.add(hits_out ? (size_t)n * 16 : 0),
                 at_refl = io.add((size_t)n_reflectivity * 4), at_pose = io.add((size_t)n_cols * 48),
                 at_motion = io.add((size_t)n_motions * tr->H * 48), at_n = io.add(4);
    if ((rc = ensure(tr, buf, io.total()))) return rc;
    LS_HIP(hipMemcpyAsync(buf.p + at_hits, hits, (size_t)n * 16, hipMemcpyHostToDevice, s));
    if (n_reflectivity) LS_HIP(hipMemcpyAsync(buf.p + at_refl, reflectivity, (size_t)n_reflectivity * 4, hipMemcpyHostToDevice, s));
    if ((rc = stage_tables(tr, s, buf.p, at_pose, at_motion, col_pose, n_cols, by_id))) return rc;
    if ((rc = returns_moving_issue(tr, s, model, frame_index, col_pose ? reinterpret_cast<const float *>(buf.p + at_pose) : nullptr, by_id, flags,
                                   buf.p + at_hits, nullptr, n, reinterpret_cast<const float *>(buf.p + at_refl), n_reflectivity,
                                   points32 ? buf.p + at_points : nullptr, hits_out ? buf.p + at_out : nullptr,
                                   reinterpret_cast<uint32_t *>(buf.p + at_n))))
        return rc;
    return fetch_counted(tr, buf.p + at_n, n, "ls_apply_return_model_moving: more returns than records",
                         {{points32, buf.p + at_points, 32}, {hits_out, buf.p + at_out, 16}}, n_out);
}

}  // extern "C"
