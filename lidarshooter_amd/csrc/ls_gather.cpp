// ls_gather.cpp -- what needs no hierarchy, a gather over hit records: ls_hit_attributes (surface attributes of the records,
// ls_attr.hip) and ls_apply_return_model (sensor returns from them: the same gather, a model on top of it and an ordered compaction,
// ls_returns.hip), each with its host-memory variant; and the two again for the records of ls_trace_scene_sweep_moving, whose
// geometries each saw a ray of their own (ls_hit_attributes_moving, ls_apply_return_model_moving: ls_attr_moving.hip, with a
// motion-table pointer per geomID next to the gather's table); and ls_hit_velocities, the velocities at those records
// (ls_velocity.hip, with a twist-table pointer per geomID as a third array).  Their place among what the handle issues is that of the queries on the
// hierarchies (query_enter / query_leave, ls_query.cpp); LS_INFO_RAY_QUERY_BUILT is left as it is.
//
// A static call and its _moving pair share their check, their issue function and their host-memory variant: `mv` is nullptr for the
// static call (which has caller rays instead, or the sensor's own), the tables of the frame for the moving one.
#include "ls_internal.h"
#include "ls_return_model.h"

#include <algorithm>

namespace lsi {

// the table k_hit_attributes reads, one entry per geomID up to the highest committed one (free ids stay zero), from the committed
// layout and the geometries' current buffers and poses (committed_geometry's checks), and for a moving call the motion-table pointer
// per geomID next to it, as long as it is; each uploaded on s when it differs from what the device holds
int tables_prepare(ls_tracer *tr, hipStream_t s, const Moving *mv)
{
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
    if (const int rc = tr->ha.table.upload_if_changed(tr, s, tab)) return rc;
    if (!mv) return LS_OK;
    std::vector<const float *> by_id = mv->per_geom(tr->ha.table.current.size());
    return tr->ha.motion.upload_if_changed(tr, s, by_id);
}

// that table and, next to it, HitAttr::tri_first: where each geomID's triangles start in the flat triangle index (a free id: none),
// the total behind them (ls_scene_tris.h).  More than max_tris triangles: LS_ERR_OUT_OF_RANGE with the caller's message
int scene_tris_prepare(ls_tracer *tr, hipStream_t s, unsigned long long max_tris, const char *too_many, uint32_t *n_table, uint32_t *n_tris)
{
    ls_tracer::HitAttr &a = tr->ha;
    if (const int rc = tables_prepare(tr, s, nullptr)) return rc;
    *n_table = (uint32_t)a.table.current.size();
    std::vector<uint32_t> first((size_t)*n_table + 1);
    unsigned long long total = 0;
    for (uint32_t k = 0; k < *n_table; ++k) {
        const ls::AttrGeom &e = a.table.current[k];
        first[k] = (uint32_t)total;
        if (e.verts) total += e.quad ? 2ull * e.n_elems : e.n_elems;
    }
    if (total > max_tris) return fail(tr, LS_ERR_OUT_OF_RANGE, too_many);
    *n_tris = first[*n_table] = (uint32_t)total;
    return a.tri_first.upload_if_changed(tr, s, first);
}

namespace {

// what the moving calls refuse after their own NULL checks, in this order: ls_trace_scene_sweep_moving's pose table, flags and
// motions; misaligned device pointers (p16: records and points, p4: words and reflectivities; the tables 4 bytes); too many records;
// the commit state; a motion for a geometry that is not in the committed scene
int moving_check(ls_tracer *tr, Moving &mv, uint32_t n, std::initializer_list<const void *> p16, std::initializer_list<const void *> p4, bool host)
{
    if (const int rc = moving_args_check(tr, mv)) return rc;
    if (!host && moving_misaligned(p16, p4, mv))
        return fail(tr, LS_ERR_INVALID_ARGUMENT,
                    "hit records, attribute records and points must be 16-byte aligned, the counts, the poses, the motion tables and the "
                    "reflectivities 4-byte aligned");
    if (n > kMaxQueryRecords) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records in one call");
    if (const int rc = uncommitted(tr)) return rc;   // (before n = 0: the same answer whatever n)
    return moving_resolve(tr, mv);
}

// the caller's rays in a host-memory variant: NULL stands for the sensor's own rays, so rays given with n_rays = 0 keep an address
// (the hit records': it is never read)
const void *staged_rays(const Staged &io, int p_rays, int p_hits, const void *rays) { return io.dev(rays && !io.dev(p_rays) ? p_hits : p_rays); }

// ---- ls_hit_attributes, ls_hit_attributes_moving ------------------------------------------------------------------------------

// what the device entry points and the host-memory variants (any alignment; the ray count is checked too) refuse, in this order
int attr_check(ls_tracer *tr, const void *rays, uint32_t n_rays, Moving *mv, const void *hits, const uint32_t *count, uint32_t n, const void *out,
               bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (n && (!hits || !out)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records or output");
    if (mv) return moving_check(tr, *mv, n, {hits, out}, {count}, host);
    if (!host && (misaligned16(rays, hits, out) || misaligned(count, 4)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "rays, hit records and attribute records must be 16-byte aligned, the count 4-byte aligned");
    if (n > kMaxQueryRecords || (host && rays && n_rays > kMaxQueryRecords)) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records in one call");
    return uncommitted(tr);   // (before n = 0: the same answer whatever n)
}

int attr_issue(ls_tracer *tr, hipStream_t s, const void *d_rays, uint32_t n_rays, const Moving *mv, const void *d_hits, const uint32_t *d_count,
               uint32_t n, void *d_out)
{
    const ls_tracer::HitAttr &a = tr->ha;
    if (const int rc = tables_prepare(tr, s, mv)) return rc;
    const uint32_t n_geoms = (uint32_t)a.table.current.size();
    if (mv)
        ls::launch_hit_attributes_moving(s, d_hits, d_count, n, tables(tr), a.table.dev.p, a.motion.dev.p, n_geoms, mv->col_pose,
                                         (mv->flags & LS_SWEEP_DESKEW) != 0, d_out);
    else
        ls::launch_hit_attributes(s, d_hits, d_count, n, d_rays, n_rays, tables(tr), a.table.dev.p, n_geoms, d_out);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// records, rays or tables, and results staged in q.io, on the handle's stream; returns when out is filled
int attr_host(ls_tracer *tr, const void *rays, uint32_t n_rays, Moving *mv, const void *hits, uint32_t n, void *out)
{
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    Staging st;
    const int p_hits = st.in(hits, (size_t)n * 16), p_rays = st.in(rays, (size_t)n_rays * 32), p_out = st.out(out, n, 48);
    if (mv) mv->stage(tr, st);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    if (mv) mv->use_staged(io);
    if ((rc = attr_issue(tr, s, staged_rays(io, p_rays, p_hits, rays), n_rays, mv, io.dev(p_hits), nullptr, n, io.dev(p_out)))) return rc;
    return io.fetch(tr);
}

// ---- ls_apply_return_model, ls_apply_return_model_moving ----------------------------------------------------------------------

// what the entry points refuse, in this order: the model and the reflectivities first, before anything touches the device
int returns_check(ls_tracer *tr, const ls_return_model *model, const void *rays, uint32_t n_rays, Moving *mv, const void *hits, const uint32_t *count,
                  uint32_t n, const float *refl, uint32_t n_refl, const void *points32, const void *hits_out, const uint32_t *n_out, bool host)
{
    if (const char *why = n_refl && !refl ? "null reflectivities" : ls::return_model_invalid(model)) return fail(tr, LS_ERR_INVALID_ARGUMENT, why);
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!n_out || (n && !hits)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records or count output");
    if (mv) return moving_check(tr, *mv, n, {hits, points32, hits_out}, {count, n_out, refl}, host);
    if (!host && (misaligned16(rays, hits, points32, hits_out) || misaligned(count, 4) || misaligned(n_out, 4) || misaligned(refl, 4)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "rays, hit records and points must be 16-byte aligned, counts and reflectivities 4-byte aligned");
    if (n > kMaxQueryRecords || (host && rays && n_rays > kMaxQueryRecords)) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records in one call");
    return uncommitted(tr);
}

// the static call keeps its fused launch, the moving one evaluates and packs
int returns_issue(ls_tracer *tr, hipStream_t s, const ls_return_model *model, uint32_t frame_index, const void *d_rays, uint32_t n_rays, const Moving *mv,
                  const void *d_hits, const uint32_t *d_count, uint32_t n, const float *d_refl, uint32_t n_refl, void *d_points32, void *d_hits_out,
                  uint32_t *d_n_out)
{
    ls_tracer::HitAttr &a = tr->ha;
    int rc;
    if (!n) {
        LS_HIP(hipMemsetAsync(d_n_out, 0, 4, s));   // no record: no return
        return LS_OK;
    }
    if ((rc = tables_prepare(tr, s, mv))) return rc;
    if ((rc = ensure(tr, a.park, 2 * (size_t)n))) return rc;
    if ((rc = ensure(tr, a.block_counts, ls::returns_block_count(n)))) return rc;
    const ls::SensorTables tb = tables(tr);
    const uint32_t n_geoms = (uint32_t)a.table.current.size();
    if (!n_refl) d_refl = nullptr;
    if (mv) {
        ls::launch_returns_eval_moving(s, d_hits, d_count, n, tb, a.table.dev.p, a.motion.dev.p, n_geoms, mv->col_pose,
                                       (mv->flags & LS_SWEEP_DESKEW) != 0, *model, frame_index, d_refl, n_refl, a.park.p, a.block_counts.p);
        ls::launch_returns_pack(s, a.park.p, a.block_counts.p, d_count, n, tb.H, d_points32, d_hits_out, d_n_out);
    } else {
        ls::launch_returns(s, d_hits, d_count, n, d_rays, n_rays, tb, a.table.dev.p, n_geoms, *model, frame_index, d_refl, n_refl, a.park.p,
                           a.block_counts.p, d_points32, d_hits_out, d_n_out);
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// inputs, rays or tables, and results staged in q.io, on the handle's stream; the count comes back first, then as many records
int returns_host(ls_tracer *tr, const char *overflow, const ls_return_model *model, uint32_t frame_index, const void *rays, uint32_t n_rays, Moving *mv,
                 const void *hits, uint32_t n, const float *refl, uint32_t n_refl, void *points32, void *hits_out, uint32_t *n_out)
{
    if (!n) {
        *n_out = 0;
        return LS_OK;
    }
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    Staging st;
    const int p_hits = st.in(hits, (size_t)n * 16), p_rays = st.in(rays, (size_t)n_rays * 32), p_refl = st.in(refl, (size_t)n_refl * 4),
              p_points = st.out(points32, n, 32), p_out = st.out(hits_out, n, 16), p_n = st.scratch(4);
    if (mv) mv->stage(tr, st);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    if (mv) mv->use_staged(io);
    if ((rc = returns_issue(tr, s, model, frame_index, staged_rays(io, p_rays, p_hits, rays), n_rays, mv, io.dev(p_hits), nullptr, n,
                            io.dev<const float>(p_refl), n_refl, io.dev(p_points), io.dev(p_out), io.dev<uint32_t>(p_n))))
        return rc;
    return io.fetch_counted(tr, p_n, n, overflow, n_out);
}

// ---- ls_hit_velocities ----------------------------------------------------------------------------------------------------------

// the sensor's twist table and the twists of the geometries as the caller gave them (host or device addresses; no table: at rest),
// resolved and staged the way Moving resolves and stages motions: the kernel takes the tables per geomID
struct Twists {
    const float *sensor;
    const ls_geometry_twist *twists;
    uint32_t n_twists;
    struct Entry { uint32_t geom; const float *table; int piece; };
    std::vector<Entry> e;
    int sensor_piece = -1;

    // what every call refuses of them, in this order (nothing of it needs a commit or the device)
    int args_check(ls_tracer *tr) const
    {
        if (n_twists && !twists) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null twists with n_twists > 0");
        for (uint32_t k = 0; k < n_twists; ++k)
            if (!twists[k].col_twist) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a twist without a table");
        for (uint32_t k = 0; k < n_twists; ++k)
            if (twists[k].reserved) return fail(tr, LS_ERR_INVALID_ARGUMENT, "ls_geometry_twist.reserved must be 0");
        if (n_twists > tr->geoms.size()) return fail(tr, LS_ERR_INVALID_ARGUMENT, "more twists than geometries");
        std::vector<uint32_t> ids(n_twists);
        for (uint32_t k = 0; k < n_twists; ++k) ids[k] = twists[k].geom;
        std::sort(ids.begin(), ids.end());
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a geometry named by two twists");
        return LS_OK;
    }
    bool misaligned4() const
    {
        bool bad = misaligned(sensor, 4);
        for (uint32_t k = 0; k < n_twists; ++k) bad = bad || misaligned(twists[k].col_twist, 4);
        return bad;
    }
    // the last refusal, after the motions': LS_ERR_UNKNOWN_GEOMETRY for a twist of a geometry that is not in the committed scene
    int resolve(ls_tracer *tr)
    {
        const std::vector<int> &ids = tr->slot_geom_ids;
        for (uint32_t k = 0; k < n_twists; ++k) {
            const size_t slot = (size_t)(std::find(ids.begin(), ids.end(), (int)twists[k].geom) - ids.begin());
            if (slot >= tr->layout.size()) return fail(tr, LS_ERR_UNKNOWN_GEOMETRY, "a twist names a geometry that is not in the committed scene");
            e.push_back({twists[k].geom, twists[k].col_twist, -1});
        }
        return LS_OK;
    }
    std::vector<const float *> per_geom(size_t n) const   // (a geomID beyond n is left out: the kernel checks against one bound)
    {
        std::vector<const float *> t(n, nullptr);
        for (const Entry &x : e)
            if (x.geom < n) t[x.geom] = x.table;
        return t;
    }
    // the sensor's table (H records of 24 bytes, or none) and the named geometries'
    void stage(const ls_tracer *tr, Staging &st)
    {
        sensor_piece = st.in(sensor, (size_t)tr->H * 24);
        for (Entry &x : e) x.piece = st.in(x.table, (size_t)tr->H * 24);
    }
    void use_staged(const Staged &io)
    {
        sensor = io.dev<const float>(sensor_piece);
        for (Entry &x : e) x.table = io.dev<const float>(x.piece);
    }
};

// what the device entry point and the host-memory variant (any alignment) refuse, in this order
int vel_check(ls_tracer *tr, Moving &mv, uint32_t flags, Twists &tw, const void *hits, const uint32_t *count, uint32_t n, const void *out,
              const float *radial, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (n && (!hits || (!out && !radial))) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records, or neither output");
    // the pose table, then the flags -- this call has none, LS_SWEEP_DESKEW included --, then the motions
    if (const int rc = pose_flags_check(tr, mv.col_pose, mv.n_cols, 0)) return rc;
    if (flags) return fail(tr, LS_ERR_INVALID_ARGUMENT, "unknown flags: ls_hit_velocities takes none");
    if (const int rc = moving_args_check(tr, mv)) return rc;
    if (const int rc = tw.args_check(tr)) return rc;
    if (!host && (moving_misaligned({hits, out}, {count, radial}, mv) || tw.misaligned4()))
        return fail(tr, LS_ERR_INVALID_ARGUMENT,
                    "hit records and velocity records must be 16-byte aligned, the count, the radial array, the poses, the motion tables and the "
                    "twist tables 4-byte aligned");
    if (n > kMaxQueryRecords) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records in one call");
    if (const int rc = uncommitted(tr)) return rc;   // (before n = 0: the same answer whatever n)
    if (const int rc = moving_resolve(tr, mv)) return rc;
    return tw.resolve(tr);
}

int vel_issue(ls_tracer *tr, hipStream_t s, const Moving &mv, const Twists &tw, const void *d_hits, const uint32_t *d_count, uint32_t n, void *d_out,
              float *d_radial)
{
    ls_tracer::HitAttr &a = tr->ha;
    if (const int rc = tables_prepare(tr, s, &mv)) return rc;
    std::vector<const float *> by_id = tw.per_geom(a.table.current.size());
    if (const int rc = a.twist.upload_if_changed(tr, s, by_id)) return rc;
    ls::launch_hit_velocities(s, d_hits, d_count, n, tables(tr), a.table.dev.p, a.motion.dev.p, a.twist.dev.p, (uint32_t)a.table.current.size(),
                              mv.col_pose, tw.sensor, d_out, d_radial);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// records, tables and results staged in q.io, on the handle's stream; returns when the outputs are filled
int vel_host(ls_tracer *tr, Moving &mv, Twists &tw, const void *hits, uint32_t n, void *out, float *radial)
{
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    Staging st;
    const int p_hits = st.in(hits, (size_t)n * 16), p_out = st.out(out, n, 32), p_radial = st.out(radial, n, 4);
    mv.stage(tr, st);
    tw.stage(tr, st);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    mv.use_staged(io);
    tw.use_staged(io);
    if ((rc = vel_issue(tr, s, mv, tw, io.dev(p_hits), nullptr, n, io.dev(p_out), io.dev<float>(p_radial)))) return rc;
    return io.fetch(tr);
}

}  // namespace

void hit_attr_release(ls_tracer *tr)
{
    ls_tracer::HitAttr &a = tr->ha;
    a.table.release();
    a.motion.release();
    a.twist.release();
    a.tri_first.release();
    release(a.park); release(a.block_counts);
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
    if ((rc = attr_check(tr, d_rays, n_rays, nullptr, d_hits, d_count, n, d_out, false)) || !n) return rc;
    return query_run(tr, s, [&] { return attr_issue(tr, s, d_rays, n_rays, nullptr, d_hits, d_count, n, d_out); });
}

int ls_hit_attributes_host(ls_tracer *tr, const void *rays, uint32_t n_rays, const void *hits, uint32_t n, void *out)
{
    LS_ENTER(tr);
    int rc;
    if ((rc = attr_check(tr, rays, n_rays, nullptr, hits, nullptr, n, out, true)) || !n) return rc;
    return attr_host(tr, rays, n_rays, nullptr, hits, n, out);
}

int ls_apply_return_model(ls_tracer *tr, void *hip_stream, const ls_return_model *model, uint32_t frame_index, const void *d_rays, uint32_t n_rays,
                          const void *d_hits, const uint32_t *d_count, uint32_t n, const float *d_reflectivity, uint32_t n_reflectivity,
                          void *d_points32, void *d_hits_out, uint32_t *d_n_out)
{
    LS_ENTER_CHECKED(tr, returns_check(tr, model, d_rays, n_rays, nullptr, d_hits, d_count, n, d_reflectivity, n_reflectivity, d_points32, d_hits_out,
                                       d_n_out, false));
    const hipStream_t s = stream_of(tr, hip_stream);
    return query_run(tr, s, [&] {
        return returns_issue(tr, s, model, frame_index, d_rays, n_rays, nullptr, d_hits, d_count, n, d_reflectivity, n_reflectivity, d_points32,
                             d_hits_out, d_n_out);
    });
}

int ls_apply_return_model_host(ls_tracer *tr, const ls_return_model *model, uint32_t frame_index, const void *rays, uint32_t n_rays,
                               const void *hits, uint32_t n, const float *reflectivity, uint32_t n_reflectivity, void *points32, void *hits_out,
                               uint32_t *n_out)
{
    LS_ENTER_CHECKED(tr, returns_check(tr, model, rays, n_rays, nullptr, hits, nullptr, n, reflectivity, n_reflectivity, points32, hits_out, n_out,
                                       true));
    return returns_host(tr, "ls_apply_return_model: more returns than records", model, frame_index, rays, n_rays, nullptr, hits, n, reflectivity,
                        n_reflectivity, points32, hits_out, n_out);
}

int ls_hit_attributes_moving(ls_tracer *tr, void *hip_stream, const float *d_col_pose, uint32_t n_cols, const ls_geometry_motion *motions,
                             uint32_t n_motions, uint32_t flags, const void *d_hits, const uint32_t *d_count, uint32_t n, void *d_out)
{
    Moving mv = {d_col_pose, n_cols, motions, n_motions, flags};
    LS_ENTER_CHECKED(tr, attr_check(tr, nullptr, 0, &mv, d_hits, d_count, n, d_out, false));
    if (!n) return LS_OK;
    const hipStream_t s = stream_of(tr, hip_stream);
    return query_run(tr, s, [&] { return attr_issue(tr, s, nullptr, 0, &mv, d_hits, d_count, n, d_out); });
}

int ls_hit_attributes_moving_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions,
                                  uint32_t flags, const void *hits, uint32_t n, void *out)
{
    Moving mv = {col_pose, n_cols, motions, n_motions, flags};
    LS_ENTER_CHECKED(tr, attr_check(tr, nullptr, 0, &mv, hits, nullptr, n, out, true));
    if (!n) return LS_OK;
    return attr_host(tr, nullptr, 0, &mv, hits, n, out);
}

int ls_apply_return_model_moving(ls_tracer *tr, void *hip_stream, const ls_return_model *model, uint32_t frame_index, const float *d_col_pose,
                                 uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags, const void *d_hits,
                                 const uint32_t *d_count, uint32_t n, const float *d_reflectivity, uint32_t n_reflectivity, void *d_points32,
                                 void *d_hits_out, uint32_t *d_n_out)
{
    Moving mv = {d_col_pose, n_cols, motions, n_motions, flags};
    LS_ENTER_CHECKED(tr, returns_check(tr, model, nullptr, 0, &mv, d_hits, d_count, n, d_reflectivity, n_reflectivity, d_points32, d_hits_out, d_n_out,
                                       false));
    const hipStream_t s = stream_of(tr, hip_stream);
    return query_run(tr, s, [&] {
        return returns_issue(tr, s, model, frame_index, nullptr, 0, &mv, d_hits, d_count, n, d_reflectivity, n_reflectivity, d_points32, d_hits_out,
                             d_n_out);
    });
}

int ls_apply_return_model_moving_host(ls_tracer *tr, const ls_return_model *model, uint32_t frame_index, const float *col_pose, uint32_t n_cols,
                                      const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags, const void *hits, uint32_t n,
                                      const float *reflectivity, uint32_t n_reflectivity, void *points32, void *hits_out, uint32_t *n_out)
{
    Moving mv = {col_pose, n_cols, motions, n_motions, flags};
    LS_ENTER_CHECKED(tr, returns_check(tr, model, nullptr, 0, &mv, hits, nullptr, n, reflectivity, n_reflectivity, points32, hits_out, n_out, true));
    return returns_host(tr, "ls_apply_return_model_moving: more returns than records", model, frame_index, nullptr, 0, &mv, hits, n, reflectivity,
                        n_reflectivity, points32, hits_out, n_out);
}

int ls_hit_velocities(ls_tracer *tr, void *hip_stream, const float *d_col_pose, uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions,
                      const float *d_sensor_twist, const ls_geometry_twist *twists, uint32_t n_twists, uint32_t flags, const void *d_hits,
                      const uint32_t *d_count, uint32_t n, void *d_out, float *d_radial)
{
    Moving mv = {d_col_pose, n_cols, motions, n_motions, 0u};
    Twists tw = {d_sensor_twist, twists, n_twists};
    LS_ENTER_CHECKED(tr, vel_check(tr, mv, flags, tw, d_hits, d_count, n, d_out, d_radial, false));
    if (!n) return LS_OK;
    const hipStream_t s = stream_of(tr, hip_stream);
    return query_run(tr, s, [&] { return vel_issue(tr, s, mv, tw, d_hits, d_count, n, d_out, d_radial); });
}

int ls_hit_velocities_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions,
                           const float *sensor_twist, const ls_geometry_twist *twists, uint32_t n_twists, uint32_t flags, const void *hits, uint32_t n,
                           void *out, float *radial)
{
    Moving mv = {col_pose, n_cols, motions, n_motions, 0u};
    Twists tw = {sensor_twist, twists, n_twists};
    LS_ENTER_CHECKED(tr, vel_check(tr, mv, flags, tw, hits, nullptr, n, out, radial, true));
    if (!n) return LS_OK;
    return vel_host(tr, mv, tw, hits, n, out, radial);
}

}  // extern "C"
