// ls_scan.cpp -- the frames built around the queries' walk (query_enter / query_walk / query_leave, ls_query.cpp; its hierarchies, its
// return codes, its stream order), each with its host-memory variant:
//   ls_trace_scene_sweep  a frame whose sensor moves during the turn -- the shard's rays through per-column poses, the closest-hit
//                         walk over them, an ordered pack (ls_sweep.hip); ls_sweep_poses_constant_twist: a pose table;
//   ls_trace_scene_beams  a frame of diverging beams -- S sub-rays per ray of the shard, the same walk over them, the echoes of every
//                         beam and an ordered pack of the selected returns (ls_beam.hip); ls_beam_pattern_rings: a sample pattern;
//   ls_trace_scene_beams_sweep  the two together, with a weight per sample: the sub-rays through per-column poses, the same walk,
//                         the weighted echoes and their pack (ls_beam.hip); ls_beam_weights_gaussian: a weight per sample;
//   ls_trace_scene_sweep_moving  the sweep with geometries that move during the turn: the sweep's rays and pack around the walk that
//                         carries each ray through the inverse of a geometry's motion (ls_moving.hip); ls_motion_constant_twist: a
//                         motion table; ls_twist_table_constant: that body's twist table (ls_hit_velocities, ls_gather.cpp).
#include "ls_internal.h"
#include "ls_beam.h"

#include <algorithm>
#include <cmath>

namespace lsi {

int pose_flags_check(ls_tracer *tr, const float *col_pose, uint32_t n_cols, uint32_t flags)
{
    if (col_pose ? n_cols != tr->H : n_cols != 0u)
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "one pose per azimuth column of the full raster (LS_INFO_AZIMUTH_COUNT), or no table and n_cols 0");
    if (flags & ~(uint32_t)LS_SWEEP_DESKEW) return fail(tr, LS_ERR_INVALID_ARGUMENT, "unknown sweep flags");
    return LS_OK;
}

int moving_args_check(ls_tracer *tr, const Moving &mv)
{
    const ls_geometry_motion *motions = mv.motions;
    const uint32_t n_motions = mv.n_motions;
    if (const int rc = pose_flags_check(tr, mv.col_pose, mv.n_cols, mv.flags)) return rc;
    if (n_motions && !motions) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null motions with n_motions > 0");
    for (uint32_t k = 0; k < n_motions; ++k)
        if (!motions[k].col_motion) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a motion without a table");
    for (uint32_t k = 0; k < n_motions; ++k)
        if (motions[k].reserved) return fail(tr, LS_ERR_INVALID_ARGUMENT, "ls_geometry_motion.reserved must be 0");
    if (n_motions > tr->geoms.size()) return fail(tr, LS_ERR_INVALID_ARGUMENT, "more motions than geometries");
    std::vector<uint32_t> ids(n_motions);
    for (uint32_t k = 0; k < n_motions; ++k) ids[k] = motions[k].geom;
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a geometry named by two motions");
    return LS_OK;
}

bool moving_misaligned(std::initializer_list<const void *> p16, std::initializer_list<const void *> p4, const Moving &mv)
{
    bool bad = misaligned(mv.col_pose, 4);
    for (const void *p : p16) bad = bad || misaligned(p, 16);
    for (const void *p : p4) bad = bad || misaligned(p, 4);
    for (uint32_t k = 0; k < mv.n_motions; ++k) bad = bad || misaligned(mv.motions[k].col_motion, 4);
    return bad;
}

int moving_resolve(ls_tracer *tr, Moving &mv)
{
    const std::vector<int> &ids = tr->slot_geom_ids;   // geometry ids in layout order
    for (uint32_t k = 0; k < mv.n_motions; ++k) {
        const size_t slot = (size_t)(std::find(ids.begin(), ids.end(), (int)mv.motions[k].geom) - ids.begin());
        if (slot >= tr->layout.size()) return fail(tr, LS_ERR_UNKNOWN_GEOMETRY, "a motion names a geometry that is not in the committed scene");
        mv.e.push_back({slot, mv.motions[k].geom, mv.motions[k].col_motion, -1});
    }
    return LS_OK;
}

std::vector<const float *> Moving::per_slot(size_t n) const
{
    std::vector<const float *> t(n, nullptr);
    for (const Entry &x : e) t[x.slot] = x.table;
    return t;
}

std::vector<const float *> Moving::per_geom(size_t n) const
{
    std::vector<const float *> t(n, nullptr);
    for (const Entry &x : e)
        if (x.geom < n) t[x.geom] = x.table;
    return t;
}

// the pose table (H records of 48 bytes, or none) and the named geometries' tables (48 H bytes each: every one starts 16-byte aligned)
void Moving::stage(const ls_tracer *tr, Staging &st)
{
    pose_piece = st.in(col_pose, (size_t)n_cols * 48);
    for (Entry &x : e) x.piece = st.in(x.table, (size_t)tr->H * 48);
}

void Moving::use_staged(const Staged &io)
{
    col_pose = io.dev<const float>(pose_piece);
    for (Entry &x : e) x.table = io.dev<const float>(x.piece);
}

namespace {

// the last refusals of the sweeps, in this order: the shard's rays against the capacity and the limit of one call, the commit state
int shard_check(ls_tracer *tr, uint32_t capacity)
{
    if (capacity < shard_rays(tr)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "capacity below the shard's ray count");
    if (shard_rays(tr) > kMaxQueryRecords) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many rays in one call");
    tr->rq.last_built = 0;
    return uncommitted(tr);   // (nothing is written, the count included)
}

// what both sweep entry points refuse, in this order (none of it needs a commit); host memory may have any alignment
int sweep_check(ls_tracer *tr, const float *col_pose, uint32_t n_cols, uint32_t flags, const void *points32, const void *hits, const uint32_t *n_points,
                uint32_t capacity, const void *rays_out, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!col_pose || !n_points) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null pose table or count output");
    if (n_cols != tr->H) return fail(tr, LS_ERR_INVALID_ARGUMENT, "one pose per azimuth column of the full raster (LS_INFO_AZIMUTH_COUNT)");
    if (flags & ~(uint32_t)LS_SWEEP_DESKEW) return fail(tr, LS_ERR_INVALID_ARGUMENT, "unknown sweep flags");
    if (!host && (misaligned(col_pose, 4) || misaligned(n_points, 4) || misaligned16(points32, hits, rays_out)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "points, hit records and rays must be 16-byte aligned, the poses and the count 4-byte aligned");
    return shard_check(tr, capacity);
}

// what both entry points of the sweep over moving geometries refuse, in this order; host memory may have any alignment
int sweep_moving_check(ls_tracer *tr, Moving &mv, const void *points32, const void *hits, const uint32_t *n_points, uint32_t capacity, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!n_points) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null count output");
    if (const int rc = moving_args_check(tr, mv)) return rc;
    if (!host && moving_misaligned({points32, hits}, {n_points}, mv))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "points and hit records must be 16-byte aligned, the poses, the motion tables and the count 4-byte aligned");
    if (const int rc = shard_check(tr, capacity)) return rc;
    return moving_resolve(tr, mv);
}

// Both sweeps: the shard's rays, the closest-hit walk over them, the ordered pack.  No pose table: the sensor at rest -- the nominal
// rays from the origin (the centre sample of a beam: ls_trace_scene's rays), nothing to deskew; no motions: the walk of
// ls_trace_scene_sweep; d_rays_out: that call's
int sweep_issue(ls_tracer *tr, hipStream_t s, const Moving &mv, void *d_points32, void *d_hits, uint32_t *d_n_points, void *d_rays_out)
{
    ls_tracer::RayQuery &q = tr->rq;
    const uint32_t nq = shard_rays(tr);
    const float *d_col_pose = mv.col_pose;
    int rc;
    if ((rc = ensure(tr, q.sweep_rays, (size_t)nq * 32))) return rc;
    if ((rc = ensure(tr, q.sweep_hits, (size_t)nq * 16))) return rc;
    if ((rc = ensure(tr, q.sweep_counts, ls::sweep_block_count(nq)))) return rc;
    const ls::SensorTables tb = tables(tr);
    if (d_col_pose) {
        ls::launch_sweep_rays(s, tb, d_col_pose, q.sweep_rays.p, d_rays_out);
    } else {
        ls::BeamPattern pat;
        std::memset(static_cast<void *>(&pat), 0, sizeof(pat));
        pat.k[0] = 1.0f;
        ls::launch_beam_rays(s, tb, pat, 1, q.sweep_rays.p);
    }
    const std::vector<const float *> d_motion = mv.per_slot(tr->layout.size());
    if ((rc = query_walk(tr, s, q.sweep_rays.p, nq, q.sweep_hits.p, closest_hits(), mv.n_motions ? d_motion.data() : nullptr))) return rc;
    ls::launch_sweep_pack(s, tb, q.sweep_hits.p, q.sweep_counts.p, d_col_pose, d_col_pose && (mv.flags & LS_SWEEP_DESKEW) != 0, d_points32, d_hits,
                          d_n_points);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// the poses (or none), the motion tables and the outputs staged in q.io, on the handle's stream; the count comes back first, then as
// many records; of rays_out (ls_trace_scene_sweep_host's) only the shard's columns are written: V rows of naz records, at their
// place in the rows of H
int sweep_host(ls_tracer *tr, const char *overflow, Moving &mv, void *points32, void *hits, uint32_t *n_points, void *rays_out)
{
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    const size_t nq = shard_rays(tr), row_bytes = (size_t)tr->H * 32;
    Staging st;
    const int p_points = st.out(points32, nq, 32), p_hits = st.out(hits, nq, 16), p_rays = st.scratch(rays_out ? tr->V * row_bytes : 0),
              p_n = st.scratch(4);
    mv.stage(tr, st);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    mv.use_staged(io);
    if ((rc = sweep_issue(tr, s, mv, io.dev(p_points), io.dev(p_hits), io.dev<uint32_t>(p_n), io.dev(p_rays)))) return rc;
    const StridedRows rows = {rays_out, p_rays, (size_t)tr->az0 * 32, (size_t)tr->naz * 32, tr->V, row_bytes};
    return io.fetch_counted(tr, p_n, nq, overflow, n_points, &rows);
}

// what ls_trace_scene_beams_sweep takes beyond ls_trace_scene_beams (nullptr where a function serves both: that call)
struct BeamSweep {
    const uint32_t *weights;
    uint32_t min_weight;
    const float *col_pose;
    uint32_t n_cols, flags;
};

// what the entry points of both beam frames refuse, in this order, before anything touches the device; host memory may have any alignment
int beams_check(ls_tracer *tr, const ls_beam_model *model, const BeamSweep *sw, const void *points32, const void *hits, const uint32_t *echo,
                const uint32_t *n_points, uint32_t capacity, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!n_points) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null count output");
    int status = LS_OK;
    if (const char *why = ls::beam_model_invalid(model, shard_rays(tr), capacity, &status)) return fail(tr, status, why);
    if (sw) {
        if (const char *why = ls::beam_weights_invalid(sw->weights, model->n_samples)) return fail(tr, LS_ERR_INVALID_ARGUMENT, why);
        if (const int rc = pose_flags_check(tr, sw->col_pose, sw->n_cols, sw->flags)) return rc;
    }
    if (!host && (misaligned16(points32, hits) || misaligned(echo, 4) || misaligned(n_points, 4) || (sw && misaligned(sw->col_pose, 4))))
        return fail(tr, LS_ERR_INVALID_ARGUMENT,
                    sw ? "points and hit records must be 16-byte aligned, the echo words, the count and the poses 4-byte aligned"
                       : "points and hit records must be 16-byte aligned, the echo words and the count 4-byte aligned");
    tr->rq.last_built = 0;
    return uncommitted(tr);   // (nothing is written, the count included)
}

// Both beam frames: the sub-rays, the closest-hit walk over them, the echoes of every beam and their ordered pack -- each frame with
// its own two launches.  The caller's pattern and weights are read here and now: they travel in the kernel arguments.  The scratch:
// sub-rays, their hit records, the returns of every beam; in one array the return count of every beam, of every 256 of them and,
// under a sweep, a strength per record
int beams_issue(ls_tracer *tr, hipStream_t s, const ls_beam_model *model, const BeamSweep *sw, void *d_points32, void *d_hits, uint32_t *d_echo,
                uint32_t *d_n_points, uint32_t capacity)
{
    ls_tracer::RayQuery &q = tr->rq;
    const uint32_t nq = shard_rays(tr), S = model->n_samples, n = nq * S;   // n <= 2^27
    const size_t n_blocks = ls::beam_block_count(nq);
    ls::BeamPattern pat;
    std::memset(static_cast<void *>(&pat), 0, sizeof(pat));
    for (uint32_t k = 0; k < S; ++k) {
        pat.a[k] = model->pattern[3 * k];
        pat.b[k] = model->pattern[3 * k + 1];
        pat.k[k] = model->pattern[3 * k + 2];
    }
    int rc;
    if ((rc = ensure(tr, q.beam_rays, (size_t)n * 32))) return rc;
    if ((rc = ensure(tr, q.beam_hits, (size_t)n * 16))) return rc;
    if ((rc = ensure(tr, q.beam_blocks, 3 * (size_t)nq))) return rc;
    if ((rc = ensure(tr, q.beam_counts, (size_t)nq + n_blocks + (sw ? 3 * (size_t)nq : 0)))) return rc;
    const ls::SensorTables tb = tables(tr);
    if (sw) ls::launch_beam_sweep_rays(s, tb, pat, S, sw->col_pose, q.beam_rays.p);
    else ls::launch_beam_rays(s, tb, pat, S, q.beam_rays.p);
    if ((rc = query_walk(tr, s, q.beam_rays.p, n, q.beam_hits.p, closest_hits()))) return rc;
    if (sw) {
        uint32_t w_total = 0;
        const ls::BeamWeights wts = ls::beam_weights_by_value(sw->weights, S, &w_total);
        ls::launch_beam_sweep_pack(s, tb, pat, wts, w_total, S, model->echo_separation, model->min_count, sw->min_weight, model->returns, sw->col_pose,
                                   (sw->flags & LS_SWEEP_DESKEW) != 0, q.beam_hits.p, q.beam_blocks.p, q.beam_counts.p + nq + n_blocks, q.beam_counts.p,
                                   q.beam_counts.p + nq, d_points32, d_hits, d_echo, d_n_points, capacity);
    } else {
        ls::launch_beam_pack(s, tb, pat, S, model->echo_separation, model->min_count, model->returns, q.beam_hits.p, q.beam_blocks.p, q.beam_counts.p,
                             q.beam_counts.p + nq, d_points32, d_hits, d_echo, d_n_points, capacity);
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// the poses (if any) and the outputs staged in q.io, on the handle's stream; the count comes back first, then as many records
int beams_host(ls_tracer *tr, const char *overflow, const ls_beam_model *model, const BeamSweep *sw, void *points32, void *hits, uint32_t *echo,
               uint32_t *n_points)
{
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    const size_t cap = (size_t)__builtin_popcount(model->returns) * shard_rays(tr);   // what the beams can give: <= 3 * 2^27
    Staging st;
    const int p_pose = st.in(sw ? sw->col_pose : nullptr, sw ? (size_t)sw->n_cols * 48 : 0), p_points = st.out(points32, cap, 32),
              p_hits = st.out(hits, cap, 16), p_echo = st.out(echo, cap, 4), p_n = st.scratch(4);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    BeamSweep d_sw = sw ? *sw : BeamSweep();
    d_sw.col_pose = io.dev<const float>(p_pose);
    if ((rc = beams_issue(tr, s, model, sw ? &d_sw : nullptr, io.dev(p_points), io.dev(p_hits), io.dev<uint32_t>(p_echo), io.dev<uint32_t>(p_n),
                          (uint32_t)cap)))
        return rc;
    return io.fetch_counted(tr, p_n, cap, overflow, n_points);
}

// tau_h = t0 + h dt; Q_h = Rodrigues' rotation by ang_vel * tau_h, c_h = (pivot - Q_h pivot) + lin_vel * tau_h (pivot nullptr: the
// origin); double throughout, one rounding.  A turn about a pivot that leaves an offset of zero adds nothing: -0 + 0 would be +0.
void twist_table(const float *lin_vel, const float *ang_vel, const float *pivot, double t0, double dt, uint32_t n_cols, float *out)
{
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
        float *p = out + 12 * (size_t)h;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) p[4 * i + j] = (float)R[3 * i + j];
            const double drive = (double)lin_vel[i] * tau;
            double turn = 0.0;
            if (pivot) turn = (double)pivot[i] - ((R[3 * i] * (double)pivot[0] + R[3 * i + 1] * (double)pivot[1]) + R[3 * i + 2] * (double)pivot[2]);
            p[4 * i + 3] = (float)(turn != 0.0 ? turn + drive : drive);
        }
    }
}

bool twist_finite(const float *lin_vel, const float *ang_vel, const float *pivot, double t0, double dt)
{
    if (!std::isfinite(t0) || !std::isfinite(dt)) return false;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(lin_vel[k]) || !std::isfinite(ang_vel[k]) || (pivot && !std::isfinite(pivot[k]))) return false;
    return true;
}

}  // namespace

}  // namespace lsi

using namespace lsi;

extern "C" {

int ls_trace_scene_sweep(ls_tracer *tr, void *hip_stream, const float *d_col_pose, uint32_t n_cols, uint32_t flags, void *d_points32, void *d_hits,
                         uint32_t *d_n_points, uint32_t capacity, void *d_rays_out)
{
    LS_ENTER(tr);
    const hipStream_t s = stream_of(tr, hip_stream);
    if (const int rc = sweep_check(tr, d_col_pose, n_cols, flags, d_points32, d_hits, d_n_points, capacity, d_rays_out, false)) return rc;
    const Moving mv = {d_col_pose, n_cols, nullptr, 0, flags};
    return query_run(tr, s, [&] { return sweep_issue(tr, s, mv, d_points32, d_hits, d_n_points, d_rays_out); });
}

int ls_trace_scene_sweep_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols, uint32_t flags, void *points32, void *hits, uint32_t *n_points,
                              uint32_t capacity, void *rays_out)
{
    LS_ENTER(tr);
    if (const int rc = sweep_check(tr, col_pose, n_cols, flags, points32, hits, n_points, capacity, rays_out, true)) return rc;
    Moving mv = {col_pose, n_cols, nullptr, 0, flags};
    return sweep_host(tr, "ls_trace_scene_sweep: more points than rays", mv, points32, hits, n_points, rays_out);
}

int ls_trace_scene_beams(ls_tracer *tr, void *hip_stream, const ls_beam_model *model, void *d_points32, void *d_hits, uint32_t *d_echo,
                         uint32_t *d_n_points, uint32_t capacity)
{
    LS_ENTER_CHECKED(tr, beams_check(tr, model, nullptr, d_points32, d_hits, d_echo, d_n_points, capacity, false));
    const hipStream_t s = stream_of(tr, hip_stream);
    return query_run(tr, s, [&] { return beams_issue(tr, s, model, nullptr, d_points32, d_hits, d_echo, d_n_points, capacity); });
}

int ls_trace_scene_beams_host(ls_tracer *tr, const ls_beam_model *model, void *points32, void *hits, uint32_t *echo, uint32_t *n_points,
                              uint32_t capacity)
{
    LS_ENTER_CHECKED(tr, beams_check(tr, model, nullptr, points32, hits, echo, n_points, capacity, true));
    return beams_host(tr, "ls_trace_scene_beams: more returns than the beams can give", model, nullptr, points32, hits, echo, n_points);
}

int ls_trace_scene_beams_sweep(ls_tracer *tr, void *hip_stream, const ls_beam_model *model, const uint32_t *weights, uint32_t min_weight,
                               const float *d_col_pose, uint32_t n_cols, uint32_t flags, void *d_points32, void *d_hits, uint32_t *d_echo,
                               uint32_t *d_n_points, uint32_t capacity)
{
    const BeamSweep sw = {weights, min_weight, d_col_pose, n_cols, flags};
    LS_ENTER_CHECKED(tr, beams_check(tr, model, &sw, d_points32, d_hits, d_echo, d_n_points, capacity, false));
    const hipStream_t s = stream_of(tr, hip_stream);
    return query_run(tr, s, [&] { return beams_issue(tr, s, model, &sw, d_points32, d_hits, d_echo, d_n_points, capacity); });
}

int ls_trace_scene_beams_sweep_host(ls_tracer *tr, const ls_beam_model *model, const uint32_t *weights, uint32_t min_weight, const float *col_pose,
                                    uint32_t n_cols, uint32_t flags, void *points32, void *hits, uint32_t *echo, uint32_t *n_points, uint32_t capacity)
{
    const BeamSweep sw = {weights, min_weight, col_pose, n_cols, flags};
    LS_ENTER_CHECKED(tr, beams_check(tr, model, &sw, points32, hits, echo, n_points, capacity, true));
    return beams_host(tr, "ls_trace_scene_beams_sweep: more returns than the beams can give", model, &sw, points32, hits, echo, n_points);
}

// host only: w_s = max(1, round(65535 exp(-((a / sigma_az)^2 + (b / sigma_el)^2) / 2))); double throughout, one rounding
int ls_beam_weights_gaussian(const float *pattern, uint32_t n_samples, float sigma_az, float sigma_el, uint32_t *weights)
{
    if (!pattern || !weights || n_samples < 1u || n_samples > ls::kBeamMaxSamples) return LS_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(sigma_az) || !std::isfinite(sigma_el) || !(sigma_az > 0.0f) || !(sigma_el > 0.0f)) return LS_ERR_INVALID_ARGUMENT;
    for (uint32_t k = 0; k < 3u * n_samples; ++k)
        if (!std::isfinite(pattern[k])) return LS_ERR_INVALID_ARGUMENT;
    for (uint32_t s = 0; s < n_samples; ++s) {
        const double a = (double)pattern[3 * s] / (double)sigma_az, b = (double)pattern[3 * s + 1] / (double)sigma_el;
        const double w = std::round(65535.0 * std::exp(-0.5 * (a * a + b * b)));
        weights[s] = w < 1.0 ? 1u : (uint32_t)w;
    }
    return LS_OK;
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
    if (!twist_finite(lin_vel, ang_vel, nullptr, t0, dt)) return LS_ERR_INVALID_ARGUMENT;
    twist_table(lin_vel, ang_vel, nullptr, t0, dt, n_cols, col_pose);
    return LS_OK;
}

// host only: the same table for a body that turns about `pivot` while it drives on: c_h = pivot - Q_h pivot + lin_vel * tau_h
int ls_motion_constant_twist(const float lin_vel[3], const float ang_vel[3], const float pivot[3], double t0, double dt, uint32_t n_cols,
                             float *col_motion)
{
    if (!lin_vel || !ang_vel || !pivot || (n_cols && !col_motion)) return LS_ERR_INVALID_ARGUMENT;
    if (!twist_finite(lin_vel, ang_vel, pivot, t0, dt)) return LS_ERR_INVALID_ARGUMENT;
    twist_table(lin_vel, ang_vel, pivot, t0, dt, n_cols, col_motion);
    return LS_OK;
}

// host only: the twist of the body whose displacement table ls_motion_constant_twist writes for the same arguments -- w_h = ang_vel,
// u_h = lin_vel - ang_vel x (pivot + lin_vel tau_h); double throughout, one rounding; a cross product that is zero leaves lin_vel's bits
int ls_twist_table_constant(const float lin_vel[3], const float ang_vel[3], const float pivot[3], double t0, double dt, uint32_t n_cols,
                            float *col_twist)
{
    if (!lin_vel || !ang_vel || !pivot || (n_cols && !col_twist)) return LS_ERR_INVALID_ARGUMENT;
    if (!twist_finite(lin_vel, ang_vel, pivot, t0, dt)) return LS_ERR_INVALID_ARGUMENT;
    const double w[3] = {ang_vel[0], ang_vel[1], ang_vel[2]};
    for (uint32_t h = 0; h < n_cols; ++h) {
        const double tau = t0 + (double)h * dt;
        double a[3];
        for (int i = 0; i < 3; ++i) a[i] = (double)pivot[i] + (double)lin_vel[i] * tau;
        const double cross[3] = {w[1] * a[2] - w[2] * a[1], w[2] * a[0] - w[0] * a[2], w[0] * a[1] - w[1] * a[0]};
        float *p = col_twist + 6 * (size_t)h;
        for (int i = 0; i < 3; ++i) {
            p[i] = ang_vel[i];
            p[3 + i] = cross[i] != 0.0 ? (float)((double)lin_vel[i] - cross[i]) : lin_vel[i];
        }
    }
    return LS_OK;
}

int ls_trace_scene_sweep_moving(ls_tracer *tr, void *hip_stream, const float *d_col_pose, uint32_t n_cols, const ls_geometry_motion *motions,
                                uint32_t n_motions, uint32_t flags, void *d_points32, void *d_hits, uint32_t *d_n_points, uint32_t capacity)
{
    Moving mv = {d_col_pose, n_cols, motions, n_motions, flags};
    LS_ENTER_CHECKED(tr, sweep_moving_check(tr, mv, d_points32, d_hits, d_n_points, capacity, false));
    const hipStream_t s = stream_of(tr, hip_stream);
    return query_run(tr, s, [&] { return sweep_issue(tr, s, mv, d_points32, d_hits, d_n_points, nullptr); });
}

int ls_trace_scene_sweep_moving_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions,
                                     uint32_t flags, void *points32, void *hits, uint32_t *n_points, uint32_t capacity)
{
    Moving mv = {col_pose, n_cols, motions, n_motions, flags};
    LS_ENTER_CHECKED(tr, sweep_moving_check(tr, mv, points32, hits, n_points, capacity, true));
    return sweep_host(tr, "ls_trace_scene_sweep_moving: more points than rays", mv, points32, hits, n_points, nullptr);
}

}  // extern "C"
