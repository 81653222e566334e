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
//                         motion table.
#include "ls_internal.h"
#include "ls_beam.h"

#include <algorithm>
#include <cmath>

namespace lsi {

int motion_args_check(ls_tracer *tr, const float *col_pose, uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags)
{
    if (col_pose ? n_cols != tr->H : n_cols != 0u)
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "one pose per azimuth column of the full raster (LS_INFO_AZIMUTH_COUNT), or no table and n_cols 0");
    if (flags & ~(uint32_t)LS_SWEEP_DESKEW) return fail(tr, LS_ERR_INVALID_ARGUMENT, "unknown sweep flags");
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

namespace {

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
    if (capacity < shard_rays(tr)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "capacity below the shard's ray count");
    if (shard_rays(tr) > kMaxQueryRecords) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many rays in one call");
    tr->rq.last_built = 0;
    return uncommitted(tr);   // (nothing is written, the count included)
}

int sweep_issue(ls_tracer *tr, hipStream_t s, const float *d_col_pose, uint32_t flags, void *d_points32, void *d_hits, uint32_t *d_n_points,
                void *d_rays_out)
{
    ls_tracer::RayQuery &q = tr->rq;
    const uint32_t nq = shard_rays(tr);
    int rc;
    if ((rc = ensure(tr, q.sweep_rays, (size_t)nq * 32))) return rc;
    if ((rc = ensure(tr, q.sweep_hits, (size_t)nq * 16))) return rc;
    if ((rc = ensure(tr, q.sweep_counts, ls::sweep_block_count(nq)))) return rc;
    const ls::SensorTables tb = tables(tr);
    ls::launch_sweep_rays(s, tb, d_col_pose, q.sweep_rays.p, d_rays_out);
    if ((rc = query_walk(tr, s, q.sweep_rays.p, nq, q.sweep_hits.p, closest_hits()))) return rc;
    ls::launch_sweep_pack(s, tb, q.sweep_hits.p, q.sweep_counts.p, d_col_pose, (flags & LS_SWEEP_DESKEW) != 0, d_points32, d_hits, d_n_points);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// what both beam entry points refuse, in this order, before anything touches the device; host memory may have any alignment
int beams_check(ls_tracer *tr, const ls_beam_model *model, const void *points32, const void *hits, const uint32_t *echo, const uint32_t *n_points,
                uint32_t capacity, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!n_points) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null count output");
    int status = LS_OK;
    if (const char *why = ls::beam_model_invalid(model, shard_rays(tr), capacity, &status)) return fail(tr, status, why);
    if (!host && (misaligned16(points32, hits) || misaligned(echo, 4) || misaligned(n_points, 4)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "points and hit records must be 16-byte aligned, the echo words and the count 4-byte aligned");
    tr->rq.last_built = 0;
    return uncommitted(tr);   // (nothing is written, the count included)
}

int beams_issue(ls_tracer *tr, hipStream_t s, const ls_beam_model *model, void *d_points32, void *d_hits, uint32_t *d_echo, uint32_t *d_n_points,
                uint32_t capacity)
{
    ls_tracer::RayQuery &q = tr->rq;
    const uint32_t nq = shard_rays(tr), S = model->n_samples, n = nq * S;   // n <= 2^27
    ls::BeamPattern pat;   // the caller's pattern, read here and now: it travels in the kernel arguments
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
    if ((rc = ensure(tr, q.beam_counts, (size_t)nq + ls::beam_block_count(nq)))) return rc;
    const ls::SensorTables tb = tables(tr);
    ls::launch_beam_rays(s, tb, pat, S, q.beam_rays.p);
    if ((rc = query_walk(tr, s, q.beam_rays.p, n, q.beam_hits.p, closest_hits()))) return rc;
    ls::launch_beam_pack(s, tb, pat, S, model->echo_separation, model->min_count, model->returns, q.beam_hits.p, q.beam_blocks.p, q.beam_counts.p,
                         q.beam_counts.p + nq, d_points32, d_hits, d_echo, d_n_points, capacity);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// what both entry points of the beams under a sweep refuse, in this order, before anything touches the device; host memory may have
// any alignment
int beams_sweep_check(ls_tracer *tr, const ls_beam_model *model, const uint32_t *weights, const float *col_pose, uint32_t n_cols, uint32_t flags,
                      const void *points32, const void *hits, const uint32_t *echo, const uint32_t *n_points, uint32_t capacity, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!n_points) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null count output");
    int status = LS_OK;
    if (const char *why = ls::beam_model_invalid(model, shard_rays(tr), capacity, &status)) return fail(tr, status, why);
    if (const char *why = ls::beam_weights_invalid(weights, model->n_samples)) return fail(tr, LS_ERR_INVALID_ARGUMENT, why);
    if (col_pose ? n_cols != tr->H : n_cols != 0u)
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "one pose per azimuth column of the full raster (LS_INFO_AZIMUTH_COUNT), or no table and n_cols 0");
    if (flags & ~(uint32_t)LS_SWEEP_DESKEW) return fail(tr, LS_ERR_INVALID_ARGUMENT, "unknown sweep flags");
    if (!host && (misaligned16(points32, hits) || misaligned(echo, 4) || misaligned(n_points, 4) || misaligned(col_pose, 4)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT,
                    "points and hit records must be 16-byte aligned, the echo words, the count and the poses 4-byte aligned");
    tr->rq.last_built = 0;
    return uncommitted(tr);   // (nothing is written, the count included)
}

int beams_sweep_issue(ls_tracer *tr, hipStream_t s, const ls_beam_model *model, const uint32_t *weights, uint32_t min_weight, const float *d_col_pose,
                      uint32_t flags, void *d_points32, void *d_hits, uint32_t *d_echo, uint32_t *d_n_points, uint32_t capacity)
{
    ls_tracer::RayQuery &q = tr->rq;
    const uint32_t nq = shard_rays(tr), S = model->n_samples, n = nq * S;   // n <= 2^27
    ls::BeamPattern pat;   // the caller's pattern and weights, read here and now: they travel in the kernel arguments
    std::memset(static_cast<void *>(&pat), 0, sizeof(pat));
    for (uint32_t k = 0; k < S; ++k) {
        pat.a[k] = model->pattern[3 * k];
        pat.b[k] = model->pattern[3 * k + 1];
        pat.k[k] = model->pattern[3 * k + 2];
    }
    uint32_t w_total = 0;
    const ls::BeamWeights wts = ls::beam_weights_by_value(weights, S, &w_total);
    const size_t n_blocks = ls::beam_block_count(nq);
    int rc;
    if ((rc = ensure(tr, q.beam_rays, (size_t)n * 32))) return rc;
    if ((rc = ensure(tr, q.beam_hits, (size_t)n * 16))) return rc;
    if ((rc = ensure(tr, q.beam_blocks, 3 * (size_t)nq))) return rc;
    if ((rc = ensure(tr, q.beam_counts, (size_t)nq + n_blocks + 3 * (size_t)nq))) return rc;   // counts, block counts, a strength per record
    const ls::SensorTables tb = tables(tr);
    ls::launch_beam_sweep_rays(s, tb, pat, S, d_col_pose, q.beam_rays.p);
    if ((rc = query_walk(tr, s, q.beam_rays.p, n, q.beam_hits.p, closest_hits()))) return rc;
    ls::launch_beam_sweep_pack(s, tb, pat, wts, w_total, S, model->echo_separation, model->min_count, min_weight, model->returns, d_col_pose,
                               (flags & LS_SWEEP_DESKEW) != 0, q.beam_hits.p, q.beam_blocks.p, q.beam_counts.p + nq + n_blocks, q.beam_counts.p,
                               q.beam_counts.p + nq, d_points32, d_hits, d_echo, d_n_points, capacity);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// what both entry points of the sweep over moving geometries refuse, in this order; host memory may have any alignment.  On LS_OK
// table[i] is the motion table of layout entry i (nullptr: at rest)
int moving_check(ls_tracer *tr, const float *col_pose, uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags,
                 const void *points32, const void *hits, const uint32_t *n_points, uint32_t capacity, bool host, std::vector<const float *> &table)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!n_points) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null count output");
    if (const int rc = motion_args_check(tr, col_pose, n_cols, motions, n_motions, flags)) return rc;
    if (!host) {
        bool bad = misaligned(col_pose, 4) || misaligned(n_points, 4) || misaligned16(points32, hits);
        for (uint32_t k = 0; k < n_motions; ++k) bad = bad || misaligned(motions[k].col_motion, 4);
        if (bad)
            return fail(tr, LS_ERR_INVALID_ARGUMENT,
                        "points and hit records must be 16-byte aligned, the poses, the motion tables and the count 4-byte aligned");
    }
    if (capacity < shard_rays(tr)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "capacity below the shard's ray count");
    if (shard_rays(tr) > kMaxQueryRecords) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many rays in one call");
    tr->rq.last_built = 0;
    if (const int rc = uncommitted(tr)) return rc;   // (nothing is written, the count included)
    // every geomID to its layout entry: the walk takes the tables in layout order
    table.assign(tr->layout.size(), nullptr);
    for (uint32_t k = 0; k < n_motions; ++k) {
        size_t i = 0;
        while (i < tr->slot_geom_ids.size() && (uint32_t)tr->slot_geom_ids[i] != motions[k].geom) ++i;
        if (i >= table.size()) return fail(tr, LS_ERR_UNKNOWN_GEOMETRY, "a motion names a geometry that is not in the committed scene");
        table[i] = motions[k].col_motion;
    }
    return LS_OK;
}

// d_col_pose nullptr: the sensor at rest -- the nominal rays from the origin (the centre sample of a beam: ls_trace_scene's rays),
// nothing to deskew; moving false: no motions -- the walk of ls_trace_scene_sweep
int moving_issue(ls_tracer *tr, hipStream_t s, const float *d_col_pose, const std::vector<const float *> &d_table, bool moving, uint32_t flags,
                 void *d_points32, void *d_hits, uint32_t *d_n_points)
{
    ls_tracer::RayQuery &q = tr->rq;
    const uint32_t nq = shard_rays(tr);
    int rc;
    if ((rc = ensure(tr, q.sweep_rays, (size_t)nq * 32))) return rc;
    if ((rc = ensure(tr, q.sweep_hits, (size_t)nq * 16))) return rc;
    if ((rc = ensure(tr, q.sweep_counts, ls::sweep_block_count(nq)))) return rc;
    const ls::SensorTables tb = tables(tr);
    if (d_col_pose) {
        ls::launch_sweep_rays(s, tb, d_col_pose, q.sweep_rays.p, nullptr);
    } else {
        ls::BeamPattern pat;
        std::memset(static_cast<void *>(&pat), 0, sizeof(pat));
        pat.k[0] = 1.0f;
        ls::launch_beam_rays(s, tb, pat, 1, q.sweep_rays.p);
    }
    if ((rc = query_walk(tr, s, q.sweep_rays.p, nq, q.sweep_hits.p, closest_hits(), moving ? d_table.data() : nullptr))) return rc;
    ls::launch_sweep_pack(s, tb, q.sweep_hits.p, q.sweep_counts.p, d_col_pose, d_col_pose && (flags & LS_SWEEP_DESKEW) != 0, d_points32, d_hits,
                          d_n_points);
    LS_HIP(hipGetLastError());
    return LS_OK;
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
    int rc;
    if ((rc = sweep_check(tr, d_col_pose, n_cols, flags, d_points32, d_hits, d_n_points, capacity, d_rays_out, false))) return rc;
    if ((rc = query_enter(tr, s)) || (rc = sweep_issue(tr, s, d_col_pose, flags, d_points32, d_hits, d_n_points, d_rays_out))) return rc;
    return query_leave(tr, s);
}

// the poses, the outputs and the optional ray records staged in q.io, on the handle's stream; the count comes back first, then as
// many records; of rays_out only the shard's columns are written: V rows of naz records, at their place in the rows of H
int ls_trace_scene_sweep_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols, uint32_t flags, void *points32, void *hits, uint32_t *n_points,
                              uint32_t capacity, void *rays_out)
{
    LS_ENTER(tr);
    DevBuf<uint8_t> &buf = tr->rq.io;
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = sweep_check(tr, col_pose, n_cols, flags, points32, hits, n_points, capacity, rays_out, true))) return rc;
    if ((rc = query_enter(tr, s))) return rc;
    const size_t nq = shard_rays(tr), row_bytes = (size_t)tr->H * 32, first = (size_t)tr->az0 * 32;
    IoPlan io;
    const size_t at_points = io.add(points32 ? nq * 32 : 0), at_hits = io.add(hits ? nq * 16 : 0), at_rays = io.add(rays_out ? tr->V * row_bytes : 0),
                 at_pose = io.add((size_t)n_cols * 48), at_n = io.add(4);
    if ((rc = ensure(tr, buf, io.total()))) return rc;
    LS_HIP(hipMemcpyAsync(buf.p + at_pose, col_pose, (size_t)n_cols * 48, hipMemcpyHostToDevice, s));
    if ((rc = sweep_issue(tr, s, reinterpret_cast<const float *>(buf.p + at_pose), flags, points32 ? buf.p + at_points : nullptr,
                          hits ? buf.p + at_hits : nullptr, reinterpret_cast<uint32_t *>(buf.p + at_n), rays_out ? buf.p + at_rays : nullptr)))
        return rc;
    return fetch_counted(tr, buf.p + at_n, nq, "ls_trace_scene_sweep: more points than rays",
                         {{points32, buf.p + at_points, 32},
                          {hits, buf.p + at_hits, 16},
                          {rays_out ? static_cast<uint8_t *>(rays_out) + first : nullptr, buf.p + at_rays + first, (size_t)tr->naz * 32, tr->V, row_bytes}},
                         n_points);
}

int ls_trace_scene_beams(ls_tracer *tr, void *hip_stream, const ls_beam_model *model, void *d_points32, void *d_hits, uint32_t *d_echo,
                         uint32_t *d_n_points, uint32_t capacity)
{
    LS_ENTER_CHECKED(tr, beams_check(tr, model, d_points32, d_hits, d_echo, d_n_points, capacity, false));
    const hipStream_t s = stream_of(tr, hip_stream);
    int rc;
    if ((rc = query_enter(tr, s)) || (rc = beams_issue(tr, s, model, d_points32, d_hits, d_echo, d_n_points, capacity))) return rc;
    return query_leave(tr, s);
}

// the outputs staged in q.io, on the handle's stream; the count comes back first, then as many records
int ls_trace_scene_beams_host(ls_tracer *tr, const ls_beam_model *model, void *points32, void *hits, uint32_t *echo, uint32_t *n_points,
                              uint32_t capacity)
{
    LS_ENTER_CHECKED(tr, beams_check(tr, model, points32, hits, echo, n_points, capacity, true));
    DevBuf<uint8_t> &buf = tr->rq.io;
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    const size_t cap = (size_t)__builtin_popcount(model->returns) * shard_rays(tr);   // what the beams can give: <= 3 * 2^27
    IoPlan io;
    const size_t at_points = io.add(points32 ? cap * 32 : 0), at_hits = io.add(hits ? cap * 16 : 0), at_echo = io.add(echo ? cap * 4 : 0), at_n = io.add(4);
    if ((rc = ensure(tr, buf, io.total()))) return rc;
    if ((rc = beams_issue(tr, s, model, points32 ? buf.p + at_points : nullptr, hits ? buf.p + at_hits : nullptr,
                          echo ? reinterpret_cast<uint32_t *>(buf.p + at_echo) : nullptr, reinterpret_cast<uint32_t *>(buf.p + at_n), (uint32_t)cap)))
        return rc;
    return fetch_counted(tr, buf.p + at_n, cap, "ls_trace_scene_beams: more returns than the beams can give",
                         {{points32, buf.p + at_points, 32}, {hits, buf.p + at_hits, 16}, {echo, buf.p + at_echo, 4}}, n_points);
}

int ls_trace_scene_beams_sweep(ls_tracer *tr, void *hip_stream, const ls_beam_model *model, const uint32_t *weights, uint32_t min_weight,
                               const float *d_col_pose, uint32_t n_cols, uint32_t flags, void *d_points32, void *d_hits, uint32_t *d_echo,
                               uint32_t *d_n_points, uint32_t capacity)
{
    LS_ENTER_CHECKED(tr, beams_sweep_check(tr, model, weights, d_col_pose, n_cols, flags, d_points32, d_hits, d_echo, d_n_points, capacity, false));
    const hipStream_t s = stream_of(tr, hip_stream);
    int rc;
    if ((rc = query_enter(tr, s)) ||
        (rc = beams_sweep_issue(tr, s, model, weights, min_weight, d_col_pose, flags, d_points32, d_hits, d_echo, d_n_points, capacity)))
        return rc;
    return query_leave(tr, s);
}

// the poses and the outputs staged in q.io, on the handle's stream; the count comes back first, then as many records
int ls_trace_scene_beams_sweep_host(ls_tracer *tr, const ls_beam_model *model, const uint32_t *weights, uint32_t min_weight, const float *col_pose,
                                    uint32_t n_cols, uint32_t flags, void *points32, void *hits, uint32_t *echo, uint32_t *n_points, uint32_t capacity)
{
    LS_ENTER_CHECKED(tr, beams_sweep_check(tr, model, weights, col_pose, n_cols, flags, points32, hits, echo, n_points, capacity, true));
    DevBuf<uint8_t> &buf = tr->rq.io;
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    const size_t cap = (size_t)__builtin_popcount(model->returns) * shard_rays(tr);   // what the beams can give: <= 3 * 2^27
    IoPlan io;
    const size_t at_points = io.add(points32 ? cap * 32 : 0), at_hits = io.add(hits ? cap * 16 : 0), at_pose = io.add((size_t)n_cols * 48),
                 at_echo = io.add(echo ? cap * 4 : 0), at_n = io.add(4);
    if ((rc = ensure(tr, buf, io.total()))) return rc;
    if (col_pose) LS_HIP(hipMemcpyAsync(buf.p + at_pose, col_pose, (size_t)n_cols * 48, hipMemcpyHostToDevice, s));
    if ((rc = beams_sweep_issue(tr, s, model, weights, min_weight, col_pose ? reinterpret_cast<const float *>(buf.p + at_pose) : nullptr, flags,
                                points32 ? buf.p + at_points : nullptr, hits ? buf.p + at_hits : nullptr,
                                echo ? reinterpret_cast<uint32_t *>(buf.p + at_echo) : nullptr, reinterpret_cast<uint32_t *>(buf.p + at_n), (uint32_t)cap)))
        return rc;
    return fetch_counted(tr, buf.p + at_n, cap, "ls_trace_scene_beams_sweep: more returns than the beams can give",
                         {{points32, buf.p + at_points, 32}, {hits, buf.p + at_hits, 16}, {echo, buf.p + at_echo, 4}}, n_points);
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

int ls_trace_scene_sweep_moving(ls_tracer *tr, void *hip_stream, const float *d_col_pose, uint32_t n_cols, const ls_geometry_motion *motions,
                                uint32_t n_motions, uint32_t flags, void *d_points32, void *d_hits, uint32_t *d_n_points, uint32_t capacity)
{
    std::vector<const float *> table;
    LS_ENTER_CHECKED(tr, moving_check(tr, d_col_pose, n_cols, motions, n_motions, flags, d_points32, d_hits, d_n_points, capacity, false, table));
    const hipStream_t s = stream_of(tr, hip_stream);
    int rc;
    if ((rc = query_enter(tr, s)) || (rc = moving_issue(tr, s, d_col_pose, table, n_motions != 0, flags, d_points32, d_hits, d_n_points))) return rc;
    return query_leave(tr, s);
}

// the poses, the motion tables and the outputs staged in q.io, on the handle's stream; the count comes back first, then as many records
int ls_trace_scene_sweep_moving_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols, const ls_geometry_motion *motions, uint32_t n_motions,
                                     uint32_t flags, void *points32, void *hits, uint32_t *n_points, uint32_t capacity)
{
    std::vector<const float *> table;
    LS_ENTER_CHECKED(tr, moving_check(tr, col_pose, n_cols, motions, n_motions, flags, points32, hits, n_points, capacity, true, table));
    DevBuf<uint8_t> &buf = tr->rq.io;
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    const size_t nq = shard_rays(tr), table_bytes = (size_t)tr->H * 48;
    IoPlan io;
    const size_t at_points = io.add(points32 ? nq * 32 : 0), at_hits = io.add(hits ? nq * 16 : 0), at_pose = io.add((size_t)n_cols * 48),
                 at_motion = io.add((size_t)n_motions * table_bytes), at_n = io.add(4);   // (48 H: every table starts 16-byte aligned)
    if ((rc = ensure(tr, buf, io.total()))) return rc;
    if (col_pose) LS_HIP(hipMemcpyAsync(buf.p + at_pose, col_pose, (size_t)n_cols * 48, hipMemcpyHostToDevice, s));
    size_t staged = 0;
    for (const float *&t : table) {
        if (!t) continue;
        uint8_t *dst = buf.p + at_motion + staged++ * table_bytes;
        LS_HIP(hipMemcpyAsync(dst, t, table_bytes, hipMemcpyHostToDevice, s));
        t = reinterpret_cast<const float *>(dst);
    }
    if ((rc = moving_issue(tr, s, col_pose ? reinterpret_cast<const float *>(buf.p + at_pose) : nullptr, table, n_motions != 0, flags,
                           points32 ? buf.p + at_points : nullptr, hits ? buf.p + at_hits : nullptr, reinterpret_cast<uint32_t *>(buf.p + at_n))))
        return rc;
    return fetch_counted(tr, buf.p + at_n, nq, "ls_trace_scene_sweep_moving: more points than rays",
                         {{points32, buf.p + at_points, 32}, {hits, buf.p + at_hits, 16}}, n_points);
}

}  // extern "C"
