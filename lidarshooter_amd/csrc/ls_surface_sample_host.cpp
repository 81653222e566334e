// ls_surface_sample_host.cpp -- ls_sample_surface, its host-memory variant and the descriptor's check: points drawn from the surface
// of the committed scene in proportion to area (ls_surface_sample.hip; the arithmetic is ls_surface_sample.h).  The scene is the
// flat triangle index (scene_tris_prepare; ls_scene_tris.h); the call's place among what the handle issues is that of every query
// (query_enter / query_leave).  No hierarchy is touched and LS_INFO_RAY_QUERY_BUILT is left as it is.
#include "ls_internal.h"
#include "ls_surface_sample.h"

namespace lsi {

namespace {

// k_surface_sample's bisection: 0 the plain one over P in global memory, 1 its first ten levels over 1025 entries of P staged in LDS
// (the same bytes either way).  What ships is what EXPERIMENTS.md E25 says of the two; an EXPERIMENTAL build reads the knob at every
// call, so that tools/surface_sample_cost.py can alternate the forms in one process.
constexpr int kSurfaceLdsTop = 0;

// what the device entry point and the host-memory variant (any alignment) refuse, in this order
int surface_sample_check(ls_tracer *tr, const ls_surface_sample_desc *desc, const float *xf, const uint8_t *select, uint32_t n_select,
                         const void *samples, const void *info, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!desc) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null sample descriptor");
    if (desc->n_samples && !samples) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null samples with n_samples > 0");
    if (n_select && !select) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null select with n_select > 0");
    if (const char *why = ls::surface_sample_args_invalid(*desc, xf)) return fail(tr, LS_ERR_INVALID_ARGUMENT, why);
    if (!host && (misaligned(samples, 16) || misaligned(info, 8)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "samples must be 16-byte aligned, info 8-byte aligned");
    return uncommitted(tr);
}

int surface_sample_issue(ls_tracer *tr, hipStream_t s, const ls::SurfaceSample &d, const uint8_t *d_select, uint32_t n_select, void *d_samples,
                         void *d_info)
{
    const ls_tracer::HitAttr &a = tr->ha;
    int rc;
    uint32_t n_table, n_tris;
    // (a lane per triangle, in 32 bits)
    if ((rc = scene_tris_prepare(tr, s, 0xFFFFFF00ull, "more than 2^32 - 256 triangles", &n_table, &n_tris))) return rc;
    // the maximum's word and an area word per triangle; P[0 .. n_tris] and the workgroups' pairs {sum, count} behind it
    if ((rc = ensure(tr, tr->rq.surface_area, (size_t)n_tris + 1))) return rc;
    if ((rc = ensure(tr, tr->rq.surface_prefix, (size_t)n_tris + 1 + 2 * (size_t)ls::surface_blocks(n_tris)))) return rc;
    uint32_t *area = tr->rq.surface_area.p;
    uint64_t *prefix = tr->rq.surface_prefix.p;
    ls::launch_surface_area(s, d, a.table.dev.p, n_table, a.tri_first.dev.p, n_tris, d_select, n_select, area);
    ls::launch_surface_prefix(s, area, n_tris, prefix, d_info);
    if (tune_int("LS_SURFACE_SETUP_ONLY", 0)) return LS_OK;   // (the cost tool's split: the set-up launches alone)
    ls::launch_surface_sample(s, d, a.table.dev.p, n_table, a.tri_first.dev.p, n_tris, prefix, tune_int("LS_SURFACE_LDS_TOP", kSurfaceLdsTop) != 0,
                              d_samples);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

}  // namespace

}  // namespace lsi

using namespace lsi;

extern "C" {

int ls_surface_sample_check(const ls_surface_sample_desc *desc)
{
    if (!desc) return LS_ERR_INVALID_ARGUMENT;
    return ls::surface_sample_args_invalid(*desc, nullptr) ? LS_ERR_INVALID_ARGUMENT : LS_OK;
}

int ls_sample_surface(ls_tracer *tr, void *hip_stream, const ls_surface_sample_desc *desc, const float *sensor_to_out3x4, const uint8_t *d_select,
                      uint32_t n_select, void *d_samples, void *d_info)
{
    LS_ENTER(tr);
    const hipStream_t s = stream_of(tr, hip_stream);
    if (const int rc = surface_sample_check(tr, desc, sensor_to_out3x4, d_select, n_select, d_samples, d_info, false)) return rc;
    const ls::SurfaceSample d = ls::surface_sample(*desc, sensor_to_out3x4);
    return query_run(tr, s, [&] { return surface_sample_issue(tr, s, d, d_select, n_select, d_samples, d_info); });
}

int ls_sample_surface_host(ls_tracer *tr, const ls_surface_sample_desc *desc, const float *sensor_to_out3x4, const uint8_t *select, uint32_t n_select,
                           void *samples, void *info)
{
    LS_ENTER(tr);
    int rc;
    if ((rc = surface_sample_check(tr, desc, sensor_to_out3x4, select, n_select, samples, info, true))) return rc;
    const hipStream_t s = tr->stream;
    if ((rc = query_enter(tr, s))) return rc;
    Staging st;
    const int p_select = st.in(select, n_select);
    const int p_samples = st.out(samples, desc->n_samples, 48), p_info = st.out(info, 1, 16);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    const ls::SurfaceSample d = ls::surface_sample(*desc, sensor_to_out3x4);
    if ((rc = surface_sample_issue(tr, s, d, io.dev<const uint8_t>(p_select), n_select, io.dev(p_samples), io.dev(p_info)))) return rc;
    return io.fetch(tr);
}

}  // extern "C"
