// ls_cloud_nearest_host.cpp -- ls_cloud_nearest, its host-memory variant and the descriptor's check: for each query the nearest point
// of a cloud within a radius (ls_cloud_nearest.hip; the arithmetic is ls_cloud_nearest.h).  The call needs no committed scene: the
// handle gives it the stream, the scratch of its index (ls_tracer::RayQuery), the error text and its place among what the handle issues
// (query_enter / query_leave: the cloud will usually be a frame's output).  No hierarchy is touched and LS_INFO_RAY_QUERY_BUILT is left
// as it is.
#include "ls_internal.h"
#include "ls_cloud_nearest.h"

namespace lsi {

namespace {

// what the device entry point and the host-memory variant (any alignment) refuse, in this order
int cloud_nearest_check(ls_tracer *tr, const ls_cloud_nearest_desc *desc, const float *xf, const void *cloud, uint32_t n_cloud, const void *queries,
                        uint32_t n_queries, const void *out, const void *info, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (!desc) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null descriptor");
    if (n_queries && !out) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null output with n_queries > 0");
    if (n_cloud && !cloud) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null cloud with n_cloud > 0");
    if (n_queries && !queries) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null queries with n_queries > 0");
    if (const char *why = ls::cloud_nearest_args_invalid(*desc, xf)) return fail(tr, LS_ERR_INVALID_ARGUMENT, why);
    if (!host && (misaligned(cloud, 4) || misaligned(queries, 4) || misaligned(out, 16) || misaligned(info, 8)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "cloud and queries must be 4-byte aligned, the output 16-byte, info 8-byte");
    if (n_cloud > ls::kCloudMaxPoints) return fail(tr, LS_ERR_OUT_OF_RANGE, "more than 2^27 cloud points");
    if (n_queries > ls::kCloudMaxQueries) return fail(tr, LS_ERR_OUT_OF_RANGE, "more than 2^32 - 256 queries");
    return LS_OK;
}

int cloud_nearest_issue(ls_tracer *tr, hipStream_t s, const ls::CloudNearest &d, const void *d_cloud, uint32_t n_cloud, const void *d_queries,
                        uint32_t n_queries, void *d_out, void *d_info)
{
    ls_tracer::RayQuery &q = tr->rq;
    int rc;
    ls::CloudIndex ix{};
    ix.log2_buckets = ls::cloud_log2_buckets(n_cloud);
    // three words per point -- its key, the sorted keys, the sorted indices -- and the counter behind them; a 16-byte record per point;
    // a pair per bucket; the sort's own scratch (the query state's: one call at a time uses it)
    if ((rc = ensure(tr, q.cloud_words, 3 * (size_t)n_cloud + 1))) return rc;
    if ((rc = ensure(tr, q.cloud_sorted, (size_t)n_cloud + 1))) return rc;
    if ((rc = ensure(tr, q.cloud_range, (size_t)1 << ix.log2_buckets))) return rc;
    if ((rc = ensure(tr, q.sort_temp, ls::sort_temp_bytes(n_cloud)))) return rc;
    ix.keys_in = q.cloud_words.p;
    ix.keys_out = ix.keys_in + n_cloud;
    ix.order = ix.keys_out + n_cloud;
    ix.counter = ix.order + n_cloud;
    ix.sorted = q.cloud_sorted.p;
    ix.range = q.cloud_range.p;
    ls::launch_cloud_keys(s, d, d_cloud, n_cloud, ix, d_info);
    if (!ls::launch_sort(s, q.sort_temp.p, q.sort_temp.cap, ix.keys_in, ix.keys_out, nullptr, ix.order, n_cloud))
        return fail(tr, LS_ERR_OUT_OF_RANGE, "sort scratch too small");
    ls::launch_cloud_arrange(s, d, d_cloud, n_cloud, ix);
    if (tune_int("LS_CLOUD_BUILD_ONLY", 0)) return LS_OK;   // (the cost tool's split: the index build alone)
    ls::launch_cloud_nearest(s, d, ix, n_cloud, d_queries, n_queries, d_out, d_info, tune_int("LS_CLOUD_COUNT", 0) != 0);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// the bytes n records of `stride` bytes span when only x, y, z of the last one are read
size_t cloud_span(uint32_t n, uint32_t stride) { return n ? ((size_t)n - 1) * stride + 12 : 0; }

}  // namespace

}  // namespace lsi

using namespace lsi;

extern "C" {

int ls_cloud_nearest_check(const ls_cloud_nearest_desc *desc)
{
    if (!desc) return LS_ERR_INVALID_ARGUMENT;
    return ls::cloud_nearest_args_invalid(*desc, nullptr) ? LS_ERR_INVALID_ARGUMENT : LS_OK;
}

int ls_cloud_nearest(ls_tracer *tr, void *hip_stream, const ls_cloud_nearest_desc *desc, const float *query_to_cloud3x4, const void *d_cloud,
                     uint32_t n_cloud, const void *d_queries, uint32_t n_queries, void *d_out, void *d_info)
{
    LS_ENTER(tr);
    const hipStream_t s = stream_of(tr, hip_stream);
    if (const int rc = cloud_nearest_check(tr, desc, query_to_cloud3x4, d_cloud, n_cloud, d_queries, n_queries, d_out, d_info, false)) return rc;
    const ls::CloudNearest d = ls::cloud_nearest(*desc, query_to_cloud3x4);
    return query_run(tr, s, [&] { return cloud_nearest_issue(tr, s, d, d_cloud, n_cloud, d_queries, n_queries, d_out, d_info); });
}

int ls_cloud_nearest_host(ls_tracer *tr, const ls_cloud_nearest_desc *desc, const float *query_to_cloud3x4, const void *cloud, uint32_t n_cloud,
                          const void *queries, uint32_t n_queries, void *out, void *info)
{
    LS_ENTER(tr);
    int rc;
    if ((rc = cloud_nearest_check(tr, desc, query_to_cloud3x4, cloud, n_cloud, queries, n_queries, out, info, true))) return rc;
    const hipStream_t s = tr->stream;
    if ((rc = query_enter(tr, s))) return rc;
    Staging st;
    const int p_cloud = st.in(cloud, cloud_span(n_cloud, desc->cloud_stride)), p_queries = st.in(queries, cloud_span(n_queries, desc->query_stride));
    const int p_out = st.out(out, n_queries, 16), p_info = st.out(info, 1, 16);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    const ls::CloudNearest d = ls::cloud_nearest(*desc, query_to_cloud3x4);
    if ((rc = cloud_nearest_issue(tr, s, d, io.dev(p_cloud), n_cloud, io.dev(p_queries), n_queries, io.dev(p_out), io.dev(p_info)))) return rc;
    return io.fetch(tr);
}

}  // extern "C"
