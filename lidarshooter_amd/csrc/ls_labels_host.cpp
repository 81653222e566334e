// ls_labels_host.cpp -- ls_object_labels and its host-memory variant: per geomID the count, t range and box of hit records (a reduction,
// ls_labels.hip) and, with LS_LABEL_FOOTPRINT, the rays that hit the geometry taken alone (a walk over the query hierarchies,
// query_footprint in ls_query.cpp).  The records' table is the gathers' (tables_prepare, ls_gather.cpp); the call's place among what
// the handle issues is that of every query (query_enter / query_leave).  Without the flag no hierarchy is touched and
// LS_INFO_RAY_QUERY_BUILT is left as it is.
#include "ls_internal.h"
#include "ls_labels.h"

namespace lsi {

namespace {

// what the device entry point and the host-memory variant (any alignment) refuse, in this order
int labels_check(ls_tracer *tr, uint32_t flags, const void *rays, uint32_t n_rays, const void *hits, const uint32_t *count, uint32_t n,
                 const void *labels, uint32_t n_labels, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (n_labels && !labels) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null label records with n_labels > 0");
    if (n && !hits) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records with n > 0");
    if (flags & ~LS_LABEL_FOOTPRINT) return fail(tr, LS_ERR_INVALID_ARGUMENT, "unknown flags");
    if (!host && (misaligned16(rays, hits, labels) || misaligned(count, 4)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "rays, hit records and label records must be 16-byte aligned, the count 4-byte aligned");
    if (n > kMaxQueryRecords || (rays && n_rays > kMaxQueryRecords)) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records or rays in one call");
    if (n_labels > ls::kMaxLabels) return fail(tr, LS_ERR_OUT_OF_RANGE, "more than 65536 label records");
    return uncommitted(tr);   // (before n = 0: the same answer whatever n)
}

// own_rays: the handle's sensor rays (d_rays is not read); otherwise n_rays caller rays, which may be none
int labels_issue(ls_tracer *tr, hipStream_t s, uint32_t flags, const void *d_rays, uint32_t n_rays, bool own_rays, const void *d_hits,
                 const uint32_t *d_count, uint32_t n, void *d_labels, uint32_t n_labels)
{
    ls_tracer::RayQuery &q = tr->rq;
    int rc;
    if (!n_labels) return LS_OK;   // no record to write, and nothing counts without one
    if ((rc = tables_prepare(tr, s, nullptr))) return rc;
    if ((rc = ensure(tr, q.label_acc, (size_t)n_labels * sizeof(ls::LabelAcc)))) return rc;
    ls::LabelAcc *acc = reinterpret_cast<ls::LabelAcc *>(q.label_acc.p);
    const ls_tracer::HitAttr &a = tr->ha;
    const uint32_t n_table = (uint32_t)a.table.current.size();
    ls::SensorTables tb = tables(tr);
    tb.az0 = 0;   // the full raster whatever the shard: hit.ray is the global ray index
    tb.naz = tb.H;
    ls::launch_label_init(s, acc, n_labels);
    ls::launch_label_reduce(s, d_hits, d_count, n, d_rays, n_rays, own_rays, tb, a.table.dev.p, n_table, acc, n_labels);
    LS_HIP(hipGetLastError());
    if (flags & LS_LABEL_FOOTPRINT) {
        q.last_built = 0;
        const void *walk_rays = d_rays;
        uint32_t n_walk = n_rays;
        if (own_rays) {
            n_walk = tb.V * tb.H;
            if ((rc = ensure(tr, q.label_rays, (size_t)n_walk * 32))) return rc;
            ls::launch_raygen_aos(s, tb, q.label_rays.p, nullptr);
            walk_rays = q.label_rays.p;
        }
        if ((rc = query_footprint(tr, s, walk_rays, n_walk, own_rays, n_labels, acc))) return rc;
    }
    ls::launch_label_finish(s, acc, a.table.dev.p, n_table, d_labels, n_labels);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

}  // namespace

}  // namespace lsi

using namespace lsi;

extern "C" {

int ls_object_labels(ls_tracer *tr, void *hip_stream, uint32_t flags, const void *d_rays, uint32_t n_rays, const void *d_hits,
                     const uint32_t *d_count, uint32_t n, void *d_labels, uint32_t n_labels)
{
    LS_ENTER(tr);
    const hipStream_t s = stream_of(tr, hip_stream);
    if (const int rc = labels_check(tr, flags, d_rays, n_rays, d_hits, d_count, n, d_labels, n_labels, false)) return rc;
    return query_run(tr, s, [&] { return labels_issue(tr, s, flags, d_rays, n_rays, d_rays == nullptr, d_hits, d_count, n, d_labels, n_labels); });
}

int ls_object_labels_host(ls_tracer *tr, uint32_t flags, const void *rays, uint32_t n_rays, const void *hits, uint32_t n, void *labels,
                          uint32_t n_labels)
{
    LS_ENTER(tr);
    int rc;
    if ((rc = labels_check(tr, flags, rays, n_rays, hits, nullptr, n, labels, n_labels, true)) || !n_labels) return rc;
    const hipStream_t s = tr->stream;
    if ((rc = query_enter(tr, s))) return rc;
    Staging st;
    const int p_hits = st.in(hits, (size_t)n * 16), p_rays = st.in(rays, (size_t)n_rays * 32), p_out = st.out(labels, n_labels, 64);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    if ((rc = labels_issue(tr, s, flags, io.dev(p_rays), n_rays, rays == nullptr, io.dev(p_hits), nullptr, n, io.dev(p_out), n_labels))) return rc;
    return io.fetch(tr);
}

}  // extern "C"
