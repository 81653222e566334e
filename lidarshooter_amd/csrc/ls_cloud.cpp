// ls_cloud.cpp -- ls_format_cloud: a frame's records as a cloud in a driver's own PointCloud2 record (ls_format.hip), with its
// host-memory variant; the format's check, a format from the config's pointFields, the columns' firing times.  A gather over
// records like those of ls_gather.cpp -- the same place among what the handle issues (query_enter / query_leave, ls_query.cpp),
// LS_INFO_RAY_QUERY_BUILT left as it is -- but no table of the scene: the call needs no commit, only the sensor's raster size.
#include "ls_internal.h"
#include "ls_cloud_format.h"

#include <cmath>

namespace lsi {

namespace {

// what ls_cloud_format_check refuses, in this order (nullptr: the format is fine)
const char *cloud_format_invalid(const ls_cloud_format *f)
{
    if (!f) return "null format";
    if (f->point_step < 1u || f->point_step > LS_CLOUD_MAX_STEP) return "point_step outside 1..LS_CLOUD_MAX_STEP";
    if (f->n_fields < 1u || f->n_fields > LS_CLOUD_MAX_FIELDS) return "field count outside 1..LS_CLOUD_MAX_FIELDS";
    if (f->flags & ~(uint32_t)LS_CLOUD_ORGANIZED) return "unknown format flags";
    if (f->layer > 2u || (f->layer && !(f->flags & LS_CLOUD_ORGANIZED))) return "layer above 2, or a layer without LS_CLOUD_ORGANIZED";
    unsigned long long covered[2] = {0ull, 0ull};
    for (uint32_t k = 0; k < f->n_fields; ++k) {
        const ls_cloud_field &fd = f->fields[k];
        if (fd.source < LS_FIELD_X || fd.source > LS_FIELD_ECHO) return "unknown field source";
        if (fd.datatype < 1u || fd.datatype > 8u) return "unknown field datatype";
        const uint32_t nb = ls::cloud_datatype_bytes(fd.datatype);
        if ((uint32_t)fd.offset + nb > f->point_step) return "a field does not fit inside point_step";
        for (uint32_t b = fd.offset; b < fd.offset + nb; ++b) {
            if ((covered[b >> 6] >> (b & 63u)) & 1ull) return "two fields overlap";
            covered[b >> 6] |= 1ull << (b & 63u);
        }
        if (!std::isfinite(fd.scale) || !std::isfinite(fd.bias)) return "a non-finite scale or bias";
        if (!ls::cloud_float_source(fd.source) && (fd.scale != 1.0f || fd.bias != 0.0f)) return "a word source takes scale 1 and bias 0";
    }
    return nullptr;
}

bool format_names(const ls_cloud_format *f, uint32_t first, uint32_t last)
{
    for (uint32_t k = 0; k < f->n_fields; ++k)
        if (f->fields[k].source >= first && f->fields[k].source <= last) return true;
    return false;
}

// what both entry points refuse, in this order, before anything touches the device (the host variant takes any alignment)
int format_check(ls_tracer *tr, const ls_cloud_format *fmt, const void *points32, const void *hits, const uint32_t *echo, const uint32_t *count,
                 uint32_t n, const float *col_time, const float *chan_time, const void *out, bool host)
{
    if (tr->fg_open) return fail(tr, LS_ERR_INVALID_ARGUMENT, "a frame graph is open");
    if (const char *why = cloud_format_invalid(fmt)) return fail(tr, LS_ERR_INVALID_ARGUMENT, why);
    const bool organized = (fmt->flags & LS_CLOUD_ORGANIZED) != 0;
    if ((n && !hits) || ((n || organized) && !out)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "null hit records or output");
    if (n && !points32 && format_names(fmt, LS_FIELD_X, LS_FIELD_INTENSITY))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "the format names x, y, z or intensity: points are required");
    if (!col_time && format_names(fmt, LS_FIELD_TIME, LS_FIELD_TIME)) return fail(tr, LS_ERR_INVALID_ARGUMENT, "the format names time: column times are required");
    if (!host && (misaligned16(out, points32, hits) || misaligned(echo, 4) || misaligned(count, 4) || misaligned(col_time, 4) || misaligned(chan_time, 4)))
        return fail(tr, LS_ERR_INVALID_ARGUMENT, "output, points and hit records must be 16-byte aligned, the words and the times 4-byte aligned");
    if (n > kMaxQueryRecords) return fail(tr, LS_ERR_OUT_OF_RANGE, "too many hit records in one call");
    return LS_OK;
}

int format_issue(ls_tracer *tr, hipStream_t s, const ls_cloud_format *fmt, const void *d_points32, const void *d_hits, const uint32_t *d_echo,
                 const uint32_t *d_count, uint32_t n, const float *d_col_time, const float *d_chan_time, void *d_out)
{
    const ls::CloudInputs in = {d_points32, d_hits, d_echo, d_count, n, d_col_time, d_chan_time, tr->V, tr->H};
    const uint32_t *map = nullptr;
    if (fmt->flags & LS_CLOUD_ORGANIZED) {
        DevBuf<uint32_t> &m = tr->rq.cloud_map;
        const uint32_t cells = tr->V * tr->H;
        int rc;
        if ((rc = ensure(tr, m, cells))) return rc;
        ls::launch_cloud_map(s, d_hits, d_count, n, fmt->layer, cells, m.p);
        map = m.p;
    }
    ls::launch_format_cloud(s, *fmt, in, map, d_out);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

}  // namespace

}  // namespace lsi

using namespace lsi;

extern "C" {

int ls_format_cloud(ls_tracer *tr, void *hip_stream, const ls_cloud_format *fmt, const void *d_points32, const void *d_hits, const uint32_t *d_echo,
                    const uint32_t *d_count, uint32_t n, const float *d_col_time, const float *d_chan_time, void *d_out)
{
    LS_ENTER_CHECKED(tr, format_check(tr, fmt, d_points32, d_hits, d_echo, d_count, n, d_col_time, d_chan_time, d_out, false));
    if (!n && !(fmt->flags & LS_CLOUD_ORGANIZED)) return LS_OK;
    const hipStream_t s = stream_of(tr, hip_stream);
    return query_run(tr, s, [&] { return format_issue(tr, s, fmt, d_points32, d_hits, d_echo, d_count, n, d_col_time, d_chan_time, d_out); });
}

// records, tables and the cloud staged in q.io, on the handle's stream; returns when out is filled
int ls_format_cloud_host(ls_tracer *tr, const ls_cloud_format *fmt, const void *points32, const void *hits, const uint32_t *echo, uint32_t n,
                         const float *col_time, const float *chan_time, void *out)
{
    LS_ENTER_CHECKED(tr, format_check(tr, fmt, points32, hits, echo, nullptr, n, col_time, chan_time, out, true));
    const bool organized = (fmt->flags & LS_CLOUD_ORGANIZED) != 0;
    if (!n && !organized) return LS_OK;
    const hipStream_t s = tr->stream;
    int rc;
    if ((rc = query_enter(tr, s))) return rc;
    Staging st;
    const int p_hits = st.in(hits, (size_t)n * 16), p_points = st.in(points32, (size_t)n * 32), p_echo = st.in(echo, (size_t)n * 4),
              p_col = st.in(col_time, (size_t)tr->H * 4), p_chan = st.in(chan_time, (size_t)tr->V * 4),
              p_out = st.out(out, organized ? (size_t)tr->V * tr->H : (size_t)n, fmt->point_step);
    Staged io;
    if ((rc = st.commit(tr, s, io))) return rc;
    if ((rc = format_issue(tr, s, fmt, io.dev(p_points), io.dev(p_hits), io.dev<const uint32_t>(p_echo), nullptr, n, io.dev<const float>(p_col),
                           io.dev<const float>(p_chan), io.dev(p_out))))
        return rc;
    return io.fetch(tr);
}

int ls_cloud_format_check(const ls_cloud_format *fmt) { return cloud_format_invalid(fmt) ? LS_ERR_INVALID_ARGUMENT : LS_OK; }

// host only: the names a config's message.pointFields[] may carry, and the sources they stand for
int ls_cloud_format_from_point_fields(const char *const *names, const uint32_t *offsets, const uint8_t *datatypes, const uint32_t *counts,
                                      uint32_t n_fields, uint32_t point_step, ls_cloud_format *out)
{
    static const struct { const char *name; uint8_t source; } kNames[] = {
        {"x", LS_FIELD_X}, {"y", LS_FIELD_Y}, {"z", LS_FIELD_Z}, {"intensity", LS_FIELD_INTENSITY},
        {"ring", LS_FIELD_RING}, {"channel", LS_FIELD_RING},
        {"time", LS_FIELD_TIME}, {"t", LS_FIELD_TIME}, {"timestamp", LS_FIELD_TIME},
        {"range", LS_FIELD_RANGE}, {"distance", LS_FIELD_RANGE},
        {"label", LS_FIELD_GEOM}, {"geom", LS_FIELD_GEOM}, {"prim", LS_FIELD_PRIM}, {"ray", LS_FIELD_RAY}, {"column", LS_FIELD_COLUMN},
        {"echo", LS_FIELD_ECHO}, {"return_type", LS_FIELD_ECHO},
    };
    if (!out || (n_fields && (!names || !offsets || !datatypes || !counts)) || n_fields > LS_CLOUD_MAX_FIELDS) return LS_ERR_INVALID_ARGUMENT;
    ls_cloud_format f;
    std::memset(&f, 0, sizeof(f));
    f.point_step = point_step;
    f.n_fields = n_fields;
    for (uint32_t k = 0; k < n_fields; ++k) {
        if (!names[k]) return LS_ERR_INVALID_ARGUMENT;
        uint8_t source = 0;
        for (const auto &e : kNames)
            if (std::strcmp(names[k], e.name) == 0) source = e.source;
        if (!source || counts[k] != 1u) return LS_ERR_UNSUPPORTED_TYPE;
        if (offsets[k] > 65535u) return LS_ERR_INVALID_ARGUMENT;
        f.fields[k].source = source;
        f.fields[k].datatype = datatypes[k];
        f.fields[k].offset = (uint16_t)offsets[k];
        f.fields[k].scale = 1.0f;
        f.fields[k].bias = 0.0f;
    }
    if (const int rc = ls_cloud_format_check(&f)) return rc;
    *out = f;
    return LS_OK;
}

// host only: tau_h = t0 + h dt in double, one rounding -- twist_table's tau (ls_scan.cpp)
int ls_column_times(double t0, double dt, uint32_t n_cols, float *col_time)
{
    if ((n_cols && !col_time) || !std::isfinite(t0) || !std::isfinite(dt)) return LS_ERR_INVALID_ARGUMENT;
    for (uint32_t h = 0; h < n_cols; ++h) col_time[h] = (float)(t0 + (double)h * dt);
    return LS_OK;
}

}  // extern "C"
