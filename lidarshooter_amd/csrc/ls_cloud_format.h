// ls_cloud_format.h -- the record of ls_format_cloud (include/lidarshooter_hip.h) that the kernel (ls_format.hip)
// and the host (ls_debug_format_record, ls_debug.cpp) both compile: ONE operation sequence per output record.
//
//   cloud_split_ray      hit.ray -> (ring, column); a ray that is not of the V x H raster has neither: no table is indexed by it
//   cloud_sources        a 32-byte point, an ls_hit and an echo word -- or the miss cell of a ray -- as the twelve sources LS_FIELD_*
//   cloud_format_record  the sources through the format's fields into point_step bytes: every byte is written, the bytes no field
//                        covers with 0
// Float sources (X, Y, Z, INTENSITY, RANGE, TIME) travel as their bits: FLOAT32 with scale 1 and bias 0 stores them untouched.
// Otherwise g = (f * scale) + bias in float32 (the library is compiled with -ffp-contract=off: no fused multiply-add; scale 1 and
// bias 0: g = f), FLOAT32 / FLOAT64 store g with a NaN made the canonical quiet one, the integers rintf(g) (ties to even) saturated
// to their range in double, a NaN as 0.  Word sources (RING, COLUMN, RAY, GEOM, PRIM, ECHO) store their low bits, or (float)w /
// (double)w.  Little-endian, any byte offset: a field goes out byte by byte.
#pragma once

#include "../../include/lidarshooter_hip.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LS_CLOUD_HD __host__ __device__ __forceinline__
#else
#define LS_CLOUD_HD inline
#endif

namespace ls {

constexpr uint32_t kCloudNaN32 = 0x7FC00000u;
constexpr uint64_t kCloudNaN64 = 0x7FF8000000000000ull;
constexpr uint32_t kCloudNoRecord = 0xFFFFFFFFu;   // the organized map: no record fills this cell

// sensor_msgs::PointField datatypes 1..8: INT8 UINT8 INT16 UINT16 INT32 UINT32 FLOAT32 FLOAT64
LS_CLOUD_HD uint32_t cloud_datatype_bytes(uint32_t dt) { return dt <= 2u ? 1u : dt <= 4u ? 2u : dt <= 7u ? 4u : 8u; }
LS_CLOUD_HD bool cloud_float_source(uint32_t source) { return source >= LS_FIELD_X && source <= LS_FIELD_TIME; }

LS_CLOUD_HD float cloud_as_float(uint32_t bits)
{
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}
LS_CLOUD_HD uint32_t cloud_float_bits(float f)
{
    uint32_t b;
    __builtin_memcpy(&b, &f, 4);
    return b;
}
LS_CLOUD_HD uint64_t cloud_double_bits(double d)
{
    uint64_t b;
    __builtin_memcpy(&b, &d, 8);
    return b;
}

// the twelve sources of one record: float sources as their bits, word sources as they are (a switch, not an array: the fields'
// sources are only known at run time, and an indexed array would live in scratch memory)
struct CloudSources {
    uint32_t x, y, z, intensity, range, time, ring, column, ray, geom, prim, echo;
};

LS_CLOUD_HD uint32_t cloud_source(const CloudSources &s, uint32_t source)
{
    switch (source) {
    case LS_FIELD_X: return s.x;
    case LS_FIELD_Y: return s.y;
    case LS_FIELD_Z: return s.z;
    case LS_FIELD_INTENSITY: return s.intensity;
    case LS_FIELD_RANGE: return s.range;
    case LS_FIELD_TIME: return s.time;
    case LS_FIELD_RING: return s.ring;
    case LS_FIELD_COLUMN: return s.column;
    case LS_FIELD_RAY: return s.ray;
    case LS_FIELD_GEOM: return s.geom;
    case LS_FIELD_PRIM: return s.prim;
    case LS_FIELD_ECHO: return s.echo;
    default: return 0u;
    }
}

// ring = ray / H, column = ray % H; false (and zeros) for a ray that is not of the raster
LS_CLOUD_HD bool cloud_split_ray(uint32_t ray, uint32_t V, uint32_t H, uint32_t *ring, uint32_t *column)
{
    *ring = 0u;
    *column = 0u;
    if (!H || (uint64_t)ray >= (uint64_t)V * H) return false;
    *ring = ray / H;
    *column = ray - *ring * H;
    return true;
}

// point8: the 32-byte point as words (nullptr: the format names none of its fields -- zeros); hit4: the ls_hit as words; miss: the
// record is the miss cell of the ray hit4[0], the other three words are not looked at.  col_time / chan_time: the table entries of
// the ray's column and ring (the caller reads them only for a ray of the raster); a foreign ray has ring, column and time 0.
LS_CLOUD_HD CloudSources cloud_sources(const uint32_t *point8, const uint32_t *hit4, bool miss, uint32_t echo, float col_time, float chan_time,
                                       uint32_t V, uint32_t H)
{
    CloudSources s;
    uint32_t ring, column;
    const bool mine = cloud_split_ray(hit4[0], V, H, &ring, &column);
    s.ring = ring;
    s.column = column;
    s.ray = hit4[0];
    s.time = mine ? cloud_float_bits(col_time + chan_time) : 0u;
    s.x = miss ? kCloudNaN32 : point8 ? point8[0] : 0u;
    s.y = miss ? kCloudNaN32 : point8 ? point8[1] : 0u;
    s.z = miss ? kCloudNaN32 : point8 ? point8[2] : 0u;
    s.intensity = miss ? kCloudNaN32 : point8 ? point8[4] : 0u;
    s.range = miss ? kCloudNaN32 : hit4[3];
    s.geom = miss ? 0xFFFFFFFFu : hit4[1];
    s.prim = miss ? 0xFFFFFFFFu : hit4[2];
    s.echo = miss ? 0u : echo;
    return s;
}

// the bytes one field stores, in the low cloud_datatype_bytes(datatype) bytes of the result
LS_CLOUD_HD uint64_t cloud_field_bits(const ls_cloud_field &fd, uint32_t v)
{
    const uint32_t dt = fd.datatype;
    if (!cloud_float_source(fd.source)) {
        if (dt == 7u) return cloud_float_bits((float)v);
        if (dt == 8u) return cloud_double_bits((double)v);
        return v;
    }
    const bool plain = fd.scale == 1.0f && fd.bias == 0.0f;
    if (plain && dt == 7u) return v;
    const float f = cloud_as_float(v);
    const float g = plain ? f : (f * fd.scale) + fd.bias;
    if (dt == 7u) return g != g ? kCloudNaN32 : cloud_float_bits(g);
    if (dt == 8u) return g != g ? kCloudNaN64 : cloud_double_bits((double)g);
    if (g != g) return 0u;
    const bool is_signed = (dt & 1u) != 0u;   // INT8 1, INT16 3, INT32 5
    const uint32_t bits = 8u * cloud_datatype_bytes(dt);
    const double hi = is_signed ? (double)((1ull << (bits - 1u)) - 1ull) : (double)((1ull << bits) - 1ull);
    const double lo = is_signed ? -(double)(1ull << (bits - 1u)) : 0.0;
    double r = (double)rintf(g);
    r = r < lo ? lo : r > hi ? hi : r;
    return (uint64_t)(long long)r;
}

LS_CLOUD_HD void cloud_format_record(const ls_cloud_format &fmt, const CloudSources &s, uint8_t *out)
{
    uint64_t covered_lo = 0ull, covered_hi = 0ull;   // byte b of the record belongs to a field (the fields fit and do not overlap: the check)
    for (uint32_t k = 0; k < fmt.n_fields; ++k) {
        const ls_cloud_field &fd = fmt.fields[k];
        const uint32_t nb = cloud_datatype_bytes(fd.datatype), off = fd.offset;
        const uint64_t m = (1ull << nb) - 1ull;
        if (off < 64u) covered_lo |= m << off;
        if (off >= 64u) covered_hi |= m << (off - 64u);
        else if (off + nb > 64u) covered_hi |= m >> (64u - off);
        uint64_t b = cloud_field_bits(fd, cloud_source(s, fd.source));
        for (uint32_t j = 0; j < nb; ++j, b >>= 8) out[off + j] = (uint8_t)b;
    }
    for (uint32_t b = 0; b < fmt.point_step; ++b)
        if (!(((b < 64u ? covered_lo : covered_hi) >> (b & 63u)) & 1ull)) out[b] = 0;
}

}  // namespace ls
