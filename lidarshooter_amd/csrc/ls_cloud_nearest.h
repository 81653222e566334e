// ls_cloud_nearest.h -- the arithmetic of ls_cloud_nearest (include/lidarshooter_hip.h) that the kernels
// (k_cloud_keys, k_cloud_arrange, k_cloud_nearest: ls_cloud_nearest.hip), the host hooks (ls_debug_cloud_cell, ls_debug_cloud_bucket:
// ls_debug.cpp) and the descriptor's check all compile: ONE float32 sequence per point and per pair, and what ls_cloud_nearest.hip
// gives the host code of the call (ls_cloud_nearest_host.cpp).
//
// Everything float is float32 and every operation rounds once (the library is compiled with -ffp-contract=off); there is no fmaf.
//   1. D = radius * 65536.0f (exact: a power of two), r2 = radius * radius;
//   2. a point takes part iff its three coordinates are finite and each |c| <= D -- cloud points and queries alike, a query after
//      the transform ((m0 x + m1 y) + m2 z) + m3 per row where the call has one;
//   3. a query that does not take part: index 0xFFFFFFFF, dist2 = dist = +inf, flags 2;
//   4. query q, cloud point p_i, both taking part: dx = p.x - q.x, dy, dz likewise; d2 = (dx dx + dy dy) + dz dz; i is a candidate iff
//      d2 <= r2 and, under LS_CLOUD_NEAREST_SKIP_SAME_INDEX, i is not the query's own index;
//   5. the answer is the minimum over the candidates of the 64-bit key (bits(d2) << 32) | i: d2 >= +0, so the bits order as the values
//      do, ties go to the lowest index, and a minimum has no order (ls_scene_distance_grid's key);
//   6. dist = sqrtf(d2), flags 1; no candidate: the record of 3 with flags 0;
//   7. n_cloud == 0: there is no candidate, every query gets the record steps 3 and 6 give it without one.
// The index appears nowhere above: it only has to find every candidate.
//
// THE DOMAIN RULE AND WHAT IT BUYS.  The index is a grid of cells of edge h = radius * 1.015625f (1 + 2^-6), a point's cell per axis
// floorf(c / h).  Step 2 bounds |c| by D = 2^16 radius, so |c / h| < 2^16: the cell is an integer of at most 17 bits, and the ROUNDED
// quotient is within 2^16 * 2^-24 = 2^-8 of the true one -- of a cell, whatever the radius.  Without the rule a coordinate of 10^6
// radii would round its quotient by more than a cell and no finite neighbourhood would be safe.  With it, every pair that passes step 4
// has cells at most 1 apart per axis, so the 27 cells around the query's hold every candidate:
//   * every rounded operation is monotone in its operand, so only the sizes of the errors count, not their signs;
//   * d2 <= r2 in float32 admits |dx| only up to radius (1 + 2^-21): r2 is within 2^-24 of radius^2, d2 is at least dx^2 less three
//     roundings of 2^-24 each (the product and the two sums; dy^2, dz^2 >= 0), the square root halves what these add up to, and dx
//     itself is within 2^-24 of p.x - q.x -- under 2^-22 in all, 2^-21 with room (a dx so small that its square underflows is far
//     inside one cell);
//   * h is within 2^-24 of radius (1 + 2^-6), so the true quotients p.x / h and q.x / h lie at most (1 + 2^-21) / ((1 + 2^-6)
//     (1 - 2^-24)) < 1 - 2^-6.03 apart: 0.98462;
//   * the two rounded quotients lie at most 0.98462 + 2 * 2^-8 = 0.99244 < 1 apart, and two numbers less than 1 apart have floors
//     at most 1 apart.
// The slack of h, 2^-6 / (1 + 2^-6) = 0.01538 of a cell, covers 2 * 2^-8 + 2^-21 = 0.00781: were the argument to need more, h's
// factor would change and the domain rule would not.  tests/test_cloud_nearest_cpu.py holds the claim against this compiled
// sequence (ls_debug_cloud_cell) on adversarial pairs at seven radii.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lidarshooter_hip.h"
#include "ls_kernels.h"

#if defined(__HIPCC__)
#define LS_CN_HD __host__ __device__ __forceinline__
#else
#define LS_CN_HD inline
#endif

namespace ls {

constexpr uint32_t kCloudMaxPoints = 1u << 27;          // n_cloud: the bucket table has at most 2^27 entries, a key fits launch_sort's 30 bits
constexpr uint32_t kCloudMaxQueries = 0xFFFFFF00u;      // n_queries: a lane per query, in 32 bits
constexpr uint32_t kCloudMinLog2 = 10, kCloudMaxLog2 = 27;

// the descriptor as the kernels take it, with the call's transform next to it
struct CloudNearest {
    float radius, D, r2, h;
    uint32_t flags, cloud_stride, query_stride, has_xf;
    float xf[12];   // query -> cloud, row-major 3 x 4 (read only with has_xf)
};

// what the call refuses of a descriptor and a transform (nullptr: none), in the order of the header: the message of an
// LS_ERR_INVALID_ARGUMENT
inline const char *cloud_nearest_args_invalid(const ls_cloud_nearest_desc &d, const float *xf)
{
    if (d.flags & ~LS_CLOUD_NEAREST_SKIP_SAME_INDEX) return "unknown flags";
    if (d.reserved[0] || d.reserved[1] || d.reserved[2] || d.reserved[3]) return "reserved words must be 0";
    if (!isfinite(d.radius) || !(d.radius >= 9.5367431640625e-07f) || !(d.radius <= 1048576.0f)) return "the radius is not in 2^-20 .. 2^20";
    const uint32_t strides[2] = {d.cloud_stride, d.query_stride};
    for (uint32_t s : strides)
        if ((s & 3u) || s < 12u || s > 128u) return "a stride is not a multiple of 4 in 12 .. 128";
    if (xf)
        for (int k = 0; k < 12; ++k)
            if (!isfinite(xf[k])) return "non-finite transform";
    return nullptr;
}

inline CloudNearest cloud_nearest(const ls_cloud_nearest_desc &d, const float *query_to_cloud3x4)
{
    CloudNearest v{};
    v.radius = d.radius;
    v.D = d.radius * 65536.0f;
    v.r2 = d.radius * d.radius;
    v.h = d.radius * 1.015625f;
    v.flags = d.flags; v.cloud_stride = d.cloud_stride; v.query_stride = d.query_stride;
    v.has_xf = query_to_cloud3x4 ? 1u : 0u;
    for (int k = 0; k < 12; ++k) v.xf[k] = query_to_cloud3x4 ? query_to_cloud3x4[k] : 0.0f;
    return v;
}

// the table: 2^k buckets, k the smallest with 2^k >= 2 n_cloud, clamped to 10 .. 27
inline uint32_t cloud_log2_buckets(uint32_t n_cloud)
{
    uint32_t k = kCloudMinLog2;
    while (k < kCloudMaxLog2 && (1ull << k) < 2ull * n_cloud) ++k;
    return k;
}

// step 2's transform of a query
LS_CN_HD void cloud_query_point(const CloudNearest &d, float &x, float &y, float &z)
{
    if (!d.has_xf) return;
    const float *m = d.xf;
    const float tx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const float ty = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const float tz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    x = tx; y = ty; z = tz;
}

// step 2: whether the point takes part (NaN and +-inf fail the comparison)
LS_CN_HD bool cloud_takes_part(float D, float x, float y, float z) { return fabsf(x) <= D && fabsf(y) <= D && fabsf(z) <= D; }

// the cell of a coordinate that takes part: an integer in -65536 .. 65536
LS_CN_HD int32_t cloud_cell(float h, float c) { return (int32_t)floorf(c / h); }

// the bucket of a cell: a fixed integer hash of the three coordinates -- a sum of odd multiples (a linear map modulo 2^32: cells a few
// apart do not meet in it), then a bijective finishing mix of shifts and odd multipliers so that the low bits depend on all of it --,
// masked
LS_CN_HD uint32_t cloud_bucket(int32_t cx, int32_t cy, int32_t cz, uint32_t mask)
{
    uint32_t v = (uint32_t)cx * 0x8DA6B343u + (uint32_t)cy * 0xD8163841u + (uint32_t)cz * 0xCB1AB31Fu;
    v ^= v >> 16;
    v *= 0x7FEB352Du;
    v ^= v >> 15;
    v *= 0x846CA68Bu;
    v ^= v >> 16;
    return v & mask;
}

// steps 4 and 5 for one candidate: (best_d2, best_i) is the key's minimum so far, as two words
LS_CN_HD void cloud_consider(float r2, float qx, float qy, float qz, float px, float py, float pz, uint32_t i, uint32_t &best_d2, uint32_t &best_i)
{
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    uint32_t bits;
    __builtin_memcpy(&bits, &d2, 4);
    if (d2 <= r2 && (bits < best_d2 || (bits == best_d2 && i < best_i))) { best_d2 = bits; best_i = i; }
}

// ---- the launches of ls_cloud_nearest.hip ------------------------------------------------------------------------------------------

// The index of one call, in the handle's scratch.  keys / order: n_cloud words each, the bucket of every point (n_buckets for one that
// does not take part) and the points' indices sorted by it; sorted: n_cloud records (x, y, z, bits(i)) in that order; range:
// n_buckets pairs (begin, end) into `sorted`, (0, 0) for an empty bucket; counter: n_cloud_indexed
struct CloudIndex {
    uint32_t *keys_in, *keys_out, *order;
    uint4 *sorted;
    uint2 *range;
    uint32_t *counter;
    uint32_t log2_buckets;
};

// one lane per cloud point: its key to keys_in; how many take part to *counter and, with info != nullptr, to the info's third word
// (both zero before: the launch clears counter and the info's 16 bytes on s first)
void launch_cloud_keys(hipStream_t s, const CloudNearest &d, const void *cloud, uint32_t n_cloud, const CloudIndex &ix, void *info);
// after the sort: one lane per sorted position (range is cleared on s first)
void launch_cloud_arrange(hipStream_t s, const CloudNearest &d, const void *cloud, uint32_t n_cloud, const CloudIndex &ix);
// one lane per query: one 16-byte record each; n_found and n_query_outside added to info.  count_candidates (an EXPERIMENTAL build
// only): the candidates examined by all queries are added to the info's reserved word
void launch_cloud_nearest(hipStream_t s, const CloudNearest &d, const CloudIndex &ix, uint32_t n_cloud, const void *queries, uint32_t n_queries,
                          void *out, void *info, bool count_candidates);

}  // namespace ls
