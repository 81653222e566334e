// ls_cloud_nearest.hip -- the kernels of ls_cloud_nearest (include/lidarshooter_hip.h): for each query the nearest
// point of a cloud within a radius.  The definition is brute force (ls_cloud_nearest.h); what runs is a hashed uniform grid over the
// cloud, rebuilt by every call:
//
//   k_cloud_keys      one lane per cloud point: the domain test, the cell, the bucket; (key, i) for the sort -- the key of a point that
//                     does not take part is n_buckets, behind every bucket; how many take part, one atomicAdd per wave;
//   launch_sort       ls_sort.hip's stable three-pass sort of the keys, the values the points' indices;
//   k_cloud_arrange   one lane per sorted position: the point as one 16-byte record (x, y, z, bits(i)) in bucket order -- a bucket is
//                     contiguous memory --, and where the key changes the bucket's begin and its predecessor's end;
//   k_cloud_nearest   one lane per query: the 27 buckets of the cells around its own, 16 bytes per candidate, the minimum of the key
//                     (bits(d2) << 32) | i in two registers, one 16-byte store; the info from ballots, one atomic per wave.
//
// Two cells that hash to one bucket are scanned twice and a bucket holds the points of every cell that hashes to it: a minimum over
// points that are tested by their distance minds neither.  Every loop bound is a count or is clipped to one (a bucket's range to
// n_cloud_indexed <= n_cloud, begin <= end by the loop's own test) and every index is checked before an address is formed from it.
#include "ls_cloud_nearest.h"
#include "ls_device.h"

namespace ls {

namespace {

// x, y, z of record i of an array of `stride` bytes per record (a multiple of 4; the base 4-byte aligned)
__device__ __forceinline__ void cloud_load(const void *base, uint32_t stride, uint64_t i, float &x, float &y, float &z)
{
    const float *p = reinterpret_cast<const float *>(static_cast<const uint8_t *>(base) + i * stride);
    x = p[0]; y = p[1]; z = p[2];
}

__global__ __launch_bounds__(kBlock) void k_cloud_keys(CloudNearest d, const void *__restrict__ cloud, uint32_t n_cloud, uint32_t log2_buckets,
                                                       uint32_t *__restrict__ keys, uint32_t *__restrict__ counter, uint32_t *__restrict__ info)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n_buckets = 1u << log2_buckets;
    bool part = false;
    if (i < n_cloud) {
        float x, y, z;
        cloud_load(cloud, d.cloud_stride, i, x, y, z);
        part = cloud_takes_part(d.D, x, y, z);
        keys[i] = part ? cloud_bucket(cloud_cell(d.h, x), cloud_cell(d.h, y), cloud_cell(d.h, z), n_buckets - 1u) : n_buckets;
    }
    const uint32_t count = (uint32_t)__popcll(__ballot(part));
    if ((threadIdx.x & 63u) == 0u && count) {
        atomicAdd(counter, count);
        if (info) atomicAdd(info + 2, count);
    }
}

__global__ __launch_bounds__(kBlock) void k_cloud_arrange(CloudNearest d, const void *__restrict__ cloud, uint32_t n_cloud, uint32_t log2_buckets,
                                                          const uint32_t *__restrict__ keys, const uint32_t *__restrict__ order,
                                                          uint4 *__restrict__ sorted, uint2 *__restrict__ range)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_cloud) return;
    const uint32_t n_buckets = 1u << log2_buckets;
    const uint32_t key = keys[j], i = order[j];
    const uint32_t prev = j ? keys[j - 1u] : kInvalid;
    uint4 rec = make_uint4(0u, 0u, 0u, kInvalid);
    if (key < n_buckets && i < n_cloud) {
        float x, y, z;
        cloud_load(cloud, d.cloud_stride, i, x, y, z);
        rec = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), i);
    }
    sorted[j] = rec;
    if (key != prev) {
        if (key < n_buckets) range[key].x = j;
        if (j && prev < n_buckets) range[prev].y = j;
    }
    if (j == n_cloud - 1u && key < n_buckets) range[key].y = n_cloud;
}

// cell c of the 27 around (cx, cy, cz): x fastest
__device__ __forceinline__ uint32_t cloud_neighbour(int32_t cx, int32_t cy, int32_t cz, int c, uint32_t mask)
{
    const int oz = c / 9, oy = (c - 9 * oz) / 3, ox = c - 9 * oz - 3 * oy;
    return cloud_bucket(cx + ox - 1, cy + oy - 1, cz + oz - 1, mask);
}

template <bool COUNT>
__global__ __launch_bounds__(kBlock) void k_cloud_nearest(CloudNearest d, const uint4 *__restrict__ sorted, const uint2 *__restrict__ range,
                                                          const uint32_t *__restrict__ counter, uint32_t log2_buckets, uint32_t n_cloud,
                                                          const void *__restrict__ queries, uint32_t n_queries, uint4 *__restrict__ out,
                                                          uint32_t *__restrict__ info)
{
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;   // (64 bits: n_queries may lie within a workgroup of 2^32)
    const bool live = k < n_queries;
    uint32_t best_d2 = 0x7F800000u, best_i = kInvalid, flags = 0u, examined = 0u;
    if (live) {
        float qx, qy, qz;
        cloud_load(queries, d.query_stride, k, qx, qy, qz);
        cloud_query_point(d, qx, qy, qz);
        if (!cloud_takes_part(d.D, qx, qy, qz)) {
            flags = 2u;
        } else if (n_cloud) {
            const uint32_t mask = (1u << log2_buckets) - 1u;
            const uint32_t n_indexed = min(*counter, n_cloud);
            const int32_t cx = cloud_cell(d.h, qx), cy = cloud_cell(d.h, qy), cz = cloud_cell(d.h, qz);
            // (no cloud index is 0xFFFFFFFF: n_cloud <= 2^27)
            const uint32_t own = (d.flags & LS_CLOUD_NEAREST_SKIP_SAME_INDEX) ? (uint32_t)k : kInvalid;
            uint2 next = range[cloud_neighbour(cx, cy, cz, 0, mask)];
            for (int c = 0; c < 27; ++c) {
                const uint2 r = next;
                if (c + 1 < 27) next = range[cloud_neighbour(cx, cy, cz, c + 1, mask)];   // the next bucket's range is on its way during the scan
                const uint32_t e = min(r.y, n_indexed);
                uint32_t j = min(r.x, n_indexed);
                if (COUNT) examined += e > j ? e - j : 0u;
                for (; j + 4u <= e; j += 4u) {   // four 16-byte loads in flight
                    uint4 p[4];
#pragma unroll
                    for (uint32_t u = 0; u < 4u; ++u) p[u] = sorted[j + u];
#pragma unroll
                    for (uint32_t u = 0; u < 4u; ++u)
                        if (p[u].w != own)
                            cloud_consider(d.r2, qx, qy, qz, __uint_as_float(p[u].x), __uint_as_float(p[u].y), __uint_as_float(p[u].z), p[u].w, best_d2, best_i);
                }
                for (; j < e; ++j) {
                    const uint4 p = sorted[j];
                    if (p.w != own) cloud_consider(d.r2, qx, qy, qz, __uint_as_float(p.x), __uint_as_float(p.y), __uint_as_float(p.z), p.w, best_d2, best_i);
                }
            }
            flags = best_i != kInvalid ? 1u : 0u;
        }
        out[k] = make_uint4(best_i, best_d2, __float_as_uint(sqrtf(__uint_as_float(best_d2))), flags);
    }
    if (info) {
        const uint32_t found = (uint32_t)__popcll(__ballot(flags == 1u)), outside = (uint32_t)__popcll(__ballot(flags == 2u));
        if (COUNT) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) examined += (uint32_t)__shfl_xor((int)examined, off);
        }
        if ((threadIdx.x & 63u) == 0u) {
            if (found) atomicAdd(info, found);
            if (outside) atomicAdd(info + 1, outside);
            if (COUNT && examined) atomicAdd(info + 3, examined);
        }
    }
}

inline dim3 cloud_grid(uint32_t n) { return dim3((uint32_t)(((uint64_t)n + kBlock - 1) / kBlock)); }

}  // namespace

void launch_cloud_keys(hipStream_t s, const CloudNearest &d, const void *cloud, uint32_t n_cloud, const CloudIndex &ix, void *info)
{
    (void)hipMemsetAsync(ix.counter, 0, 4, s);
    if (info) (void)hipMemsetAsync(info, 0, 16, s);
    if (!n_cloud) return;
    hipLaunchKernelGGL(k_cloud_keys, cloud_grid(n_cloud), dim3(kBlock), 0, s, d, cloud, n_cloud, ix.log2_buckets, ix.keys_in, ix.counter,
                       static_cast<uint32_t *>(info));
}

void launch_cloud_arrange(hipStream_t s, const CloudNearest &d, const void *cloud, uint32_t n_cloud, const CloudIndex &ix)
{
    if (!n_cloud) return;
    (void)hipMemsetAsync(ix.range, 0, sizeof(uint2) << ix.log2_buckets, s);
    hipLaunchKernelGGL(k_cloud_arrange, cloud_grid(n_cloud), dim3(kBlock), 0, s, d, cloud, n_cloud, ix.log2_buckets, ix.keys_out, ix.order, ix.sorted,
                       ix.range);
}

void launch_cloud_nearest(hipStream_t s, const CloudNearest &d, const CloudIndex &ix, uint32_t n_cloud, const void *queries, uint32_t n_queries,
                          void *out, void *info, bool count_candidates)
{
    if (!n_queries) return;
    (void)count_candidates;
#ifdef LS_EXPERIMENTAL
    if (count_candidates) {
        hipLaunchKernelGGL(k_cloud_nearest<true>, cloud_grid(n_queries), dim3(kBlock), 0, s, d, ix.sorted, ix.range, ix.counter, ix.log2_buckets, n_cloud,
                           queries, n_queries, static_cast<uint4 *>(out), static_cast<uint32_t *>(info));
        return;
    }
#endif
    hipLaunchKernelGGL(k_cloud_nearest<false>, cloud_grid(n_queries), dim3(kBlock), 0, s, d, ix.sorted, ix.range, ix.counter, ix.log2_buckets, n_cloud,
                       queries, n_queries, static_cast<uint4 *>(out), static_cast<uint32_t *>(info));
}

}  // namespace ls
