// ls_surface_sample.hip -- the kernels of ls_sample_surface (include/lidarshooter_hip.h): points drawn from the
// surface of the committed scene in proportion to area, each with its unit normal, its owner and its barycentrics.
//
//   k_surface_area         one lane per triangle of the scene's flat index: its vertices (ls_scene_tris.h); the area's bits to
//                          area[1 + i], and their maximum -- reduced in the wave, one atomicMax per wave -- to area[0];
//   k_surface_block_sums   the weights (from the areas and the maximum) of every 256 triangles summed, and how many are > 0;
//   k_surface_prefix       every workgroup adds up the sums of the workgroups before its own (ls_pack.h's style: no workgroup waits
//                          for another, no atomic append), scans its own 256 weights and writes P; the last one writes P[n_tris]
//                          and the call's info;
//   k_surface_sample       one lane per sample: Philox, T, the bisection over P -- plain, or its first ten levels over 1025 evenly
//                          spaced entries of P staged in LDS --, the triangle's reload, one 48-byte record as three 16-byte stores.
//
// Every weight is an integer and every sum an integer sum: P is the same bytes whatever the order of the waves.  Every loop bound
// comes from a count (n_table, n_tris, the number of workgroups, 32 trips of a bisection) and never from data; every index is
// checked before an address is formed from it.
#include "ls_surface_sample.h"
#include "ls_scene_tris.h"

namespace ls {

namespace {

static_assert(kSurfaceBlock == kBlock, "the scan below is written for four waves");

// Triangle `tri` of geometry ge (in range of the table) in the output frame (scene_tri_vertices).  false: no such geometry or an
// index out of range
__device__ __forceinline__ bool surface_tri_load(const SurfaceSample &d, const AttrGeom &ge, uint32_t tri, float *q)
{
    V3 a, b, c;
    if (!scene_tri_vertices(d.has_xf != 0u, d.xf, ge, tri, a, b, c)) return false;
    q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = b.x; q[4] = b.y; q[5] = b.z; q[6] = c.x; q[7] = c.y; q[8] = c.z;
    return true;
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t x, int off)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), off);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t x, uint32_t off)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, off), hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), off);
    return ((uint64_t)hi << 32) | lo;
}

// x summed over the 64 lanes of the wave, in every lane
__device__ __forceinline__ uint64_t wave_sum64(uint64_t x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += shfl_xor64(x, off);
    return x;
}

__global__ __launch_bounds__(kBlock) void k_surface_area(SurfaceSample d, const AttrGeom *__restrict__ table, uint32_t n_table,
                                                         const uint32_t *__restrict__ tri_first, uint32_t n_tris,
                                                         const uint8_t *__restrict__ select, uint32_t n_select, uint32_t *__restrict__ area)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t bits = 0u;
    if (i < n_tris) {
        const uint32_t gid = scene_geom_of(tri_first, n_table, i);
        const uint32_t tri = i - tri_first[gid];
        const bool selected = gid >= n_select || select[gid] != 0;
        float q[9], n[3];
        if (selected && surface_tri_load(d, table[gid], tri, q)) bits = __float_as_uint(surface_tri_area(q, n));
        area[1u + i] = bits;
    }
    // a >= +0: the bit patterns order as the values do
    uint32_t top = bits;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, off));
    if ((threadIdx.x & 63u) == 0u && top != 0u) atomicMax(&area[0], top);
}

// the weight of triangle i (0 beyond n_tris)
__device__ __forceinline__ uint64_t surface_weight_of(const uint32_t *__restrict__ area, uint32_t n_tris, uint32_t i, int e)
{
    return i < n_tris ? surface_weight(__uint_as_float(area[1u + i]), e) : 0ull;
}

// sums[2 b] = the weights of workgroup b's triangles, sums[2 b + 1] = how many of them are > 0
__global__ __launch_bounds__(kBlock) void k_surface_block_sums(const uint32_t *__restrict__ area, uint32_t n_tris, uint64_t *__restrict__ sums)
{
    __shared__ uint64_t s_sum[kBlock / 64], s_cnt[kBlock / 64];
    const int e = surface_exponent(area[0]);
    const uint64_t w = surface_weight_of(area, n_tris, blockIdx.x * kBlock + threadIdx.x, e);
    const uint64_t total = wave_sum64(w);
    const uint64_t count = (uint64_t)__popcll(__ballot(w != 0ull));
    if ((threadIdx.x & 63u) == 0u) { s_sum[threadIdx.x >> 6] = total; s_cnt[threadIdx.x >> 6] = count; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sums[2 * (size_t)blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        sums[2 * (size_t)blockIdx.x + 1] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    }
}

// P[i] for the workgroup's triangles; the last workgroup: P[n_tris] and the info.  gridDim.x = surface_blocks(n_tris)
__global__ __launch_bounds__(kBlock) void k_surface_prefix(const uint32_t *__restrict__ area, uint32_t n_tris, const uint64_t *__restrict__ sums,
                                                           uint64_t *__restrict__ prefix, void *__restrict__ info)
{
    __shared__ uint64_t s_sum[kBlock / 64], s_cnt[kBlock / 64], s_wave[kBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const bool last = blockIdx.x == gridDim.x - 1u;
    const int e = surface_exponent(area[0]);
    // what the workgroups before this one hold: each lane its share, then the wave, then the four waves
    uint64_t acc = 0ull, cnt = 0ull;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kBlock) {
        acc += sums[2 * (size_t)b];
        if (last) cnt += sums[2 * (size_t)b + 1];
    }
    acc = wave_sum64(acc);
    cnt = wave_sum64(cnt);
    // this workgroup's own: an inclusive scan inside the wave
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint64_t w = surface_weight_of(area, n_tris, i, e);
    uint64_t incl = w;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint64_t below = shfl_up64(incl, off);
        if (lane >= off) incl += below;
    }
    cnt += (uint64_t)__popcll(__ballot(w != 0ull));
    if (lane == 63u) { s_sum[wv] = acc; s_cnt[wv] = cnt; s_wave[wv] = incl; }
    __syncthreads();
    uint64_t base = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    for (uint32_t k = 0; k < wv; ++k) base += s_wave[k];
    if (i < n_tris) prefix[i] = base + (incl - w);
    if (last && threadIdx.x == kBlock - 1) {
        const uint64_t W = base + incl;
        prefix[n_tris] = W;
        if (info) {
            static_cast<uint64_t *>(info)[0] = W;
            static_cast<int32_t *>(info)[2] = e;
            static_cast<uint32_t *>(info)[3] = (uint32_t)((s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]));
        }
    }
}

// TOP: the bisection's first levels run over s_top[k] = P[min(k step, n_tris)], k = 0 .. kSurfaceTop, step = ceil(n_tris /
// kSurfaceTop), staged once per workgroup: ten reads of LDS in place of as many dependent loads from L2.  The triangle found is the
// same: s_top[k] <= T < s_top[k + 1] brackets it as P[lo] <= T < P[hi] does.
template <bool TOP>
__global__ __launch_bounds__(kBlock) void k_surface_sample(SurfaceSample d, const AttrGeom *__restrict__ table, uint32_t n_table,
                                                           const uint32_t *__restrict__ tri_first, uint32_t n_tris,
                                                           const uint64_t *__restrict__ prefix, uint4 *__restrict__ out)
{
    __shared__ uint64_t s_top[TOP ? kSurfaceTop + 1 : 1];
    const uint32_t step = (uint32_t)(((uint64_t)n_tris + kSurfaceTop - 1) / kSurfaceTop);
    if (TOP) {
        for (uint32_t k = threadIdx.x; k <= kSurfaceTop; k += kBlock) {
            const uint64_t at = (uint64_t)k * step;
            s_top[k] = prefix[at < n_tris ? (uint32_t)at : n_tris];
        }
        __syncthreads();
    }
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;   // (64 bits: n may lie within a workgroup of 2^32)
    if (k >= d.n) return;
    const uint64_t W = prefix[n_tris];
    uint4 r0 = make_uint4(0u, 0u, 0u, kInvalid), r1 = make_uint4(0u, 0u, 0u, 0u), r2 = make_uint4(0u, 0u, 0u, 0u);
    if (W != 0ull && n_table != 0u) {
        uint32_t x[4];
        surface_words(d.seed, d.first + k, x);
        const uint64_t T = surface_mulhi(((uint64_t)x[0] << 32) | x[1], W);   // (below W)
        uint32_t lo = 0u, hi = n_tris;
        if (TOP) {
            const uint32_t t = surface_bisect(s_top, 0u, kSurfaceTop, T);
            const uint64_t a = (uint64_t)t * step, b = a + step;
            lo = a < n_tris ? (uint32_t)a : n_tris;
            hi = b < n_tris ? (uint32_t)b : n_tris;
        }
        const uint32_t i = surface_bisect(prefix, lo, hi, T);   // (below n_tris: lo < hi <= n_tris)
        const uint32_t gid = scene_geom_of(tri_first, n_table, i);
        const uint32_t tri = i - tri_first[gid];
        const AttrGeom &ge = table[gid];
        float q[9], n[3], p[3], u, v, w;
        // a triangle that is drawn has a weight, so it loaded and had an area when the weights were made; whatever P holds, no
        // address is formed from an index that fails the check
        if (i < n_tris && tri < (ge.quad ? 2u * ge.n_elems : ge.n_elems) && surface_tri_load(d, ge, tri, q)) {
            surface_tri_area(q, n);
            surface_bary(x[2], x[3], &u, &v, &w);
            surface_point(q, u, v, w, p);
            r0 = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]), gid);
            r1 = make_uint4(__float_as_uint(n[0]), __float_as_uint(n[1]), __float_as_uint(n[2]), ge.quad ? tri >> 1 : tri);
            r2 = make_uint4(__float_as_uint(u), __float_as_uint(v), tri, 1u);
        }
    }
    out[3 * (size_t)k] = r0;
    out[3 * (size_t)k + 1] = r1;
    out[3 * (size_t)k + 2] = r2;
}

}  // namespace

void launch_surface_area(hipStream_t s, const SurfaceSample &d, const AttrGeom *table, uint32_t n_table, const uint32_t *tri_first, uint32_t n_tris,
                         const uint8_t *select, uint32_t n_select, uint32_t *area)
{
    (void)hipMemsetAsync(area, 0, 4, s);
    if (!n_tris || !n_table) return;
    hipLaunchKernelGGL(k_surface_area, dim3(surface_blocks(n_tris)), dim3(kBlock), 0, s, d, table, n_table, tri_first, n_tris, select, n_select,
                       area);
}

void launch_surface_prefix(hipStream_t s, const uint32_t *area, uint32_t n_tris, uint64_t *prefix, void *info)
{
    const uint32_t blocks = surface_blocks(n_tris);
    uint64_t *sums = prefix + (size_t)n_tris + 1;
    hipLaunchKernelGGL(k_surface_block_sums, dim3(blocks), dim3(kBlock), 0, s, area, n_tris, sums);
    hipLaunchKernelGGL(k_surface_prefix, dim3(blocks), dim3(kBlock), 0, s, area, n_tris, sums, prefix, info);
}

void launch_surface_sample(hipStream_t s, const SurfaceSample &d, const AttrGeom *table, uint32_t n_table, const uint32_t *tri_first, uint32_t n_tris,
                           const uint64_t *prefix, bool lds_top, void *samples)
{
    if (!d.n) return;
    const dim3 grid((uint32_t)(((uint64_t)d.n + kBlock - 1) / kBlock));
    if (lds_top)
        hipLaunchKernelGGL(k_surface_sample<true>, grid, dim3(kBlock), 0, s, d, table, n_table, tri_first, n_tris, prefix, static_cast<uint4 *>(samples));
    else
        hipLaunchKernelGGL(k_surface_sample<false>, grid, dim3(kBlock), 0, s, d, table, n_table, tri_first, n_tris, prefix, static_cast<uint4 *>(samples));
}

}  // namespace ls
