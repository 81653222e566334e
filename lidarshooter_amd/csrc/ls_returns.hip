// ls_returns.hip -- k_returns_eval + k_returns_pack: sensor returns from hit records (ls_apply_return_model,
// include/lidarshooter_hip.h): intensity from reflectivity, incidence and range, a range gate, an intensity
// floor, Gaussian range noise, random drop-out -- and an ordered compaction of what is kept into 32-byte points and 16-byte
// ls_hit records, with the count, all in device memory.
//
// k_returns_eval, one lane per record: k_hit_attributes' gather and validity test (ls_attr.hip: hit -> per-geomID table entry
// -> three indices -> three vertex records -> the frame's transform -> hit_attributes_on_triangle, t bit-equal to hit.t; every
// index checked before an address is formed from it) -- done ONCE per record --, then the model (ls_return_model.h, the
// arithmetic ls_debug_return_model runs on the host) and the point o + t' d.  The evaluated record is parked in a scratch buffer
// of the handle: (ray, geom, prim, t' bits) always -- t' bits = 0 says "lost"; a kept t' is > 0 --, (x, y, z, I) when kept; and
// the workgroup's count of kept records goes to block_counts[blockIdx.x].
// k_returns_pack, one lane per record, the frame's ordered pack (k_rowcount + k_pack, ls_kernels.hip): the offset of a
// workgroup is the sum of the counts of the workgroups before it, which every workgroup adds up for itself -- no workgroup
// waits for another, the order of the input is kept for any n; the last workgroup writes *n_out.  Coalesced: 32 bytes read
// per record, 48 written per kept one.
// The device count word is read by both kernels; records beyond min(n, *d_count) are never read, and nothing is written past
// record *n_out.
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_hit_attr.h"
#include "ls_return_model.h"

namespace ls {

namespace {

__global__ __launch_bounds__(kBlock) void k_returns_eval(const uint4 *__restrict__ hits, const uint32_t *__restrict__ d_count, uint32_t n,
                                                         const float4 *__restrict__ rays, uint32_t n_rays, SensorTables tb,
                                                         const AttrGeom *__restrict__ table, uint32_t n_table, ls_return_model model,
                                                         uint32_t frame_index, const float *__restrict__ refl, uint32_t n_refl,
                                                         float4 *__restrict__ park_point, uint4 *__restrict__ park_hit,
                                                         uint32_t *__restrict__ block_counts)
{
    __shared__ uint32_t s_cnt[kBlock / 64];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t count = d_count ? min(n, *d_count) : n;
    bool keep = false;
    if (i < count) {
        const uint4 h = hits[i];   // (ray, geom, prim, t bits)
        const uint32_t ray_bound = rays ? n_rays : tb.V * tb.H;
        float tp = 0.f, I = 0.f, px = 0.f, py = 0.f, pz = 0.f;
        if (h.x < ray_bound && h.y < n_table) {
            const AttrGeom &g = table[h.y];
            if (g.verts && h.z < g.n_elems) {
                const float rho = refl && h.y < n_refl ? refl[h.y] : 1.0f;
                float o[3] = {0.f, 0.f, 0.f}, d[3];
                if (rays) {
                    const float4 r0 = rays[2 * (size_t)h.x], r1 = rays[2 * (size_t)h.x + 1];
                    o[0] = r0.x; o[1] = r0.y; o[2] = r0.z;
                    d[0] = r1.x; d[1] = r1.y; d[2] = r1.z;
                } else {
                    // LidarDevice.cpp:310-316: d = (sin(theta)cos(phi), sin(theta)sin(phi), cos(theta)), the products the trace kernels form
                    const uint32_t v = h.x / tb.H, hh = h.x - v * tb.H;
                    const float st = tb.sin_theta[v];
                    const float2 cs = tb.cs_phi[hh];
                    d[0] = st * cs.x; d[1] = st * cs.y; d[2] = tb.cos_theta[v];
                }
                const uint32_t halves = g.quad ? 2u : 1u;
                bool valid = false;
                float cos_inc = 0.f;
                for (uint32_t c = 0; c < halves && !valid; ++c) {
                    const uint32_t k = g.quad ? 2u * h.z + c : h.z;
                    const uint32_t *ix = g.idx + 3 * (size_t)k;
                    const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
                    if (i0 >= g.n_verts || i1 >= g.n_verts || i2 >= g.n_verts) continue;
                    const V3 a = xform_vertex(g.m, g.verts + (size_t)i0 * g.stride);
                    const V3 b = xform_vertex(g.m, g.verts + (size_t)i1 * g.stride);
                    const V3 cc = xform_vertex(g.m, g.verts + (size_t)i2 * g.stride);
                    const float v0[3] = {a.x, a.y, a.z}, v1[3] = {b.x, b.y, b.z}, v2[3] = {cc.x, cc.y, cc.z};
                    float t, r9[9];
                    if (hit_attributes_on_triangle(o, d, v0, v1, v2, &t, r9) && __float_as_uint(t) == h.w) {
                        cos_inc = r9[3];
                        valid = true;
                    }
                }
                if (valid) {
                    const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
                    keep = return_model_eval(model, h.x, frame_index, __uint_as_float(h.w), len, cos_inc, rho, &tp, &I);
                    if (rays) {
                        px = o[0] + tp * d[0]; py = o[1] + tp * d[1]; pz = o[2] + tp * d[2];
                    } else {   // a sensor ray: xyz = t' * dir with no sum, the bits of k_pack (EmbreeTracer.cpp:341-345)
                        px = tp * d[0]; py = tp * d[1]; pz = tp * d[2];
                    }
                }
            }
        }
        park_hit[i] = make_uint4(h.x, h.y, h.z, keep ? __float_as_uint(tp) : 0u);
        if (keep) park_point[i] = make_float4(px, py, pz, I);
    }
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// ring_div: the raster's H for sensor rays (ring = ray / H), 0 for caller rays (ring 0)
__global__ __launch_bounds__(kBlock) void k_returns_pack(const float4 *__restrict__ park_point, const uint4 *__restrict__ park_hit,
                                                         const uint32_t *__restrict__ block_counts, const uint32_t *__restrict__ d_count,
                                                         uint32_t n, uint32_t ring_div, float4 *__restrict__ points, uint4 *__restrict__ hits_out,
                                                         uint32_t *__restrict__ n_out)
{
    __shared__ uint32_t s_part[kBlock / 64];
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t count = d_count ? min(n, *d_count) : n;
    const bool last = blockIdx.x == gridDim.x - 1;
    if (blockIdx.x * kBlock >= count && !last) return;   // (the whole workgroup: nothing of it is kept, and *n_out is not its to write)
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    // both parked halves requested up front, next to the counts: one memory round trip (a lost record's point half was
    // never written: whatever the scratch holds there is loaded and dropped)
    uint4 h = make_uint4(0u, 0u, 0u, 0u);
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < count) { h = park_hit[i]; p = park_point[i]; }
    // the counts of the workgroups before this one (those beyond the count hold zeros: not read)
    const uint32_t before = min(blockIdx.x, (count + kBlock - 1) / kBlock);
    uint32_t acc = 0;
    constexpr uint32_t kCountsAhead = 8;
    for (uint32_t r0 = threadIdx.x; r0 < before; r0 += kCountsAhead * kBlock) {
        uint32_t c[kCountsAhead];
#pragma unroll
        for (uint32_t k = 0; k < kCountsAhead; ++k) c[k] = r0 + k * kBlock < before ? block_counts[r0 + k * kBlock] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < kCountsAhead; ++k) acc += c[k];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    const bool keep = h.w != 0u;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) { s_part[w] = acc; s_wave[w] = (uint32_t)__popcll(m); }
    __syncthreads();
    uint32_t base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (uint32_t k = 0; k < w; ++k) base += s_wave[k];
    if (last && threadIdx.x == 0) *n_out = base + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (!keep) return;
    const uint32_t dst = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (points) {
        const uint32_t ring = ring_div ? h.x / ring_div : 0u;
        points[2 * (size_t)dst] = make_float4(p.x, p.y, p.z, 0.0f);
        points[2 * (size_t)dst + 1] = make_float4(p.w, __int_as_float((int)ring), 0.0f, 0.0f);
    }
    if (hits_out) hits_out[dst] = h;
}

}  // namespace

size_t returns_block_count(uint32_t n) { return ((size_t)n + kBlock - 1) / kBlock; }

void launch_returns(hipStream_t s, const void *hits, const uint32_t *d_count, uint32_t n, const void *rays, uint32_t n_rays, const SensorTables &tb,
                    const AttrGeom *table, uint32_t n_table, const ls_return_model &model, uint32_t frame_index, const float *refl,
                    uint32_t n_refl, void *park, uint32_t *block_counts, void *points32, void *hits_out, uint32_t *n_out)
{
    if (!n) return;
    const dim3 grid((n + kBlock - 1) / kBlock);
    float4 *park_point = static_cast<float4 *>(park);
    uint4 *park_hit = reinterpret_cast<uint4 *>(park_point + n);
    hipLaunchKernelGGL(k_returns_eval, grid, dim3(kBlock), 0, s, static_cast<const uint4 *>(hits), d_count, n, static_cast<const float4 *>(rays),
                       n_rays, tb, table, n_table, model, frame_index, refl, n_refl, park_point, park_hit, block_counts);
    hipLaunchKernelGGL(k_returns_pack, grid, dim3(kBlock), 0, s, park_point, park_hit, block_counts, d_count, n, rays ? 0u : tb.H,
                       static_cast<float4 *>(points32), static_cast<uint4 *>(hits_out), n_out);
}

// k_returns_pack alone, over records another kernel parked in k_returns_eval's layout (k_returns_eval_moving, ls_attr_moving.hip)
void launch_returns_pack(hipStream_t s, const void *park, const uint32_t *block_counts, const uint32_t *d_count, uint32_t n, uint32_t ring_div,
                         void *points32, void *hits_out, uint32_t *n_out)
{
    if (!n) return;
    const float4 *park_point = static_cast<const float4 *>(park);
    const uint4 *park_hit = reinterpret_cast<const uint4 *>(park_point + n);
    hipLaunchKernelGGL(k_returns_pack, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, park_point, park_hit, block_counts, d_count, n, ring_div,
                       static_cast<float4 *>(points32), static_cast<uint4 *>(hits_out), n_out);
}

}  // namespace ls
