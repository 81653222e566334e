// ls_returns.hip -- k_returns_eval + k_returns_pack: sensor returns from hit records (ls_apply_return_model,
// include/lidarshooter_hip.h): intensity from reflectivity, incidence and range, a range gate, an intensity
// floor, Gaussian range noise, random drop-out -- and an ordered compaction of what is kept into 32-byte points and 16-byte
// ls_hit records, with the count, all in device memory.
//
// k_returns_eval, one lane per record: k_hit_attributes' gather and validity test (ls_hit_gather.h: sensor_ray_dir,
// record_on_triangle -- hit -> per-geomID table entry -> three indices -> three vertex records -> the frame's transform ->
// hit_attributes_on_triangle, t bit-equal to hit.t; every index checked before an address is formed from it) -- done ONCE per
// record --, then the model (ls_return_model.h, the
// arithmetic ls_debug_return_model runs on the host) and the point o + t' d.  The evaluated record is parked in a scratch buffer
// of the handle: (ray, geom, prim, t' bits) always -- t' bits = 0 says "lost"; a kept t' is > 0 --, (x, y, z, I) when kept; and
// the workgroup's count of kept records goes to block_counts[blockIdx.x].
// k_returns_pack, one lane per record, the ordered pack (ls_pack.h) with a ballot bit per lane: the offset of a workgroup is
// the sum of the counts of the workgroups before it -- those up to the device count only --, which every workgroup adds up for
// itself; the order of the input is kept for any n; the last workgroup writes *n_out.  Coalesced: 32 bytes read per record, 48
// written per kept one.
// The device count word is read by both kernels; records beyond min(n, *d_count) are never read, and nothing is written past
// record *n_out.
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_hit_attr.h"
#include "ls_hit_gather.h"
#include "ls_pack.h"
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
                    uint32_t v, hh;
                    sensor_ray_dir(tb, h.x, d, &v, &hh);
                }
                uint32_t tri;
                float t, r9[9];
                if (record_on_triangle(g, h, o, d, &tri, &t, r9)) {
                    const float cos_inc = r9[3];
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
    block_count_store((uint32_t)__popcll(__ballot(keep)), block_counts);
}

// ring_div: the raster's H for sensor rays (ring = ray / H), 0 for caller rays (ring 0)
__global__ __launch_bounds__(kBlock) void k_returns_pack(const float4 *__restrict__ park_point, const uint4 *__restrict__ park_hit,
                                                         const uint32_t *__restrict__ block_counts, const uint32_t *__restrict__ d_count,
                                                         uint32_t n, uint32_t ring_div, float4 *__restrict__ points, uint4 *__restrict__ hits_out,
                                                         uint32_t *__restrict__ n_out)
{
    const uint32_t lane = threadIdx.x & 63u;
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
    const uint32_t acc = counts_before(block_counts, min(blockIdx.x, (count + kBlock - 1) / kBlock));
    const bool keep = h.w != 0u;
    const unsigned long long m = __ballot(keep);
    const uint32_t base = pack_wave_base(acc, (uint32_t)__popcll(m), 0u, last, n_out);
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
    const ParkHalves pk = park_halves(park, n);
    hipLaunchKernelGGL(k_returns_eval, grid, dim3(kBlock), 0, s, static_cast<const uint4 *>(hits), d_count, n, static_cast<const float4 *>(rays),
                       n_rays, tb, table, n_table, model, frame_index, refl, n_refl, pk.point, pk.hit, block_counts);
    hipLaunchKernelGGL(k_returns_pack, grid, dim3(kBlock), 0, s, pk.point, pk.hit, block_counts, d_count, n, rays ? 0u : tb.H,
                       static_cast<float4 *>(points32), static_cast<uint4 *>(hits_out), n_out);
}

// k_returns_pack alone, over records another kernel parked in k_returns_eval's layout (k_returns_eval_moving, ls_attr_moving.hip)
void launch_returns_pack(hipStream_t s, const void *park, const uint32_t *block_counts, const uint32_t *d_count, uint32_t n, uint32_t ring_div,
                         void *points32, void *hits_out, uint32_t *n_out)
{
    if (!n) return;
    const ParkHalves pk = park_halves(park, n);
    hipLaunchKernelGGL(k_returns_pack, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pk.point, pk.hit, block_counts, d_count, n, ring_div,
                       static_cast<float4 *>(points32), static_cast<uint4 *>(hits_out), n_out);
}

}  // namespace ls
