// ls_labels.hip -- the kernels of ls_object_labels (include/lidarshooter_hip.h): per geomID the number of hit
// records, the range of their t with the rays that hold it, the box of their points, and -- LS_LABEL_FOOTPRINT -- the number of rays
// that hit the geometry taken alone.
//
//   k_label_init       the accumulators (LabelAcc, ls_labels.h) to the identity of their reductions;
//   k_label_reduce     one lane per hit record; a wave reduces its records per geometry before anything goes to memory;
//   k_label_footprint  k_occluded_rays' walk (ls_rays.hip), which here goes on into the next geometry after a hit;
//   k_label_finish     the accumulators decoded into the 64-byte records, the empty values where nothing counted.
//
// Every accumulated value is an integer sum, an integer minimum or an integer maximum: the records are the same bits whatever the order
// of the hit records and whatever the order in which waves arrive.
#include "ls_labels.h"
#include "ls_device.h"
#include "ls_hit_gather.h"

namespace ls {

namespace {

// ---- the reduction over records ---------------------------------------------------------------------------------------------------

constexpr uint32_t kLabelChunks = 8;   // 64-record chunks a wave takes, one after the other, before it sends what it still holds

// a float as an unsigned key of the same order, negative values and -0 < +0 included (+inf is 0xFF800000, -inf 0x007FFFFF)
__device__ __forceinline__ uint32_t label_key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t label_unkey(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// what a wave holds of one geometry: the same values in every lane
struct LabelPart {
    uint32_t n, lo0, lo1, lo2, hi0, hi1, hi2;
    unsigned long long kmin, kmax;
};

__device__ __forceinline__ void label_merge(LabelPart &a, const LabelPart &b)
{
    a.n += b.n;
    a.lo0 = min(a.lo0, b.lo0); a.lo1 = min(a.lo1, b.lo1); a.lo2 = min(a.lo2, b.lo2);
    a.hi0 = max(a.hi0, b.hi0); a.hi1 = max(a.hi1, b.hi1); a.hi2 = max(a.hi2, b.hi2);
    a.kmin = min(a.kmin, b.kmin);
    a.kmax = max(a.kmax, b.kmax);
}

// One lane sends a part to its geometry's accumulator.  The count always goes; a minimum (maximum) goes only when it is below (above)
// the value read just before: the stored values only fall (rise), so a value read earlier bounds the present one from above (below)
// and an atomic that is left out could not have changed anything.  After the first waves of a large mesh have set its box, the
// later ones send one atomic, not nine, to that line.
__device__ __forceinline__ void label_flush(LabelAcc *a, const LabelPart &p)
{
    atomicAdd(&a->n_hits, p.n);
    const uint32_t l0 = __hip_atomic_load(&a->lo[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t l1 = __hip_atomic_load(&a->lo[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t l2 = __hip_atomic_load(&a->lo[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t h0 = __hip_atomic_load(&a->hi[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t h1 = __hip_atomic_load(&a->hi[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t h2 = __hip_atomic_load(&a->hi[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long kn = __hip_atomic_load(&a->t_ray_min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long kx = __hip_atomic_load(&a->t_ray_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p.lo0 < l0) atomicMin(&a->lo[0], p.lo0);
    if (p.lo1 < l1) atomicMin(&a->lo[1], p.lo1);
    if (p.lo2 < l2) atomicMin(&a->lo[2], p.lo2);
    if (p.hi0 > h0) atomicMax(&a->hi[0], p.hi0);
    if (p.hi1 > h1) atomicMax(&a->hi[1], p.hi1);
    if (p.hi2 > h2) atomicMax(&a->hi[2], p.hi2);
    if (p.kmin < kn) atomicMin(&a->t_ray_min, p.kmin);
    if (p.kmax > kx) atomicMax(&a->t_ray_max, p.kmax);
}

__global__ __launch_bounds__(kBlock) void k_label_init(LabelAcc *__restrict__ acc, uint32_t n_labels)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_labels) return;
    uint4 *dst = reinterpret_cast<uint4 *>(acc + i);
    dst[0] = make_uint4(0u, 0u, kInvalid, kInvalid);     // n_hits, n_alone, t_ray_min = ~0
    dst[1] = make_uint4(0u, 0u, kInvalid, kInvalid);     // t_ray_max = 0, lo[0], lo[1]
    dst[2] = make_uint4(kInvalid, 0u, 0u, 0u);           // lo[2], hi[0 .. 2]
    dst[3] = make_uint4(0u, 0u, 0u, 0u);
}

// A record counts when its geomID is below n_labels and names a geometry of the table, its element and its ray are in range, its t
// is finite and >= 0 and, for a caller ray, the ray is one k_trace_rays walks.  The triangle is NOT tested: this is a reduction, not
// the validity gather (k_hit_attributes).  Every index is checked before an address is formed from it.
// Frame hits come in ray order: a wave mostly holds one to three geometries.  It takes the geomID of its first pending lane, reduces
// the lanes that share it over the wave (six box keys and the two (t, ray) keys by butterfly, the count by a ballot), and goes on
// until no lane is pending; a part whose geometry is the one the wave already holds is merged in registers, another one sends the
// held part to memory first.  After kLabelChunks chunks the held part goes out.
__global__ __launch_bounds__(kBlock) void k_label_reduce(const uint4 *__restrict__ hits, const uint32_t *__restrict__ d_count, uint32_t n,
                                                         const float4 *__restrict__ rays, uint32_t n_rays, uint32_t own_rays, SensorTables tb,
                                                         const AttrGeom *__restrict__ table, uint32_t n_table, LabelAcc *__restrict__ acc,
                                                         uint32_t n_labels)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = d_count ? min(n, *d_count) : n;
    const uint32_t ray_bound = own_rays ? tb.V * tb.H : n_rays;
    const uint32_t geom_bound = min(n_table, n_labels);
    const unsigned long long first = ((unsigned long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * (64ull * kLabelChunks) + lane;

    // (ray, geom, prim, t bits) of this lane in chunk c; beyond the count: geom = kInvalid, which is below no bound
    auto record = [&](uint32_t c) {
        const unsigned long long i = first + 64ull * c;
        return i < count ? hits[i] : make_uint4(kInvalid, kInvalid, kInvalid, 0u);
    };

    uint32_t held = kInvalid;   // the geometry whose part the wave holds (none yet)
    LabelPart part = {0u, kInvalid, kInvalid, kInvalid, 0u, 0u, 0u, ~0ull, 0ull};
    uint4 ahead = record(0);
#pragma unroll 1
    for (uint32_t c = 0; c < kLabelChunks; ++c) {
        const uint4 hit = ahead;
        if (c + 1 < kLabelChunks) ahead = record(c + 1);   // the next chunk's record travels while this one is reduced
        const float t = __uint_as_float(hit.w);
        bool ok = hit.y < geom_bound && hit.x < ray_bound && t >= 0.0f && t < INFINITY;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (ok) {
            const AttrGeom &g = table[hit.y];
            ok = g.verts != nullptr && hit.z < g.n_elems;
        }
        if (ok) {
            if (own_rays) {   // a sensor ray: t * d with no sum, the bits of the frame's points32
                float d[3];
                uint32_t v, hh;
                sensor_ray_dir(tb, hit.x, d, &v, &hh);
                px = t * d[0]; py = t * d[1]; pz = t * d[2];
            } else {
                const float4 r0 = rays[2 * (size_t)hit.x], r1 = rays[2 * (size_t)hit.x + 1];
                ok = isfinite(r0.x) && isfinite(r0.y) && isfinite(r0.z) && isfinite(r1.x) && isfinite(r1.y) && isfinite(r1.z) &&
                     (r1.x != 0.f || r1.y != 0.f || r1.z != 0.f) && r0.w <= r1.w;
                px = r0.x + t * r1.x; py = r0.y + t * r1.y; pz = r0.z + t * r1.z;
            }
        }
        bool pending = ok;
        unsigned long long todo;
        while ((todo = __ballot(pending)) != 0ull) {
            const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)hit.y, __ffsll((long long)todo) - 1);
            const bool mine = pending && hit.y == g;
            LabelPart p;
            p.n = (uint32_t)__popcll(__ballot(mine));
            p.lo0 = mine ? label_key(px) : kInvalid; p.lo1 = mine ? label_key(py) : kInvalid; p.lo2 = mine ? label_key(pz) : kInvalid;
            p.hi0 = mine ? label_key(px) : 0u; p.hi1 = mine ? label_key(py) : 0u; p.hi2 = mine ? label_key(pz) : 0u;
            p.kmin = mine ? ((unsigned long long)(hit.w & 0x7FFFFFFFu) << 32) | hit.x : ~0ull;    // (t = -0 counts as +0)
            p.kmax = mine ? ((unsigned long long)(hit.w & 0x7FFFFFFFu) << 32) | (~hit.x) : 0ull;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                p.lo0 = min(p.lo0, (uint32_t)__shfl_xor((int)p.lo0, m)); p.lo1 = min(p.lo1, (uint32_t)__shfl_xor((int)p.lo1, m));
                p.lo2 = min(p.lo2, (uint32_t)__shfl_xor((int)p.lo2, m));
                p.hi0 = max(p.hi0, (uint32_t)__shfl_xor((int)p.hi0, m)); p.hi1 = max(p.hi1, (uint32_t)__shfl_xor((int)p.hi1, m));
                p.hi2 = max(p.hi2, (uint32_t)__shfl_xor((int)p.hi2, m));
                p.kmin = min(p.kmin, (unsigned long long)__shfl_xor((long long)p.kmin, m));
                p.kmax = max(p.kmax, (unsigned long long)__shfl_xor((long long)p.kmax, m));
            }
            if (g == held) {
                label_merge(part, p);
            } else {
                if (held != kInvalid && lane == 0) label_flush(acc + held, part);
                held = g;
                part = p;
            }
            pending = pending && !mine;
        }
    }
    if (held != kInvalid && lane == 0) label_flush(acc + held, part);
}

__global__ __launch_bounds__(kBlock) void k_label_finish(const LabelAcc *__restrict__ acc, const AttrGeom *__restrict__ table, uint32_t n_table,
                                                         uint4 *__restrict__ labels, uint32_t n_labels)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_labels) return;
    const LabelAcc a = acc[i];
    const uint32_t present = i < n_table && table[i].verts != nullptr ? 1u : 0u;
    const uint32_t pinf = 0x7F800000u, ninf = 0xFF800000u;
    uint4 *dst = labels + 4 * (size_t)i;
    if (a.n_hits) {
        dst[0] = make_uint4(a.n_hits, a.n_alone, (uint32_t)(a.t_ray_min >> 32), (uint32_t)a.t_ray_min);
        dst[1] = make_uint4((uint32_t)(a.t_ray_max >> 32), ~(uint32_t)a.t_ray_max, label_unkey(a.lo[0]), label_unkey(a.lo[1]));
        dst[2] = make_uint4(label_unkey(a.lo[2]), label_unkey(a.hi[0]), label_unkey(a.hi[1]), label_unkey(a.hi[2]));
    } else {
        dst[0] = make_uint4(0u, a.n_alone, pinf, kInvalid);
        dst[1] = make_uint4(ninf, kInvalid, pinf, pinf);
        dst[2] = make_uint4(pinf, ninf, ninf, ninf);
    }
    dst[3] = make_uint4(present, 0u, 0u, 0u);
}

// ---- the footprint ----------------------------------------------------------------------------------------------------------------

constexpr uint32_t kRaysRefillMin = 56;   // idle lanes of a wave that trigger a refill (k_occluded_rays')
constexpr uint32_t kRaysLeafWait = 16;    // lanes that must stand at a leaf before a wave runs its leaf tests (k_occluded_rays')

__device__ __forceinline__ bool finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// k_occluded_rays' walk -- the same refill, four-wide node step, leaf phase and LDS + spill stack, the same exact test and range --
// asked per geometry: the first triangle of geometry gi that passes ends GEOMETRY gi for the ray, not the ray.  The lane counts the
// hit (an LDS add on the workgroup's counter of gi), drops what its stack still holds -- those references are nodes of gi, and would
// be read as nodes of the next geometry --, and enters geometry gi + 1.  There is no running best: a closer hit elsewhere says nothing
// about whether THIS geometry is hit, so the far clamp of the box test stays tmax all the way and nothing prunes across geometries.
// At the end of the workgroup one lane per geometry adds the non-zero counts to acc[geom_id].n_alone.  A launch carries nothing to
// the next one: with more than kGeomsPerLaunch geometries every launch walks all the rays through its own batch.
__global__ __launch_bounds__(kBlock) void k_label_footprint(const float4 *__restrict__ rays, uint32_t n, uint32_t own_rays, RayBatch batch,
                                                            const WideNode *__restrict__ wide, const TriRecord *__restrict__ records, uint32_t g,
                                                            LabelAcc *__restrict__ acc, uint32_t *__restrict__ counter,
                                                            uint32_t *__restrict__ spill)
{
    __shared__ uint32_t s_stack[kStackLds][kBlock];
    __shared__ uint32_t s_count[kGeomsPerLaunch];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t *my_spill = spill + ((size_t)blockIdx.x * kBlock + tid) * kStackSpill;
    bool drained = false;
    if (tid < (uint32_t)kGeomsPerLaunch) s_count[tid] = 0u;
    __syncthreads();

    bool has = false;
    V3 o = {0.f, 0.f, 0.f}, d = {0.f, 0.f, 1.f};
    float tmin = 0.f, far = INFINITY;   // far = tmax: the box test's clamp
    float ix = 1.f, iy = 1.f, iz = 1.f;
    float cxl = 0.f, cxh = 0.f, cyl = 0.f, cyh = 0.f, czl = 0.f, czh = 0.f;   // -(o_m +- eps) * inv per axis
    uint32_t cur = kInvalid, sp = 0, gi = 0;
    const float4 *rec4 = reinterpret_cast<const float4 *>(records);

    // the ray of this lane in geometry k's mesh space; cur = its root (kInvalid: nothing there)
    auto enter = [&](uint32_t k) {
        const RayGeom &ig = batch.g[k];
        cur = kInvalid;
        if (!ig.n_leaves) return;
        const float dx = (ig.minv[0] * d.x + ig.minv[1] * d.y) + ig.minv[2] * d.z;
        const float dy = (ig.minv[3] * d.x + ig.minv[4] * d.y) + ig.minv[5] * d.z;
        const float dz = (ig.minv[6] * d.x + ig.minv[7] * d.y) + ig.minv[8] * d.z;
        const float ox = ((ig.minv[0] * o.x + ig.minv[1] * o.y) + ig.minv[2] * o.z) + ig.o[0];
        const float oy = ((ig.minv[3] * o.x + ig.minv[4] * o.y) + ig.minv[5] * o.z) + ig.o[1];
        const float oz = ((ig.minv[6] * o.x + ig.minv[7] * o.y) + ig.minv[8] * o.z) + ig.o[2];
        const float eps = ig.eps + ig.eps_o * fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
        ix = safe_inv(dx); iy = safe_inv(dy); iz = safe_inv(dz);
        cxl = -(ox + eps) * ix; cxh = -(ox - eps) * ix;
        cyl = -(oy + eps) * iy; cyh = -(oy - eps) * iy;
        czl = -(oz + eps) * iz; czh = -(oz - eps) * iz;
        cur = ig.n_leaves > 1u ? 0u : kLeafBit;
    };
    // the next geometry of the batch that has something to walk (the stack is empty here, or has just been dropped)
    auto next_geometry = [&]() {
        cur = kInvalid;
        while (cur == kInvalid && ++gi < batch.n) enter(gi);
    };
    // next thing to do for a lane whose current subtree is finished: the stack, else the next geometry, else done
    auto advance = [&]() {
        cur = kInvalid;
        if (sp) { --sp; cur = sp < (uint32_t)kStackLds ? s_stack[sp][tid] : my_spill[sp - kStackLds]; return; }
        next_geometry();
    };

    while (true) {
        unsigned long long act = __ballot(has);
        // refill trips repeat while kRaysRefillMin lanes stay idle: a degenerate ray, or one no geometry lets in, leaves its lane idle
        while (!drained && (uint32_t)__popcll(act) <= 64u - kRaysRefillMin) {
            const unsigned long long idle = ~act;
            const uint32_t nidle = (uint32_t)__popcll(idle);
            const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(counter, nidle);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= n) drained = true;
            const uint32_t sidx = base + rank;
            if (!drained && !has && sidx < n) {
                const float4 r0 = rays[2 * (size_t)sidx], r1 = rays[2 * (size_t)sidx + 1];
                o = {r0.x, r0.y, r0.z};
                d = {r1.x, r1.y, r1.z};
                tmin = own_rays ? 0.f : r0.w;
                far = own_rays ? INFINITY : r1.w;
                sp = 0; gi = 0;
                // a non-finite origin or direction, a zero direction, tmin > tmax or a NaN bound: counted nowhere, nothing walked
                const bool ok = finite3(o.x, o.y, o.z) && finite3(d.x, d.y, d.z) && (d.x != 0.f || d.y != 0.f || d.z != 0.f) && tmin <= far;
                cur = kInvalid;
                if (ok) {
                    enter(0);
                    while (cur == kInvalid && ++gi < batch.n) enter(gi);
                }
                has = cur != kInvalid;
            }
            act = __ballot(has);
        }
        if (act == 0ull) break;
        bool leaf_phase = true;
        // one traversal step of this lane in geometry `ig`: a four-wide node, then the leaves it leads to
        auto step = [&](const RayGeom &ig) {
            const uint32_t at_entry = gi;   // advance() may move the lane on to another geometry: its leaves wait for the next trip
            if (cur != kInvalid && !(cur & kLeafBit)) {
                const float4 *nd = wide[ig.node_first + cur].q;
                const float4 l0 = nd[0], l1 = nd[1], l2 = nd[2], l3 = nd[3], h0 = nd[4], h1 = nd[5], h2 = nd[6], h3 = nd[7];
                auto slab = [&](const float4 &lo, const float4 &hi, float &tn) {
                    const float x1 = fmaf(lo.x, ix, cxl), x2 = fmaf(hi.x, ix, cxh), y1 = fmaf(lo.y, iy, cyl), y2 = fmaf(hi.y, iy, cyh),
                                z1 = fmaf(lo.z, iz, czl), z2 = fmaf(hi.z, iz, czh);
                    tn = fmaxf(fmaxf(fminf(x1, x2), fminf(y1, y2)), fmaxf(fminf(z1, z2), 0.0f));
                    const float tf = fminf(fminf(fmaxf(x1, x2), fmaxf(y1, y2)), fminf(fmaxf(z1, z2), far));
                    // (the far bound gets two ulps: the products above round once each; an empty slot's reference is kInvalid)
                    return tn <= tf * 1.0000003f && __float_as_uint(lo.w) != kInvalid;
                };
                float k0, k1, k2, k3;
                const bool b0 = slab(l0, h0, k0), b1 = slab(l1, h1, k1), b2 = slab(l2, h2, k2), b3 = slab(l3, h3, k3);
                uint32_t r0 = __float_as_uint(l0.w), r1 = __float_as_uint(l1.w), r2 = __float_as_uint(l2.w), r3 = __float_as_uint(l3.w);
                k0 = b0 ? k0 : INFINITY; k1 = b1 ? k1 : INFINITY; k2 = b2 ? k2 : INFINITY; k3 = b3 ? k3 : INFINITY;
                r0 = b0 ? r0 : kInvalid; r1 = b1 ? r1 : kInvalid; r2 = b2 ? r2 : kInvalid; r3 = b3 ? r3 : kInvalid;
                // the nearest hit child comes to the front and is walked on; the other hits are pushed as they stand
                auto cswap = [](float &ka, uint32_t &ra, float &kb, uint32_t &rb) {
                    const bool sw = kb < ka || (ra == kInvalid && rb != kInvalid);
                    const float kt = sw ? kb : ka; kb = sw ? ka : kb; ka = kt;
                    const uint32_t rt = sw ? rb : ra; rb = sw ? ra : rb; ra = rt;
                };
                cswap(k0, r0, k1, r1); cswap(k0, r0, k2, r2); cswap(k0, r0, k3, r3);
                if (r0 == kInvalid) {
                    advance();
                } else {
                    const uint32_t v3 = r3 != kInvalid ? 1u : 0u, v2 = r2 != kInvalid ? 1u : 0u, v1 = r1 != kInvalid ? 1u : 0u;
                    if (sp + 3u <= (uint32_t)kStackLds) {
                        s_stack[sp][tid] = r3;
                        s_stack[sp + v3][tid] = r2;
                        s_stack[sp + v3 + v2][tid] = r1;
                        sp += v3 + v2 + v1;
                    } else {
                        auto push = [&](uint32_t ref) {
                            if (sp < (uint32_t)kStackLds) s_stack[sp][tid] = ref;
                            else if (sp < (uint32_t)(kStackLds + kStackSpill)) my_spill[sp - kStackLds] = ref;
                            ++sp;
                        };
                        if (v3) push(r3);
                        if (v2) push(r2);
                        if (v1) push(r1);
                    }
                    cur = r0;
                }
            }
            while (leaf_phase && cur != kInvalid && (cur & kLeafBit) && gi == at_entry) {
                const uint32_t first = (cur & ~kLeafBit) * g;
                const uint32_t last = min(first + g, ig.n_tris);
                bool hit = false;
                for (uint32_t s = first; s < last; ++s) {
                    const size_t at = 3 * ((size_t)ig.rec_first + s);
                    const float4 r0 = rec4[at], r1 = rec4[at + 1], r2 = rec4[at + 2];
                    V3 v0 = {r0.x, r0.y, r0.z}, v1 = {r1.x, r1.y, r1.z}, v2 = {r2.x, r2.y, r2.z};
                    if (ig.xform == 2) {
                        v0 = xform_vertex_sensor_only(ig.m, reinterpret_cast<const uint8_t *>(&r0));
                        v1 = xform_vertex_sensor_only(ig.m, reinterpret_cast<const uint8_t *>(&r1));
                        v2 = xform_vertex_sensor_only(ig.m, reinterpret_cast<const uint8_t *>(&r2));
                    } else if (ig.xform == 1) {
                        v0 = xform_vertex(ig.m, reinterpret_cast<const uint8_t *>(&r0));
                        v1 = xform_vertex(ig.m, reinterpret_cast<const uint8_t *>(&r1));
                        v2 = xform_vertex(ig.m, reinterpret_cast<const uint8_t *>(&r2));
                    }
                    float t;
                    if (tri_test_org(o, d, v0, sub(v0, v1), sub(v2, v0), t) && tmin <= t && t <= far) { hit = true; break; }
                }
                if (hit) {   // this geometry's answer: its count, its pending references dropped, on to the next geometry
                    atomicAdd(&s_count[at_entry], 1u);
                    sp = 0;
                    next_geometry();
                    break;
                }
                advance();
            }
        };
        // the leaf tests run when enough lanes stand at a leaf (or nobody has a node to go to): a lane at a leaf waits
        {
            const unsigned long long at_leaf = __ballot(has && cur != kInvalid && (cur & kLeafBit));
            const unsigned long long at_node = __ballot(has && cur != kInvalid && !(cur & kLeafBit));
            leaf_phase = (uint32_t)__popcll(at_leaf) >= kRaysLeafWait || at_node == 0ull;
        }
        if (has) {
            if (cur != kInvalid) step(batch.g[gi]);
            if (cur == kInvalid) has = false;
        }
    }
    __syncthreads();
    if (tid < batch.n) {
        const uint32_t c = s_count[tid];
        if (c) atomicAdd(&acc[batch.g[tid].geom_id].n_alone, c);
    }
}

}  // namespace

void launch_label_init(hipStream_t s, LabelAcc *acc, uint32_t n_labels)
{
    if (!n_labels) return;
    hipLaunchKernelGGL(k_label_init, dim3((n_labels + kBlock - 1) / kBlock), dim3(kBlock), 0, s, acc, n_labels);
}

void launch_label_reduce(hipStream_t s, const void *hits, const uint32_t *d_count, uint32_t n, const void *rays, uint32_t n_rays, bool own_rays,
                         const SensorTables &tb, const AttrGeom *table, uint32_t n_table, LabelAcc *acc, uint32_t n_labels)
{
    if (!n || !n_labels) return;
    const uint32_t per_block = kBlock * kLabelChunks;
    hipLaunchKernelGGL(k_label_reduce, dim3((uint32_t)(((unsigned long long)n + per_block - 1) / per_block)), dim3(kBlock), 0, s,
                       static_cast<const uint4 *>(hits), d_count, n, static_cast<const float4 *>(rays), n_rays, own_rays ? 1u : 0u, tb, table,
                       n_table, acc, n_labels);
}

void launch_label_footprint(hipStream_t s, uint32_t grid_blocks, const void *rays, uint32_t n, bool own_rays, const RayBatch &batch,
                            const WideNode *wide, const TriRecord *records, uint32_t leaf_size, LabelAcc *acc, uint32_t *counter, uint32_t *spill)
{
    if (!n || !batch.n) return;
    const uint32_t grid = min(grid_blocks, (n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_label_footprint, dim3(grid), dim3(kBlock), 0, s, static_cast<const float4 *>(rays), n, own_rays ? 1u : 0u, batch, wide,
                       records, leaf_size, acc, counter, spill);
}

void launch_label_finish(hipStream_t s, const LabelAcc *acc, const AttrGeom *table, uint32_t n_table, void *labels, uint32_t n_labels)
{
    if (!n_labels) return;
    hipLaunchKernelGGL(k_label_finish, dim3((n_labels + kBlock - 1) / kBlock), dim3(kBlock), 0, s, acc, table, n_table,
                       static_cast<uint4 *>(labels), n_labels);
}

}  // namespace ls
