// ls_moving.hip -- k_trace_rays_moving: the closest-hit walk of ls_trace_scene_sweep_moving (include/lidarshooter_hip.h; DESIGN.md
// 3.3.8), a sibling of k_trace_rays (ls_rays.hip) whose walk it copies the way k_occluded_rays does.
//
// A geometry that has moved rigidly by D = [Q | c] since the frame began is tested where it was committed, with the ray carried
// through D^-1 (ls_motion.h: the arithmetic ls_debug_motion_ray runs on the host): per geometry the lane's ray is just another
// ray record k_trace_rays would accept, so its box test -- eps + eps_o |o|inf of the ray the geometry sees -- and its exact test
// stand as they are.  The differences:
//   * next to the RayBatch the kernel takes one table pointer per geometry of the launch (nullptr: at rest) and the shard's az0
//     and naz: the lane of shard-local ray q reads record h = az0 + q % naz of geometry k's table;
//   * enter(k) reads the lane's 32-byte record again from the ray buffer (only at a change of geometry; the line is hot), forms
//     (o_g, d_g) and keeps them in the registers that hold (o, d) in k_trace_rays -- both rays live at once would cost a wave
//     (EXPERIMENTS.md) --; a non-finite record, or one that gives a zero direction, skips the geometry for that lane alone;
//   * the leaf test runs tri_test_org(o_g, d_g, ...): t is along the direction as given, and a rotation keeps it.
// best, far and the tie-break (t, global triangle id) are shared across geometries as in k_trace_rays; more than kGeomsPerLaunch
// geometries are successive launches that start from the running best in `out`, the table pointers following their geometries.
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_motion.h"

namespace ls {

// the kernel arguments (the two batches, seven pointers and words) must fit the 4 KB the runtime passes by value
static_assert(sizeof(RayBatch) + sizeof(MotionBatch) + 64 <= 4096, "k_trace_rays_moving: kernel arguments above 4 KB");

namespace {

constexpr uint32_t kRaysRefillMin = 56;   // idle lanes of a wave that trigger a refill (k_trace_rays')
constexpr uint32_t kRaysLeafWait = 16;    // lanes that must stand at a leaf before a wave runs its leaf tests (k_trace_rays')

__device__ __forceinline__ bool finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// amdgpu_waves_per_eu(5, 5): the 32 KB of stacks allow five waves per SIMD, 96 registers each; left to itself the allocator takes
// 102 for the twelve floats of a record in enter() and gives a wave away -- told the target, it fits in 93 with no scratch
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(5, 5)))
void k_trace_rays_moving(const float4 *__restrict__ rays, uint32_t n, RayBatch batch, MotionBatch mb, const WideNode *__restrict__ wide,
                         const TriRecord *__restrict__ records, uint32_t g, uint4 *__restrict__ out, uint32_t *__restrict__ counter,
                         uint32_t *__restrict__ spill)
{
    __shared__ uint32_t s_stack[kStackLds][kBlock];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t *my_spill = spill + ((size_t)blockIdx.x * kBlock + tid) * kStackSpill;
    bool drained = false;

    bool has = false;
    V3 o = {0.f, 0.f, 0.f}, d = {0.f, 0.f, 1.f};
    float tmin = 0.f, far = INFINITY, best = INFINITY;   // far = min(best, tmax): the box test's clamp
    float ix = 1.f, iy = 1.f, iz = 1.f;
    float cxl = 0.f, cxh = 0.f, cyl = 0.f, cyh = 0.f, czl = 0.f, czh = 0.f;   // -(o_m +- eps) * inv per axis
    uint32_t bid = kInvalid, bid0 = kInvalid, bg = 0, q = 0, cur = kInvalid, sp = 0, gi = 0;
    const float4 *rec4 = reinterpret_cast<const float4 *>(records);

    // the ray geometry k sees -- the lane's record, read again (o and d hold the previous geometry's), through the inverse of k's
    // motion at the lane's column -- in k's mesh space; cur = its root (kInvalid: nothing there, or a record that hides k)
    auto enter = [&](uint32_t k) {
        const RayGeom &ig = batch.g[k];
        cur = kInvalid;
        if (!ig.n_leaves) return;
        const float4 r0 = rays[2 * (size_t)q], r1 = rays[2 * (size_t)q + 1];
        o = {r0.x, r0.y, r0.z};
        d = {r1.x, r1.y, r1.z};
        if (const float *tab = mb.table[k]) {
            float p[12];
            load_pose(tab, mb.az0 + q % mb.naz, ((uintptr_t)tab & 15u) == 0u, p);
            const float in[8] = {o.x, o.y, o.z, 0.f, d.x, d.y, d.z, 0.f};
            float rg[8];
            motion_ray(p, in, rg);
            if (!motion_ray_usable(rg)) return;
            o = {rg[0], rg[1], rg[2]};
            d = {rg[4], rg[5], rg[6]};
        }
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
    // next thing to do for a lane whose current subtree is finished: the stack, else the next geometry, else done
    auto advance = [&]() {
        cur = kInvalid;
        if (sp) { --sp; cur = sp < (uint32_t)kStackLds ? s_stack[sp][tid] : my_spill[sp - kStackLds]; return; }
        while (cur == kInvalid && ++gi < batch.n) enter(gi);
    };

    while (true) {
        unsigned long long act = __ballot(has);
        if (!drained && (uint32_t)__popcll(act) <= 64u - kRaysRefillMin) {
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
                tmin = r0.w;
                const float tmax = r1.w;
                q = sidx;
                best = INFINITY; bid0 = kInvalid;
                if (!batch.first) {   // a later batch: the running best of the earlier ones, never replaced by an equal t
                    const uint4 prev = out[q];
                    if (prev.y != kInvalid) { best = __uint_as_float(prev.w); bid0 = 0u; }
                }
                bid = bid0; sp = 0; has = true; gi = 0;
                far = fminf(best, tmax);
                // a non-finite origin or direction, a zero direction, tmin > tmax or a NaN bound: a miss, nothing walked
                const bool ok = finite3(o.x, o.y, o.z) && finite3(d.x, d.y, d.z) && (d.x != 0.f || d.y != 0.f || d.z != 0.f) && tmin <= tmax;
                cur = kInvalid;
                if (ok) {
                    enter(0);
                    while (cur == kInvalid && ++gi < batch.n) enter(gi);
                }
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
                for (uint32_t s = first; s < last; ++s) {
                    const size_t at = 3 * ((size_t)ig.rec_first + s);
                    const float4 r0 = rec4[at], r1 = rec4[at + 1], r2 = rec4[at + 2];
                    const uint32_t local = __float_as_uint(r0.w);
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
                    if (tri_test_org(o, d, v0, sub(v0, v1), sub(v2, v0), t) && tmin <= t && t <= far) {
                        const uint32_t id = ig.gid_first + local;
                        if (t < best || (t == best && id < bid)) { best = t; bid = id; bg = gi; far = fminf(far, t); }
                    }
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
            if (cur == kInvalid) {
                if (bid != bid0) {
                    const RayGeom &hg = batch.g[bg];
                    out[q] = make_uint4(q, hg.geom_id, (bid - hg.gid_first) >> hg.prim_shift, __float_as_uint(best));
                } else if (batch.first) {
                    out[q] = make_uint4(q, kInvalid, kInvalid, __float_as_uint(-1.0f));
                }
                has = false;
            }
        }
    }
}

}  // namespace

void launch_trace_rays_moving(hipStream_t s, uint32_t grid_blocks, const void *rays, uint32_t n, const RayBatch &batch, const MotionBatch &mb,
                              const WideNode *wide, const TriRecord *records, uint32_t leaf_size, void *out, uint32_t *counter, uint32_t *spill)
{
    if (!n || !batch.n) return;
    const uint32_t grid = min(grid_blocks, (n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_trace_rays_moving, dim3(grid), dim3(kBlock), 0, s, static_cast<const float4 *>(rays), n, batch, mb, wide, records,
                       leaf_size, static_cast<uint4 *>(out), counter, spill);
}

}  // namespace ls
