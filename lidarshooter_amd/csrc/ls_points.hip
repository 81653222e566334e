// ls_points.hip -- k_closest_points: the nearest point of the committed scene's surface to each of n caller-supplied points
// (ls_closest_points, include/lidarshooter_hip.h).
//
// The frame of k_trace_rays (ls_rays.hip) -- persistent waves, wave-ballot refill from one atomic counter on [0, n), a
// per-lane LDS stack of 32-bit references with the global spill, leaf tests postponed until kPointsLeafWait lanes stand at a
// leaf, one launch per batch of kGeomsPerLaunch geometries in ascending geomID -- around a distance-ordered walk:
//   * per four-wide node the squared distance of the query point to each child box, in the hierarchy's own space (mesh space:
//     p_m = minv * p + o), every box widened by E, and scaled into the sensor frame by s2 <= sigma_min^2 of mesh -> sensor;
//   * a child is dropped only when that lower bound is STRICTLY greater than the current bound min(best d2, radius^2): the
//     margins E and s2 (PointMargins, ls_query.cpp: point_margins) make it a lower bound of the float32 d2 the exact test
//     gives for every triangle below the box, so the result is the brute force's bit for bit, ties included;
//   * the four children are sorted nearest first; the nearest is walked on, the others are pushed farthest first.  The stack
//     holds references only (a bound next to each would double the 32 KiB of LDS that sets the occupancy): a node popped
//     after the bound has shrunk costs its fetch, where all its children are dropped.
// The exact test is closest_on_triangle (ls_closest.h, the arithmetic ls_debug_closest_on_triangle runs on the host) on the
// corners through the frame's own transform, obtained as k_trace_rays' leaf test obtains them.
// Output: two 16-byte stores per point -- (qx, qy, qz, dist) and (geom, prim, index, 0).  Between the launches of one query
// the last word carries the running best d2 (dist = sqrtf(d2) does not determine it); the last launch leaves 0 there.
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_closest.h"

namespace ls {

namespace {

constexpr uint32_t kPointsRefillMin = 56;   // idle lanes of a wave that trigger a refill (k_trace_rays')
constexpr uint32_t kPointsLeafWait = 16;    // lanes that must stand at a leaf before a wave runs its leaf tests (k_trace_rays')

__global__ __launch_bounds__(kBlock) void k_closest_points(const float4 *__restrict__ pts, uint32_t n, RayBatch batch, PointMargins pm,
                                                           const WideNode *__restrict__ wide, const TriRecord *__restrict__ records,
                                                           uint32_t g, uint4 *__restrict__ out, uint32_t *__restrict__ counter,
                                                           uint32_t *__restrict__ spill)
{
    __shared__ uint32_t s_stack[kStackLds][kBlock];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t *my_spill = spill + ((size_t)blockIdx.x * kBlock + tid) * kStackSpill;
    bool drained = false;

    bool has = false;
    float px = 0.f, py = 0.f, pz = 0.f, pinf = 0.f;     // the query point (sensor frame) and its largest |coordinate|
    float r2 = 0.f, best = INFINITY, bound = INFINITY;  // bound = min(best, r2): what a box has to beat
    float bqx = 0.f, bqy = 0.f, bqz = 0.f;              // the closest point so far
    float mx = 0.f, my = 0.f, mz = 0.f, E = 0.f, s2 = 1.f;   // the point in the current geometry's space, its box widening and scale
    uint32_t bid = kInvalid, bid0 = kInvalid, bg = 0, q = 0, cur = kInvalid, sp = 0, gi = 0;
    const float4 *rec4 = reinterpret_cast<const float4 *>(records);

    // the point of this lane in geometry k's space; cur = its root (kInvalid: nothing there)
    auto enter = [&](uint32_t k) {
        const RayGeom &ig = batch.g[k];
        cur = kInvalid;
        if (!ig.n_leaves) return;
        mx = ((ig.minv[0] * px + ig.minv[1] * py) + ig.minv[2] * pz) + ig.o[0];
        my = ((ig.minv[3] * px + ig.minv[4] * py) + ig.minv[5] * pz) + ig.o[1];
        mz = ((ig.minv[6] * px + ig.minv[7] * py) + ig.minv[8] * pz) + ig.o[2];
        E = pm.e0[k] + pm.e1[k] * pinf;
        s2 = pm.s2[k];
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
        if (!drained && (uint32_t)__popcll(act) <= 64u - kPointsRefillMin) {
            const unsigned long long idle = ~act;
            const uint32_t nidle = (uint32_t)__popcll(idle);
            const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(counter, nidle);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= n) drained = true;
            const uint32_t sidx = base + rank;
            if (!drained && !has && sidx < n) {
                const float4 r = pts[sidx];
                px = r.x; py = r.y; pz = r.z;
                pinf = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
                r2 = r.w * r.w;
                q = sidx;
                best = INFINITY; bid0 = kInvalid;
                if (!batch.first) {   // a later batch: the running best of the earlier ones, never replaced by an equal d2
                    const uint4 prev = out[2 * (size_t)q + 1];
                    if (prev.x != kInvalid) { best = __uint_as_float(prev.w); bid0 = 0u; }
                }
                bid = bid0; sp = 0; has = true; gi = 0;
                // a non-finite coordinate, a NaN or negative radius: a miss, nothing walked
                const bool ok = isfinite(px) && isfinite(py) && isfinite(pz) && r.w >= 0.0f;
                bound = fminf(best, ok ? r2 : 0.0f);
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
                // lower bound of the sensor-frame d2 of everything below a child; false: the child is dropped
                auto boxd = [&](const float4 &lo, const float4 &hi, float &k) {
                    const float dx = fmaxf(fmaxf(lo.x - mx, mx - hi.x) - E, 0.0f);
                    const float dy = fmaxf(fmaxf(lo.y - my, my - hi.y) - E, 0.0f);
                    const float dz = fmaxf(fmaxf(lo.z - mz, mz - hi.z) - E, 0.0f);
                    k = ((dx * dx + dy * dy) + dz * dz) * s2;
                    k = k != k ? 0.0f : k;   // (a box that is not a number is walked, first)
                    return !(k > bound) && __float_as_uint(lo.w) != kInvalid;   // (an empty slot's reference is kInvalid)
                };
                float k0, k1, k2, k3;
                const bool b0 = boxd(l0, h0, k0), b1 = boxd(l1, h1, k1), b2 = boxd(l2, h2, k2), b3 = boxd(l3, h3, k3);
                uint32_t r0 = __float_as_uint(l0.w), r1 = __float_as_uint(l1.w), r2_ = __float_as_uint(l2.w), r3 = __float_as_uint(l3.w);
                k0 = b0 ? k0 : INFINITY; k1 = b1 ? k1 : INFINITY; k2 = b2 ? k2 : INFINITY; k3 = b3 ? k3 : INFINITY;
                r0 = b0 ? r0 : kInvalid; r1 = b1 ? r1 : kInvalid; r2_ = b2 ? r2_ : kInvalid; r3 = b3 ? r3 : kInvalid;
                // nearest first (a five-comparator network; a dropped child sorts behind every kept one)
                auto cswap = [](float &ka, uint32_t &ra, float &kb, uint32_t &rb) {
                    const bool sw = kb < ka || (ra == kInvalid && rb != kInvalid);
                    const float kt = sw ? kb : ka; kb = sw ? ka : kb; ka = kt;
                    const uint32_t rt = sw ? rb : ra; rb = sw ? ra : rb; ra = rt;
                };
                cswap(k0, r0, k1, r1); cswap(k2, r2_, k3, r3); cswap(k0, r0, k2, r2_); cswap(k1, r1, k3, r3); cswap(k1, r1, k2, r2_);
                if (r0 == kInvalid) {
                    advance();
                } else {
                    const uint32_t v3 = r3 != kInvalid ? 1u : 0u, v2 = r2_ != kInvalid ? 1u : 0u, v1 = r1 != kInvalid ? 1u : 0u;
                    if (sp + 3u <= (uint32_t)kStackLds) {
                        s_stack[sp][tid] = r3;
                        s_stack[sp + v3][tid] = r2_;
                        s_stack[sp + v3 + v2][tid] = r1;
                        sp += v3 + v2 + v1;
                    } else {
                        auto push = [&](uint32_t ref) {
                            if (sp < (uint32_t)kStackLds) s_stack[sp][tid] = ref;
                            else if (sp < (uint32_t)(kStackLds + kStackSpill)) my_spill[sp - kStackLds] = ref;
                            ++sp;
                        };
                        if (v3) push(r3);
                        if (v2) push(r2_);
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
                    const float4 c0 = rec4[at], c1 = rec4[at + 1], c2 = rec4[at + 2];
                    const uint32_t local = __float_as_uint(c0.w);
                    V3 v0 = {c0.x, c0.y, c0.z}, v1 = {c1.x, c1.y, c1.z}, v2 = {c2.x, c2.y, c2.z};
                    if (ig.xform == 2) {
                        v0 = xform_vertex_sensor_only(ig.m, reinterpret_cast<const uint8_t *>(&c0));
                        v1 = xform_vertex_sensor_only(ig.m, reinterpret_cast<const uint8_t *>(&c1));
                        v2 = xform_vertex_sensor_only(ig.m, reinterpret_cast<const uint8_t *>(&c2));
                    } else if (ig.xform == 1) {
                        v0 = xform_vertex(ig.m, reinterpret_cast<const uint8_t *>(&c0));
                        v1 = xform_vertex(ig.m, reinterpret_cast<const uint8_t *>(&c1));
                        v2 = xform_vertex(ig.m, reinterpret_cast<const uint8_t *>(&c2));
                    }
                    const float P[3] = {px, py, pz}, A[3] = {v0.x, v0.y, v0.z}, B[3] = {v1.x, v1.y, v1.z}, C[3] = {v2.x, v2.y, v2.z};
                    float Q[3], d2;
                    closest_on_triangle(P, A, B, C, Q, &d2);
                    if (d2 <= r2 && d2 < INFINITY) {
                        const uint32_t id = ig.gid_first + local;
                        if (d2 < best || (d2 == best && id < bid)) {
                            best = d2; bid = id; bg = gi; bqx = Q[0]; bqy = Q[1]; bqz = Q[2];
                            bound = fminf(bound, d2);
                        }
                    }
                }
                advance();
            }
        };
        // the leaf tests run when enough lanes stand at a leaf (or nobody has a node to go to): a lane at a leaf waits
        {
            const unsigned long long at_leaf = __ballot(has && cur != kInvalid && (cur & kLeafBit));
            const unsigned long long at_node = __ballot(has && cur != kInvalid && !(cur & kLeafBit));
            leaf_phase = (uint32_t)__popcll(at_leaf) >= kPointsLeafWait || at_node == 0ull;
        }
        if (has) {
            if (cur != kInvalid) step(batch.g[gi]);
            if (cur == kInvalid) {
                if (bid != bid0) {
                    const RayGeom &hg = batch.g[bg];
                    out[2 * (size_t)q] = make_uint4(__float_as_uint(bqx), __float_as_uint(bqy), __float_as_uint(bqz), __float_as_uint(sqrtf(best)));
                    out[2 * (size_t)q + 1] = make_uint4(hg.geom_id, (bid - hg.gid_first) >> hg.prim_shift, q, pm.last ? 0u : __float_as_uint(best));
                } else if (batch.first) {
                    out[2 * (size_t)q] = make_uint4(0u, 0u, 0u, __float_as_uint(-1.0f));
                    out[2 * (size_t)q + 1] = make_uint4(kInvalid, kInvalid, q, 0u);
                } else if (pm.last) {
                    reinterpret_cast<uint32_t *>(out)[8 * (size_t)q + 7] = 0u;   // (the running d2 of an earlier launch's answer)
                }
                has = false;
            }
        }
    }
}

}  // namespace

void launch_closest_points(hipStream_t s, uint32_t grid_blocks, const void *points, uint32_t n, const RayBatch &batch, const PointMargins &pm,
                           const WideNode *wide, const TriRecord *records, uint32_t leaf_size, void *out, uint32_t *counter, uint32_t *spill)
{
    if (!n || !batch.n) return;
    const uint32_t grid = min(grid_blocks, (n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_closest_points, dim3(grid), dim3(kBlock), 0, s, static_cast<const float4 *>(points), n, batch, pm, wide, records,
                       leaf_size, static_cast<uint4 *>(out), counter, spill);
}

}  // namespace ls
