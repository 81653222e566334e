// ls_standing.hip -- the kernels of the standing list (ls_standing.h).  Not a translation unit of its own: ls_project.hip
// includes it, inside namespace ls, behind the device functions both are made of -- a record holds what project_body stages for
// a triangle, computed by the same functions (xform_corners, outside_sector, band, columns, sub, cross_fma, dot_fma) under the
// same compiler options, and a frame expands it with the same queue_big / stage_foot / expand_staged: a frame traced from the
// list is the frame traced from the mesh, bit for bit.

namespace {

// One lane per triangle; a wave takes eight runs of eight triangles a stride of the wave count apart, as the unculled launch of
// a big mesh does, so that the records a wave appends -- and a wave of k_project_standing later takes -- mix the near field,
// where the cells are, with the far.  The wave's records go to the list behind one atomicAdd.  No keys, no queue, no counter of
// a frame is touched.  The channel tables are read where they are: the launch runs once per list.
__global__ __launch_bounds__(kBlock) void k_standing_build(ProjectParams pp, GeomSource src, StandingRecord *__restrict__ recs,
                                                           uint32_t capacity, uint32_t *__restrict__ count)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t n_waves = (src.ntris + 63u) / 64u, rank = blockIdx.x * (kBlock / 64) + w;
    if (rank >= n_waves) return;   // (the grid is rounded up to whole workgroups; no barrier follows)
    const uint32_t k = ((lane >> 3) * n_waves + rank) * 8u + (lane & 7u);
    const ChanTables ct = {pp.chan_tan_up, pp.chan_tan_dn, pp.tb.sin_theta, pp.tb.cos_theta, pp.chan_perm, nullptr};
    uint32_t cells = 0;
    Foot f = {0, 0, 0, 0, 0, 0};
    V3 v0 = {0.f, 0.f, 0.f}, v1 = v0, v2 = v0;
    if (k < src.ntris) {
        const uint32_t a = src.idx[3 * (size_t)k + 0], b = src.idx[3 * (size_t)k + 1], c = src.idx[3 * (size_t)k + 2];
        const float *pa = reinterpret_cast<const float *>(src.verts + (size_t)a * src.stride);
        const float *pb = reinterpret_cast<const float *>(src.verts + (size_t)b * src.stride);
        const float *pc = reinterpret_cast<const float *>(src.verts + (size_t)c * src.stride);
        const float raw[9] = {pa[0], pa[1], pa[2], pb[0], pb[1], pb[2], pc[0], pc[1], pc[2]};
        xform_corners(src, raw, v0, v1, v2);
        if (!outside_sector(pp, v0, v1, v2)) band(pp, ct, v0, v1, v2, f.i0, f.nch);
        if (f.nch) columns(pp, v0, v1, v2, f.h0a, f.na, f.h0b, f.nb);
        cells = f.nch * (f.na + f.nb);
    }
    const unsigned long long mine = __ballot(cells != 0);
    if (!mine) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(count, (uint32_t)__popcll(mine));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    const uint32_t at = base + lanes_below(mine);
    if (cells && at < capacity) {   // (a list that does not fit is counted to the end and never used)
        const V3 e1 = sub(v0, v1), e2 = sub(v2, v0);
        const float NgC = dot_fma(cross_fma(e2, e1), v0);
        const uint32_t gid = src.gid_first + (src.perm ? src.perm[k] : k);
        float4 *out = reinterpret_cast<float4 *>(recs + at);
        out[0] = make_float4(v0.x, v0.y, v0.z, e1.x);
        out[1] = make_float4(e1.y, e1.z, e2.x, e2.y);
        out[2] = make_float4(e2.z, NgC, __uint_as_float(gid), __uint_as_float(f.i0 | (f.nch << 16)));
        out[3] = make_float4(__uint_as_float(f.h0a), __uint_as_float(f.na), __uint_as_float(f.h0b), __uint_as_float(f.nb));
    }
}

// A wave takes N consecutive records of its list -- a lane one, as four 16-byte loads -- and expands them as k_project's waves
// expand what they staged.  What is left of k_project's chain of dependent steps (index load -> vertex gather -> transform ->
// band -> columns -> staging -> scan -> trips) is one load, the staging, the scan and the trips.
template <uint32_t N, bool LDS_TABLES>
__global__ __launch_bounds__(kBlock) void k_project_standing(ProjectParams pp, StandingBatch batch, unsigned long long *__restrict__ best,
                                                             BigItem *__restrict__ big, uint32_t big_capacity, uint32_t *__restrict__ big_count)
{
    static_assert(N >= 1 && N <= 64, "a lane takes at most one record");
    __shared__ ProjectLds lds;
    extern __shared__ __attribute__((aligned(16))) float s_chan[];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t gi = 0;   // the workgroup's list (uniform)
    while (gi + 1u < batch.n && blockIdx.x >= batch.block_first[gi + 1u]) ++gi;
    const uint32_t count = batch.count[gi];
    const uint32_t first = ((blockIdx.x - batch.block_first[gi]) * (kBlock / 64) + w) * N;
    // the record's loads go out before the channel tables are staged, as project_body's do
    const bool have = lane < N && first + lane < count;
    float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0, q2 = q0, q3 = q0;
    if (have) {
        const float4 *r = reinterpret_cast<const float4 *>(batch.recs[gi] + first + lane);
        q0 = r[0]; q1 = r[1]; q2 = r[2]; q3 = r[3];
    }
    ChanTables ct = {nullptr, nullptr, pp.tb.sin_theta, pp.tb.cos_theta, pp.chan_perm, nullptr};   // (no band is computed here)
    if (LDS_TABLES) {
        const uint32_t V = pp.tb.V;
        for (uint32_t i = threadIdx.x; i < V; i += kBlock) {
            s_chan[i] = pp.tb.sin_theta[i];
            s_chan[V + i] = pp.tb.cos_theta[i];
            s_chan[2 * V + i] = __uint_as_float(pp.chan_perm[i]);
        }
        ct = {nullptr, nullptr, s_chan, s_chan + V, reinterpret_cast<const uint32_t *>(s_chan + 2 * V), nullptr};
        __syncthreads();
    }
    if (first >= count) return;   // the list's last workgroup is partly filled (no barrier follows)
    uint32_t cells = 0, slot = 0;
    if (have) {
        const V3 v0 = {q0.x, q0.y, q0.z}, e1 = {q0.w, q1.x, q1.y}, e2 = {q1.z, q1.w, q2.x};
        const float NgC = q2.y;
        const uint32_t gid = __float_as_uint(q2.z), i0_nch = __float_as_uint(q2.w);
        const Foot f = {i0_nch & 0xFFFFu, i0_nch >> 16, __float_as_uint(q3.x), __float_as_uint(q3.y), __float_as_uint(q3.z), __float_as_uint(q3.w)};
        cells = f.nch * (f.na + f.nb);
        if (cells > pp.big_cells && queue_big(big, big_capacity, big_count, v0, e1, e2, NgC, gid, f)) {
            cells = 0;
        } else {
            slot = lanes_below(__ballot(true));
            stage_foot(lds, w, slot, v0, e1, e2, NgC, gid, f);
        }
    }
    expand_staged(pp, ct, lds, w, lane, cells, slot, best);
}

// records per wave: one instantiation ships; the experiment build keeps the three that E27 measured against each other
uint32_t standing_per_wave()
{
#ifdef LS_EXPERIMENTAL
    static const uint32_t n = (uint32_t)lsi::tune_int("LS_STANDING_PER_WAVE", (int)kStandingPerWave);
    return n == 16u || n == 64u ? n : 32u;
#else
    return kStandingPerWave;
#endif
}

}  // namespace

hipError_t launch_standing_build(hipStream_t s, const ProjectParams &pp, const GeomSource &src, StandingRecord *recs, uint32_t capacity, uint32_t *count)
{
    const hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), s);
    if (e != hipSuccess || !src.ntris || !(pp.tb.V * pp.tb.naz)) return e;
    const uint32_t n_waves = (src.ntris + 63u) / 64u;
    hipLaunchKernelGGL(k_standing_build, dim3((n_waves + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, s, pp, src, recs, capacity, count);
    return hipSuccess;
}

void standing_batch_add(StandingBatch &batch, const StandingRecord *recs, uint32_t count)
{
    const uint32_t per_block = standing_per_wave() * (kBlock / 64);
    batch.recs[batch.n] = recs;
    batch.count[batch.n] = count;
    batch.block_first[batch.n + 1u] = batch.block_first[batch.n] + (count + per_block - 1u) / per_block;
    ++batch.n;
}

void launch_project_standing(hipStream_t s, const ProjectParams &pp, const StandingBatch &batch, unsigned long long *best, void *big,
                             uint32_t big_capacity, uint32_t *big_count)
{
    const uint32_t blocks = batch.block_first[batch.n];
    if (!blocks || !(pp.tb.V * pp.tb.naz)) return;
    BigItem *bq = static_cast<BigItem *>(big);
    const bool lt = pp.tb.V <= 2048u;   // channel tables fit in LDS
    const uint32_t lds = lt ? (uint32_t)(3 * (size_t)pp.tb.V * sizeof(float)) : 0u;
#define LS_STANDING(N) do { \
        if (lt) launch_k(k_project_standing<N, true>, dim3(blocks), dim3(kBlock), lds, s, pp, batch, best, bq, big_capacity, big_count); \
        else launch_k(k_project_standing<N, false>, dim3(blocks), dim3(kBlock), lds, s, pp, batch, best, bq, big_capacity, big_count); } while (0)
#ifdef LS_EXPERIMENTAL
    if (standing_per_wave() == 16u) { LS_STANDING(16); return; }
    if (standing_per_wave() == 64u) { LS_STANDING(64); return; }
#endif
    LS_STANDING(kStandingPerWave);
#undef LS_STANDING
}
