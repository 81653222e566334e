// ls_beam.hip -- k_beam_rays, k_beam_reduce, k_beam_count + k_beam_pack: the passes ls_trace_scene_beams (include/lidarshooter_hip.h;
// DESIGN.md 3.3.6) puts around the ray queries' walk (k_trace_rays, ls_rays.hip), which it runs unchanged; and their siblings for
// ls_trace_scene_beams_sweep: k_beam_sweep_rays, k_beam_reduce_weighted, k_beam_sweep_pack.
//
// k_beam_rays, one lane per sub-ray: the S samples of a beam around the nominal direction of its ray (ls_beam.h: the arithmetic
// ls_debug_beam_ray runs on the host) as 32-byte lidarshooter::Ray records at q * S + s, q the shard-local ray index -- what the walk
// reads.  A wave is 64 consecutive sub-rays of ONE ring: the ring's two table entries are the same in every lane, its records 2 KB
// of contiguous memory written once, 16 bytes per store.  The pattern arrives by value (768 bytes of kernel arguments).
// k_beam_reduce, P lanes per beam (the smallest power of two >= S, 64 / P beams per wave): every lane takes the walk's dense record of
// one sub-ray and makes its key (bits(t k) << 8 | s, a miss all ones), the group sorts its keys with a bitonic network over
// __shfl_xor, a lane whose range lies more than the separation behind its neighbour's starts an echo (beam_reduce_head), the group's
// part of the ballot mask goes through beam_select (ls_beam.h, the code the host hook runs) in registers, and the first 0..3 lanes of
// the group fetch geom / prim of their echo's nearest member with one 16-byte load and write the beam's block: up to three 16-byte
// records {bits(r), geom, prim, echo word} and, apart from them, a count (beam_reduce_tail).
// k_beam_count + k_beam_pack, one lane per beam: the ordered pack (ls_pack.h) with 0..3 records per lane -- the records of every 256
// beams counted, then each workgroup adds up the counts of the workgroups before it, ranks its own by a wave scan and a four-entry
// prefix across its waves, and writes point, hit record and echo word at that position: ascending ray index, ascending range inside
// a beam.  Both pack kernels are beam_pack_body, the two reduces share beam_reduce_head / beam_reduce_tail, the two ray generators
// beam_sub_ray.
// Bytes per sub-ray: 32 written; 16 read (8 of them used).  Per beam: 4 + 16 per return written, read twice / once.  Per return:
// 16 read again (geom / prim), 52 written.
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_beam.h"
#include "ls_sweep.h"
#include "ls_pack.h"
#include "ls_hit_gather.h"

namespace ls {

namespace {

constexpr uint32_t kBeamRows = kBlock / 64;   // rings per workgroup of k_beam_rays: one per wave

// sub-ray i = c * S + s of ring v (i < naz * S): sample s of the beam around the nominal direction of column az0 + c -> its record
// at rest, its column *h and its place *q among the shard's sub-rays (< 2^27: beams_locked, beams_sweep_check)
__device__ __forceinline__ void beam_sub_ray(const SensorTables &tb, const BeamPattern &pat, uint32_t S, uint32_t v, uint32_t i, float *ray8,
                                             uint32_t *h, size_t *q)
{
    const uint32_t c = i / S, s = i - c * S;
    *h = tb.az0 + c;   // < H: the shard lies inside the raster (ls_tracer_set_shard)
    const float st = tb.sin_theta[v], ctv = tb.cos_theta[v];
    const float2 cs = tb.cs_phi[*h];
    beam_ray(st, ctv, cs.x, cs.y, pat.a[s], pat.b[s], ray8);
    *q = (size_t)v * tb.naz * S + i;
}

__global__ __launch_bounds__(kBlock) void k_beam_rays(SensorTables tb, BeamPattern pat, uint32_t S, float4 *__restrict__ rays)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t v = blockIdx.y * kBeamRows + w, i = blockIdx.x * 64u + lane;   // i: the sub-ray inside its ring, c * S + s
    if (v >= tb.V || i >= tb.naz * S) return;
    uint32_t h;
    size_t q;
    float r[8];
    beam_sub_ray(tb, pat, S, v, i, r, &h, &q);
    rays[2 * q] = make_float4(r[0], r[1], r[2], r[3]);
    rays[2 * q + 1] = make_float4(r[4], r[5], r[6], r[7]);
}

// The head of both reduces.  P lanes per beam, a power of two in 1..64 (wave-uniform): the lane's position jl in its group, the
// group's first lane, its beam q (grid: ceil(nq / (4 * 64 / P)) workgroups -- no overflow, nq P <= 2^28); the lane's key after the
// group has sorted its keys; the group's part of the two ballots: the positions that start an echo, and how many hold a hit.
struct BeamGroup {
    uint32_t jl, base, q;
    bool beam;                      // q < nq
    unsigned long long key;         // position jl of the beam's ascending order (a miss: kBeamMiss)
    unsigned long long mask;        // P ones
    unsigned long long starts;
    uint32_t n_hits;
};

__device__ __forceinline__ BeamGroup beam_reduce_head(const uint4 *__restrict__ dense, uint32_t nq, uint32_t S, uint32_t P, const BeamPattern &pat,
                                                      float separation)
{
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6);
    const uint32_t jl = lane & (P - 1u), base = lane - jl;
    const uint32_t q = wave * (64u / P) + base / P;
    const bool beam = q < nq;
    unsigned long long key = kBeamMiss;
    if (beam && jl < S) {
        const uint4 rec = dense[(size_t)q * S + jl];
        if (rec.y != kInvalid) key = beam_key(__uint_as_float(rec.w) * pat.k[jl], jl);
    }
    // ascending inside every group of P lanes (the bitonic network; keys differ in their sample, so the order is total)
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const unsigned long long other = __shfl_xor(key, (int)j);
            const bool up = (jl & k) == 0u, low = (jl & j) == 0u;
            const bool take_min = up == low;
            key = (other < key) == take_min ? other : key;
        }
    const unsigned long long prev = __shfl_up(key, 1u);   // (position 0 ignores it)
    const unsigned long long m_start = __ballot(beam_starts_echo(prev, key, jl, separation));
    const unsigned long long m_hit = __ballot(key != kBeamMiss);
    const unsigned long long group = P == 64u ? ~0ull : (1ull << P) - 1ull;
    return {jl, base, q, beam, key, group, (m_start >> base) & group, (uint32_t)__popcll((m_hit >> base) & group)};
}

// The tail of both reduces, for the lanes of a beam: the beam's count n and, in its first n lanes, the block's record {bits(r), geom,
// prim, echo word} -- geom / prim of the echo's nearest member, one 16-byte load.  word: the lane's echo word of the selection; sel:
// the key at that echo's position.  n <= the beam's sub-hits <= S <= P: such lanes exist.  Returns whether the lane wrote a record.
__device__ __forceinline__ bool beam_reduce_tail(const BeamGroup &g, const uint4 *__restrict__ dense, uint32_t S, uint32_t n, uint32_t word,
                                                 unsigned long long sel, uint4 *__restrict__ blocks, uint32_t *__restrict__ cnt)
{
    if (g.jl == 0u) cnt[g.q] = n;
    if (g.jl >= n) return false;
    const uint32_t s = beam_key_sample(sel);
    const uint4 rec = dense[(size_t)g.q * S + s];
    blocks[3 * (size_t)g.q + g.jl] = make_uint4((uint32_t)(sel >> 8), rec.y, rec.z, beam_word(word & 7u, beam_word_count(word), s));
    return true;
}

__global__ __launch_bounds__(kBlock) void k_beam_reduce(const uint4 *__restrict__ dense, uint32_t nq, uint32_t S, uint32_t P, BeamPattern pat,
                                                        float separation, uint32_t min_count, uint32_t returns, uint4 *__restrict__ blocks,
                                                        uint32_t *__restrict__ cnt)
{
    const BeamGroup g = beam_reduce_head(dense, nq, S, P, pat, separation);
    const BeamReturns ret = beam_select(g.starts, g.n_hits, min_count, returns);
    const uint32_t n = ret.n, word = g.jl == 0u ? ret.w0 : g.jl == 1u ? ret.w1 : ret.w2;
    // the key at the echo's position (every lane takes part: a lane without a record reads position 0 of its group)
    const unsigned long long sel = __shfl(g.key, (int)(g.base + beam_word_where(word)));
    if (!g.beam) return;
    beam_reduce_tail(g, dense, S, n, word, sel, blocks, cnt);
}

// records per 256 consecutive beams (feeds the ordered pack)
__global__ __launch_bounds__(kBlock) void k_beam_count(const uint32_t *__restrict__ cnt, uint32_t nq, uint32_t *__restrict__ block_counts)
{
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    block_count_store(wave_sum(q < nq ? cnt[q] : 0u), block_counts);
}

// Both pack kernels.  !WEIGHTED: the intensity from an echo's member count out of S, xyz = r * d -- the range the sensor reports along
// its axis, no sum: the frame's bits when r is the ray's t.  WEIGHTED: the intensity from wsum out of w_total, and under
// LS_SWEEP_DESKEW with a pose table the point carried through its column's pose, o_h + r * d' per axis (ls_sweep.h).  A compile-time
// flag: the instantiation ls_trace_scene_beams runs stays the code it was.
template <bool WEIGHTED>
__device__ __forceinline__ void beam_pack_body(const SensorTables &tb, uint32_t S, const uint4 *__restrict__ blocks, const uint32_t *__restrict__ wsum,
                                               const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ block_counts, uint32_t w_total,
                                               const float *__restrict__ pose, uint32_t aligned16, uint32_t deskew, float4 *__restrict__ points,
                                               uint4 *__restrict__ hits, uint32_t *__restrict__ echo, uint32_t *__restrict__ n_points,
                                               uint32_t capacity)
{
    const uint32_t nq = tb.V * tb.naz;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    // the beam's count, the ray's table entries and the counts of the workgroups before this one: all requested up front
    const uint32_t c = q < nq ? cnt[q] : 0u;
    uint32_t v, h;
    float d[3];
    shard_ray_dir(tb, q < nq ? q : 0u, d, &v, &h);
    const uint32_t acc = counts_before(block_counts, blockIdx.x);
    const uint32_t upto = wave_inclusive_sum(c, lane);   // the records of this lane and the lanes before it in the wave
    const uint32_t first = pack_wave_base(acc, upto, 63u, blockIdx.x == gridDim.x - 1, n_points);
    if (WEIGHTED && !c) return;   // (past the barrier and the shuffles)
    const uint32_t dst = first + upto - c;
    float p[12];
    const bool carried = WEIGHTED && points && deskew && pose;
    if (carried) load_pose(pose, h, aligned16 != 0u, p);
#pragma unroll
    for (uint32_t i = 0; i < 3u; ++i) {
        if (i >= c || dst + i >= capacity) break;   // (dst + c <= K * the shard's rays <= capacity: the second never holds)
        const uint4 rec = blocks[3 * (size_t)q + i];
        const size_t at = (size_t)dst + i;
        const float r = __uint_as_float(rec.x);
        if (points) {
            float xyz[3];
            if (carried) {
                sweep_point(p, d[0], d[1], d[2], r, xyz);
            } else {
                xyz[0] = r * d[0]; xyz[1] = r * d[1]; xyz[2] = r * d[2];
            }
            const float intensity = WEIGHTED ? beam_intensity_weighted(wsum[3 * (size_t)q + i], w_total) : beam_intensity(beam_word_count(rec.w), S);
            points[2 * at] = make_float4(xyz[0], xyz[1], xyz[2], 0.0f);
            points[2 * at + 1] = make_float4(intensity, __int_as_float((int)v), 0.0f, 0.0f);
        }
        if (hits) hits[at] = make_uint4(v * tb.H + h, rec.y, rec.z, rec.x);
        if (echo) echo[at] = rec.w;
    }
}

__global__ __launch_bounds__(kBlock) void k_beam_pack(SensorTables tb, uint32_t S, const uint4 *__restrict__ blocks, const uint32_t *__restrict__ cnt,
                                                      const uint32_t *__restrict__ block_counts, float4 *__restrict__ points,
                                                      uint4 *__restrict__ hits, uint32_t *__restrict__ echo, uint32_t *__restrict__ n_points,
                                                      uint32_t capacity)
{
    beam_pack_body<false>(tb, S, blocks, nullptr, cnt, block_counts, 0u, nullptr, 0u, 0u, points, hits, echo, n_points, capacity);
}

// ---- ls_trace_scene_beams_sweep: the same passes with a pose per azimuth column and a weight per sample.  At rest
// the sub-rays ARE k_beam_rays', the count is k_beam_count.

// k_beam_rays under the per-column poses: the same layout (a wave is 64 consecutive sub-rays of one ring, two 16-byte stores per
// lane), beam_ray and then sweep_ray on its direction.  The record belongs to the column, not to the wave -- a wave spans up to
// ceil(64 / S) + 1 columns --, so every lane loads its own: three 16-byte loads where the table's address allows them (checked once
// on the host, wave-uniform), twelve 4-byte loads otherwise, as k_sweep_rays does; the lanes of one column read the same addresses.
__global__ __launch_bounds__(kBlock) void k_beam_sweep_rays(SensorTables tb, BeamPattern pat, uint32_t S, const float *__restrict__ pose,
                                                            uint32_t aligned16, float4 *__restrict__ rays)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t v = blockIdx.y * kBeamRows + w, i = blockIdx.x * 64u + lane;   // i: the sub-ray inside its ring, c * S + s
    if (v >= tb.V || i >= tb.naz * S) return;
    uint32_t h;
    size_t q;
    float p[12], b[8], r[8];
    beam_sub_ray(tb, pat, S, v, i, b, &h, &q);
    load_pose(pose, h, aligned16 != 0u, p);
    sweep_ray(p, b[4], b[5], b[6], r);
    rays[2 * q] = make_float4(r[0], r[1], r[2], r[3]);
    rays[2 * q + 1] = make_float4(r[4], r[5], r[6], r[7]);
}

// k_beam_reduce with weights.  After the head every lane holds one POSITION of its beam's ascending order: it looks up the weight of
// the sample its key names (a miss weighs 0), an inclusive prefix sum runs inside the group, a lane that starts an echo finds the
// echo's end in the start mask and takes W_e from the prefix at the end and n_e from the positions; FIRST and LAST come out of the
// ballot of the detectable starts, STRONGEST out of a maximum over the group.  Every __shfl* and __ballot is executed by all 64
// lanes: the loops that hold one run log2(P) times, P the same in the whole launch, and nothing crosses lanes under a condition
// that differs inside a wave.  blocks / cnt: as k_beam_reduce; wsum: W_e of every record, at the record's index.
__global__ __launch_bounds__(kBlock) void k_beam_reduce_weighted(const uint4 *__restrict__ dense, uint32_t nq, uint32_t S, uint32_t P, BeamPattern pat,
                                                                 BeamWeights wts, float separation, uint32_t min_count, uint32_t min_weight,
                                                                 uint32_t returns, uint4 *__restrict__ blocks, uint32_t *__restrict__ wsum,
                                                                 uint32_t *__restrict__ cnt)
{
    const BeamGroup g = beam_reduce_head(dense, nq, S, P, pat, separation);
    const uint32_t jl = g.jl, base = g.base;
    // the weight at this position and the sum of the weights up to it (a sample index is < S <= 64; the group's lanes only)
    const uint32_t wj = g.key != kBeamMiss ? (uint32_t)wts.w[beam_key_sample(g.key)] : 0u;
    uint32_t upto = wj;
    for (uint32_t off = 1; off < P; off <<= 1) {
        const uint32_t below = __shfl_up(upto, off);
        if (jl >= off) upto += below;
    }
    // as if this position started an echo: a lane that starts none computes values nobody reads (end >= 1 wherever n_hits >= 1)
    const bool start = ((g.starts >> jl) & 1ull) != 0ull;
    const uint32_t end = beam_echo_end(g.starts, g.n_hits, jl);
    const uint32_t last = end > jl ? end - 1u : jl;   // a start: jl < end <= n_hits <= P; any lane: inside its group
    const uint32_t W = __shfl(upto, (int)(base + last)) - (upto - wj);
    const bool det = start && beam_detectable(end - jl, W, min_count, min_weight);
    const unsigned long long m_det = __ballot(det);
    uint32_t best = det ? beam_strength(W, jl) : 0u;
    for (uint32_t off = 1; off < P; off <<= 1) {
        const uint32_t other = __shfl_xor(best, (int)off);
        best = other > best ? other : best;
    }
    const BeamReturns ret = beam_select_weighted(g.starts, g.n_hits, (m_det >> base) & g.mask, beam_strength_where(best), returns);
    const uint32_t n = ret.n, word = jl == 0u ? ret.w0 : jl == 1u ? ret.w1 : ret.w2;
    // the key and the strength at the echo's position (every lane takes part: a lane without a record reads position 0 of its group)
    const unsigned long long sel = __shfl(g.key, (int)(base + beam_word_where(word)));
    const uint32_t W_sel = __shfl(W, (int)(base + beam_word_where(word)));
    if (!g.beam) return;
    if (beam_reduce_tail(g, dense, S, n, word, sel, blocks, cnt)) wsum[3 * (size_t)g.q + jl] = W_sel;
}

// k_beam_pack with the weighted intensity and, under LS_SWEEP_DESKEW, the point carried through the column's pose.  pose == nullptr:
// the sensor at rest, the flag changes nothing.
__global__ __launch_bounds__(kBlock) void k_beam_sweep_pack(SensorTables tb, const uint4 *__restrict__ blocks, const uint32_t *__restrict__ wsum,
                                                            const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ block_counts,
                                                            uint32_t w_total, const float *__restrict__ pose, uint32_t aligned16, uint32_t deskew,
                                                            float4 *__restrict__ points, uint4 *__restrict__ hits, uint32_t *__restrict__ echo,
                                                            uint32_t *__restrict__ n_points, uint32_t capacity)
{
    beam_pack_body<true>(tb, 0u, blocks, wsum, cnt, block_counts, w_total, pose, aligned16, deskew, points, hits, echo, n_points, capacity);
}

// P, the lanes a beam of S samples takes in k_beam_reduce*: the smallest power of two >= S
uint32_t beam_group_lanes(uint32_t S)
{
    uint32_t P = 1;
    while (P < S) P <<= 1;
    return P;
}

// the grids: 4 * 64 / P beams per workgroup of k_beam_reduce*; one wave per 64 sub-rays of a ring in k_beam_*rays
dim3 beam_reduce_grid(uint32_t nq, uint32_t P) { return dim3((nq + 256u / P - 1u) / (256u / P)); }
dim3 beam_rays_grid(const SensorTables &tb, uint32_t S) { return dim3((tb.naz * S + 63u) / 64u, (tb.V + kBeamRows - 1u) / kBeamRows); }

}  // namespace

size_t beam_block_count(uint32_t nq) { return ((size_t)nq + kBlock - 1) / kBlock; }

void launch_beam_rays(hipStream_t s, const SensorTables &tb, const BeamPattern &pat, uint32_t S, void *rays)
{
    hipLaunchKernelGGL(k_beam_rays, beam_rays_grid(tb, S), dim3(kBlock), 0, s, tb, pat, S, static_cast<float4 *>(rays));
}

void launch_beam_pack(hipStream_t s, const SensorTables &tb, const BeamPattern &pat, uint32_t S, float separation, uint32_t min_count,
                      uint32_t returns, const void *dense, void *blocks, uint32_t *cnt, uint32_t *block_counts, void *points32, void *hits,
                      uint32_t *echo, uint32_t *n_points, uint32_t capacity)
{
    const uint32_t nq = tb.V * tb.naz, P = beam_group_lanes(S);
    hipLaunchKernelGGL(k_beam_reduce, beam_reduce_grid(nq, P), dim3(kBlock), 0, s, static_cast<const uint4 *>(dense), nq, S, P, pat, separation,
                       min_count, returns, static_cast<uint4 *>(blocks), cnt);
    const dim3 grid((uint32_t)beam_block_count(nq));
    hipLaunchKernelGGL(k_beam_count, grid, dim3(kBlock), 0, s, static_cast<const uint32_t *>(cnt), nq, block_counts);
    hipLaunchKernelGGL(k_beam_pack, grid, dim3(kBlock), 0, s, tb, S, static_cast<const uint4 *>(blocks), static_cast<const uint32_t *>(cnt),
                       static_cast<const uint32_t *>(block_counts), static_cast<float4 *>(points32), static_cast<uint4 *>(hits), echo, n_points,
                       capacity);
}

void launch_beam_sweep_rays(hipStream_t s, const SensorTables &tb, const BeamPattern &pat, uint32_t S, const float *pose, void *rays)
{
    if (!pose) return launch_beam_rays(s, tb, pat, S, rays);   // at rest: the sub-rays of ls_trace_scene_beams
    hipLaunchKernelGGL(k_beam_sweep_rays, beam_rays_grid(tb, S), dim3(kBlock), 0, s, tb, pat, S, pose, table_aligned16(pose),
                       static_cast<float4 *>(rays));
}

void launch_beam_sweep_pack(hipStream_t s, const SensorTables &tb, const BeamPattern &pat, const BeamWeights &wts, uint32_t w_total, uint32_t S,
                            float separation, uint32_t min_count, uint32_t min_weight, uint32_t returns, const float *pose, bool deskew,
                            const void *dense, void *blocks, uint32_t *wsum, uint32_t *cnt, uint32_t *block_counts, void *points32, void *hits,
                            uint32_t *echo, uint32_t *n_points, uint32_t capacity)
{
    const uint32_t nq = tb.V * tb.naz, P = beam_group_lanes(S);
    hipLaunchKernelGGL(k_beam_reduce_weighted, beam_reduce_grid(nq, P), dim3(kBlock), 0, s, static_cast<const uint4 *>(dense), nq, S, P, pat, wts,
                       separation, min_count, min_weight, returns, static_cast<uint4 *>(blocks), wsum, cnt);
    const dim3 grid((uint32_t)beam_block_count(nq));
    hipLaunchKernelGGL(k_beam_count, grid, dim3(kBlock), 0, s, static_cast<const uint32_t *>(cnt), nq, block_counts);
    hipLaunchKernelGGL(k_beam_sweep_pack, grid, dim3(kBlock), 0, s, tb, static_cast<const uint4 *>(blocks), static_cast<const uint32_t *>(wsum),
                       static_cast<const uint32_t *>(cnt), static_cast<const uint32_t *>(block_counts), w_total, pose, table_aligned16(pose),
                       deskew ? 1u : 0u, static_cast<float4 *>(points32), static_cast<uint4 *>(hits), echo, n_points, capacity);
}

}  // namespace ls
