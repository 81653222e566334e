// ls_beam.hip -- k_beam_rays, k_beam_reduce, k_beam_count + k_beam_pack: the passes ls_trace_scene_beams (include/lidarshooter_hip.h;
// DESIGN.md 3.3.6) puts around the ray queries' walk (k_trace_rays, ls_rays.hip), which it runs unchanged.
//
// k_beam_rays, one lane per sub-ray: the S samples of a beam around the nominal direction of its ray (ls_beam.h: the arithmetic
// ls_debug_beam_ray runs on the host) as 32-byte lidarshooter::Ray records at q * S + s, q the shard-local ray index -- what the walk
// reads.  A wave is 64 consecutive sub-rays of ONE ring: the ring's two table entries are the same in every lane, its records 2 KB
// of contiguous memory written once, 16 bytes per store.  The pattern arrives by value (768 bytes of kernel arguments).
// k_beam_reduce, P lanes per beam (the smallest power of two >= S, 64 / P beams per wave): every lane takes the walk's dense record of
// one sub-ray and makes its key (bits(t k) << 8 | s, a miss all ones), the group sorts its keys with a bitonic network over
// __shfl_xor, a lane whose range lies more than the separation behind its neighbour's starts an echo, the group's part of the ballot
// mask goes through beam_select (ls_beam.h, the code the host hook runs) in registers, and the first 0..3 lanes of the group fetch geom
// / prim of their echo's nearest member with one 16-byte load and write the beam's block: up to three 16-byte records {bits(r), geom,
// prim, echo word} and, apart from them, a count.
// k_beam_count + k_beam_pack, one lane per beam: the ordered pack of k_sweep_count + k_sweep_pack (ls_sweep.hip) with 0..3 records
// per lane instead of a ballot bit -- the records of every 256 beams counted, then each workgroup adds up the counts of the
// workgroups before it, ranks its own by a wave scan and a four-entry prefix across its waves, and writes point, hit record and echo
// word at that position: ascending ray index, ascending range inside a beam, no atomic append, no workgroup waiting for another.
// Bytes per sub-ray: 32 written; 16 read (8 of them used).  Per beam: 4 + 16 per return written, read twice / once.  Per return:
// 16 read again (geom / prim), 52 written.
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_beam.h"
#include "ls_sweep.h"

namespace ls {

namespace {

constexpr uint32_t kBeamRows = kBlock / 64;   // rings per workgroup of k_beam_rays: one per wave

__global__ __launch_bounds__(kBlock) void k_beam_rays(SensorTables tb, BeamPattern pat, uint32_t S, float4 *__restrict__ rays)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t v = blockIdx.y * kBeamRows + w, i = blockIdx.x * 64u + lane;   // i: the sub-ray inside its ring, c * S + s
    if (v >= tb.V || i >= tb.naz * S) return;
    const uint32_t c = i / S, s = i - c * S;
    const uint32_t h = tb.az0 + c;   // < H: the shard lies inside the raster (ls_tracer_set_shard)
    const float st = tb.sin_theta[v], ctv = tb.cos_theta[v];
    const float2 cs = tb.cs_phi[h];
    float r[8];
    beam_ray(st, ctv, cs.x, cs.y, pat.a[s], pat.b[s], r);
    const size_t q = (size_t)v * tb.naz * S + i;   // < 2^27 (beams_locked)
    rays[2 * q] = make_float4(r[0], r[1], r[2], r[3]);
    rays[2 * q + 1] = make_float4(r[4], r[5], r[6], r[7]);
}

// P: lanes per beam, a power of two in 1..64 (wave-uniform)
__global__ __launch_bounds__(kBlock) void k_beam_reduce(const uint4 *__restrict__ dense, uint32_t nq, uint32_t S, uint32_t P, BeamPattern pat,
                                                        float separation, uint32_t min_count, uint32_t returns, uint4 *__restrict__ blocks,
                                                        uint32_t *__restrict__ cnt)
{
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6);
    const uint32_t jl = lane & (P - 1u), base = lane - jl;
    const uint32_t q = wave * (64u / P) + base / P;   // grid: ceil(nq / (4 * 64 / P)) workgroups -- no overflow (nq P <= 2^28)
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
    const BeamReturns ret = beam_select((m_start >> base) & group, (uint32_t)__popcll((m_hit >> base) & group), min_count, returns);
    const uint32_t n = ret.n, word = jl == 0u ? ret.w0 : jl == 1u ? ret.w1 : ret.w2;
    // the key at the echo's position (every lane takes part: a lane without a record reads position 0 of its group)
    const unsigned long long sel = __shfl(key, (int)(base + beam_word_where(word)));
    if (!beam) return;
    if (jl == 0u) cnt[q] = n;
    if (jl < n) {   // n <= the beam's sub-hits <= S <= P: such a lane exists
        const uint32_t s = beam_key_sample(sel);
        const uint4 rec = dense[(size_t)q * S + s];
        blocks[3 * (size_t)q + jl] = make_uint4((uint32_t)(sel >> 8), rec.y, rec.z, beam_word(word & 7u, beam_word_count(word), s));
    }
}

// records per 256 consecutive beams (feeds the ordered pack)
__global__ __launch_bounds__(kBlock) void k_beam_count(const uint32_t *__restrict__ cnt, uint32_t nq, uint32_t *__restrict__ block_counts)
{
    __shared__ uint32_t s_cnt[kBlock / 64];
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    uint32_t c = q < nq ? cnt[q] : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(kBlock) void k_beam_pack(SensorTables tb, uint32_t S, const uint4 *__restrict__ blocks, const uint32_t *__restrict__ cnt,
                                                      const uint32_t *__restrict__ block_counts, float4 *__restrict__ points,
                                                      uint4 *__restrict__ hits, uint32_t *__restrict__ echo, uint32_t *__restrict__ n_points,
                                                      uint32_t capacity)
{
    __shared__ uint32_t s_part[kBlock / 64];
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t nq = tb.V * tb.naz;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    // the beam's count, the ray's table entries and the counts of the workgroups before this one: all requested up front
    const uint32_t c = q < nq ? cnt[q] : 0u;
    const uint32_t qq = q < nq ? q : 0u;
    const uint32_t v = qq / tb.naz, h = tb.az0 + (qq - v * tb.naz);
    const float st = tb.sin_theta[v], ctv = tb.cos_theta[v];
    const float2 cs = tb.cs_phi[h];
    uint32_t acc = 0;
    constexpr uint32_t kCountsAhead = 8;
    for (uint32_t r0 = threadIdx.x; r0 < blockIdx.x; r0 += kCountsAhead * kBlock) {
        uint32_t a[kCountsAhead];
#pragma unroll
        for (uint32_t k = 0; k < kCountsAhead; ++k) a[k] = r0 + k * kBlock < blockIdx.x ? block_counts[r0 + k * kBlock] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < kCountsAhead; ++k) acc += a[k];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    uint32_t upto = c;   // the records of this lane and the lanes before it in the wave
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t below = __shfl_up(upto, off);
        if (lane >= off) upto += below;
    }
    if (lane == 63u) { s_part[w] = acc; s_wave[w] = upto; }
    __syncthreads();
    uint32_t first = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (uint32_t k = 0; k < w; ++k) first += s_wave[k];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_points = first + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    const uint32_t dst = first + upto - c;
    const float dx = st * cs.x, dy = st * cs.y;
#pragma unroll
    for (uint32_t i = 0; i < 3u; ++i) {
        if (i >= c || dst + i >= capacity) break;   // (dst + c <= K * the shard's rays <= capacity: the second never holds)
        const uint4 rec = blocks[3 * (size_t)q + i];
        const size_t at = (size_t)dst + i;
        const float r = __uint_as_float(rec.x);
        if (points) {   // the range the sensor reports along its axis: xyz = r * d with no sum, the frame's bits when r is the ray's t
            points[2 * at] = make_float4(r * dx, r * dy, r * ctv, 0.0f);
            points[2 * at + 1] = make_float4(beam_intensity(beam_word_count(rec.w), S), __int_as_float((int)v), 0.0f, 0.0f);
        }
        if (hits) hits[at] = make_uint4(v * tb.H + h, rec.y, rec.z, rec.x);
        if (echo) echo[at] = rec.w;
    }
}

// ---- ls_trace_scene_beams_sweep: the same passes with a pose per azimuth column and a weight per sample.  The
// kernels above are not touched: at rest the sub-rays ARE k_beam_rays', the count is k_beam_count.

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
    const uint32_t c = i / S, s = i - c * S;
    const uint32_t h = tb.az0 + c;   // < H: the shard lies inside the raster (ls_tracer_set_shard)
    float p[12], b[8], r[8];
    load_pose(pose, h, aligned16 != 0u, p);
    const float st = tb.sin_theta[v], ctv = tb.cos_theta[v];
    const float2 cs = tb.cs_phi[h];
    beam_ray(st, ctv, cs.x, cs.y, pat.a[s], pat.b[s], b);
    sweep_ray(p, b[4], b[5], b[6], r);
    const size_t q = (size_t)v * tb.naz * S + i;   // < 2^27 (beams_sweep_check)
    rays[2 * q] = make_float4(r[0], r[1], r[2], r[3]);
    rays[2 * q + 1] = make_float4(r[4], r[5], r[6], r[7]);
}

// k_beam_reduce with weights.  After the sort and the two ballots every lane holds one POSITION of its beam's ascending order: it
// looks up the weight of the sample its key names (a miss weighs 0), an inclusive prefix sum runs inside the group, a lane that
// starts an echo finds the echo's end in the start mask and takes W_e from the prefix at the end and n_e from the positions; FIRST
// and LAST come out of the ballot of the detectable starts, STRONGEST out of a maximum over the group.  Every __shfl* and __ballot
// is executed by all 64 lanes: the loops that hold one run log2(P) times, P the same in the whole launch, and nothing crosses lanes
// under a condition that differs inside a wave.  blocks / cnt: as k_beam_reduce; wsum: W_e of every record, at the record's index.
__global__ __launch_bounds__(kBlock) void k_beam_reduce_weighted(const uint4 *__restrict__ dense, uint32_t nq, uint32_t S, uint32_t P, BeamPattern pat,
                                                                 BeamWeights wts, float separation, uint32_t min_count, uint32_t min_weight,
                                                                 uint32_t returns, uint4 *__restrict__ blocks, uint32_t *__restrict__ wsum,
                                                                 uint32_t *__restrict__ cnt)
{
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6);
    const uint32_t jl = lane & (P - 1u), base = lane - jl;
    const uint32_t q = wave * (64u / P) + base / P;   // grid: ceil(nq / (4 * 64 / P)) workgroups -- no overflow (nq P <= 2^28)
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
    const unsigned long long starts = (m_start >> base) & group;
    const uint32_t n_hits = (uint32_t)__popcll((m_hit >> base) & group);
    // the weight at this position and the sum of the weights up to it (a sample index is < S <= 64; the group's lanes only)
    const uint32_t wj = key != kBeamMiss ? (uint32_t)wts.w[beam_key_sample(key)] : 0u;
    uint32_t upto = wj;
    for (uint32_t off = 1; off < P; off <<= 1) {
        const uint32_t below = __shfl_up(upto, off);
        if (jl >= off) upto += below;
    }
    // as if this position started an echo: a lane that starts none computes values nobody reads (end >= 1 wherever n_hits >= 1)
    const bool start = ((starts >> jl) & 1ull) != 0ull;
    const uint32_t end = beam_echo_end(starts, n_hits, jl);
    const uint32_t last = end > jl ? end - 1u : jl;   // a start: jl < end <= n_hits <= P; any lane: inside its group
    const uint32_t W = __shfl(upto, (int)(base + last)) - (upto - wj);
    const bool det = start && beam_detectable(end - jl, W, min_count, min_weight);
    const unsigned long long m_det = __ballot(det);
    uint32_t best = det ? beam_strength(W, jl) : 0u;
    for (uint32_t off = 1; off < P; off <<= 1) {
        const uint32_t other = __shfl_xor(best, (int)off);
        best = other > best ? other : best;
    }
    const BeamReturns ret = beam_select_weighted(starts, n_hits, (m_det >> base) & group, beam_strength_where(best), returns);
    const uint32_t n = ret.n, word = jl == 0u ? ret.w0 : jl == 1u ? ret.w1 : ret.w2;
    // the key and the strength at the echo's position (every lane takes part: a lane without a record reads position 0 of its group)
    const unsigned long long sel = __shfl(key, (int)(base + beam_word_where(word)));
    const uint32_t W_sel = __shfl(W, (int)(base + beam_word_where(word)));
    if (!beam) return;
    if (jl == 0u) cnt[q] = n;
    if (jl < n) {   // n <= the beam's sub-hits <= S <= P: such a lane exists
        const uint32_t s = beam_key_sample(sel);
        const uint4 rec = dense[(size_t)q * S + s];
        blocks[3 * (size_t)q + jl] = make_uint4((uint32_t)(sel >> 8), rec.y, rec.z, beam_word(word & 7u, beam_word_count(word), s));
        wsum[3 * (size_t)q + jl] = W_sel;
    }
}

// k_beam_pack with the weighted intensity and, under LS_SWEEP_DESKEW, the point carried through the column's pose.  A second
// kernel rather than a parameter of k_beam_pack: the instantiation ls_trace_scene_beams runs stays the code it was.  pose ==
// nullptr: the sensor at rest, the flag changes nothing.
__global__ __launch_bounds__(kBlock) void k_beam_sweep_pack(SensorTables tb, const uint4 *__restrict__ blocks, const uint32_t *__restrict__ wsum,
                                                            const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ block_counts,
                                                            uint32_t w_total, const float *__restrict__ pose, uint32_t aligned16, uint32_t deskew,
                                                            float4 *__restrict__ points, uint4 *__restrict__ hits, uint32_t *__restrict__ echo,
                                                            uint32_t *__restrict__ n_points, uint32_t capacity)
{
    __shared__ uint32_t s_part[kBlock / 64];
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t nq = tb.V * tb.naz;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    // the beam's count, the ray's table entries and the counts of the workgroups before this one: all requested up front
    const uint32_t c = q < nq ? cnt[q] : 0u;
    const uint32_t qq = q < nq ? q : 0u;
    const uint32_t v = qq / tb.naz, h = tb.az0 + (qq - v * tb.naz);
    const float st = tb.sin_theta[v], ctv = tb.cos_theta[v];
    const float2 cs = tb.cs_phi[h];
    uint32_t acc = 0;
    constexpr uint32_t kCountsAhead = 8;
    for (uint32_t r0 = threadIdx.x; r0 < blockIdx.x; r0 += kCountsAhead * kBlock) {
        uint32_t a[kCountsAhead];
#pragma unroll
        for (uint32_t k = 0; k < kCountsAhead; ++k) a[k] = r0 + k * kBlock < blockIdx.x ? block_counts[r0 + k * kBlock] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < kCountsAhead; ++k) acc += a[k];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    uint32_t upto = c;   // the records of this lane and the lanes before it in the wave
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t below = __shfl_up(upto, off);
        if (lane >= off) upto += below;
    }
    if (lane == 63u) { s_part[w] = acc; s_wave[w] = upto; }
    __syncthreads();
    uint32_t first = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (uint32_t k = 0; k < w; ++k) first += s_wave[k];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_points = first + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (!c) return;   // (past the barrier and the shuffles)
    const uint32_t dst = first + upto - c;
    const float dx = st * cs.x, dy = st * cs.y;
    float p[12];
    const bool carried = points && deskew && pose;
    if (carried) load_pose(pose, h, aligned16 != 0u, p);
#pragma unroll
    for (uint32_t i = 0; i < 3u; ++i) {
        if (i >= c || dst + i >= capacity) break;   // (dst + c <= K * the shard's rays <= capacity: the second never holds)
        const uint4 rec = blocks[3 * (size_t)q + i];
        const size_t at = (size_t)dst + i;
        const float r = __uint_as_float(rec.x);
        if (points) {
            float xyz[3];
            if (carried) {   // o_h + r * d' per axis, d' the nominal direction through the column's pose (ls_sweep.h)
                sweep_point(p, dx, dy, ctv, r, xyz);
            } else {         // the range the sensor reports along its axis: xyz = r * d with no sum (k_beam_pack)
                xyz[0] = r * dx; xyz[1] = r * dy; xyz[2] = r * ctv;
            }
            points[2 * at] = make_float4(xyz[0], xyz[1], xyz[2], 0.0f);
            points[2 * at + 1] = make_float4(beam_intensity_weighted(wsum[3 * (size_t)q + i], w_total), __int_as_float((int)v), 0.0f, 0.0f);
        }
        if (hits) hits[at] = make_uint4(v * tb.H + h, rec.y, rec.z, rec.x);
        if (echo) echo[at] = rec.w;
    }
}

}  // namespace

size_t beam_block_count(uint32_t nq) { return ((size_t)nq + kBlock - 1) / kBlock; }

void launch_beam_rays(hipStream_t s, const SensorTables &tb, const BeamPattern &pat, uint32_t S, void *rays)
{
    const dim3 grid((tb.naz * S + 63u) / 64u, (tb.V + kBeamRows - 1u) / kBeamRows);
    hipLaunchKernelGGL(k_beam_rays, grid, dim3(kBlock), 0, s, tb, pat, S, static_cast<float4 *>(rays));
}

void launch_beam_pack(hipStream_t s, const SensorTables &tb, const BeamPattern &pat, uint32_t S, float separation, uint32_t min_count,
                      uint32_t returns, const void *dense, void *blocks, uint32_t *cnt, uint32_t *block_counts, void *points32, void *hits,
                      uint32_t *echo, uint32_t *n_points, uint32_t capacity)
{
    const uint32_t nq = tb.V * tb.naz;
    uint32_t P = 1;
    while (P < S) P <<= 1;
    const uint32_t per_block = (kBlock / 64u) * (64u / P);
    hipLaunchKernelGGL(k_beam_reduce, dim3((nq + per_block - 1u) / per_block), dim3(kBlock), 0, s, static_cast<const uint4 *>(dense), nq, S, P, pat,
                       separation, min_count, returns, static_cast<uint4 *>(blocks), cnt);
    const dim3 grid((uint32_t)beam_block_count(nq));
    hipLaunchKernelGGL(k_beam_count, grid, dim3(kBlock), 0, s, static_cast<const uint32_t *>(cnt), nq, block_counts);
    hipLaunchKernelGGL(k_beam_pack, grid, dim3(kBlock), 0, s, tb, S, static_cast<const uint4 *>(blocks), static_cast<const uint32_t *>(cnt),
                       static_cast<const uint32_t *>(block_counts), static_cast<float4 *>(points32), static_cast<uint4 *>(hits), echo, n_points,
                       capacity);
}

void launch_beam_sweep_rays(hipStream_t s, const SensorTables &tb, const BeamPattern &pat, uint32_t S, const float *pose, void *rays)
{
    if (!pose) return launch_beam_rays(s, tb, pat, S, rays);   // at rest: the sub-rays of ls_trace_scene_beams
    const dim3 grid((tb.naz * S + 63u) / 64u, (tb.V + kBeamRows - 1u) / kBeamRows);
    hipLaunchKernelGGL(k_beam_sweep_rays, grid, dim3(kBlock), 0, s, tb, pat, S, pose, ((uintptr_t)pose & 15u) ? 0u : 1u, static_cast<float4 *>(rays));
}

void launch_beam_sweep_pack(hipStream_t s, const SensorTables &tb, const BeamPattern &pat, const BeamWeights &wts, uint32_t w_total, uint32_t S,
                            float separation, uint32_t min_count, uint32_t min_weight, uint32_t returns, const float *pose, bool deskew,
                            const void *dense, void *blocks, uint32_t *wsum, uint32_t *cnt, uint32_t *block_counts, void *points32, void *hits,
                            uint32_t *echo, uint32_t *n_points, uint32_t capacity)
{
    const uint32_t nq = tb.V * tb.naz;
    uint32_t P = 1;
    while (P < S) P <<= 1;
    const uint32_t per_block = (kBlock / 64u) * (64u / P);
    hipLaunchKernelGGL(k_beam_reduce_weighted, dim3((nq + per_block - 1u) / per_block), dim3(kBlock), 0, s, static_cast<const uint4 *>(dense), nq, S, P,
                       pat, wts, separation, min_count, min_weight, returns, static_cast<uint4 *>(blocks), wsum, cnt);
    const dim3 grid((uint32_t)beam_block_count(nq));
    hipLaunchKernelGGL(k_beam_count, grid, dim3(kBlock), 0, s, static_cast<const uint32_t *>(cnt), nq, block_counts);
    hipLaunchKernelGGL(k_beam_sweep_pack, grid, dim3(kBlock), 0, s, tb, static_cast<const uint4 *>(blocks), static_cast<const uint32_t *>(wsum),
                       static_cast<const uint32_t *>(cnt), static_cast<const uint32_t *>(block_counts), w_total, pose,
                       ((uintptr_t)pose & 15u) ? 0u : 1u, deskew ? 1u : 0u, static_cast<float4 *>(points32), static_cast<uint4 *>(hits), echo, n_points,
                       capacity);
}

}  // namespace ls
