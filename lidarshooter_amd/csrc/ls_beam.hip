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

}  // namespace ls
