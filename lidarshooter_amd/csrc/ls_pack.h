// ls_pack.h -- the pieces of the ordered pack that the scan frames and the return model share (device only): k_sweep_count +
// k_sweep_pack (ls_sweep.hip), k_beam_count + k_beam_pack / k_beam_sweep_pack (ls_beam.hip), k_returns_eval + k_returns_pack
// (ls_returns.hip), k_returns_eval_moving (ls_attr_moving.hip).
//
// The pack of a frame (k_rowcount + k_pack, ls_kernels.hip), one lane per item, 0..n records per lane: a count kernel stores the
// records of every 256 items (block_count_store); the pack kernel adds up the counts of the workgroups before its own
// (counts_before), ranks its records inside the wave -- a ballot for 0 / 1 per lane, wave_inclusive_sum for more -- and across its
// four waves (pack_wave_base), and writes there: the items' order is kept, no atomic append, no workgroup waits for another.
// Every function here is called by all 256 lanes of a workgroup (they hold a barrier or a shuffle).
#pragma once

#include "ls_device.h"

namespace ls {
namespace {

// x summed over the 64 lanes of the wave, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// x summed over this lane and the lanes before it in the wave
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t x, uint32_t lane)
{
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t below = __shfl_up(x, off);
        if (lane >= off) x += below;
    }
    return x;
}

// the count tail: block_counts[blockIdx.x] = the records of this workgroup; wave_total: those of the lane's wave
__device__ __forceinline__ void block_count_store(uint32_t wave_total, uint32_t *block_counts)
{
    __shared__ uint32_t s_cnt[kBlock / 64];
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// this wave's share of block_counts[0 .. before), before <= blockIdx.x: the four waves' values add up to the records ahead of the
// workgroup.  Eight guarded loads are requested before the first is added; one trip covers 2048 workgroups.
__device__ __forceinline__ uint32_t counts_before(const uint32_t *block_counts, uint32_t before)
{
    uint32_t acc = 0;
    constexpr uint32_t kCountsAhead = 8;
    for (uint32_t r0 = threadIdx.x; r0 < before; r0 += kCountsAhead * kBlock) {
        uint32_t c[kCountsAhead];
#pragma unroll
        for (uint32_t k = 0; k < kCountsAhead; ++k) c[k] = r0 + k * kBlock < before ? block_counts[r0 + k * kBlock] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < kCountsAhead; ++k) acc += c[k];
    }
    return wave_sum(acc);
}

// the position of the first record of the lane's wave.  acc: counts_before's value; wave_total: the records of the wave, valid in
// lane publisher_lane (0 after a ballot, 63 after a scan); last: this is the workgroup that writes the total to *n_total.
__device__ __forceinline__ uint32_t pack_wave_base(uint32_t acc, uint32_t wave_total, uint32_t publisher_lane, bool last, uint32_t *n_total)
{
    __shared__ uint32_t s_part[kBlock / 64];
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (lane == publisher_lane) { s_part[w] = acc; s_wave[w] = wave_total; }
    __syncthreads();
    uint32_t base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (uint32_t k = 0; k < w; ++k) base += s_wave[k];
    if (last && threadIdx.x == 0) *n_total = base + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    return base;
}

}  // namespace
}  // namespace ls
