// ls_beam.h -- the arithmetic and the echo logic of ls_trace_scene_beams (include/lidarshooter_hip.h) that the
// kernels (ls_beam.hip) and the host (ls_debug_beam_ray, ls_debug_beam_echoes, ls_debug.cpp) both compile.
//
// The sub-ray.  For a ray of the raster with table entries st, ct, (cphi, sphi):
//   d = (st cphi, st sphi, ct)                 the nominal direction, the factor-table products of the frame kernels
//   u = (-sphi, cphi, 0)                       the tangent along the ring
//   w = (-(ct cphi), -(ct sphi), st)           the tangent towards higher elevation
//   d_s,i = (d_i + a_s u_i) + b_s w_i          two sums, two products, each rounded once (the library is compiled with
//   ray   = (origin 0, tmin 0, d_s, tmax 1e16) -ffp-contract=off: no fused multiply-add); a component -0 becomes +0
// The sample (0, 0, k) gives d: 0 * x is a zero, and x + 0 is x.
//
// The echoes of a beam.  Every sub-hit has the key (bits(r) << 8) | s, r = t_s * k_s >= 0 (bit order is float order), a miss all
// ones; in ascending key order -- (r, s) ascending, the misses last -- an echo starts at position 0 and wherever
// r_j - r_{j-1} > echo_separation.  beam_select() takes the start positions as a bit mask and the number of sub-hits and picks
// FIRST / LAST / STRONGEST among the echoes with at least min_count members: plain integer code, the same on both sides.
#pragma once

#include <stdint.h>

#include "../../include/lidarshooter_hip.h"

#if defined(__HIPCC__)
#define LS_BEAM_HD __host__ __device__ __forceinline__
#else
#define LS_BEAM_HD inline
#endif

namespace ls {

constexpr float kBeamTmax = 1e16f;            // the tmax of every ray the library generates (ls_sweep.h)
constexpr uint32_t kBeamMaxSamples = 64;      // one wave holds a beam
constexpr uint32_t kBeamMaxRays = 1u << 27;   // sub-rays of one call
constexpr unsigned long long kBeamMiss = ~0ull;

// the pattern as the kernels take it: by value, 768 bytes of kernel arguments
struct BeamPattern {
    float a[kBeamMaxSamples], b[kBeamMaxSamples], k[kBeamMaxSamples];
};

LS_BEAM_HD float beam_plus_zero(float x) { return x == 0.0f ? 0.0f : x; }

// the 32-byte lidarshooter::Ray record of sample (a, b) of the ray with table entries st, ct, (cphi, sphi)
LS_BEAM_HD void beam_ray(float st, float ct, float cphi, float sphi, float a, float b, float *ray8)
{
    const float dx = st * cphi, dy = st * sphi, dz = ct;
    const float ux = -sphi, uy = cphi, uz = 0.0f;
    const float wx = -(ct * cphi), wy = -(ct * sphi), wz = st;
    ray8[0] = 0.0f;
    ray8[1] = 0.0f;
    ray8[2] = 0.0f;
    ray8[3] = 0.0f;
    ray8[4] = beam_plus_zero((dx + a * ux) + b * wx);
    ray8[5] = beam_plus_zero((dy + a * uy) + b * wy);
    ray8[6] = beam_plus_zero((dz + a * uz) + b * wz);
    ray8[7] = kBeamTmax;
}

LS_BEAM_HD uint32_t beam_float_bits(float x)
{
    union { float f; uint32_t u; } c;
    c.f = x;
    return c.u;
}
LS_BEAM_HD float beam_bits_float(uint32_t u)
{
    union { float f; uint32_t u; } c;
    c.u = u;
    return c.f;
}

// the key of a sub-hit of sample s at range r (>= 0)
LS_BEAM_HD unsigned long long beam_key(float r, uint32_t s) { return ((unsigned long long)beam_float_bits(r) << 8) | s; }
LS_BEAM_HD float beam_key_range(unsigned long long key) { return beam_bits_float((uint32_t)(key >> 8)); }
LS_BEAM_HD uint32_t beam_key_sample(unsigned long long key) { return (uint32_t)(key & 0xFFu); }

// whether the sub-hit `key` at position j of the ascending order starts an echo; prev: the key at position j - 1
LS_BEAM_HD bool beam_starts_echo(unsigned long long prev, unsigned long long key, uint32_t j, float separation)
{
    if (key == kBeamMiss) return false;
    return j == 0 || beam_key_range(key) - beam_key_range(prev) > separation;
}

LS_BEAM_HD uint32_t beam_ctz64(unsigned long long m) { return (uint32_t)__builtin_ctzll(m); }   // (m != 0)

// one selected echo: the kinds it was selected as (bits 0-2), its member count (bits 8-14), the POSITION of its nearest member
// in the ascending order (bits 16-21) -- the echo word of the record once the position is replaced by that member's sample
LS_BEAM_HD uint32_t beam_word(uint32_t kinds, uint32_t count, uint32_t where) { return kinds | (count << 8) | (where << 16); }
LS_BEAM_HD uint32_t beam_word_count(uint32_t w) { return (w >> 8) & 0x7Fu; }
LS_BEAM_HD uint32_t beam_word_where(uint32_t w) { return (w >> 16) & 0x3Fu; }

// The returns of a beam.  starts: bit j set when position j of the ascending order starts an echo (bit 0 whenever n_hits > 0);
// n_hits: the number of sub-hits, positions 0 .. n_hits - 1.  An echo reaches from its start to the next start (or n_hits), and
// is detectable with at least min_count members.  Among the detectable ones FIRST is the nearest, LAST the farthest, STRONGEST
// the one with the most members (the nearer of equals).  -> n, the number of distinct selected echoes, 0 .. 3, and their words in
// ascending range (position) order in w0, w1, w2 (0 beyond n).  No array, no pointer: registers on the device.
struct BeamReturns {
    uint32_t n, w0, w1, w2;
};
LS_BEAM_HD BeamReturns beam_select(unsigned long long starts, uint32_t n_hits, uint32_t min_count, uint32_t returns)
{
    uint32_t first_at = 0, first_n = 0, last_at = 0, last_n = 0, best_at = 0, best_n = 0;
    while (starts) {
        const uint32_t at = beam_ctz64(starts);
        starts &= starts - 1ull;
        const uint32_t n = (starts ? beam_ctz64(starts) : n_hits) - at;
        if (n < min_count) continue;
        if (!first_n) { first_at = at; first_n = n; }
        last_at = at;
        last_n = n;
        if (n > best_n) { best_at = at; best_n = n; }   // (ascending range: an equal count later on does not replace it)
    }
    BeamReturns out = {0u, 0u, 0u, 0u};
    if (!first_n) return out;
    uint32_t wf = (returns & LS_BEAM_FIRST) ? beam_word(LS_BEAM_FIRST, first_n, first_at) : 0u;
    uint32_t ws = (returns & LS_BEAM_STRONGEST) ? beam_word(LS_BEAM_STRONGEST, best_n, best_at) : 0u;
    uint32_t wl = (returns & LS_BEAM_LAST) ? beam_word(LS_BEAM_LAST, last_n, last_at) : 0u;
    // first_at <= best_at <= last_at: the three are in ascending range; equal positions become one record
    if (wf && ws && first_at == best_at) { wf |= LS_BEAM_STRONGEST; ws = 0u; }
    if (wl && ws && best_at == last_at) { ws |= LS_BEAM_LAST; wl = 0u; }
    if (wl && wf && first_at == last_at) { wf |= LS_BEAM_LAST; wl = 0u; }   // (then best_at is there too: ws went into wf)
    out.n = (wf ? 1u : 0u) + (ws ? 1u : 0u) + (wl ? 1u : 0u);
    out.w0 = wf ? wf : ws ? ws : wl;
    out.w1 = wf ? (ws ? ws : wl) : (ws ? wl : 0u);
    out.w2 = wf && ws ? wl : 0u;
    return out;
}

// the intensity of an echo of n members out of S samples: the frame's constant when every sample is in it
LS_BEAM_HD float beam_intensity(uint32_t n, uint32_t S) { return (64.0f * (float)n) / (float)S; }

// ---- ls_trace_scene_beams_sweep: weighted echoes.  Sample s weighs w_s, an integer in 1..65535; the strength of
// an echo is W_e, the sum of its members' weights -- exact, independent of the order, at most 64 * 65535 < 2^24 and so exact as a
// float.  An echo is detectable with n_e >= min_count members AND W_e >= min_weight; STRONGEST is the largest W_e, the nearer of
// equals.  k_beam_reduce_weighted gives every position of the ascending order a lane and ls_debug_beam_echoes_weighted a loop
// turn; both run the per-position functions below and then beam_select_weighted.

// the weights as the kernels take them: by value, 128 bytes of kernel arguments; every entry beyond the samples is 0
struct BeamWeights {
    uint16_t w[kBeamMaxSamples];
};

// the end (one past the last position) of the echo that starts at position `at`: the next start, or n_hits
LS_BEAM_HD uint32_t beam_echo_end(unsigned long long starts, uint32_t n_hits, uint32_t at)
{
    const unsigned long long later = starts & ~((2ull << at) - 1ull);   // (at = 63: 2 << 63 is 0, no later position)
    return later ? beam_ctz64(later) : n_hits;
}

LS_BEAM_HD bool beam_detectable(uint32_t n, uint32_t W, uint32_t min_count, uint32_t min_weight) { return n >= min_count && W >= min_weight; }

// what the maximum is taken over: the larger W_e wins, among equals the lower position; 0 stands for no echo (W_e >= 1)
LS_BEAM_HD uint32_t beam_strength(uint32_t W, uint32_t at) { return (W << 6) | (63u - at); }
LS_BEAM_HD uint32_t beam_strength_where(uint32_t strength) { return 63u - (strength & 63u); }

// beam_select with the detectable echoes and the strongest of them found by the caller.  starts, n_hits: as for beam_select;
// detectable: the start positions of the detectable echoes; best_at: the start of the strongest one (read only when there is a
// detectable echo).  The words carry the member count, as beam_select's do; the caller looks W_e up at the word's position.
LS_BEAM_HD BeamReturns beam_select_weighted(unsigned long long starts, uint32_t n_hits, unsigned long long detectable, uint32_t best_at,
                                            uint32_t returns)
{
    BeamReturns out = {0u, 0u, 0u, 0u};
    if (!detectable) return out;
    const uint32_t first_at = beam_ctz64(detectable), last_at = 63u - (uint32_t)__builtin_clzll(detectable);
    const uint32_t first_n = beam_echo_end(starts, n_hits, first_at) - first_at, last_n = beam_echo_end(starts, n_hits, last_at) - last_at,
                   best_n = beam_echo_end(starts, n_hits, best_at) - best_at;
    uint32_t wf = (returns & LS_BEAM_FIRST) ? beam_word(LS_BEAM_FIRST, first_n, first_at) : 0u;
    uint32_t ws = (returns & LS_BEAM_STRONGEST) ? beam_word(LS_BEAM_STRONGEST, best_n, best_at) : 0u;
    uint32_t wl = (returns & LS_BEAM_LAST) ? beam_word(LS_BEAM_LAST, last_n, last_at) : 0u;
    // first_at <= best_at <= last_at: the three are in ascending range; equal positions become one record (as in beam_select)
    if (wf && ws && first_at == best_at) { wf |= LS_BEAM_STRONGEST; ws = 0u; }
    if (wl && ws && best_at == last_at) { ws |= LS_BEAM_LAST; wl = 0u; }
    if (wl && wf && first_at == last_at) { wf |= LS_BEAM_LAST; wl = 0u; }
    out.n = (wf ? 1u : 0u) + (ws ? 1u : 0u) + (wl ? 1u : 0u);
    out.w0 = wf ? wf : ws ? ws : wl;
    out.w1 = wf ? (ws ? ws : wl) : (ws ? wl : 0u);
    out.w2 = wf && ws ? wl : 0u;
    return out;
}

// the intensity of an echo of strength W out of W_total, the sum of all S weights: (64 n) / S with unit weights, beam_intensity's bits
LS_BEAM_HD float beam_intensity_weighted(uint32_t W, uint32_t W_total) { return (64.0f * (float)W) / (float)W_total; }

// nullptr when the weights (nullptr: every sample weighs 1) of S samples can be used, else what is wrong with them
inline const char *beam_weights_invalid(const uint32_t *weights, uint32_t S)
{
    if (!weights) return nullptr;
    for (uint32_t s = 0; s < S; ++s)
        if (weights[s] < 1u || weights[s] > 65535u) return "beam weights: a weight outside 1..65535";
    return nullptr;
}

// the weights by value (nullptr: 1 each) and their sum W_total
inline BeamWeights beam_weights_by_value(const uint32_t *weights, uint32_t S, uint32_t *total)
{
    BeamWeights out = {};
    *total = 0u;
    for (uint32_t s = 0; s < S; ++s) {
        out.w[s] = (uint16_t)(weights ? weights[s] : 1u);
        *total += out.w[s];
    }
    return out;
}

// nullptr when the model can be traced over shard_rays rays into `capacity` records, else what is wrong with it; *status:
// LS_ERR_INVALID_ARGUMENT, or LS_ERR_OUT_OF_RANGE for more than 2^27 sub-rays (an otherwise valid call)
inline const char *beam_model_invalid(const ls_beam_model *m, uint32_t shard_rays, uint32_t capacity, int *status)
{
    *status = LS_ERR_INVALID_ARGUMENT;
    if (!m) return "null beam model";
    if (!m->pattern) return "beam model: null pattern";
    if (m->n_samples < 1u || m->n_samples > kBeamMaxSamples) return "beam model: n_samples outside 1..64";
    if (!m->returns || (m->returns & ~(uint32_t)(LS_BEAM_FIRST | LS_BEAM_LAST | LS_BEAM_STRONGEST))) return "beam model: no return bit, or unknown ones";
    if (m->min_count < 1u || m->min_count > m->n_samples) return "beam model: min_count outside 1..n_samples";
    if (!(m->echo_separation >= 0.0f)) return "beam model: a NaN or negative echo_separation";
    for (int i = 0; i < 4; ++i)
        if (m->reserved[i]) return "beam model: non-zero reserved words";
    for (uint32_t s = 0; s < m->n_samples; ++s) {
        const float a = m->pattern[3 * s], b = m->pattern[3 * s + 1], k = m->pattern[3 * s + 2];
        // (x - x is 0 for a finite x, NaN otherwise)
        if (a - a != 0.0f || b - b != 0.0f || k - k != 0.0f) return "beam model: a non-finite pattern entry";
        if (!(k > 0.0f)) return "beam model: a pattern's k must be positive";
    }
    const uint32_t K = ((m->returns >> 0) & 1u) + ((m->returns >> 1) & 1u) + ((m->returns >> 2) & 1u);
    if ((unsigned long long)capacity < (unsigned long long)K * shard_rays) return "capacity below the returns per beam times the shard's ray count";
    if ((unsigned long long)shard_rays * m->n_samples > kBeamMaxRays) {
        *status = LS_ERR_OUT_OF_RANGE;
        return "too many sub-rays in one call (the shard's rays times n_samples above 2^27)";
    }
    return nullptr;
}

}  // namespace ls
