// ls_return_model.h -- the sensor return model of ls_apply_return_model (include/lidarshooter_hip.h): from a
// valid hit (t, |d|, incidence cosine, reflectivity) to (kept / lost, noisy t', intensity).  ONE float32 operation sequence that
// the device (k_returns_eval, ls_returns.hip) and the host (ls_debug_return_model, ls_debug.cpp) both compile, with
// -ffp-contract=off -fno-fast-math: every operation rounds once, in the order written; no fmaf, no libm call (the caller's
// sqrtf gives len), so that the model can be restated on the host bit for bit.
//
//   1. r = t * len                                     the true range (len = |d|)
//   2. c = 1 | max(cos_inc, 0) | |cos_inc|             flags: none | LAMBERT | LAMBERT + TWO_SIDED
//   3. f = q * q, q = ref_range / max(r, ref_range)    (a true division; ref_range = 0: f = 1)
//   4. I = ((intensity_scale * rho) * c) * f, then min(I, intensity_max)
//   5. Philox4x32-10, key (seed, 0), counters (ray, frame_index, j, 0), j = 0, 1 -> a0..a3, b0..b3: keyed by the RAY, not by
//      the record's position -- any subset, order or azimuth shard draws what the full turn draws
//   6. dropped when dropout > 0 and (float)(b2 >> 8) * 2^-24 < dropout   (24 bits: the conversion and the product are exact)
//   7. z = (float)((int)S - 393210) * 2^-16, S = the sum of the twelve 16-bit halves of a0 a1 a2 a3 b0 b1 (Irwin-Hall: mean
//      12 * 65535 / 2, variance 12 * (65536^2 - 1) / 12 -> std 1 to 1e-9 after the scaling, tails to +-6; |S - 393210| < 2^24: exact)
//   8. t' = t + (sigma * z) / len, sigma = noise_sigma0 + noise_sigma1 * r   (both sigmas 0: t' = t, whatever z)
//   9. kept when range_min <= r <= range_max, I >= intensity_floor (a NaN I is lost), not dropped, t' > 0
#pragma once

#include <stdint.h>

#include "../../include/lidarshooter_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LS_RM_HD __host__ __device__ inline
#else
#define LS_RM_HD inline
#endif

namespace ls {

LS_RM_HD void rm_mulhilo(uint32_t a, uint32_t b, uint32_t *hi, uint32_t *lo)
{
    const uint64_t p = (uint64_t)a * (uint64_t)b;
    *hi = (uint32_t)(p >> 32);
    *lo = (uint32_t)p;
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), as in Random123
LS_RM_HD void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int round = 0; round < 10; ++round) {
        uint32_t hi0, lo0, hi1, lo1;
        rm_mulhilo(0xD2511F53u, c0, &hi0, &lo0);
        rm_mulhilo(0xCD9E8D57u, c2, &hi1, &lo1);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// nullptr when the model is usable, else what is wrong with it (ls_apply_return_model refuses it before any device call)
inline const char *return_model_invalid(const ls_return_model *m)
{
    if (!m) return "null return model";
    const float f[9] = {m->range_min, m->range_max, m->intensity_scale, m->ref_range, m->intensity_floor, m->intensity_max,
                        m->noise_sigma0, m->noise_sigma1, m->dropout};
    for (int i = 0; i < 9; ++i)
        if (f[i] != f[i]) return "return model: a field is NaN";
    if (m->range_min > m->range_max) return "return model: range_min > range_max";
    if (m->range_min < 0.0f || m->intensity_scale < 0.0f || m->ref_range < 0.0f || m->intensity_floor < 0.0f || m->noise_sigma0 < 0.0f ||
        m->noise_sigma1 < 0.0f)
        return "return model: a negative range_min, scale, ref_range, floor or sigma";
    if (m->dropout < 0.0f || m->dropout > 1.0f) return "return model: dropout outside [0, 1]";
    if (m->flags & ~(LS_RETURN_LAMBERT | LS_RETURN_TWO_SIDED)) return "return model: unknown flag bits";
    for (int i = 0; i < 5; ++i)
        if (m->reserved[i]) return "return model: reserved words must be 0";
    return nullptr;
}

// steps 1-9 above.  *t_out and *intensity are written whether the return is kept or lost.
LS_RM_HD bool return_model_eval(const ls_return_model &m, uint32_t ray, uint32_t frame_index, float t, float len, float cos_inc, float rho,
                                float *t_out, float *intensity)
{
    const float r = t * len;
    float c = 1.0f;
    if (m.flags & LS_RETURN_LAMBERT) {
        if (m.flags & LS_RETURN_TWO_SIDED) c = cos_inc < 0.0f ? -cos_inc : cos_inc;
        else c = cos_inc > 0.0f ? cos_inc : 0.0f;
    }
    float f = 1.0f;
    if (m.ref_range > 0.0f) {
        const float q = m.ref_range / (r > m.ref_range ? r : m.ref_range);
        f = q * q;
    }
    float I = ((m.intensity_scale * rho) * c) * f;
    if (I > m.intensity_max) I = m.intensity_max;

    const uint32_t key[2] = {m.seed, 0u};
    const uint32_t ca[4] = {ray, frame_index, 0u, 0u}, cb[4] = {ray, frame_index, 1u, 0u};
    uint32_t a[4], b[4];
    philox4x32_10(ca, key, a);
    philox4x32_10(cb, key, b);
    const bool dropped = m.dropout > 0.0f && (float)(b[2] >> 8) * (1.0f / 16777216.0f) < m.dropout;
    const uint32_t S = (a[0] & 0xFFFFu) + (a[0] >> 16) + (a[1] & 0xFFFFu) + (a[1] >> 16) + (a[2] & 0xFFFFu) + (a[2] >> 16) + (a[3] & 0xFFFFu) +
                       (a[3] >> 16) + (b[0] & 0xFFFFu) + (b[0] >> 16) + (b[1] & 0xFFFFu) + (b[1] >> 16);
    const float z = (float)((int)S - 393210) * (1.0f / 65536.0f);
    float tp = t;
    if (!(m.noise_sigma0 == 0.0f && m.noise_sigma1 == 0.0f)) {
        const float sigma = m.noise_sigma0 + m.noise_sigma1 * r;
        tp = t + (sigma * z) / len;
    }
    *t_out = tp;
    *intensity = I;
    return (m.range_min <= r) & (r <= m.range_max) & (I >= m.intensity_floor) & !dropped & (tp > 0.0f);
}

}  // namespace ls
