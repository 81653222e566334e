// ls_surface_sample.h -- the arithmetic of ls_sample_surface (include/lidarshooter_hip.h) that the kernels
// (k_surface_area, k_surface_block_sums, k_surface_prefix, k_surface_sample: ls_surface_sample.hip) and the host
// (ls_debug_surface_weights, ls_debug_surface_pick, ls_debug_surface_point: ls_debug.cpp; the descriptor's check) both compile: ONE
// float32 / integer sequence per triangle and per sample, and what ls_surface_sample.hip gives the host code of the call
// (ls_surface_sample_host.cpp).
//
// Everything float is float32 and every operation rounds once (the library is compiled with -ffp-contract=off); there is no fmaf.
// Per triangle i of the flat index, q_k its vertices in the output frame (ls_scene_tris.h's vertex path):
//   1. weight 0 for an unselected geometry, a free id, an index >= n_verts, a non-finite coordinate;
//   2. N = (q1 - q0) x (q2 - q0) as products and differences -- scene_tri_setup's form (ls_scene_grid.h), NOT attr_cross's fused one
//      (ls_hit_attr.h): the normal of a sample is not bit-equal to ls_hit_attributes' --; m = max |N_k|, weight 0 unless m > 0 and
//      finite; g = N / m; len = sqrtf((gx gx + gy gy) + gz gz); n = g / len; area a = (0.5f * m) * len, weight 0 unless a is finite.
//      A triangle of weight 0 has a = +0;
//   3. A = max_i a_i, as a maximum of bit patterns (a >= 0: the same order; it does not depend on the order of the triangles).
//      A == 0: W = 0, e = 0.  Otherwise A = f 2^E, f in [1, 2) (ilogbf, subnormals included), e = E - 30;
//   4. w_i = (uint64)floorf(ldexpf(a_i, -e)): the largest weight is in [2^30, 2^31); ldexpf is exact wherever its result is >= 1;
//   5. P[0] = 0, P[i + 1] = P[i] + w_i, W = P[n_tris] < 2^63: integer sums, the same bytes in any order;
//   6. sample j: Philox4x32-10, key (seed, 1), counter (lo32(j), hi32(j), 0, 0) -> x0 .. x3;
//   7. r = (x0 << 32) | x1, T = hi64(r W) < W; the triangle is the largest i < n_tris with P[i] <= T, so w_i > 0;
//   8. alpha = x2 >> 8, beta = x3 >> 8; alpha + beta > 2^24: alpha = 2^24 - alpha, beta = 2^24 - beta; gamma = 2^24 - alpha - beta;
//      u = (float)alpha 2^-24, v = (float)beta 2^-24, w = (float)gamma 2^-24, all exact;
//   9. p = ((w q0 + u q1) + v q2) per axis;
//  10. W == 0: every record is zeros with geom = 0xFFFFFFFF.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/lidarshooter_hip.h"
#include "ls_kernels.h"
#include "ls_grid_box.h"
#include "ls_return_model.h"

#if defined(__HIPCC__)
#define LS_SURF_HD __host__ __device__ __forceinline__
#else
#define LS_SURF_HD inline
#endif

namespace ls {

constexpr uint32_t kSurfaceTop = 1024;   // k_surface_sample, LDS-topped form: the entries of P staged per workgroup (+ 1: 8 KB)

// the descriptor as the kernels take it, with the call's transform next to it
struct SurfaceSample {
    uint64_t first;
    uint32_t n, seed;
    uint32_t has_xf, pad[3];
    float xf[12];   // sensor -> out, row-major 3 x 4 (read only with has_xf)
};

// what the call refuses of a descriptor and a transform (nullptr: none): the message of an LS_ERR_INVALID_ARGUMENT
inline const char *surface_sample_args_invalid(const ls_surface_sample_desc &d, const float *xf)
{
    if (d.flags & ~LS_SURFACE_SAMPLE_FLAGS) return "unknown flags";
    if (d.reserved[0] || d.reserved[1] || d.reserved[2]) return "reserved words must be 0";
    if (xf)
        for (int k = 0; k < 12; ++k)
            if (!isfinite(xf[k])) return "non-finite transform";
    return nullptr;
}

inline SurfaceSample surface_sample(const ls_surface_sample_desc &d, const float *sensor_to_out3x4)
{
    SurfaceSample v{};
    v.first = d.first_sample; v.n = d.n_samples; v.seed = d.seed;
    grid_set_xf(v, sensor_to_out3x4);
    return v;
}

// step 2 (and step 1's last case): the area of the triangle q (nine coordinates in the output frame) and its unit normal; +0 and a
// zero normal where one of their tests fails (an area that underflows is +0 as well, and keeps its normal)
LS_SURF_HD float surface_tri_area(const float *q, float *n)
{
    n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) finite &= (bool)isfinite(q[k]);
    if (!finite) return 0.0f;
    const float ax = q[3] - q[0], ay = q[4] - q[1], az = q[5] - q[2];
    const float bx = q[6] - q[0], by = q[7] - q[1], bz = q[8] - q[2];
    const float Nx = (ay * bz) - (az * by), Ny = (az * bx) - (ax * bz), Nz = (ax * by) - (ay * bx);
    const float m = fmaxf(fmaxf(fabsf(Nx), fabsf(Ny)), fabsf(Nz));
    if (!(m > 0.0f) || !isfinite(m)) return 0.0f;
    const float gx = Nx / m, gy = Ny / m, gz = Nz / m;
    const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
    const float a = (0.5f * m) * len;
    if (!isfinite(a)) return 0.0f;   // (a NaN component of N that fmaxf passed over ends here as well)
    n[0] = gx / len; n[1] = gy / len; n[2] = gz / len;
    return a;
}

// step 3: e from the bits of A
LS_SURF_HD int surface_exponent(uint32_t a_max_bits)
{
    float A;
    __builtin_memcpy(&A, &a_max_bits, 4);
    return a_max_bits ? ilogbf(A) - 30 : 0;
}

// step 4
LS_SURF_HD uint64_t surface_weight(float a, int e) { return (uint64_t)floorf(ldexpf(a, -e)); }

// the high 64 bits of a 128-bit product, through 32-bit halves
LS_SURF_HD uint64_t surface_mulhi(uint64_t a, uint64_t b)
{
    const uint64_t al = (uint32_t)a, ah = a >> 32, bl = (uint32_t)b, bh = b >> 32;
    const uint64_t ll = al * bl, lh = al * bh, hl = ah * bl, hh = ah * bh;
    const uint64_t mid = (ll >> 32) + (uint32_t)lh + (uint32_t)hl;   // (below 3 * 2^32)
    return hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
}

// step 6
LS_SURF_HD void surface_words(uint32_t seed, uint64_t j, uint32_t x[4])
{
    const uint32_t key[2] = {seed, 1u}, ctr[4] = {(uint32_t)j, (uint32_t)(j >> 32), 0u, 0u};
    philox4x32_10(ctr, key, x);
}

// step 7 between lo and hi, P[lo] <= T < P[hi]: at most 32 trips, whatever P holds
LS_SURF_HD uint32_t surface_bisect(const uint64_t *P, uint32_t lo, uint32_t hi, uint64_t T)
{
    for (int trip = 0; trip < 32 && hi - lo > 1u; ++trip) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (P[mid] <= T) lo = mid; else hi = mid;
    }
    return lo;
}

// step 8
LS_SURF_HD void surface_bary(uint32_t x2, uint32_t x3, float *u, float *v, float *w)
{
    uint32_t alpha = x2 >> 8, beta = x3 >> 8;
    if (alpha + beta > 0x1000000u) { alpha = 0x1000000u - alpha; beta = 0x1000000u - beta; }
    const uint32_t gamma = 0x1000000u - alpha - beta;
    *u = (float)alpha * (1.0f / 16777216.0f);
    *v = (float)beta * (1.0f / 16777216.0f);
    *w = (float)gamma * (1.0f / 16777216.0f);
}

// step 9
LS_SURF_HD void surface_point(const float *q, float u, float v, float w, float *p)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = ((w * q[a] + u * q[3 + a]) + v * q[6 + a]);
}

// ---- the launches of ls_surface_sample.hip -----------------------------------------------------------------------------------------

constexpr uint32_t kSurfaceBlock = 256;   // the workgroup of every kernel here, and the triangles behind one entry of the sums
inline uint32_t surface_blocks(uint32_t n_tris) { return n_tris ? (uint32_t)(((uint64_t)n_tris + kSurfaceBlock - 1) / kSurfaceBlock) : 1u; }

// one lane per triangle of the table (tri_first[geom] .. tri_first[geom + 1], n_table + 1 words; n_tris = tri_first[n_table]): the
// bits of a_i to area[1 + i], their maximum to area[0] (zero before the launch: the launch clears it on s first)
void launch_surface_area(hipStream_t s, const SurfaceSample &d, const AttrGeom *table, uint32_t n_table, const uint32_t *tri_first, uint32_t n_tris,
                         const uint8_t *select, uint32_t n_select, uint32_t *area);
// the weights from area, their exclusive prefix P[0 .. n_tris] (prefix; behind it surface_blocks(n_tris) pairs {sum, count} of
// scratch) and, with info != nullptr, the 16 bytes of the call's info
void launch_surface_prefix(hipStream_t s, const uint32_t *area, uint32_t n_tris, uint64_t *prefix, void *info);
// one lane per sample: three 16-byte stores per record.  lds_top: the first levels of the bisection run over kSurfaceTop + 1 evenly
// spaced entries of P staged in LDS (the same bytes either way)
void launch_surface_sample(hipStream_t s, const SurfaceSample &d, const AttrGeom *table, uint32_t n_table, const uint32_t *tri_first, uint32_t n_tris,
                           const uint64_t *prefix, bool lds_top, void *samples);

}  // namespace ls
