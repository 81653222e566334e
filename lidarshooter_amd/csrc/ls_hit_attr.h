// ls_hit_attr.h -- hit_attributes_on_triangle: the surface attributes of a ray / triangle hit (geometric normal, incidence
// cosine, Embree's barycentrics, the hit point), ONE float32 operation sequence that the device (k_hit_attributes,
// ls_attr.hip) and the host (ls_debug_hit_attributes_on_triangle, ls_debug.cpp) both compile, so that the definition of
// ls_hit_attributes can be restated on the host bit for bit.  Compiled with -ffp-contract=off -fno-fast-math on both sides:
// every operation rounds once, in the order written; the fused multiply-adds are the explicit fmaf calls of tri_test_org
// (ls_device.h), nothing else is fused; quotients and square roots are the correctly rounded ones.
//
//   1. the test: tri_test_org's sequence (e1 = v0 - v1, e2 = v2 - v0, Ng = cross(e2, e1), C = v0 - o, R = cross(C, d),
//      den, U, V, T) -- t bit-equal to lso_tri_intersect, and with o = 0 to the frame's test;
//   2. u = U / absDen, v = V / absDen (Embree's: the hit point is (1 - u - v) v0 + u v1 + v v2);
//   3. m = max |Ng.k|, g = Ng / m, len = sqrtf((gx gx + gy gy) + gz gz), n = g / len -- Ng = (v1 - v0) x (v2 - v0), Embree's
//      Ng direction; the pre-scaling keeps triangles of edge 1e-18 and 1e15 finite;
//   4. cos_inc = -((nx dx + ny dy) + nz dz) / sqrtf((dx dx + dy dy) + dz dz), clamped to [-1, 1];
//   5. p = o + t d per axis (one product, one sum).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LS_ATTR_HD __host__ __device__ inline
#else
#define LS_ATTR_HD inline
#endif

namespace ls {

LS_ATTR_HD uint32_t attr_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
LS_ATTR_HD float attr_xor_sign(float f, uint32_t s) { const uint32_t u = attr_bits(f) ^ s; float r; memcpy(&r, &u, 4); return r; }
// Embree's cross and dot (ls_device.h: cross_fma, dot_fma)
LS_ATTR_HD void attr_cross(const float *a, const float *b, float *c)
{
    c[0] = fmaf(a[1], b[2], -(a[2] * b[1]));
    c[1] = fmaf(a[2], b[0], -(a[0] * b[2]));
    c[2] = fmaf(a[0], b[1], -(a[1] * b[0]));
}
LS_ATTR_HD float attr_dot(const float *a, const float *b) { return fmaf(a[0], b[0], fmaf(a[1], b[1], a[2] * b[2])); }

// o, d, v0, v1, v2: three floats each.  true: the test passes; *t, and out9 = nx ny nz cos_inc u v px py pz.  false: nothing
// is written.
LS_ATTR_HD bool hit_attributes_on_triangle(const float *o, const float *d, const float *v0, const float *v1, const float *v2, float *t,
                                           float *out9)
{
    const float e1[3] = {v0[0] - v1[0], v0[1] - v1[1], v0[2] - v1[2]};
    const float e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const float C[3] = {v0[0] - o[0], v0[1] - o[1], v0[2] - o[2]};
    float Ng[3], R[3];
    attr_cross(e2, e1, Ng);
    attr_cross(C, d, R);
    const float den = attr_dot(Ng, d);
    const float absDen = fabsf(den);
    const uint32_t sgn = attr_bits(den) & 0x80000000u;
    const float U = attr_xor_sign(attr_dot(R, e2), sgn);
    const float V = attr_xor_sign(attr_dot(R, e1), sgn);
    const float T = attr_xor_sign(attr_dot(Ng, C), sgn);
    const bool ok = (den != 0.0f) & (U >= 0.0f) & (V >= 0.0f) & (U + V <= absDen) & (absDen * 0.0f < T) & (T <= absDen * INFINITY);
    if (!ok) return false;
    const float tt = T / absDen;
    if (!(tt < INFINITY)) return false;
    *t = tt;
    const float m = fmaxf(fmaxf(fabsf(Ng[0]), fabsf(Ng[1])), fabsf(Ng[2]));
    const float gx = Ng[0] / m, gy = Ng[1] / m, gz = Ng[2] / m;
    const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
    const float nx = gx / len, ny = gy / len, nz = gz / len;
    float c = -((nx * d[0] + ny * d[1]) + nz * d[2]) / sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    c = c > 1.0f ? 1.0f : c;
    c = c < -1.0f ? -1.0f : c;
    out9[0] = nx; out9[1] = ny; out9[2] = nz;
    out9[3] = c;
    out9[4] = U / absDen;
    out9[5] = V / absDen;
    out9[6] = o[0] + tt * d[0];
    out9[7] = o[1] + tt * d[1];
    out9[8] = o[2] + tt * d[2];
    return true;
}

}  // namespace ls
