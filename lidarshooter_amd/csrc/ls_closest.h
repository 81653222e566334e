// ls_closest.h -- closest_on_triangle: the closest point of a triangle to a point, ONE float32 operation sequence that
// the device (k_closest_points, ls_points.hip) and the host (ls_debug_closest_on_triangle, ls_debug.cpp) both compile, so
// that a brute force on the host reproduces the device's answer bit for bit.  Compiled with -ffp-contract=off
// -fno-fast-math on both sides: every operation below rounds once, in the order written; no fmaf; the quotients and the
// reciprocal are true (correctly rounded) divisions.
//
// Ericson's seven regions (Real-Time Collision Detection, 5.1.5): vertex A, vertex B, edge AB, vertex C, edge AC, edge BC,
// face, tested in that order.  Dot products are (x*x + y*y) + z*z.  Two additions to the textbook form, both so that the
// returned q is a point of the triangle (up to a few ulps of the coordinates) whatever the rounding did -- the hierarchy
// walk prunes on "no point of this box's triangles is nearer than", which only holds for such a q:
//   * a triangle whose normal n = ab x ac has n.n == 0, not finite or NaN (zero area -- a mesh scaled to nothing --, a
//     non-finite corner) is skipped: d2 = +inf, q = 0;
//   * in the face region the three barycentric numerators are clamped at 0 before they are normalised (rounding can leave
//     one of them a hair below 0 next to an edge; on a needle, far below).
// d2 = |p - q|^2 from the returned q itself.  A caller counts the triangle when d2 is finite (and within its radius).
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LS_CLOSEST_HD __host__ __device__ inline
#else
#define LS_CLOSEST_HD inline
#endif

namespace ls {

LS_CLOSEST_HD float closest_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// p, a, b, c: three floats each; q[3] and *d2 out
LS_CLOSEST_HD void closest_on_triangle(const float *p, const float *a, const float *b, const float *c, float *q, float *d2)
{
    const float abx = b[0] - a[0], aby = b[1] - a[1], abz = b[2] - a[2];
    const float acx = c[0] - a[0], acy = c[1] - a[1], acz = c[2] - a[2];
    const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const float nn = closest_dot(nx, ny, nz, nx, ny, nz);
    q[0] = 0.0f; q[1] = 0.0f; q[2] = 0.0f;
    *d2 = INFINITY;
    if (!(nn > 0.0f && nn < INFINITY)) return;
    float qx, qy, qz;
    const float apx = p[0] - a[0], apy = p[1] - a[1], apz = p[2] - a[2];
    const float d1 = closest_dot(abx, aby, abz, apx, apy, apz);
    const float d2a = closest_dot(acx, acy, acz, apx, apy, apz);
    const float bpx = p[0] - b[0], bpy = p[1] - b[1], bpz = p[2] - b[2];
    const float d3 = closest_dot(abx, aby, abz, bpx, bpy, bpz);
    const float d4 = closest_dot(acx, acy, acz, bpx, bpy, bpz);
    const float cpx = p[0] - c[0], cpy = p[1] - c[1], cpz = p[2] - c[2];
    const float d5 = closest_dot(abx, aby, abz, cpx, cpy, cpz);
    const float d6 = closest_dot(acx, acy, acz, cpx, cpy, cpz);
    float vc = d1 * d4 - d3 * d2a;
    float vb = d5 * d2a - d1 * d6;
    float va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0f && d2a <= 0.0f) {                                   // vertex A
        qx = a[0]; qy = a[1]; qz = a[2];
    } else if (d3 >= 0.0f && d4 <= d3) {                               // vertex B
        qx = b[0]; qy = b[1]; qz = b[2];
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {               // edge AB
        const float v = d1 / (d1 - d3);
        qx = a[0] + abx * v; qy = a[1] + aby * v; qz = a[2] + abz * v;
    } else if (d6 >= 0.0f && d5 <= d6) {                               // vertex C
        qx = c[0]; qy = c[1]; qz = c[2];
    } else if (vb <= 0.0f && d2a >= 0.0f && d6 <= 0.0f) {              // edge AC
        const float w = d2a / (d2a - d6);
        qx = a[0] + acx * w; qy = a[1] + acy * w; qz = a[2] + acz * w;
    } else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) { // edge BC
        const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        qx = b[0] + (c[0] - b[0]) * w; qy = b[1] + (c[1] - b[1]) * w; qz = b[2] + (c[2] - b[2]) * w;
    } else {                                                           // face
        va = va > 0.0f ? va : 0.0f;
        vb = vb > 0.0f ? vb : 0.0f;
        vc = vc > 0.0f ? vc : 0.0f;
        const float denom = 1.0f / ((va + vb) + vc);
        const float v = vb * denom, w = vc * denom;
        qx = (a[0] + abx * v) + acx * w; qy = (a[1] + aby * v) + acy * w; qz = (a[2] + abz * v) + acz * w;
    }
    const float dx = p[0] - qx, dy = p[1] - qy, dz = p[2] - qz;
    q[0] = qx; q[1] = qy; q[2] = qz;
    *d2 = closest_dot(dx, dy, dz, dx, dy, dz);
}

}  // namespace ls
