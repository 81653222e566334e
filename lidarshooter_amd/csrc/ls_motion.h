// ls_motion.h -- the arithmetic of ls_trace_scene_sweep_moving (include/lidarshooter_hip.h) that the kernel
// (k_trace_rays_moving, ls_moving.hip) and the host (ls_debug_motion_ray, ls_debug.cpp) both compile: ONE float32 operation
// sequence per (ray, moving geometry).  The gather over such a frame's records (ls_attr_moving.hip) rebuilds the same ray with it
// and carries a normal the other way (motion_normal, below).
//
// A motion record is 12 floats, row-major [Q | c]: p[4 i + j] = Q[i][j], p[4 i + 3] = c[i] -- the rigid displacement x_h = Q x_0 + c
// of a geometry at the moment a column fires, relative to where it was committed, in the handle's sensor frame.  A moved
// geometry is a moved ray: the ray (o, d) meets the displaced geometry where the ray (Q^T (o - c), Q^T d) meets the committed
// one, at the same t.  Q is taken to be a rotation (its transpose serves as its inverse):
//   e_i   = o_i - c_i
//   o_g,i = (Q[0][i] e_0 + Q[1][i] e_1) + Q[2][i] e_2          one difference, two sums, three products, each rounded once (the
//   d_g,i = (Q[0][i] d_0 + Q[1][i] d_1) + Q[2][i] d_2          library is compiled with -ffp-contract=off: no fused multiply-add)
//   ray   = (o_g, tmin 0, d_g, tmax 1e16)
// An identity record gives the ray back: x - 0 is x, 1 * x is x, 0 * y is a zero, and x + 0 is x.  A non-finite entry of a record
// leaves a non-finite origin or direction (0 * inf is a NaN): motion_ray_usable says no, and the geometry is invisible to the ray.
#pragma once

#include "ls_sweep.h"

namespace ls {

// the 32-byte lidarshooter::Ray record geometry g sees: the ray record `ray8` through the inverse of the motion record p
LS_SWEEP_HD void motion_ray(const float *p, const float *ray8, float *out8)
{
    const float e0 = ray8[0] - p[3], e1 = ray8[1] - p[7], e2 = ray8[2] - p[11];
    out8[0] = (p[0] * e0 + p[4] * e1) + p[8] * e2;
    out8[1] = (p[1] * e0 + p[5] * e1) + p[9] * e2;
    out8[2] = (p[2] * e0 + p[6] * e1) + p[10] * e2;
    out8[3] = 0.0f;
    out8[4] = (p[0] * ray8[4] + p[4] * ray8[5]) + p[8] * ray8[6];
    out8[5] = (p[1] * ray8[4] + p[5] * ray8[5]) + p[9] * ray8[6];
    out8[6] = (p[2] * ray8[4] + p[6] * ray8[5]) + p[10] * ray8[6];
    out8[7] = kSweepTmax;
}

// whether the geometry is tested at all: a finite origin, a finite direction that is not zero (what k_trace_rays asks of a ray)
LS_SWEEP_HD bool motion_ray_usable(const float *r)
{
    const float s = ((r[0] - r[0]) + (r[1] - r[1])) + (r[2] - r[2]);   // 0, or a NaN when an entry is not finite
    const float u = ((r[4] - r[4]) + (r[5] - r[5])) + (r[6] - r[6]);
    return s == 0.0f && u == 0.0f && (r[4] != 0.0f || r[5] != 0.0f || r[6] != 0.0f);
}

// ls_hit_attributes_moving (k_hit_attributes_moving, ls_attr_moving.hip; ls_debug_motion_normal): the way back for a direction.  The
// unit normal n_g found on the geometry where it was committed, carried forward by the motion record p into the sensor frame:
//   n_i = (Q[i][0] n_g,0 + Q[i][1] n_g,1) + Q[i][2] n_g,2      two sums, three products, each rounded once
// An identity record gives n_g back numerically (a -0 component may come back as +0: 0 * y + -0 is +0).  out3 may be n3.
LS_SWEEP_HD void motion_normal(const float *p, const float *n3, float *out3)
{
    const float n0 = n3[0], n1 = n3[1], n2 = n3[2];
    out3[0] = (p[0] * n0 + p[1] * n1) + p[2] * n2;
    out3[1] = (p[4] * n0 + p[5] * n1) + p[6] * n2;
    out3[2] = (p[8] * n0 + p[9] * n1) + p[10] * n2;
}

}  // namespace ls
