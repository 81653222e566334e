// ls_velocity.h -- the arithmetic of ls_hit_velocities (include/lidarshooter_hip.h) that the kernel
// (k_hit_velocities, ls_velocity.hip) and the host (ls_debug_hit_velocity, ls_debug.cpp) both compile: ONE float32 operation
// sequence per valid hit record.
//
// A twist record is 6 floats [w | u]: the spatial twist of a rigid body at the moment a column fires, in the handle's sensor frame
// as the scene was committed (the frame of the pose and motion tables).  A material point of the body that is at x at that moment
// moves with v(x) = u + w x x:
//   v_0 = u_0 + (w_1 x_2 - w_2 x_1)
//   v_1 = u_1 + (w_2 x_0 - w_0 x_2)          two products, one difference, one sum per axis, each rounded once (the library is
//   v_2 = u_2 + (w_0 x_1 - w_1 x_0)          compiled with -ffp-contract=off: no fused multiply-add)
// No record: the body is at rest, v = (+0, +0, +0) and nothing is evaluated.  A pure translation (w = 0) gives u back numerically.
// A non-finite entry leaves non-finite components; nothing here looks at them.
//
// A hit record: with (o, c) the ray the record's COLUMN cast (ls_debug_sweep_ray's record; o = +0 and c the nominal direction without
// a pose table) and t the record's,
//   P_i    = o_i + t c_i                                     the hit point at its own instant, in the frame-start frame
//   v_s    = v(P) of the twist of the geometry that was hit   the surface's velocity
//   v_o    = v(o) of the sensor's twist                       the velocity of the sensor's origin
//   rel_i  = v_s,i - v_o,i
//   len    = sqrtf((c_0 c_0 + c_1 c_1) + c_2 c_2)             the return model's len
//   radial = ((rel_0 c_0 + rel_1 c_1) + rel_2 c_2) / len      the range rate: positive, the range grows
// The range rate of a material point is (v_p - v_o) . c^: a sensor that turns about its own origin contributes nothing.
#pragma once

#include <math.h>

#include "ls_sweep.h"

namespace ls {

// v(x) of the twist record tw; moving false: the body is at rest and tw is not read
LS_SWEEP_HD void twist_velocity(bool moving, const float *tw, const float *x, float *v3)
{
    if (!moving) {
        v3[0] = 0.0f; v3[1] = 0.0f; v3[2] = 0.0f;
        return;
    }
    v3[0] = tw[3] + (tw[1] * x[2] - tw[2] * x[1]);
    v3[1] = tw[4] + (tw[2] * x[0] - tw[0] * x[2]);
    v3[2] = tw[5] + (tw[0] * x[1] - tw[1] * x[0]);
}

// the seven floats of ls_hit_velocities' record for a valid hit at t along the cast ray cast8 (origin xyz, tmin, direction xyz,
// tmax): v_s xyz, radial, v_o xyz; sensor_tw / geom_tw: the twist records of the column, read only where sensor_moves / geom_moves
// says there is one (flags, not null pointers: the kernel's records stay in registers)
LS_SWEEP_HD void hit_velocity(const float *cast8, float t, bool sensor_moves, const float *sensor_tw, bool geom_moves, const float *geom_tw,
                              float *out7)
{
    const float *o = cast8, *c = cast8 + 4;
    const float P[3] = {o[0] + t * c[0], o[1] + t * c[1], o[2] + t * c[2]};
    float vs[3], vo[3];
    twist_velocity(geom_moves, geom_tw, P, vs);
    twist_velocity(sensor_moves, sensor_tw, o, vo);
    const float r0 = vs[0] - vo[0], r1 = vs[1] - vo[1], r2 = vs[2] - vo[2];
    const float len = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    out7[0] = vs[0]; out7[1] = vs[1]; out7[2] = vs[2];
    out7[3] = ((r0 * c[0] + r1 * c[1]) + r2 * c[2]) / len;
    out7[4] = vo[0]; out7[5] = vo[1]; out7[6] = vo[2];
}

}  // namespace ls
