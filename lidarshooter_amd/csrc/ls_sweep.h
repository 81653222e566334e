// ls_sweep.h -- the arithmetic of ls_trace_scene_sweep (include/lidarshooter_hip.h) that the kernels
// (ls_sweep.hip) and the host (ls_debug_sweep_ray, ls_debug.cpp) both compile: ONE float32 operation sequence per ray.
//
// A column's pose is 12 floats, row-major [R | o]: p[4 i + j] = R[i][j], p[4 i + 3] = o[i] -- the sensor at the moment the column
// fires, in the handle's sensor frame.  A nominal direction d (the factor-table products of the frame kernels) becomes
//   d'_i = (R[i][0] dx + R[i][1] dy) + R[i][2] dz          two sums, three products, each rounded once (the library is
//   ray   = (o, tmin 0, d', tmax 1e16)                      compiled with -ffp-contract=off: no fused multiply-add)
// An identity record gives d' = d and o = 0: 1 * x is x, 0 * y is a zero, and x + 0 is x.  A non-finite entry of a record
// leaves a non-finite origin or direction -- k_trace_rays calls such a ray a miss.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LS_SWEEP_HD __host__ __device__ __forceinline__
#else
#define LS_SWEEP_HD inline
#endif

namespace ls {

constexpr float kSweepTmax = 1e16f;   // the tmax ls_generate_rays_aos writes (OptixTracerModules.cu:45-46)

// d' of the nominal direction (dx, dy, dz) under the pose record p
LS_SWEEP_HD void sweep_direction(const float *p, float dx, float dy, float dz, float *out3)
{
    out3[0] = (p[0] * dx + p[1] * dy) + p[2] * dz;
    out3[1] = (p[4] * dx + p[5] * dy) + p[6] * dz;
    out3[2] = (p[8] * dx + p[9] * dy) + p[10] * dz;
}

// the 32-byte lidarshooter::Ray record of a ray: origin xyz, tmin, direction xyz, tmax
LS_SWEEP_HD void sweep_ray(const float *p, float dx, float dy, float dz, float *ray8)
{
    ray8[0] = p[3];
    ray8[1] = p[7];
    ray8[2] = p[11];
    ray8[3] = 0.0f;
    sweep_direction(p, dx, dy, dz, ray8 + 4);
    ray8[7] = kSweepTmax;
}

// LS_SWEEP_DESKEW: the hit in the frame-start sensor frame, o + t d' per axis -- one product, one sum: the bits
// hit_attributes_on_triangle (ls_hit_attr.h) gives as p for the ray record above
LS_SWEEP_HD void sweep_point(const float *p, float dx, float dy, float dz, float t, float *out3)
{
    float d[3];
    sweep_direction(p, dx, dy, dz, d);
    out3[0] = p[3] + t * d[0];
    out3[1] = p[7] + t * d[1];
    out3[2] = p[11] + t * d[2];
}

// whether a table's address allows 16-byte loads of its records (checked once per launch, or per table pointer: wave-uniform)
LS_SWEEP_HD bool table_aligned16(const float *table) { return ((uintptr_t)table & 15u) == 0u; }

#if defined(__HIPCC__)
// the 12 floats of column h's record (k_sweep_rays, k_sweep_pack; k_beam_sweep_rays, k_beam_sweep_pack); aligned16: the table's
// address allows three 16-byte loads per record
__device__ __forceinline__ void load_pose(const float *__restrict__ pose, uint32_t h, bool aligned16, float *p)
{
    const float *src = pose + 12 * (size_t)h;
    if (aligned16) {
        const float4 a = reinterpret_cast<const float4 *>(src)[0], b = reinterpret_cast<const float4 *>(src)[1],
                     c = reinterpret_cast<const float4 *>(src)[2];
        p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w;
        p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w;
        p[8] = c.x; p[9] = c.y; p[10] = c.z; p[11] = c.w;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) p[k] = src[k];
    }
}
#endif

}  // namespace ls
