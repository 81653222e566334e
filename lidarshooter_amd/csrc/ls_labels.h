// ls_labels.h -- what ls_labels.hip gives the host code of ls_object_labels (ls_labels_host.cpp, and the walk's hook in ls_query.cpp): the
// per-geomID accumulator and the four launches.  Internal to the library; the call is described in include/lidarshooter_hip.h.
#pragma once

#include "ls_kernels.h"

namespace ls {

// One accumulator per geomID below n_labels, 64 bytes = one line, in a scratch buffer of the handle.  Every field is reduced by an
// integer atomic whose result does not depend on the order of arrival:
//   n_hits, n_alone   sums;
//   t_ray_min         (t bits << 32) | ray, atomicMin: the smallest t, then the lowest ray (t >= 0: its bits are monotone);
//   t_ray_max         (t bits << 32) | ~ray, atomicMax: the largest t, then the lowest ray;
//   lo, hi            ordered keys of the points' coordinates (label_key), atomicMin / atomicMax.
struct alignas(64) LabelAcc {
    uint32_t n_hits, n_alone;
    unsigned long long t_ray_min, t_ray_max;
    uint32_t lo[3], hi[3];
    uint32_t pad[4];
};
static_assert(sizeof(LabelAcc) == 64, "one accumulator is one 64-byte line");

constexpr uint32_t kMaxLabels = 65536;   // ls_object_labels' n_labels

void launch_label_init(hipStream_t s, LabelAcc *acc, uint32_t n_labels);
// the reduction over n ls_hit records (min(n, *d_count) with a device count).  own_rays: hit.ray indexes the handle's full raster
// (tb) and the point is t * d; otherwise the n_rays 32-byte caller rays and o + t * d.  table, n_table: launch_hit_attributes'.
void launch_label_reduce(hipStream_t s, const void *hits, const uint32_t *d_count, uint32_t n, const void *rays, uint32_t n_rays, bool own_rays,
                         const SensorTables &tb, const AttrGeom *table, uint32_t n_table, LabelAcc *acc, uint32_t n_labels);
// the per-geometry any-hit walk: launch_occluded_rays' arguments; ray r adds one to acc[g].n_alone for every geometry g of the batch
// it hits in [tmin, tmax] (a geometry with n_leaves = 0 is not walked).  own_rays: the records are the handle's own (tmin = 0, tmax
// = +inf whatever the record says).  Every launch stands alone: `counter` starts at zero, nothing is carried from batch to batch.
void launch_label_footprint(hipStream_t s, uint32_t grid_blocks, const void *rays, uint32_t n, bool own_rays, const RayBatch &batch,
                            const WideNode *wide, const TriRecord *records, uint32_t leaf_size, LabelAcc *acc, uint32_t *counter, uint32_t *spill);
// the accumulators decoded into n_labels 64-byte ls_object_label records (flags: the table's presence)
void launch_label_finish(hipStream_t s, const LabelAcc *acc, const AttrGeom *table, uint32_t n_table, void *labels, uint32_t n_labels);

}  // namespace ls
