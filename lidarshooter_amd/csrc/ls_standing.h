// ls_standing.h -- the standing list of a geometry (projection engine): one record per triangle whose footprint on the raster
// holds at least one cell -- exactly what k_project stages for it (v0, e1, e2, NgC, global triangle id, footprint) --, kept from
// frame to frame while nothing a record depends on changes: the geometry's vertices, indices and pose, the sensor's pose and
// tables, the shard, the triangle's global id.  A frame then expands the records (k_project_standing) instead of loading,
// gathering, transforming and bounding every triangle of the mesh again to learn the same thing; five triangles in six of a
// large ground mesh fall between two rings and have no record at all.
// The list is built by a launch of its own at a commit (k_standing_build), never changes while it is in use, is validated by a
// bytewise compare of StandingKey, and is used only after the host has seen its build complete (ls_commit.cpp, ls_trace.cpp).
// The kernels sit in ls_standing.hip, which is part of ls_project.hip's translation unit: they are made of its device functions.
#pragma once

#include "ls_kernels.h"

namespace ls {

struct alignas(16) StandingRecord {
    float v0[3], e1[3], e2[3], NgC;
    uint32_t gid;
    uint32_t i0_nch;               // i0 | nch << 16 (the engine takes at most 32 767 channels here)
    uint32_t h0a, na, h0b, nb;
};
static_assert(sizeof(StandingRecord) == 64, "a standing record is four 16-byte loads");

constexpr uint32_t kStandingMaxChannels = 32767u;
// records one wave of k_project_standing takes (its 64 lanes share their cells): of 16, 32 and 64 the default run is fastest
// with 32 (10.97 - 11.10 us per frame against 11.29 - 11.51 and 11.33 - 11.39, EXPERIMENTS.md E27); LS_STANDING_PER_WAVE in the experiment build
constexpr uint32_t kStandingPerWave = 32u;

// room for a quarter of the triangles (a sixth have a footprint on the headline frame), never less than 4 096 or more than all
inline uint32_t standing_capacity(uint32_t ntris)
{
    const uint32_t want = ntris / 4u > 4096u ? ntris / 4u : 4096u;
    return ntris < want ? ntris : want;
}

// the lists of one k_project_standing launch (kernel argument, as GeomBatch)
struct StandingBatch {
    uint32_t n;
    uint32_t block_first[kGeomsPerLaunch + 1];   // first workgroup of list i; [n] = grid size
    uint32_t count[kGeomsPerLaunch];
    const StandingRecord *recs[kGeomsPerLaunch];
};

// one lane per triangle of src (read as the unculled launch reads it): the records of the triangles with a footprint, in no
// particular order, to recs[0 .. capacity), their number -- which may exceed capacity: such a list is never used -- in *count
// (zeroed here, on s; -> that memset's status)
hipError_t launch_standing_build(hipStream_t s, const ProjectParams &pp, const GeomSource &src, StandingRecord *recs, uint32_t capacity, uint32_t *count);
// the frame's launch over up to kGeomsPerLaunch lists (standing_batch_add: one more list in a zeroed batch -- an empty one takes
// no workgroup); keys, queue and queue counter as launch_project's
void standing_batch_add(StandingBatch &batch, const StandingRecord *recs, uint32_t count);
void launch_project_standing(hipStream_t s, const ProjectParams &pp, const StandingBatch &batch, unsigned long long *best, void *big,
                             uint32_t big_capacity, uint32_t *big_count);

}  // namespace ls
