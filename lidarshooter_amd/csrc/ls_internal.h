// ls_internal.h -- the tracer handle (struct ls_tracer) and the functions the translation units of the host side share.
// Internal to liblidarshooter_hip.so; the public surface is include/lidarshooter_hip.h (+ lidarshooter_hip_debug.h).
//
//   ls_handle.cpp    lifetime, sensor tables, options, info, shard / stream / output buffers, the small stand-alone calls
//   ls_registry.cpp  ITracer's geometry bookkeeping: add / remove / update (EmbreeTracer.cpp:115-288), uploads
//   ls_commit.cpp    commitScene: layout, group-culling data, BVH build / refit / instanced hierarchies
//   ls_trace.cpp     traceScene: output buffers, frames in flight, the per-frame launch sequence, stage timings
//   ls_query.cpp     ls_trace_rays / ls_occluded_rays / ls_closest_points: the query set of per-geometry hierarchies (built lazily),
//                    batches of geometries per launch; what every query entry point shares (stream hand-over, staging, read-back)
//   ls_gather.cpp    ls_hit_attributes: the per-geomID table of its gather kernel; ls_apply_return_model: the same table, its scratch;
//                    their _moving pairs for the records of ls_trace_scene_sweep_moving (ls_attr_moving.hip): a motion table per geomID;
//                    the scene's flat triangle index next to that table, for the scene-side queries (ls_scene_tris.h)
//   ls_cloud.cpp     ls_format_cloud: the records of a frame as a cloud in a driver's own record (ls_format.hip), its format helpers
//   ls_scan.cpp      ls_trace_scene_sweep, ls_trace_scene_beams, ls_trace_scene_sweep_moving: their scratch around the queries' walk
//                    (ls_sweep.hip, ls_beam.hip, ls_moving.hip)
//   ls_voxel_host.cpp ls_occupancy_grid: the voxel grid a frame's rays carve (ls_voxel.hip), its descriptor's check
//   ls_scene_grid_host.cpp ls_scene_grid: the voxels the committed scene's surface occupies (ls_scene_grid.hip), its descriptor's check
//   ls_distance_grid_host.cpp ls_scene_distance_grid: the truncated distance from every cell centre to that surface (ls_distance_grid.hip)
//   ls_surface_sample_host.cpp ls_sample_surface: points drawn from that surface in proportion to area (ls_surface_sample.hip)
//   ls_host_pool.cpp worker threads for host-side copies, point expansion
//   ls_debug.cpp     include/lidarshooter_hip_debug.h (tests and bench.py only)
#pragma once

#include "../../include/lidarshooter_hip.h"
#include "../../include/lidarshooter_hip_debug.h"   // (LS_OPT_DEBUG_FAULT)
#include "ls_kernels.h"
#include "ls_standing.h"
#include "ls_launch.h"
#include "ls_tuning.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

namespace lsi {

// Everything a record of a geometry's standing list depends on (ls_standing.h), compared byte for byte -- at every commit with
// the key of the commit before, which decides whether a list is built, kept or dropped (ls_commit.cpp: standing_commit), and
// once more by the frame that is about to use the list (ls_trace.cpp).  Zeroed before it is filled (padding).
struct StandingKey {
    uint64_t vert_gen, idx_gen;       // which uploads / hand-overs the mesh is
    uint64_t sensor_gen;              // ls_tracer::sensor_gen: the sensor's tables, band map, raster
    const void *raw;
    const uint32_t *idx;
    uint32_t n_tris, stride, quad;
    uint32_t az0, naz;                // the shard
    uint32_t tfirst;                  // the geometry's first global triangle id in the layout
    uint32_t big_cells;
    float margin_az, margin_elev;
    float affine[12], rinv[9], t[3];
};

// A geometry's standing list and the policy's state.  A list is built once the key has been equal at `wait` commits in a row;
// one that is dropped before it has served kStandingBreakEven frames doubles `wait` (at most kStandingMaxWait), one that has
// served that many puts it back to kStandingFirstWait: a geometry that keeps moving stops costing builds.
constexpr uint32_t kStandingFirstWait = 2, kStandingMaxWait = 256;
constexpr uint64_t kStandingBreakEven = 72;   // frames: a build of the headline mesh 183 us, 2.5 us saved per frame (EXPERIMENTS.md E27)
// Under LS_OPT_FRAME_GRAPH a list that comes into use costs three captures (a wait for the stream, the capture, the instantiation:
// of the order of 100 us each, not measured) against a few microseconds saved per frame: of the order of a hundred frames to pay back
constexpr uint32_t kStandingGraphWait = 64;
struct Standing {
    enum State { kNone = 0, kBuilding, kUsable, kTooLong };
    StandingKey key;
    bool key_valid = false;
    uint32_t same = 0;                 // commits in a row that found the key unchanged
    uint32_t wait = kStandingFirstWait;
    State state = kNone;
    ls::StandingRecord *d_recs = nullptr;   // standing_capacity(n_tris) records, kept across drops for the next build
    uint32_t cap = 0;
    uint32_t *d_count = nullptr;       // the build's record count ...
    uint32_t *h_count = nullptr;       // ... copied to this pinned word behind the build ...
    hipEvent_t ev = nullptr;           // ... and this event behind the copy: a commit that finds it complete reads the word
    uint32_t count = 0;                // kUsable: records in the list
    uint64_t served = 0;               // frames traced from the current list
    bool in_graphs = false;            // the captured frame graphs may hold its launch (ls_trace.cpp: route_standing)
};

struct Geometry {
    std::string name;
    int id = -1;
    uint32_t n_verts = 0, n_tris = 0;
    bool quad = false;          // RTC_GEOMETRY_TYPE_QUAD: n_elems quads, traced as n_tris = 2 n_elems triangles
    uint32_t n_elems = 0;       // elements as registered by addGeometry (= n_tris for triangle geometries)
    uint32_t *d_quad_idx = nullptr;   // 4*n_elems indices as handed over (converted into d_idx)
    void *d_raw = nullptr;      // vertex records as uploaded (n_verts * stride bytes)
    size_t raw_cap = 0;
    uint32_t stride = 0;
    uint32_t *d_idx = nullptr;  // 3*n_tris mesh-local vertex indices
    const void *shared_raw = nullptr;       // ls_update_geometry_device_shared: caller-owned device buffers
    const uint32_t *shared_idx = nullptr;   // read in place by the kernels, never copied or freed
    bool has_verts = false, has_idx = false, idx_dirty = true;
    // index validation: every index upload / hand-over launches k_index_max into d_idx_max; the next commit reads it back
    uint32_t *d_idx_max = nullptr;
    bool idx_unchecked = false;   // a reduction is in flight (or done) whose result no commit has looked at
    bool idx_bad = false;         // the last check found an index >= n_verts: every commit fails until new indices arrive
    uint32_t idx_bad_value = 0;
    // host uploads (ls_update_geometry): pinned staging, written by the copy pool, read by the DMA
    void *h_stage_v = nullptr, *h_stage_i = nullptr;
    size_t stage_v_cap = 0, stage_i_cap = 0;
    hipEvent_t ev_stage_v = nullptr, ev_stage_i = nullptr;   // recorded behind the last DMA that reads the staging buffer
    // group culling (projection engine, meshes with 64 triangles per wave): Morton order of the triangles, the
    // indices in that order, a mesh-space bound (sheared box) per kCullGroup sorted triangles
    uint32_t *d_perm = nullptr, *d_idx_sorted = nullptr;
    float4 *d_boxes = nullptr, *d_corners = nullptr;
    bool order_stale = true;    // the topology changed since d_perm / d_idx_sorted were made
    bool bounds_stale = true;   // vertices (may have) changed since d_boxes were made
    bool blas_dirty = true;     // BVH engine, instanced mode: vertices or topology changed since this geometry's hierarchy was built
    bool blas_topo_dirty = true;   // ... the topology did (vertices alone: the sorted order stays, the hierarchy is refitted)
    uint64_t blas_sorted_epoch = 0;   // key_scratch_epoch at which this geometry's sorted keys were written (0: never)
    float mesh_maxabs = 0.0f;   // largest |coordinate| of the mesh as uploaded (read back when that hierarchy is built)
    // which upload the vertices / indices are (ls_tracer::upload_seq at the time): the ray-query set compares them with what its
    // hierarchies were built from (blas_dirty is the frame path's, consumed by the commit)
    uint64_t vert_gen = 0, idx_gen = 0;
    Standing standing;          // projection engine: the triangles with a footprint, kept while nothing they depend on changes
    const void *raw() const { return shared_raw ? shared_raw : d_raw; }
    const uint32_t *idx() const { return shared_idx ? shared_idx : d_idx; }
    float affine[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
};

// LS_OPT_FRAME_GRAPH: the captured launches of one stream of the three-stream rotation
struct FrameGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    uint64_t sig = 0;                       // what decides the launch SEQUENCE (trace_locked: frame_signature)
    std::vector<ls::LaunchRecord> recs;     // the launches as captured (arguments as of the last replay), in order
    std::vector<hipGraphNode_t> nodes;      // their kernel nodes
};

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;  // elements
};

// The standing base (ls_trace.cpp, next to route_standing): the per-ray minimum that the routed standing lists
// give -- the same one every frame while the set stands, atomicMin does not depend on order -- kept once, 8 bytes per ray of the
// shard.  A frame whose routed set is the base's starts from it (its keys are armed with it) instead of from all ones, and
// launches no k_project_standing.  It belongs to one exact set: the frame's standing_bits and every routed geometry's key.
// Built at the first eligible frame that finds its set equal to that of the `wait` - 1 frames before it; one that is dropped
// before it has served kBaseBreakEven frames doubles `wait` (at most kStandingMaxWait), one that has served them puts it back.
// frames: a build is ~28 us of device work behind a drained pipeline (the standing launch 9 - 14, its finish pass 5 - 6, a memset and a
// copy of 4 MB per slot) and about twenty host calls, ~53 us if nothing of the two overlaps; a headline frame saves 6.4 us, one with
// something left to project 4.9: 8 - 11 frames (EXPERIMENTS.md E28).  8 ships.
constexpr uint64_t kBaseBreakEven = 8;
struct StandingBase {
    DevBuf<unsigned long long> keys;     // the base itself
    DevBuf<uint8_t> big;                 // its build's big-footprint queue (big_capacity items) ...
    uint32_t *counter = nullptr;         // ... and counter row (kCounterSlotWords words, zero between builds)
    DevBuf<uint32_t> counts;             // hits per 256-ray block of the base, left by the build's finish pass
    uint32_t gen = 0;                    // 0: none; else the generation the slots' arming words speak of
    uint32_t next_gen = 2;
    uint64_t bits = 0;                   // the set it was built for ...
    std::vector<StandingKey> set;
    uint64_t prev_bits = 0;              // ... and the set of the eligible frame issued last (none: empty)
    std::vector<StandingKey> prev;
    uint32_t same = 0;                   // eligible frames in a row with the set `prev`
    uint32_t wait = kStandingFirstWait;
    uint64_t served = 0;                 // frames that started from the current base
    bool failed = false;                 // no memory for it: nothing is tried again until the set changes
};

// a small device table a call refreshes when it finds it out of date: uploaded through a pinned staging block of its own, so that
// the caller's stream never waits for the host (T: plain data, compared byte for byte)
template <typename T>
struct StagedTable {
    DevBuf<T> dev;
    std::vector<T> current;        // what dev holds (empty after a refresh that failed: the next call uploads again)
    T *h_stage = nullptr;          // pinned staging of the upload ...
    size_t stage_cap = 0;
    hipEvent_t ev_stage = nullptr; // ... recorded behind the last copy that reads it
    // on s, when `table` differs from `current` or dev does not exist; `table` is left in an unspecified state
    int upload_if_changed(ls_tracer *tr, hipStream_t s, std::vector<T> &table);
    void release();
};

}  // namespace lsi

struct ls_tracer {
    std::mutex mu;
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::string err;

    // sensor (LidarDevice state needed by the path)
    std::vector<float> vertical;
    float h_begin = 0, h_end = 0, h_step = 0;
    std::vector<float> given_tables;   // ls_tracer_create_tables: sin_theta[V] cos_theta[V] sin_phi[H] cos_phi[H] as handed over
    uint32_t V = 0, H = 0;
    float rinv[9], t[3];
    float *d_tables = nullptr;  // sin_theta[V] cos_theta[V] sin_phi[H] cos_phi[H] ... (fill_tables)
    std::vector<float> host_tables;   // the same words on the host (ls_trace_scene_expand rebuilds points from (ray, t) records)
    float lut_t0 = 0.0f, lut_scale = 0.0f;   // k_cull's channel look-up table (ProjectParams::chan_lut)
    bool lut_ok = false;
    ls::BandMap band = {{0.0f, 0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, 0, -1};   // k_project's channel band by guess and verify (ls_band_map.h; fill_tables)
    uint32_t az0 = 0, naz = 0;

    // geometry registry
    std::map<std::string, lsi::Geometry> geoms;
    long geometry_count = 0;
    bool layout_dirty = true;

    // committed scene
    std::vector<int> slot_geom_ids;       // geometry ids in layout order
    std::vector<uint32_t> slot_tri_first; // [n+1]
    uint32_t n_verts = 0, n_tris = 0, n_leaves = 0, n_slots = 0, leaf_size = 1, committed_leaf_size = 1;
    bool committed = false;
    lsi::DevBuf<float> verts;
    lsi::DevBuf<uint32_t> tris, keys_a, keys_b, vals_a, vals_b, geom_table;
    lsi::DevBuf<uint8_t> sort_temp;
    lsi::DevBuf<ls::TriRecord> records;
    lsi::DevBuf<ls::FatNode> nodes;
    lsi::DevBuf<float4> range_boxes;
    lsi::DevBuf<unsigned long long> best_keys;  // projection engine: per-ray (t bits, gid) closest-hit key
    lsi::DevBuf<uint8_t> big_queue;             // projection engine: triangles with very large footprints
    uint32_t big_capacity = 0;
    uint32_t *d_big_count = nullptr;
    // what each slot's keys hold between frames (slot 0: best_keys, 1: best_keys_b, 2: best_keys_c; k_pack re-arms them every
    // frame): 0 unknown, 1 all ones, g >= 2 the standing base of generation g.  Slot 0's word also speaks for the counters: 0 there
    // sends the next frame through launch_project_init
    uint32_t keys_arm[3] = {0, 0, 0};
    uint32_t frame_parity = 0;             // which of the two block-counter arrays this frame adds into
    bool scene_materialized = false;       // verts / tris hold the transformed scene of the last commit
    struct LayoutEntry { std::string name; uint32_t vfirst, tfirst; };
    std::vector<LayoutEntry> layout;
    bool projection_ok = true;             // all channel elevations within [-90, 90] degrees
    int engine = 0;                        // LS_OPT_ENGINE: 0 auto, 1 BVH, 2 projection
    bool bvh_built = false;
    lsi::DevBuf<uint32_t> spill;       // traversal-stack overflow area of the persistent trace grid
    uint32_t *d_queue_heads = nullptr;
    bool queue_heads_armed = false;   // the last BVH frame's k_rowcount zeroed them again
    uint32_t trace_blocks = 0, chan_mul = 1, refill_min = 56;
    // LS_OPT_PIPELINE: the finish + pack workgroups of frame i ride in the launch of frame i+1's k_project;
    // everything a frame in flight touches exists twice (parity), the queue counter three times
    int opt_pipeline = 0;
    bool pipe_pending = false;              // a frame is projected, its finish + pack not launched yet
    uint32_t pipe_seq = 0;                  // frames issued in pipelined mode since the last flush
    ls::FinishPackArgs pipe_fa{};           // the pending frame's finish + pack
    lsi::DevBuf<unsigned long long> pack_status; // chained prefix: (epoch << 32) | hits of every 256-ray workgroup
    uint32_t pack_epoch = 0;
    lsi::DevBuf<unsigned long long> best_keys_b; // parity 1 twins of best_keys, big_queue, points, hits, d_n_points
    lsi::DevBuf<uint8_t> big_queue_b, points_b, hits_b;
    uint32_t *d_n_points_b = nullptr;
    // LS_OPT_PIPELINE = 2: whole frames rotate over three streams (three frames in flight); slot 0 / 1 use
    // the buffers above, slot 2 the ones below; every slot has its own block-count array
    hipStream_t slot_stream[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_main = nullptr, ev_done[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_frame = nullptr;          // ls_tracer_order_after_last_frame on the handle's stream
    bool slot_pending[3] = {false, false, false};   // frames issued on slot_stream[s] since the last flush
    // the library enqueues mesh copies on the handle's stream; a slot stream whose epoch is behind orders itself
    // after that stream before its next frame (every slot, not only the first frame after the copy)
    uint64_t main_epoch = 0, slot_epoch[3] = {0, 0, 0};
    uint32_t ms_seq = 0;
    lsi::DevBuf<unsigned long long> best_keys_c;
    lsi::DevBuf<uint8_t> big_queue_c, points_c, hits_c;
    uint32_t *d_n_points_c = nullptr;
    // three-stream mode, small shards: finish + pack of a frame as ONE launch with the chained prefix (k_finish_pack); per slot
    // the status words of its ray blocks and, behind them, the tag word the kernel itself steps (FinishPackArgs::epoch_word)
    lsi::DevBuf<unsigned long long> pack_status_ms;
    bool traced_projection = false;        // the last trace ran on the projection engine (dense arrays on demand)
    const void *last_d_hits = nullptr;     // its hit records and count (device)
    const uint32_t *last_d_n = nullptr;
    std::vector<ls::GeomSource> project_srcs;  // scratch of trace_locked
    // standing lists (ls_standing.h): LS_OPT_STANDING; bumped whenever the sensor's tables, band map, raster or shard change;
    // the lists the frame being issued is traced from (scratch of trace_locked); LS_INFO_STANDING_*
    int opt_standing = 1;
    uint64_t sensor_gen = 0;
    std::vector<ls::StandingBatch> standing_batches;
    long standing_geometries = 0, standing_records = 0, standing_builds = 0;
    lsi::StandingBase base;                    // the routed lists' per-ray minimum, kept (StandingBase)
    std::vector<lsi::StandingKey> routed_keys; // the keys of the geometries route_standing routed (scratch of trace_locked)
    long base_in_use = 0, base_builds = 0;     // LS_INFO_STANDING_BASE (the last frame started from it), LS_INFO_STANDING_BASE_BUILDS
    long base_finish_skipped = 0;              // LS_INFO_STANDING_BASE_NO_FINISH: frames that started from it and launched no finish pass
    ls::RangeTree rt{};
    uint32_t range_entries = 0;
    uint32_t *d_maxabs = nullptr;
    unsigned long long *d_visits = nullptr;

    // trace outputs
    lsi::DevBuf<float> hit_t;
    lsi::DevBuf<uint32_t> hit_gid, row_counts;
    lsi::DevBuf<uint8_t> points;   // 32 B per ray
    lsi::DevBuf<uint8_t> hits;     // 16 B per ray
    uint32_t *d_n_points = nullptr;
    void *ext_points = nullptr, *ext_hits = nullptr;
    uint32_t *ext_n_points = nullptr;
    uint32_t ext_capacity = 0;
    bool ext_hits_only = false;   // ls_tracer_set_hit_buffers: ext_points is only a marker, no point record may be written
    uint8_t *h_points = nullptr;
    ls_hit *h_hits = nullptr;
    size_t h_cap = 0;  // records
    uint32_t *h_n_points = nullptr;
    bool traced = false;
    int opt_bvh_refit = 1;       // LS_OPT_BVH_REFIT
    int opt_bvh_instanced = 1;   // LS_OPT_BVH_INSTANCED: per-geometry hierarchies in mesh space, no build / refit for pose changes
    bool bvh_inst = false;       // the committed BVH is the instanced one
    bool inst_valid = false;     // records / nodes / inst_layout hold instanced hierarchies for the current layout and leaf size
    uint64_t key_scratch_epoch = 1;   // bumped whenever keys_b / vals_b are overwritten by something other than a geometry's own slice
    bool last_commit_built = false;
    struct InstSlot {
        uint32_t node_first, rec_first, n_leaves, range_first;
        ls::RangeTree rt;
        bool wide_made = false;   // its four-wide twins (wide_nodes) are those of its current binary nodes
        uint32_t wide_age = 0;    // frames traced over the current binary nodes while the twins were not made (kWidenAfterFrames)
    };
    std::vector<InstSlot> inst_layout;   // per layout entry
    uint32_t inst_leaf_size = 0;
    lsi::DevBuf<float> inst_verts;    // packed mesh-space vertices of all geometries (build input)
    uint32_t *d_inst_maxabs = nullptr;   // kGeomsPerLaunch words
    lsi::DevBuf<ls::FatNode> treelet; // one-geometry scenes: the top of that hierarchy, breadth-first (k_trace_inst stages it in LDS)
    bool treelet_valid = false;
    lsi::DevBuf<ls::WideNode> wide_nodes;   // instanced mode, LS_OPT_BVH_WIDE: the four-wide twins of `nodes` (k_widen), same indexing
    bool wide_valid = false;     // the twins' buffer exists and LS_OPT_BVH_WIDE was on at the last commit
    bool wide_in_use = false;    // the last trace walked them (every geometry's were made)
    int opt_bvh_wide = 1;
    bool bvh_order_valid = false;   // keys_b / vals_b hold the sorted Morton keys / order of the scene's triangles
    bool tris_rebased = false;          // tr->tris holds the rebased indices of the current layout and index uploads
    bool classic_nodes_valid = false;   // tr->nodes holds the classic hierarchy of the keys bvh_order_valid speaks of (k_refit_nodes may reuse its topology)
    uint32_t bvh_order_tris = 0;
    bool last_commit_refit = false;
    int opt_block_cull = 2;      // LS_OPT_BLOCK_CULL: 0 off, 1 on, 2 auto (geometries of 2 M triangles or more; from 512 k under an azimuth shard: cull_enabled)
    lsi::DevBuf<uint32_t> cull_list;  // three survivor lists (one per frame that can be in flight) of cull_chunks entries
    uint32_t cull_chunks = 0;
    uint32_t *d_aabb6 = nullptr; // scratch of launch_mesh_order
    int opt_host_output = 1;     // LS_OPT_HOST_OUTPUT: the pack kernel writes the pinned host buffers itself
    int opt_readback_hits = 1;   // LS_OPT_READBACK_HITS
    int opt_upload_mode = 1;     // LS_OPT_UPLOAD_MODE
    int opt_emit_points = 1;     // LS_OPT_EMIT_POINTS
    int opt_debug_fault = 0;     // LS_OPT_DEBUG_FAULT (one frame)
    int debug_force_cull = 0;    // ls_debug_force_group_cull: LS_OPT_BLOCK_CULL = 1 applies to a geometry of any size (cull_size_ok)
    uint32_t *h_status = nullptr;   // sticky device status word in pinned host memory (bit 0: chained prefix gave up)
    uint32_t cull_hint_in_use = 0;  // the survivor hint the culled grid is sized from (h_status[1] with hysteresis: trace_once)
    // ls_trace_scene_begin / ls_trace_scene_expand: the device tells the host how far the frame is (ls::HostProgress)
    ls::HostProgress *h_progress = nullptr;   // pinned host memory
    uint32_t progress_epoch = 0;
    bool progress_req = false;                // set by ls_trace_scene_begin around its trace_locked call
    bool progress_active = false;             // the frame begun last reports through h_progress (else it is complete already)
    bool begin_open = false;                  // a begun frame waits for its ls_trace_scene_expand
    uint32_t begin_points = 0, begin_first = 0, begin_blocks = 0;
    uint32_t pack_split = 0, pack_split_blocks = 0;   // ray block at which the pack pass's second launch starts, and the raster it was made for
    int concurrent_streams = 0;     // LS_OPT_PIPELINE = 2 calibration result (0 = not run yet)

    // LS_OPT_FRAME_GRAPH (three-stream mode): one captured graph per slot stream; fg_sink collects the launches of the
    // frame being built (capture: launched into the capturing stream and recorded; describe: only recorded)
    int opt_frame_graph = 0;
    bool fg_broken = false;      // the runtime refused a capture: plain launches from then on
    bool fg_bracket = false;     // ls_frame_graph_begin: the next frame's graph stays open for the caller's work
    bool fg_open = false;        // a frame is being captured / described (fg_sink.mode says which)
    uint64_t fg_tag = 0;
    uint32_t fg_slot = 0;
    lsi::FrameGraph fgraph[3];
    ls::LaunchSink fg_sink;
    uint64_t fg_captures = 0, fg_replays = 0, fg_patches = 0, fg_patch_waits = 0;   // (waits: a patch found its stream's previous frame still in flight)
    uint32_t fg_last_patched = 0;  // bit i: launch i of the frame replayed last went out with new arguments
    uint32_t last_slot = 0xFFFFFFFFu;   // the frame issued last: its stream of the three-stream rotation (none: it ran on `stream`)
    hipStream_t last_stream = nullptr;

    // ls_trace_rays (ls_query.cpp): a hierarchy set of its own -- nothing here is read or written by the frame path, so that
    // frames issued after a query on other streams may overlap it
    struct RayQuerySlot {
        bool valid = false;
        int geom_id = -1;
        uint64_t vert_gen = 0, idx_gen = 0;   // the uploads it was built from
        bool sensor_frame = false;            // built over the sensor-frame vertices (no usable mesh-space inverse) ...
        float affine[12], rinv[9], t[3];      // ... for this pose
        float maxabs = 0.0f;                  // largest |coordinate| of the vertices it was built over
    };
    struct RayQuery {
        lsi::DevBuf<ls::TriRecord> records;
        lsi::DevBuf<ls::FatNode> nodes;
        lsi::DevBuf<ls::WideNode> wide_nodes;
        lsi::DevBuf<float4> range_boxes;
        std::vector<InstSlot> slots;           // per layout entry, as inst_layout
        lsi::DevBuf<float> verts;              // build input: packed vertices (mesh space, or sensor frame)
        lsi::DevBuf<uint32_t> keys_a, keys_b, vals_b;   // per-geometry slices; keys_b / vals_b keep each geometry's sorted order (its refit)
        lsi::DevBuf<uint8_t> sort_temp;
        uint32_t *d_maxabs = nullptr;          // kMaxGeoms words
        uint32_t *d_counters = nullptr;        // ray counter of each launch (kMaxGeoms / kGeomsPerLaunch words)
        lsi::DevBuf<uint32_t> spill;
        lsi::DevBuf<uint8_t> io;               // the host-memory variants' staging (Staging)
        // ls_trace_scene_sweep: the shard's ray records (32 bytes each, ascending ray index), the walk's dense hit records (16
        // bytes each) and the hit count of every 256 of them (every call is ordered through the handle's stream: one at a time)
        lsi::DevBuf<uint8_t> sweep_rays, sweep_hits;
        lsi::DevBuf<uint32_t> sweep_counts;
        // ls_trace_scene_beams: the shard's sub-ray records (32 bytes each, at ray * S + sample), the walk's dense hit records (16
        // bytes each), the returns of every beam (3 x 16 bytes) and, in one array, the return count of every beam and of every 256
        // of them (one call at a time, as the sweep)
        lsi::DevBuf<uint8_t> beam_rays, beam_hits;
        lsi::DevBuf<uint4> beam_blocks;
        lsi::DevBuf<uint32_t> beam_counts;
        // ls_format_cloud, organized: which record fills each of the V * H cells (one call at a time, as the sweep)
        lsi::DevBuf<uint32_t> cloud_map;
        // ls_object_labels: one 64-byte accumulator per geomID below n_labels (ls::LabelAcc), and the V * H records of the handle's own
        // rays for its footprint (32 bytes each) -- one call at a time, as the sweep
        lsi::DevBuf<uint8_t> label_acc, label_rays;
        // ls_occupancy_grid: per ray the (t bits << 32) | geom key of its closest counted record (one call at a time, as the sweep)
        lsi::DevBuf<unsigned long long> voxel_keys;
        // ls_scene_grid: the count word of k_scene_grid_big's queue (entry 0) and 8 bytes (geom, triangle) per triangle of the scene
        // behind it (one call at a time, as the sweep)
        lsi::DevBuf<uint2> scene_queue;
        // ls_scene_distance_grid: the same for k_distance_grid_big's queue (one call at a time, as the sweep)
        lsi::DevBuf<uint2> dist_queue;
        // ls_sample_surface: the bits of the largest area (entry 0) and of every triangle's behind it; the weights' exclusive prefix
        // P[0 .. n_tris] and, behind it, a pair {sum, count} per 256 triangles (one call at a time, as the sweep)
        lsi::DevBuf<uint32_t> surface_area;
        lsi::DevBuf<uint64_t> surface_prefix;
        // ls_cloud_nearest: the index of one call (ls::CloudIndex) -- three words per cloud point and the count word behind them, a
        // 16-byte record per point, a pair per bucket; its sort goes through sort_temp (one call at a time, as the sweep)
        lsi::DevBuf<uint32_t> cloud_words;
        lsi::DevBuf<uint4> cloud_sorted;
        lsi::DevBuf<uint2> cloud_range;
        std::vector<RayQuerySlot> built;       // per layout entry
        std::vector<int> layout_ids;           // geometry ids of the layout the slots were made for ...
        std::vector<uint32_t> layout_firsts;   // ... and their first vertex, first triangle in it
        uint32_t leaf = 0;
        hipEvent_t ev_ready = nullptr, ev_done = nullptr;
        long last_built = 0;                   // LS_INFO_RAY_QUERY_BUILT
    } rq;
    // ls_hit_attributes (ls_gather.cpp): the per-geomID table k_hit_attributes reads, refreshed by the call that finds it out of
    // date (a pose, a vertex or index buffer, the registry or the sensor pose changed)
    struct HitAttr {
        lsi::StagedTable<ls::AttrGeom> table;      // indexed by geomID
        // ls_apply_return_model: the evaluated records between its two kernels (2 x 16 bytes each) and the kept count of every
        // 256 (every call is ordered through the handle's stream: one call uses them at a time)
        lsi::DevBuf<uint4> park;
        lsi::DevBuf<uint32_t> block_counts;
        // ls_hit_attributes_moving / ls_apply_return_model_moving: a motion-table pointer per geomID next to `table` (nullptr: at
        // rest), as long as it is
        lsi::StagedTable<const float *> motion;
        // ls_hit_velocities: a twist-table pointer per geomID next to them (nullptr: at rest), as long as they are
        lsi::StagedTable<const float *> twist;
        // ls_scene_grid: where each geomID's triangles start in the flat triangle index, and the total behind them
        lsi::StagedTable<uint32_t> tri_first;
    } ha;
    uint64_t upload_seq = 0;

    // options / measurement
    int opt_timing = 0;  // 0 off, 1 every stage, 2 only the trace kernel
    bool opt_count = false;
    // hipEvent records: one TimingRecord per frame (commit marks 0..6, trace marks 7..9), kept until
    // ls_get_timings averages and recycles them, so that timing a run never synchronises inside it.
    struct TimingRecord {
        hipEvent_t ev[LS_T_COUNT + 2];
        bool set[LS_T_COUNT + 2];
    };
    std::vector<TimingRecord> trec;
    size_t trec_used = 0;
    bool trec_open = false;
};

namespace lsi {

#define LS_HIP(call)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            tr->err = std::string(#call) + ": " + hipGetErrorString(e_);                             \
            return LS_ERR_HIP;                                                                       \
        }                                                                                            \
    } while (0)

inline int fail(ls_tracer *tr, int code, const char *msg)
{
    tr->err = msg;
    return code;
}

template <typename T>
inline int ensure(ls_tracer *tr, DevBuf<T> &b, size_t need)
{
    if (need <= b.cap) return LS_OK;
    if (b.p) LS_HIP(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    const size_t cap = need + need / 8 + 64;
    LS_HIP(hipMalloc(reinterpret_cast<void **>(&b.p), cap * sizeof(T)));
    b.cap = cap;
    return LS_OK;
}

template <typename T>
inline void release(DevBuf<T> &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

template <typename T>
int StagedTable<T>::upload_if_changed(ls_tracer *tr, hipStream_t s, std::vector<T> &table)
{
    const size_t bytes = table.size() * sizeof(T);
    if (dev.p && table.size() == current.size() && (!bytes || std::memcmp(table.data(), current.data(), bytes) == 0)) return LS_OK;
    current.clear();   // (whatever fails from here on, the next call refreshes: ensure may give the table another buffer)
    int rc;
    if ((rc = ensure(tr, dev, table.size()))) return rc;
    if (!ev_stage) LS_HIP(hipEventCreateWithFlags(&ev_stage, hipEventDisableTiming));
    LS_HIP(hipEventSynchronize(ev_stage));   // (the copy of an earlier refresh may still be reading the staging buffer)
    if (stage_cap < table.size()) {
        if (h_stage) LS_HIP(hipHostFree(h_stage));
        h_stage = nullptr;
        stage_cap = 0;
        LS_HIP(hipHostMalloc(reinterpret_cast<void **>(&h_stage), bytes + bytes / 8, hipHostMallocDefault));
        stage_cap = (bytes + bytes / 8) / sizeof(T);
    }
    std::memcpy(static_cast<void *>(h_stage), table.data(), bytes);
    LS_HIP(hipMemcpyAsync(dev.p, h_stage, bytes, hipMemcpyHostToDevice, s));
    LS_HIP(hipEventRecord(ev_stage, s));
    current.swap(table);
    return LS_OK;
}

template <typename T>
void StagedTable<T>::release()
{
    if (ev_stage) { (void)hipEventSynchronize(ev_stage); (void)hipEventDestroy(ev_stage); }
    if (h_stage) (void)hipHostFree(h_stage);
    lsi::release(dev);
    ev_stage = nullptr;
    h_stage = nullptr;
    stage_cap = 0;
    current.clear();
}

constexpr float kProjectMarginDeg = 0.005f;  // AZIMUTH slack of the footprints, ~8.7e-5 rad: 5x the polynomial atan2 error (1e-3 deg) + table / test rounding
// ELEVATION slack of the channel tables (tan(chi +- margin), fill_tables): what it has to cover is the distance between a
// channel's nominal elevation and the elevation of the ray the kernels actually build for it -- theta = float((90 - chi) pi / 180)
// is off by half an ulp of ~1.5 rad (6e-8 rad), sinf / cosf by an ulp each, |(cos phi, sin phi)| by 1.2e-7 relative: under
// 3e-7 rad = 1.7e-5 degrees in all (the quotients of the band test and k_cull's remainder carry their own relative slack).
// Until round 5 the azimuth's 0.005 degrees stood here too: 1.7e-4 rad over both sides of every ring, 3 % of the ring
// spacing of SYN-128 -- a sixth of all the footprints k_project expanded at SYN-1M and a quarter of the groups k_cull kept at
// SYN-10M were that margin's.
constexpr float kProjectElevMarginDeg = 2e-4f;

inline bool use_projection(const ls_tracer *tr) { return tr->engine == 2 || (tr->engine == 0 && tr->projection_ok); }
inline uint32_t shard_rays(const ls_tracer *tr) { return tr->V * tr->naz; }

// ls_trace.cpp
ls::SensorTables tables(const ls_tracer *tr);
ls::ProjectParams project_params(const ls_tracer *tr);
ls::GeomTable geom_table(const ls_tracer *tr);
int ensure_slot_streams(ls_tracer *tr);
int check_device_status(ls_tracer *tr);
int flush_pipeline(ls_tracer *tr);   // order the handle's stream after every frame still in flight (no host wait)
inline int order_after_projects(ls_tracer *tr) { return flush_pipeline(tr); }
void mark(ls_tracer *tr, int i, hipEvent_t *ride = nullptr);
int trace_locked(ls_tracer *tr, uint32_t frame, ls_frame *out, bool readback);
void frame_graph_destroy(ls_tracer *tr);   // every cached graph (nothing may be open)
// installs the handle's launch sink for the calling thread while an entry point runs (LS_ENTER)
struct SinkScope {
    ls::LaunchSink *prev;
    explicit SinkScope(ls_tracer *tr) : prev(ls::thread_sink()) { ls::thread_sink() = tr->fg_open ? &tr->fg_sink : nullptr; }
    ~SinkScope() { ls::thread_sink() = prev; }
};
// ls_registry.cpp
void affine_from_components(const float *lin, const float *ang, float *A);
void free_geometry(Geometry &g);
// ls_commit.cpp
int materialize_scene(ls_tracer *tr, bool with_maxabs, bool keep_indices = false);
bool cull_enabled(const ls_tracer *tr, const Geometry &g);
bool cull_size_ok(const ls_tracer *tr, uint32_t n_tris);   // large enough for 64 triangles per wave (or ls_debug_force_group_cull)
// the committed geometries as the projection engine's next frame reads them (ls_trace.cpp): culling data attached where it is current
int project_sources(ls_tracer *tr, std::vector<ls::GeomSource> &srcs, bool &any_culled);
ls::GeomSource project_source(const ls_tracer *tr, const Geometry &ge, uint32_t tfirst);   // one of them
// standing lists: whether frames may be traced from them at all as the handle's options stand (ls_trace.cpp); a geometry's key
// as of now; a list let go (the policy's back-off; its buffer stays); the policy, at the end of a commit (ls_commit.cpp)
bool standing_allowed(const ls_tracer *tr);
StandingKey standing_key(const ls_tracer *tr, const Geometry &ge, uint32_t tfirst);
void standing_drop(Standing &st);
int standing_commit(ls_tracer *tr);
bool shard_sector(const ls_tracer *tr, double &lo_deg, double &hi_deg);   // ls_trace.cpp
bool inst_inverse(const ls_tracer *tr, const Geometry &ge, double *minv9, double *o3, double *cond);
int commit_locked(ls_tracer *tr);
// ls_host_pool.cpp
void parallel_copy(void *dst, const void *src, size_t bytes);
int host_pool_threads();
constexpr size_t kExpandItem = 16384;   // points per work item of an expansion: 256 KB read, 512 KB written
void expand_points_range(uint8_t *dst_points32, const uint8_t *compact16, size_t count);
// 8-byte (ray, t) records in ascending ray order -> 32-byte points: xyz = t * direction from the factor tables, the float
// operations of k_pack in the same order
void expand_hits_range(uint8_t *dst_points32, const uint8_t *hits8, size_t count, const float *sin_theta, const float *cos_theta,
                       const float *cs_phi, uint32_t V, uint32_t H);
void pool_run(size_t n, const std::function<void(size_t)> &fn);   // fn(0) .. fn(n-1) on the worker threads and the caller

// A set of per-geometry hierarchies: the frame path's instanced one (records / nodes / wide_nodes / range_boxes / inst_layout,
// ls_commit.cpp) or the ray-query set (ls_tracer::RayQuery).  hier_layout gives every geometry of `order` its slices (slot
// i: nodes, records, range boxes) and sizes the arrays; hier_build (re)builds or refits the hierarchy of slot i from the
// geometry's vertices through (A, R, T) -- identity for mesh space -- with the kernels of the classic build.
struct HierSet {
    DevBuf<ls::TriRecord> *records;
    DevBuf<ls::FatNode> *nodes;
    DevBuf<ls::WideNode> *wide;                 // (nullptr: no four-wide twins)
    DevBuf<float4> *range_boxes;
    std::vector<ls_tracer::InstSlot> *slots;
    DevBuf<float> *verts;
    DevBuf<uint32_t> *keys_a, *keys_b, *vals_b;
    DevBuf<uint8_t> *sort_temp;
    uint32_t *d_maxabs;                         // one word per slot, zero before the build
};
int hier_layout(ls_tracer *tr, HierSet &hs, const std::vector<Geometry *> &order, uint32_t leaf_size, uint32_t *n_nodes);
// refit: the slot's sorted keys / values and its nodes are those of the same topology (only the vertices changed); widen: make the
// four-wide twins now (the slot's wide_made says whether they were made)
int hier_build(ls_tracer *tr, HierSet &hs, hipStream_t s, size_t i, const Geometry &ge, uint32_t vfirst, uint32_t tfirst, const float *A12,
               const float *R9, const float *T3, uint32_t leaf_size, bool refit, bool widen);
// ls_query.cpp
void ray_query_release(ls_tracer *tr);
#pragma GCC visibility push(hidden)   // what ls_gather.cpp and ls_scan.cpp share with it: not exported
constexpr uint32_t kMaxQueryRecords = 0xFFF00000u;   // rays, points or hit records in one call
// the registry's geometry of layout entry i, provided it still is what the last commit laid out (every query's check)
int committed_geometry(ls_tracer *tr, size_t i, Geometry **out);
// the last test of every query's check: -1 without a committed, non-empty scene, as ls_trace_scene (nothing is written)
inline int uncommitted(const ls_tracer *tr) { return !tr->committed || tr->n_tris == 0 ? -1 : LS_OK; }
hipStream_t stream_of(const ls_tracer *tr, void *hip_stream);   // the caller's stream, or the handle's for NULL
inline bool misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
template <typename... P>
inline bool misaligned16(const P *...p) { return (misaligned(p, 16) || ...); }
// a query's place among what the handle issues (query_enter: the call's one flush_pipeline) and its walk over the hierarchies
struct RayQueryKind;
struct Moving;
const RayQueryKind &closest_hits();   // ls_trace_rays' kind: the walk of the frames in ls_scan.cpp
int query_enter(ls_tracer *tr, hipStream_t s);
int query_walk(ls_tracer *tr, hipStream_t s, const void *d_rays, uint32_t n, void *d_out, const RayQueryKind &kind,
               const float *const *motion = nullptr);   // motion: ls_trace_scene_sweep_moving's tables, one per layout entry
int query_leave(ls_tracer *tr, hipStream_t s);
// ls_object_labels' footprint (ls_labels_host.cpp): the query set brought up to date as query_walk does, then k_label_footprint over the n
// rays, one launch per batch of kGeomsPerLaunch geometries, each on its own -- a geometry whose id is >= n_labels is not walked
int query_footprint(ls_tracer *tr, hipStream_t s, const void *d_rays, uint32_t n, bool own_rays, uint32_t n_labels, void *d_acc);
// ls_gather.cpp: the per-geomID table of the gathers (tr->ha.table) brought up to date on s; mv: a moving call's motion tables too
int tables_prepare(ls_tracer *tr, hipStream_t s, const Moving *mv);
// ... and the scene's flat triangle index next to it (tr->ha.tri_first; ls_scene_tris.h): *n_table entries, *n_tris triangles; more
// than max_tris of them: LS_ERR_OUT_OF_RANGE with the message too_many
int scene_tris_prepare(ls_tracer *tr, hipStream_t s, unsigned long long max_tris, const char *too_many, uint32_t *n_table, uint32_t *n_tris);
// the queue of a scene query's big kernel: the count word (in an entry of its own), then 8 bytes per triangle of the scene -- it
// cannot overflow
inline int scene_queue_ensure(ls_tracer *tr, DevBuf<uint2> &q, uint32_t n_tris, uint32_t **count, uint2 **first)
{
    if (const int rc = ensure(tr, q, (size_t)n_tris + 1)) return rc;
    *count = reinterpret_cast<uint32_t *>(q.p);
    *first = q.p + 1;
    return LS_OK;
}
// the tail of every device entry point: the query's place on s around what it issues
template <typename Issue>
inline int query_run(ls_tracer *tr, hipStream_t s, Issue &&issue)
{
    int rc;
    if ((rc = query_enter(tr, s)) || (rc = issue())) return rc;
    return query_leave(tr, s);
}
// The host-memory variants stage in RayQuery::io, on the handle's stream.  A call declares every piece first -- in(): copied to the
// device by commit(); out(): `records` records of `bytes` each, read back afterwards; inout(): an out() that commit() also copies in
// when the call accumulates into what the caller's array holds; scratch(): neither -- and a null or empty piece is absent: no room,
// no copy, nullptr for an address.  commit() sizes q.io (a growing buffer: the frame path's frames in
// flight never read it), starts the copies and fills in the Staged, which alone gives a piece's device address: no pointer can be
// formed before the buffer has its final place.  Every piece starts 16-byte aligned.
struct StagePiece {
    void *host;
    size_t at, bytes, record;   // record != 0: an output, in records of this size
    bool copy_in;
};
// a scratch piece read back as `rows` rows of `bytes` at `pitch`, from byte `first` of the piece to byte `first` of dst (NULL: not wanted)
struct StridedRows {
    void *dst;
    int piece;
    size_t first, bytes, rows, pitch;
};
class Staged {
public:
    template <typename T = uint8_t>
    T *dev(int piece) const { return pieces[(size_t)piece].bytes ? reinterpret_cast<T *>(base + pieces[(size_t)piece].at) : nullptr; }
    int fetch(ls_tracer *tr) const;   // every output whole; returns when they are filled
    // the count word (a scratch piece) comes back first (above limit: LS_ERR_HIP with this message), then as many records of every
    // output and, whatever the count, `strided`; returns when they are filled and *n_out is the count
    int fetch_counted(ls_tracer *tr, int count, size_t limit, const char *overflow, uint32_t *n_out, const StridedRows *strided = nullptr) const;

private:
    friend class Staging;
    std::vector<StagePiece> pieces;
    uint8_t *base = nullptr;
};
class Staging {
public:
    int in(const void *src, size_t bytes) { return add(const_cast<void *>(src), src ? bytes : 0, 0, true); }
    int out(void *dst, size_t records, size_t bytes) { return inout(dst, records, bytes, false); }
    int inout(void *p, size_t records, size_t bytes, bool copy_in) { return add(p, p ? records * bytes : 0, bytes, copy_in); }
    int scratch(size_t bytes) { return add(nullptr, bytes, 0, false); }
    int commit(ls_tracer *tr, hipStream_t s, Staged &io);

private:
    int add(void *host, size_t bytes, size_t record, bool copy_in)
    {
        pieces.push_back({host, total, bytes, record, copy_in});
        total += (bytes + 15) & ~(size_t)15;
        return (int)pieces.size() - 1;
    }
    std::vector<StagePiece> pieces;
    size_t total = 0;
};
// ls_scan.cpp: the pose table, the flags and the motions of ls_trace_scene_sweep_moving and of the gathers over its records
// (ls_gather.cpp), as the caller gave them (host or device addresses; no table: the sensor at rest); after moving_resolve the layout
// entry of every motion.  The walk takes the motion tables per layout entry, the gathers per geomID (nullptr: at rest).  A
// host-memory variant declares the tables in its Staging (stage) and goes on with their device copies (use_staged)
struct Moving {
    const float *col_pose;
    uint32_t n_cols;
    const ls_geometry_motion *motions;
    uint32_t n_motions, flags;
    struct Entry { size_t slot; uint32_t geom; const float *table; int piece; };
    std::vector<Entry> e;
    int pose_piece = -1;
    std::vector<const float *> per_slot(size_t n) const;
    std::vector<const float *> per_geom(size_t n) const;   // (a geomID beyond n is left out: the kernels check against one bound)
    void stage(const ls_tracer *tr, Staging &st);
    void use_staged(const Staged &io);
};
// what every call refuses of them, in this order (nothing of it needs a commit or the device): the pose table's length and the flags
// (pose_flags_check: these two alone), then the motions
int pose_flags_check(ls_tracer *tr, const float *col_pose, uint32_t n_cols, uint32_t flags);
int moving_args_check(ls_tracer *tr, const Moving &mv);
// the device entry points' alignment test: p16 to 16 bytes; p4, the pose table and every motion table to 4
bool moving_misaligned(std::initializer_list<const void *> p16, std::initializer_list<const void *> p4, const Moving &mv);
// the last refusal, after uncommitted(): LS_ERR_UNKNOWN_GEOMETRY for a motion of a geometry that is not in the committed scene
int moving_resolve(ls_tracer *tr, Moving &mv);
#pragma GCC visibility pop
// ls_gather.cpp
void hit_attr_release(ls_tracer *tr);

}  // namespace lsi

// every entry point that takes a handle: argument check, the handle's mutex, what it refuses before anything touches the device
// (an expression evaluated under the mutex: a status to return, or 0), its device
#define LS_ENTER_CHECKED(tr, refusal)                   \
    if (!(tr)) return LS_ERR_INVALID_ARGUMENT;          \
    std::lock_guard<std::mutex> lock_((tr)->mu);        \
    if (const int refused_ = (refusal)) return refused_; \
    lsi::SinkScope sink_scope_(tr);                     \
    if (hipSetDevice((tr)->device) != hipSuccess) return lsi::fail((tr), LS_ERR_HIP, "hipSetDevice failed")
#define LS_ENTER(tr) LS_ENTER_CHECKED(tr, LS_OK)
