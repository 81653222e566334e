/*
 * lidarshooter_hip.h -- C ABI of the MI355X (gfx950) LiDAR ray-casting backend.
 *
 * Drop-in boundary: the reference's tracer plugin surface `lidarshooter::ITracer`
 * (ros_ws/src/lidarshooter/src/ITracer.hpp:29-152) as implemented by EmbreeTracer (CPU) and
 * OptixTracer (CUDA).  The reference has no FFI for this path -- its backends are compiled in --
 * so the entry points below are exactly what a `HipTracer : public ITracer` adapter binds, one
 * call per virtual (INTEGRATION.md shows that adapter).  Plain pointers and sizes only; no
 * exceptions cross this boundary; every mutator returns 0 / a non-negative id on success and a
 * negative ls_status on failure, and ls_last_error() holds the message.
 *
 * Threading (ITracer callers: ROS spinner thread for update/commit/trace, Qt thread for
 * add/remove, unsynchronised -- mainwindow.cpp:153,320 vs MeshProjector.cpp:446-464): every call
 * takes the handle's internal mutex.  Buffers returned by ls_trace_scene stay valid until the
 * next call on the same handle.
 *
 * All paths in comments are relative to /root/reference/ros_ws/src/lidarshooter/src/.
 */
#ifndef LIDARSHOOTER_HIP_H
#define LIDARSHOOTER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 (round 6): + ls_tracer_set_hit_buffers, ls_group_frame_status, LS_INFO_EMIT_POINTS, LS_INFO_FRAME_GRAPH_PATCH_WAITS,
 *    ls_source_hash, LS_OPT_BVH_WIDE / LS_INFO_BVH_WIDE, LS_GROUP_INFO_ARRANGEMENT_*; ls_tracer_set_sensor* is refused while external output buffers are
 *    installed; ls_commit_scene can return LS_ERR_OUT_OF_RANGE; the test hooks left this header for lidarshooter_hip_debug.h.
 *    The bindings (capi.py, groupapi.py, integration/HipTracer.hpp) check it against ls_abi_version() at load. */
#define LS_ABI_VERSION 4

typedef struct ls_tracer ls_tracer;

typedef enum ls_status {
    LS_OK = 0,
    LS_ERR_INVALID_ARGUMENT = -2,
    LS_ERR_UNKNOWN_GEOMETRY = -3, /* name not registered (EmbreeTracer.cpp:224-225 returns -1 for remove) */
    LS_ERR_DUPLICATE_GEOMETRY = -4,
    LS_ERR_UNSUPPORTED_TYPE = -5, /* neither triangles nor quads (EmbreeTracer.cpp:200-201 returns 0/false there) */
    LS_ERR_HIP = -6,              /* a HIP runtime call failed; message in ls_last_error */
    LS_ERR_NO_DEVICE = -7,        /* no usable gfx950 device: the product never falls back to the CPU */
    LS_ERR_NOT_COMMITTED = -8,
    LS_ERR_OUT_OF_RANGE = -9
    /* -1 is reserved for the reference's own "empty scene" / "unknown name" return value */
} ls_status;

/* Geometry element types; values follow Embree's RTCGeometryType so the adapter can pass the
 * enum it receives through ITracer::addGeometry (ITracer.hpp:50) unchanged. */
#define LS_GEOMETRY_TYPE_TRIANGLE 0 /* RTC_GEOMETRY_TYPE_TRIANGLE */
#define LS_GEOMETRY_TYPE_QUAD 1     /* RTC_GEOMETRY_TYPE_QUAD (EmbreeTracer.cpp:179-198): 4 indices per element; traced as
                                     * Embree does, as the triangle pair (v0,v1,v3), (v2,v3,v1); ls_hit.prim = quad index */

/* Sensor description = what LidarDevice holds after loadConfiguration()
 * (LidarDevice.cpp:482-633, :758-822).  The adapter fills it from its LidarDevice; the repo's own
 * host mirror (lidarshooter_amd/host/LidarDevice.hpp) fills it from the same JSON files. */
typedef struct ls_sensor_desc {
    const float *vertical_deg; /* channels.vertical[]: degrees above the horizon, channel order   */
    uint32_t n_vertical;       /* V                                                                */
    float h_begin;             /* channels.horizontal.range.begin (degrees)                        */
    float h_end;               /* channels.horizontal.range.end                                    */
    uint32_t h_count;          /* channels.horizontal.count = H; step = (end-begin)/(H-1) (:611)   */
    float Rinv[9];             /* sensorToBase.Rinv, row-major (:813)                              */
    float t[3];                /* (baseToOrigin.tx, baseToOrigin.ty, sensorToBase.tz) (:383-388)   */
} ls_sensor_desc;

/* The same sensor as ray-direction factor tables, for a caller that holds a live LidarDevice but not its
 * private fields (the ROS-typed adapter integration/HipTracer.hpp recovers these through the public
 * API only: LidarDevice::nextRay1 and originToSensor, LidarDevice.hpp:180,252).  Ray (v, h) has the
 * direction (sin_theta[v]*cos_phi[h], sin_theta[v]*sin_phi[h], cos_theta[v]) -- the products the
 * reference forms (LidarDevice.cpp:310-316); the kernels multiply exactly these entries.
 * The footprint bounds of the projection engine need the ANGLES too.  Elevations: the library derives every
 * channel's from the tables themselves, atan2(cos_theta, sin_theta) in double (the bounds' elevation slack is
 * 2e-4 degrees: no description could be trusted to that); elevation_deg is a cross-check -- tables whose
 * elevation_deg is more than 0.01 degrees off that are refused (LS_ERR_INVALID_ARGUMENT), never traced wrongly.
 * Azimuths: h_begin_deg + h * h_step_deg feeds bounds with 0.005 degrees + 1/16 column of slack and must be within
 * 0.002 degrees of atan2(sin_phi, cos_phi) for every column, or the tables are refused as well. */
typedef struct ls_sensor_tables {
    const float *sin_theta;     /* [n_vertical]                                              */
    const float *cos_theta;     /* [n_vertical]                                              */
    const float *elevation_deg; /* [n_vertical] degrees above the horizon (90 - theta)       */
    uint32_t n_vertical;
    const float *sin_phi;       /* [h_count]                                                 */
    const float *cos_phi;       /* [h_count]                                                 */
    uint32_t h_count;
    float h_begin_deg;          /* azimuth of column 0                                       */
    float h_step_deg;           /* azimuth of column h = h_begin_deg + h_step_deg * h        */
    float Rinv[9];              /* as in ls_sensor_desc                                      */
    float t[3];
} ls_sensor_tables;

/* One hit, 16 bytes.  Points and hit records are emitted in ray-index order (r = v*H + h,
 * LidarDevice.cpp:824-845), one record per point. */
typedef struct ls_hit {
    uint32_t ray;   /* global ray index r; channel (ring) = r / H, azimuth column = r % H */
    uint32_t geom;  /* geomID as returned by ls_add_geometry                               */
    uint32_t prim;  /* triangle index within that geometry (Embree primID)                 */
    float t;        /* hit distance along the unit ray direction                           */
} ls_hit;

/* Result of one traceScene().  points32 is the PointCloud2 `data` payload: n_points records of
 * 32 bytes, x f32@0 y f32@4 z f32@8 0@12 intensity f32@16 ring i32@20 0@24..31
 * (XYZIRBytes.cpp:24-40); the adapter sets cloud.width = n_points (EmbreeTracer.cpp:364). */
typedef struct ls_frame {
    const uint8_t *points32; /* pinned host memory, 32*n_points bytes              */
    const ls_hit *hits;      /* pinned host memory, n_points records               */
    uint32_t n_points;
    uint32_t n_rays;         /* rays traced by this handle's shard (V * shard width) */
    uint32_t frame;          /* echo of the frame index (PointCloud2 header.seq, LidarDevice.cpp:108) */
    const void *d_points32;  /* the same data in device memory (for RCCL gathers)  */
    const void *d_hits;
    const uint32_t *d_n_points; /* device word holding n_points                    */
    const void *compact16;   /* LS_OPT_HOST_OUTPUT = 2: n_points records of 16 bytes (x, y, z f32, ring i32) in pinned
                              * host memory instead of points32 (which is NULL then); ls_expand_points rebuilds the
                              * 32-byte records -- half the bytes cross PCIe                                        */
} ls_frame;

/* ---- lifetime: EmbreeTracer::create / ~EmbreeTracer (EmbreeTracer.cpp:10-70),
 *      OptixTracer::create (OptixTracer.hpp:91) --------------------------------------------- */
int ls_tracer_create(const ls_sensor_desc *sensor, int hip_device, ls_tracer **out);
int ls_tracer_create_tables(const ls_sensor_tables *sensor, int hip_device, ls_tracer **out);
/* ITracer::setSensorConfig (ITracer.hpp:129, ITracer.cpp:48) / a LidarDevice initialised again (LidarDevice.hpp:116-117):
 * EmbreeTracer::traceScene reads its LidarDevice every frame (EmbreeTracer.cpp:299-307), so another sensor -- raster,
 * channel table, pose -- takes effect at the next trace.  These calls give the handle another sensor and keep its
 * geometries: frames in flight complete first, the shard goes back to the full turn, a committed scene is committed
 * again for the new sensor.  Forms as the two create calls. */
int ls_tracer_set_sensor(ls_tracer *tr, const ls_sensor_desc *sensor);
int ls_tracer_set_sensor_tables(ls_tracer *tr, const ls_sensor_tables *sensor);
void ls_tracer_destroy(ls_tracer *tr);

/* ---- ITracer::addGeometry (ITracer.hpp:50; EmbreeTracer.cpp:115-218; OptixTracer.cpp:63-133).
 * Returns the geomID (>= 0, lowest free id like rtcAttachGeometry) or a negative ls_status. */
int ls_add_geometry(ls_tracer *tr, const char *name, int geometry_type, int n_vertices, int n_elements);

/* ---- ITracer::removeGeometry (ITracer.hpp:59; EmbreeTracer.cpp:220-260).
 * Returns the removed geomID, or -1 if the name is unknown (Embree behaviour). */
int ls_remove_geometry(ls_tracer *tr, const char *name);

/* ---- ITracer::updateGeometry(name, Eigen::Affine3f, mesh) (ITracer.hpp:69; EmbreeTracer.cpp:262-274;
 * MeshTransformer.cpp:142-205).  affine3x4: row-major [linear | translation].  verts: n_vertices
 * records of vert_stride bytes whose first 12 bytes are x,y,z float32 (pcl cloud.data with
 * point_step, MeshTransformer.cpp:176-181).  tri_idx: 3*n_elements vertex indices (polygons[i].vertices,
 * MeshTransformer.cpp:512-518; 4*n_elements for a quad geometry, :521-552); NULL keeps the indices of the previous update.  Host pointers; the
 * caller may reuse them as soon as the call returns (MeshProjector.cpp:448-461 does).  By default the copy
 * goes straight from the caller's pageable memory at PCIe rate and the call returns when the memory has been
 * read; with LS_OPT_UPLOAD_MODE = 0 the library's worker threads stage it through pinned memory instead and the
 * call never waits for the device. */
int ls_update_geometry(ls_tracer *tr, const char *name, const float affine3x4[12], const void *verts,
                       uint32_t vert_stride, const uint32_t *tri_idx);

/* ---- ITracer::updateGeometry(name, translation, rotation, mesh) (ITracer.hpp:80;
 * EmbreeTracer.cpp:276-288): T = Translation(lin)*Rz(ang.z)*Ry(ang.y)*Rx(ang.x)
 * (MeshTransformer.cpp:467-477). */
int ls_update_geometry_components(ls_tracer *tr, const char *name, const float lin[3], const float ang[3],
                                  const void *verts, uint32_t vert_stride, const uint32_t *tri_idx);

/* Same as ls_update_geometry with verts / tri_idx already resident in HBM on the tracer's device
 * (no PCIe in the frame loop; used by bench.py).  The copies are stream-ordered. */
int ls_update_geometry_device(ls_tracer *tr, const char *name, const float affine3x4[12], const void *d_verts,
                              uint32_t vert_stride, const uint32_t *d_tri_idx);

/* Zero-copy variant: the library keeps the two device pointers and READS THE CALLER'S BUFFERS IN PLACE
 * during the following commitScene / traceScene calls (the vertex transform is fused into the trace
 * kernel, so nothing needs to be staged).  The caller must leave the buffers unchanged and alive until
 * that traceScene has completed on the handle's stream, or until the next update of this geometry.
 * New contents of a shared buffer are announced by handing it over again: the library keeps data derived
 * from the mesh (group bounds, standing lists), and a transform-only update says the mesh did not change.
 * d_tri_idx = NULL keeps the previously shared / copied indices. */
int ls_update_geometry_device_shared(ls_tracer *tr, const char *name, const float affine3x4[12], const void *d_verts,
                                     uint32_t vert_stride, const uint32_t *d_tri_idx);

/* Only the rigid transform of an already uploaded mesh changes (AffineMesh pose integration,
 * AffineMesh.cpp:108-128): no vertex traffic at all. */
int ls_update_geometry_transform(ls_tracer *tr, const char *name, const float affine3x4[12]);

/* T = Translation(lin) * Rz(ang.z) * Ry(ang.y) * Rx(ang.x) as the row-major 3x4 matrix the calls above take
 * (MeshTransformer.cpp:467-477, Eigen's AngleAxis arithmetic) -- lets the adapter turn the (translation,
 * rotation) overload of ITracer::updateGeometry into ls_update_geometry_transform when the mesh is unchanged. */
void ls_affine_from_components(const float lin[3], const float ang[3], float affine3x4[12]);

/* ---- ITracer::commitScene (ITracer.hpp:87; EmbreeTracer.cpp:290-295 rtcCommitScene;
 * OptixTracer.cpp:263-275, :517-571).  Fixes the geometry layout (global triangle ids in (geomID,
 * primID) order); with the BVH engine it also transforms every geometry into the sensor frame and
 * builds the BVH on the device (the projection engine has nothing to build).  Returns 0, or -1 on an
 * empty scene (OptixTracer.cpp:266-267).  A geometry whose index buffer changed since the last commit is
 * checked here (one max-reduction over the indices on the device, read back): LS_ERR_OUT_OF_RANGE when a
 * triangle names a vertex the geometry does not have -- the message (ls_last_error) names geometry and
 * index; nothing is built, ls_trace_scene is refused until a commit succeeds, and new indices for that
 * geometry (or ls_remove_geometry) clear the condition.  Non-finite or huge
 * vertex COORDINATES are not an error: such triangles are never hit (as in the reference's ray test). */
int ls_commit_scene(ls_tracer *tr);

/* ---- ITracer::traceScene (ITracer.hpp:94; EmbreeTracer.cpp:297-367; OptixTracer.cpp:277-358).
 * Ray generation + closest hit + packing.  Returns 0, or -1 on an empty scene with a zero-point
 * frame (OptixTracer.cpp:280-288). */
int ls_trace_scene(ls_tracer *tr, uint32_t frame_index, ls_frame *out);

/* As ls_trace_scene but leaves the results on the device (out->points32 / hits are NULL,
 * n_points is not read back): nothing in it blocks the host.  The results are ordered on the handle's
 * stream when the call returns -- unless LS_OPT_PIPELINE keeps several frames in flight (see there). */
int ls_trace_scene_async(ls_tracer *tr, uint32_t frame_index, ls_frame *out);

/* traceScene for a caller whose cloud lives in ordinary host memory (PointCloud2::data, EmbreeTracer.cpp:297-367), in two
 * steps that overlap the device, the PCIe link and the host:
 *   ls_trace_scene_begin   launches the frame and returns as soon as the HIT COUNT is known -- the pack pass is still
 *                          running -- so that the caller can size its cloud (data.resize(32 * n_points)) meanwhile;
 *   ls_trace_scene_expand  writes the n_points 32-byte records (XYZIRBytes.cpp:24-40) to dst_points32 with the library's
 *                          worker threads: the first half of the cloud while the second half is still crossing PCIe as
 *                          8-byte (ray, t) records, from which the host rebuilds xyz = t * direction with the factor
 *                          tables and the operation order of the device (the same bits).  Returns when the cloud is
 *                          complete.
 * Same results as ls_trace_scene + ls_expand_points; -1 / zero points on an empty scene.  One frame in flight. */
int ls_trace_scene_begin(ls_tracer *tr, uint32_t frame_index, uint32_t *n_points);
int ls_trace_scene_expand(ls_tracer *tr, void *dst_points32);

/* ---- ITracer::getGeometryCount (ITracer.hpp:101) */
long ls_geometry_count(ls_tracer *tr);

/* Per-name getters of EmbreeTracer (EmbreeTracer.cpp:82-113, :369-439); LS_ERR_UNKNOWN_GEOMETRY if the name is not
 * registered (the reference returns -1 from getGeometryId and throws TraceException codes 1 / 4 / 8 from
 * getVertexCount / getElementCount / getGeometryType: the adapter maps the status to exactly those). */
int ls_geometry_id(ls_tracer *tr, const char *name);
long ls_vertex_count(ls_tracer *tr, const char *name);
long ls_element_count(ls_tracer *tr, const char *name);
/* EmbreeTracer::getGeometryType (EmbreeTracer.cpp:103-113; test/EmbreeTracer_test.cpp:116-120): the LS_GEOMETRY_TYPE_*
 * the geometry was added with (= the RTCGeometryType value). */
int ls_geometry_type(ls_tracer *tr, const char *name);

/* LidarDevice::getTotalRays / getTotalChannels (LidarDevice.cpp:411-419) for this handle. */
uint32_t ls_total_rays(ls_tracer *tr);
uint32_t ls_total_channels(ls_tracer *tr);

const char *ls_last_error(ls_tracer *tr);
int ls_abi_version(void);
/* Sixteen hex digits: SHA-256 over the library's sources (every .hip / .h / .cpp file of csrc: file name then contents, in sorted order)
 * as they were when THIS binary was built.  bench.py prints it next to the hash of the sources it finds, so that a stale
 * .so cannot speak for newer sources (the library is built in-tree and travels to the GPU box as a binary). */
const char *ls_source_hash(void);

/* ---- multi-GPU: restrict this handle to the azimuth columns [first_az, first_az + n_az) of every
 * channel.  Ray indices in ls_hit stay global.  Default: the full revolution. */
int ls_tracer_set_shard(ls_tracer *tr, uint32_t first_az, uint32_t n_az);

/* Multi-GPU collection (the all-gatherv of hit records).  Each rank points its outputs
 * (ls_tracer_set_output_buffers) into a slot of 64 + 16*capacity bytes: [n_points u32 | pad to 64 B |
 * capacity ls_hit records] -- the 32-byte points need not travel, they are a function of (ray, t).
 * After one all-gather of the slots (RCCL, in rank order), this call compacts the `world` slots at
 * d_gathered into one contiguous cloud on the device: d_hits (all records, ascending azimuth
 * sector), d_points32 (rebuilt points), *d_n_points.  Stream-ordered on the handle's stream. */
int ls_expand_gathered_hits(ls_tracer *tr, const void *d_gathered, uint32_t world, uint32_t capacity, void *d_points32,
                            void *d_hits, uint32_t *d_n_points);
/* The same on a stream of the caller's (a hipStream_t): the collective's stream, so that the compaction follows the
 * gather without holding up the tracer's stream (include/lidarshooter_group.h does this). */
int ls_expand_gathered_hits_on(ls_tracer *tr, void *hip_stream, const void *d_gathered, uint32_t world, uint32_t capacity,
                               void *d_points32, void *d_hits, uint32_t *d_n_points);
/* The sized gather's form (include/lidarshooter_group.h, LS_GROUP_FLAG_SIZED_GATHER): only the FRONT of every slot travelled --
 * the header with the rank's true count and the first gathered_capacity records; the `world` pieces lie 64 + 16 *
 * gathered_capacity bytes apart.  The cloud is rebuilt from the records that are there, and 64 bytes of pinned host memory
 * (host_stat64; may be NULL) receive { u32 largest true count of any rank, u32 truncated (some rank had more hits than
 * travelled), u32 epoch (released last) }. */
int ls_expand_gathered_hits_sized(ls_tracer *tr, void *hip_stream, const void *d_gathered, uint32_t world, uint32_t gathered_capacity,
                                  void *d_points32, void *d_hits, uint32_t *d_n_points, void *host_stat64, uint32_t epoch);

/* The step after the tracer: the sensor-frame cloud into the world frame, on the
 * device.  Replaces CloudTransformer::applyInverseTransform (CloudTransformer.cpp:283-318) +
 * LidarDevice::originToSensorInverse (LidarDevice.cpp:393-401): p_world = R * (T * p) + t for the
 * x,y,z of every 32-byte point; T = affine3x4 (row-major, NULL = identity), R = the sensor's
 * sensorToBase rotation (row-major; the handle only holds its inverse), t = the handle's translation.
 * d_points32_in holds *d_n_points records (as ls_trace_scene_async leaves them); they are written to
 * d_points32_out starting at record *d_out_base (NULL = 0) -- in == out with base 0 transforms in
 * place -- and *d_out_total (NULL = not wanted) receives *d_out_base + *d_n_points, so the clouds of
 * several sensors merge into one buffer by chaining total -> base.  Records that would not fit
 * out_capacity are dropped.  Stream-ordered on the handle's stream. */
int ls_cloud_to_world(ls_tracer *tr, const float *affine3x4, const float *R, const void *d_points32_in,
                      const uint32_t *d_n_points, void *d_points32_out, const uint32_t *d_out_base,
                      uint32_t *d_out_total, uint32_t out_capacity);

/* Run all device work of this handle on `hip_stream` (a hipStream_t; NULL = the handle's own
 * stream).  Lets the caller order its collectives after ls_trace_scene_async. */
int ls_tracer_set_stream(ls_tracer *tr, void *hip_stream);
int ls_tracer_synchronize(ls_tracer *tr);
/* LS_OPT_PIPELINE: order the handle's stream after every frame still in flight (no host wait). */
int ls_tracer_flush(ls_tracer *tr);
/* Finer than a flush, for a consumer that works on frames one by one while later frames are already in flight (the
 * collective stream of include/lidarshooter_group.h):
 *   ls_tracer_order_after_last_frame  orders hip_stream (a hipStream_t) after the frame issued last -- its points, hit
 *       records and count are complete for work enqueued on hip_stream afterwards -- and after nothing else: with
 *       three frames in flight the two other frames keep running.
 *   ls_tracer_wait_event  makes everything the handle does from now on (its next frames included, whatever stream
 *       carries them) start after hip_event (a hipEvent_t) has completed -- e.g. the event behind the last reader of an
 *       output buffer that the next frame writes again.
 *   ls_tracer_next_frame_waits  the narrow form of the same: only the frame issued NEXT starts after hip_event (with three
 *       frames in flight that is one wait on that frame's stream instead of three runtime calls; the frames after it are
 *       not ordered behind the event unless they are behind that frame anyway). */
int ls_tracer_order_after_last_frame(ls_tracer *tr, void *hip_stream);
int ls_tracer_wait_event(ls_tracer *tr, void *hip_event);
int ls_tracer_next_frame_waits(ls_tracer *tr, void *hip_event);

/* Write packed points / hit records into caller-owned device buffers (capacity in records,
 * >= ls_total_rays of the shard) instead of the handle's own; NULL restores the default. */
int ls_tracer_set_output_buffers(ls_tracer *tr, void *d_points32, void *d_hits, uint32_t *d_n_points,
                                 uint32_t capacity);
/* The same for hit records alone (LS_OPT_EMIT_POINTS = 0: a sharded group rebuilds the points of the whole frame from the
 * gathered records, include/lidarshooter_group.h): no point buffer exists, so while these buffers are installed
 * LS_OPT_EMIT_POINTS = 1 is refused, and a trace with it set fails with LS_ERR_INVALID_ARGUMENT instead of writing 32 bytes
 * per hit through a pointer that was never meant for them.  NULL d_hits restores the default. */
int ls_tracer_set_hit_buffers(ls_tracer *tr, void *d_hits, uint32_t *d_n_points, uint32_t capacity);

/* ---- options */
#define LS_OPT_LEAF_SIZE 1      /* triangles per BVH leaf (1,2,4,8), default 1; takes effect at next commit  */
#define LS_OPT_TIMING 2         /* 1: bracket every stage with hipEvents, 2: only the trace kernel        */
#define LS_OPT_COUNT_VISITS 3   /* 1: trace kernel also counts node fetches / triangle tests              */
#define LS_OPT_PIPELINE 6       /* frames in flight (projection engine, asynchronous API).  0 (default): one.
                                 * 1: two, on the handle's stream -- the finish + pack workgroups of a frame ride in the
                                 *    launch of the next frame's k_project; a frame's outputs are ordered on the
                                 *    handle's stream after the NEXT ls_trace_scene_async.
                                 * 2: three -- whole frames rotate over three streams of the library; outputs are ordered
                                 *    on the handle's stream by ls_tracer_flush (no event or wait per frame).
                                 * In both modes ls_tracer_flush / ls_tracer_synchronize complete everything, the
                                 * library's own output buffers rotate with the frames (a caller that sets output
                                 * buffers rotates them itself), and meshes handed over with
                                 * ls_update_geometry_device_shared must stay unchanged while frames are in flight.  */
#define LS_OPT_HOST_OUTPUT 7    /* synchronous ls_trace_scene: 1 (default) the pack kernel writes points (and hit
                                 *    records) straight into the pinned host buffers that ls_frame returns -- one
                                 *    host wait per frame, no copy engine; 2: the same with 16-byte compact point
                                 *    records (ls_frame.compact16, expanded by ls_expand_points); 0: device buffers,
                                 *    then count + sized D2H copies (two waits).                               */
#define LS_OPT_READBACK_HITS 8  /* synchronous ls_trace_scene: 1 (default) ls_frame.hits is filled; 0: the 16-byte
                                 *    hit records stay on the device (ls_frame.hits = NULL, d_hits valid) -- the ITracer
                                 *    adapter only needs the 32-byte points.                                   */
/*      option 9 is a test hook (lidarshooter_hip_debug.h: LS_OPT_DEBUG_FAULT); not part of this surface             */
#define LS_OPT_BVH_REFIT 11     /* BVH engine: 1 (default) a commit after which only vertices / poses differ refits the
                                 *    hierarchy (OptixTracer.cpp:532-535 OPERATION_UPDATE): no key pass, no sort; 0: always
                                 *    a full build.  Identical results.                                                   */
#define LS_OPT_BVH_INSTANCED 12 /* BVH engine: 1 (default) one hierarchy per geometry, built once in MESH space; every frame
                                 *    carries the rays into each geometry's mesh space and tests a leaf's triangles exactly as
                                 *    the other paths do (corners through the frame's transform, same bits) -- a commit after
                                 *    which only poses differ, the sensor's or a mesh's, builds and refits nothing; new vertices refit that geometry
                                 *    alone (LS_OPT_BVH_REFIT), new indices rebuild it.  Scenes of
                                 *    more than 16 geometries or with a (nearly) singular mesh matrix take the classic path
                                 *    (0: always): one hierarchy in the sensor frame, refitted per LS_OPT_BVH_REFIT.
                                 *    Identical results.  Takes effect at the next commit.                                */
#define LS_OPT_BLOCK_CULL 10    /* projection engine, meshes of 524 288 triangles or more: keep the mesh in Morton order with a
                                 *    bound per 4 triangles and drop, before their indices are read, the groups that no ring
                                 *    of the raster and no column of the shard can meet.  0 off, 1 on, 2 (default) auto: on for
                                 *    geometries of 2 000 000 triangles or more (where the kernel is bandwidth-bound), and
                                 *    from 524 288 triangles when the handle is an azimuth shard narrower than the raster
                                 *    (ls_tracer_set_shard: most groups then lie outside the sector).  Identical results.  */
#define LS_OPT_UPLOAD_MODE 13   /* ls_update_geometry from host memory: 1 (default) one copy straight from the caller's pageable
                                 *    memory at PCIe rate, the call returns when the memory has been read; 0: worker threads
                                 *    stage it through pinned memory chunk by chunk, the call never waits for the device
                                 *    (measured slower: 0.26-0.31 ms against 0.15 ms for 8 MB); 2: one thread, one copy.  */
#define LS_OPT_ENGINE 5         /* closest-hit engine: 0 auto (default), 1 BVH traversal, 2 sensor-space
                                 *    projection (streams triangles over the ray raster); identical results.
                                 *    Takes effect at the next commit.                                      */
#define LS_OPT_BVH_WIDE 16      /* BVH engine, instanced mode: 1 (default) the trace walks FOUR-wide nodes made of the binary hierarchy (a
                                 *    node's slots are its grandchildren: half the trips per ray, four slab tests in flight per trip;
                                 *    + 128 bytes per node) -- made at the commit for hierarchies of up to 65 536 leaves, and for bigger
                                 *    ones by the second frame that finds them unchanged (34 us per million nodes: a hierarchy rebuilt
                                 *    or refitted every frame never pays it and is walked through its binary nodes); 0: the binary
                                 *    nodes always.  Identical results.  Takes effect at the next commit.                            */
#define LS_OPT_EMIT_POINTS 15   /* ls_trace_scene_async: 1 (default) the pack pass writes the 32-byte points and the 16-byte hit
                                 *    records; 0: the hit records only (d_points32 stays untouched) -- for a consumer that
                                 *    rebuilds points from (ray, t) anyway: a sharded group gathers hit records and
                                 *    ls_expand_gathered_hits rebuilds every rank's points from them (8 MB of writes per
                                 *    frame less at 524 288 rays).  The synchronous ls_trace_scene always delivers points.  */
#define LS_OPT_FRAME_GRAPH 14   /* LS_OPT_PIPELINE = 2 (three frames in flight, projection engine): 1 = the launches of a frame
                                 *    are captured ONCE per stream of the rotation into a HIP graph and every later frame
                                 *    on that stream is one hipGraphLaunch; the kernel nodes whose arguments changed since
                                 *    (a pose, an output buffer, the shard) are patched first
                                 *    (hipGraphExecKernelNodeSetParams); a change of the launch sequence itself (another
                                 *    set of geometries, culling switched) captures anew.  0 (default): plain launches.
                                 *    Identical results; host cost per frame 9 -> 6 us for the three launches of a frame,
                                 *    26 -> 6-8 us for a sharded group frame (tools/micro/graph_launch.hip).  A runtime
                                 *    that refuses the capture leaves the handle on plain launches
                                 *    (LS_INFO_FRAME_GRAPH_STATE).                                                        */
#define LS_OPT_STANDING 17      /* projection engine: 1 (default) a geometry that has not changed for a few commits -- its
                                 *    vertices, indices and pose, the sensor's pose and raster, the shard, its place in the
                                 *    scene -- gets a STANDING LIST: one 64-byte record per triangle whose footprint on the
                                 *    raster holds a cell (a sixth of a large ground mesh), built once by a launch of its own;
                                 *    frames then expand the list instead of streaming the mesh.  Any change drops the list at
                                 *    the next commit (a frame checks once more before it uses one) and a geometry that keeps
                                 *    moving stops getting builds.  At most min(n, max(n / 4, 4096)) records for n triangles:
                                 *    16 bytes per triangle; a mesh with more footprints is never standing.  Not used by
                                 *    frames with LS_OPT_COUNT_VISITS, LS_OPT_TIMING or LS_OPT_PIPELINE = 1, nor between
                                 *    ls_frame_graph_begin and ls_frame_graph_end.  With LS_OPT_FRAME_GRAPH a list that comes
                                 *    into use or goes is another launch sequence: the graphs are captured anew, so a list is taken
                                 *    into use there only after 64 unchanged commits, or when no graph is cached.  0: frames always
                                 *    stream the meshes.  Identical results.  Takes effect at the next frame.
                                 *    While the set of geometries traced from their lists stays the same from frame to frame,
                                 *    the per-ray minimum those lists give is kept too (the STANDING BASE, 8 bytes per ray of
                                 *    the shard): frames start from it and launch nothing for the standing geometries.  Not
                                 *    with LS_OPT_FRAME_GRAPH, nor in the two-step trace.  0 switches lists and base off.    */
int ls_tracer_set_option(ls_tracer *tr, int option, int value);

/* A frame graph that also holds work of the CALLER's (include/lidarshooter_group.h: the frame's collective and the
 * rebuild of the gathered cloud), so that the whole frame is one graph launch.  Needs LS_OPT_PIPELINE = 2 and
 * LS_OPT_FRAME_GRAPH = 1.
 *   ls_frame_graph_begin   the next ls_trace_scene_async leaves its frame graph open.  `tag` names the caller's part: a
 *                          graph captured under another tag is captured anew.
 *   ls_frame_graph_stream  after that ls_trace_scene_async: the stream (a hipStream_t) the frame is on, which of the three
 *                          streams of the rotation it is (0..2: one graph, hence one set of caller buffers, per slot;
 *                          LS_FRAME_NO_SLOT for a frame that ran on the handle's own stream: timing / counting frames) and
 *                          how it is being built: LS_FRAME_EAGER (plain launches: the caller enqueues its own work on the
 *                          stream as usual), LS_FRAME_CAPTURING (the stream is capturing: the caller enqueues its work on
 *                          it ONCE, kernels of this library through this library's entry points, and it becomes part of the
 *                          graph) or LS_FRAME_REPLAYING (the graph exists: the caller enqueues NOTHING except through
 *                          this library's entry points, which only compare their arguments with the captured ones).
 *   ls_frame_graph_end     closes the graph and launches it.  Returns 0, or 1 = nothing was launched, the graph was
 *                          discarded (the launch sequence changed, or the runtime refused the capture): issue the
 *                          frame again from ls_frame_graph_begin (at most once more).
 *   ls_frame_graph_reset   destroys the cached graphs (a caller whose captured work dies -- a communicator -- calls it). */
#define LS_FRAME_NO_SLOT 0xFFFFFFFFu
#define LS_FRAME_EAGER 0
#define LS_FRAME_CAPTURING 1
#define LS_FRAME_REPLAYING 2
int ls_frame_graph_begin(ls_tracer *tr, uint64_t tag);
int ls_frame_graph_stream(ls_tracer *tr, void **hip_stream, uint32_t *slot, int *mode);
int ls_frame_graph_end(ls_tracer *tr);
int ls_frame_graph_reset(ls_tracer *tr);

/* Rebuild n_points 32-byte PointCloud2 records (XYZIRBytes.cpp:24-40; intensity 64.0, EmbreeTracer.cpp:343) at
 * dst_points32 from the compact records of ls_frame.compact16, with the library's worker threads. */
int ls_expand_points(void *dst_points32, const void *compact16, uint32_t n_points);

/* Copy `bytes` from src to dst with the library's worker threads (both host pointers).  The adapter
 * uses it to move a frame's points from the pinned buffer of ls_frame into PointCloud2::data; a single
 * thread moves 8 MB in ~0.7 ms, the PCIe transfer of the same bytes takes 0.15 ms. */
int ls_parallel_copy(void *dst, const void *src, uint64_t bytes);

/* Facts about the handle: returns the value or a negative ls_status. */
#define LS_INFO_CONCURRENT_STREAMS 1 /* LS_OPT_PIPELINE = 2: mutually concurrent streams found by the calibration
                                      *    (3 = full three-stream mode; fewer: the handle runs mode 1 instead)    */
#define LS_INFO_PIPELINE_MODE 2      /* the frames-in-flight mode actually in use (0, 1 or 2)                    */
#define LS_INFO_DEVICE_STATUS 3      /* sticky device status word (0 = ok); read-and-clear, synchronises          */
#define LS_INFO_HOST_THREADS 4       /* worker threads of the host copy pool                                     */
#define LS_INFO_AZIMUTH_COUNT 5      /* H: azimuth columns of the sensor's full raster (whatever the shard)       */
#define LS_INFO_LAST_COMMIT_REFIT 6  /* BVH engine: 1 if the last commitScene refitted instead of rebuilding      */
#define LS_INFO_BVH_INSTANCED 7      /* BVH engine: 0 classic hierarchy; 1 instanced and the last commit built nothing;
                                      *    2 instanced and the last commit (re)built some geometry's hierarchy        */
#define LS_INFO_NEXT_SLOT 8           /* LS_OPT_PIPELINE = 2: which of the three streams (0..2) the NEXT frame runs on   */
#define LS_INFO_FRAME_GRAPH_STATE 9   /* 0 off, 1 on, 2 on but the runtime refused a capture: plain launches since       */
#define LS_INFO_FRAME_GRAPH_CAPTURES 10 /* frame graphs captured so far                                                  */
#define LS_INFO_FRAME_GRAPH_REPLAYS 11  /* frames issued as one graph launch                                              */
#define LS_INFO_FRAME_GRAPH_PATCHES 12  /* kernel nodes patched with new arguments before a replay                        */
#define LS_INFO_FRAME_GRAPH_LAST_PATCHED 13 /* bit i: launch i of the frame replayed last went out with new arguments     */
#define LS_INFO_EMIT_POINTS 14       /* the current LS_OPT_EMIT_POINTS                                            */
#define LS_INFO_BVH_WIDE 16                /* 1: the last trace walked the four-wide nodes (LS_OPT_BVH_WIDE, instanced mode, every geometry's made) */
#define LS_INFO_FRAME_GRAPH_PATCH_WAITS 15 /* patches that first had to wait for the previous launch of their graph (the host ran more than three frames ahead) */
#define LS_INFO_RAY_QUERY_BUILT 17         /* geometries whose query hierarchy the last ls_trace_rays* / ls_occluded_rays* / ls_closest_points* built or refitted (see there) */
#define LS_INFO_STANDING_GEOMETRIES 18     /* LS_OPT_STANDING: geometries the last frame traced from their standing lists   */
#define LS_INFO_STANDING_BUILDS 19         /* standing lists built so far                                                    */
#define LS_INFO_STANDING_RECORDS 20        /* records in the lists the last frame used                                       */
#define LS_INFO_STANDING_BASE 21           /* 1: the last frame started from the standing base (LS_OPT_STANDING)             */
#define LS_INFO_STANDING_BASE_BUILDS 22    /* standing bases built so far                                                    */
#define LS_INFO_STANDING_BASE_NO_FINISH 23 /* frames so far that started from the base with nothing left to project: no finish pass */
long ls_get_info(ls_tracer *tr, int what);

/* Mean stage durations (milliseconds, hipEvents on the handle's stream) over every frame recorded
 * since the previous call; recording never synchronises, this call does.  Returns the number of
 * frames averaged (>= 0) or a negative ls_status. */
#define LS_T_TRANSFORM 0
#define LS_T_MORTON 1
#define LS_T_SORT 2
#define LS_T_LEAVES 3
#define LS_T_RANGE_TREE 4
#define LS_T_HIERARCHY 5
#define LS_T_TRACE 6      /* BVH: traversal kernel; projection: per-triangle footprint kernel */
#define LS_T_TRACE_AUX 7  /* BVH: row counts; projection: long-row kernel + resolve          */
#define LS_T_PACK 8
#define LS_T_COUNT 9
int ls_get_timings(ls_tracer *tr, float ms[LS_T_COUNT]);

/* Totals of the last trace when LS_OPT_COUNT_VISITS is on: {node fetches, triangle tests,
 * sum over waves of traversal-loop trips (a wave runs as long as its slowest lane), max trips}. */
int ls_get_visit_counts(ls_tracer *tr, uint64_t counts[4]);

/* ---- ray generation on its own: LidarDevice::allRaysGPU (LidarDeviceKernels.cu:25-126).
 * Writes the shard's rays as SoA float arrays of n = ls_total_rays() entries each, in device
 * memory owned by the caller: dir_x, dir_y, dir_z (origins are all zero, LidarDevice.cpp:320).  The kernel runs on the handle's
 * stream, behind whatever the device's default stream held when the call was made (a fill of the new buffers, say): one event
 * recorded there, no host wait.  As any call that touches the default stream it must not be made while the calling thread captures a
 * stream of its own; while the handle's frame graph is open it is not ordered at all. */
int ls_generate_rays(ls_tracer *tr, float *d_dir_x, float *d_dir_y, float *d_dir_z);

/* The same kernel's two outputs in the reference's own layout (LidarDeviceKernels.cu:38-51): n = ls_total_rays() records
 * each, in ray-index order, device memory owned by the caller.
 *   d_rays:  lidarshooter::Ray, 32 bytes (Ray.hpp:16-35): origin xyz f32@0 (0, 0, 0), tmin f32@12, direction xyz f32@16,
 *            tmax f32@28.  The reference's kernel leaves tmin / tmax as it found them; here they are written as its
 *            OptiX programs use them: tmin 0, tmax 1e16 (OptixTracerModules.cu:45-46).
 *   d_hits:  lidarshooter::Hit, 24 bytes (Hit.hpp:16-29): t f32@0 = 1e16 ("no hit yet"), normal xyz f32@4 (left alone by
 *            the reference; written as 0 here), intensity f32@16 = 64.0, ring i32@20 = the channel index.
 * Either pointer may be NULL (that output is skipped).  Stream order as ls_generate_rays. */
int ls_generate_rays_aos(ls_tracer *tr, void *d_rays, void *d_hits);

/* ---- ray queries: the closest hit of each of n CALLER rays against the scene as of the last successful ls_commit_scene
 * (the geometries' current poses, as a frame would use them) -- scan patterns that are not a uniform raster, several sensors
 * on one scene, "what does this ray hit", "is anything between A and B" (a ray with a tmax; ls_occluded_rays below answers
 * that one without searching for the closest hit).
 *   d_rays: n lidarshooter::Ray records, 32 bytes each (origin xyz f32@0, tmin f32@12, direction xyz f32@16, tmax f32@28) --
 *           the layout ls_generate_rays_aos writes -- in the handle's SENSOR frame (the frame of ls_frame.points32; a caller
 *           whose rays are in the world frame creates the handle with Rinv = I, t = 0).  16-byte aligned.
 *   d_out:  n ls_hit records (16-byte aligned) in ray order: ray = index, geom / prim as in ls_frame.hits, t = distance along
 *           the direction as given (not normalised); a miss is geom = prim = 0xFFFFFFFF, t = -1.
 * A triangle counts when the frame's exact test hits it (Embree's Moeller-Trumbore, from the ray's own origin) and
 * tmin <= t <= tmax; equal t: the lowest (geomID, primID) wins, as in frames.  A ray with a non-finite origin or direction,
 * a zero direction, a NaN bound or tmin > tmax is a miss (tmax = +inf is no bound).
 * Enqueued on hip_stream (NULL: the handle's stream) after everything already issued on the handle; returns without waiting.
 * What the handle issues afterwards on its own stream (mesh copies, commits, the next query) comes after the query; frames of
 * the three-stream rotation (LS_OPT_PIPELINE = 2) may overlap it.
 * Returns what ls_trace_scene returns in the same state: -1 with no commit or an empty scene (out is not written),
 * LS_ERR_NOT_COMMITTED when a geometry was removed since the commit; LS_ERR_INVALID_ARGUMENT for NULL pointers with n > 0
 * and while a frame graph is open; n = 0 launches nothing.
 * The query uses hierarchies of its own, one per geometry, built at the first query after a commit that changed a
 * geometry's vertices (a refit) or indices (a rebuild) -- a commit after which only poses changed builds nothing
 * (LS_INFO_RAY_QUERY_BUILT = 0) -- in mesh space; a geometry whose pose has no usable inverse (scaled to zero, a scale
 * ratio above 10^3) is kept in the sensor frame instead and rebuilt when its pose changes.  Memory: about 0.3 GB per
 * million triangles at leaf size 1 (48-byte records, 64-byte binary and 128-byte four-wide nodes, range boxes, sorted keys;
 * counted from those sizes, not measured), on top of the frame path's own; LS_OPT_ENGINE does not matter. */
int ls_trace_rays(ls_tracer *tr, void *hip_stream, const void *d_rays, uint32_t n, void *d_out);
/* The same with host memory (pageable) in and out, on the handle's stream; returns when out is filled. */
int ls_trace_rays_host(ls_tracer *tr, const void *rays, uint32_t n, void *out);

/* ---- occlusion queries: whether each of n CALLER rays hits anything -- the any-hit half of the ray queries (Embree's
 * rtcOccluded, OptiX's terminate-on-first-hit): line of sight, visibility labels, multi-sensor coverage, shadow rays.
 *   d_rays: as ls_trace_rays (n 32-byte lidarshooter::Ray records in the sensor frame, 16-byte aligned).
 *   d_out:  n bytes in ray order, any alignment: 1 when some triangle of the committed scene passes the frame's exact test
 *           from the ray's origin with tmin <= t <= tmax, else 0 -- by definition exactly when ls_trace_rays, in the same state,
 *           reports a hit (geom != 0xFFFFFFFF) for that ray.  Degenerate rays (as there) give 0.
 * The walk stops at the first triangle that passes: no closest hit is searched for, no tie broken.
 * A segment A -> B: origin A, direction B - A, tmax = 1 - eps (B on a surface: its own triangle is hit at t ~ 1).
 * Return codes, stream order, the frame graph and n limits, and the query hierarchies are those of ls_trace_rays; both queries
 * share the hierarchies (what one built or refitted serves the other), and LS_INFO_RAY_QUERY_BUILT reports for whichever ran
 * last. */
int ls_occluded_rays(ls_tracer *tr, void *hip_stream, const void *d_rays, uint32_t n, void *d_out);
/* The same with host memory (pageable) in and out, on the handle's stream; returns when out is filled. */
int ls_occluded_rays_host(ls_tracer *tr, const void *rays, uint32_t n, void *out);

/* ---- nearest-point queries: the closest point of the scene's surface to each of n CALLER points (Embree's rtcPointQuery):
 * cloud-to-mesh residuals of a recorded scan, labelling scan points with the (geomID, primID) they lie on, clearance of a pose.
 *   d_points: n records of 16 bytes, 16-byte aligned: x, y, z f32@0/4/8 in the handle's SENSOR frame (as the ray queries),
 *             radius f32@12 = the largest distance of interest (+inf: no bound).
 *   d_out:    n records of 32 bytes, 16-byte aligned, in input order: the closest surface point qx, qy, qz f32@0/4/8 (sensor
 *             frame), dist f32@12, geom u32@16 and prim u32@20 as in ls_hit (a quad geometry: the quad index), index u32@24 =
 *             the position in the input, u32@28 = 0.  A miss: geom = prim = 0xFFFFFFFF, dist = -1, q = 0.
 * Every triangle of the scene as of the last successful ls_commit_scene, corners through the frame's own transform, gives
 * (q, d2) by ONE float32 operation sequence (Ericson's seven regions; ls_debug_closest_on_triangle in
 * lidarshooter_hip_debug.h runs the same sequence on the host); it counts when d2 is finite and d2 <= radius * radius (the
 * float32 product).  The answer is the triangle with the smallest d2 -- equal d2: the lowest (geomID, primID) --, dist =
 * sqrtf(d2): bit for bit what a loop over all triangles gives.  A point with a non-finite coordinate, a NaN or negative
 * radius: a miss.  Triangles with a non-finite corner or no area never count.
 * Return codes, stream order, the frame graph and n limits, and the query hierarchies are those of ls_trace_rays: the three
 * queries share the hierarchies, and LS_INFO_RAY_QUERY_BUILT reports for whichever ran last.  While a query of more than 16
 * geometries is in flight the last word of a record holds an intermediate value. */
int ls_closest_points(ls_tracer *tr, void *hip_stream, const void *d_points, uint32_t n, void *d_out);
/* The same with host memory (pageable) in and out, on the handle's stream; returns when out is filled. */
int ls_closest_points_host(ls_tracer *tr, const void *points, uint32_t n, void *out);

/* ---- hit attributes: what RTCHit carries beyond (geomID, primID, t) -- the geometric normal Ng and the barycentrics u, v --
 * plus the incidence cosine and which half of a quad was hit, for hit records of the frame (ls_frame.d_hits / hits) or of
 * ls_trace_rays: incidence for intensity / drop-out models, labelled normals, point-to-plane residuals, interpolation of
 * per-vertex data.  No hierarchy is built or walked: a gather over the records.
 *   d_hits:  n ls_hit records, 16-byte aligned, in any order, a subset is fine; hit.ray indexes the rays.
 *   d_rays:  non-NULL: the n_rays 32-byte lidarshooter::Ray records (sensor frame, 16-byte aligned) that were given to
 *            ls_trace_rays; a hit with ray >= n_rays is invalid.  NULL: the handle's own sensor rays -- hit.ray is the global
 *            ray index v * H + h of the full raster whatever the shard, origin 0, direction the factor-table products the
 *            trace kernels form; n_rays is ignored, the bound is V * H.
 *   d_count: NULL, or a device word: min(n, *d_count) records are handled and nothing is written beyond them (the records
 *            of ls_trace_scene_async: d_hits, d_n_points, n = the capacity -- no host read-back).
 *   d_out:   one 48-byte record per handled hit, 16-byte aligned, in input order:
 *              nx, ny, nz f32@0   unit geometric normal in the sensor frame, along (v1 - v0) x (v2 - v0): Embree's Ng direction
 *              cos_inc f32@12     -(n . d) / |d| clamped to [-1, 1]; positive: the ray meets the front face
 *              u, v f32@16        Embree's barycentrics: hit point = (1 - u - v) v0 + u v1 + v v2
 *              tri u32@24         triangle inside the geometry: prim, or 2 prim / 2 prim + 1 of a quad (Embree's split
 *                                 (v0,v1,v3), (v2,v3,v1))
 *              flags u32@28       bit 0 = valid, the other bits 0
 *              px, py, pz f32@32  o + t d per axis (one product, one sum); a sensor ray: t d, the bits of the frame's points32 xyz
 *              ray u32@44         hit.ray
 * A record is valid when geom names a geometry of the committed scene, prim < its element count, the ray index is in range
 * and the library's exact test from the ray's origin against the named triangle -- corners through the frame's own transform
 * as of the geometries' current poses, like the other queries -- passes with t bit-equal to hit.t; a quad: the first of its
 * two triangles for which that holds.  Anything else -- a miss record, a stale hit of a geometry moved since, a wrong or
 * removed id, a t that is one ulp off or NaN -- gets flags = 0 and zeros everywhere but `ray`.  Every index is checked
 * before an address is formed from it.  The values are ONE float32 operation sequence (csrc/ls_hit_attr.h), which
 * ls_debug_hit_attributes_on_triangle in lidarshooter_hip_debug.h runs on the host.
 * Return codes, argument checks, stream order and the frame graph rule are those of ls_trace_rays (d_count must be 4-byte
 * aligned); LS_INFO_RAY_QUERY_BUILT is left as it is. */
int ls_hit_attributes(ls_tracer *tr, void *hip_stream, const void *d_rays, uint32_t n_rays,
                      const void *d_hits, const uint32_t *d_count, uint32_t n, void *d_out);
/* The same with host memory (pageable) in and out and no count word, on the handle's stream; returns when out is filled. */
int ls_hit_attributes_host(ls_tracer *tr, const void *rays, uint32_t n_rays,
                           const void *hits, uint32_t n, void *out);

/* ---- sensor returns: from exact hit records to what a LiDAR delivers -- intensity that falls with incidence and range, a
 * range gate, returns too weak to detect dropping out, Gaussian range noise, random drop-out -- for hit records of the frame
 * (ls_frame.d_hits / hits) or of ls_trace_rays.  The kept returns are compacted IN INPUT ORDER into a ready points32 / ls_hit
 * pair in device memory, with their count: no host read-back, no 48-byte attribute record in between. */
#define LS_RETURN_LAMBERT   1u  /* intensity carries the incidence term */
#define LS_RETURN_TWO_SIDED 2u  /* with LAMBERT: |cos_inc| instead of max(cos_inc, 0) */

typedef struct ls_return_model {   /* 64 bytes, no pointers */
    float range_min, range_max;        /* keep when range_min <= r <= range_max, r = t * |d| (true range); 0 / +inf: no gate */
    float intensity_scale;             /* I0; 64.0 with flags = 0 and ref_range = 0 reproduces the frame's constant */
    float ref_range;                   /* r0 > 0: falloff (r0 / max(r, r0))^2; 0: none */
    float intensity_floor;             /* returns with I < floor are lost (0: none) */
    float intensity_max;               /* saturation (+inf: none) */
    float noise_sigma0, noise_sigma1;  /* sigma = sigma0 + sigma1 * r, metres along the ray */
    float dropout;                     /* probability in [0, 1] of losing a return at random */
    uint32_t seed;
    uint32_t flags;
    uint32_t reserved[5];              /* must be 0 */
} ls_return_model;

/*   d_rays, n_rays, d_hits, d_count, n: exactly as ls_hit_attributes (d_rays = NULL: the handle's own sensor rays, hit.ray the
 *            global ray index whatever the shard; d_count: NULL or the device word of ls_trace_scene_async, min(n, *d_count)
 *            records are handled).
 *   d_reflectivity: NULL, or n_reflectivity floats in device memory indexed by geomID; NULL or geom >= n_reflectivity: 1.0.
 *   frame_index: part of the random numbers' counter -- another frame, other noise; the same frame, the same noise.
 *   d_points32: NULL, or room for n 32-byte points in the ls_frame.points32 layout (x, y, z f32@0, 0@12, intensity f32@16,
 *            ring i32@20, 0@24..31), 16-byte aligned; ring = hit.ray / H for sensor rays, 0 for caller rays.
 *   d_hits_out: NULL, or room for n ls_hit records, 16-byte aligned: the kept records with t replaced by the noisy t'.
 *   d_n_out: a device word (not NULL): the count of kept returns.  Nothing is written past record *d_n_out.
 * The outputs must not overlap the inputs.  Per handled record, ONE float32 operation sequence (csrc/ls_return_model.h;
 * ls_debug_return_model in lidarshooter_hip_debug.h runs it on the host):
 *   1. the record counts when ls_hit_attributes calls it valid (the exact test on the named triangle, t bit-equal to hit.t);
 *      an invalid record is lost;
 *   2. len = sqrtf((dx dx + dy dy) + dz dz), r = t * len;
 *   3. c = 1; with LAMBERT max(cos_inc, 0); with LAMBERT | TWO_SIDED |cos_inc|;
 *   4. ref_range > 0: f = q q, q = ref_range / max(r, ref_range); else f = 1;
 *   5. I = ((intensity_scale * rho) * c) * f, and I = intensity_max where it is larger;
 *   6. Philox4x32-10 with key (seed, 0) and counters (hit.ray, frame_index, j, 0), j = 0, 1 -> words a0..a3, b0..b3 -- keyed by
 *      the RAY index, not the record's position: any subset, order or azimuth shard sees the noise of the full turn;
 *      the return is dropped when dropout > 0 and (float)(b2 >> 8) * 2^-24 < dropout; z = (float)((int)S - 393210) * 2^-16 with
 *      S the sum of the twelve 16-bit halves of a0, a1, a2, a3, b0, b1 (standard deviation 1, tails to +-6);
 *   7. both sigmas 0: t' = t; else sigma = noise_sigma0 + noise_sigma1 * r, t' = t + (sigma * z) / len; the point is o + t' d
 *      per axis, t' d with no sum for a sensor ray (the frame's bits);
 *   8. kept when valid, range_min <= r <= range_max, I >= intensity_floor (a NaN intensity is lost), not dropped, t' > 0.
 * LS_ERR_INVALID_ARGUMENT before any device call: a NULL handle or model, a NaN field, range_min > range_max, a negative
 * scale, floor, sigma, ref_range or range_min, dropout outside [0, 1], unknown flag bits, non-zero reserved words,
 * n_reflectivity > 0 with a NULL pointer.  The other return codes, the alignment checks (points and records 16 bytes, the
 * words and the reflectivities 4), stream order and the frame graph rule are those of ls_hit_attributes; -1 writes nothing;
 * n = 0 gives *d_n_out = 0; LS_INFO_RAY_QUERY_BUILT is left as it is.  Calls on one handle use a scratch buffer of the handle
 * (32 bytes per record) one after the other. */
int ls_apply_return_model(ls_tracer *tr, void *hip_stream, const ls_return_model *model, uint32_t frame_index,
                          const void *d_rays, uint32_t n_rays, const void *d_hits, const uint32_t *d_count, uint32_t n,
                          const float *d_reflectivity, uint32_t n_reflectivity,
                          void *d_points32, void *d_hits_out, uint32_t *d_n_out);
/* The same with host memory (pageable) in and out and no count word, on the handle's stream; returns when the outputs are
 * filled (*n_out records of each). */
int ls_apply_return_model_host(ls_tracer *tr, const ls_return_model *model, uint32_t frame_index,
                               const void *rays, uint32_t n_rays, const void *hits, uint32_t n,
                               const float *reflectivity, uint32_t n_reflectivity,
                               void *points32, void *hits_out, uint32_t *n_out);

/* ---- sweep frames: a frame whose SENSOR moves during the turn.  A spinning LiDAR fires azimuth column after column while its
 * carrier drives on, and the cloud it delivers is skewed by that motion: what odometry, deskewing and mapping work against.  The
 * scene is the committed one (no geometry pose is interpolated, no hierarchy touched); every azimuth column has a sensor pose of
 * its own.  One call: the shard's rays through their columns' poses, their closest hits, and the hits compacted into a frame's
 * points32 / ls_hit pair with the count, all in device memory. */
#define LS_SWEEP_DESKEW 1u   /* points in the frame-start sensor frame instead of the instantaneous one */

/*   d_col_pose: n_cols records of 12 floats in device memory, 4-byte aligned, row-major [R_h | o_h] (R[i][j] at 4 i + j, o[i] at
 *            4 i + 3): the sensor's pose at the moment azimuth column h fires, expressed in the handle's sensor frame as the scene
 *            was committed (the frame-start frame; identity records: an ordinary frame).  Indexed by the GLOBAL column whatever the
 *            shard; n_cols must equal LS_INFO_AZIMUTH_COUNT.  Nothing on the host reads the table.
 *   rays:    only the rays of the handle's shard are cast (ls_tracer_set_shard); ray indices stay global, r = v * H + h.  With d
 *            the nominal direction -- the factor-table products the frame kernels and ls_generate_rays_aos form -- ray r has origin
 *            o_h, direction d'_i = (R[i][0] dx + R[i][1] dy) + R[i][2] dz in float32 with no fused multiply-add, tmin 0 and tmax
 *            1e16: ONE operation sequence (csrc/ls_sweep.h; ls_debug_sweep_ray in lidarshooter_hip_debug.h runs it on the host).
 *            An identity record gives d' = d and o = 0 exactly.
 *   hits:    the hit of a ray is by definition what ls_trace_rays returns for that ray record in the same state: the same test,
 *            the same tie-break, the same treatment of degenerate rays -- a column whose pose holds a non-finite value yields
 *            misses.
 *   d_hits:  NULL, or room for `capacity` ls_hit records, 16-byte aligned: {ray, geom, prim, t} of the hits in ascending ray
 *            index, as in a frame.
 *   d_points32: NULL, or room for `capacity` 32-byte points in the ls_frame.points32 layout, 16-byte aligned, intensity 64.0, ring
 *            v.  By default xyz = t * d with no sum, the frame's bits: what the moving sensor reports, each point in the sensor
 *            frame of its own instant.  With LS_SWEEP_DESKEW xyz = o_h + t * d' per axis (one product, one sum): the point in
 *            the frame-start sensor frame -- the bits ls_hit_attributes gives as px, py, pz for that ray.
 *   d_n_points: a device word (not NULL, 4-byte aligned): the count.  Nothing is written past record *d_n_points.
 *   capacity: at least the shard's ls_total_rays(), else LS_ERR_INVALID_ARGUMENT.
 *   d_rays_out: NULL, or room for V * H 32-byte lidarshooter::Ray records, 16-byte aligned: the records of the shard's rays are
 *            written at their global index, the others are left alone.  With them the frame's hit records feed ls_hit_attributes
 *            and ls_apply_return_model as caller rays with n_rays = V * H (the return model then writes ring 0, as it does for all
 *            caller rays).
 * Return codes, stream order, the frame graph rule and the query hierarchies are those of ls_trace_rays (-1 with no commit or an
 * empty scene writes nothing, the count included); LS_INFO_RAY_QUERY_BUILT reports for it; LS_OPT_ENGINE does not matter.
 * LS_ERR_INVALID_ARGUMENT also for a NULL table or count, n_cols != H, unknown flag bits and misaligned pointers.  Frames of
 * ls_trace_scene* are unaffected.  The sweep uses scratch of its own on the handle -- the shard's rays x 32 bytes of contiguous ray
 * records and x 16 bytes of dense hit records, grown on demand and released with the query state --; calls on one handle use it
 * one after the other. */
int ls_trace_scene_sweep(ls_tracer *tr, void *hip_stream, const float *d_col_pose, uint32_t n_cols, uint32_t flags,
                         void *d_points32, void *d_hits, uint32_t *d_n_points, uint32_t capacity, void *d_rays_out);
/* The same with host memory (pageable) in and out, on the handle's stream; returns when the outputs are filled (*n_points
 * records of each; of rays_out the shard's records). */
int ls_trace_scene_sweep_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols, uint32_t flags,
                              void *points32, void *hits, uint32_t *n_points, uint32_t capacity, void *rays_out);

/* Pose table of a sensor moving at a constant twist (host only, no handle, no device): tau_h = t0 + h * dt; R_h = Rodrigues'
 * formula for the rotation ang_vel * tau_h (exactly the identity when |ang_vel| * tau_h == 0), o_h = lin_vel * tau_h -- a constant
 * velocity in the frame-start sensor frame; evaluated in double, rounded once to float32.  col_pose: n_cols records of 12
 * floats.  LS_ERR_INVALID_ARGUMENT for NULL pointers or non-finite inputs. */
int ls_sweep_poses_constant_twist(const float lin_vel[3], const float ang_vel[3], double t0, double dt,
                                  uint32_t n_cols, float *col_pose);

/* ---- beam frames: a frame whose rays are diverging BEAMS with multi-echo returns.  Every other path casts one infinitely thin ray
 * per raster cell; a real LiDAR beam diverges by 1 - 3 mrad: at a silhouette its footprint covers a near and a far surface, on
 * grazing ground it smears over metres of range, and the sensor reports echoes -- the first, the last or the strongest return,
 * often two per beam.  One call: S sub-rays per ray of the shard, their closest hits, the echoes of every beam, and the selected
 * returns compacted into a frame's points32 / ls_hit pair with an echo word per record and the count, all in device memory. */
#define LS_BEAM_FIRST     1u
#define LS_BEAM_LAST      2u
#define LS_BEAM_STRONGEST 4u
typedef struct ls_beam_model {
    const float *pattern;     /* HOST memory: n_samples records of 3 floats (a, b, k) */
    uint32_t n_samples;       /* S, 1..64 */
    uint32_t returns;         /* LS_BEAM_* mask, at least one bit; K = popcount */
    uint32_t min_count;       /* an echo is detectable with >= min_count sub-hits; 1..S */
    float echo_separation;    /* metres, >= 0; +inf: one echo per beam */
    uint32_t reserved[4];     /* must be 0 */
} ls_beam_model;

/*   pattern: the library reads and validates it on the host during the call, and hands it to the kernels by value (768 bytes of
 *            kernel arguments at most): no copy from caller memory outlives the call, and the call does not wait for the device.
 *            Sample s = (a_s, b_s, k_s): tangent offsets along the ring and towards higher elevation (radians for small ones), and
 *            the factor that turns the distance along the sub-ray into the range the sensor reports along its axis.
 *   sub-rays: for ray (v, h) of the shard, with the factor-table entries st = sin_theta[v], ct = cos_theta[v], (cphi, sphi) of
 *            column h: the nominal direction d = (st cphi, st sphi, ct), the tangents u = (-sphi, cphi, 0) and w = (-(ct cphi),
 *            -(ct sphi), st).  Sample s casts origin 0, tmin 0, tmax 1e16, direction d_s,i = (d_i + a_s u_i) + b_s w_i in float32
 *            with no fused multiply-add: ONE operation sequence (csrc/ls_beam.h; ls_debug_beam_ray in lidarshooter_hip_debug.h
 *            runs it on the host).  The sample (0, 0, 1) gives d exactly; a component -0 becomes +0.  The sub-hit of a sub-ray
 *            is by definition what ls_trace_rays returns for that record in the same state.  Sub-ray index: q * S + s, q the
 *            shard-local ray index.
 *   echoes:  r_s = t_s * k_s, one float32 product.  With the sub-hits of a beam ordered by (r ascending, s ascending), an echo
 *            starts at the first of them and at every sub-hit j with r_j - r_{j-1} > echo_separation (a float32 difference).  An
 *            echo carries the range, sample, geom and prim of its nearest member (leading edge: no sums) and its member count
 *            n_e; it is detectable when n_e >= min_count.  Among the detectable echoes FIRST is the nearest, LAST the farthest,
 *            STRONGEST the one with the largest n_e (the nearer of equals).  The distinct selected echoes are the beam's
 *            returns, in ascending range: 0..K per beam.
 *   outputs: device memory, in ascending global ray index and, within a beam, ascending range; any of the three arrays may be
 *            NULL.
 *     d_points32: room for `capacity` 32-byte points in the ls_frame.points32 layout, 16-byte aligned: xyz = r_e * d per axis
 *            with the nominal d and no sum (the range the sensor reports along its axis), intensity = (64.0f * (float)n_e) /
 *            (float)S, ring = v.
 *     d_hits: room for `capacity` ls_hit records, 16-byte aligned: {ray = v * H + h, geom, prim, t = r_e}.
 *     d_echo: room for `capacity` words, 4-byte aligned: bits 0-2 which of FIRST / LAST / STRONGEST the record is, bits 8-14
 *            n_e, bits 16-21 the nearest member's sample, every other bit 0.
 *     d_n_points: a device word (not NULL, 4-byte aligned): the count.  Nothing is written past record *d_n_points.
 *   capacity: at least K times the shard's ls_total_rays().
 * With S = 1, the pattern (0, 0, 1), FIRST and min_count 1 the call returns ls_trace_scene's points, records and count byte for
 * byte.  LS_ERR_INVALID_ARGUMENT before any device call: a NULL handle, model, pattern or count; S outside 1..64; no return bit
 * or unknown ones; min_count outside 1..S; a NaN or negative separation; a non-finite pattern entry or k <= 0; non-zero reserved
 * words; a capacity too small; misaligned pointers.  LS_ERR_OUT_OF_RANGE: the shard's rays times S above 2^27.  The other
 * return codes, stream order, the frame graph rule, the shard handling and the query hierarchies are those of
 * ls_trace_scene_sweep (-1 with no commit or an empty scene writes nothing, the count included); LS_INFO_RAY_QUERY_BUILT reports
 * for it.  Frames of ls_trace_scene* are unaffected.  The call uses scratch of its own on the handle, grown on demand and released
 * with the query state: the shard's rays x S x (32 bytes of ray record + 16 of dense hit record), 48 + 4 bytes per ray for its
 * returns, one word per 256 rays; calls on one handle use it one after the other.
 * Per-sample weights and beams under the per-column poses of ls_trace_scene_sweep: ls_trace_scene_beams_sweep below (here every
 * sub-hit counts once and the sensor is at rest).  Not offered: a call of the ITracer adapter.  ls_apply_return_model refuses these records (ls_hit_attributes calls them invalid): their t is the
 * reported range r_e, not the distance along the sub-ray that the exact test needs. */
int ls_trace_scene_beams(ls_tracer *tr, void *hip_stream, const ls_beam_model *model,
                         void *d_points32, void *d_hits, uint32_t *d_echo, uint32_t *d_n_points, uint32_t capacity);
/* The same with host memory (pageable) out, on the handle's stream; returns when the outputs are filled (*n_points records of
 * each). */
int ls_trace_scene_beams_host(ls_tracer *tr, const ls_beam_model *model,
                              void *points32, void *hits, uint32_t *echo, uint32_t *n_points, uint32_t capacity);

/* A pattern of concentric rings (host only, no handle, no device): S = 1 + n_rings * per_ring samples, at most 64.  Sample 0 is
 * (0, 0, 1); ring j = 1..n_rings, i = 0..per_ring - 1: rho = j / n_rings, phi = 2 pi (i + 0.5 (j - 1)) / per_ring, a =
 * half_angle_az * rho * cos(phi), b = half_angle_el * rho * sin(phi), evaluated in double and rounded once; k = sqrt(1 + (a^2 +
 * b^2)), evaluated in double from the ROUNDED a and b, then rounded once.  pattern: S records of 3 floats.
 * LS_ERR_INVALID_ARGUMENT for a NULL pointer, more than 64 samples or non-finite angles. */
int ls_beam_pattern_rings(float half_angle_az, float half_angle_el, uint32_t n_rings, uint32_t per_ring, float *pattern);

/* ---- beam frames of a moving sensor, with a weight per sample: ls_trace_scene_beams and ls_trace_scene_sweep in one call.  A
 * spinning LiDAR on a moving carrier both diverges and skews, and the power across its footprint is no top hat but roughly a
 * Gaussian: the sub-rays of every beam go through their column's pose, and an echo is as strong as the weights of its members.
 *   model:   exactly as in ls_trace_scene_beams: the same validation, the same limits (S <= 64, the shard's rays x S <= 2^27), the
 *            same capacity rule.
 *   weights: HOST memory: NULL -- every sample weighs 1 -- or n_samples integers, each in 1..65535 (else
 *            LS_ERR_INVALID_ARGUMENT).  Like the pattern they are read and validated during the call and travel in the kernel
 *            arguments (128 bytes on top of the pattern's 768): nothing of the caller's outlives the call.  Integers on purpose: the
 *            strength W_e of an echo, the sum of its members' weights, is exact and independent of any order, and at most 64 x 65535
 *            < 2^24, so exact as a float.
 *   echoes:  formed as in ls_trace_scene_beams: the keys, the (r, s) order, the separation rule.  An echo is detectable when n_e
 *            >= min_count AND W_e >= min_weight (min_weight 0: no strength threshold).  Among the detectable echoes FIRST is the
 *            nearest, LAST the farthest, STRONGEST the one with the largest W_e (the nearer of equals); coinciding selections are
 *            one record, the records in ascending range, as there.
 *   d_col_pose, n_cols: NULL with n_cols 0: the sensor is at rest.  Otherwise the table of ls_trace_scene_sweep: n_cols must equal
 *            LS_INFO_AZIMUTH_COUNT, 12 floats per GLOBAL column, device memory, 4-byte aligned, never read on the host.
 *   sub-rays: sample s of ray (v, h) is ls_trace_scene_beams' sub-ray d_s (a component -0 made +0) carried through the pose of
 *            column h by ls_trace_scene_sweep's sequence: origin o_h, direction d'_s,i = (R[i][0] d_s,x + R[i][1] d_s,y) + R[i][2]
 *            d_s,z, tmin 0, tmax 1e16 -- two existing sequences composed, no new arithmetic (ls_debug_beam_sweep_ray in
 *            lidarshooter_hip_debug.h runs them on the host).  An identity record gives ls_trace_scene_beams' sub-ray bit for bit,
 *            a centre-only pattern ls_trace_scene_sweep's ray; a column whose record holds a non-finite value yields misses for
 *            all its sub-rays, hence no returns.  At rest the sub-rays are ls_trace_scene_beams'.
 *   flags:   0 or LS_SWEEP_DESKEW (other bits: LS_ERR_INVALID_ARGUMENT).  By default xyz = r_e * d per axis with the nominal d
 *            and no sum: ls_trace_scene_beams' points, the sensor's report in the frame of its own instant.  With LS_SWEEP_DESKEW
 *            xyz = o_h + r_e * d' per axis, d' = R_h d (ls_trace_scene_sweep's deskewed point for the nominal direction and the
 *            reported range).  At rest the flag changes nothing.
 *   intensity: (64.0f * (float)W_e) / (float)W_total, W_total the sum of all S weights; with NULL weights (64 n_e) / S, the bits of
 *            ls_trace_scene_beams.  The echo word keeps its layout (n_e in bits 8-14); W_e is not reported apart from the intensity.
 *   d_hits, d_echo, d_n_points, capacity, the order of the records, NULL outputs: as in ls_trace_scene_beams.
 * With NULL weights, min_weight 0 and no table (or an identity table) the call returns ls_trace_scene_beams' bytes.  Return codes,
 * alignment checks, stream order, the frame graph rule, the shard handling and LS_INFO_RAY_QUERY_BUILT are those of
 * ls_trace_scene_beams and ls_trace_scene_sweep; the checks run in the order: frame graph, NULL count, model, weights, pose table
 * and flags, alignment, then the commit (-1 with no commit or an empty scene writes nothing, the count included).  The call uses
 * the scratch of ls_trace_scene_beams on the handle and 12 more bytes per ray; calls on one handle use it one after the other.
 * Not offered: these echoes through ls_apply_return_model (their t is still the reported range); a rays_out; a call of the ITracer
 * adapter; geometries that move during the turn (without beams: ls_trace_scene_sweep_moving below). */
int ls_trace_scene_beams_sweep(ls_tracer *tr, void *hip_stream, const ls_beam_model *model,
                               const uint32_t *weights, uint32_t min_weight,
                               const float *d_col_pose, uint32_t n_cols, uint32_t flags,
                               void *d_points32, void *d_hits, uint32_t *d_echo, uint32_t *d_n_points, uint32_t capacity);
/* The same with host memory (pageable) in and out, on the handle's stream: the table is copied to the device; returns when the
 * outputs are filled (*n_points records of each). */
int ls_trace_scene_beams_sweep_host(ls_tracer *tr, const ls_beam_model *model,
                                    const uint32_t *weights, uint32_t min_weight,
                                    const float *col_pose, uint32_t n_cols, uint32_t flags,
                                    void *points32, void *hits, uint32_t *echo, uint32_t *n_points, uint32_t capacity);

/* Gaussian weights for a pattern (host only, no handle, no device): w_s = max(1, round(65535 exp(-((a_s / sigma_az)^2 + (b_s /
 * sigma_el)^2) / 2))), evaluated in double and rounded once: the centre sample gets 65535.  weights: n_samples words.
 * LS_ERR_INVALID_ARGUMENT for NULL pointers, n_samples outside 1..64, non-finite pattern entries, sigmas that are non-finite or
 * <= 0. */
int ls_beam_weights_gaussian(const float *pattern, uint32_t n_samples, float sigma_az, float sigma_el, uint32_t *weights);

/* ---- sweep frames with GEOMETRIES that move during the turn.  A car that crosses the field of view during the 0.1 s turn is
 * sheared, stretched or compressed in the real cloud, for a sensor at rest as for a moving one; ls_trace_scene_sweep freezes every
 * geometry at its committed pose.  Here a geometry may have a rigid displacement of its own per azimuth column.  Nothing is
 * re-posed and no hierarchy is touched: a moved geometry is a moved ray -- the walk carries the ray through the inverse of the
 * geometry's displacement and tests it against the geometry where it was committed. */
typedef struct ls_geometry_motion {
    uint32_t geom;             /* geomID (ls_add_geometry / ls_geometry_id) */
    uint32_t reserved;         /* must be 0 */
    const float *col_motion;   /* H records of 12 floats, row-major [Q | c]; DEVICE memory for the device call, host memory for _host */
} ls_geometry_motion;

/*   d_col_pose, n_cols: the sensor's pose table of ls_trace_scene_sweep, or NULL with n_cols 0: the sensor is at rest (the nominal
 *            rays from the origin; LS_SWEEP_DESKEW then changes nothing).
 *   motions: HOST memory, n_motions entries, read during the call; geometries not named are at rest.  Each names a geometry of the
 *            committed scene once and gives its table: LS_INFO_AZIMUTH_COUNT records whatever the shard, 4-byte aligned, in device
 *            memory, never read on the host.  Record h is the rigid displacement of the geometry at the moment the GLOBAL azimuth
 *            column h fires, relative to where it was committed, expressed in the handle's sensor frame as the scene was committed
 *            (the frame the sensor poses use): x_h = Q_h x_0 + c_h, Q[i][j] at 4 i + j, c[i] at 4 i + 3.  Q is taken to be a
 *            rotation: its transpose serves as its inverse, and nothing checks that.  A caller whose motion is in the world frame
 *            creates the handle with Rinv = I, t = 0, as for caller rays.
 *   rays:    with (o, d) the ray ls_trace_scene_sweep casts for (v, h), geometry g sees e_i = o_i - c_i, o_g,i = (Q[0][i] e_0 +
 *            Q[1][i] e_1) + Q[2][i] e_2, d_g,i = (Q[0][i] d_0 + Q[1][i] d_1) + Q[2][i] d_2, tmin 0, tmax 1e16, in float32 with no
 *            fused multiply-add: ONE operation sequence (csrc/ls_motion.h; ls_debug_motion_ray in lidarshooter_hip_debug.h runs it
 *            on the host).  An identity record gives the ray back.  A record with a non-finite entry, or one that yields a zero
 *            d_g, makes THAT geometry invisible to THAT column; every other geometry is still tested.
 *   hits:    for every ray, every geometry g of the committed scene contributes what ls_trace_rays would return for the record
 *            (o_g, 0, d_g, 1e16) -- (o, 0, d, 1e16) for a geometry at rest -- against a scene that holds g alone at its committed
 *            pose; the answer is the contribution with the smallest t, the lowest (geomID, primID) among equals.  t is along the
 *            direction as given, as everywhere else.
 *   outputs: those of ls_trace_scene_sweep -- d_points32, d_hits, d_n_points, capacity, the order of the records, NULL outputs --:
 *            by default xyz = t * d with the nominal d and no sum, what the sensor reports; with LS_SWEEP_DESKEW xyz = o_h + t *
 *            d'_h per axis: where the surface was, in the frame-start sensor frame, at the instant it was hit.
 * With n_motions 0 the call returns ls_trace_scene_sweep's bytes, with identity tables for every geometry too; with no motions and
 * no pose table ls_trace_scene's points, records and count.  LS_ERR_INVALID_ARGUMENT before any device call, in this order: a frame
 * graph is open; a NULL count; a pose table whose n_cols is not H, or n_cols != 0 without one; unknown flag bits; motions NULL with
 * n_motions > 0; a NULL table; a non-zero reserved; n_motions above ls_geometry_count() or the same geom twice; misaligned pointers;
 * a capacity below the shard's ls_total_rays().  Then the commit state (-1 with no commit or an empty scene writes nothing, the
 * count included), then LS_ERR_UNKNOWN_GEOMETRY for a geom that is not in the committed scene.  Stream order, the shard handling,
 * LS_INFO_RAY_QUERY_BUILT and the query hierarchies are those of ls_trace_scene_sweep, whose scratch the call uses: a commit after
 * which only poses changed still builds nothing.
 * These records go through ls_hit_attributes_moving / ls_apply_return_model_moving below, which rebuild per record the ray its
 * geometry saw; ls_hit_attributes / ls_apply_return_model know one ray per record and call most of a moving geometry's invalid.
 * Not offered: a d_rays_out; beams; deforming meshes; a call of the ITracer adapter. */
int ls_trace_scene_sweep_moving(ls_tracer *tr, void *hip_stream, const float *d_col_pose, uint32_t n_cols,
                                const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags,
                                void *d_points32, void *d_hits, uint32_t *d_n_points, uint32_t capacity);
/* The same with host memory (pageable) in and out, on the handle's stream: the pose table and the motion tables are copied to the
 * device; returns when the outputs are filled (*n_points records of each). */
int ls_trace_scene_sweep_moving_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols,
                                     const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags,
                                     void *points32, void *hits, uint32_t *n_points, uint32_t capacity);

/* Motion table of a body at a constant twist (host only, no handle, no device): tau_h = t0 + h * dt; Q_h = Rodrigues' formula for
 * the rotation ang_vel * tau_h, c_h = pivot - Q_h pivot + lin_vel * tau_h -- a body turning about `pivot` while it drives on;
 * evaluated in double, rounded once to float32.  With pivot = 0 the bytes of ls_sweep_poses_constant_twist.  col_motion: n_cols
 * records of 12 floats.  LS_ERR_INVALID_ARGUMENT for NULL pointers or non-finite inputs. */
int ls_motion_constant_twist(const float lin_vel[3], const float ang_vel[3], const float pivot[3], double t0, double dt,
                             uint32_t n_cols, float *col_motion);

/* ---- hit attributes and sensor returns for the records of a sweep: ls_hit_attributes and ls_apply_return_model for a frame of
 * ls_trace_scene_sweep_moving (or ls_trace_scene_sweep, or ls_trace_scene), whose every geometry saw a ray of its own.  The caller
 * passes the tables the frame was traced with; per record the call rebuilds the ray the record's geometry saw, runs the exact test
 * with it, and carries the normal back into the sensor frame.  No hierarchy is built or walked, no 32-byte ray record exists, and
 * the points keep their ring.
 *   d_col_pose, n_cols, motions, n_motions, flags: exactly the arguments of ls_trace_scene_sweep_moving (a NULL pose table with
 *            n_cols 0: the sensor at rest; motions in HOST memory, their tables in device memory -- host memory for _host --, H records
 *            indexed by the GLOBAL column whatever the shard; geometries not named are at rest; flags 0 or LS_SWEEP_DESKEW).
 *   d_hits, d_count, n: as ls_hit_attributes; hit.ray is the global ray index v * H + h of the handle's raster.  The calls do not
 *            depend on the shard.
 * Per handled record, ONE float32 operation sequence, composed of the existing ones and one new one:
 *   1. the ray the column cast: with the nominal d from the factor tables, (o, d') = ls_debug_sweep_ray's record for pose[h]; (0, d)
 *      without a pose table;
 *   2. the ray geometry hit.geom saw: (o_g, d_g) = ls_debug_motion_ray's record for table[h] of that geometry, and the record is
 *      invalid when o_g or d_g is not finite or d_g is zero (the walk skipped the geometry there); (o, d') for a geometry at rest;
 *   3. validity as ls_hit_attributes with the caller ray (o_g, d_g): geom, prim and the vertex indices in range, corners through the
 *      frame's transform, the exact test with t bit-equal to hit.t, a quad's first half for which that holds; every index -- the
 *      ray, the geomID, the element, the vertices, the column -- is checked before an address is formed from it;
 *   4. the 48-byte record of ls_hit_attributes, offsets unchanged: cos_inc, u, v, tri, flags as that call gives them for (o_g, d_g);
 *      the normal n_g of a geometry at rest as it is, of a moving one carried forward, n_i = (Q[i][0] n_g,0 + Q[i][1] n_g,1) +
 *      Q[i][2] n_g,2 (csrc/ls_motion.h; ls_debug_motion_normal runs it on the host; an identity record gives n_g back numerically, a
 *      -0 component may come back as +0); px, py, pz = t * d with the nominal d and no sum -- the bits of the frame's points32 --,
 *      with LS_SWEEP_DESKEW under a pose table o_h + t * d'_h per axis -- the deskewed frame's bits --; ray = hit.ray.  An invalid
 *      record: flags 0 and zeros everywhere but `ray`;
 *   5. ls_apply_return_model_moving: steps 2-8 of ls_apply_return_model on the valid records, with len = sqrtf((d'x d'x + d'y d'y) +
 *      d'z d'z) of the ray the COLUMN cast (the sensor ranges along its own ray, not along d_g), the noise keyed by hit.ray and
 *      frame_index, the point t' * d (flags 0) or o_h + t' * d' per axis (LS_SWEEP_DESKEW), ring = hit.ray / H, d_hits_out with t';
 *      the kept records compacted in input order, model, reflectivities and outputs as ls_apply_return_model.
 * With no pose table and no motions the bytes of ls_hit_attributes / ls_apply_return_model with d_rays = NULL; with tables that do not
 * belong to the frame the records of the geometries concerned are invalid.
 * LS_ERR_INVALID_ARGUMENT before any device call, in this order: (the return model: the model and the reflectivities, as
 * ls_apply_return_model;) a frame graph is open; NULL hit records or output with n > 0, a NULL d_n_out; ls_trace_scene_sweep_moving's
 * checks of the pose table, the flags and the motions, in its order; misaligned pointers (records and points 16 bytes; words, tables
 * and reflectivities 4).  Then LS_ERR_OUT_OF_RANGE for an n above the query-record limit, then the commit state as
 * ls_hit_attributes (-1 writes nothing), then LS_ERR_UNKNOWN_GEOMETRY for a motion whose geom is not in the committed scene.  n = 0
 * gives *d_n_out = 0.  Stream order, scratch and the frame graph rule are those of ls_hit_attributes / ls_apply_return_model;
 * LS_INFO_RAY_QUERY_BUILT is left as it is: nothing is built.
 * Not offered: beam echoes through these calls (their t is a reported range); deforming meshes; a call of the ITracer adapter. */
int ls_hit_attributes_moving(ls_tracer *tr, void *hip_stream, const float *d_col_pose, uint32_t n_cols,
                             const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags,
                             const void *d_hits, const uint32_t *d_count, uint32_t n, void *d_out);
/* The same with host memory (pageable) in and out and no count word, on the handle's stream: the pose table and the motion tables
 * are copied to the device; returns when out is filled. */
int ls_hit_attributes_moving_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols,
                                  const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags,
                                  const void *hits, uint32_t n, void *out);
int ls_apply_return_model_moving(ls_tracer *tr, void *hip_stream, const ls_return_model *model, uint32_t frame_index,
                                 const float *d_col_pose, uint32_t n_cols,
                                 const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags,
                                 const void *d_hits, const uint32_t *d_count, uint32_t n,
                                 const float *d_reflectivity, uint32_t n_reflectivity,
                                 void *d_points32, void *d_hits_out, uint32_t *d_n_out);
/* The same with host memory (pageable) in and out and no count word, on the handle's stream; returns when the outputs are filled
 * (*n_out records of each). */
int ls_apply_return_model_moving_host(ls_tracer *tr, const ls_return_model *model, uint32_t frame_index,
                                      const float *col_pose, uint32_t n_cols,
                                      const ls_geometry_motion *motions, uint32_t n_motions, uint32_t flags,
                                      const void *hits, uint32_t n,
                                      const float *reflectivity, uint32_t n_reflectivity,
                                      void *points32, void *hits_out, uint32_t *n_out);

/* ---- surface and Doppler velocity at hit records.  An FMCW LiDAR reports the range rate next to every point, and scene-flow and
 * moving-object labels are made of the surface's velocity.  The frame calls above say where a hit is; this gather says how fast the
 * surface there moves, how fast the sensor's origin moves, and the rate at which the range between the two changes.  The rate is no
 * difference of pose or motion tables (their float32 quantisation divided by a column spacing of tens of microseconds is more than
 * 0.1 m/s of noise at 100 m): the caller supplies the instantaneous twist of every moving body per column, as they supply its
 * displacement per column, and the call evaluates the rigid-body velocity field at the hit point. */
typedef struct ls_geometry_twist {
    uint32_t geom;            /* geomID */
    uint32_t reserved;        /* must be 0 */
    const float *col_twist;   /* H records of 6 floats [w | u]; DEVICE memory for the device call, host memory for _host */
} ls_geometry_twist;

/*   twist tables: a record is a spatial twist [w | u] in the handle's sensor frame as the scene was committed -- the frame the pose
 *            and motion tables use --: a material point of the body that is at x at the instant column h fires moves with v(x) =
 *            u_h + w_h x x.  LS_INFO_AZIMUTH_COUNT records indexed by the GLOBAL column whatever the shard, 4-byte aligned, in device
 *            memory, never read on the host.
 *   d_sensor_twist: NULL (the sensor at rest), or one such table for the sensor body.
 *   twists:  HOST memory, n_twists entries, read during the call, like motions; each names a geometry of the committed scene once;
 *            geometries not named have velocity 0.  Twists and motions are independent of each other: a frame of ls_trace_scene (no
 *            pose table, no motions) with twists gives the Doppler field of a snapshot; a frame of ls_trace_scene_sweep_moving gets
 *            both, and the caller makes both from the same motion (ls_motion_constant_twist and ls_twist_table_constant).
 *   d_col_pose, n_cols, motions, n_motions: exactly the arguments of ls_hit_attributes_moving -- the tables the frame was traced with.
 *   flags:   must be 0; LS_SWEEP_DESKEW has no meaning here and is refused like any other bit.
 *   d_hits, d_count, n: as ls_hit_attributes; hit.ray is the global ray index.  The call does not depend on the shard.
 * Per handled record, ONE float32 operation sequence with no fused multiply-add (csrc/ls_velocity.h; ls_debug_hit_velocity in
 * lidarshooter_hip_debug.h runs it on the host):
 *   1. column h = hit.ray % H and the nominal d; the ray the column cast, (o, c) = ls_debug_sweep_ray's record for pose[h], or (0, d)
 *      without a pose table; the ray the record's geometry saw, as ls_hit_attributes_moving rebuilds it;
 *   2. validity is exactly ls_hit_attributes_moving's for the same tables: the indices in range, a usable ray for the geometry, the
 *      exact test with t bit-equal to hit.t.  The valid bit of record i equals the valid bit that call gives record i, always; every
 *      index -- the ray, the geomID, the element, the vertices, the column -- is checked before an address is formed from it;
 *   3. the hit point at its own instant, in the frame-start frame: P_i = o_i + t * c_i, one product and one sum (without a pose table o
 *      is +0: t * d_i numerically);
 *   4. the surface velocity, with (w, u) = twist[hit.geom][h]: v_s,0 = u_0 + (w_1 P_2 - w_2 P_1), v_s,1 = u_1 + (w_2 P_0 - w_0 P_2),
 *      v_s,2 = u_2 + (w_0 P_1 - w_1 P_0), every product, difference and sum rounded once; without a twist for the geometry (+0, +0, +0);
 *   5. the velocity of the sensor's origin v_o: the same sequence with the sensor's record h at o; without a sensor twist (+0, +0, +0);
 *   6. rel_i = v_s,i - v_o,i; len = sqrtf((c_0 c_0 + c_1 c_1) + c_2 c_2), the return model's len; radial = ((rel_0 c_0 + rel_1 c_1) +
 *      rel_2 c_2) / len.  Positive: the range grows.  The range rate of a material point is (v_p - v_o) . c^: a sensor that TURNS
 *      about its own origin contributes nothing to it -- the sensor's w enters only through v_o, which it leaves alone at o = 0 --,
 *      so do not expect the sensor's ang_vel to show up in `radial`.
 *   d_out:   NULL, or one 32-byte record per handled hit, 16-byte aligned, in input order: v_s xyz f32@0, radial f32@12, v_o xyz
 *            f32@16, flags u32@28 (bit 0 valid, the others 0).  An invalid record: zeros and flags 0.
 *   d_radial: NULL, or n floats, 4-byte aligned: the radial of a valid record, 0x7FC00000 for an invalid one -- the dense field a
 *            publisher puts next to the cloud.
 *   At least one of the two must be given when n > 0; nothing is written past min(n, *d_count) records.  A non-finite twist entry
 *   gives non-finite values in a record that stays valid: the sequence is what it is.
 * LS_ERR_INVALID_ARGUMENT before any device call, in this order: a frame graph is open; NULL hit records with n > 0, or both outputs
 * NULL with n > 0; ls_trace_scene_sweep_moving's checks of the pose table, the flags (none is known here) and the motions, in its
 * order; twists NULL with n_twists > 0; a NULL twist table; a non-zero reserved; n_twists above ls_geometry_count() or the same geom
 * twice; misaligned pointers for the device call (records 16 bytes; words, tables and d_radial 4).  Then LS_ERR_OUT_OF_RANGE for an n
 * above the query-record limit, then the commit state as ls_hit_attributes (-1 writes nothing), then LS_ERR_UNKNOWN_GEOMETRY for a
 * motion or a twist whose geom is not in the committed scene.  Stream order, scratch and the frame graph rule are those of
 * ls_hit_attributes_moving; LS_INFO_RAY_QUERY_BUILT is left as it is: nothing is built.
 * Not offered: beam echoes (their t is a reported range: the records are invalid, as for the attributes); deforming meshes; vectors
 * in the instantaneous sensor frame; a velocity source for ls_format_cloud; a call of the ITracer adapter. */
int ls_hit_velocities(ls_tracer *tr, void *hip_stream,
                      const float *d_col_pose, uint32_t n_cols,
                      const ls_geometry_motion *motions, uint32_t n_motions,
                      const float *d_sensor_twist,
                      const ls_geometry_twist *twists, uint32_t n_twists, uint32_t flags,
                      const void *d_hits, const uint32_t *d_count, uint32_t n,
                      void *d_out, float *d_radial);
/* The same with host memory (pageable, any alignment) in and out and no count word, on the handle's stream: the tables are copied to
 * the device; returns when the outputs are filled. */
int ls_hit_velocities_host(ls_tracer *tr, const float *col_pose, uint32_t n_cols,
                           const ls_geometry_motion *motions, uint32_t n_motions,
                           const float *sensor_twist,
                           const ls_geometry_twist *twists, uint32_t n_twists, uint32_t flags,
                           const void *hits, uint32_t n, void *out, float *radial);
/* Twist table of a body at a constant twist (host only, no handle, no device): tau_h = t0 + h * dt; w_h = ang_vel, u_h = lin_vel -
 * ang_vel x (pivot + lin_vel * tau_h), evaluated in double and rounded once -- the twist of the body whose displacement table
 * ls_motion_constant_twist writes for the same arguments; with pivot = 0 the twist of the sensor of ls_sweep_poses_constant_twist.
 * With ang_vel = 0 every record is (0, 0, 0, lin_vel) bit for bit.  col_twist: n_cols records of 6 floats.
 * LS_ERR_INVALID_ARGUMENT for NULL pointers or non-finite inputs. */
int ls_twist_table_constant(const float lin_vel[3], const float ang_vel[3], const float pivot[3],
                            double t0, double dt, uint32_t n_cols, float *col_twist);

/* ---- object labels: what detection and tracking ground truth asks per GEOMETRY of a frame -- how many points it got, where they
 * are (a box in the sensor frame), how near it is, and how much of it other geometries hide (KITTI's occlusion level) -- from hit
 * records that are already in device memory, without reading the cloud back.  The first three are a reduction over the records; the
 * last needs the rays that would hit the geometry if it stood alone, which no other call answers: a walk over the query hierarchies
 * of ls_trace_rays, one geometry after the other, that does not stop at a ray's first hit.
 *   d_labels: n_labels ls_object_label records indexed by geomID (the convention of d_reflectivity), 16-byte aligned; every one of
 *            them is written.  A geomID below n_labels that names no geometry of the committed scene gets the empty record with
 *            flags = 0; a committed geometry whose id is >= n_labels is counted nowhere, neither in hits nor in the footprint.
 *   d_rays, n_rays, d_hits, d_count, n: exactly as ls_hit_attributes takes them.  d_rays = NULL: the handle's own sensor rays,
 *            hit.ray the global ray index, the bound V * H, n_rays ignored.  d_count NULL or a device word: min(n, *d_count)
 *            records are handled.  n = 0 with d_hits = NULL is allowed: the footprint alone.
 *   flags:   0 or LS_LABEL_FOOTPRINT; any other bit is refused.
 * A record COUNTS when hit.geom < n_labels and names a geometry of the committed scene, hit.prim < its element count, hit.ray < the
 * ray bound, hit.t is finite and >= 0 (a -0 counts as +0) and, with caller rays, the ray is one ls_trace_rays walks: finite origin
 * and direction, a non-zero direction, tmin <= tmax.  The triangle is NOT tested again: this is a reduction, not the validity gather
 * of ls_hit_attributes -- a stale t of a geometry moved since counts where it says.  Every index is checked before an address is
 * formed from it.  A record's point is ls_hit_attributes' px, py, pz: o + t d per axis (one product, one sum) for a caller ray, t d
 * with no sum for a sensor ray -- the bits of the frame's points32.
 * Every value is an integer count, a minimum or a maximum (of floats, -0 below +0; of (t, ray) pairs): none depends on the order of
 * the records or of the device's work, so the records are the same bytes from call to call and for shuffled input.
 * LS_LABEL_FOOTPRINT: over the n_rays caller rays -- or, with d_rays = NULL, over all V * H rays of the handle's full raster whatever
 * the shard, generated into a scratch buffer of the handle as ls_generate_rays_aos generates them, with tmin = 0 and tmax = +inf --
 * ray r adds one to n_alone[g] for every committed geometry g with id < n_labels on which the exact test of ls_occluded_rays passes
 * for some triangle with tmin <= t <= tmax.  A ray through three geometries counts in all three; a degenerate ray, as ls_trace_rays
 * defines it, counts nowhere.  When the records are the closest hits of those same rays, n_hits[g] <= n_alone[g], and the visible
 * fraction of g is n_hits / n_alone.  The flag uses the query hierarchies ls_trace_rays and its siblings share and builds what they
 * lack: LS_INFO_RAY_QUERY_BUILT reports for it.  Without the flag no hierarchy is touched and that word is left as it is.
 * LS_ERR_INVALID_ARGUMENT before any device call, in this order: a frame graph is open; NULL d_labels with n_labels > 0; NULL hits
 * with n > 0; unknown flag bits; misaligned pointers for the device call (rays, records and labels 16 bytes, the count 4).  Then
 * LS_ERR_OUT_OF_RANGE for n or n_rays above the query-record limit or n_labels above 65536, then the commit state as
 * ls_hit_attributes (-1 with no commit or an empty scene: nothing is written).  Stream order and the frame graph rule are those of
 * ls_trace_rays.  Calls on one handle use scratch buffers of the handle (64 bytes per label; 32 bytes per ray of the raster for the
 * footprint of the sensor's own rays) and are ordered through its stream: one at a time.
 * Not offered: labels for sweep, moving or beam frames (their points are not o + t d of one ray); centroids (float sums depend on
 * the order). */
#define LS_LABEL_FOOTPRINT 1u   /* also count, per geometry, the rays that hit it taken alone (n_alone) */

typedef struct ls_object_label {   /* 64 bytes, no pointers */
    uint32_t n_hits;     /* records that name this geometry and count (above) */
    uint32_t n_alone;    /* LS_LABEL_FOOTPRINT: rays that pass the exact test on some triangle of THIS geometry within [tmin, tmax],
                            whatever else is in the scene; 0 without the flag */
    float    t_min;      /* smallest t of the counted records; +inf when n_hits = 0 */
    uint32_t ray_min;    /* the lowest hit.ray among the records with that t; 0xFFFFFFFF when n_hits = 0 */
    float    t_max;      /* largest t; -inf when n_hits = 0 */
    uint32_t ray_max;    /* the lowest hit.ray among the records with that t; 0xFFFFFFFF when n_hits = 0 */
    float    lo[3];      /* per-axis minimum of the counted records' points; +inf when n_hits = 0 */
    float    hi[3];      /* per-axis maximum; -inf when n_hits = 0 */
    uint32_t flags;      /* bit 0: this geomID names a geometry of the committed scene */
    uint32_t reserved[3];/* 0 */
} ls_object_label;

int ls_object_labels(ls_tracer *tr, void *hip_stream, uint32_t flags,
                     const void *d_rays, uint32_t n_rays,
                     const void *d_hits, const uint32_t *d_count, uint32_t n,
                     void *d_labels, uint32_t n_labels);
/* The same with host memory (pageable, any alignment) in and out and no count word, on the handle's stream; returns when labels is
 * filled. */
int ls_object_labels_host(ls_tracer *tr, uint32_t flags, const void *rays, uint32_t n_rays,
                          const void *hits, uint32_t n, void *labels, uint32_t n_labels);

/* ---- occupancy grid: what mapping and occupancy-prediction ground truth asks per CELL of a voxel grid -- did a return fall in it,
 * did a ray cross it before its return or before it ran out of range (observed free space), or did no ray touch it (unknown) -- from
 * hit records that are already in device memory.  Every call above describes what the rays hit; this one describes what they passed
 * through: each ray is walked through the grid, cell by cell, up to its return.
 *   grid:     the descriptor below, a host pointer, copied during the call.
 *   sensor_to_grid3x4: a host pointer to 12 floats (row-major 3 x 4, copied during the call), or NULL.  NULL applies no arithmetic
 *             at all to the ray: the grid is given in the sensor frame, and for the handle's own rays the occupied cell is the cell
 *             of the frame's points32 xyz, bit for bit.  Non-NULL: origin and direction go through the affine in the order
 *             ls_cloud_to_world applies its affine to a point -- o'_i = ((m[i][0] o_0 + m[i][1] o_1) + m[i][2] o_2) + m[i][3], the
 *             direction the same without the translation --; t is unchanged: the matrix is taken as rigid, only finiteness is checked.
 *   d_rays, n_rays, d_hits, d_count, n: exactly as ls_object_labels takes them.  d_rays = NULL: the handle's own sensor rays, the full
 *             V x H raster whatever the shard, hit.ray the global ray index, tmin = 0 and tmax = +inf.  n = 0 with d_hits = NULL is
 *             allowed: every ray is a miss.
 *   d_counts: nx ny nz records of two uint32_t {n_free, n_occ}, 16-byte aligned; every one of them is written.
 *   d_geom:   NULL, or nx ny nz uint32_t: the lowest geomID among the counted records whose point fell in the cell, 0xFFFFFFFF
 *             where there is none.
 * A record COUNTS by ls_object_labels' rule: hit.geom names a committed geometry, hit.prim < its element count, hit.ray < the ray
 * bound, t is finite and >= 0 (a -0 counts as +0) and the ray is walkable (finite origin and direction, a non-zero direction, tmin <=
 * tmax).  Every index is checked before an address is formed from it.  Where several counted records name one ray, the one with the
 * smallest t decides, then the lowest geomID (a 64-bit minimum per ray in a scratch buffer of the handle, 8 bytes per ray).
 * Per ray, with t_start = max(tmin, min_range) and t_far = min(tmax, max_range):
 *   no deciding record, without LS_OCC_CARVE_MISSES, or a ray that is not walkable:   nothing;
 *   no deciding record, with the flag:        free cells on [t_start, t_far];
 *   t < min_range:                            nothing (blocked in the blind zone);
 *   min_range <= t <= max_range:              free cells on [t_start, t], and the cell of p = o + t d is occupied if p is inside;
 *   t > max_range:                            free cells on [t_start, t_far], with or without the flag.
 * p is one product and one sum per axis (t d with no sum for an own ray without a transform); its cell is floorf((p - origin) /
 * cell) per axis, compared as floats against [0, n) before any cast, and does not depend on the walk.  The occupied cell gets n_occ
 * += 1 and geom = min(geom, hit.geom).  The walk adds n_free += 1 to every cell it visits except this ray's own occupied cell; it
 * visits a cell at most once, so n_free counts rays.  A cell with n_free = n_occ = 0 is unknown.
 * The walk (csrc/ls_voxel.h, float32, every operation rounded once, no reciprocal and no accumulated boundary): the span is clipped
 * against the grid's box per axis by two divisions; the first cell is floorf of the entry point, clamped into the grid; from cell
 * c the ray leaves along axis a at ((c_a + (d_a > 0)) cell - q_a) / d_a, q = o - origin; the smallest of the three decides, ties
 * going to x, then y, then z; the walk ends when that parameter is beyond the span or the next cell is outside, after at most nx +
 * ny + nz cells.  ls_debug_voxel_walk runs the same sequence on the host for one ray.
 * Every value is an integer count or a minimum: the grid is the same bytes whatever the order of the records and of the device's
 * work, from call to call.
 * LS_ERR_INVALID_ARGUMENT before any device call, in this order: a frame graph is open; NULL grid; NULL d_counts; NULL hits with n >
 * 0; unknown flag bits or non-zero reserved; a non-finite origin or transform; cell not finite or not > 0; min_range not finite or
 * < 0; max_range not finite or < min_range; misaligned pointers for the device call (rays, records and counts 16 bytes; geom and the
 * count word 4).  Then LS_ERR_OUT_OF_RANGE for a dimension of 0 or above 2048, nx ny nz above 2^27, a non-finite origin + n cell, n
 * or n_rays above the query-record limit; then the commit state as ls_object_labels (-1 with no commit or an empty scene: nothing
 * is written).  ls_occupancy_grid_check returns the descriptor's part of this (host only, no device call).  Stream order, the
 * one-call-at-a-time rule and the frame graph rule are those of ls_trace_rays.
 * Not offered: grids of sweep, moving or beam frames (their points are not o + t d of one ray); a majority label per cell; log-odds
 * (float sums depend on the order); non-cubic cells; a call of the ITracer adapter. */
#define LS_OCC_CARVE_MISSES 1u   /* a ray with no counted record carves free space up to min(tmax, max_range) */
#define LS_OCC_ACCUMULATE   2u   /* add to what d_counts / d_geom hold instead of clearing them first */

typedef struct ls_occupancy_grid_desc {   /* 48 bytes, no pointers */
    float    origin[3];   /* minimum corner of cell (0,0,0), in the grid's frame */
    float    cell;        /* edge of a cubic cell */
    uint32_t dims[3];     /* nx, ny, nz; cell (x,y,z) is word pair (z*ny + y)*nx + x */
    uint32_t flags;
    float    min_range;   /* the walk starts at max(tmin, min_range): the sensor's blind zone */
    float    max_range;   /* range gate, finite */
    uint32_t reserved[2]; /* 0 */
} ls_occupancy_grid_desc;

int ls_occupancy_grid(ls_tracer *tr, void *hip_stream, const ls_occupancy_grid_desc *grid, const float *sensor_to_grid3x4,
                      const void *d_rays, uint32_t n_rays, const void *d_hits, const uint32_t *d_count, uint32_t n,
                      void *d_counts, void *d_geom);
/* The same with host memory (pageable, any alignment) in and out and no count word, on the handle's stream; returns when counts and
 * geom are filled.  With LS_OCC_ACCUMULATE the two arrays travel to the device first. */
int ls_occupancy_grid_host(ls_tracer *tr, const ls_occupancy_grid_desc *grid, const float *sensor_to_grid3x4,
                           const void *rays, uint32_t n_rays, const void *hits, uint32_t n, void *counts, void *geom);
int ls_occupancy_grid_check(const ls_occupancy_grid_desc *grid);   /* host only, no device call: LS_OK or the refusal */

/* ---- scene grid: the COMPLETE grid next to the observed one.  ls_occupancy_grid says what a frame saw of each cell; scene
 * completion and occupancy prediction ground truth (SemanticKITTI SSC, Occ3D, nvblox / OctoMap evaluation) also asks, whatever the
 * sensor happened to see, whether any surface of the scene lies in the cell and whose it is.  The two grids share the cell order,
 * so they overlay: observed and occupied, observed and free, occupied but never observed (the completion target), unknown.
 *   grid:     the descriptor below, a host pointer, copied during the call.
 *   sensor_to_grid3x4: exactly as ls_occupancy_grid takes it.  NULL: the grid is in the sensor frame and a vertex is what the frame's
 *             triangle test sees, bit for bit.  Non-NULL: that vertex goes through ((m0 x + m1 y) + m2 z) + m3 per row.
 *   d_select: NULL, or n_select bytes in device memory indexed by geomID: a geometry whose byte is 0 is left out; geom >= n_select
 *             (or NULL) means selected.  Static scenery and moving bodies can so go into separate grids.
 *   d_counts: nx ny nz uint32_t, 16-byte aligned: the number of triangles of the committed scene that overlap the cell; every word
 *             is written.
 *   d_geom:   NULL, or nx ny nz uint32_t: the lowest geomID among those triangles, 0xFFFFFFFF where there is none.
 * The scene is what ls_hit_attributes would see: the committed layout with the geometries' current buffers and poses.  A quad is its
 * two triangles 2q, 2q + 1, and each counts on its own.  Only the surface counts: the interior of a closed mesh is not filled.
 * Per selected triangle (csrc/ls_scene_grid.h: float32, every operation rounded once):
 *   1. the three vertex indices are checked against the vertex count before an address is formed from them; a triangle that fails
 *      is skipped;
 *   2. q_k = v_k - origin per axis, v_k the transformed vertex; a triangle with a non-finite q is skipped;
 *   3. per axis a: lo_a = floorf(min_k q_k[a] / cell), hi_a = floorf(max_k q_k[a] / cell), compared as floats before any cast; the
 *      triangle is skipped if hi_a < 0 or lo_a >= n_a; otherwise both are clamped to [0, n_a - 1];
 *   4. for every cell c of the range: ctr_a = ((float)c_a + 0.5f) * cell, h = 0.5f * cell, p_k = q_k - ctr; the edges are
 *      e0 = q1 - q0, e1 = q2 - q1, e2 = q0 - q2 (from q, not from p);
 *   5. the cell overlaps unless one of 13 axes separates: the 3 box axes (min_k p_k[a] > h or max_k p_k[a] < -h); the 9 axes
 *      unit_i x e_j -- for i = x the projection of vertex k is (e_y * p_k.z) - (e_z * p_k.y) and r = h * (|e_z| + |e_y|), for i = y
 *      (e_z * p_k.x) - (e_x * p_k.z) and r = h * (|e_x| + |e_z|), for i = z (e_x * p_k.y) - (e_y * p_k.x) and r = h * (|e_y| + |e_x|);
 *      all three vertices are projected; the axis separates if min > r or max < -r --; and the plane axis, n = cross(e0, e1) as
 *      products and differences, d = ((n.x * p_0.x) + (n.y * p_0.y)) + (n.z * p_0.z), r = h * ((|n.x| + |n.y|) + |n.z|), which
 *      separates if d > r or d < -r;
 *   6. the comparisons are written so that a NaN never separates; a cell index is in range by construction;
 *   7. an overlapping cell gets counts += 1 and, with d_geom, geom = min(geom, geomID).
 * A cell's box is closed, but the range is floorf's: a triangle that ends on a face plane reaches the cell above that plane and
 * touches it; one that begins on the plane does not reach the cell below.  A segment or a point needs no special case.
 * ls_debug_scene_grid_triangle runs the same sequence on the host for one triangle.  Every value is an integer count or a minimum:
 * the grid is the same bytes whatever the order of the device's work, from call to call.
 * LS_ERR_INVALID_ARGUMENT before any device call, in this order: a frame graph is open; NULL grid; NULL d_counts; n_select > 0 with
 * NULL d_select; unknown flag bits; a non-finite origin or transform; cell not finite or not > 0; misaligned pointers for the
 * device call (counts 16 bytes, geom 4).  Then LS_ERR_OUT_OF_RANGE for a dimension of 0 or above 2048, nx ny nz above 2^27 or a
 * non-finite origin + n cell; then the commit state as ls_occupancy_grid (-1 with no commit or an empty scene: nothing is written).
 * ls_scene_grid_check returns the descriptor's part of this (host only, no device call).  No hierarchy is touched; stream order,
 * the one-call-at-a-time rule and the frame graph rule are those of ls_trace_rays.
 * Not offered: solid (interior) fill; meshes that deform during the call; a majority label per cell; a call of the ITracer adapter. */
#define LS_SCENE_GRID_ACCUMULATE 1u   /* add to what d_counts / d_geom hold instead of clearing them first */

typedef struct ls_scene_grid_desc {   /* 32 bytes, no pointers */
    float    origin[3];   /* minimum corner of cell (0,0,0), in the grid's frame */
    float    cell;        /* edge of a cubic cell */
    uint32_t dims[3];     /* nx, ny, nz; cell (x,y,z) is word (z*ny + y)*nx + x -- ls_occupancy_grid's order, so the two grids overlay */
    uint32_t flags;
} ls_scene_grid_desc;

int ls_scene_grid(ls_tracer *tr, void *hip_stream, const ls_scene_grid_desc *grid, const float *sensor_to_grid3x4,
                  const uint8_t *d_select, uint32_t n_select, void *d_counts, void *d_geom);
/* The same with host memory (pageable, any alignment) in and out, on the handle's stream; returns when counts and geom are filled.
 * With LS_SCENE_GRID_ACCUMULATE the two arrays travel to the device first. */
int ls_scene_grid_host(ls_tracer *tr, const ls_scene_grid_desc *grid, const float *sensor_to_grid3x4,
                       const uint8_t *select, uint32_t n_select, void *counts, void *geom);
int ls_scene_grid_check(const ls_scene_grid_desc *grid);   /* host only, no device call: LS_OK or the refusal */

/* ---- scene distance grid: the third grid of the family, over the same cells.  The consumers of ls_scene_grid (nvblox / voxblox TSDF
 * and ESDF evaluation, implicit-surface and occupancy networks trained on truncated distance targets, clearance maps for planning)
 * also ask how far each cell's CENTRE is from the nearest surface of the scene, up to a truncation distance.  Every triangle visits
 * only the cells within that distance of it (a scatter: no hierarchy is built or walked), and the result is a minimum, the same bytes
 * in any order.
 *   grid:     the descriptor below, a host pointer, copied during the call.
 *   sensor_to_grid3x4, d_select / n_select, the scene that is seen and the quad rule: word for word ls_scene_grid's -- the committed
 *             layout with the geometries' current buffers and poses; a quad is its triangles 2q and 2q + 1.
 *   d_cells:  nx ny nz records of 8 bytes, 16-byte aligned: geom u32 @0, dist f32 @4; read as one little-endian 64-bit word a record
 *             is (bits(dist) << 32) | geom.  A cell with no surface within trunc of its centre holds {0xFFFFFFFF, +inf} =
 *             0x7F800000FFFFFFFF.  Every record is written.
 * Per selected triangle (csrc/ls_distance_grid.h: float32, every operation rounded once, no fmaf), v_k its vertices in the grid's
 * frame exactly as ls_scene_grid obtains them (indices checked before an address is formed, the frame's transform, the call's):
 *   1. q_k = v_k - origin per axis; a triangle with a non-finite q is skipped;
 *   2. per axis a: lo_a = floorf((min_k q_k[a] - trunc) / cell), hi_a = floorf((max_k q_k[a] + trunc) / cell), compared as floats
 *      before any cast; the triangle is skipped if hi_a < 0 or lo_a >= n_a; otherwise both are clamped to [0, n_a - 1].  In exact
 *      arithmetic the first cell left out on either side has its centre at least half a cell beyond trunc from the triangle's box,
 *      so the range is part of the definition without changing the answer for any sane input (|q| / cell < 2^20);
 *   3. per cell c of the range: ctr_a = ((float)c_a + 0.5f) * cell; closest_on_triangle(ctr, q_0, q_1, q_2) of csrc/ls_closest.h
 *      (ls_closest_points' sequence) gives d2; the pair counts iff d2 is finite and dist = sqrtf(d2) <= trunc.  A triangle without
 *      area never counts (closest_on_triangle gives it d2 = +inf) -- unlike ls_scene_grid, where a segment marks cells;
 *   4. a counting pair sends (bits(dist) << 32) | geomID to its cell, whose word becomes the 64-bit unsigned minimum: the smallest
 *      rounded distance, and the lowest geomID among the triangles that attain it.  sqrtf is correctly rounded and monotone, so this
 *      is the sqrtf of the smallest d2.  Every value is a minimum: the same bytes whatever the order of the device's work;
 *   5. with LS_DIST_GRID_ACCUMULATE the words d_cells holds are the starting values, compared as 64-bit words whatever their bits:
 *      the minimum over several poses, or over static scenery and moving bodies selected into one grid.
 * ls_debug_distance_grid_triangle runs steps 1 to 3 on the host for one triangle.
 * LS_ERR_INVALID_ARGUMENT before any device call, in this order: a frame graph is open; NULL grid; NULL d_cells; n_select > 0 with NULL
 * d_select; unknown flag bits or a non-zero reserved word; a non-finite origin or transform; cell not finite or not > 0; trunc not
 * finite or < 0; a misaligned d_cells (16 bytes; the device call only).  Then LS_ERR_OUT_OF_RANGE for a dimension of 0 or above 2048,
 * nx ny nz above 2^27, a non-finite origin + n cell, or trunc > 32.0f * cell (the float32 product): the band bounds the work per
 * triangle.  Then the commit state as ls_scene_grid (-1 with no commit or an empty scene: nothing is written).
 * ls_scene_distance_grid_check returns the descriptor's part of this (host only, no device call).  No hierarchy is touched and
 * LS_INFO_RAY_QUERY_BUILT is left as it is; stream order, the one-call-at-a-time rule and the frame graph rule are those of
 * ls_trace_rays.
 * Not offered: a sign (the scene's meshes need not be closed, and a face-normal sign is wrong at edges); the nearest primitive or
 * point (ls_closest_points gives them per point); distances beyond trunc; non-cubic cells; meshes that deform during the call; a call
 * of the ITracer adapter. */
#define LS_DIST_GRID_ACCUMULATE 1u   /* take the minimum with what d_cells holds instead of clearing it first */

typedef struct ls_distance_grid_desc {   /* 48 bytes, no pointers */
    float    origin[3];   /* minimum corner of cell (0,0,0), in the grid's frame */
    float    cell;        /* edge of a cubic cell */
    uint32_t dims[3];     /* nx, ny, nz; cell (x,y,z) is record (z*ny + y)*nx + x: the order of the other two grids */
    uint32_t flags;
    float    trunc;       /* truncation distance, finite, >= 0 */
    uint32_t reserved[3]; /* 0 */
} ls_distance_grid_desc;

int ls_scene_distance_grid(ls_tracer *tr, void *hip_stream, const ls_distance_grid_desc *grid, const float *sensor_to_grid3x4,
                           const uint8_t *d_select, uint32_t n_select, void *d_cells);
/* The same with host memory (pageable, any alignment) in and out, on the handle's stream; returns when cells is filled.  With
 * LS_DIST_GRID_ACCUMULATE the array travels to the device first. */
int ls_scene_distance_grid_host(ls_tracer *tr, const ls_distance_grid_desc *grid, const float *sensor_to_grid3x4,
                                const uint8_t *select, uint32_t n_select, void *cells);
int ls_scene_distance_grid_check(const ls_distance_grid_desc *grid);   /* host only, no device call */

/* ---- surface samples: the POINT form of the scene's ground truth, next to the three grids.  Points spread uniformly, by area, over
 * the whole surface of the selected geometries, whatever the sensor saw: the complete cloud beside a frame's partial one (PCN / KITTI
 * completion pairs, point-based scene completion), oriented on-surface samples (point, unit normal, owner) for implicit-surface
 * training beside ls_scene_distance_grid's band, the mesh side of Chamfer distance and F-score (ls_closest_points gives cloud -> mesh;
 * mesh -> cloud needs points drawn from the mesh), and the surface area of a selection, from which a sample density is chosen.  The
 * vertices are the frame's, bit for bit, and the same call gives the same bytes on every run.
 *   desc:     the descriptor below, a host pointer, copied during the call.
 *   sensor_to_out3x4, d_select / n_select, the scene that is seen and the quad rule: word for word ls_scene_grid's -- NULL: the output
 *             frame is the sensor frame and a vertex is what the frame's triangle test sees; non-NULL: that vertex goes through
 *             ((m0 x + m1 y) + m2 z) + m3 per row; a geometry whose select byte is 0 is left out, geom >= n_select (or NULL) means
 *             selected; the committed layout with the geometries' current buffers and poses; a quad is its triangles 2q and 2q + 1 of
 *             the geometry's triangle list.  The three vertex indices of a triangle are checked against the vertex count before an
 *             address is formed from them.
 *   d_samples: n_samples records of 48 bytes, 16-byte aligned; may be NULL only when n_samples == 0.  Every record is written:
 *             px, py, pz  f32 @0   the point, in the output frame
 *             geom        u32 @12  geomID; 0xFFFFFFFF in an invalid record
 *             nx, ny, nz  f32 @16  unit normal along (v1 - v0) x (v2 - v0)
 *             prim        u32 @28  as ls_hit.prim (a quad's index for a quad geometry)
 *             u, v        f32 @32  point = (1 - u - v) v0 + u v1 + v v2
 *             tri         u32 @40  triangle inside the geometry, as ls_hit_attributes' tri
 *             flags       u32 @44  bit 0 = valid
 *   d_info:   NULL, or 16 bytes, 8-byte aligned: weight_total u64 @0 (W below), exponent i32 @8 (e below), n_weighted u32 @12 (the
 *             triangles with weight > 0).  The selection's area is weight_total * 2^exponent, up to the weights' flooring (less than
 *             n_weighted * 2^exponent below the sum of the float32 areas).  n_samples == 0 with d_info asks for a selection's area.
 * The definition (csrc/ls_surface_sample.h: float32, every operation rounded once, no fmaf; the integers exact).  Per triangle i of
 * the flat index -- the geometries in ascending geomID, each one's triangles in order --, q_k its vertices in the output frame:
 *   1. weight 0 for an unselected geometry, a free id, an index >= the vertex count, a non-finite coordinate;
 *   2. N = (q1 - q0) x (q2 - q0) as products and differences (ls_scene_grid's form: the normal is NOT bit-equal to ls_hit_attributes',
 *      which fuses); m = max |N_k|, weight 0 unless m > 0 and finite; g = N / m; len = sqrtf((gx gx + gy gy) + gz gz); n = g / len;
 *      the area a = (0.5f * m) * len, weight 0 unless a is finite;
 *   3. A = max_i a_i (a maximum of bit patterns: it has no order).  A == 0: W = 0, e = 0.  Otherwise A = f 2^E with f in [1, 2)
 *      (subnormals included) and e = E - 30;
 *   4. w_i = (uint64)floorf(ldexpf(a_i, -e)): the largest weight lies in [2^30, 2^31), and a triangle 2^30 times smaller than the
 *      largest has weight 0 and is never drawn;
 *   5. P[0] = 0, P[i + 1] = P[i] + w_i, W = P[n_tris] (< 2^63): integer sums, the same bytes in any order;
 *   6. sample j: Philox4x32-10 with key (seed, 1) and counter (lo32(j), hi32(j), 0, 0) gives x0 .. x3.  Only j keys the sample: a call
 *      for a slice [first_sample, first_sample + n_samples) draws what the full call draws there;
 *   7. r = (x0 << 32) | x1, T = hi64(r W); the triangle is the largest i < n_tris with P[i] <= T: one of weight > 0;
 *   8. alpha = x2 >> 8, beta = x3 >> 8; if alpha + beta > 2^24 (integers): alpha = 2^24 - alpha, beta = 2^24 - beta; gamma = 2^24 -
 *      alpha - beta; u = (float)alpha 2^-24, v = (float)beta 2^-24, w = (float)gamma 2^-24, all exact;
 *   9. p = ((w q0 + u q1) + v q2) per axis; the record gets p, n, the ids, u, v and flags 1;
 *  10. W == 0 (nothing selected, or nothing with an area): every record is zeros with geom = 0xFFFFFFFF and flags 0; LS_OK.
 * ls_debug_surface_weights, ls_debug_surface_pick and ls_debug_surface_point run steps 2 to 5, 7 and 8 to 9 on the host.
 * LS_ERR_INVALID_ARGUMENT before any device call, nothing written, in this order: a frame graph is open; NULL desc; NULL d_samples
 * with n_samples > 0; n_select > 0 with NULL d_select; unknown flag bits or a non-zero reserved word; a non-finite transform;
 * misaligned pointers for the device call (samples 16 bytes, info 8).  Then the commit state as ls_scene_grid (-1 with no commit or
 * an empty scene: nothing is written).  LS_ERR_OUT_OF_RANGE for a scene of more than 2^32 - 256 triangles.
 * ls_surface_sample_check returns the descriptor's part of this (host only, no device call).  No hierarchy is touched and
 * LS_INFO_RAY_QUERY_BUILT is left as it is; stream order, the one-call-at-a-time rule and the frame graph rule are those of
 * ls_trace_rays.  The call keeps 12 bytes per triangle of the scene on the handle (released with the query state), and every call
 * makes the weights anew: 2^20 samples in slices of 2^10 pay for them 2^10 times.
 * Not offered: sampling restricted to a box or to the visible surface; per-vertex attribute interpolation (the record carries u, v
 * and tri for it); an offset along the normal (the caller has n); stratified or blue-noise sets; meshes that deform during the call;
 * a call of the ITracer adapter. */
#define LS_SURFACE_SAMPLE_FLAGS 0u        /* no flag yet: any bit set is refused */

typedef struct ls_surface_sample_desc {   /* 32 bytes, no pointers */
    uint64_t first_sample;   /* index j of the first sample of this call */
    uint32_t n_samples;      /* samples j = first_sample .. first_sample + n_samples - 1 (mod 2^64); 0 is allowed */
    uint32_t seed;
    uint32_t flags;
    uint32_t reserved[3];    /* 0 */
} ls_surface_sample_desc;

int ls_sample_surface(ls_tracer *tr, void *hip_stream, const ls_surface_sample_desc *desc, const float *sensor_to_out3x4,
                      const uint8_t *d_select, uint32_t n_select, void *d_samples, void *d_info);
/* The same with host memory (pageable, any alignment) in and out, on the handle's stream; returns when samples and info are filled. */
int ls_sample_surface_host(ls_tracer *tr, const ls_surface_sample_desc *desc, const float *sensor_to_out3x4,
                           const uint8_t *select, uint32_t n_select, void *samples, void *info);
int ls_surface_sample_check(const ls_surface_sample_desc *desc);   /* host only, no device call */

/* ---- the nearest cloud point to each query, within a radius.  Every query above takes the mesh as its target: ls_closest_points gives
 * cloud -> mesh, ls_sample_surface draws the points for mesh -> cloud, and this call answers them: which point of a cloud is nearest to
 * a point, and how far.  It is the other half of a Chamfer distance or an F-score at a threshold (the completeness term: surface
 * sample -> cloud), of ICP correspondences with a maximum correspondence distance, of associating one frame's returns with the next
 * frame's, and of spacing and outlier statistics inside one cloud -- on clouds and samples that already sit in device memory in the
 * library's own record layouts.
 *   desc:      radius: the search radius, finite, 2^-20 <= radius <= 2^20.  cloud_stride / query_stride: bytes from one point to the
 *              next, a multiple of 4 in 12 .. 128, with x, y, z as float32 at bytes 0, 4, 8 of every record (only these 12 bytes of a
 *              record are read) -- so that the 32-byte points of a frame, the 48-byte records of ls_sample_surface, the 32-byte records
 *              of ls_closest_points (their point leads the record; any other record with the pointer advanced to its point), and packed
 *              12- or 16-byte xyz go in as they are.
 *              flags: LS_CLOUD_NEAREST_SKIP_SAME_INDEX -- cloud point i is no candidate for query i: a cloud against itself.
 *   query_to_cloud3x4: NULL, or a row-major 3 x 4 transform applied to every query first.
 *   d_cloud:   n_cloud points, 4-byte aligned; may be NULL only when n_cloud == 0.  d_queries: likewise, n_queries points.
 *   d_out:     n_queries records of 16 bytes, 16-byte aligned; may be NULL only when n_queries == 0.  Every record is written:
 *              index  u32 @0   the cloud point's index; 0xFFFFFFFF when nothing was found
 *              dist2  f32 @4   d2 below; +inf when nothing was found
 *              dist   f32 @8   sqrtf(dist2)
 *              flags  u32 @12  bit 0 = found; bit 1 = the query was outside the domain
 *   d_info:    NULL, or 16 bytes, 8-byte aligned: n_found u32 @0 (with radius = tau, F-score's count), n_query_outside u32 @4,
 *              n_cloud_indexed u32 @8 (the cloud points that take part), one reserved zero word.  Integer counts: the same bytes in
 *              any order.
 * The call needs NO committed scene: the handle provides the stream, the scratch, the error text and the call's place among the
 * frames it has in flight (the cloud will usually be a frame's output).
 * The definition (csrc/ls_cloud_nearest.h: float32, every operation rounded once, no fmaf):
 *   1. D = radius * 65536.0f, r2 = radius * radius;
 *   2. a point takes part iff its three coordinates are finite and each |c| <= D: cloud points and queries alike, a query after the
 *      transform ((m0 x + m1 y) + m2 z) + m3 per row;
 *   3. a query that does not take part gets index 0xFFFFFFFF, dist2 = dist = +inf and flags 2;
 *   4. for a query q and a cloud point p_i that take part: dx = p.x - q.x, dy and dz likewise, d2 = (dx dx + dy dy) + dz dz; i is a
 *      candidate iff d2 <= r2 and, under SKIP_SAME_INDEX, i is not the query's own index;
 *   5. the answer is the minimum over the candidates of the 64-bit key (bits(d2) << 32) | i: d2 >= +0, so bit order is value order;
 *      ties go to the lowest index; a minimum has no order (ls_scene_distance_grid's key);
 *   6. dist = sqrtf(d2), flags 1.  No candidate: the record of 3 with flags 0;
 *   7. n_cloud == 0: nothing is a candidate; every query gets the record 3 or 6 gives it without one; LS_OK.
 * How the candidates are found is not part of the definition.  The library builds a hashed grid of cells of edge radius * 1.015625f
 * over the cloud, per call, and visits the 27 cells around a query's.  The domain rule of step 2 is what makes that provably complete
 * in float32: |c| <= 2^16 radius keeps a rounded quotient c / h within 2^-8 of a cell of the true one whatever the radius, the float
 * test of step 4 admits |dx| no larger than radius (1 + 2^-21), and together these stay inside the 2^-6 by which a cell is wider than
 * the radius -- so the cells of every pair that passes step 4 differ by at most 1 per axis (the argument in full:
 * csrc/ls_cloud_nearest.h).  A point beyond 65 536 radii of the origin takes no part instead of being found unreliably.
 * LS_ERR_INVALID_ARGUMENT before any device call, nothing written, in this order: a frame graph is open; NULL desc; NULL d_out with
 * n_queries > 0; NULL d_cloud with n_cloud > 0; NULL d_queries with n_queries > 0; unknown flag bits or a non-zero reserved word; a
 * radius that is not finite or outside [2^-20, 2^20]; a stride that is not a multiple of 4 in 12 .. 128; a non-finite transform;
 * misaligned pointers for the device call (cloud and queries 4 bytes, out 16, info 8).  Then LS_ERR_OUT_OF_RANGE: n_cloud > 2^27;
 * n_queries > 2^32 - 256; sort scratch that is too small.  ls_cloud_nearest_check returns the descriptor's part of this (host only,
 * no device call).  No hierarchy is touched and LS_INFO_RAY_QUERY_BUILT is left as it is; stream order, the one-call-at-a-time rule
 * and the frame graph rule are those of ls_trace_rays.  The output must not overlap the inputs.  The call keeps 28 bytes per cloud
 * point, 8 bytes per bucket (2 n_cloud rounded up to a power of two, at least 1024) and the sort's scratch on the handle, released
 * with the query state.
 * Not offered: the k nearest; all neighbours within the radius; an unbounded nearest (a radius is what bounds the work per query); an
 * index kept across calls -- every call sorts the cloud anew, so 2^20 queries in slices of 2^10 pay for the index 2^10 times: pass
 * the queries in one call --; float sums of distances (the caller reduces `dist`, e.g. with torch); a call of the ITracer adapter. */
#define LS_CLOUD_NEAREST_SKIP_SAME_INDEX 1u   /* candidate i is skipped for query i: a cloud against itself */

typedef struct ls_cloud_nearest_desc {        /* 32 bytes, no pointers */
    float    radius;          /* finite, 2^-20 <= radius <= 2^20 */
    uint32_t flags;
    uint32_t cloud_stride;    /* bytes from one cloud point to the next: a multiple of 4, 12 .. 128; x, y, z f32 at 0, 4, 8 */
    uint32_t query_stride;    /* likewise for the queries */
    uint32_t reserved[4];     /* 0 */
} ls_cloud_nearest_desc;

int ls_cloud_nearest(ls_tracer *tr, void *hip_stream, const ls_cloud_nearest_desc *desc, const float *query_to_cloud3x4,
                     const void *d_cloud, uint32_t n_cloud, const void *d_queries, uint32_t n_queries,
                     void *d_out, void *d_info);
/* The same with host memory (pageable, any alignment) in and out, on the handle's stream; returns when out and info are filled. */
int ls_cloud_nearest_host(ls_tracer *tr, const ls_cloud_nearest_desc *desc, const float *query_to_cloud3x4,
                          const void *cloud, uint32_t n_cloud, const void *queries, uint32_t n_queries,
                          void *out, void *info);
int ls_cloud_nearest_check(const ls_cloud_nearest_desc *desc);   /* host only, no device call */

/* ---- clouds in a driver's own PointCloud2 layout.  Every frame call above leaves the same fixed cloud: 32-byte XYZIR records
 * (XYZIRBytes.cpp:24-40), compacted, and next to it the ls_hit records (and, for beams, the echo words).  What a driver publishes
 * differs: Velodyne's 22-byte XYZIRT with a per-point `time` (what LIO-SAM, FAST-LIO and KISS-ICP deskew by), Ouster's organized
 * V x H image with NaN for a miss, a `label` for segmentation ground truth, a second return.  The reference's sensor config declares
 * such a layout (message.pointStep, message.pointFields[]: LidarDevice.cpp:559-584) and both of its tracers ignore it.  One more
 * pass over records that are already in device memory delivers the cloud in whatever record is asked for, ready for
 * PointCloud2::data; the frame calls, their outputs and LS_ABI_VERSION are unchanged. */
/* sources */
#define LS_FIELD_X 1          /* points32 x, y, z, intensity: float sources */
#define LS_FIELD_Y 2
#define LS_FIELD_Z 3
#define LS_FIELD_INTENSITY 4
#define LS_FIELD_RANGE 5      /* hit.t as it stands (the beams' reported range, the return model's noisy t'): float source */
#define LS_FIELD_TIME 6       /* col_time[column] + chan_time[ring], one float32 sum: float source */
#define LS_FIELD_RING 7       /* hit.ray / H        : word sources */
#define LS_FIELD_COLUMN 8     /* hit.ray % H */
#define LS_FIELD_RAY 9
#define LS_FIELD_GEOM 10      /* the label */
#define LS_FIELD_PRIM 11
#define LS_FIELD_ECHO 12      /* the word of d_echo (NULL: 0) */

typedef struct ls_cloud_field {
    uint8_t source;      /* LS_FIELD_* */
    uint8_t datatype;    /* sensor_msgs::PointField: 1 INT8, 2 UINT8, 3 INT16, 4 UINT16, 5 INT32, 6 UINT32, 7 FLOAT32, 8 FLOAT64 */
    uint16_t offset;     /* any byte offset: Velodyne's XYZIRT has its float `time` at 18 */
    float scale, bias;   /* float sources only; word sources: must be 1, 0 */
} ls_cloud_field;

#define LS_CLOUD_MAX_FIELDS 16
#define LS_CLOUD_MAX_STEP 128
#define LS_CLOUD_ORGANIZED 1u

typedef struct ls_cloud_format {
    uint32_t point_step;   /* 1..LS_CLOUD_MAX_STEP, any value (22 is real) */
    uint32_t n_fields;     /* 1..LS_CLOUD_MAX_FIELDS */
    uint32_t flags;        /* 0 or LS_CLOUD_ORGANIZED */
    uint32_t layer;        /* organized: 0..2, which of a ray's records fills the cell (below); else must be 0 */
    ls_cloud_field fields[LS_CLOUD_MAX_FIELDS];
} ls_cloud_format;         /* no pointers: travels in the kernel arguments */

/*   d_hits:  n ls_hit records, 16-byte aligned; required when n > 0.
 *   d_points32: the 32-byte points that belong to them, record for record, 16-byte aligned; required when the format names X, Y, Z
 *            or INTENSITY, and may be NULL otherwise.
 *   d_echo:  NULL, or n words, 4-byte aligned (ls_trace_scene_beams' d_echo).
 *   d_count: NULL, or the device count word of the call that produced the records: min(n, *d_count) records are handled -- no host
 *            read-back (the records of ls_trace_scene_async: d_points32, d_hits, d_n_points, n = the capacity).
 *   d_col_time: H floats indexed by the GLOBAL column, d_chan_time: V floats; device memory, 4-byte aligned, never read on the host.
 *            NULL means all zeros (the sum is still formed); d_col_time is required when the format names TIME.  H and V are the
 *            handle's raster: LS_INFO_AZIMUTH_COUNT and ls_total_channels.
 * The call needs NO committed scene: it reads only the sensor's raster size, so recorded hits can be formatted too.
 * One record, ONE operation sequence (csrc/ls_cloud_format.h; ls_debug_format_record in lidarshooter_hip_debug.h runs it on the
 * host):
 *   1. every byte of the point_step bytes is written; bytes no field covers are 0;
 *   2. a float source gives f (X, Y, Z, INTENSITY, RANGE, TIME).  With scale == 1 && bias == 0 and FLOAT32 the bits of f are stored
 *      untouched (-0 and NaN payloads included).  Otherwise g = (f * scale) + bias in float32 with no fused multiply-add (for the
 *      other datatypes with scale 1 and bias 0, g = f); FLOAT32 stores g, FLOAT64 (double)g, a NaN g as the canonical quiet NaN
 *      0x7FC00000 / 0x7FF8000000000000; the integers: a NaN g gives 0, otherwise r = rintf(g) (ties to even), saturated to the
 *      datatype's range -- below its lowest the lowest, above its highest the highest, +-inf included --, then converted;
 *   3. a word source gives a uint32 w (RING, COLUMN, RAY, GEOM, PRIM, ECHO): the integer datatypes store its low bits (a C
 *      conversion: 0xFFFFFFFF is all ones in every width), FLOAT32 (float)w, FLOAT64 (double)w;
 *   4. a record with hit.ray >= V * H is not of this raster: its RING, COLUMN and TIME sources are 0, and no table is indexed by
 *      it.  Every index is checked before an address is formed from it.
 *   Values are little-endian.
 * Unorganized (flags = 0): record i of the output is record i of the input; min(n, *d_count) * point_step bytes are written from
 *   d_out and nothing past them; n = 0 writes nothing.
 * Organized (LS_CLOUD_ORGANIZED): the output is exactly V * H records, cell c = v * H + h at byte c * point_step: the FULL raster
 *   whatever the shard (the cells of other shards are misses); n = 0 gives V * H misses.  The rank of input record i is the number
 *   of immediately preceding records i-1, i-2, i-3 that carry the same ray, counted up to the first one that differs: 0..3.  A
 *   record fills its ray's cell when its rank equals fmt->layer; a record of rank 3 is never used.  Every producer in the library
 *   emits a ray's records adjacently and a beam's in ascending range: layer 0 is the nearest return, layer 1 the second (Ouster's
 *   two range images).  If several non-adjacent records claim one cell, the cell holds one of them whole; which one is
 *   unspecified.  A record with ray >= V * H is left out.  A cell nobody fills is a miss: X, Y, Z, INTENSITY and RANGE have f =
 *   the canonical NaN (float types store NaN, integer types 0), GEOM and PRIM are 0xFFFFFFFF, ECHO is 0, and RING, COLUMN, RAY and
 *   TIME are the cell's own -- a missed cell still has a ring and a firing time.
 * LS_ERR_INVALID_ARGUMENT before any device call, in this order: a frame graph is open; a NULL handle or format; a format
 * ls_cloud_format_check refuses; NULL hits with n > 0, or a NULL output where something is to be written; X, Y, Z or INTENSITY named
 * without points (n > 0); TIME named without d_col_time; misaligned pointers (16 bytes for d_out, points and hits; 4 for the words
 * and the times).  LS_ERR_OUT_OF_RANGE: n above 0xFFF00000.  The output must not overlap the inputs.  Stream order and the frame
 * graph rule are those of ls_hit_attributes; LS_INFO_RAY_QUERY_BUILT is left as it is; frames of ls_trace_scene* are unaffected.
 * The organized mode uses a scratch map of V * H words on the handle, grown on demand and released with the query state; calls on
 * one handle use it one after the other.
 * Not offered: a call of the ITracer adapter; big-endian clouds; fields with count > 1; planar (structure-of-arrays) images. */
int ls_format_cloud(ls_tracer *tr, void *hip_stream, const ls_cloud_format *fmt,
                    const void *d_points32, const void *d_hits, const uint32_t *d_echo,
                    const uint32_t *d_count, uint32_t n,
                    const float *d_col_time, const float *d_chan_time, void *d_out);
/* The same with host memory (pageable, any alignment) in and out and no count word, on the handle's stream; returns when out is
 * filled (n * point_step bytes, or V * H * point_step organized). */
int ls_format_cloud_host(ls_tracer *tr, const ls_cloud_format *fmt, const void *points32, const void *hits,
                         const uint32_t *echo, uint32_t n, const float *col_time, const float *chan_time, void *out);

/* host only, no handle, no device */
/* LS_OK, or LS_ERR_INVALID_ARGUMENT for: a NULL format; a step outside 1..LS_CLOUD_MAX_STEP or a field count outside
 * 1..LS_CLOUD_MAX_FIELDS; an unknown source, datatype or flag bit; layer > 2, or layer != 0 without LS_CLOUD_ORGANIZED; a field that
 * does not fit inside the step; two fields that overlap; a non-finite scale or bias, or a scale or bias other than 1 and 0 on a word
 * source. */
int ls_cloud_format_check(const ls_cloud_format *fmt);
/* A format from what the reference's sensor config declares (message.pointFields[] and message.pointStep, LidarDevice.cpp:570-582):
 * names match case-sensitively -- x, y, z, intensity; ring, channel -> RING; time, t, timestamp -> TIME; range, distance -> RANGE;
 * label, geom -> GEOM; prim -> PRIM; ray -> RAY; column -> COLUMN; echo, return_type -> ECHO --, scale 1, bias 0, flags and layer 0.
 * LS_ERR_UNSUPPORTED_TYPE for an unknown name or a count other than 1; LS_ERR_INVALID_ARGUMENT for NULL pointers, more than
 * LS_CLOUD_MAX_FIELDS fields, an offset above 65535, or a result ls_cloud_format_check refuses. */
int ls_cloud_format_from_point_fields(const char *const *names, const uint32_t *offsets, const uint8_t *datatypes,
                                      const uint32_t *counts, uint32_t n_fields, uint32_t point_step, ls_cloud_format *out);
/* Firing times of the azimuth columns: tau_h = t0 + h * dt evaluated in double and rounded once to float32 -- the tau of
 * ls_sweep_poses_constant_twist and ls_motion_constant_twist.  col_time: n_cols floats.  LS_ERR_INVALID_ARGUMENT for a NULL pointer
 * or non-finite inputs. */
int ls_column_times(double t0, double dt, uint32_t n_cols, float *col_time);

#ifdef __cplusplus
}
#endif
#endif /* LIDARSHOOTER_HIP_H */
