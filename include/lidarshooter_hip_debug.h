/*
 * lidarshooter_hip_debug.h -- test and measurement hooks of liblidarshooter_hip.so: views into a tracer handle that
 * tests/ and bench.py use to compare the device's results with the CPU oracle.  Not part of the drop-in surface of
 * include/lidarshooter_hip.h (no ITracer virtual maps to any of these) and not needed by the adapter.
 */
#ifndef LIDARSHOOTER_HIP_DEBUG_H
#define LIDARSHOOTER_HIP_DEBUG_H

#include "lidarshooter_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fault injection (values live in the option / flag spaces of the public headers, their names do not) --------- */
/* ls_tracer_set_option: 1 makes the next pipelined frame publish a wrong epoch, so that the chained prefix gives up and
 * the device status word is raised (one frame). */
#define LS_OPT_DEBUG_FAULT 9
/* ls_group_create_opts (include/lidarshooter_group.h): the gathered arrangement answers are treated as if a peer had
 * answered "neither" -- a one-rank test takes the disagreement path.  (With two real ranks tests/shim/ makes a peer that
 * really refuses.) */
#define LS_GROUP_FLAG_DEBUG_PEER_REFUSES 0x100u

/* Dense per-ray results of the last trace, host buffers of n_rays entries (shard-local order
 * q = v*n_az + (h-first_az)): t (< 0 = miss) and global triangle id (0xFFFFFFFF = miss). */
int ls_debug_dense_hits(ls_tracer *tr, float *t, uint32_t *gid);

/* Exhaustive closest hit on the device (every ray against every triangle, same triangle test):
 * the full-size checker for the BVH path. */
int ls_debug_trace_bruteforce(ls_tracer *tr, float *t, uint32_t *gid);

/* Transformed (sensor-frame) vertices and rebased indices of the committed scene. */
int ls_debug_scene_size(ls_tracer *tr, uint32_t *n_verts, uint32_t *n_tris, uint32_t *n_node_slots,
                        uint32_t *leaf_size);
int ls_debug_download_scene(ls_tracer *tr, float *verts_xyz, uint32_t *tri_idx);

/* BVH arrays: n_node_slots BVH2 nodes (64 B each) and n_tris triangle records (48 B each):
 *   node i: float4 q[4] = (L.lo.xyz, bits(left ref)), (L.hi.xyz, bits(right ref)), (R.lo.xyz, 0), (R.hi.xyz, 0)
 *     child ref: bit 31 set = leaf k (records [k*leaf_size, k*leaf_size+leaf_size) clipped to n_tris),
 *     else index of another node; node 0 is the root (a one-leaf scene has no node at all)
 *   triangle record: float v0[3]; uint32 gid; float e1[3]; float NgC; float e2[3]; uint32 pad */
int ls_debug_download_bvh(ls_tracer *tr, void *nodes, void *tri_records);

/* The hierarchy of geometry geom_id in the frame path's instanced set (the default of the BVH engine: one hierarchy per geometry
 * in MESH space): *n_leaves, *leaf_size, n_leaves - 1 binary nodes (64 B each, as above; references and leaf ranges local to the
 * geometry), their n_leaves - 1 four-wide twins (128 B each: float4 lo[4], hi[4]; lo[c].w = slot c's reference, 0xFFFFFFFF empty)
 * and the geometry's triangle records (48 B each: float v0[3]; uint32 local id; float v1[3]; uint32 0; float v2[3]; uint32 0 --
 * the corners as uploaded).  NULL pointers: sizes only.  LS_ERR_NOT_COMMITTED when the commit was not instanced, and for wide128
 * while the four-wide twins of this hierarchy have not been made; LS_ERR_UNKNOWN_GEOMETRY for a geometry the commit left out. */
int ls_debug_download_hierarchy(ls_tracer *tr, uint32_t geom_id, uint32_t *n_leaves, uint32_t *leaf_size, void *nodes64, void *wide128,
                                void *records48);

/* The build path's radix sort on its own (ls_sort.hip): sorts n (key, value) pairs by their 30-bit keys in place (host
 * arrays; stable: equal keys keep their input order). */
int ls_debug_sort_pairs(ls_tracer *tr, uint32_t *keys, uint32_t *vals, uint32_t n);

/* The host half of ls_trace_scene_expand on its own (no device, no handle): n 8-byte (ray, t) records in ascending ray
 * order -> n 32-byte points, from factor tables sin_theta[V], cos_theta[V] and interleaved (cos_phi, sin_phi)[H]. */
int ls_debug_expand_hits(void *dst_points32, const void *hits8, uint32_t n, const float *sin_theta, const float *cos_theta,
                         const float *cs_phi, uint32_t V, uint32_t H);

/* the library's point-triangle arithmetic on the host (no device, no handle): q[3], *d2 -- the float32 operation sequence
 * k_closest_points runs per triangle (csrc/ls_closest.h); d2 = +inf, q = 0 for a triangle that never counts */
int ls_debug_closest_on_triangle(const float p[3], const float v0[3], const float v1[3], const float v2[3], float q[3], float *d2);

/* the library's hit-attribute arithmetic on the host (no device, no handle): the float32 operation sequence k_hit_attributes
 * runs per triangle (csrc/ls_hit_attr.h) -- the exact ray / triangle test from the origin o, then normal, incidence cosine,
 * barycentrics and hit point.  Returns 1 when the test passes (*t and out9 written), 0 when it does not (nothing written). */
int ls_debug_hit_attributes_on_triangle(const float o[3], const float d[3], const float v0[3], const float v1[3], const float v2[3], float *t, float out9[9] /* n, cos_inc, u, v, p */);

/* Philox4x32-10 as ls_apply_return_model draws it (csrc/ls_return_model.h), on the host: no device, no handle */
int ls_debug_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* the library's return model on the host (no device, no handle): steps 2-8 of ls_apply_return_model for one valid hit of ray
 * `ray` -- t, len = |d|, the incidence cosine, the reflectivity rho --, the float32 operation sequence k_returns_eval runs.
 * Returns 1 when the return is kept, 0 when it is lost (*t_out = t', *intensity = I either way), a negative status for NULL
 * pointers or a model ls_apply_return_model refuses. */
int ls_debug_return_model(const ls_return_model *m, uint32_t ray, uint32_t frame_index, float t, float len, float cos_inc, float rho,
                          float *t_out, float *intensity);

/* the ray ls_trace_scene_sweep casts for a nominal direction d under one column's pose record (12 floats, [R | o] row-major), on
 * the host (no device, no handle): the float32 operation sequence k_sweep_rays runs (csrc/ls_sweep.h) -> the 32-byte
 * lidarshooter::Ray record: origin o, tmin 0, d'_i = (R[i][0] dx + R[i][1] dy) + R[i][2] dz, tmax 1e16 */
int ls_debug_sweep_ray(const float d[3], const float pose12[12], float ray8[8]);

/* the sub-ray ls_trace_scene_beams casts for sample abk = (a, b, k) of the ray with the factor-table entries sin_theta, cos_theta,
 * (cos_phi, sin_phi), on the host (no device, no handle): the float32 operation sequence k_beam_rays runs (csrc/ls_beam.h) -> the
 * 32-byte lidarshooter::Ray record: origin 0, tmin 0, d_i = (d_i + a u_i) + b w_i, tmax 1e16 */
int ls_debug_beam_ray(float sin_theta, float cos_theta, float cos_phi, float sin_phi, const float abk[3], float ray8[8]);
/* the echoes of one beam on the host (no device, no handle; the model's pattern is not read): r and hit hold the reported range
 * r_s = t_s * k_s and a hit flag (0: a miss) of each of the model's n_samples sub-rays; the keys, the echo starts and the selection
 * k_beam_reduce runs (csrc/ls_beam.h) -> *n_out returns, 0..3, in ascending range, two words each in out: the bits of r_e and the
 * echo word of ls_trace_scene_beams' d_echo.  LS_ERR_INVALID_ARGUMENT for NULL pointers, n_samples outside 1..64, no or unknown
 * return bits, min_count outside 1..n_samples, a NaN or negative separation. */
int ls_debug_beam_echoes(const ls_beam_model *model, const float *r, const uint8_t *hit, uint32_t *out /* up to 3 x {r bits, echo word} */, uint32_t *n_out);
/* the status ls_trace_scene_beams would return for this model on a handle whose shard has shard_rays rays, with this capacity and
 * otherwise valid arguments (no device, no handle): LS_OK, LS_ERR_INVALID_ARGUMENT or LS_ERR_OUT_OF_RANGE */
int ls_debug_beam_model_check(const ls_beam_model *model, uint32_t shard_rays, uint32_t capacity);

/* the sub-ray ls_trace_scene_beams_sweep casts for sample abk of the ray with these factor-table entries under one column's pose
 * record, on the host (no device, no handle): ls_debug_beam_ray's sequence, then ls_debug_sweep_ray's on its direction -- what
 * k_beam_sweep_rays runs -> origin o, tmin 0, d'_s = R d_s, tmax 1e16 */
int ls_debug_beam_sweep_ray(float sin_theta, float cos_theta, float cos_phi, float sin_phi, const float abk[3], const float pose12[12], float ray8[8]);
/* ls_debug_beam_echoes with a weight per sample (NULL: 1 each; n_samples integers in 1..65535 otherwise) and the strength threshold
 * min_weight: the keys, the echo starts, the strengths and the selection k_beam_reduce_weighted runs (csrc/ls_beam.h) -> *n_out
 * returns, 0..3, in ascending range, three words each in out: the bits of r_e, the echo word and the strength W_e.
 * LS_ERR_INVALID_ARGUMENT as ls_debug_beam_echoes, and for a weight outside 1..65535. */
int ls_debug_beam_echoes_weighted(const ls_beam_model *model, const uint32_t *weights, uint32_t min_weight, const float *r, const uint8_t *hit, uint32_t *out /* up to 3 x {r bits, echo word, W_e} */, uint32_t *n_out);
/* the status ls_trace_scene_beams_sweep would return for this model and these weights (NULL: 1 each) on a handle whose shard has
 * shard_rays rays, with this capacity and otherwise valid arguments (no device, no handle) */
int ls_debug_beam_sweep_check(const ls_beam_model *model, const uint32_t *weights, uint32_t shard_rays, uint32_t capacity);


/* the ray a moving geometry sees (ls_trace_scene_sweep_moving): the 32-byte ray record ray8_in through the inverse of one motion
 * record (12 floats, [Q | c] row-major), on the host (no device, no handle): the float32 operation sequence k_trace_rays_moving
 * runs (csrc/ls_motion.h) -> origin Q^T (o - c), tmin 0, direction Q^T d, tmax 1e16 */
int ls_debug_motion_ray(const float ray8_in[8], const float motion12[12], float ray8_out[8]);
/* the normal of a moving geometry back in the sensor frame (ls_hit_attributes_moving): the normal n3 found on the geometry where it
 * was committed, carried forward by one motion record, on the host (no device, no handle): the float32 operation sequence
 * k_hit_attributes_moving runs (csrc/ls_motion.h) -> out_i = (Q[i][0] n_0 + Q[i][1] n_1) + Q[i][2] n_2 */
int ls_debug_motion_normal(const float n3[3], const float motion12[12], float out3[3]);
/* one valid record of ls_hit_velocities on the host (no device, no handle): the float32 operation sequence k_hit_velocities runs
 * (csrc/ls_velocity.h) for a hit at t along the ray its column cast (cast8: ls_debug_sweep_ray's record, or origin 0 and the nominal
 * direction without a pose table), with the column's twist records [w | u] of the sensor and of the geometry that was hit; either
 * may be NULL: at rest, that velocity is (+0, +0, +0) -> the 32-byte record: v_s xyz, radial, v_o xyz, flags = 1 */
int ls_debug_hit_velocity(const float cast8[8], float t, const float sensor_twist6[6], const float geom_twist6[6], float out8[8]);

/* one ray of ls_occupancy_grid on the host (no device, no handle): the float32 operation sequence k_voxel_carve runs per ray
 * (csrc/ls_voxel.h) -- the affine (sensor_to_grid3x4, or NULL), the span of the header's table, the occupied cell and the walk.
 * ray32: a 32-byte ray record (origin xyz, tmin, direction xyz, tmax); t_end: the t of the ray's deciding record, or NaN: the ray has
 * none (it carves only with LS_OCC_CARVE_MISSES in grid->flags).  -> cells_out[0 .. min(*n_cells, capacity)): the cells the walk
 * visits, in order, as word-pair indices (z ny + y) nx + x -- the ray's own occupied cell among them where the walk reaches it --;
 * *n_cells: how many it visits; *occupied_cell_out: the cell the record's point marks, or 0xFFFFFFFF.  A ray that is not walkable
 * visits and marks nothing.  LS_ERR_INVALID_ARGUMENT for NULL grid, ray32, n_cells or occupied_cell_out, NULL cells_out with capacity
 * > 0, a non-finite transform or a descriptor ls_occupancy_grid_check refuses; LS_ERR_OUT_OF_RANGE when *n_cells > capacity. */
int ls_debug_voxel_walk(const ls_occupancy_grid_desc *grid, const float *sensor_to_grid3x4, const float ray32[8], float t_end,
                        uint32_t *cells_out, uint32_t capacity, uint32_t *n_cells, uint32_t *occupied_cell_out);

/* one triangle of ls_scene_grid on the host (no device, no handle): the float32 operation sequence k_scene_grid_small and
 * k_scene_grid_big run per triangle and per cell (csrc/ls_scene_grid.h) -- q = v - origin, the clamped cell range and the 13-axis
 * test of every cell of it.  tri9: the three vertices, already in the grid's frame.  -> cells_out[0 .. min(*n_cells, capacity)): the
 * overlapping cells as word indices (z ny + y) nx + x, ascending; *n_cells: how many there are.  A triangle with a non-finite q or
 * outside the grid has none.  LS_ERR_INVALID_ARGUMENT for NULL grid, tri9 or n_cells, NULL cells_out with capacity > 0 or a
 * descriptor ls_scene_grid_check refuses; LS_ERR_OUT_OF_RANGE when *n_cells > capacity. */
int ls_debug_scene_grid_triangle(const ls_scene_grid_desc *grid, const float tri9[9], uint32_t *cells_out, uint32_t capacity,
                                 uint32_t *n_cells);
/* how many triangles the handle's last ls_scene_grid call queued for k_scene_grid_big: the count word of the queue, read back after a
 * wait for the handle's stream (a call on a caller's stream must have been waited for by the caller); 0 before the first call */
int ls_debug_scene_grid_queued(ls_tracer *tr, uint32_t *n_queued);

/* one triangle of ls_scene_distance_grid on the host (no device, no handle): the float32 operation sequence k_distance_grid_small and
 * k_distance_grid_big run per triangle and per cell (csrc/ls_distance_grid.h) -- q = v - origin, the widened, clamped cell range and
 * closest_on_triangle from every cell centre of it.  tri9: the three vertices, already in the grid's frame.  -> cells_out / dist_out
 * [0 .. min(*n_cells, capacity)): the cells that count (dist <= trunc) as record indices (z ny + y) nx + x, ascending, and their dist;
 * *n_cells: how many there are.  A triangle with a non-finite q, without area or farther than trunc from the grid has none.
 * LS_ERR_INVALID_ARGUMENT for NULL grid, tri9 or n_cells, NULL cells_out or dist_out with capacity > 0 or a descriptor
 * ls_scene_distance_grid_check refuses; LS_ERR_OUT_OF_RANGE when *n_cells > capacity. */
int ls_debug_distance_grid_triangle(const ls_distance_grid_desc *grid, const float tri9[9], uint32_t *cells_out, float *dist_out,
                                    uint32_t capacity, uint32_t *n_cells);
/* how many triangles the handle's last ls_scene_distance_grid call queued for k_distance_grid_big: the count word of the queue, read
 * back after a wait for the handle's stream (a call on a caller's stream must have been waited for by the caller); 0 before the
 * first call */
int ls_debug_distance_grid_queued(ls_tracer *tr, uint32_t *n_queued);

/* ls_sample_surface on the host (no device, no handle): the float32 / integer sequences its kernels run (csrc/ls_surface_sample.h).
 * ls_debug_surface_weights: steps 2 to 5 over n triangles already in the output frame (tris9: 9 floats each; every one counts as
 * selected) -> area_out[n] (+0 for a triangle of weight 0), weight_out[n], prefix_out[n + 1] and the 16 bytes of the call's info
 * (weight_total, exponent, n_weighted); any output may be NULL.
 * ls_debug_surface_pick: step 7 for the 64-bit word r64 over a prefix of n + 1 entries -> *tri_out, or 0xFFFFFFFF when prefix[n] is 0.
 * ls_debug_surface_point: steps 2, 8 and 9 for one triangle and the words x2, x3 -> out9 = the point, the unit normal, u, v, w.
 * LS_ERR_INVALID_ARGUMENT for a NULL input or result pointer. */
int ls_debug_surface_weights(const float *tris9, uint32_t n, float *area_out, uint64_t *weight_out, uint64_t *prefix_out, void *info_out);
int ls_debug_surface_pick(const uint64_t *prefix, uint32_t n, uint64_t r64, uint32_t *tri_out);
int ls_debug_surface_point(const float tri9[9], uint32_t x2, uint32_t x3, float out9[9]);

/* ls_cloud_nearest's index on the host (no device, no handle): the sequences its kernels run (csrc/ls_cloud_nearest.h).
 * ls_debug_cloud_cell: for n points (xyz: 3 floats each) under `radius`, whether each takes part (takes_part_out[n], 0 / 1) and its
 * cell (cell_out[3 n]; zeros for a point that does not take part).  LS_ERR_INVALID_ARGUMENT for a radius the call refuses or a NULL
 * pointer with n > 0.
 * ls_debug_cloud_bucket: the bucket of a cell in a table of 2^log2_buckets (10 .. 27); 0xFFFFFFFF for a NULL cell or another size.
 * The tests hold the 27-cell claim against the first and construct hash collisions with the second; no result of the device is ever
 * compared with either. */
int ls_debug_cloud_cell(float radius, const float *xyz, uint32_t n, int32_t *cell_out, uint8_t *takes_part_out);
uint32_t ls_debug_cloud_bucket(const int32_t cell[3], uint32_t log2_buckets);

/* one record of ls_format_cloud on the host (no device, no handle): the operation sequence k_format_cloud runs per record
 * (csrc/ls_cloud_format.h).  point32: the 32-byte point, or NULL (zeros: the format names none of its fields); hit: the ls_hit, or
 * NULL -- the miss cell of cell_ray (an organized cloud's cell nobody fills); echo_word; col_time_value / chan_time_value: the
 * entries of the record's column and ring (ignored for a ray >= V * H, whose ring, column and time are 0); out_bytes: point_step
 * bytes, all written.  LS_ERR_INVALID_ARGUMENT for NULL fmt / out_bytes or a format ls_cloud_format_check refuses. */
int ls_debug_format_record(const ls_cloud_format *fmt, const void *point32, const ls_hit *hit, uint32_t echo_word,
                           float col_time_value, float chan_time_value, uint32_t V, uint32_t H, uint32_t cell_ray, void *out_bytes);

/* k_project's start of a footprint's channel band by guess and verify (csrc/ls_band_map.h), on the host (no device, no handle).
 * ls_debug_band_map_fit: the map the library fits to an ascending table tan_up[V] -> map8 = a0 a1 a2 a3 t0 t1 (floats), then back
 * and walk (int32 words); walk < 0: the handle would keep the bisection.  ls_debug_band_guess: the kernel's start position
 * (0 .. V) for the query t under such a map, the float32 operation sequence the kernel runs.  ls_debug_tracer_band_map: the
 * map a handle's frames use, same layout. */
int ls_debug_band_map_fit(const float *tan_up, uint32_t V, float map8[8]);
int ls_debug_band_guess(const float map8[8], uint32_t V, float t, uint32_t *start);
int ls_debug_tracer_band_map(const ls_tracer *tr, float map8[8]);

/* ---- group culling of the projection engine (k_group_bounds, k_cull: csrc/ls_project.hip) ----------------------------
 * ls_debug_force_group_cull: while on, LS_OPT_BLOCK_CULL = 1 applies to a geometry of ANY size from one triangle (as shipped
 * it applies to meshes large enough for waves of 64 triangles: 524 225 or more); the culling data is made by the next commit.
 * Off (the default): nothing changes. */
int ls_debug_force_group_cull(ls_tracer *tr, int on);
/* The culling data of committed geometry geom_id: *n_tris; perm[n_tris]: sorted position -> the caller's triangle;
 * group_boxes: 8 floats per group of 4 sorted triangles (the last group may be partial) = (cx, cy, cz, hx), (hy, hz, sx, sy):
 * the mesh-space box { c + a e1 + b e2 + g e3 : |a|, |b|, |g| <= 1 }, e1 = (hx, 0, sx hx), e2 = (0, hy, sy hy), e3 = (0, 0, hz);
 * hx = +inf: unbounded (never rejected); block_boxes: the same per 64 groups.  NULL pointers are skipped.
 * LS_ERR_NOT_COMMITTED when the geometry has no current culling data. */
int ls_debug_download_cull(ls_tracer *tr, uint32_t geom_id, uint32_t *n_tris, uint32_t *perm, float *group_boxes, float *block_boxes);
/* The groups of geometry geom_id that the NEXT frame's cull pass keeps: the pass is run as launch_project would run it --
 * committed scene, current poses and shard, the same batch of geometries, the same k_cull instantiation -- into scratch of this
 * call (the frames' counters, survivor lists, statistics and hint word are not touched), synchronously.  out[0 .. *n): group
 * numbers ascending (LS_ERR_OUT_OF_RANGE when *n > cap; *n is set); *variant: LS_DEBUG_CULL_* bits of the instantiation, or
 * LS_DEBUG_CULL_UNCULLED alone when the frame projects every triangle of the geometry (no culling data, or more culled
 * geometries than one launch takes: 17): then every group is reported. */
#define LS_DEBUG_CULL_LUT 1u        /* channel query by look-up table (else binary search) */
#define LS_DEBUG_CULL_LDS 2u        /* channel tables staged in LDS (else read from global memory: V > 2048) */
#define LS_DEBUG_CULL_SECTOR 4u     /* azimuth-sector test of a shard narrower than half a turn */
#define LS_DEBUG_CULL_COUNT 8u      /* LS_OPT_COUNT_VISITS: the counting instantiation */
#define LS_DEBUG_CULL_UNCULLED 16u
int ls_debug_cull_survivors(ls_tracer *tr, uint32_t geom_id, uint32_t *out, uint32_t cap, uint32_t *n, uint32_t *variant);
/* The channel tables k_cull queries, V entries each in ascending elevation: tan_up, tan_dn, the channel of each position, and
 * whether the look-up table passed the host's check (NULL pointers are skipped). */
int ls_debug_cull_tables(ls_tracer *tr, float *tan_up, float *tan_dn, uint32_t *chan_perm, int *lut_ok);
/* k_cull's channel query on the device -- is there a channel i with tan_up[i] >= tan_lo and tan_dn[i] <= tan_hi -- for n
 * (tan_lo, tan_hi) pairs against the handle's tables, staged as k_cull stages them: lut_search[2 i] = the look-up table's
 * answer (0 / 1; 2 when this handle's k_cull does not use the table), lut_search[2 i + 1] = the binary search's. */
int ls_debug_chan_query(ls_tracer *tr, const float *tan_lo_hi, uint32_t n, uint8_t *lut_search);

#ifdef __cplusplus
}
#endif
#endif /* LIDARSHOOTER_HIP_DEBUG_H */
