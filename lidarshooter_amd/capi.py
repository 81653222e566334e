"""ctypes binding of the C ABI in include/lidarshooter_hip.h (liblidarshooter_hip.so).

Used by tests/, bench.py and __graft_entry__.py to drive the HIP library exactly the way the
reference's C++ adapter would (one call per ITracer virtual, ITracer.hpp:50-94).  This module
holds no algorithm: if the shared library is missing it raises, it never computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LS_LIB_PATH: kernel-variant experiments (tools/) load another build of the same library
LIB_PATH = os.environ.get("LS_LIB_PATH") or os.path.join(_HERE, "liblidarshooter_hip.so")
INVALID = 0xFFFFFFFF
ABI_VERSION = 4   # include/lidarshooter_hip.h: LS_ABI_VERSION (checked at load)

LS_OPT_LEAF_SIZE, LS_OPT_TIMING, LS_OPT_COUNT_VISITS, LS_OPT_ENGINE, LS_OPT_PIPELINE = 1, 2, 3, 5, 6
LS_OPT_HOST_OUTPUT, LS_OPT_READBACK_HITS, LS_OPT_DEBUG_FAULT, LS_OPT_BLOCK_CULL, LS_OPT_BVH_REFIT = 7, 8, 9, 10, 11
LS_INFO_LAST_COMMIT_REFIT = 6
LS_OPT_BVH_INSTANCED = 12
LS_OPT_UPLOAD_MODE = 13
LS_OPT_FRAME_GRAPH = 14
LS_OPT_EMIT_POINTS = 15
LS_OPT_BVH_WIDE = 16
LS_INFO_BVH_WIDE = 16
LS_INFO_FRAME_GRAPH_LAST_PATCHED = 13
LS_INFO_EMIT_POINTS, LS_INFO_FRAME_GRAPH_PATCH_WAITS = 14, 15
LS_INFO_NEXT_SLOT, LS_INFO_FRAME_GRAPH_STATE, LS_INFO_FRAME_GRAPH_CAPTURES, LS_INFO_FRAME_GRAPH_REPLAYS, LS_INFO_FRAME_GRAPH_PATCHES = 8, 9, 10, 11, 12
LS_GEOMETRY_TYPE_TRIANGLE, LS_GEOMETRY_TYPE_QUAD = 0, 1
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("direction", "<f4", 3), ("tmax", "<f4")])   # Ray.hpp:16-35
REFHIT_DTYPE = np.dtype([("t", "<f4"), ("normal", "<f4", 3), ("intensity", "<f4"), ("ring", "<i4")])       # Hit.hpp:16-29
LS_INFO_BVH_INSTANCED = 7
LS_INFO_RAY_QUERY_BUILT = 17
LS_OPT_STANDING = 17
LS_INFO_STANDING_GEOMETRIES, LS_INFO_STANDING_BUILDS, LS_INFO_STANDING_RECORDS = 18, 19, 20
LS_INFO_STANDING_BASE, LS_INFO_STANDING_BASE_BUILDS, LS_INFO_STANDING_BASE_NO_FINISH = 21, 22, 23
LS_INFO_CONCURRENT_STREAMS, LS_INFO_PIPELINE_MODE, LS_INFO_DEVICE_STATUS, LS_INFO_HOST_THREADS, LS_INFO_AZIMUTH_COUNT = 1, 2, 3, 4, 5
ENGINE_AUTO, ENGINE_BVH, ENGINE_PROJECTION = 0, 1, 2
STAGES = ("transform", "morton", "sort", "leaves", "range_tree", "hierarchy", "trace", "trace_aux", "pack")

# every symbol include/lidarshooter_hip.h declares (tests/test_abi.py checks the .so exports them all)
SYMBOLS = (
    "ls_abi_version", "ls_source_hash", "ls_tracer_create", "ls_tracer_create_tables", "ls_tracer_destroy", "ls_parallel_copy", "ls_expand_points", "ls_get_info", "ls_affine_from_components", "ls_add_geometry", "ls_remove_geometry",
    "ls_update_geometry", "ls_update_geometry_components", "ls_update_geometry_device",
    "ls_update_geometry_device_shared", "ls_update_geometry_transform", "ls_commit_scene", "ls_trace_scene", "ls_trace_scene_async",
    "ls_geometry_count", "ls_geometry_id", "ls_vertex_count", "ls_element_count", "ls_total_rays",
    "ls_total_channels", "ls_last_error", "ls_tracer_set_shard", "ls_tracer_set_stream",
    "ls_tracer_synchronize", "ls_tracer_flush", "ls_tracer_set_output_buffers", "ls_tracer_set_hit_buffers", "ls_expand_gathered_hits", "ls_expand_gathered_hits_on", "ls_cloud_to_world", "ls_tracer_set_option", "ls_get_timings",
    "ls_get_visit_counts", "ls_generate_rays", "ls_generate_rays_aos", "ls_geometry_type", "ls_tracer_order_after_last_frame", "ls_tracer_wait_event", "ls_tracer_next_frame_waits", "ls_trace_scene_begin", "ls_trace_scene_expand",
    "ls_frame_graph_begin", "ls_frame_graph_stream", "ls_frame_graph_end", "ls_frame_graph_reset",
    "ls_tracer_set_sensor", "ls_tracer_set_sensor_tables", "ls_expand_gathered_hits_sized",
    "ls_trace_rays", "ls_trace_rays_host", "ls_occluded_rays", "ls_occluded_rays_host",
    "ls_closest_points", "ls_closest_points_host",
    "ls_hit_attributes", "ls_hit_attributes_host",
    "ls_apply_return_model", "ls_apply_return_model_host",
    "ls_trace_scene_sweep", "ls_trace_scene_sweep_host", "ls_sweep_poses_constant_twist",
    "ls_trace_scene_beams", "ls_trace_scene_beams_host", "ls_beam_pattern_rings",
    "ls_trace_scene_beams_sweep", "ls_trace_scene_beams_sweep_host", "ls_beam_weights_gaussian",
    "ls_trace_scene_sweep_moving", "ls_trace_scene_sweep_moving_host", "ls_motion_constant_twist",
    "ls_hit_attributes_moving", "ls_hit_attributes_moving_host", "ls_apply_return_model_moving", "ls_apply_return_model_moving_host",
    "ls_hit_velocities", "ls_hit_velocities_host", "ls_twist_table_constant",
    "ls_object_labels", "ls_object_labels_host",
    "ls_occupancy_grid", "ls_occupancy_grid_host", "ls_occupancy_grid_check",
    "ls_scene_grid", "ls_scene_grid_host", "ls_scene_grid_check",
    "ls_scene_distance_grid", "ls_scene_distance_grid_host", "ls_scene_distance_grid_check",
    "ls_sample_surface", "ls_sample_surface_host", "ls_surface_sample_check",
    "ls_cloud_nearest", "ls_cloud_nearest_host", "ls_cloud_nearest_check",
    "ls_format_cloud", "ls_format_cloud_host", "ls_cloud_format_check", "ls_cloud_format_from_point_fields", "ls_column_times",
)
# include/lidarshooter_hip_debug.h: test / measurement hooks (not part of the drop-in surface)
DEBUG_SYMBOLS = ("ls_debug_dense_hits", "ls_debug_trace_bruteforce", "ls_debug_scene_size", "ls_debug_download_scene",
                 "ls_debug_download_bvh", "ls_debug_download_hierarchy", "ls_debug_sort_pairs", "ls_debug_expand_hits", "ls_debug_closest_on_triangle",
                 "ls_debug_hit_attributes_on_triangle", "ls_debug_philox4x32", "ls_debug_return_model", "ls_debug_sweep_ray",
                 "ls_debug_beam_ray", "ls_debug_beam_echoes", "ls_debug_beam_model_check",
                 "ls_debug_beam_sweep_ray", "ls_debug_beam_echoes_weighted", "ls_debug_beam_sweep_check", "ls_debug_motion_ray",
                 "ls_debug_motion_normal", "ls_debug_hit_velocity", "ls_debug_format_record", "ls_debug_voxel_walk", "ls_debug_scene_grid_triangle", "ls_debug_scene_grid_queued",
                 "ls_debug_distance_grid_triangle", "ls_debug_distance_grid_queued",
                 "ls_debug_surface_weights", "ls_debug_surface_pick", "ls_debug_surface_point",
                 "ls_debug_cloud_cell", "ls_debug_cloud_bucket",
                 "ls_debug_band_map_fit", "ls_debug_band_guess", "ls_debug_tracer_band_map",
                 "ls_debug_force_group_cull", "ls_debug_download_cull", "ls_debug_cull_survivors", "ls_debug_cull_tables", "ls_debug_chan_query")
# ls_debug_cull_survivors: which k_cull instantiation ran
LS_DEBUG_CULL_LUT, LS_DEBUG_CULL_LDS, LS_DEBUG_CULL_SECTOR, LS_DEBUG_CULL_COUNT, LS_DEBUG_CULL_UNCULLED = 1, 2, 4, 8, 16


class SensorDesc(C.Structure):
    _fields_ = [("vertical_deg", C.POINTER(C.c_float)), ("n_vertical", C.c_uint32), ("h_begin", C.c_float),
                ("h_end", C.c_float), ("h_count", C.c_uint32), ("Rinv", C.c_float * 9), ("t", C.c_float * 3)]


class SensorTables(C.Structure):
    _fields_ = [("sin_theta", C.POINTER(C.c_float)), ("cos_theta", C.POINTER(C.c_float)),
                ("elevation_deg", C.POINTER(C.c_float)), ("n_vertical", C.c_uint32),
                ("sin_phi", C.POINTER(C.c_float)), ("cos_phi", C.POINTER(C.c_float)), ("h_count", C.c_uint32),
                ("h_begin_deg", C.c_float), ("h_step_deg", C.c_float), ("Rinv", C.c_float * 9), ("t", C.c_float * 3)]


LS_RETURN_LAMBERT = 1
LS_RETURN_TWO_SIDED = 2
LS_SWEEP_DESKEW = 1   # ls_trace_scene_sweep: points in the frame-start sensor frame instead of the instantaneous one


LS_BEAM_FIRST, LS_BEAM_LAST, LS_BEAM_STRONGEST = 1, 2, 4   # ls_trace_scene_beams: which echoes of a beam are returned


class BeamModel(C.Structure):
    """ls_beam_model: `pattern` float32 (S, 3) records (a, b, k) -- kept alive by this object --, the LS_BEAM_* mask of the returns,
    the member count that makes an echo detectable, the range gap (metres) that separates two echoes"""
    _fields_ = [("pattern", C.POINTER(C.c_float)), ("n_samples", C.c_uint32), ("returns", C.c_uint32), ("min_count", C.c_uint32),
                ("echo_separation", C.c_float), ("reserved", C.c_uint32 * 4)]

    def __init__(self, pattern=((0.0, 0.0, 1.0),), returns: int = LS_BEAM_FIRST, min_count: int = 1, echo_separation: float = float("inf")):
        super().__init__()
        self._pattern = np.ascontiguousarray(pattern, np.float32).reshape(-1, 3)
        self.pattern = self._pattern.ctypes.data_as(C.POINTER(C.c_float))
        self.n_samples, self.returns, self.min_count, self.echo_separation = self._pattern.shape[0], returns, min_count, echo_separation

    @property
    def n_returns(self) -> int:
        return bin(self.returns & 7).count("1")


class GeometryMotion(C.Structure):
    """ls_geometry_motion: the geomID of a geometry that moves during the turn and its table of H records [Q | c] (an address:
    device memory for the device call, host memory for the host variant)"""
    _fields_ = [("geom", C.c_uint32), ("reserved", C.c_uint32), ("col_motion", C.c_void_p)]


class GeometryTwist(C.Structure):
    """ls_geometry_twist: the geomID of a moving geometry and its table of H twist records [w | u] (an address: device memory for
    the device call, host memory for the host variant)"""
    _fields_ = [("geom", C.c_uint32), ("reserved", C.c_uint32), ("col_twist", C.c_void_p)]


# ls_format_cloud: the sources of a cloud field, the sensor_msgs::PointField datatypes, the limits and the flag
(LS_FIELD_X, LS_FIELD_Y, LS_FIELD_Z, LS_FIELD_INTENSITY, LS_FIELD_RANGE, LS_FIELD_TIME, LS_FIELD_RING, LS_FIELD_COLUMN, LS_FIELD_RAY,
 LS_FIELD_GEOM, LS_FIELD_PRIM, LS_FIELD_ECHO) = range(1, 13)
LS_INT8, LS_UINT8, LS_INT16, LS_UINT16, LS_INT32, LS_UINT32, LS_FLOAT32, LS_FLOAT64 = range(1, 9)
LS_CLOUD_MAX_FIELDS, LS_CLOUD_MAX_STEP, LS_CLOUD_ORGANIZED = 16, 128, 1
# name -> source of ls_cloud_format_from_point_fields (message.pointFields[].name of the reference's sensor config)
CLOUD_FIELD_NAMES = {"x": LS_FIELD_X, "y": LS_FIELD_Y, "z": LS_FIELD_Z, "intensity": LS_FIELD_INTENSITY, "ring": LS_FIELD_RING,
                     "channel": LS_FIELD_RING, "time": LS_FIELD_TIME, "t": LS_FIELD_TIME, "timestamp": LS_FIELD_TIME,
                     "range": LS_FIELD_RANGE, "distance": LS_FIELD_RANGE, "label": LS_FIELD_GEOM, "geom": LS_FIELD_GEOM,
                     "prim": LS_FIELD_PRIM, "ray": LS_FIELD_RAY, "column": LS_FIELD_COLUMN, "echo": LS_FIELD_ECHO,
                     "return_type": LS_FIELD_ECHO}


class CloudField(C.Structure):
    _fields_ = [("source", C.c_uint8), ("datatype", C.c_uint8), ("offset", C.c_uint16), ("scale", C.c_float), ("bias", C.c_float)]


class CloudFormat(C.Structure):
    """ls_cloud_format: `fields` tuples (source, datatype, offset[, scale, bias]) -- LS_FIELD_*, a PointField datatype 1..8, a byte
    offset, scale 1 and bias 0 by default -- in records of `point_step` bytes; organized: the V x H image of layer `layer` instead
    of record after record.  Nothing is checked here: cloud_format_check and the calls do that."""
    _fields_ = [("point_step", C.c_uint32), ("n_fields", C.c_uint32), ("flags", C.c_uint32), ("layer", C.c_uint32),
                ("fields", CloudField * LS_CLOUD_MAX_FIELDS)]

    def __init__(self, point_step: int = 0, fields=(), organized: bool = False, layer: int = 0):
        super().__init__()
        fields = list(fields)
        if len(fields) > LS_CLOUD_MAX_FIELDS:
            raise ValueError("ls_cloud_format holds at most LS_CLOUD_MAX_FIELDS fields")
        self.point_step, self.n_fields, self.flags, self.layer = point_step, len(fields), LS_CLOUD_ORGANIZED if organized else 0, layer
        for f, t in zip(self.fields, fields):
            f.source, f.datatype, f.offset = t[0], t[1], t[2]
            f.scale, f.bias = (t[3], t[4]) if len(t) > 3 else (1.0, 0.0)

    @property
    def organized(self) -> bool:
        return bool(self.flags & LS_CLOUD_ORGANIZED)


class ReturnModel(C.Structure):
    """ls_return_model (64 bytes): the defaults change nothing -- no gate, no floor, no saturation, no noise, no drop-out, the
    frame's constant intensity 64.0"""
    _fields_ = [("range_min", C.c_float), ("range_max", C.c_float), ("intensity_scale", C.c_float), ("ref_range", C.c_float),
                ("intensity_floor", C.c_float), ("intensity_max", C.c_float), ("noise_sigma0", C.c_float), ("noise_sigma1", C.c_float),
                ("dropout", C.c_float), ("seed", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 5)]

    def __init__(self, **kw):
        super().__init__()
        self.range_max = self.intensity_max = float("inf")
        self.intensity_scale = 64.0
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"ls_return_model has no field {k}")
            setattr(self, k, v)


class Frame(C.Structure):
    _fields_ = [("points32", C.POINTER(C.c_uint8)), ("hits", C.c_void_p), ("n_points", C.c_uint32),
                ("n_rays", C.c_uint32), ("frame", C.c_uint32), ("d_points32", C.c_void_p),
                ("d_hits", C.c_void_p), ("d_n_points", C.c_void_p), ("compact16", C.c_void_p)]


HIT_DTYPE = np.dtype([("ray", "<u4"), ("geom", "<u4"), ("prim", "<u4"), ("t", "<f4")])
# ls_closest_points: a query point (sensor frame) with the largest distance of interest, and its answer
POINT_QUERY_DTYPE = np.dtype([("point", "<f4", 3), ("radius", "<f4")])
CLOSEST_DTYPE = np.dtype([("q", "<f4", 3), ("dist", "<f4"), ("geom", "<u4"), ("prim", "<u4"), ("index", "<u4"), ("pad", "<u4")])
# ls_hit_attributes: surface attributes of one ls_hit (flags bit 0: valid; an invalid record is zeros but for `ray`)
HIT_ATTR_DTYPE = np.dtype([("n", "<f4", 3), ("cos_inc", "<f4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4"), ("flags", "<u4"),
                           ("p", "<f4", 3), ("ray", "<u4")])
# ls_hit_velocities: the surface's velocity, the range rate and the velocity of the sensor's origin at one ls_hit (flags bit 0: valid;
# an invalid record is zeros)
HIT_VELOCITY_DTYPE = np.dtype([("v_s", "<f4", 3), ("radial", "<f4"), ("v_o", "<f4", 3), ("flags", "<u4")])
# ls_object_labels: what one geometry got of a frame's hit records (flags bit 0: the geomID names a committed geometry; n_hits = 0:
# t_min / lo = +inf, t_max / hi = -inf, the rays 0xFFFFFFFF)
LS_LABEL_FOOTPRINT = 1
OBJECT_LABEL_DTYPE = np.dtype([("n_hits", "<u4"), ("n_alone", "<u4"), ("t_min", "<f4"), ("ray_min", "<u4"), ("t_max", "<f4"), ("ray_max", "<u4"),
                               ("lo", "<f4", 3), ("hi", "<f4", 3), ("flags", "<u4"), ("reserved", "<u4", 3)])
# ls_occupancy_grid: per cell of a voxel grid the rays that crossed it (n_free) and the returns that fell in it (n_occ)
LS_OCC_CARVE_MISSES, LS_OCC_ACCUMULATE = 1, 2
OCCUPANCY_MAX_DIM, OCCUPANCY_MAX_CELLS = 2048, 1 << 27


class OccupancyGridDesc(C.Structure):
    """ls_occupancy_grid_desc (48 bytes): cell (x, y, z) of the grid is word pair (z * ny + y) * nx + x"""
    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float), ("dims", C.c_uint32 * 3), ("flags", C.c_uint32),
                ("min_range", C.c_float), ("max_range", C.c_float), ("reserved", C.c_uint32 * 2)]

    @classmethod
    def make(cls, origin, cell, dims, flags=0, min_range=0.0, max_range=1e4):
        d = cls()
        d.origin = (C.c_float * 3)(*[float(x) for x in origin])
        d.cell = float(cell)
        d.dims = (C.c_uint32 * 3)(*[int(x) for x in dims])
        d.flags, d.min_range, d.max_range = int(flags), float(min_range), float(max_range)
        return d


# ls_scene_grid: per cell of a voxel grid the triangles of the committed scene that overlap it
LS_SCENE_GRID_ACCUMULATE = 1


class SceneGridDesc(C.Structure):
    """ls_scene_grid_desc (32 bytes): cell (x, y, z) of the grid is word (z * ny + y) * nx + x, ls_occupancy_grid's order"""
    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float), ("dims", C.c_uint32 * 3), ("flags", C.c_uint32)]

    @classmethod
    def make(cls, origin, cell, dims, flags=0):
        d = cls()
        d.origin = (C.c_float * 3)(*[float(x) for x in origin])
        d.cell = float(cell)
        d.dims = (C.c_uint32 * 3)(*[int(x) for x in dims])
        d.flags = int(flags)
        return d


# ls_scene_distance_grid: per cell of a voxel grid the distance from its centre to the nearest surface of the committed scene within
# trunc; a record read as one 64-bit word is (bits(dist) << 32) | geom, and a cell with no surface in reach holds DIST_GRID_REST
LS_DIST_GRID_ACCUMULATE = 1
DIST_GRID_DTYPE = np.dtype([("geom", "<u4"), ("dist", "<f4")])
DIST_GRID_REST = 0x7F800000FFFFFFFF


class DistanceGridDesc(C.Structure):
    """ls_distance_grid_desc (48 bytes): cell (x, y, z) of the grid is record (z * ny + y) * nx + x, the other two grids' order"""
    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float), ("dims", C.c_uint32 * 3), ("flags", C.c_uint32), ("trunc", C.c_float),
                ("reserved", C.c_uint32 * 3)]

    @classmethod
    def make(cls, origin, cell, dims, flags=0, trunc=0.0):
        d = cls()
        d.origin = (C.c_float * 3)(*[float(x) for x in origin])
        d.cell = float(cell)
        d.dims = (C.c_uint32 * 3)(*[int(x) for x in dims])
        d.flags, d.trunc = int(flags), float(trunc)
        return d


# ls_sample_surface: points drawn from the surface of the committed scene in proportion to area; the call's info says what the
# weights add up to: the selection's area is weight_total * 2 ** exponent, up to the weights' flooring
SURFACE_SAMPLE_DTYPE = np.dtype([("p", "<f4", 3), ("geom", "<u4"), ("n", "<f4", 3), ("prim", "<u4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4"),
                                 ("flags", "<u4")])
SURFACE_INFO_DTYPE = np.dtype([("weight_total", "<u8"), ("exponent", "<i4"), ("n_weighted", "<u4")])


class SurfaceSampleDesc(C.Structure):
    """ls_surface_sample_desc (32 bytes): samples first_sample .. first_sample + n_samples - 1 of the sequence `seed` names"""
    _fields_ = [("first_sample", C.c_uint64), ("n_samples", C.c_uint32), ("seed", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]

    @classmethod
    def make(cls, n_samples, seed=0, first_sample=0, flags=0):
        d = cls()
        d.first_sample, d.n_samples, d.seed, d.flags = int(first_sample) & 0xFFFFFFFFFFFFFFFF, int(n_samples), int(seed) & 0xFFFFFFFF, int(flags)
        return d


# ls_cloud_nearest: per query the nearest point of a cloud within a radius; index 0xFFFFFFFF and +inf distances when nothing was found
# (flags bit 0: found, bit 1: the query was outside the domain); the call's info counts
LS_CLOUD_NEAREST_SKIP_SAME_INDEX = 1
CLOUD_NEAREST_DTYPE = np.dtype([("index", "<u4"), ("dist2", "<f4"), ("dist", "<f4"), ("flags", "<u4")])
CLOUD_NEAREST_INFO_DTYPE = np.dtype([("n_found", "<u4"), ("n_query_outside", "<u4"), ("n_cloud_indexed", "<u4"), ("reserved", "<u4")])


class CloudNearestDesc(C.Structure):
    """ls_cloud_nearest_desc (32 bytes): the radius and the bytes from one point to the next in the cloud and in the queries"""
    _fields_ = [("radius", C.c_float), ("flags", C.c_uint32), ("cloud_stride", C.c_uint32), ("query_stride", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]

    @classmethod
    def make(cls, radius, cloud_stride=12, query_stride=12, flags=0):
        d = cls()
        d.radius, d.flags, d.cloud_stride, d.query_stride = float(radius), int(flags), int(cloud_stride), int(query_stride)
        return d


NODE_DTYPE = np.dtype([("llo", "<f4", 3), ("left", "<u4"), ("lhi", "<f4", 3), ("right", "<u4"),
                       ("rlo", "<f4", 3), ("pad0", "<u4"), ("rhi", "<f4", 3), ("pad1", "<u4")])
LEAF_BIT = 0x80000000
TRI_DTYPE = np.dtype([("v0", "<f4", 3), ("gid", "<u4"), ("e1", "<f4", 3), ("NgC", "<f4"), ("e2", "<f4", 3),
                      ("pad", "<u4")])
# ls_debug_download_hierarchy: a four-wide node (lo[c] = slot c's box minimum and reference, hi[c] = its maximum and 0) and an
# instanced hierarchy's triangle record (the corners as uploaded, the triangle's index in its geometry)
WIDE_DTYPE = np.dtype([("lo", "<f4", (4, 4)), ("hi", "<f4", (4, 4))])
MESH_TRI_DTYPE = np.dtype([("v0", "<f4", 3), ("gid", "<u4"), ("v1", "<f4", 3), ("pad0", "<u4"), ("v2", "<f4", 3), ("pad1", "<u4")])

_lib = None


class LidarShooterHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the HIP library; fails loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (soname
    # libamdhip64.so.7, the one this library needs).  Importing torch first makes the loader bind
    # this library to that copy; loading /opt/rocm's copy first and torch's afterwards would put
    # two HIP runtimes in the process and the second one finds no GPU.
    if "torch" not in sys.modules and os.environ.get("LS_HIP_STANDALONE") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise LidarShooterHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C lidarshooter_amd/csrc). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, u32, i32, f32p, u32p = C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    L.ls_abi_version.restype = i32
    if L.ls_abi_version() != ABI_VERSION:   # (a stale .so next to a newer binding, or the other way round)
        raise LidarShooterHipError(f"{LIB_PATH} speaks ABI {L.ls_abi_version()}, this binding {ABI_VERSION}: rebuild (make -C lidarshooter_amd/csrc)")
    L.ls_source_hash.argtypes = []
    L.ls_source_hash.restype = C.c_char_p
    L.ls_tracer_create.argtypes = [C.POINTER(SensorDesc), i32, C.POINTER(vp)]
    L.ls_tracer_create_tables.argtypes = [C.POINTER(SensorTables), i32, C.POINTER(vp)]
    L.ls_tracer_set_sensor.argtypes = [vp, C.POINTER(SensorDesc)]
    L.ls_tracer_set_sensor_tables.argtypes = [vp, C.POINTER(SensorTables)]
    L.ls_affine_from_components.argtypes = [f32p, f32p, f32p]
    L.ls_affine_from_components.restype = None
    L.ls_expand_points.argtypes = [vp, vp, u32]
    L.ls_parallel_copy.argtypes = [vp, vp, C.c_uint64]
    L.ls_get_info.argtypes = [vp, i32]
    L.ls_get_info.restype = C.c_long
    L.ls_tracer_destroy.argtypes = [vp]
    L.ls_tracer_destroy.restype = None
    L.ls_add_geometry.argtypes = [vp, C.c_char_p, i32, i32, i32]
    L.ls_remove_geometry.argtypes = [vp, C.c_char_p]
    L.ls_update_geometry.argtypes = [vp, C.c_char_p, f32p, vp, u32, vp]
    L.ls_update_geometry_components.argtypes = [vp, C.c_char_p, f32p, f32p, vp, u32, vp]
    L.ls_update_geometry_device.argtypes = [vp, C.c_char_p, f32p, vp, u32, vp]
    L.ls_update_geometry_device_shared.argtypes = [vp, C.c_char_p, f32p, vp, u32, vp]
    L.ls_update_geometry_transform.argtypes = [vp, C.c_char_p, f32p]
    L.ls_commit_scene.argtypes = [vp]
    L.ls_trace_scene.argtypes = [vp, u32, C.POINTER(Frame)]
    L.ls_trace_scene_async.argtypes = [vp, u32, C.POINTER(Frame)]
    L.ls_trace_scene_begin.argtypes = [vp, u32, u32p]
    L.ls_trace_scene_expand.argtypes = [vp, vp]
    L.ls_geometry_count.argtypes = [vp]
    L.ls_geometry_count.restype = C.c_long
    L.ls_geometry_id.argtypes = [vp, C.c_char_p]
    L.ls_vertex_count.argtypes = [vp, C.c_char_p]
    L.ls_vertex_count.restype = C.c_long
    L.ls_element_count.argtypes = [vp, C.c_char_p]
    L.ls_element_count.restype = C.c_long
    L.ls_total_rays.argtypes = [vp]
    L.ls_total_rays.restype = u32
    L.ls_total_channels.argtypes = [vp]
    L.ls_total_channels.restype = u32
    L.ls_last_error.argtypes = [vp]
    L.ls_last_error.restype = C.c_char_p
    L.ls_tracer_set_shard.argtypes = [vp, u32, u32]
    L.ls_tracer_set_stream.argtypes = [vp, vp]
    L.ls_tracer_synchronize.argtypes = [vp]
    L.ls_tracer_set_output_buffers.argtypes = [vp, vp, vp, vp, u32]
    L.ls_tracer_set_hit_buffers.argtypes = [vp, vp, vp, u32]
    L.ls_expand_gathered_hits.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.ls_expand_gathered_hits_on.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp]
    L.ls_cloud_to_world.argtypes = [vp, f32p, f32p, vp, vp, vp, vp, vp, u32]
    L.ls_tracer_flush.argtypes = [vp]
    L.ls_tracer_order_after_last_frame.argtypes = [vp, vp]
    L.ls_tracer_wait_event.argtypes = [vp, vp]
    L.ls_tracer_next_frame_waits.argtypes = [vp, vp]
    L.ls_frame_graph_begin.argtypes = [vp, C.c_uint64]
    L.ls_frame_graph_stream.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    L.ls_frame_graph_end.argtypes = [vp]
    L.ls_frame_graph_reset.argtypes = [vp]
    L.ls_tracer_set_option.argtypes = [vp, i32, i32]
    L.ls_get_timings.argtypes = [vp, f32p]
    L.ls_get_visit_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.ls_generate_rays.argtypes = [vp, vp, vp, vp]
    L.ls_generate_rays_aos.argtypes = [vp, vp, vp]
    L.ls_trace_rays.argtypes = [vp, vp, vp, u32, vp]
    L.ls_trace_rays_host.argtypes = [vp, vp, u32, vp]
    L.ls_occluded_rays.argtypes = [vp, vp, vp, u32, vp]
    L.ls_occluded_rays_host.argtypes = [vp, vp, u32, vp]
    L.ls_closest_points.argtypes = [vp, vp, vp, u32, vp]
    L.ls_closest_points_host.argtypes = [vp, vp, u32, vp]
    L.ls_debug_closest_on_triangle.argtypes = [f32p, f32p, f32p, f32p, f32p, f32p]
    L.ls_hit_attributes.argtypes = [vp, vp, vp, u32, vp, vp, u32, vp]
    L.ls_hit_attributes_host.argtypes = [vp, vp, u32, vp, u32, vp]
    L.ls_debug_hit_attributes_on_triangle.argtypes = [f32p, f32p, f32p, f32p, f32p, f32p, f32p]
    L.ls_apply_return_model.argtypes = [vp, vp, C.POINTER(ReturnModel), u32, vp, u32, vp, vp, u32, vp, u32, vp, vp, vp]
    L.ls_apply_return_model_host.argtypes = [vp, C.POINTER(ReturnModel), u32, vp, u32, vp, u32, vp, u32, vp, vp, u32p]
    L.ls_debug_philox4x32.argtypes = [u32p, u32p, u32p]
    L.ls_debug_return_model.argtypes = [C.POINTER(ReturnModel), u32, u32, C.c_float, C.c_float, C.c_float, C.c_float, f32p, f32p]
    L.ls_trace_scene_sweep.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, u32, vp]
    L.ls_trace_scene_sweep_host.argtypes = [vp, vp, u32, u32, vp, vp, u32p, u32, vp]
    L.ls_sweep_poses_constant_twist.argtypes = [f32p, f32p, C.c_double, C.c_double, u32, f32p]
    L.ls_debug_sweep_ray.argtypes = [f32p, f32p, f32p]
    L.ls_trace_scene_beams.argtypes = [vp, vp, C.POINTER(BeamModel), vp, vp, vp, vp, u32]
    L.ls_trace_scene_beams_host.argtypes = [vp, C.POINTER(BeamModel), vp, vp, vp, u32p, u32]
    L.ls_beam_pattern_rings.argtypes = [C.c_float, C.c_float, u32, u32, f32p]
    L.ls_debug_beam_ray.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, f32p, f32p]
    L.ls_debug_beam_echoes.argtypes = [C.POINTER(BeamModel), f32p, vp, u32p, u32p]
    L.ls_debug_beam_model_check.argtypes = [C.POINTER(BeamModel), u32, u32]
    L.ls_trace_scene_beams_sweep.argtypes = [vp, vp, C.POINTER(BeamModel), u32p, u32, vp, u32, u32, vp, vp, vp, vp, u32]
    L.ls_trace_scene_beams_sweep_host.argtypes = [vp, C.POINTER(BeamModel), u32p, u32, vp, u32, u32, vp, vp, vp, u32p, u32]
    L.ls_beam_weights_gaussian.argtypes = [f32p, u32, C.c_float, C.c_float, u32p]
    L.ls_debug_beam_sweep_ray.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, f32p, f32p, f32p]
    L.ls_debug_beam_echoes_weighted.argtypes = [C.POINTER(BeamModel), u32p, u32, f32p, vp, u32p, u32p]
    L.ls_debug_beam_sweep_check.argtypes = [C.POINTER(BeamModel), u32p, u32, u32]
    L.ls_trace_scene_sweep_moving.argtypes = [vp, vp, vp, u32, C.POINTER(GeometryMotion), u32, u32, vp, vp, vp, u32]
    L.ls_trace_scene_sweep_moving_host.argtypes = [vp, vp, u32, C.POINTER(GeometryMotion), u32, u32, vp, vp, u32p, u32]
    L.ls_motion_constant_twist.argtypes = [f32p, f32p, f32p, C.c_double, C.c_double, u32, f32p]
    L.ls_debug_motion_ray.argtypes = [f32p, f32p, f32p]
    L.ls_hit_attributes_moving.argtypes = [vp, vp, vp, u32, C.POINTER(GeometryMotion), u32, u32, vp, vp, u32, vp]
    L.ls_hit_attributes_moving_host.argtypes = [vp, vp, u32, C.POINTER(GeometryMotion), u32, u32, vp, u32, vp]
    L.ls_apply_return_model_moving.argtypes = [vp, vp, C.POINTER(ReturnModel), u32, vp, u32, C.POINTER(GeometryMotion), u32, u32, vp, vp, u32, vp, u32,
                                               vp, vp, vp]
    L.ls_apply_return_model_moving_host.argtypes = [vp, C.POINTER(ReturnModel), u32, vp, u32, C.POINTER(GeometryMotion), u32, u32, vp, u32, vp, u32,
                                                    vp, vp, u32p]
    L.ls_debug_motion_normal.argtypes = [f32p, f32p, f32p]
    L.ls_hit_velocities.argtypes = [vp, vp, vp, u32, C.POINTER(GeometryMotion), u32, vp, C.POINTER(GeometryTwist), u32, u32, vp, vp, u32, vp, vp]
    L.ls_hit_velocities_host.argtypes = [vp, vp, u32, C.POINTER(GeometryMotion), u32, vp, C.POINTER(GeometryTwist), u32, u32, vp, u32, vp, vp]
    L.ls_twist_table_constant.argtypes = [f32p, f32p, f32p, C.c_double, C.c_double, u32, f32p]
    L.ls_object_labels.argtypes = [vp, vp, u32, vp, u32, vp, vp, u32, vp, u32]
    L.ls_object_labels_host.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32]
    L.ls_occupancy_grid.argtypes = [vp, vp, C.POINTER(OccupancyGridDesc), vp, vp, u32, vp, vp, u32, vp, vp]
    L.ls_occupancy_grid_host.argtypes = [vp, C.POINTER(OccupancyGridDesc), vp, vp, u32, vp, u32, vp, vp]
    L.ls_occupancy_grid_check.argtypes = [C.POINTER(OccupancyGridDesc)]
    L.ls_debug_voxel_walk.argtypes = [C.POINTER(OccupancyGridDesc), vp, vp, C.c_float, vp, u32, u32p, u32p]
    L.ls_scene_grid.argtypes = [vp, vp, C.POINTER(SceneGridDesc), vp, vp, u32, vp, vp]
    L.ls_scene_grid_host.argtypes = [vp, C.POINTER(SceneGridDesc), vp, vp, u32, vp, vp]
    L.ls_scene_grid_check.argtypes = [C.POINTER(SceneGridDesc)]
    L.ls_debug_scene_grid_triangle.argtypes = [C.POINTER(SceneGridDesc), vp, vp, u32, u32p]
    L.ls_debug_scene_grid_queued.argtypes = [vp, u32p]
    L.ls_scene_distance_grid.argtypes = [vp, vp, C.POINTER(DistanceGridDesc), vp, vp, u32, vp]
    L.ls_scene_distance_grid_host.argtypes = [vp, C.POINTER(DistanceGridDesc), vp, vp, u32, vp]
    L.ls_scene_distance_grid_check.argtypes = [C.POINTER(DistanceGridDesc)]
    L.ls_debug_distance_grid_triangle.argtypes = [C.POINTER(DistanceGridDesc), vp, vp, vp, u32, u32p]
    L.ls_debug_distance_grid_queued.argtypes = [vp, u32p]
    L.ls_sample_surface.argtypes = [vp, vp, C.POINTER(SurfaceSampleDesc), vp, vp, u32, vp, vp]
    L.ls_sample_surface_host.argtypes = [vp, C.POINTER(SurfaceSampleDesc), vp, vp, u32, vp, vp]
    L.ls_surface_sample_check.argtypes = [C.POINTER(SurfaceSampleDesc)]
    L.ls_debug_surface_weights.argtypes = [vp, u32, vp, vp, vp, vp]
    L.ls_debug_surface_pick.argtypes = [vp, u32, C.c_uint64, u32p]
    L.ls_debug_surface_point.argtypes = [vp, u32, u32, vp]
    L.ls_cloud_nearest.argtypes = [vp, vp, C.POINTER(CloudNearestDesc), vp, vp, u32, vp, u32, vp, vp]
    L.ls_cloud_nearest_host.argtypes = [vp, C.POINTER(CloudNearestDesc), vp, vp, u32, vp, u32, vp, vp]
    L.ls_cloud_nearest_check.argtypes = [C.POINTER(CloudNearestDesc)]
    L.ls_debug_cloud_cell.argtypes = [C.c_float, vp, u32, vp, vp]
    L.ls_debug_cloud_bucket.argtypes = [vp, u32]
    L.ls_debug_cloud_bucket.restype = u32
    L.ls_debug_hit_velocity.argtypes = [f32p, C.c_float, f32p, f32p, f32p]
    L.ls_format_cloud.argtypes = [vp, vp, C.POINTER(CloudFormat), vp, vp, vp, vp, u32, vp, vp, vp]
    L.ls_format_cloud_host.argtypes = [vp, C.POINTER(CloudFormat), vp, vp, vp, u32, vp, vp, vp]
    L.ls_cloud_format_check.argtypes = [C.POINTER(CloudFormat)]
    L.ls_cloud_format_from_point_fields.argtypes = [C.POINTER(C.c_char_p), u32p, C.POINTER(C.c_uint8), u32p, u32, u32, C.POINTER(CloudFormat)]
    L.ls_column_times.argtypes = [C.c_double, C.c_double, u32, f32p]
    L.ls_debug_band_map_fit.argtypes = [f32p, u32, f32p]
    L.ls_debug_band_guess.argtypes = [f32p, u32, C.c_float, u32p]
    L.ls_debug_tracer_band_map.argtypes = [vp, f32p]
    L.ls_debug_force_group_cull.argtypes = [vp, i32]
    L.ls_debug_download_cull.argtypes = [vp, u32, u32p, vp, vp, vp]
    L.ls_debug_cull_survivors.argtypes = [vp, u32, vp, u32, u32p, u32p]
    L.ls_debug_cull_tables.argtypes = [vp, vp, vp, vp, C.POINTER(i32)]
    L.ls_debug_chan_query.argtypes = [vp, vp, u32, vp]
    L.ls_debug_format_record.argtypes = [C.POINTER(CloudFormat), vp, vp, u32, C.c_float, C.c_float, u32, u32, u32, vp]
    L.ls_geometry_type.argtypes = [vp, C.c_char_p]
    L.ls_debug_dense_hits.argtypes = [vp, f32p, u32p]
    L.ls_debug_trace_bruteforce.argtypes = [vp, f32p, u32p]
    L.ls_debug_scene_size.argtypes = [vp, u32p, u32p, u32p, u32p]
    L.ls_debug_download_scene.argtypes = [vp, vp, vp]
    L.ls_debug_download_bvh.argtypes = [vp, vp, vp]
    L.ls_debug_download_hierarchy.argtypes = [vp, u32, u32p, u32p, vp, vp, vp]
    L.ls_debug_sort_pairs.argtypes = [vp, vp, vp, u32]
    L.ls_debug_expand_hits.argtypes = [vp, vp, u32, vp, vp, vp, u32, u32]
    _lib = L
    return L


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


IDENTITY_AFFINE = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def _floats(a, n):
    return (C.c_float * n)(*[float(x) for x in np.asarray(a, np.float32).reshape(n)])


def _sensor_desc(vert, h_begin, h_end, h_count, Rinv, t) -> SensorDesc:
    """ls_sensor_desc over `vert`, a contiguous float32 array the caller keeps alive"""
    sd = SensorDesc()
    sd.vertical_deg, sd.n_vertical = _f32p(vert), vert.shape[0]
    sd.h_begin, sd.h_end, sd.h_count = float(h_begin), float(h_end), int(h_count)
    sd.Rinv, sd.t = _floats(Rinv, 9), _floats(t, 3)
    return sd


def _sensor_tables(tabs, h_begin_deg, h_step_deg, Rinv, t) -> SensorTables:
    """ls_sensor_tables over `tabs` (sin_theta, cos_theta, elevation_deg, sin_phi, cos_phi), contiguous float32 arrays the caller
    keeps alive"""
    st = SensorTables()
    st.sin_theta, st.cos_theta, st.elevation_deg, st.sin_phi, st.cos_phi = [_f32p(a) for a in tabs]
    st.n_vertical, st.h_count = tabs[0].shape[0], tabs[3].shape[0]
    st.h_begin_deg, st.h_step_deg = float(h_begin_deg), float(h_step_deg)
    st.Rinv, st.t = _floats(Rinv, 9), _floats(t, 3)
    return st


class _Outputs:
    """The outputs of a host-memory call that counts its records: of points uint8 (n, 32), hits HIT_DTYPE (n,) and echo words uint32
    (n,), in this order, those asked for with True (None stands for one that is not); `k` takes the count."""
    _KINDS = (((32,), np.uint8), ((), HIT_DTYPE), ((), np.uint32))

    def __init__(self, n: int, *wanted: bool):
        self.arrays = tuple(np.zeros((n,) + shape, dtype) if w else None for w, (shape, dtype) in zip(wanted, self._KINDS))
        self.ptrs = tuple(a.ctypes.data if a is not None and n else None for a in self.arrays)
        self.k = C.c_uint32(0)

    def first(self, k: int) -> tuple:
        return tuple(None if a is None else a[:k].copy() for a in self.arrays)


class Tracer:
    """Thin object wrapper over an ls_tracer handle; method names follow ITracer."""

    def __init__(self, vertical_deg, h_begin, h_end, h_count, Rinv, t, device: int = 0):
        self.L = load()
        self._vert = np.ascontiguousarray(vertical_deg, np.float32)
        sd = _sensor_desc(self._vert, h_begin, h_end, h_count, Rinv, t)
        self._raster(sd.n_vertical, h_count)
        h = C.c_void_p()
        rc = self.L.ls_tracer_create(C.byref(sd), device, C.byref(h))
        if rc != 0:
            raise LidarShooterHipError(f"ls_tracer_create failed with status {rc} (no HIP device / bad sensor)")
        self.h = h

    @classmethod
    def fromTables(cls, sin_theta, cos_theta, elevation_deg, sin_phi, cos_phi, h_begin_deg, h_step_deg, Rinv, t, device: int = 0):
        """ls_tracer_create_tables: the sensor as ray-direction factor tables (what integration/HipTracer.hpp probes out of a live
        LidarDevice); raises when the library refuses them (elevation_deg / h_begin_deg / h_step_deg off their own tables)"""
        self = cls.__new__(cls)
        self.L = load()
        self._tabs = [np.ascontiguousarray(a, np.float32) for a in (sin_theta, cos_theta, elevation_deg, sin_phi, cos_phi)]
        st = _sensor_tables(self._tabs, h_begin_deg, h_step_deg, Rinv, t)
        self._raster(st.n_vertical, st.h_count)
        h = C.c_void_p()
        rc = self.L.ls_tracer_create_tables(C.byref(st), device, C.byref(h))
        if rc != 0:
            raise LidarShooterHipError(f"ls_tracer_create_tables failed with status {rc} (no HIP device / tables refused)")
        self.h = h
        return self

    def _raster(self, V, H):
        self.V, self.H = int(V), int(H)
        self.az0, self.naz = 0, self.H

    def setSensorTables(self, sin_theta, cos_theta, elevation_deg, sin_phi, cos_phi, h_begin_deg, h_step_deg, Rinv, t):
        """ls_tracer_set_sensor_tables: another sensor, given as factor tables, for this handle (its geometries stay)"""
        tabs = [np.ascontiguousarray(a, np.float32) for a in (sin_theta, cos_theta, elevation_deg, sin_phi, cos_phi)]
        st = _sensor_tables(tabs, h_begin_deg, h_step_deg, Rinv, t)
        self._check(self.L.ls_tracer_set_sensor_tables(self.h, C.byref(st)), "ls_tracer_set_sensor_tables")
        self._tabs = tabs
        self._raster(st.n_vertical, st.h_count)

    def setSensor(self, vertical_deg, h_begin, h_end, h_count, Rinv, t):
        """ITracer::setSensorConfig: another sensor for this handle, its geometries stay (ls_tracer_set_sensor)"""
        self._vert = np.ascontiguousarray(vertical_deg, np.float32)
        sd = _sensor_desc(self._vert, h_begin, h_end, h_count, Rinv, t)
        self._check(self.L.ls_tracer_set_sensor(self.h, C.byref(sd)), "ls_tracer_set_sensor")
        self._raster(sd.n_vertical, h_count)

    # ---- lifetime
    def close(self):
        if getattr(self, "h", None):
            self.L.ls_tracer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0 and rc != -1:
            raise LidarShooterHipError(f"{what}: status {rc}: {self.last_error()}")
        return rc

    def last_error(self) -> str:
        return (self.L.ls_last_error(self.h) or b"").decode()

    # ---- ITracer surface
    def addGeometry(self, name: str, n_vertices: int, n_elements: int, geometry_type: int = 0) -> int:
        gid = self.L.ls_add_geometry(self.h, name.encode(), geometry_type, int(n_vertices), int(n_elements))
        if gid >= 0:
            self.__dict__.setdefault("_geom_ids", {})[name] = int(gid)   # (objectLabels' default n_labels)
        return gid

    def removeGeometry(self, name: str) -> int:
        rc = self.L.ls_remove_geometry(self.h, name.encode())
        if rc >= 0:
            self.__dict__.setdefault("_geom_ids", {}).pop(name, None)
        return rc

    def updateGeometry(self, name: str, affine, verts: np.ndarray, tris: np.ndarray | None, stride: int | None = None):
        A = np.ascontiguousarray(affine, np.float32).reshape(12)
        verts = np.ascontiguousarray(verts)
        if stride is None:
            verts = np.ascontiguousarray(verts, np.float32)
            stride = 12
        tp = None
        if tris is not None:   # uint32[n,3] triangles, or [n,4] quads for a geometry added with geometry_type=1
            tris = np.ascontiguousarray(tris, np.uint32)
            tp = tris.ctypes.data
        return self._check(self.L.ls_update_geometry(self.h, name.encode(), _f32p(A), verts.ctypes.data, stride, tp),
                           "ls_update_geometry")

    def updateGeometryComponents(self, name: str, lin, ang, verts: np.ndarray, tris: np.ndarray | None):
        lin = np.ascontiguousarray(lin, np.float32)
        ang = np.ascontiguousarray(ang, np.float32)
        verts = np.ascontiguousarray(verts, np.float32)
        tp = None
        if tris is not None:
            tris = np.ascontiguousarray(tris, np.uint32)
            tp = tris.ctypes.data
        return self._check(self.L.ls_update_geometry_components(self.h, name.encode(), _f32p(lin), _f32p(ang),
                                                                verts.ctypes.data, 12, tp),
                           "ls_update_geometry_components")

    def updateGeometryDevice(self, name: str, affine, d_verts: int, stride: int, d_tris: int | None):
        A = np.ascontiguousarray(affine, np.float32).reshape(12)
        return self._check(self.L.ls_update_geometry_device(self.h, name.encode(), _f32p(A), d_verts, stride, d_tris),
                           "ls_update_geometry_device")

    def updateGeometryDeviceShared(self, name: str, affine, d_verts: int, stride: int, d_tris: int | None):
        A = np.ascontiguousarray(affine, np.float32).reshape(12)
        return self._check(self.L.ls_update_geometry_device_shared(self.h, name.encode(), _f32p(A), d_verts, stride, d_tris),
                           "ls_update_geometry_device_shared")

    def updateGeometryTransform(self, name: str, affine):
        A = np.ascontiguousarray(affine, np.float32).reshape(12)
        return self._check(self.L.ls_update_geometry_transform(self.h, name.encode(), _f32p(A)),
                           "ls_update_geometry_transform")

    def commitScene(self) -> int:
        return self._check(self.L.ls_commit_scene(self.h), "ls_commit_scene")

    def traceScene(self, frame_index: int = 0):
        """-> (rc, points uint8[n,32], hits HIT_DTYPE[n]) copied out of the handle's pinned buffers."""
        fr = Frame()
        rc = self._check(self.L.ls_trace_scene(self.h, frame_index, C.byref(fr)), "ls_trace_scene")
        n = int(fr.n_points)
        if n and fr.compact16:   # LS_OPT_HOST_OUTPUT = 2
            pts = np.zeros((n, 32), np.uint8)
            self._check(self.L.ls_expand_points(pts.ctypes.data, fr.compact16, n), "ls_expand_points")
            hits = (np.frombuffer(C.string_at(fr.hits, n * 16), dtype=HIT_DTYPE).copy() if fr.hits else np.zeros(0, HIT_DTYPE))
        elif n:
            pts = np.ctypeslib.as_array(fr.points32, shape=(n * 32,)).reshape(n, 32).copy()
            hits = (np.frombuffer(C.string_at(fr.hits, n * 16), dtype=HIT_DTYPE).copy() if fr.hits
                    else np.zeros(0, HIT_DTYPE))   # LS_OPT_READBACK_HITS = 0: the records stay on the device
        else:
            pts = np.zeros((0, 32), np.uint8)
            hits = np.zeros(0, HIT_DTYPE)
        self.last_frame = fr
        return rc, pts, hits

    def traceSceneTwoStep(self, frame_index: int = 0):
        """ls_trace_scene_begin + ls_trace_scene_expand into a numpy buffer: -> (rc, points uint8[n,32])"""
        n = C.c_uint32()
        rc = self.L.ls_trace_scene_begin(self.h, frame_index, C.byref(n))
        if rc < -1:
            self._check(rc, "ls_trace_scene_begin")
        pts = np.empty((int(n.value), 32), np.uint8)
        if rc >= 0:
            self._check(self.L.ls_trace_scene_expand(self.h, pts.ctypes.data), "ls_trace_scene_expand")
        return rc, pts

    def traceSceneAsync(self, frame_index: int = 0) -> Frame:
        fr = Frame()
        self._check(self.L.ls_trace_scene_async(self.h, frame_index, C.byref(fr)), "ls_trace_scene_async")
        return fr

    def getGeometryCount(self) -> int:
        return int(self.L.ls_geometry_count(self.h))

    def getGeometryId(self, name: str) -> int:
        return self.L.ls_geometry_id(self.h, name.encode())

    def getGeometryType(self, name: str) -> int:
        """EmbreeTracer::getGeometryType (EmbreeTracer.cpp:103-113): LS_GEOMETRY_TYPE_* or a negative status."""
        return self.L.ls_geometry_type(self.h, name.encode())

    def getVertexCount(self, name: str) -> int:
        return int(self.L.ls_vertex_count(self.h, name.encode()))

    def getElementCount(self, name: str) -> int:
        return int(self.L.ls_element_count(self.h, name.encode()))

    def getTotalRays(self) -> int:
        return int(self.L.ls_total_rays(self.h))

    # ---- extensions
    def setShard(self, first_az: int, n_az: int):
        rc = self._check(self.L.ls_tracer_set_shard(self.h, first_az, n_az), "ls_tracer_set_shard")
        self.az0, self.naz = first_az, n_az
        return rc

    def setStream(self, stream_ptr: int | None):
        return self._check(self.L.ls_tracer_set_stream(self.h, stream_ptr), "ls_tracer_set_stream")

    def synchronize(self):
        return self._check(self.L.ls_tracer_synchronize(self.h), "ls_tracer_synchronize")

    def setOutputBuffers(self, d_points: int | None, d_hits: int | None, d_n: int | None, capacity: int):
        return self._check(self.L.ls_tracer_set_output_buffers(self.h, d_points, d_hits, d_n, capacity),
                           "ls_tracer_set_output_buffers")

    def setHitBuffers(self, d_hits: int | None, d_n: int | None, capacity: int):
        return self._check(self.L.ls_tracer_set_hit_buffers(self.h, d_hits, d_n, capacity), "ls_tracer_set_hit_buffers")

    def expandGatheredHits(self, d_gathered: int, world: int, capacity: int, d_points: int, d_hits: int, d_n: int):
        return self._check(self.L.ls_expand_gathered_hits(self.h, d_gathered, world, capacity, d_points, d_hits, d_n),
                           "ls_expand_gathered_hits")

    def expandGatheredHitsOn(self, stream_ptr: int, d_gathered: int, world: int, capacity: int, d_points: int, d_hits: int, d_n: int):
        self._check(self.L.ls_expand_gathered_hits_on(self.h, stream_ptr, d_gathered, world, capacity, d_points, d_hits, d_n),
                    "ls_expand_gathered_hits_on")

    def cloudToWorld(self, R, d_points_in: int, d_n_points: int, d_points_out: int, out_capacity: int, affine=None,
                     d_out_base: int | None = None, d_out_total: int | None = None):
        """ls_cloud_to_world: sensor-frame points (device) -> world frame, appended at *d_out_base."""
        R = np.ascontiguousarray(R, np.float32).reshape(9)
        A = None if affine is None else np.ascontiguousarray(affine, np.float32).reshape(12)
        return self._check(self.L.ls_cloud_to_world(self.h, None if A is None else _f32p(A), _f32p(R), d_points_in, d_n_points,
                                                    d_points_out, d_out_base, d_out_total, out_capacity),
                           "ls_cloud_to_world")

    def info(self, what: int) -> int:
        return int(self._check(self.L.ls_get_info(self.h, what), "ls_get_info"))

    def orderAfterLastFrame(self, stream_ptr: int):
        self._check(self.L.ls_tracer_order_after_last_frame(self.h, stream_ptr), "ls_tracer_order_after_last_frame")

    def waitEvent(self, event_ptr: int):
        self._check(self.L.ls_tracer_wait_event(self.h, event_ptr), "ls_tracer_wait_event")

    def nextFrameWaits(self, event_ptr: int):
        """only the frame issued next starts after the hipEvent_t (one wait on that frame's stream)"""
        self._check(self.L.ls_tracer_next_frame_waits(self.h, event_ptr), "ls_tracer_next_frame_waits")

    def flush(self):
        return self._check(self.L.ls_tracer_flush(self.h), "ls_tracer_flush")

    def setOption(self, option: int, value: int):
        return self._check(self.L.ls_tracer_set_option(self.h, option, value), "ls_tracer_set_option")

    def timings(self) -> dict:
        """Mean stage durations in ms over the frames recorded since the last call (+ 'frames')."""
        ms = np.zeros(len(STAGES), np.float32)
        n = self._check(self.L.ls_get_timings(self.h, _f32p(ms)), "ls_get_timings")
        d = dict(zip(STAGES, [float(x) for x in ms]))
        d["frames"] = int(n)
        return d

    def visitCounts(self):
        """-> (node fetches, triangle tests) of the last counted trace."""
        return self.visitStats()[:2]

    def visitStats(self):
        """-> (node fetches, triangle tests, sum of per-wave loop trips, max loop trips)."""
        c = (C.c_uint64 * 4)()
        self._check(self.L.ls_get_visit_counts(self.h, c), "ls_get_visit_counts")
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    def generateRays(self, d_dx: int, d_dy: int, d_dz: int):
        return self._check(self.L.ls_generate_rays(self.h, d_dx, d_dy, d_dz), "ls_generate_rays")

    @staticmethod
    def _ray_array(rays):
        r = np.ascontiguousarray(rays)
        if r.dtype != RAY_DTYPE:
            r = np.ascontiguousarray(r, np.float32)
            if r.ndim != 2 or r.shape[1] != 8:
                raise ValueError("rays: float32 (n, 8) or RAY_DTYPE")
        return r

    def traceRays(self, rays):
        """Closest hits of caller rays (ls_trace_rays_host): `rays` float32 (n, 8) -- origin xyz, tmin, direction xyz, tmax per
        row, the RAY_DTYPE layout, in the sensor frame -- or a RAY_DTYPE array.  -> (rc, HIT_DTYPE[n]); rc = -1 (no commit, empty
        scene): every record a miss."""
        r = self._ray_array(rays)
        n = r.shape[0]
        out = np.zeros(n, HIT_DTYPE)
        rc = self.L.ls_trace_rays_host(self.h, r.ctypes.data if n else None, n, out.ctypes.data if n else None)
        if rc == -1:
            out["ray"] = np.arange(n, dtype=np.uint32)
            out["geom"] = INVALID
            out["prim"] = INVALID
            out["t"] = -1.0
            return -1, out
        self._check(rc, "ls_trace_rays_host")
        return int(rc), out

    def traceRaysDevice(self, d_rays: int, n: int, d_out: int, stream=None) -> int:
        """ls_trace_rays on device pointers (n 32-byte rays in, n 16-byte ls_hit records out); enqueued on `stream` (a hipStream_t
        as an int, None: the handle's), no wait.  -> 0, or -1 on an empty / uncommitted scene (d_out not written)."""
        rc = self.L.ls_trace_rays(self.h, stream, d_rays, n, d_out)
        return -1 if rc == -1 else int(self._check(rc, "ls_trace_rays"))

    def occludedRays(self, rays):
        """Occlusion tests of caller rays (ls_occluded_rays_host): `rays` as traceRays takes them.  -> (rc, bool[n]): True where
        some triangle lies in [tmin, tmax] along the ray -- exactly where traceRays reports a hit; rc = -1 (no commit, empty
        scene): every entry False."""
        r = self._ray_array(rays)
        n = r.shape[0]
        out = np.zeros(n, np.uint8)
        rc = self.L.ls_occluded_rays_host(self.h, r.ctypes.data if n else None, n, out.ctypes.data if n else None)
        if rc == -1:
            return -1, np.zeros(n, np.bool_)
        self._check(rc, "ls_occluded_rays_host")
        return int(rc), out.view(np.bool_)

    def occludedRaysDevice(self, d_rays: int, n: int, d_out: int, stream=None) -> int:
        """ls_occluded_rays on device pointers (n 32-byte rays in, n bytes out, 1 = occluded); enqueued on `stream` (a
        hipStream_t as an int, None: the handle's), no wait.  -> 0, or -1 on an empty / uncommitted scene (d_out not written)."""
        rc = self.L.ls_occluded_rays(self.h, stream, d_rays, n, d_out)
        return -1 if rc == -1 else int(self._check(rc, "ls_occluded_rays"))

    def closestPoints(self, points):
        """Nearest surface points (ls_closest_points_host): `points` float32 (n, 4) -- x, y, z in the sensor frame and the
        largest distance of interest (inf: no bound) per row -- or a POINT_QUERY_DTYPE array.  -> (rc, CLOSEST_DTYPE[n]);
        rc = -1 (no commit, empty scene): every record a miss."""
        p = np.ascontiguousarray(points)
        if p.dtype != POINT_QUERY_DTYPE:
            p = np.ascontiguousarray(p, np.float32)
            if p.ndim != 2 or p.shape[1] != 4:
                raise ValueError("points: float32 (n, 4) or POINT_QUERY_DTYPE")
        n = p.shape[0]
        out = np.zeros(n, CLOSEST_DTYPE)
        rc = self.L.ls_closest_points_host(self.h, p.ctypes.data if n else None, n, out.ctypes.data if n else None)
        if rc == -1:
            out["index"] = np.arange(n, dtype=np.uint32)
            out["geom"] = INVALID
            out["prim"] = INVALID
            out["dist"] = -1.0
            return -1, out
        self._check(rc, "ls_closest_points_host")
        return int(rc), out

    def closestPointsDevice(self, d_points: int, n: int, d_out: int, stream=None) -> int:
        """ls_closest_points on device pointers (n 16-byte points in, n 32-byte records out); enqueued on `stream` (a hipStream_t
        as an int, None: the handle's), no wait.  -> 0, or -1 on an empty / uncommitted scene (d_out not written)."""
        rc = self.L.ls_closest_points(self.h, stream, d_points, n, d_out)
        return -1 if rc == -1 else int(self._check(rc, "ls_closest_points"))

    @staticmethod
    def _hit_array(hits):
        h = np.ascontiguousarray(hits)
        if h.dtype != HIT_DTYPE:
            h = np.ascontiguousarray(h, np.uint32)
            if h.ndim != 2 or h.shape[1] != 4:
                raise ValueError("hits: HIT_DTYPE or uint32 (n, 4)")
        return h

    @staticmethod
    def _pose_array(col_pose):
        pose = np.ascontiguousarray(col_pose, np.float32)
        if pose.ndim != 2 or pose.shape[1] != 12:
            raise ValueError("col_pose: float32 (H, 12)")
        return pose

    def _host_tables(self, col_pose, motions):
        """the pose table and the motion tables of traceSweepMoving as the _host entry points take them -> (the pose table's
        address or None, its length, the ls_geometry_motion array or None, its length, what keeps the tables alive)"""
        pose = None if col_pose is None else self._pose_array(col_pose)
        tabs = {int(g): np.ascontiguousarray(t, np.float32) for g, t in dict(motions).items()}
        H = self.info(LS_INFO_AZIMUTH_COUNT)
        if any(t.shape != (H, 12) for t in tabs.values()):
            raise ValueError("motions: float32 (H, 12) per geometry")
        arr, n_motions = self._device_motions({g: t.ctypes.data for g, t in tabs.items()})
        return None if pose is None else pose.ctypes.data, 0 if pose is None else pose.shape[0], arr, n_motions, (pose, tabs)

    @staticmethod
    def _device_motions(motions):
        items = list(dict(motions).items())
        arr = (GeometryMotion * max(1, len(items)))()
        for m, (g, addr) in zip(arr, items):
            m.geom, m.reserved, m.col_motion = int(g), 0, int(addr)
        return (arr if items else None), len(items)

    @staticmethod
    def _rays_arg(r, h):
        """the caller's rays as the gathers take them -> (address, count): none -- the handle's own sensor rays -- is (None, 0);
        rays given, but none of them, keep an address"""
        return (None, 0) if r is None else (r.ctypes.data if r.shape[0] else h.ctypes.data, r.shape[0])

    @staticmethod
    def _refl_arg(reflectivity):
        """-> (address or None, count, what keeps it alive)"""
        rho = None if reflectivity is None else np.ascontiguousarray(reflectivity, np.float32).reshape(-1)
        return rho.ctypes.data if rho is not None and rho.size else None, 0 if rho is None else rho.size, rho

    def _records(self, rc, what, o: _Outputs, count: bool = True):
        """what a call with _Outputs returns: (rc[, k], the first k records of every output); rc = -1: none of them"""
        if rc != -1:
            self._check(rc, what)
        k = 0 if rc == -1 else int(o.k.value)
        return (int(rc),) + ((k,) if count else ()) + o.first(k)

    def _attributes(self, rc, what, h, out):
        """what the attribute calls return: (rc, out); rc = -1: every record invalid, with its ray"""
        if rc == -1:
            out["ray"] = h["ray"] if h.dtype == HIT_DTYPE else h[:, 0]
            return -1, out
        self._check(rc, what)
        return int(rc), out

    def hitAttributes(self, hits, rays=None):
        """Surface attributes of hit records (ls_hit_attributes_host): `hits` a HIT_DTYPE array (a frame's, or traceRays'), `rays`
        None -- the handle's own sensor rays, hit.ray the global ray index -- or the rays given to traceRays (float32 (n, 8) or
        RAY_DTYPE).  -> (rc, HIT_ATTR_DTYPE[n]); rc = -1 (no commit, empty scene): every record invalid."""
        h = self._hit_array(hits)
        n = h.shape[0]
        r = None if rays is None else self._ray_array(rays)
        out = np.zeros(n, HIT_ATTR_DTYPE)
        rc = self.L.ls_hit_attributes_host(self.h, *self._rays_arg(r, h), h.ctypes.data if n else None, n, out.ctypes.data if n else None)
        return self._attributes(rc, "ls_hit_attributes_host", h, out)

    def hitAttributesDevice(self, d_hits: int, n: int, d_out: int, d_rays: int = 0, n_rays: int = 0, d_count: int = 0, stream=None) -> int:
        """ls_hit_attributes on device pointers (n 16-byte ls_hit records in, 48-byte records out; d_rays = 0: the handle's sensor
        rays; d_count != 0: a device word, min(n, *d_count) records are handled); enqueued on `stream` (a hipStream_t as an int,
        None: the handle's), no wait.  -> 0, or -1 on an empty / uncommitted scene (d_out not written)."""
        rc = self.L.ls_hit_attributes(self.h, stream, d_rays or None, n_rays, d_hits or None, d_count or None, n, d_out or None)
        return -1 if rc == -1 else int(self._check(rc, "ls_hit_attributes"))

    @staticmethod
    def emptyObjectLabels(n_labels: int):
        """n_labels records of a geomID that got nothing and names nothing: what objectLabels returns for rc = -1"""
        out = np.zeros(n_labels, OBJECT_LABEL_DTYPE)
        out["t_min"], out["lo"] = np.inf, np.inf
        out["t_max"], out["hi"] = -np.inf, -np.inf
        out["ray_min"], out["ray_max"] = INVALID, INVALID
        return out

    def objectLabels(self, hits, rays=None, footprint: bool = True, n_labels: int | None = None):
        """Per-geometry labels of hit records (ls_object_labels_host): `hits` and `rays` as hitAttributes takes them (`hits` may be
        None or empty: the footprint alone), `footprint`: also n_alone, the rays that hit each geometry taken alone
        (LS_LABEL_FOOTPRINT); `n_labels` records indexed by geomID, by default the highest id added through this object + 1.
        -> (rc, OBJECT_LABEL_DTYPE[n_labels]); rc = -1 (no commit, empty scene): every record empty with flags = 0."""
        h = self._hit_array(np.zeros(0, HIT_DTYPE) if hits is None else hits)
        n = h.shape[0]
        r = None if rays is None else self._ray_array(rays)
        if n_labels is None:
            n_labels = max(self.__dict__.get("_geom_ids", {}).values(), default=-1) + 1
        out = np.zeros(n_labels, OBJECT_LABEL_DTYPE)
        rc = self.L.ls_object_labels_host(self.h, LS_LABEL_FOOTPRINT if footprint else 0, None if r is None else (r.ctypes.data if r.shape[0] else out.ctypes.data),
                                          0 if r is None else r.shape[0], h.ctypes.data if n else None, n, out.ctypes.data if n_labels else None, n_labels)
        if rc == -1:
            return -1, self.emptyObjectLabels(n_labels)
        self._check(rc, "ls_object_labels_host")
        return int(rc), out

    def objectLabelsDevice(self, d_labels: int, n_labels: int, d_hits: int = 0, n: int = 0, d_rays: int = 0, n_rays: int = 0, d_count: int = 0,
                           footprint: bool = True, stream=None) -> int:
        """ls_object_labels on device pointers (n 16-byte ls_hit records in, n_labels 64-byte records out; d_rays = 0: the handle's
        sensor rays; d_count != 0: a device word, min(n, *d_count) records are handled); enqueued on `stream` (a hipStream_t as an
        int, None: the handle's), no wait.  -> 0, or -1 on an empty / uncommitted scene (d_labels not written)."""
        rc = self.L.ls_object_labels(self.h, stream, LS_LABEL_FOOTPRINT if footprint else 0, d_rays or None, n_rays, d_hits or None, d_count or None,
                                     n, d_labels or None, n_labels)
        return -1 if rc == -1 else int(self._check(rc, "ls_object_labels"))

    @staticmethod
    def _grid_shape(desc, call="ls_occupancy_grid"):
        """(nz, ny, nx) of a descriptor (an OccupancyGridDesc or a SceneGridDesc) the library would not refuse for its size (the arrays
        are made before the call)"""
        nx, ny, nz = (int(x) for x in desc.dims)
        if not (0 < nx <= OCCUPANCY_MAX_DIM and 0 < ny <= OCCUPANCY_MAX_DIM and 0 < nz <= OCCUPANCY_MAX_DIM and nx * ny * nz <= OCCUPANCY_MAX_CELLS):
            raise LidarShooterHipError(call + ": a grid dimension of 0 or above 2048, or more than 2^27 cells")
        return nz, ny, nx

    def occupancyGrid(self, desc: OccupancyGridDesc, hits, rays=None, sensor_to_grid=None, into=None):
        """The voxel grid a frame carves (ls_occupancy_grid_host): `hits` and `rays` as objectLabels takes them (`hits` may be None or
        empty: every ray is a miss), `sensor_to_grid` None or 12 floats (row-major 3 x 4), `into` None or a pair (counts, geom) to
        accumulate on -- the call then runs with LS_OCC_ACCUMULATE and returns new arrays.
        -> (rc, counts uint32[nz, ny, nx, 2] = {n_free, n_occ}, geom uint32[nz, ny, nx]); rc = -1 (no commit, empty scene): cleared
        arrays (zeros and 0xFFFFFFFF)."""
        h = self._hit_array(np.zeros(0, HIT_DTYPE) if hits is None else hits)
        n = h.shape[0]
        r = None if rays is None else self._ray_array(rays)
        nz, ny, nx = self._grid_shape(desc)
        d = OccupancyGridDesc.from_buffer_copy(desc)
        if into is None:
            counts, geom = np.zeros((nz, ny, nx, 2), np.uint32), np.full((nz, ny, nx), INVALID, np.uint32)
            d.flags &= ~LS_OCC_ACCUMULATE
        else:
            counts = np.array(into[0], np.uint32, order="C").reshape(nz, ny, nx, 2)
            geom = np.array(into[1], np.uint32, order="C").reshape(nz, ny, nx)
            d.flags |= LS_OCC_ACCUMULATE
        m = None if sensor_to_grid is None else np.ascontiguousarray(sensor_to_grid, np.float32).reshape(12)
        rc = self.L.ls_occupancy_grid_host(self.h, C.byref(d), None if m is None else m.ctypes.data,
                                           None if r is None else (r.ctypes.data if r.shape[0] else counts.ctypes.data), 0 if r is None else r.shape[0],
                                           h.ctypes.data if n else None, n, counts.ctypes.data, geom.ctypes.data)
        if rc == -1:
            return -1, np.zeros((nz, ny, nx, 2), np.uint32), np.full((nz, ny, nx), INVALID, np.uint32)
        self._check(rc, "ls_occupancy_grid_host")
        return int(rc), counts, geom

    def occupancyGridDevice(self, desc: OccupancyGridDesc, d_counts: int, d_geom: int = 0, d_hits: int = 0, n: int = 0, d_rays: int = 0,
                            n_rays: int = 0, d_count: int = 0, sensor_to_grid=None, stream=None) -> int:
        """ls_occupancy_grid on device pointers (n 16-byte ls_hit records in; nx ny nz {n_free, n_occ} pairs and, with d_geom != 0, as
        many geom words out; d_rays = 0: the handle's sensor rays; d_count != 0: a device word, min(n, *d_count) records are
        handled); enqueued on `stream` (a hipStream_t as an int, None: the handle's), no wait.  -> 0, or -1 on an empty /
        uncommitted scene (nothing written)."""
        m = None if sensor_to_grid is None else np.ascontiguousarray(sensor_to_grid, np.float32).reshape(12)
        rc = self.L.ls_occupancy_grid(self.h, stream, C.byref(desc), None if m is None else m.ctypes.data, d_rays or None, n_rays,
                                      d_hits or None, d_count or None, n, d_counts or None, d_geom or None)
        return -1 if rc == -1 else int(self._check(rc, "ls_occupancy_grid"))

    def sceneGrid(self, desc: SceneGridDesc, select=None, sensor_to_grid=None, into=None):
        """The voxels the committed scene's surface occupies (ls_scene_grid_host): `select` None or bytes indexed by geomID (0: the
        geometry is left out), `sensor_to_grid` None or 12 floats (row-major 3 x 4), `into` None or a pair (counts, geom) to accumulate
        on -- the call then runs with LS_SCENE_GRID_ACCUMULATE and returns new arrays.
        -> (rc, counts uint32[nz, ny, nx], geom uint32[nz, ny, nx]); rc = -1 (no commit, empty scene): cleared arrays (zeros and
        0xFFFFFFFF)."""
        nz, ny, nx = self._grid_shape(desc, "ls_scene_grid")
        d = SceneGridDesc.from_buffer_copy(desc)
        if into is None:
            counts, geom = np.zeros((nz, ny, nx), np.uint32), np.full((nz, ny, nx), INVALID, np.uint32)
            d.flags &= ~LS_SCENE_GRID_ACCUMULATE
        else:
            counts = np.array(into[0], np.uint32, order="C").reshape(nz, ny, nx)
            geom = np.array(into[1], np.uint32, order="C").reshape(nz, ny, nx)
            d.flags |= LS_SCENE_GRID_ACCUMULATE
        m = None if sensor_to_grid is None else np.ascontiguousarray(sensor_to_grid, np.float32).reshape(12)
        sel = None if select is None else np.ascontiguousarray(select, np.uint8).reshape(-1)
        rc = self.L.ls_scene_grid_host(self.h, C.byref(d), None if m is None else m.ctypes.data,
                                       sel.ctypes.data if sel is not None and sel.size else None, 0 if sel is None else sel.size,
                                       counts.ctypes.data, geom.ctypes.data)
        if rc == -1:
            return -1, np.zeros((nz, ny, nx), np.uint32), np.full((nz, ny, nx), INVALID, np.uint32)
        self._check(rc, "ls_scene_grid_host")
        return int(rc), counts, geom

    def sceneGridDevice(self, desc: SceneGridDesc, d_counts: int, d_geom: int = 0, d_select: int = 0, n_select: int = 0, sensor_to_grid=None,
                        stream=None) -> int:
        """ls_scene_grid on device pointers (nx ny nz count words and, with d_geom != 0, as many geom words out; d_select = 0: every
        geometry); enqueued on `stream` (a hipStream_t as an int, None: the handle's), no wait.  -> 0, or -1 on an empty /
        uncommitted scene (nothing written)."""
        m = None if sensor_to_grid is None else np.ascontiguousarray(sensor_to_grid, np.float32).reshape(12)
        rc = self.L.ls_scene_grid(self.h, stream, C.byref(desc), None if m is None else m.ctypes.data, d_select or None, n_select,
                                  d_counts or None, d_geom or None)
        return -1 if rc == -1 else int(self._check(rc, "ls_scene_grid"))

    def sceneDistanceGrid(self, desc: DistanceGridDesc, select=None, sensor_to_grid=None, into=None):
        """The truncated distance field of the committed scene (ls_scene_distance_grid_host): `select` and `sensor_to_grid` as sceneGrid
        takes them, `into` None or a pair (dist, geom) to take the minimum with -- the call then runs with LS_DIST_GRID_ACCUMULATE
        and returns new arrays.
        -> (rc, dist float32[nz, ny, nx], geom uint32[nz, ny, nx]); a cell with no surface within trunc of its centre: +inf and
        0xFFFFFFFF; rc = -1 (no commit, empty scene): every cell so."""
        nz, ny, nx = self._grid_shape(desc, "ls_scene_distance_grid")
        d = DistanceGridDesc.from_buffer_copy(desc)
        cells = np.zeros((nz, ny, nx), DIST_GRID_DTYPE)
        if into is None:
            cells.view(np.uint64)[...] = DIST_GRID_REST
            d.flags &= ~LS_DIST_GRID_ACCUMULATE
        else:
            cells["dist"] = np.asarray(into[0], np.float32).reshape(nz, ny, nx)
            cells["geom"] = np.asarray(into[1], np.uint32).reshape(nz, ny, nx)
            d.flags |= LS_DIST_GRID_ACCUMULATE
        m = None if sensor_to_grid is None else np.ascontiguousarray(sensor_to_grid, np.float32).reshape(12)
        sel = None if select is None else np.ascontiguousarray(select, np.uint8).reshape(-1)
        rc = self.L.ls_scene_distance_grid_host(self.h, C.byref(d), None if m is None else m.ctypes.data,
                                                sel.ctypes.data if sel is not None and sel.size else None, 0 if sel is None else sel.size,
                                                cells.ctypes.data)
        if rc == -1:
            return -1, np.full((nz, ny, nx), np.inf, np.float32), np.full((nz, ny, nx), INVALID, np.uint32)
        self._check(rc, "ls_scene_distance_grid_host")
        return int(rc), np.ascontiguousarray(cells["dist"]), np.ascontiguousarray(cells["geom"])

    def sceneDistanceGridDevice(self, desc: DistanceGridDesc, d_cells: int, d_select: int = 0, n_select: int = 0, sensor_to_grid=None,
                                stream=None) -> int:
        """ls_scene_distance_grid on device pointers (nx ny nz 8-byte records {geom, dist} out, 16-byte aligned; d_select = 0: every
        geometry); enqueued on `stream` (a hipStream_t as an int, None: the handle's), no wait.  -> 0, or -1 on an empty /
        uncommitted scene (nothing written)."""
        m = None if sensor_to_grid is None else np.ascontiguousarray(sensor_to_grid, np.float32).reshape(12)
        rc = self.L.ls_scene_distance_grid(self.h, stream, C.byref(desc), None if m is None else m.ctypes.data, d_select or None, n_select,
                                           d_cells or None)
        return -1 if rc == -1 else int(self._check(rc, "ls_scene_distance_grid"))

    @staticmethod
    def emptySurfaceSamples(n: int):
        """n invalid records: zeros with geom = 0xFFFFFFFF"""
        out = np.zeros(n, SURFACE_SAMPLE_DTYPE)
        out["geom"] = INVALID
        return out

    def sampleSurface(self, desc: SurfaceSampleDesc, select=None, sensor_to_out=None):
        """Points drawn from the surface of the committed scene in proportion to area (ls_sample_surface_host): `select` None or bytes
        indexed by geomID (0: the geometry is left out), `sensor_to_out` None or 12 floats (row-major 3 x 4).
        -> (rc, samples SURFACE_SAMPLE_DTYPE[n_samples], info SURFACE_INFO_DTYPE[()]); rc = -1 (no commit, empty scene): invalid
        records and a zero info."""
        n = int(desc.n_samples)
        samples, info = np.zeros(n, SURFACE_SAMPLE_DTYPE), np.zeros(1, SURFACE_INFO_DTYPE)
        m = None if sensor_to_out is None else np.ascontiguousarray(sensor_to_out, np.float32).reshape(12)
        sel = None if select is None else np.ascontiguousarray(select, np.uint8).reshape(-1)
        rc = self.L.ls_sample_surface_host(self.h, C.byref(desc), None if m is None else m.ctypes.data,
                                           sel.ctypes.data if sel is not None and sel.size else None, 0 if sel is None else sel.size,
                                           samples.ctypes.data if n else None, info.ctypes.data)
        if rc == -1:
            return -1, self.emptySurfaceSamples(n), np.zeros(1, SURFACE_INFO_DTYPE)[0]
        self._check(rc, "ls_sample_surface_host")
        return int(rc), samples, info[0]

    def sampleSurfaceDevice(self, desc: SurfaceSampleDesc, d_samples: int, d_info: int = 0, d_select: int = 0, n_select: int = 0,
                            sensor_to_out=None, stream=None) -> int:
        """ls_sample_surface on device pointers (n_samples 48-byte records out, 16-byte aligned, and, with d_info != 0, the 16 bytes of
        the info; d_select = 0: every geometry); enqueued on `stream` (a hipStream_t as an int, None: the handle's), no wait.  -> 0,
        or -1 on an empty / uncommitted scene (nothing written)."""
        m = None if sensor_to_out is None else np.ascontiguousarray(sensor_to_out, np.float32).reshape(12)
        rc = self.L.ls_sample_surface(self.h, stream, C.byref(desc), None if m is None else m.ctypes.data, d_select or None, n_select,
                                      d_samples or None, d_info or None)
        return -1 if rc == -1 else int(self._check(rc, "ls_sample_surface"))

    @staticmethod
    def _strided_points(a, stride):
        """an array of whole records of `stride` bytes (any dtype and shape) -> (bytes, record count)"""
        b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if b.size % int(stride):
            raise ValueError("the array is not a whole number of records of %d bytes" % stride)
        return b, b.size // int(stride)

    def cloudNearest(self, desc: CloudNearestDesc, cloud, queries, query_to_cloud=None):
        """The nearest cloud point to each query within desc.radius (ls_cloud_nearest_host; needs no committed scene): `cloud` and
        `queries` arrays of whole records of desc.cloud_stride / desc.query_stride bytes with x, y, z float32 at bytes 0, 4, 8 (a
        float32 (n, 3) array for stride 12, a frame's (n, 32) uint8 points for 32, ...), `query_to_cloud` None or 12 floats
        (row-major 3 x 4).  -> (rc, records CLOUD_NEAREST_DTYPE[n_queries], info CLOUD_NEAREST_INFO_DTYPE[()])"""
        c, n_cloud = self._strided_points(cloud, desc.cloud_stride)
        q, n_queries = self._strided_points(queries, desc.query_stride)
        out, info = np.zeros(n_queries, CLOUD_NEAREST_DTYPE), np.zeros(1, CLOUD_NEAREST_INFO_DTYPE)
        m = None if query_to_cloud is None else np.ascontiguousarray(query_to_cloud, np.float32).reshape(12)
        rc = self.L.ls_cloud_nearest_host(self.h, C.byref(desc), None if m is None else m.ctypes.data, c.ctypes.data if n_cloud else None,
                                          n_cloud, q.ctypes.data if n_queries else None, n_queries, out.ctypes.data if n_queries else None,
                                          info.ctypes.data)
        self._check(rc, "ls_cloud_nearest_host")
        return int(rc), out, info[0]

    def cloudNearestDevice(self, desc: CloudNearestDesc, d_cloud: int, n_cloud: int, d_queries: int, n_queries: int, d_out: int,
                           d_info: int = 0, query_to_cloud=None, stream=None) -> int:
        """ls_cloud_nearest on device pointers (n_queries 16-byte records out, 16-byte aligned, and, with d_info != 0, the 16 bytes of
        the info); enqueued on `stream` (a hipStream_t as an int, None: the handle's), no wait.  -> 0"""
        m = None if query_to_cloud is None else np.ascontiguousarray(query_to_cloud, np.float32).reshape(12)
        rc = self.L.ls_cloud_nearest(self.h, stream, C.byref(desc), None if m is None else m.ctypes.data, d_cloud or None, n_cloud,
                                     d_queries or None, n_queries, d_out or None, d_info or None)
        return int(self._check(rc, "ls_cloud_nearest"))

    def applyReturnModel(self, model: ReturnModel, hits, rays=None, reflectivity=None, frame_index: int = 0):
        """Sensor returns from hit records (ls_apply_return_model_host): `hits` and `rays` as hitAttributes takes them, `reflectivity`
        None or float32 per geomID.  -> (rc, points uint8[k, 32], hits HIT_DTYPE[k] with the noisy t): the kept returns in input
        order; rc = -1 (no commit, empty scene): none."""
        h = self._hit_array(hits)
        n = h.shape[0]
        r = None if rays is None else self._ray_array(rays)
        rho, n_rho, keep = self._refl_arg(reflectivity)
        o = _Outputs(n, True, True)
        rc = self.L.ls_apply_return_model_host(self.h, C.byref(model), frame_index, *self._rays_arg(r, h), h.ctypes.data if n else None, n, rho, n_rho,
                                               *o.ptrs, C.byref(o.k))
        return self._records(rc, "ls_apply_return_model_host", o, count=False)

    def applyReturnModelDevice(self, model: ReturnModel, d_hits: int, n: int, d_n_out: int, d_points32: int = 0, d_hits_out: int = 0, d_rays: int = 0,
                               n_rays: int = 0, d_count: int = 0, d_reflectivity: int = 0, n_reflectivity: int = 0, frame_index: int = 0,
                               stream=None) -> int:
        """ls_apply_return_model on device pointers (n ls_hit records in; up to n 32-byte points and n ls_hit records out, either may
        be 0; the count in the device word d_n_out; d_rays = 0: the handle's sensor rays; d_count != 0: a device word, min(n, *d_count)
        records are handled); enqueued on `stream` (a hipStream_t as an int, None: the handle's), no wait.  -> 0, or -1 on an empty
        / uncommitted scene (nothing written)."""
        rc = self.L.ls_apply_return_model(self.h, stream, C.byref(model), frame_index, d_rays or None, n_rays, d_hits or None, d_count or None, n,
                                          d_reflectivity or None, n_reflectivity, d_points32 or None, d_hits_out or None, d_n_out or None)
        return -1 if rc == -1 else int(self._check(rc, "ls_apply_return_model"))

    def traceSweep(self, col_pose, flags: int = 0, points: bool = True, hits: bool = True, rays_out=None):
        """A frame whose sensor moves during the turn (ls_trace_scene_sweep_host): `col_pose` float32 (H, 12) -- [R | o] row-major,
        the sensor's pose when azimuth column h fires, in the frame-start sensor frame -- for the FULL raster whatever the shard.
        `points` / `hits` False: that output is not asked for (None comes back); `rays_out` None, or a RAY_DTYPE / float32 (V * H, 8)
        array of the full raster whose shard records are overwritten in place.  -> (rc, k, points uint8[k, 32] or None, hits
        HIT_DTYPE[k] or None); rc = -1 (no commit, empty scene): no record."""
        pose = self._pose_array(col_pose)
        if rays_out is not None and not (isinstance(rays_out, np.ndarray) and rays_out.flags.c_contiguous and rays_out.flags.writeable and
                                         rays_out.nbytes == 32 * int(self.L.ls_total_channels(self.h)) * self.info(LS_INFO_AZIMUTH_COUNT)):
            raise ValueError("rays_out: a writable contiguous array of V * H 32-byte records")
        n = self.getTotalRays()
        o = _Outputs(n, points, hits)
        rc = self.L.ls_trace_scene_sweep_host(self.h, pose.ctypes.data if pose.size else None, pose.shape[0], flags, *o.ptrs, C.byref(o.k), n,
                                              None if rays_out is None else rays_out.ctypes.data)
        return self._records(rc, "ls_trace_scene_sweep_host", o)

    def traceSweepDevice(self, d_col_pose: int, n_cols: int, d_n_points: int, capacity: int, d_points32: int = 0, d_hits: int = 0,
                         d_rays_out: int = 0, flags: int = 0, stream=None) -> int:
        """ls_trace_scene_sweep on device pointers (n_cols 48-byte pose records in; up to `capacity` 32-byte points and ls_hit
        records out, either may be 0; the count in the device word d_n_points; d_rays_out: 0, or V * H 32-byte ray records);
        enqueued on `stream` (a hipStream_t as an int, None: the handle's), no wait.  -> 0, or -1 on an empty / uncommitted scene
        (nothing written)."""
        rc = self.L.ls_trace_scene_sweep(self.h, stream, d_col_pose or None, n_cols, flags, d_points32 or None, d_hits or None, d_n_points or None,
                                         capacity, d_rays_out or None)
        return -1 if rc == -1 else int(self._check(rc, "ls_trace_scene_sweep"))

    def traceSweepMoving(self, col_pose, motions, flags: int = 0, points: bool = True, hits: bool = True):
        """A sweep frame whose geometries move during the turn (ls_trace_scene_sweep_moving_host): `col_pose` as in traceSweep, or
        None: the sensor at rest; `motions` a dict geomID -> float32 (H, 12) table [Q | c] row-major, the rigid displacement of that
        geometry when azimuth column h fires, relative to where it was committed, in the frame-start sensor frame (geometries not
        named are at rest).  -> (rc, k, points uint8[k, 32] or None, hits HIT_DTYPE[k] or None); rc = -1: no record."""
        *tables, keep = self._host_tables(col_pose, motions)
        n = self.getTotalRays()
        o = _Outputs(n, points, hits)
        rc = self.L.ls_trace_scene_sweep_moving_host(self.h, *tables, flags, *o.ptrs, C.byref(o.k), n)
        return self._records(rc, "ls_trace_scene_sweep_moving_host", o)

    def traceSweepMovingDevice(self, d_col_pose: int, n_cols: int, motions, d_n_points: int, capacity: int, d_points32: int = 0,
                               d_hits: int = 0, flags: int = 0, stream=None) -> int:
        """ls_trace_scene_sweep_moving on device pointers: traceSweepDevice (d_col_pose 0 with n_cols 0: the sensor at rest) with
        `motions`, a dict geomID -> device address of that geometry's H 48-byte records; enqueued on `stream` (a hipStream_t as an
        int, None: the handle's), no wait.  -> 0, or -1 on an empty / uncommitted scene (nothing written)."""
        arr, n_motions = self._device_motions(motions)
        rc = self.L.ls_trace_scene_sweep_moving(self.h, stream, d_col_pose or None, n_cols, arr, n_motions, flags, d_points32 or None, d_hits or None,
                                                d_n_points or None, capacity)
        return -1 if rc == -1 else int(self._check(rc, "ls_trace_scene_sweep_moving"))

    def hitAttributesMoving(self, hits, col_pose, motions, flags: int = 0):
        """Surface attributes of the records of a sweep frame (ls_hit_attributes_moving_host): `hits` a HIT_DTYPE array of
        traceSweepMoving (hit.ray the global ray index), `col_pose`, `motions` and `flags` what that frame was traced with.  ->
        (rc, HIT_ATTR_DTYPE[n]): the normal in the sensor frame, p the frame's point; rc = -1 (no commit, empty scene): every
        record invalid."""
        h = self._hit_array(hits)
        n = h.shape[0]
        *tables, keep = self._host_tables(col_pose, motions)
        out = np.zeros(n, HIT_ATTR_DTYPE)
        rc = self.L.ls_hit_attributes_moving_host(self.h, *tables, flags, h.ctypes.data if n else None, n, out.ctypes.data if n else None)
        return self._attributes(rc, "ls_hit_attributes_moving_host", h, out)

    def hitAttributesMovingDevice(self, d_hits: int, n: int, d_out: int, d_col_pose: int = 0, n_cols: int = 0, motions=(), flags: int = 0,
                                  d_count: int = 0, stream=None) -> int:
        """ls_hit_attributes_moving on device pointers: hitAttributesDevice's records with the tables of traceSweepMovingDevice
        (d_col_pose 0 with n_cols 0: the sensor at rest; `motions` a dict geomID -> device address of H 48-byte records); enqueued on
        `stream` (a hipStream_t as an int, None: the handle's), no wait.  -> 0, or -1 on an empty / uncommitted scene (d_out not
        written)."""
        arr, n_motions = self._device_motions(motions)
        rc = self.L.ls_hit_attributes_moving(self.h, stream, d_col_pose or None, n_cols, arr, n_motions, flags, d_hits or None, d_count or None, n,
                                             d_out or None)
        return -1 if rc == -1 else int(self._check(rc, "ls_hit_attributes_moving"))

    def applyReturnModelMoving(self, model: ReturnModel, hits, col_pose, motions, flags: int = 0, reflectivity=None, frame_index: int = 0):
        """Sensor returns from the records of a sweep frame (ls_apply_return_model_moving_host): `hits`, `col_pose`, `motions` and
        `flags` as hitAttributesMoving takes them, `reflectivity` None or float32 per geomID.  -> (rc, points uint8[k, 32] with
        their ring, hits HIT_DTYPE[k] with the noisy t): the kept returns in input order; rc = -1: none."""
        h = self._hit_array(hits)
        n = h.shape[0]
        *tables, keep = self._host_tables(col_pose, motions)
        rho, n_rho, keep_rho = self._refl_arg(reflectivity)
        o = _Outputs(n, True, True)
        rc = self.L.ls_apply_return_model_moving_host(self.h, C.byref(model), frame_index, *tables, flags, h.ctypes.data if n else None, n, rho, n_rho,
                                                      *o.ptrs, C.byref(o.k))
        return self._records(rc, "ls_apply_return_model_moving_host", o, count=False)

    def applyReturnModelMovingDevice(self, model: ReturnModel, d_hits: int, n: int, d_n_out: int, d_points32: int = 0, d_hits_out: int = 0,
                                     d_col_pose: int = 0, n_cols: int = 0, motions=(), flags: int = 0, d_count: int = 0, d_reflectivity: int = 0,
                                     n_reflectivity: int = 0, frame_index: int = 0, stream=None) -> int:
        """ls_apply_return_model_moving on device pointers: applyReturnModelDevice's records and outputs with the tables of
        traceSweepMovingDevice; enqueued on `stream` (a hipStream_t as an int, None: the handle's), no wait.  -> 0, or -1 on an
        empty / uncommitted scene (nothing written)."""
        arr, n_motions = self._device_motions(motions)
        rc = self.L.ls_apply_return_model_moving(self.h, stream, C.byref(model), frame_index, d_col_pose or None, n_cols, arr, n_motions, flags,
                                                 d_hits or None, d_count or None, n, d_reflectivity or None, n_reflectivity, d_points32 or None,
                                                 d_hits_out or None, d_n_out or None)
        return -1 if rc == -1 else int(self._check(rc, "ls_apply_return_model_moving"))

    @staticmethod
    def _device_twists(twists):
        items = list(dict(twists).items())
        arr = (GeometryTwist * max(1, len(items)))()
        for m, (g, addr) in zip(arr, items):
            m.geom, m.reserved, m.col_twist = int(g), 0, int(addr)
        return (arr if items else None), len(items)

    def hitVelocities(self, hits, col_pose=None, motions=(), sensor_twist=None, twists=(), flags: int = 0, records: bool = True,
                      radial: bool = True):
        """Velocities at hit records (ls_hit_velocities_host): `hits`, `col_pose` and `motions` as hitAttributesMoving takes them --
        the tables the frame was traced with --; `sensor_twist` None (the sensor at rest) or float32 (H, 6) records [w | u];
        `twists` a dict geomID -> float32 (H, 6) (geometries not named are at rest).  -> (rc, HIT_VELOCITY_DTYPE[n] or None, the
        radial velocities float32[n] or None -- NaN for an invalid record); rc = -1 (no commit, empty scene): every record invalid."""
        h = self._hit_array(hits)
        n = h.shape[0]
        *tables, keep = self._host_tables(col_pose, motions)
        H = self.info(LS_INFO_AZIMUTH_COUNT)
        st = None if sensor_twist is None else np.ascontiguousarray(sensor_twist, np.float32)
        tabs = {int(g): np.ascontiguousarray(t, np.float32) for g, t in dict(twists).items()}
        if any(t.shape != (H, 6) for t in list(tabs.values()) + ([] if st is None else [st])):
            raise ValueError("twists: float32 (H, 6) per body")
        arr, n_twists = self._device_twists({g: t.ctypes.data for g, t in tabs.items()})
        out = np.zeros(n, HIT_VELOCITY_DTYPE) if records else None
        rad = np.full(n, np.nan, np.float32) if radial else None
        rc = self.L.ls_hit_velocities_host(self.h, *tables, None if st is None else st.ctypes.data, arr, n_twists, flags, h.ctypes.data if n else None,
                                           n, out.ctypes.data if records and n else None, rad.ctypes.data if radial and n else None)
        if rc != -1:
            self._check(rc, "ls_hit_velocities_host")
        return int(rc), out, rad

    def hitVelocitiesDevice(self, d_hits: int, n: int, d_out: int = 0, d_radial: int = 0, d_col_pose: int = 0, n_cols: int = 0, motions=(),
                            d_sensor_twist: int = 0, twists=(), flags: int = 0, d_count: int = 0, stream=None) -> int:
        """ls_hit_velocities on device pointers: hitAttributesMovingDevice's records and tables, d_sensor_twist 0 (the sensor at rest)
        or the device address of H 24-byte twist records, `twists` a dict geomID -> such an address; 32-byte records to d_out and
        floats to d_radial, either may be 0; enqueued on `stream` (a hipStream_t as an int, None: the handle's), no wait.  -> 0, or
        -1 on an empty / uncommitted scene (nothing written)."""
        arr, n_motions = self._device_motions(motions)
        tws, n_twists = self._device_twists(twists)
        rc = self.L.ls_hit_velocities(self.h, stream, d_col_pose or None, n_cols, arr, n_motions, d_sensor_twist or None, tws, n_twists, flags,
                                      d_hits or None, d_count or None, n, d_out or None, d_radial or None)
        return -1 if rc == -1 else int(self._check(rc, "ls_hit_velocities"))

    def traceBeamsHost(self, model: BeamModel, points: bool = True, hits: bool = True, echo: bool = True):
        """A frame of diverging beams with multi-echo returns (ls_trace_scene_beams_host): model.n_samples sub-rays per ray of the
        shard, the returns of every beam in ascending ray index and range.  An output asked for with False comes back None.
        -> (rc, k, points uint8[k, 32] or None, hits HIT_DTYPE[k] or None -- t the reported range --, echo words uint32[k] or
        None); rc = -1 (no commit, empty scene): no record."""
        cap = model.n_returns * self.getTotalRays()
        o = _Outputs(cap, points, hits, echo)
        rc = self.L.ls_trace_scene_beams_host(self.h, C.byref(model), *o.ptrs, C.byref(o.k), cap)
        return self._records(rc, "ls_trace_scene_beams_host", o)

    def traceBeamsDevice(self, model: BeamModel, d_n_points: int, capacity: int, d_points32: int = 0, d_hits: int = 0, d_echo: int = 0,
                         stream=None) -> int:
        """ls_trace_scene_beams on device pointers (up to `capacity` 32-byte points, ls_hit records and echo words out, any may be 0;
        the count in the device word d_n_points); the model's pattern is read during the call; enqueued on `stream` (a hipStream_t
        as an int, None: the handle's), no wait.  -> 0, or -1 on an empty / uncommitted scene (nothing written)."""
        rc = self.L.ls_trace_scene_beams(self.h, stream, C.byref(model), d_points32 or None, d_hits or None, d_echo or None, d_n_points or None,
                                         capacity)
        return -1 if rc == -1 else int(self._check(rc, "ls_trace_scene_beams"))

    def traceBeamsSweep(self, model: BeamModel, weights=None, min_weight: int = 0, col_pose=None, flags: int = 0, points: bool = True,
                        hits: bool = True, echo: bool = True):
        """A frame of weighted beams from a moving sensor (ls_trace_scene_beams_sweep_host): traceBeamsHost with `weights` -- None
        (1 each) or model.n_samples integers in 1..65535 --, the strength threshold `min_weight` and `col_pose` -- None (the sensor at
        rest) or float32 (H, 12) as for traceSweep; flags: 0 or LS_SWEEP_DESKEW.  -> (rc, k, points uint8[k, 32] or None, hits
        HIT_DTYPE[k] or None, echo words uint32[k] or None); rc = -1 (no commit, empty scene): no record."""
        w = None if weights is None else np.ascontiguousarray(weights, np.uint32).reshape(-1)
        if w is not None and w.shape[0] != model.n_samples:
            raise ValueError("weights: one per sample of the model")
        pose = None if col_pose is None else self._pose_array(col_pose)
        cap = model.n_returns * self.getTotalRays()
        o = _Outputs(cap, points, hits, echo)
        rc = self.L.ls_trace_scene_beams_sweep_host(self.h, C.byref(model), None if w is None else _u32p(w), int(min_weight),
                                                    pose.ctypes.data if pose is not None and pose.size else None, 0 if pose is None else pose.shape[0],
                                                    flags, *o.ptrs, C.byref(o.k), cap)
        return self._records(rc, "ls_trace_scene_beams_sweep_host", o)

    def traceBeamsSweepDevice(self, model: BeamModel, d_n_points: int, capacity: int, d_points32: int = 0, d_hits: int = 0, d_echo: int = 0,
                              weights=None, min_weight: int = 0, d_col_pose: int = 0, n_cols: int = 0, flags: int = 0, stream=None) -> int:
        """ls_trace_scene_beams_sweep on device pointers: traceBeamsDevice with `weights` (host memory: None, or model.n_samples
        integers in 1..65535, read during the call), `min_weight`, the pose table d_col_pose (0 with n_cols 0: the sensor at rest;
        else n_cols 48-byte records) and flags (0 or LS_SWEEP_DESKEW); enqueued on `stream`, no wait.  -> 0, or -1 on an empty /
        uncommitted scene (nothing written)."""
        w = None if weights is None else np.ascontiguousarray(weights, np.uint32).reshape(-1)
        if w is not None and w.shape[0] != model.n_samples:
            raise ValueError("weights: one per sample of the model")
        rc = self.L.ls_trace_scene_beams_sweep(self.h, stream, C.byref(model), None if w is None else _u32p(w), int(min_weight), d_col_pose or None,
                                               n_cols, flags, d_points32 or None, d_hits or None, d_echo or None, d_n_points or None, capacity)
        return -1 if rc == -1 else int(self._check(rc, "ls_trace_scene_beams_sweep"))

    # ---- test hooks
    def formatCloud(self, fmt: CloudFormat, hits, points=None, echo=None, col_time=None, chan_time=None):
        """A cloud in a driver's own record (ls_format_cloud_host): `hits` HIT_DTYPE or uint32 (n, 4), `points` the uint8 (n, 32)
        points that belong to them (None when the format names none of x, y, z, intensity), `echo` None or uint32 (n,), `col_time`
        None or float32 (H,), `chan_time` None or float32 (V,).  -> uint8 (n, point_step), or (V * H, point_step) organized.  Needs
        no committed scene."""
        h = self._hit_array(hits)
        n = h.shape[0]
        p = None if points is None else np.ascontiguousarray(points, np.uint8).reshape(-1, 32)
        e = None if echo is None else np.ascontiguousarray(echo, np.uint32).reshape(-1)
        ct = None if col_time is None else np.ascontiguousarray(col_time, np.float32).reshape(-1)
        ch = None if chan_time is None else np.ascontiguousarray(chan_time, np.float32).reshape(-1)
        V, H = int(self.L.ls_total_channels(self.h)), self.info(LS_INFO_AZIMUTH_COUNT)
        if (p is not None and p.shape[0] != n) or (e is not None and e.shape[0] != n) or (ct is not None and ct.shape[0] != H) or \
                (ch is not None and ch.shape[0] != V):
            raise ValueError("points, echo: one per hit record; col_time: H floats; chan_time: V floats")
        out = np.zeros((V * H if fmt.organized else n, max(int(fmt.point_step), 1)), np.uint8)
        rc = self.L.ls_format_cloud_host(self.h, C.byref(fmt), p.ctypes.data if p is not None and n else None, h.ctypes.data if n else None,
                                         e.ctypes.data if e is not None and n else None, n, None if ct is None else ct.ctypes.data,
                                         None if ch is None else ch.ctypes.data, out.ctypes.data if out.size else None)
        self._check(rc, "ls_format_cloud_host")
        return out

    def formatCloudDevice(self, fmt: CloudFormat, d_hits: int, n: int, d_out: int, d_points32: int = 0, d_echo: int = 0, d_count: int = 0,
                          d_col_time: int = 0, d_chan_time: int = 0, stream=None) -> int:
        """ls_format_cloud on device pointers (n ls_hit records, their 32-byte points and echo words in -- the latter two may be 0 --;
        d_count != 0: a device word, min(n, *d_count) records are handled; d_col_time: H floats, d_chan_time: V floats, 0: zeros;
        records of fmt.point_step bytes out, V * H of them organized); enqueued on `stream` (a hipStream_t as an int, None: the
        handle's), no wait."""
        rc = self.L.ls_format_cloud(self.h, stream, C.byref(fmt), d_points32 or None, d_hits or None, d_echo or None, d_count or None, n,
                                    d_col_time or None, d_chan_time or None, d_out or None)
        return int(self._check(rc, "ls_format_cloud"))

    def generateRaysAos(self, d_rays: int | None, d_hits: int | None):
        """LidarDevice::allRaysGPU's two buffers (Ray 32 B, Hit 24 B per ray) in device memory of the caller."""
        self._check(self.L.ls_generate_rays_aos(self.h, d_rays, d_hits), "ls_generate_rays_aos")

    def denseHits(self):
        n = self.getTotalRays()
        t = np.zeros(n, np.float32)
        gid = np.zeros(n, np.uint32)
        self._check(self.L.ls_debug_dense_hits(self.h, _f32p(t), gid.ctypes.data_as(C.POINTER(C.c_uint32))),
                    "ls_debug_dense_hits")
        return t, gid

    def bruteForce(self):
        n = self.getTotalRays()
        t = np.zeros(n, np.float32)
        gid = np.zeros(n, np.uint32)
        self._check(self.L.ls_debug_trace_bruteforce(self.h, _f32p(t), gid.ctypes.data_as(C.POINTER(C.c_uint32))),
                    "ls_debug_trace_bruteforce")
        return t, gid

    def sortPairs(self, keys: np.ndarray, vals: np.ndarray):
        """The build path's radix sort on its own: -> (sorted keys, values); stable, 30-bit keys."""
        k, v = np.ascontiguousarray(keys, np.uint32).copy(), np.ascontiguousarray(vals, np.uint32).copy()
        self._check(self.L.ls_debug_sort_pairs(self.h, k.ctypes.data, v.ctypes.data, k.shape[0]), "ls_debug_sort_pairs")
        return k, v

    def sceneSize(self):
        v = [C.c_uint32() for _ in range(4)]
        self._check(self.L.ls_debug_scene_size(self.h, *[C.byref(x) for x in v]), "ls_debug_scene_size")
        return dict(n_verts=v[0].value, n_tris=v[1].value, n_slots=v[2].value, leaf_size=v[3].value)

    def downloadScene(self):
        s = self.sceneSize()
        verts = np.zeros((s["n_verts"], 3), np.float32)
        tris = np.zeros((s["n_tris"], 3), np.uint32)
        self._check(self.L.ls_debug_download_scene(self.h, verts.ctypes.data, tris.ctypes.data), "ls_debug_download_scene")
        return verts, tris

    def downloadBvh(self):
        s = self.sceneSize()
        nodes = np.zeros(s["n_slots"], NODE_DTYPE)
        tri = np.zeros(s["n_tris"], TRI_DTYPE)
        self._check(self.L.ls_debug_download_bvh(self.h, nodes.ctypes.data, tri.ctypes.data), "ls_debug_download_bvh")
        return nodes, tri, s["leaf_size"]

    def downloadHierarchy(self, name: str, wide: bool = True):
        """ls_debug_download_hierarchy: the instanced hierarchy of geometry `name` (mesh space) -> (binary nodes NODE_DTYPE, their
        four-wide twins WIDE_DTYPE or None, records MESH_TRI_DTYPE, leaf size)"""
        gid, nt = self.getGeometryId(name), self.getElementCount(name)
        L, g = C.c_uint32(), C.c_uint32()
        self._check(self.L.ls_debug_download_hierarchy(self.h, gid, C.byref(L), C.byref(g), None, None, None), "ls_debug_download_hierarchy")
        nodes = np.zeros(max(L.value, 1) - 1, NODE_DTYPE)
        twins = np.zeros(nodes.shape[0], WIDE_DTYPE) if wide else None
        rec = np.zeros(nt, MESH_TRI_DTYPE)
        self._check(self.L.ls_debug_download_hierarchy(self.h, gid, None, None, nodes.ctypes.data, twins.ctypes.data if wide else None,
                                                       rec.ctypes.data), "ls_debug_download_hierarchy")
        return nodes, twins, rec, g.value

    def forceGroupCull(self, on: bool = True):
        """ls_debug_force_group_cull: LS_OPT_BLOCK_CULL = 1 then applies to geometries of any size (from the next commit)"""
        self._check(self.L.ls_debug_force_group_cull(self.h, 1 if on else 0), "ls_debug_force_group_cull")

    def downloadCull(self, name: str):
        """ls_debug_download_cull: -> (perm uint32[n_tris]: sorted position -> caller's triangle, group boxes float32[n_groups, 8],
        block boxes float32[n_blocks, 8]; a box = cx cy cz hx hy hz sx sy)"""
        gid, nt = self.getGeometryId(name), C.c_uint32()
        self._check(self.L.ls_debug_download_cull(self.h, gid, C.byref(nt), None, None, None), "ls_debug_download_cull")
        groups = (nt.value + 3) // 4
        perm, gb, bb = np.zeros(nt.value, np.uint32), np.zeros((groups, 8), np.float32), np.zeros(((groups + 63) // 64, 8), np.float32)
        self._check(self.L.ls_debug_download_cull(self.h, gid, None, perm.ctypes.data, gb.ctypes.data, bb.ctypes.data), "ls_debug_download_cull")
        return perm, gb, bb

    def cullSurvivors(self, name: str):
        """ls_debug_cull_survivors: the groups of geometry `name` the next frame's cull pass keeps -> (uint32[n] ascending,
        LS_DEBUG_CULL_* bits of the k_cull instantiation that ran)"""
        gid = self.getGeometryId(name)
        out = np.zeros((self.getElementCount(name) * (2 if self.getGeometryType(name) else 1) + 3) // 4, np.uint32)
        n, variant = C.c_uint32(), C.c_uint32()
        self._check(self.L.ls_debug_cull_survivors(self.h, gid, out.ctypes.data, out.shape[0], C.byref(n), C.byref(variant)), "ls_debug_cull_survivors")
        return out[:n.value].copy(), variant.value

    def cullTables(self):
        """ls_debug_cull_tables: -> (tan_up float32[V], tan_dn float32[V], channel of each position uint32[V], lut_ok bool)"""
        up, dn, perm, ok = np.zeros(self.V, np.float32), np.zeros(self.V, np.float32), np.zeros(self.V, np.uint32), C.c_int()
        self._check(self.L.ls_debug_cull_tables(self.h, up.ctypes.data, dn.ctypes.data, perm.ctypes.data, C.byref(ok)), "ls_debug_cull_tables")
        return up, dn, perm, bool(ok.value)

    def chanQuery(self, tan_lo, tan_hi):
        """ls_debug_chan_query: k_cull's channel query on the device -> (look-up table's answers uint8[n], 2 = not in use;
        binary search's uint8[n])"""
        q = np.ascontiguousarray(np.stack([np.asarray(tan_lo, np.float32), np.asarray(tan_hi, np.float32)], axis=1))
        out = np.zeros((q.shape[0], 2), np.uint8)
        self._check(self.L.ls_debug_chan_query(self.h, q.ctypes.data, q.shape[0], out.ctypes.data), "ls_debug_chan_query")
        return out[:, 0].copy(), out[:, 1].copy()


def closest_on_triangle(p, v0, v1, v2):
    """ls_debug_closest_on_triangle: the library's float32 point-triangle arithmetic on the host -> (q float32[3], d2 float32)"""
    L = load()
    a = [np.ascontiguousarray(x, np.float32).reshape(3) for x in (p, v0, v1, v2)]
    q = np.zeros(3, np.float32)
    d2 = C.c_float()
    rc = L.ls_debug_closest_on_triangle(_f32p(a[0]), _f32p(a[1]), _f32p(a[2]), _f32p(a[3]), _f32p(q), C.byref(d2))
    if rc != 0:
        raise LidarShooterHipError(f"ls_debug_closest_on_triangle: status {rc}")
    return q, np.float32(d2.value)


def hit_attributes_on_triangle(o, d, v0, v1, v2):
    """ls_debug_hit_attributes_on_triangle: the library's float32 hit-attribute arithmetic on the host -> None when the exact test
    fails, else (t float32, out float32[9] = n, cos_inc, u, v, p)"""
    L = load()
    a = [np.ascontiguousarray(x, np.float32).reshape(3) for x in (o, d, v0, v1, v2)]
    out = np.zeros(9, np.float32)
    t = C.c_float()
    rc = L.ls_debug_hit_attributes_on_triangle(*[_f32p(x) for x in a], C.byref(t), _f32p(out))
    if rc < 0:
        raise LidarShooterHipError(f"ls_debug_hit_attributes_on_triangle: status {rc}")
    return (np.float32(t.value), out) if rc == 1 else None


def philox4x32(ctr, key):
    """ls_debug_philox4x32: Philox4x32-10 of a 4-word counter under a 2-word key -> uint32[4]"""
    L = load()
    c, k, out = np.ascontiguousarray(ctr, np.uint32).reshape(4), np.ascontiguousarray(key, np.uint32).reshape(2), np.zeros(4, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    rc = L.ls_debug_philox4x32(c.ctypes.data_as(u32p), k.ctypes.data_as(u32p), out.ctypes.data_as(u32p))
    if rc != 0:
        raise LidarShooterHipError(f"ls_debug_philox4x32: status {rc}")
    return out


def return_model(model: ReturnModel, ray, frame_index, t, length, cos_inc, rho):
    """ls_debug_return_model: the library's float32 return model on the host for one valid hit -> (kept bool, t' float32,
    intensity float32)"""
    L = load()
    t_out, inten = C.c_float(), C.c_float()
    rc = L.ls_debug_return_model(C.byref(model), int(ray), int(frame_index), float(t), float(length), float(cos_inc), float(rho),
                                 C.byref(t_out), C.byref(inten))
    if rc < 0:
        raise LidarShooterHipError(f"ls_debug_return_model: status {rc}")
    return rc == 1, np.float32(t_out.value), np.float32(inten.value)


def sweep_poses_constant_twist(lin_vel, ang_vel, t0: float, dt: float, n_cols: int):
    """ls_sweep_poses_constant_twist: the pose table of a sensor moving at a constant twist -> float32 (n_cols, 12), [R | o]
    row-major, tau_h = t0 + h dt"""
    L = load()
    lin, ang = (np.ascontiguousarray(x, np.float32).reshape(3) for x in (lin_vel, ang_vel))
    out = np.zeros((int(n_cols), 12), np.float32)
    rc = L.ls_sweep_poses_constant_twist(_f32p(lin), _f32p(ang), float(t0), float(dt), int(n_cols), _f32p(out))
    if rc != 0:
        raise LidarShooterHipError(f"ls_sweep_poses_constant_twist: status {rc}")
    return out


def sweep_ray(d, pose12):
    """ls_debug_sweep_ray: the ray ls_trace_scene_sweep casts for the nominal direction d under one pose record, on the host ->
    float32[8] (origin, tmin, direction, tmax)"""
    L = load()
    dd, p = np.ascontiguousarray(d, np.float32).reshape(3), np.ascontiguousarray(pose12, np.float32).reshape(12)
    out = np.zeros(8, np.float32)
    rc = L.ls_debug_sweep_ray(_f32p(dd), _f32p(p), _f32p(out))
    if rc != 0:
        raise LidarShooterHipError(f"ls_debug_sweep_ray: status {rc}")
    return out


def motion_constant_twist(lin_vel, ang_vel, pivot, t0: float, dt: float, n_cols: int):
    """ls_motion_constant_twist: the motion table of a body that turns about `pivot` while it drives on -> float32 (n_cols, 12),
    [Q | c] row-major, tau_h = t0 + h dt"""
    L = load()
    lin, ang, piv = (np.ascontiguousarray(x, np.float32).reshape(3) for x in (lin_vel, ang_vel, pivot))
    out = np.zeros((int(n_cols), 12), np.float32)
    rc = L.ls_motion_constant_twist(_f32p(lin), _f32p(ang), _f32p(piv), float(t0), float(dt), int(n_cols), _f32p(out))
    if rc != 0:
        raise LidarShooterHipError(f"ls_motion_constant_twist: status {rc}")
    return out


def motion_ray(ray8, motion12):
    """ls_debug_motion_ray: the ray a geometry under one motion record sees of the ray record ray8, on the host -> float32[8]
    (origin Q^T (o - c), tmin 0, direction Q^T d, tmax 1e16)"""
    L = load()
    r, p = np.ascontiguousarray(ray8, np.float32).reshape(8), np.ascontiguousarray(motion12, np.float32).reshape(12)
    out = np.zeros(8, np.float32)
    rc = L.ls_debug_motion_ray(_f32p(r), _f32p(p), _f32p(out))
    if rc != 0:
        raise LidarShooterHipError(f"ls_debug_motion_ray: status {rc}")
    return out


def motion_normal(n3, motion12):
    """ls_debug_motion_normal: the normal n3 found on a geometry where it was committed, carried forward by one motion record into
    the sensor frame, on the host -> float32[3]"""
    L = load()
    nn, p = np.ascontiguousarray(n3, np.float32).reshape(3), np.ascontiguousarray(motion12, np.float32).reshape(12)
    out = np.zeros(3, np.float32)
    rc = L.ls_debug_motion_normal(_f32p(nn), _f32p(p), _f32p(out))
    if rc != 0:
        raise LidarShooterHipError(f"ls_debug_motion_normal: status {rc}")
    return out


def twist_table_constant(lin_vel, ang_vel, pivot, t0: float, dt: float, n_cols: int):
    """ls_twist_table_constant: the twist table of the body whose motion table motion_constant_twist writes for the same arguments
    -> float32 (n_cols, 6), [w | u], tau_h = t0 + h dt"""
    L = load()
    lin, ang, piv = (np.ascontiguousarray(x, np.float32).reshape(3) for x in (lin_vel, ang_vel, pivot))
    out = np.zeros((int(n_cols), 6), np.float32)
    rc = L.ls_twist_table_constant(_f32p(lin), _f32p(ang), _f32p(piv), float(t0), float(dt), int(n_cols), _f32p(out))
    if rc != 0:
        raise LidarShooterHipError(f"ls_twist_table_constant: status {rc}")
    return out


def hit_velocity(cast8, t, sensor_twist6=None, geom_twist6=None):
    """ls_debug_hit_velocity: one valid record of ls_hit_velocities on the host, for a hit at t along the cast ray record cast8 with
    the column's twist records of the sensor and of the geometry (None: at rest) -> uint32[8]: the bits of v_s xyz, radial, v_o xyz,
    and flags = 1"""
    L = load()
    c = np.ascontiguousarray(cast8, np.float32).reshape(8)
    st, gt = (None if x is None else np.ascontiguousarray(x, np.float32).reshape(6) for x in (sensor_twist6, geom_twist6))
    out = np.zeros(8, np.float32)
    rc = L.ls_debug_hit_velocity(_f32p(c), C.c_float(float(np.float32(t))), None if st is None else _f32p(st), None if gt is None else _f32p(gt),
                                 _f32p(out))
    if rc != 0:
        raise LidarShooterHipError(f"ls_debug_hit_velocity: status {rc}")
    return out.view(np.uint32)


def beam_pattern_rings(half_angle_az: float, half_angle_el: float, n_rings: int, per_ring: int):
    """ls_beam_pattern_rings: the centre sample and n_rings concentric rings of per_ring samples -> float32 (1 + n_rings * per_ring,
    3) records (a, b, k)"""
    L = load()
    S = 1 + int(n_rings) * int(per_ring)
    out = np.zeros((max(S, 1), 3), np.float32)
    rc = L.ls_beam_pattern_rings(float(half_angle_az), float(half_angle_el), int(n_rings), int(per_ring), _f32p(out) if S <= 64 else None)
    if rc != 0:
        raise LidarShooterHipError(f"ls_beam_pattern_rings: status {rc}")
    return out


def beam_ray(sin_theta, cos_theta, cos_phi, sin_phi, abk):
    """ls_debug_beam_ray: the sub-ray ls_trace_scene_beams casts for sample (a, b, k) of the ray with these factor-table entries, on
    the host -> float32[8] (origin, tmin, direction, tmax)"""
    L = load()
    s, out = np.ascontiguousarray(abk, np.float32).reshape(3), np.zeros(8, np.float32)
    rc = L.ls_debug_beam_ray(float(sin_theta), float(cos_theta), float(cos_phi), float(sin_phi), _f32p(s), _f32p(out))
    if rc != 0:
        raise LidarShooterHipError(f"ls_debug_beam_ray: status {rc}")
    return out


def beam_echoes(model: BeamModel, r, hit):
    """ls_debug_beam_echoes: the returns of one beam from the reported ranges r[S] and the hit flags hit[S] of its sub-rays, on the
    host -> uint32 (n, 2): the bits of r_e and the echo word, in ascending range"""
    L = load()
    rr, hh = np.ascontiguousarray(r, np.float32).reshape(-1), np.ascontiguousarray(hit, np.uint8).reshape(-1)
    if rr.shape[0] != model.n_samples or hh.shape[0] != model.n_samples:
        raise ValueError("r, hit: one entry per sample of the model")
    out, n = np.zeros((3, 2), np.uint32), C.c_uint32(0)
    rc = L.ls_debug_beam_echoes(C.byref(model), _f32p(rr), hh.ctypes.data, out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n))
    if rc != 0:
        raise LidarShooterHipError(f"ls_debug_beam_echoes: status {rc}")
    return out[:n.value].copy()


def beam_weights_gaussian(pattern, sigma_az: float, sigma_el: float):
    """ls_beam_weights_gaussian: a weight per sample of a pattern, 65535 at the centre of a Gaussian with these standard deviations
    (the units of the pattern's a and b) -> uint32 (S,), each in 1..65535"""
    L = load()
    pat = np.ascontiguousarray(pattern, np.float32).reshape(-1, 3)
    out = np.zeros(max(pat.shape[0], 1), np.uint32)
    rc = L.ls_beam_weights_gaussian(_f32p(pat), pat.shape[0], float(sigma_az), float(sigma_el), _u32p(out) if pat.shape[0] <= 64 else None)
    if rc != 0:
        raise LidarShooterHipError(f"ls_beam_weights_gaussian: status {rc}")
    return out[:pat.shape[0]]


def beam_sweep_ray(sin_theta, cos_theta, cos_phi, sin_phi, abk, pose12):
    """ls_debug_beam_sweep_ray: the sub-ray ls_trace_scene_beams_sweep casts for sample (a, b, k) of the ray with these factor-table
    entries under one pose record, on the host -> float32[8] (origin, tmin, direction, tmax)"""
    L = load()
    s, p, out = np.ascontiguousarray(abk, np.float32).reshape(3), np.ascontiguousarray(pose12, np.float32).reshape(12), np.zeros(8, np.float32)
    rc = L.ls_debug_beam_sweep_ray(float(sin_theta), float(cos_theta), float(cos_phi), float(sin_phi), _f32p(s), _f32p(p), _f32p(out))
    if rc != 0:
        raise LidarShooterHipError(f"ls_debug_beam_sweep_ray: status {rc}")
    return out


def beam_echoes_weighted(model: BeamModel, weights, min_weight, r, hit):
    """ls_debug_beam_echoes_weighted: beam_echoes with a weight per sample (None: 1 each) and the strength threshold -> uint32 (n, 3):
    the bits of r_e, the echo word and the strength W_e, in ascending range"""
    L = load()
    rr, hh = np.ascontiguousarray(r, np.float32).reshape(-1), np.ascontiguousarray(hit, np.uint8).reshape(-1)
    w = None if weights is None else np.ascontiguousarray(weights, np.uint32).reshape(-1)
    if rr.shape[0] != model.n_samples or hh.shape[0] != model.n_samples or (w is not None and w.shape[0] != model.n_samples):
        raise ValueError("r, hit, weights: one entry per sample of the model")
    out, n = np.zeros((3, 3), np.uint32), C.c_uint32(0)
    rc = L.ls_debug_beam_echoes_weighted(C.byref(model), None if w is None else _u32p(w), int(min_weight), _f32p(rr), hh.ctypes.data, _u32p(out),
                                         C.byref(n))
    if rc != 0:
        raise LidarShooterHipError(f"ls_debug_beam_echoes_weighted: status {rc}")
    return out[:n.value].copy()


def cloud_format_check(fmt: CloudFormat) -> int:
    """ls_cloud_format_check: 0, or LS_ERR_INVALID_ARGUMENT (-2) for a format ls_format_cloud refuses"""
    return int(load().ls_cloud_format_check(C.byref(fmt)))


def cloud_format_from_point_fields(point_fields, point_step: int) -> CloudFormat:
    """ls_cloud_format_from_point_fields: the format a sensor config declares -- `point_fields` the dicts of message.pointFields[]
    (name, offset, datatype, count), `point_step` message.pointStep -> CloudFormat; raises on an unknown name, a count other than 1 or
    a layout ls_cloud_format_check refuses (the status is in the message)"""
    L = load()
    pf = list(point_fields)
    n = len(pf)
    names = (C.c_char_p * max(n, 1))(*[str(f["name"]).encode() for f in pf])
    offsets = np.array([int(f["offset"]) for f in pf], np.uint32)
    datatypes = np.array([int(f["datatype"]) for f in pf], np.uint8)
    counts = np.array([int(f.get("count", 1)) for f in pf], np.uint32)
    out = CloudFormat()
    rc = L.ls_cloud_format_from_point_fields(names, _u32p(offsets), datatypes.ctypes.data_as(C.POINTER(C.c_uint8)), _u32p(counts), n, int(point_step),
                                             C.byref(out))
    if rc != 0:
        raise LidarShooterHipError(f"ls_cloud_format_from_point_fields: status {rc}")
    return out


def column_times(t0: float, dt: float, n_cols: int):
    """ls_column_times: the firing time of every azimuth column, tau_h = t0 + h dt in double rounded once -> float32 (n_cols,)"""
    L = load()
    out = np.zeros(max(int(n_cols), 1), np.float32)
    rc = L.ls_column_times(float(t0), float(dt), int(n_cols), _f32p(out))
    if rc != 0:
        raise LidarShooterHipError(f"ls_column_times: status {rc}")
    return out[:int(n_cols)]


def format_record(fmt: CloudFormat, point32, hit, echo_word: int, col_time_value: float, chan_time_value: float, V: int, H: int,
                  cell_ray: int = 0):
    """ls_debug_format_record: one record of ls_format_cloud on the host -- `point32` 32 bytes or None, `hit` a HIT_DTYPE record /
    4 words, or None: the miss cell of `cell_ray` -> uint8 (point_step,)"""
    L = load()
    p = None if point32 is None else np.ascontiguousarray(point32).view(np.uint8).reshape(32)
    h = None if hit is None else np.ascontiguousarray(hit).view(np.uint8).reshape(16)
    out = np.full(max(int(fmt.point_step), 1), 0xEE, np.uint8)
    rc = L.ls_debug_format_record(C.byref(fmt), None if p is None else p.ctypes.data, None if h is None else h.ctypes.data, int(echo_word),
                                  float(col_time_value), float(chan_time_value), int(V), int(H), int(cell_ray), out.ctypes.data)
    if rc != 0:
        raise LidarShooterHipError(f"ls_debug_format_record: status {rc}")
    return out[:int(fmt.point_step)]
