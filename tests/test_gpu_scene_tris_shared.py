"""What ls_scene_grid, ls_scene_distance_grid and ls_sample_surface share on the host, on the MI355X: the scene's flat triangle index,
which whichever of the three is called first after a commit brings up to date for the other two, and the arrays of the accumulating
host-memory variants (the three grids), which travel to the device only when the call accumulates and always travel back.  Every
result is compared with the numpy restatements of tests/*_reference.py, byte for byte; nothing with the debug entry points."""
import ctypes

import numpy as np
import pytest

import distance_grid_reference as dref
import occupancy_reference as oref
import scene_grid_reference as gref
import surface_sample_reference as sref
from conftest import make_tracer
from test_gpu_rays import INV, _add, _records
from test_gpu_scene_grid import _unposed

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64


def _two_geometries(oracle, capi, tr):
    """geomID 0: two triangles, a tilted square; geomID 1: a plate of 3 x 2 quads, twelve triangles -> the mesh list"""
    sv = np.array([[-1.5, -1.5, -0.5], [1.2, -1.4, -0.3], [1.3, 1.1, 0.4], [-1.2, 1.4, 0.6]], F)
    st = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    xs, ys = np.meshgrid(np.linspace(-1.8, 1.6, 4), np.linspace(-1.0, 1.2, 3), indexing="xy")
    pv = np.stack([xs, ys, 0.2 * xs - 0.3], -1).reshape(-1, 3).astype(F)
    pq = np.array([[j * 4 + i, j * 4 + i + 1, j * 4 + i + 5, j * 4 + i + 4] for j in range(2) for i in range(3)], np.uint32)
    assert _add(tr, "square", sv, st) == 0 and _add(tr, "plate", pv, pq, capi.LS_GEOMETRY_TYPE_QUAD) == 1
    tr.updateGeometry("square", oracle.IDENTITY_AFFINE, sv, st)
    tr.updateGeometry("plate", oracle.IDENTITY_AFFINE, pv, pq)
    assert tr.commitScene() == 0
    return [(0, sv, st, oracle.IDENTITY_AFFINE), (1, pv, pq, oracle.IDENTITY_AFFINE)]


# ---- 1. the flat triangle index after the scene changes --------------------------------------------------------------------------

BOX = dict(origin=(-2.0, -2.0, -1.0), cell=1.0, dims=(4, 4, 2))
TRUNC = 0.75
N_SAMPLES, SEED = 64, 5


def _scene_grid(tr, capi, oracle, ml, s):
    g = gref.grid(**BOX)
    rc, counts, geom = tr.sceneGrid(capi.SceneGridDesc.make(g.origin, g.cell, g.dims))
    want = gref.scene_grid(g, *gref.scene_triangles(oracle, ml, s))
    assert rc == 0 and want[0].sum() > 0
    assert counts.tobytes() == want[0].tobytes() and geom.tobytes() == want[1].tobytes()


def _distance_grid(tr, capi, oracle, ml, s):
    g = dref.grid(trunc=TRUNC, **BOX)
    rc, dist, geom = tr.sceneDistanceGrid(capi.DistanceGridDesc.make(g.origin, g.cell, g.dims, 0, g.trunc))
    want = dref.distance_grid(g, *gref.scene_triangles(oracle, ml, s))
    assert rc == 0 and np.count_nonzero(want != dref.REST) > 0
    assert dref.words(dist, geom).tobytes() == want.tobytes()


def _surface_sample(tr, capi, oracle, ml, s):
    d = capi.SurfaceSampleDesc.make(N_SAMPLES, seed=SEED)
    rc, samples, info = tr.sampleSurface(d)
    want, want_info = sref.scene_samples(oracle, ml, s, None, None, d)
    assert rc == 0 and np.all(want["flags"] == 1)
    assert samples.tobytes() == want.tobytes() and info.tobytes() == want_info.tobytes()


QUERIES = (_scene_grid, _distance_grid, _surface_sample)


@pytest.mark.parametrize("first", [0, 1, 2])
def test_first_caller_after_a_commit_refreshes_the_index_for_all(oracle, capi, sensors, first):
    """two geometries of 2 and 12 triangles (the second a quad mesh); one query, so that the index is on the device; the first geometry
    leaves and the scene is committed; then a different query first, and the other two: each must see the new scene"""
    s = _unposed(sensors["0000"])
    tr = make_tracer(capi, s)
    ml = _two_geometries(oracle, capi, tr)
    QUERIES[(first + 2) % 3](tr, capi, oracle, ml, s)
    assert tr.removeGeometry("square") >= 0
    assert tr.commitScene() == 0
    for k in range(3):
        QUERIES[(first + k) % 3](tr, capi, oracle, ml[1:], s)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 2. the arrays of the accumulating host-memory variants ----------------------------------------------------------------------

SMALL_BOX = dict(origin=(-1.5, -1.5, -1.0), cell=1.0, dims=(3, 3, 2))
CELLS = 3 * 3 * 2


def _guarded(words, dtype, fill):
    """`words` elements of dtype filled with `fill` between two guards of 0xAB bytes -> (the buffer, the elements as a view)"""
    size = words * np.dtype(dtype).itemsize
    buf = np.full(GUARD + size + GUARD, 0xAB, np.uint8)
    a = buf[GUARD:GUARD + size].view(dtype)
    a[:] = fill
    return buf, a


def _guards_intact(buf):
    return bool(np.all(buf[:GUARD] == 0xAB) and np.all(buf[-GUARD:] == 0xAB))


def _prefilled(rng):
    """counts of a few thousand and geomIDs on both sides of the scene's, so that a sum or a minimum that forgot them shows"""
    return rng.integers(1, 5000, CELLS).astype(np.uint32), rng.choice(np.array([0, 1, 7, INV], np.uint32), CELLS)


def test_scene_grid_host_arrays_travel_both_ways(oracle, capi, sensors):
    s = _unposed(sensors["0000"])
    tr = make_tracer(capi, s)
    ml = _two_geometries(oracle, capi, tr)
    g = gref.grid(**SMALL_BOX)
    T, G = gref.scene_triangles(oracle, ml, s)
    plain = gref.scene_grid(g, T, G)
    assert plain[0].sum() > 10 and set(np.unique(plain[1])) >= {0, 1}
    pc, pg = _prefilled(np.random.default_rng(3))
    total = gref.scene_grid(g, T, G, into=(pc, pg))
    L, h = tr.L, tr.h
    acc = capi.SceneGridDesc.make(g.origin, g.cell, g.dims, gref.ACCUMULATE)
    d = capi.SceneGridDesc.make(g.origin, g.cell, g.dims)
    # accumulating: what the arrays held is added to and kept the minimum of
    bc, c = _guarded(CELLS, np.uint32, 0)
    bg, gm = _guarded(CELLS, np.uint32, 0)
    c[:], gm[:] = pc, pg
    assert L.ls_scene_grid_host(h, ctypes.byref(acc), None, None, 0, c.ctypes.data, gm.ctypes.data) == 0
    assert c.tobytes() == total[0].tobytes() and gm.tobytes() == total[1].tobytes() and _guards_intact(bc) and _guards_intact(bg)
    # no geom array, accumulating and not: the counts alone
    c[:] = pc
    assert L.ls_scene_grid_host(h, ctypes.byref(acc), None, None, 0, c.ctypes.data, None) == 0
    assert c.tobytes() == total[0].tobytes() and _guards_intact(bc)
    c[:] = 0xABABABAB
    assert L.ls_scene_grid_host(h, ctypes.byref(d), None, None, 0, c.ctypes.data, None) == 0
    assert c.tobytes() == plain[0].tobytes() and _guards_intact(bc)
    # a plain call into garbage: nothing of it was copied in
    c[:], gm[:] = 0xDEADBEEF, 0x12345678
    assert L.ls_scene_grid_host(h, ctypes.byref(d), None, None, 0, c.ctypes.data, gm.ctypes.data) == 0
    assert c.tobytes() == plain[0].tobytes() and gm.tobytes() == plain[1].tobytes() and _guards_intact(bc) and _guards_intact(bg)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_distance_grid_host_array_travels_both_ways(oracle, capi, sensors):
    s = _unposed(sensors["0000"])
    tr = make_tracer(capi, s)
    ml = _two_geometries(oracle, capi, tr)
    g = dref.grid(trunc=TRUNC, **SMALL_BOX)
    T, G = gref.scene_triangles(oracle, ml, s)
    plain = dref.distance_grid(g, T, G)
    reached = plain != dref.REST
    assert np.count_nonzero(reached) > 6 and not np.all(reached)
    # half the cells hold a record nearer than any surface, the others one farther than trunc
    rng = np.random.default_rng(4)
    pre = dref.words(np.where(rng.random(CELLS) < 0.5, F(0.001), F(3.0)).astype(F), rng.integers(0, 9, CELLS).astype(np.uint32))
    total = dref.distance_grid(g, T, G, into=pre)
    assert np.any(total.reshape(-1) == pre) and np.any(total.reshape(-1) != pre)
    L, h = tr.L, tr.h
    bw, w = _guarded(CELLS, np.uint64, 0)
    w[:] = pre
    acc = capi.DistanceGridDesc.make(g.origin, g.cell, g.dims, dref.ACCUMULATE, g.trunc)
    assert L.ls_scene_distance_grid_host(h, ctypes.byref(acc), None, None, 0, w.ctypes.data) == 0
    assert w.tobytes() == total.tobytes() and _guards_intact(bw)
    # a plain call into garbage that would win every minimum: nothing of it was copied in
    w[:] = 0
    d = capi.DistanceGridDesc.make(g.origin, g.cell, g.dims, 0, g.trunc)
    assert L.ls_scene_distance_grid_host(h, ctypes.byref(d), None, None, 0, w.ctypes.data) == 0
    assert w.tobytes() == plain.tobytes() and _guards_intact(bw)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_occupancy_grid_host_arrays_travel_both_ways(oracle, capi, sensors):
    s = _unposed(sensors["0000"])
    tr = make_tracer(capi, s)
    ml = _two_geometries(oracle, capi, tr)
    geoms = {0: 2, 1: 6}
    # rays from above the box straight and slanted down through it, and two that miss everything
    rng = np.random.default_rng(5)
    rays = np.zeros((40, 8), F)
    rays[:, 0:2] = rng.uniform(-1.4, 1.4, (40, 2))
    rays[:, 2] = 2.5
    rays[:, 4:6] = rng.uniform(-0.2, 0.2, (40, 2))
    rays[:, 6], rays[:, 7] = -1.0, np.inf
    rays[38:, 0] = 30.0
    rc, hits = tr.traceRays(rays)
    assert rc == 0
    rec = _records(hits)
    assert np.count_nonzero(rec[:, 1] != INV) > 20
    g = oref.grid(flags=oref.CARVE_MISSES, **SMALL_BOX)
    plain = oref.occupancy(g, rays, rec, geoms)[:2]
    assert plain[0][..., 0].sum() > 20 and plain[0][..., 1].sum() > 10
    prng = np.random.default_rng(6)
    pc = prng.integers(1, 5000, (CELLS, 2)).astype(np.uint32)
    pg = _prefilled(prng)[1]
    total = oref.occupancy(g, rays, rec, geoms, into=(pc, pg))[:2]
    L, h = tr.L, tr.h
    d = capi.OccupancyGridDesc.make(g.origin, g.cell, g.dims, g.flags, g.min_range, g.max_range)
    acc = capi.OccupancyGridDesc.make(g.origin, g.cell, g.dims, g.flags | oref.ACCUMULATE, g.min_range, g.max_range)
    n = rec.shape[0]
    rec = np.ascontiguousarray(rec, np.uint32)

    def call(desc, counts, geom):
        return L.ls_occupancy_grid_host(h, ctypes.byref(desc), None, rays.ctypes.data, rays.shape[0], rec.ctypes.data, n, counts.ctypes.data,
                                        None if geom is None else geom.ctypes.data)
    bc, c = _guarded(CELLS * 2, np.uint32, 0)
    bg, gm = _guarded(CELLS, np.uint32, 0)
    c[:], gm[:] = pc.reshape(-1), pg
    assert call(acc, c, gm) == 0
    assert c.tobytes() == total[0].tobytes() and gm.tobytes() == total[1].tobytes() and _guards_intact(bc) and _guards_intact(bg)
    # no geom array, accumulating and not: the counts alone
    c[:] = pc.reshape(-1)
    assert call(acc, c, None) == 0
    assert c.tobytes() == total[0].tobytes() and _guards_intact(bc)
    c[:] = 0xABABABAB
    assert call(d, c, None) == 0
    assert c.tobytes() == plain[0].tobytes() and _guards_intact(bc)
    # a plain call into garbage: nothing of it was copied in
    c[:], gm[:] = 0xDEADBEEF, 0x12345678
    assert call(d, c, gm) == 0
    assert c.tobytes() == plain[0].tobytes() and gm.tobytes() == plain[1].tobytes() and _guards_intact(bc) and _guards_intact(bg)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
