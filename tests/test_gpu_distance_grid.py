"""ls_scene_distance_grid / ls_scene_distance_grid_host on the MI355X: per cell of a voxel grid the distance from its centre to the
nearest triangle of the committed scene within trunc and the lowest geomID that attains it, against the numpy restatement of
tests/distance_grid_reference.py, byte for byte -- the golden scene on both engines' handles, posed geometries and quads under
transforms, pose updates and removals, synthetic meshes built for the split between the wave-per-triangle kernel and the queued one,
ties and contention, the selection, accumulation, ls_closest_points over the same cell centres, and the entry points' plumbing.
Nothing here is compared against ls_debug_distance_grid_triangle."""
import ctypes

import numpy as np
import pytest

import distance_grid_reference as ref
from conftest import make_tracer
from test_gpu_labels import _to_device
from test_gpu_rays import INV, _add, _ground_ben, _scene_posed_quads
from test_gpu_scene_grid import SPLIT_GRID, _at, _mesh, _span, _unposed
from test_occupancy_cpu import rigid_transform, rotation

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = -2                      # LS_ERR_INVALID_ARGUMENT
OUT_OF_RANGE = -9                          # LS_ERR_OUT_OF_RANGE
FRAME_EAGER = 0                            # LS_FRAME_EAGER
GUARD = 256
ACCUMULATE = ref.ACCUMULATE
REST = ref.REST
SMALL = 5247                               # kDistGridSmall as shipped: a wider range goes to k_distance_grid_big's queue
BIG_Y = 32                                 # kDistGridBigY: gridDim.y of k_distance_grid_big
F = np.float32

# torch fills a new tensor on its own stream, the library works on the handle's: every buffer is filled (a device-wide
# synchronize) before the library gets it


def _desc(capi, g):
    return capi.DistanceGridDesc.make(g.origin, g.cell, g.dims, g.flags, g.trunc)


def _same(got, want):
    """grids as 64-bit words, byte for byte"""
    assert got.dtype == np.uint64 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (bad.shape[0], bad[:5], hex(int(got[tuple(bad[0])])), hex(int(want[tuple(bad[0])])))
    assert got.tobytes() == want.tobytes()


def _grid_device(tr, capi, g, select=None, n_select=None, xf=None, stream=None, into=None):
    """ls_scene_distance_grid on a device buffer, 0xAB behind the records -> uint64[nz, ny, nx]"""
    import torch
    nx, ny, nz = g.dims
    cells = nx * ny * nz
    d_select = None if select is None else _to_device(np.ascontiguousarray(select, np.uint8))
    d_cells = torch.full((cells * 8 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    if into is not None:
        d_cells[:cells * 8] = _to_device(np.ascontiguousarray(into, np.uint64))
    torch.cuda.synchronize()
    rc = tr.sceneDistanceGridDevice(_desc(capi, g), d_cells.data_ptr(), 0 if select is None else d_select.data_ptr(),
                                    0 if select is None else (len(select) if n_select is None else n_select), xf, stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    c = d_cells.cpu().numpy()
    assert np.all(c[cells * 8:] == 0xAB)
    return c[:cells * 8].copy().view(np.uint64).reshape(nz, ny, nx)


def _grid_host(tr, capi, g, select=None, xf=None, into=None):
    """Tracer.sceneDistanceGrid -> uint64[nz, ny, nx]"""
    rc, dist, geom = tr.sceneDistanceGrid(_desc(capi, g), select=select, sensor_to_grid=xf, into=None if into is None else ref.split(into))
    assert rc == 0 and dist.dtype == np.float32 and geom.dtype == np.uint32
    return ref.words(dist, geom).reshape(dist.shape)


def _want(oracle, g, ml, s, xf=None, select=None, into=None):
    return ref.distance_grid(g, *ref.scene_triangles(oracle, ml, s, xf, select), into=into)


def _queued(tr):
    n = ctypes.c_uint32(0xFFFFFFFF)
    assert tr.L.ls_debug_distance_grid_queued(tr.h, ctypes.byref(n)) == 0
    return n.value


# ---- 1. the golden scene on both engines' handles --------------------------------------------------------------------------------

GOLDEN_GRIDS = (((-10.0, -10.0, -3.0), 0.5, (40, 40, 12), 1.0), ((-40.0, -40.0, -10.0), 1.0, (80, 80, 16), 2.5))
_golden_reference = {}   # computed once, whichever engine asks first


@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_ground_and_ben_on_both_engines_handles(oracle, capi, sensors, meshes, engine):
    """sensor 0000 over ground + ben, the grid in the sensor frame: device and host variant against the reference; every cell
    ls_scene_grid counts lies within half a cell diagonal of the surface, and a cell at rest is counted by nobody"""
    s = sensors["0000"]
    tr = make_tracer(capi, s, engine)
    ml = _ground_ben(tr, oracle, meshes)
    built = tr.info(capi.LS_INFO_RAY_QUERY_BUILT)
    for k, (origin, cell, dims, trunc) in enumerate(GOLDEN_GRIDS):
        g = ref.grid(origin, cell, dims, trunc)
        if k not in _golden_reference:
            _golden_reference[k] = _want(oracle, g, ml, s)
        want = _golden_reference[k]
        got = _grid_device(tr, capi, g)
        _same(got, want)
        _same(_grid_host(tr, capi, g), want)
        dist, geom = ref.split(got)
        assert np.count_nonzero(got != REST) > 50 and set(np.unique(geom)) <= {0, 1, INV}
        assert np.array_equal(geom == INV, np.isposinf(dist)) and np.all(dist[geom != INV] <= g.trunc)
        rc, counts, _ = tr.sceneGrid(capi.SceneGridDesc.make(origin, cell, dims))
        assert rc == 0 and counts.sum() > 0
        half_diagonal = np.nextafter(F(np.sqrt(3.0) / 2.0 * cell), F(np.inf))
        assert np.all(dist[counts > 0] <= half_diagonal), dist[counts > 0].max()
        assert np.all(counts[np.isposinf(dist)] == 0)
    assert set(np.unique(geom)) == {0, 1, INV}                 # the wider grid holds both geometries
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == built      # no hierarchy is touched
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 2. posed geometries, quads, transforms, pose updates, removals --------------------------------------------------------------

POSED_GRID = dict(origin=(-12.0, -12.0, -6.0), cell=0.5, dims=(56, 56, 24), trunc=1.25)


def test_posed_quads_under_transforms_updates_and_removals(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    g = ref.grid(**POSED_GRID)
    plain = _want(oracle, g, ml, s)
    _same(_grid_device(tr, capi, g), plain)
    assert set(np.unique(ref.split(plain)[1])) == {0, 1, 2, INV}
    for xf in (rigid_transform(), rotation(np.random.default_rng(23))):
        want = _want(oracle, g, ml, s, xf=xf)
        assert want.tobytes() != plain.tobytes() and np.count_nonzero(want != REST) > 1000
        _same(_grid_device(tr, capi, g, xf=xf), want)
        _same(_grid_host(tr, capi, g, xf=xf), want)
    # a new pose and a commit: the grid follows
    A = oracle.affine_from_components(np.float32([-2.0, 1.0, 0.75]), np.float32([0.1, 0.3, -0.7]))
    tr.updateGeometryTransform("face", A)
    assert tr.commitScene() == 0
    ml[1] = (1, ml[1][1], ml[1][2], A)
    moved = _want(oracle, g, ml, s)
    assert moved.tobytes() != plain.tobytes()
    _same(_grid_device(tr, capi, g), moved)
    # a removal: the geomIDs are sparse, the free id's table entry is empty
    assert tr.removeGeometry("face") >= 0
    assert tr.commitScene() == 0
    sparse = _want(oracle, g, [ml[0], ml[2]], s)
    assert set(np.unique(ref.split(sparse)[1])) == {0, 2, INV}
    _same(_grid_device(tr, capi, g), sparse)
    _same(_grid_host(tr, capi, g, select=[1, 1, 0]), _want(oracle, g, [ml[0]], s))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 3. synthetic meshes built for the work split ---------------------------------------------------------------------------------

SPLIT_TRUNC = 1.0   # two cells of SPLIT_GRID


def _run_split(oracle, capi, s, geoms, expect_cells=None, expect_queued=None):
    """commit the triangle lists of `geoms` as one geometry each (geomIDs in order) under the unposed sensor; the device grid and the
    host variant against the reference; the queue's length against the reference's ranges -> the grid"""
    g = ref.grid(trunc=SPLIT_TRUNC, **SPLIT_GRID)
    tr = make_tracer(capi, s)
    ml = []
    for k, tris in enumerate(geoms):
        verts, idx = _mesh(tris)
        _add(tr, "m%d" % k, verts, idx)
        ml.append((k, verts, idx, oracle.IDENTITY_AFFINE))
    for k in reversed(range(len(geoms))):
        tr.updateGeometry("m%d" % k, oracle.IDENTITY_AFFINE, ml[k][1], ml[k][2])
    assert tr.commitScene() == 0
    T, G = ref.scene_triangles(oracle, ml, s)
    assert np.array_equal(T.view(np.uint32), np.concatenate([m[1][m[2]] for m in ml]).view(np.uint32))   # (the unposed sensor moves no bit)
    cells = ref.range_cells(g, T)
    if expect_cells is not None:
        assert cells.tolist() == list(expect_cells), cells.tolist()
    want = ref.distance_grid(g, T, G)
    got = _grid_device(tr, capi, g)
    _same(got, want)
    assert _queued(tr) == np.count_nonzero(cells > SMALL)
    if expect_queued is not None:
        assert _queued(tr) == expect_queued
    _same(_grid_host(tr, capi, g), want)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
    return got


def test_ranges_on_both_sides_of_the_threshold(oracle, capi, sensors):
    """widened ranges of exactly SMALL - 1, SMALL and SMALL + 1 cells (5246 = 43 x 61 x 2, 5247 = 33 x 53 x 3, 5248 = 32 x 41 x 4: the
    band of two cells reaches two, three and all four layers from triangles in layer -1, 0 and 1) and a small one (16 x 16 x 4); a
    triangle over the whole grid and one over most of it, both of more chunks of 256 cells than k_distance_grid_big's gridDim.y; one
    half outside; triangles wholly outside on each of the six sides but within trunc, and beyond it; a triangle without area"""
    s = _unposed(sensors["0000"])
    assert SMALL == 5247
    tris = [_span(2, 2, 39, 57, z=-0.5), _span(2, 2, 29, 49, z=0.5), _span(2, 2, 28, 37, z=1.5), _span(46, 20, 12, 12, z=1.5)]
    got = _run_split(oracle, capi, s, [tris], expect_cells=[5246, 5247, 5248, 1024], expect_queued=1)
    dist, geom = ref.split(got)
    assert dist[0, 2, 2] == 0.0 and dist[1, 2, 2] == 0.0 and dist[1, 20, 46] == 0.0           # corners at cell centres
    assert dist[0, 50, 5] == F(0.5) and np.all(np.isposinf(dist[3, 45:, :40]))                 # one cell above the lowest triangle alone; nothing near the top there
    # the whole grid (64 chunks of 256 cells: more than BIG_Y), tilted through all four layers; a flat one of 53 chunks
    whole = [_at(-1.0, -1.0, 0.25), _at(140.0, -1.0, 4.0), _at(-1.0, 140.0, 7.75)]
    flat = [_at(0.5, 0.5, 2.5), _at(55.5, 0.5, 2.5), _at(0.5, 55.5, 2.5)]
    assert 64 * 64 * 4 // 256 > BIG_Y and 58 * 58 * 4 // 256 > BIG_Y
    got = _run_split(oracle, capi, s, [[whole, flat]], expect_cells=[64 * 64 * 4, 58 * 58 * 4], expect_queued=2)
    assert np.count_nonzero(got != REST) >= 64 * 64
    # half outside; outside on each side within trunc (1.5 cells from the outermost centres); a triangle without area among them
    near = [[_at(-5.5, 30.5, 1.5), _at(5.5, 30.5, 1.5), _at(5.5, 33.5, 1.5)],
            [_at(-1.0, 5.0, 0.5), _at(-1.0, 9.0, 0.5), _at(-1.0, 5.0, 3.5)], [_at(65.0, 15.0, 0.5), _at(65.0, 19.0, 0.5), _at(65.0, 15.0, 3.5)],
            [_at(25.0, -1.0, 0.5), _at(29.0, -1.0, 0.5), _at(25.0, -1.0, 3.5)], [_at(35.0, 65.0, 0.5), _at(39.0, 65.0, 0.5), _at(35.0, 65.0, 3.5)],
            [_at(45.0, 45.0, -1.0), _at(49.0, 45.0, -1.0), _at(45.0, 49.0, -1.0)], [_at(55.0, 55.0, 5.0), _at(59.0, 55.0, 5.0), _at(55.0, 59.0, 5.0)],
            [_at(20.5, 20.5, 1.5), _at(24.5, 22.5, 2.5), _at(24.5, 22.5, 2.5)]]
    got = _run_split(oracle, capi, s, [near], expect_queued=0)
    dist, _ = ref.split(got)
    assert dist[1, 30, 0] < 1e-5 and dist[1, 6, 0] == F(0.75) and dist[1, 16, 63] == F(0.75) and dist[1, 0, 26] == F(0.75) and dist[1, 63, 36] == F(0.75)
    assert dist[0, 46, 46] == F(0.75) and dist[3, 56, 56] == F(0.75)
    assert np.all(np.isposinf(dist[:, 18:26, 18:27]))                                          # the segment marks nothing
    # ... and beyond trunc on each side: inside the widened range by a quarter cell, or outside it altogether
    far = [[_at(-1.75, 5.0, 0.5), _at(-1.75, 9.0, 0.5), _at(-1.75, 5.0, 3.5)], [_at(69.0, 15.0, 0.5), _at(69.0, 19.0, 0.5), _at(69.0, 15.0, 3.5)],
           [_at(25.0, -1.75, 0.5), _at(29.0, -1.75, 0.5), _at(25.0, -1.75, 3.5)], [_at(35.0, 65.75, 0.5), _at(39.0, 65.75, 0.5), _at(35.0, 65.75, 3.5)],
           [_at(45.0, 45.0, -5.0), _at(49.0, 45.0, -5.0), _at(45.0, 49.0, -5.0)], [_at(55.0, 55.0, 5.75), _at(59.0, 55.0, 5.75), _at(55.0, 59.0, 5.75)]]
    got = _run_split(oracle, capi, s, [far], expect_queued=0)
    assert np.all(got == REST)


@pytest.mark.parametrize("n_queued", [1, 63, 64, 65, 200])
def test_queued_triangles_between_small_ones(oracle, capi, sensors, n_queued):
    """n_queued triangles whose widened ranges exceed the threshold (37 x 37 x 4 = 5476 cells and more), between small ones (6 x 7 x 4):
    every one of them gets a slot of its own in the queue"""
    s = _unposed(sensors["0000"])
    rng = np.random.default_rng(n_queued)
    tris, cells = [], []
    for k in range(n_queued):
        for _ in range(int(rng.integers(0, 3))):             # small ones in between
            x, y = int(rng.integers(2, 58)), int(rng.integers(2, 58))
            tris.append(_span(x, y, 2, 3, z=1.5 + (k % 2)))
            cells.append(6 * 7 * 4)
        wx, wy = 33 + k % 7, 33 + k % 5
        tris.append(_span(2 + (5 * k) % 20, 2 + (11 * k) % 20, wx, wy, z=1.5 + (k % 2)))
        cells.append((wx + 4) * (wy + 4) * 4)
    assert sum(c > SMALL for c in cells) == n_queued and min(c for c in cells if c > SMALL) == 5476
    _run_split(oracle, capi, s, [tris], expect_cells=cells, expect_queued=n_queued)


# ---- 4. ties and contention ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_same", [64, 65, 200])
def test_identical_triangles_name_the_lowest_geom(oracle, capi, sensors, n_same):
    """n_same identical triangles spread over three geometries, the vertex data uploaded in descending geomID order and most of the
    copies in the highest one: every cell they reach holds the one distance and geomID 0"""
    s = _unposed(sensors["0000"])
    one = [_at(10.25, 20.25, 1.5), _at(13.5, 20.25, 1.75), _at(10.25, 23.5, 2.0)]
    got = _run_split(oracle, capi, s, [[one] * 2, [one] * 5, [one] * (n_same - 7)], expect_cells=[8 * 8 * 4] * n_same, expect_queued=0)
    dist, geom = ref.split(got)
    assert np.count_nonzero(geom == 0) > 100 and set(np.unique(geom)) == {0, INV}
    alone = _run_split(oracle, capi, s, [[one]])
    _same(got, alone)


def test_equal_distances_from_two_plates_and_another_order_of_adding(oracle, capi, sensors, meshes):
    """two parallel plates of different geometries, half a cell above and below a layer of cell centres: equal distance bits there,
    the lower geomID; then the posed scene committed with its geometries added in another order: the same distances and, per cell,
    the geomID of the same body wherever one body alone attains the distance"""
    s = _unposed(sensors["0000"])
    plate = lambda z: [[_at(10.0, 10.0, z), _at(20.0, 10.0, z), _at(10.0, 20.0, z)], [_at(20.0, 10.0, z), _at(20.0, 20.0, z), _at(10.0, 20.0, z)]]
    got = _run_split(oracle, capi, s, [plate(2.0), plate(1.0)])
    dist, geom = ref.split(got)
    assert np.all(dist[1, 10:20, 10:20] == F(0.25)) and np.all(geom[1, 10:20, 10:20] == 0)    # both plates at 0.25: the lower geomID
    assert np.all(dist[0, 10:20, 10:20] == F(0.25)) and np.all(geom[0, 10:20, 10:20] == 1)    # the lower plate alone
    assert np.all(dist[2, 10:20, 10:20] == F(0.25)) and np.all(geom[2, 10:20, 10:20] == 0)
    s = sensors["0000"]
    g = ref.grid(**POSED_GRID)
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    first = _grid_device(tr, capi, g)
    _same(first, _want(oracle, g, ml, s))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
    names, order = ("ground", "face", "plate"), (2, 0, 1)          # the plate becomes geomID 0, the ground 1, ben 2
    tr = make_tracer(capi, s)
    ml2 = []
    for new_id, body in enumerate(order):
        _, verts, elems, A = ml[body]
        _add(tr, names[body], verts, elems, capi.LS_GEOMETRY_TYPE_QUAD if elems.shape[1] == 4 else 0)
        ml2.append((new_id, verts, elems, A))
    for new_id, body in enumerate(order):
        tr.updateGeometry(names[body], ml2[new_id][3], ml2[new_id][1], ml2[new_id][2])
    assert tr.commitScene() == 0
    second = _grid_device(tr, capi, g)
    _same(second, _want(oracle, g, ml2, s))
    d1, g1 = ref.split(first)
    d2, g2 = ref.split(second)
    assert np.array_equal(d1.view(np.uint32), d2.view(np.uint32))
    # the bodies that attain each cell's distance, from the reference's grid of each body alone
    each = np.stack([ref.split(_want(oracle, g, [ml[b]], s))[0] for b in range(3)])
    attains = each.view(np.uint32) == d1.view(np.uint32)[None]
    single = (attains.sum(axis=0) == 1) & (g1 != INV)
    assert np.count_nonzero(single) > 1000
    body_of_second = np.array(order)[np.minimum(g2, 2)]
    assert np.array_equal(g1[single], body_of_second[single]) and np.array_equal(g1 == INV, g2 == INV)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 5. the selection ------------------------------------------------------------------------------------------------------------

def test_select_splits_the_grid_by_geometry(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    g = ref.grid(**POSED_GRID)
    full = _grid_device(tr, capi, g)
    _same(full, _want(oracle, g, ml, s))
    lowest = np.full_like(full, REST)
    for k in range(3):
        sel = [int(j == k) for j in range(3)]
        part = _grid_device(tr, capi, g, select=sel)
        _same(part, _want(oracle, g, ml, s, select=sel))
        assert set(np.unique(ref.split(part)[1])) == {k, INV}
        lowest = np.minimum(lowest, part)
    _same(lowest, full)                                       # the minimum of the parts, as 64-bit words
    # n_select below the highest geomID: the geometries beyond it are selected
    _same(_grid_device(tr, capi, g, select=[0, 1]), _want(oracle, g, ml, s, select=[0, 1, 1]))
    _same(_grid_device(tr, capi, g, select=[0]), _want(oracle, g, ml, s, select=[0, 1, 1]))
    _same(_grid_device(tr, capi, g, select=[1, 0, 0, 0, 1, 1]), _want(oracle, g, ml, s, select=[1, 0, 0]))   # ... and bytes beyond the table are not read as geometries
    assert np.all(_grid_device(tr, capi, g, select=[0, 0, 0]) == REST)
    _same(_grid_host(tr, capi, g, select=[0, 1, 0]), _want(oracle, g, ml, s, select=[0, 1, 0]))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 6. accumulation -------------------------------------------------------------------------------------------------------------

def test_accumulate_takes_the_minimum_of_words(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    xa = rigid_transform()
    xb = np.array([np.cos(0.7), -np.sin(0.7), 0, 0.3, np.sin(0.7), np.cos(0.7), 0, -0.2, 0, 0, 1, 0.1], np.float32)   # a turn about z, rounded
    gd = dict(POSED_GRID)
    g, ga = ref.grid(**gd), ref.grid(flags=ACCUMULATE, **gd)
    wa, wb = _want(oracle, g, ml, s, xf=xa, select=[0, 1, 1]), _want(oracle, g, ml, s, xf=xb)
    both = np.minimum(wa, wb)
    assert np.any((both == wa) & (wa != wb)) and np.any((both == wb) & (wa != wb)) and np.count_nonzero(wa != REST) > 1000
    first = _grid_device(tr, capi, g, select=[0, 1, 1], xf=xa)
    _same(first, wa)
    _same(_grid_device(tr, capi, ga, xf=xb, into=first), both)
    _same(_want(oracle, ga, ml, s, xf=xb, into=wa), both)
    # whatever the words hold, they are compared as words: a NaN's bits lie above every distance's, a zero word below
    odd = first.copy()
    odd[0, 0, :4] = [0, 0x7FC0000000000005, 0xFFFFFFFFFFFFFFFF, 0x8000000000000001]
    _same(_grid_device(tr, capi, ga, xf=xb, into=odd), np.minimum(odd, wb))
    # without the flag the second call overwrites what the buffer held
    _same(_grid_device(tr, capi, g, xf=xb, into=first), wb)
    # the host variant: `into` sets the flag, the array travels both ways; the caller's arrays stay as they were
    keep = first.copy()
    kd, kg = ref.split(first)
    kd0, kg0 = kd.copy(), kg.copy()
    rc, dist, geom = tr.sceneDistanceGrid(_desc(capi, g), sensor_to_grid=xb, into=(kd, kg))
    assert rc == 0
    _same(ref.words(dist, geom).reshape(dist.shape), both)
    assert np.array_equal(kd.view(np.uint32), kd0.view(np.uint32)) and np.array_equal(kg, kg0) and np.array_equal(first, keep)
    # accumulating on a cleared array is the plain call
    _same(_grid_host(tr, capi, g, select=[0, 1, 1], xf=xa, into=np.full_like(wa, REST)), wa)
    _same(_grid_device(tr, capi, ga, select=[0, 1, 1], xf=xa, into=np.full_like(wa, REST)), wa)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 8. plumbing -----------------------------------------------------------------------------------------------------------------

def test_entry_points(oracle, capi, sensors, meshes):
    """a caller stream; the host variant on unaligned pageable memory with guards; a 1 x 1 x 1 grid and a 2048 x 1 x 1 grid; the refusals
    of the device entry point in their order, nothing written; no commit: -1 and nothing written"""
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    g = ref.grid(**POSED_GRID)
    want = _want(oracle, g, ml, s)
    st = torch.cuda.Stream()
    _same(_grid_device(tr, capi, g, stream=st.cuda_stream), want)
    # the host variant on unaligned pageable memory, a guard around the output and the selection
    L, h = tr.L, tr.h
    nx, ny, nz = g.dims
    cells = nx * ny * nz
    d = _desc(capi, g)

    def unaligned(a, shift):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = np.full(b.size + 64, 0xAB, np.uint8)
        off = (-buf.ctypes.data) % 16 + shift
        buf[off:off + b.size] = b
        return buf, off
    hc, o_c = unaligned(np.zeros(cells, np.uint64), 5)
    hs, o_s = unaligned(np.array([1, 0, 1], np.uint8), 3)
    hc[:] = 0xAB
    part = _want(oracle, g, ml, s, select=[1, 0, 1])
    assert L.ls_scene_distance_grid_host(h, ctypes.byref(d), None, hs.ctypes.data + o_s, 3, hc.ctypes.data + o_c) == 0
    assert hc[o_c:o_c + cells * 8].tobytes() == part.tobytes()
    assert np.all(hc[:o_c] == 0xAB) and np.all(hc[o_c + cells * 8:] == 0xAB)
    # ... and accumulating there: the array travels both ways
    da = _desc(capi, ref.grid(flags=ACCUMULATE, **POSED_GRID))
    assert L.ls_scene_distance_grid_host(h, ctypes.byref(da), None, None, 0, hc.ctypes.data + o_c) == 0
    assert hc[o_c:o_c + cells * 8].tobytes() == want.tobytes() and np.all(hc[:o_c] == 0xAB) and np.all(hc[o_c + cells * 8:] == 0xAB)
    # one cell around the plate's middle; 2048 cells in a row through ben and the plate
    T, G = ref.scene_triangles(oracle, ml, s)
    mid = T[G == 2].reshape(-1, 3).mean(axis=0)
    g1 = ref.grid(tuple(mid - F(1.0)), 2.0, (1, 1, 1), 1.5)
    w1 = ref.distance_grid(g1, T, G)
    assert ref.split(w1)[1][0, 0, 0] == 2 and ref.split(w1)[0][0, 0, 0] < 0.5
    _same(_grid_device(tr, capi, g1), w1)
    row = ref.grid((-40.0, float(mid[1]) - 0.5, float(mid[2]) - 0.5), 0.0625, (2048, 1, 1), 0.5)
    wrow = ref.distance_grid(row, T, G)
    assert np.count_nonzero(wrow != REST) > 16
    _same(_grid_device(tr, capi, row), wrow)
    # refusals, nothing written
    out = torch.full((cells * 8 + 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_sel = _to_device(np.array([1, 1, 1], np.uint8))
    torch.cuda.synchronize()
    xf = rigid_transform()

    def call(handle=h, grid=d, **kw):
        a = dict(xf=None, select=d_sel.data_ptr(), n_select=3, cells=out.data_ptr())
        a.update(kw)
        return L.ls_scene_distance_grid(handle, None, None if grid is None else ctypes.byref(grid), a["xf"], a["select"], a["n_select"], a["cells"])

    def desc(**kw):
        dd = _desc(capi, g)
        for k, v in kw.items():
            if k in ("origin", "dims", "reserved"):
                for j, x in enumerate(v):
                    getattr(dd, k)[j] = x
            else:
                setattr(dd, k, v)
        return dd
    nan = float("nan")
    bad_xf = xf.copy()
    bad_xf[7] = np.inf
    assert call(grid=None) == INVALID_ARGUMENT
    assert call(cells=None) == INVALID_ARGUMENT
    assert call(select=None) == INVALID_ARGUMENT
    assert call(grid=desc(flags=2)) == INVALID_ARGUMENT and call(grid=desc(flags=0x80000001)) == INVALID_ARGUMENT
    assert call(grid=desc(reserved=(0, 1, 0))) == INVALID_ARGUMENT
    assert call(grid=desc(origin=(0.0, nan, 0.0))) == INVALID_ARGUMENT and call(xf=bad_xf.ctypes.data) == INVALID_ARGUMENT
    assert call(grid=desc(cell=0.0)) == INVALID_ARGUMENT and call(grid=desc(cell=nan)) == INVALID_ARGUMENT
    assert call(grid=desc(trunc=nan)) == INVALID_ARGUMENT and call(grid=desc(trunc=-1.0)) == INVALID_ARGUMENT
    assert call(cells=out.data_ptr() + 8) == INVALID_ARGUMENT
    assert call(grid=desc(dims=(0, 8, 6))) == OUT_OF_RANGE and call(grid=desc(dims=(2049, 1, 1))) == OUT_OF_RANGE
    assert call(grid=desc(dims=(2048, 2048, 33))) == OUT_OF_RANGE
    assert call(grid=desc(origin=(3e38, 0.0, 0.0), cell=1e35, dims=(2048, 1, 1))) == OUT_OF_RANGE
    assert call(grid=desc(trunc=16.0)) == 0 and call(grid=desc(trunc=float(np.nextafter(F(16.0), F(np.inf))))) == OUT_OF_RANGE
    tr.synchronize()
    torch.cuda.synchronize()
    out[:] = 0xAB                                              # (the one call among them that was accepted wrote its grid)
    torch.cuda.synchronize()
    # the earlier refusal answers: a misaligned pointer before a dimension or the band, a bad trunc before a misaligned pointer
    assert call(grid=desc(dims=(0, 8, 6)), cells=out.data_ptr() + 8) == INVALID_ARGUMENT
    assert call(grid=desc(trunc=17.0), cells=out.data_ptr() + 8) == INVALID_ARGUMENT
    assert call(grid=desc(trunc=nan, dims=(0, 8, 6)), cells=out.data_ptr() + 8) == INVALID_ARGUMENT
    assert L.ls_scene_distance_grid_host(h, ctypes.byref(desc(flags=8)), None, None, 0, hc.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_scene_distance_grid_host(h, ctypes.byref(d), None, None, 2, hc.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_scene_distance_grid_host(h, ctypes.byref(d), None, None, 0, None) == INVALID_ARGUMENT
    assert L.ls_scene_distance_grid_host(h, ctypes.byref(desc(dims=(1, 1, 0))), None, None, 0, hc.ctypes.data) == OUT_OF_RANGE
    assert L.ls_scene_distance_grid_host(h, ctypes.byref(desc(trunc=16.5)), None, None, 0, hc.ctypes.data) == OUT_OF_RANGE
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
    # no commit: the descriptor's refusals still come first; then -1, nothing written
    t2 = make_tracer(capi, s)
    assert call(handle=t2.h, grid=desc(dims=(0, 8, 6))) == OUT_OF_RANGE and call(handle=t2.h, cells=out.data_ptr() + 4) == INVALID_ARGUMENT
    assert t2.sceneDistanceGridDevice(d, out.data_ptr()) == -1
    keep = hc.copy()
    assert t2.L.ls_scene_distance_grid_host(t2.h, ctypes.byref(d), None, None, 0, hc.ctypes.data + o_c) == -1
    assert np.array_equal(hc, keep)
    rc, dist, geom = t2.sceneDistanceGrid(d)
    assert rc == -1 and np.all(np.isposinf(dist)) and np.all(geom == INV) and dist.shape == (nz, ny, nx) and geom.shape == (nz, ny, nx)
    t2.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB)
    assert t2.info(capi.LS_INFO_DEVICE_STATUS) == 0
    t2.close()


def test_open_frame_graph_is_refused(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0001"]
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    tr.setOption(capi.LS_OPT_FRAME_GRAPH, 1)
    ml = _ground_ben(tr, oracle, meshes)
    cap = s.V * s.H
    p, h, c = (torch.zeros(32 * cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * cap, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), cap)
    g = ref.grid((-30.0, -30.0, -8.0), 1.0, (60, 60, 12), 2.0)
    d = _desc(capi, g)
    cells = 60 * 60 * 12
    out = torch.full((cells * 8,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != FRAME_EAGER   # the frame is being captured: the graph is open
    assert L.ls_scene_distance_grid(tr.h, None, ctypes.byref(d), None, None, 0, out.data_ptr()) == INVALID_ARGUMENT
    assert L.ls_scene_distance_grid_host(tr.h, None, None, None, 0, None) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB)
    # the graph is closed: the call works
    assert tr.sceneDistanceGridDevice(d, out.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    want = _want(oracle, g, ml, s)
    _same(out.cpu().numpy().view(np.uint64).reshape(12, 60, 60), want)
    assert np.count_nonzero(want != REST) > 1000
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 7. against ls_closest_points, device against device (last: it builds the hierarchies) ----------------------------------------

def test_against_closest_points_over_the_cell_centres(oracle, capi, sensors, meshes):
    """the grid's origin exactly (0, 0, 0) and no transform: q = v bit for bit, so a cell centre's distance is what ls_closest_points
    finds from the same point with radius +inf -- the same bits wherever that is within trunc, a record at rest elsewhere; the geomID
    is never above the query's, and equal wherever one geometry alone attains the distance.  The sensor stands unposed at the world's
    origin, so that the octant the grid covers holds the plate, a part of ben and a quarter of the ground"""
    s = _unposed(sensors["0000"])
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    g = ref.grid((0.0, 0.0, 0.0), 0.5, (28, 24, 10), 1.0)
    nx, ny, nz = g.dims
    got = _grid_device(tr, capi, g)
    _same(got, _want(oracle, g, ml, s))
    each = np.stack([ref.split(_grid_device(tr, capi, g, select=[int(j == k) for j in range(3)]))[0] for k in range(3)])
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pts = np.zeros((nz * ny * nx, 4), np.float32)
    for a, c in enumerate((x, y, z)):
        pts[:, a] = ((c.reshape(-1).astype(np.float32) + F(0.5)) * g.cell)
    pts[:, 3] = np.inf
    rc, near = tr.closestPoints(pts)
    assert rc == 0 and np.all(np.isfinite(near["dist"])) and np.all(near["geom"] != INV)
    qd, qg = near["dist"].reshape(nz, ny, nx), near["geom"].reshape(nz, ny, nx)
    dist, geom = ref.split(got)
    within = qd <= g.trunc
    assert np.count_nonzero(within) > 500 and np.count_nonzero(~within) > 500
    assert np.array_equal(dist[within].view(np.uint32), qd[within].view(np.uint32))
    assert np.all(got[~within] == REST)
    assert np.all(geom[within] <= qg[within])
    single = within & ((each.view(np.uint32) == dist.view(np.uint32)[None]).sum(axis=0) == 1)
    assert np.count_nonzero(single) > 400 and np.array_equal(geom[single], qg[single])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
