"""ls_scene_grid / ls_scene_grid_host on the MI355X: per cell of a voxel grid the triangles of the committed scene that overlap it and
the lowest geomID among them, against the numpy restatement of tests/scene_grid_reference.py, byte for byte -- the golden scene on
both engines' handles, posed geometries and quads under transforms, pose updates and removals, a synthetic mesh built for the split
between the lane-per-triangle kernel and the queued one, the selection, accumulation, and the entry points' plumbing.  Nothing here
is compared against ls_debug_scene_grid_triangle."""
import ctypes
import dataclasses

import numpy as np
import pytest

import scene_grid_reference as ref
from conftest import make_tracer
from test_gpu_labels import _to_device
from test_gpu_rays import INV, _add, _ground_ben, _scene_posed_quads
from test_occupancy_cpu import rigid_transform, rotation

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = -2                      # LS_ERR_INVALID_ARGUMENT
OUT_OF_RANGE = -9                          # LS_ERR_OUT_OF_RANGE
FRAME_EAGER = 0                            # LS_FRAME_EAGER
GUARD = 256
ACCUMULATE = ref.ACCUMULATE
SMALL = 64                                 # kSceneGridSmall as shipped; 8 and 512 are the other candidates of the tunable
BIG_Y = 32                                 # kSceneGridBigY: gridDim.y of k_scene_grid_big
F = np.float32

# torch fills a new tensor on its own stream, the library works on the handle's: every buffer is filled (a device-wide
# synchronize) before the library gets it


def _desc(capi, g):
    return capi.SceneGridDesc.make(g.origin, g.cell, g.dims, g.flags)


def _same(got, want):
    """(counts, geom) pairs, byte for byte"""
    assert got[0].dtype == np.uint32 and got[0].shape == want[0].shape
    bad = np.argwhere(got[0] != want[0])
    assert bad.shape[0] == 0, ("counts", bad.shape[0], bad[:5], got[0][tuple(bad[0])], want[0][tuple(bad[0])])
    assert got[0].tobytes() == want[0].tobytes()
    if got[1] is not None:
        assert got[1].dtype == np.uint32 and got[1].shape == want[1].shape
        assert np.array_equal(got[1], want[1]), "geom"
        assert got[1].tobytes() == want[1].tobytes()


def _grid_device(tr, capi, g, select=None, n_select=None, xf=None, stream=None, with_geom=True, into=None):
    """ls_scene_grid on device buffers, 0xAB behind both outputs -> (counts uint32[nz, ny, nx], geom uint32[nz, ny, nx] or None)"""
    import torch
    nx, ny, nz = g.dims
    cells = nx * ny * nz
    d_select = None if select is None else _to_device(np.ascontiguousarray(select, np.uint8))
    d_counts = torch.full((cells * 4 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_geom = torch.full((cells * 4 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    if into is not None:
        d_counts[:cells * 4] = _to_device(np.ascontiguousarray(into[0], np.uint32))
        d_geom[:cells * 4] = _to_device(np.ascontiguousarray(into[1], np.uint32))
    torch.cuda.synchronize()
    rc = tr.sceneGridDevice(_desc(capi, g), d_counts.data_ptr(), d_geom.data_ptr() if with_geom else 0, 0 if select is None else d_select.data_ptr(),
                            0 if select is None else (len(select) if n_select is None else n_select), xf, stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    c, gm = d_counts.cpu().numpy(), d_geom.cpu().numpy()
    assert np.all(c[cells * 4:] == 0xAB) and np.all(gm[cells * 4:] == 0xAB)
    if not with_geom:
        assert np.all(gm == 0xAB)
    return c[:cells * 4].copy().view(np.uint32).reshape(nz, ny, nx), gm[:cells * 4].copy().view(np.uint32).reshape(nz, ny, nx) if with_geom else None


def _want(oracle, g, ml, s, xf=None, select=None, into=None):
    return ref.scene_grid(g, *ref.scene_triangles(oracle, ml, s, xf, select), into=into)


def _dilate(b):
    """a boolean grid OR-ed over every cell's 3 x 3 x 3 neighbourhood"""
    p = np.pad(b, 1)
    out = np.zeros_like(b)
    nz, ny, nx = b.shape
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= p[dz:dz + nz, dy:dy + ny, dx:dx + nx]
    return out


# ---- 1. the golden scene on both engines' handles --------------------------------------------------------------------------------

GOLDEN_GRIDS = (((-10.0, -10.0, -3.0), 0.5, (40, 40, 12)), ((-40.0, -40.0, -10.0), 1.0, (80, 80, 16)))
_golden_reference = {}   # computed once, whichever engine asks first


@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_ground_and_ben_on_both_engines_handles(oracle, capi, sensors, meshes, engine):
    """sensor 0000 over ground + ben, the grid in the sensor frame: a 40 x 40 x 12 grid of 0.5 m cells around the sensor, which holds a
    part of ben, and an 80 x 80 x 16 grid of 1 m cells, which also holds the ground, whose triangles span hundreds of cells each; with
    and without d_geom.  On the second grid the frame's own returns (ls_occupancy_grid) fall next to the surface that made them."""
    s = sensors["0000"]
    tr = make_tracer(capi, s, engine)
    ml = _ground_ben(tr, oracle, meshes)
    built = tr.info(capi.LS_INFO_RAY_QUERY_BUILT)
    for k, (origin, cell, dims) in enumerate(GOLDEN_GRIDS):
        g = ref.grid(origin, cell, dims)
        if k not in _golden_reference:
            _golden_reference[k] = _want(oracle, g, ml, s)
        want = _golden_reference[k]
        got = _grid_device(tr, capi, g)
        _same(got, want)
        assert got[0].sum() > 0 and set(np.unique(got[1])) <= {0, 1, INV}
        assert np.array_equal(got[1] != INV, got[0] > 0)
        c, none = _grid_device(tr, capi, g, with_geom=False)
        assert none is None and c.tobytes() == want[0].tobytes()
        rc, counts, geom = tr.sceneGrid(_desc(capi, g))
        assert rc == 0
        _same((counts, geom), want)
    assert set(np.unique(got[1])) == {0, 1, INV}              # the wider grid holds both geometries
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == built      # no hierarchy is touched
    # the frame on the same grid: every cell a return fell in has surface in its 3 x 3 x 3 neighbourhood
    rc, pts, hits = tr.traceScene(0)
    assert rc == 0 and hits.shape[0] == 1781
    rc, occ, _ = tr.occupancyGrid(capi.OccupancyGridDesc.make(origin, cell, dims, 0, 0.0, 1e4), hits)
    assert rc == 0 and np.count_nonzero(occ[..., 1]) > 300
    assert np.all(_dilate(got[0] > 0)[occ[..., 1] > 0])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 2. posed geometries, quads, transforms, pose updates, removals --------------------------------------------------------------

POSED_GRID = dict(origin=(-20.0, -20.0, -9.0), cell=0.5, dims=(80, 80, 24))


def test_posed_quads_under_transforms_updates_and_removals(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    g = ref.grid(**POSED_GRID)
    plain = _want(oracle, g, ml, s)
    _same(_grid_device(tr, capi, g), plain)
    assert set(np.unique(plain[1])) == {0, 1, 2, INV}
    # the plate's 24 quads count as 48 triangles: its grid alone, against the reference's two triangles per quad
    only = _want(oracle, g, ml, s, select=[0, 0, 1])
    assert only[0].sum() >= 48 and set(np.unique(only[1])) == {2, INV}
    _same(_grid_device(tr, capi, g, select=[0, 0, 1]), only)
    for xf in (rigid_transform(), rotation(np.random.default_rng(23))):
        want = _want(oracle, g, ml, s, xf=xf)
        assert want[0].tobytes() != plain[0].tobytes() and want[0].sum() > 0
        _same(_grid_device(tr, capi, g, xf=xf), want)
        rc, counts, geom = tr.sceneGrid(_desc(capi, g), sensor_to_grid=xf)
        assert rc == 0
        _same((counts, geom), want)
    # a new pose and a commit: the grid follows
    A = oracle.affine_from_components(np.float32([-2.0, 1.0, 0.75]), np.float32([0.1, 0.3, -0.7]))
    tr.updateGeometryTransform("face", A)
    assert tr.commitScene() == 0
    ml[1] = (1, ml[1][1], ml[1][2], A)
    moved = _want(oracle, g, ml, s)
    assert moved[0].tobytes() != plain[0].tobytes()
    _same(_grid_device(tr, capi, g), moved)
    # a removal: the geomIDs are sparse, the free id's table entry is empty
    assert tr.removeGeometry("face") >= 0
    assert tr.commitScene() == 0
    sparse = _want(oracle, g, [ml[0], ml[2]], s)
    assert set(np.unique(sparse[1])) == {0, 2, INV}
    _same(_grid_device(tr, capi, g), sparse)
    rc, counts, geom = tr.sceneGrid(_desc(capi, g), select=[1, 1, 0])
    assert rc == 0
    _same((counts, geom), _want(oracle, g, [ml[0]], s))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 3. a synthetic mesh built for the work split --------------------------------------------------------------------------------

SPLIT_GRID = dict(origin=(-16.0, -16.0, -1.0), cell=0.5, dims=(64, 64, 4))


def _unposed(s):
    """the sensor standing at the world's origin, unrotated: a vertex reaches the grid's frame as it was uploaded, bit for bit"""
    eye = np.eye(3, dtype=np.float32).reshape(9)
    return dataclasses.replace(s, R=eye, Rinv=eye.copy(), t=np.zeros(3, np.float32))


def _at(x, y, z):
    """a point given in cells of SPLIT_GRID (exact: the cell is a power of two)"""
    return [-16.0 + 0.5 * x, -16.0 + 0.5 * y, -1.0 + 0.5 * z]


def _span(x0, y0, wx, wy, z=1.5):
    """a triangle whose range is exactly wx x wy x 1 cells from cell (x0, y0): its corners at cell centres"""
    return [_at(x0 + 0.5, y0 + 0.5, z), _at(x0 + wx - 0.5, y0 + 0.5, z), _at(x0 + 0.5, y0 + wy - 0.5, z)]


def _mesh(tris):
    v = np.array(tris, np.float32).reshape(-1, 3)
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)


def _run_split(oracle, capi, s, tris, expect_cells=None):
    """commit the triangles as one geometry under the unposed sensor; the device grid and the host variant against the reference
    -> (counts, geom)"""
    g = ref.grid(**SPLIT_GRID)
    verts, idx = _mesh(tris)
    tr = make_tracer(capi, s)
    _add(tr, "m", verts, idx)
    tr.updateGeometry("m", oracle.IDENTITY_AFFINE, verts, idx)
    assert tr.commitScene() == 0
    T, G = ref.scene_triangles(oracle, [(0, verts, idx, oracle.IDENTITY_AFFINE)], s)
    assert np.array_equal(T.view(np.uint32), verts[idx].view(np.uint32))        # (the unposed sensor moves no bit)
    if expect_cells is not None:
        _, ok, lo, hi = ref.ranges(g, T)
        cells = np.where(ok, np.prod(hi - lo + 1, axis=1), 0)
        assert cells.tolist() == list(expect_cells), cells.tolist()
    want = ref.scene_grid(g, T, G)
    got = _grid_device(tr, capi, g)
    _same(got, want)
    rc, counts, geom = tr.sceneGrid(_desc(capi, g))
    assert rc == 0
    _same((counts, geom), want)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
    return got


def test_ranges_on_both_sides_of_the_threshold(oracle, capi, sensors):
    """ranges of exactly SMALL - 1, SMALL and SMALL + 1 cells (63 = 9 x 7, 64 = 8 x 8, 65 = 13 x 5), and the same around the tunable's
    other candidates where a 64 x 64 x 4 grid has room for them (7, 8, 9; 512 = 16 x 32, 513 = 27 x 19); a triangle over the whole grid
    and one over more tiles of 8 x 8 x 8 cells than k_scene_grid_big's gridDim.y; vertices exactly on cell-boundary planes; a segment
    and a point; a triangle half outside, and triangles wholly outside on each side"""
    s = _unposed(sensors["0000"])
    assert SMALL == 64
    shapes = [(9, 7), (8, 8), (13, 5), (7, 1), (8, 1), (9, 1), (16, 32), (27, 19)]
    tris, at = [], 0
    for k, (wx, wy) in enumerate(shapes):
        tris.append(_span(1 + (k % 2) * 30, 1 + at, wx, wy, z=0.5 + (k % 4)))
        at += 7 if k % 2 else 0
    _run_split(oracle, capi, s, tris, expect_cells=[wx * wy for wx, wy in shapes])
    # the whole grid (64 tiles of its range: more than BIG_Y), tilted through all four layers; a flat one over 7 x 7 tiles
    whole = [_at(-1.0, -1.0, 0.25), _at(140.0, -1.0, 4.0), _at(-1.0, 140.0, 7.75)]
    flat = [_at(0.5, 0.5, 2.5), _at(55.5, 0.5, 2.5), _at(0.5, 55.5, 2.5)]
    assert 8 * 8 > BIG_Y and 7 * 7 > BIG_Y
    got = _run_split(oracle, capi, s, [whole, flat], expect_cells=[64 * 64 * 4, 56 * 56])
    assert np.count_nonzero(got[0]) >= 64 * 64 and got[0].max() == 2
    # corners on cell-boundary planes (a face plane belongs to the cell above it), in a face plane, on the grid's own faces
    edge = [[_at(8.0, 8.0, 1.0), _at(12.0, 8.0, 1.0), _at(8.0, 12.0, 1.0)],
            [_at(20.0, 20.0, 2.0), _at(24.0, 20.5, 2.0), _at(20.5, 23.0, 3.0)],
            [_at(0.0, 0.0, 0.0), _at(2.0, 0.0, 0.0), _at(0.0, 2.0, 0.0)],
            [_at(64.0, 64.0, 4.0), _at(62.0, 64.0, 4.0), _at(64.0, 62.0, 4.0)],
            [_at(40.0, 3.5, 1.5), _at(40.0, 6.5, 1.5), _at(40.0, 3.5, 2.5)]]
    got = _run_split(oracle, capi, s, edge)
    assert got[0][1, 8, 8] == 1 and got[0][0, 8, 8] == 0 and got[0][0, 0, 0] == 1 and got[0][3, 63, 63] == 0   # (the grid's upper faces lie outside it)
    # a segment, a point, a triangle half outside, triangles wholly outside on each side
    odd = [[_at(3.5, 40.5, 1.5), _at(30.5, 47.5, 2.5), _at(30.5, 47.5, 2.5)],
           [_at(50.25, 50.25, 0.25)] * 3,
           [_at(-5.5, 30.5, 1.5), _at(5.5, 30.5, 1.5), _at(5.5, 33.5, 1.5)],
           [_at(-9.0, 5.0, 1.5), _at(-2.0, 5.0, 1.5), _at(-2.0, 9.0, 1.5)], [_at(65.0, 5.0, 1.5), _at(69.0, 5.0, 1.5), _at(65.0, 9.0, 1.5)],
           [_at(5.0, -9.0, 1.5), _at(5.0, -2.0, 1.5), _at(9.0, -2.0, 1.5)], [_at(5.0, 65.0, 1.5), _at(5.0, 69.0, 1.5), _at(9.0, 65.0, 1.5)],
           [_at(5.0, 5.0, -3.0), _at(9.0, 5.0, -3.0), _at(5.0, 9.0, -1.5)], [_at(5.0, 5.0, 4.5), _at(9.0, 5.0, 4.5), _at(5.0, 9.0, 7.0)]]
    got = _run_split(oracle, capi, s, odd)
    assert got[0][0, 50, 50] == 1 and got[0][1, 30, 0] == 1 and got[0][1, 40, 3] == 1 and got[0][2, 47, 30] == 1
    assert got[0].sum() < 100


@pytest.mark.parametrize("n_queued", [1, 63, 64, 65, 200])
def test_queued_triangles_of_a_wave(oracle, capi, sensors, n_queued):
    """n_queued triangles whose ranges exceed the threshold (66 = 11 x 6 cells and more), between small ones in a pattern that leaves
    gaps in a wave's ballot: the wave-aggregated append gives every one of them a slot of its own"""
    s = _unposed(sensors["0000"])
    rng = np.random.default_rng(n_queued)
    tris, cells = [], []
    for k in range(n_queued):
        for _ in range(int(rng.integers(0, 3))):             # small ones in between
            x, y = int(rng.integers(0, 60)), int(rng.integers(0, 60))
            tris.append(_span(x, y, 2, 3, z=0.5 + (k % 4)))
            cells.append(6)
        wx, wy = 11 + k % 7, 6 + k % 5
        tris.append(_span((5 * k) % 40, (11 * k) % 50, wx, wy, z=0.5 + (k % 4)))
        cells.append(wx * wy)
    assert sum(c > SMALL for c in cells) == n_queued and min(c for c in cells if c > SMALL) == 66
    _run_split(oracle, capi, s, tris, expect_cells=cells)


@pytest.mark.parametrize("n_tiny", [64, 65, 200])
def test_runs_of_tiny_triangles_in_one_cell(oracle, capi, sensors, n_tiny):
    """identical tiny triangles in one cell, then alternating between two cells: the runs of adjacent lanes that mark the same cell"""
    s = _unposed(sensors["0000"])
    tiny = lambda x, y: [_at(x + 0.25, y + 0.25, 1.5), _at(x + 0.5, y + 0.25, 1.5), _at(x + 0.25, y + 0.5, 1.5)]
    got = _run_split(oracle, capi, s, [tiny(10, 20)] * n_tiny, expect_cells=[1] * n_tiny)
    assert got[0][1, 20, 10] == n_tiny and got[0].sum() == n_tiny
    got = _run_split(oracle, capi, s, [tiny(10, 20) if k % 2 == 0 else tiny(11, 20) for k in range(n_tiny)], expect_cells=[1] * n_tiny)
    assert got[0][1, 20, 10] == (n_tiny + 1) // 2 and got[0][1, 20, 11] == n_tiny // 2
    # runs of three and of one, and a lane in between that marks nothing (a triangle outside the grid)
    mixed = []
    for k in range(n_tiny):
        mixed.append(tiny(10, 20) if k % 5 < 3 else tiny(30, 5) if k % 5 == 3 else tiny(-9, 20))
    got = _run_split(oracle, capi, s, mixed)
    assert got[0][1, 20, 10] == sum(k % 5 < 3 for k in range(n_tiny)) and got[0][1, 5, 30] == sum(k % 5 == 3 for k in range(n_tiny))


# ---- 4. the selection ------------------------------------------------------------------------------------------------------------

def test_select_splits_the_grid_by_geometry(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    g = ref.grid(**POSED_GRID)
    full = _grid_device(tr, capi, g)
    _same(full, _want(oracle, g, ml, s))
    total, lowest = np.zeros_like(full[0]), np.full_like(full[1], INV)
    for k in range(3):
        sel = [int(j == k) for j in range(3)]
        part = _grid_device(tr, capi, g, select=sel)
        _same(part, _want(oracle, g, ml, s, select=sel))
        assert part[0].sum() > 0 and set(np.unique(part[1])) == {k, INV}
        total += part[0]
        lowest = np.minimum(lowest, part[1])
    assert np.array_equal(total, full[0]) and np.array_equal(lowest, full[1])
    # n_select below the highest geomID: the geometries beyond it are selected
    _same(_grid_device(tr, capi, g, select=[0, 1]), _want(oracle, g, ml, s, select=[0, 1, 1]))
    _same(_grid_device(tr, capi, g, select=[0]), _want(oracle, g, ml, s, select=[0, 1, 1]))
    _same(_grid_device(tr, capi, g, select=[1, 0, 0, 0, 1, 1]), _want(oracle, g, ml, s, select=[1, 0, 0]))   # ... and bytes beyond the table are not read as geometries
    none = _grid_device(tr, capi, g, select=[0, 0, 0])
    assert not none[0].any() and np.all(none[1] == INV)
    rc, counts, geom = tr.sceneGrid(_desc(capi, g), select=[0, 1, 0])
    assert rc == 0
    _same((counts, geom), _want(oracle, g, ml, s, select=[0, 1, 0]))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 5. accumulation -------------------------------------------------------------------------------------------------------------

def test_accumulate_adds_counts_and_keeps_the_lowest_geom(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    xa = rigid_transform()
    xb = np.array([np.cos(0.7), -np.sin(0.7), 0, 0.3, np.sin(0.7), np.cos(0.7), 0, -0.2, 0, 0, 1, 0.1], np.float32)   # a turn about z, rounded
    g = ref.grid(**POSED_GRID)
    ga = ref.grid(flags=ACCUMULATE, **POSED_GRID)
    wa, wb = _want(oracle, g, ml, s, xf=xa, select=[0, 1, 1]), _want(oracle, g, ml, s, xf=xb)
    assert wa[0].tobytes() != wb[0].tobytes() and wa[0].sum() > 100 and wb[0].sum() > 100
    total = (wa[0] + wb[0], np.minimum(wa[1], wb[1]))
    assert np.any((wa[1] == 1) & (wb[1] == 0)) and np.any((total[0] > wa[0]) & (wa[0] > 0))
    first = _grid_device(tr, capi, g, select=[0, 1, 1], xf=xa)
    _same(first, wa)
    _same(_grid_device(tr, capi, ga, xf=xb, into=first), total)
    _same(_want(oracle, ga, ml, s, xf=xb, into=wa), total)
    # without the flag the second call overwrites what the buffers held
    _same(_grid_device(tr, capi, g, xf=xb, into=first), wb)
    # the host variant: `into` sets the flag, the arrays travel both ways; the caller's arrays stay as they were
    keep = (first[0].copy(), first[1].copy())
    rc, counts, geom = tr.sceneGrid(_desc(capi, g), sensor_to_grid=xb, into=first)
    assert rc == 0
    _same((counts, geom), total)
    _same(first, keep)
    # accumulating on a cleared pair is the plain call
    rc, counts, geom = tr.sceneGrid(_desc(capi, g), select=[0, 1, 1], sensor_to_grid=xa, into=(np.zeros_like(wa[0]), np.full_like(wa[1], INV)))
    assert rc == 0
    _same((counts, geom), wa)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 6. plumbing -----------------------------------------------------------------------------------------------------------------

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
    # the host variant on unaligned pageable memory, a guard around both outputs and the selection
    L, h = tr.L, tr.h
    cells = 80 * 80 * 24
    d = _desc(capi, g)

    def unaligned(a, shift):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = np.full(b.size + 64, 0xAB, np.uint8)
        off = (-buf.ctypes.data) % 16 + shift
        buf[off:off + b.size] = b
        return buf, off
    hc, o_c = unaligned(np.zeros(cells, np.uint32), 5)
    hg, o_g = unaligned(np.zeros(cells, np.uint32), 7)
    hs, o_s = unaligned(np.array([1, 0, 1], np.uint8), 3)
    hc[:], hg[:] = 0xAB, 0xAB
    part = _want(oracle, g, ml, s, select=[1, 0, 1])
    assert L.ls_scene_grid_host(h, ctypes.byref(d), None, hs.ctypes.data + o_s, 3, hc.ctypes.data + o_c, hg.ctypes.data + o_g) == 0
    assert hc[o_c:o_c + cells * 4].tobytes() == part[0].tobytes() and hg[o_g:o_g + cells * 4].tobytes() == part[1].tobytes()
    assert np.all(hc[:o_c] == 0xAB) and np.all(hc[o_c + cells * 4:] == 0xAB) and np.all(hg[:o_g] == 0xAB) and np.all(hg[o_g + cells * 4:] == 0xAB)
    hc[:] = 0xAB
    assert L.ls_scene_grid_host(h, ctypes.byref(d), None, None, 0, hc.ctypes.data + o_c, None) == 0       # no geom array
    assert hc[o_c:o_c + cells * 4].tobytes() == want[0].tobytes() and np.all(hc[:o_c] == 0xAB) and np.all(hc[o_c + cells * 4:] == 0xAB)
    # one cell around the plate's middle; 2048 cells in a row through ben and the plate
    T, G = ref.scene_triangles(oracle, ml, s)
    mid = T[G == 2].reshape(-1, 3).mean(axis=0)
    g1 = ref.grid(tuple(mid - F(1.0)), 2.0, (1, 1, 1))
    w1 = ref.scene_grid(g1, T, G)
    assert w1[0][0, 0, 0] > 10 and w1[1][0, 0, 0] == 2
    _same(_grid_device(tr, capi, g1), w1)
    row = ref.grid((-40.0, float(mid[1]) - 0.5, float(mid[2]) - 0.5), 0.0625, (2048, 1, 1))
    wrow = ref.scene_grid(row, T, G)
    assert np.count_nonzero(wrow[0]) > 4
    _same(_grid_device(tr, capi, row), wrow)
    # refusals, nothing written
    out = torch.full((cells * 4 + 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    gout = torch.full((cells * 4 + 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_sel = _to_device(np.array([1, 1, 1], np.uint8))
    torch.cuda.synchronize()
    xf = rigid_transform()

    def call(handle=h, grid=d, **kw):
        a = dict(xf=None, select=d_sel.data_ptr(), n_select=3, counts=out.data_ptr(), geom=gout.data_ptr())
        a.update(kw)
        return L.ls_scene_grid(handle, None, None if grid is None else ctypes.byref(grid), a["xf"], a["select"], a["n_select"], a["counts"], a["geom"])

    def desc(**kw):
        dd = _desc(capi, g)
        for k, v in kw.items():
            if k in ("origin", "dims"):
                for j, x in enumerate(v):
                    getattr(dd, k)[j] = x
            else:
                setattr(dd, k, v)
        return dd
    nan = float("nan")
    bad_xf = xf.copy()
    bad_xf[7] = np.inf
    assert call(grid=None) == INVALID_ARGUMENT
    assert call(counts=None) == INVALID_ARGUMENT
    assert call(select=None) == INVALID_ARGUMENT
    assert call(grid=desc(flags=2)) == INVALID_ARGUMENT and call(grid=desc(flags=0x80000001)) == INVALID_ARGUMENT
    assert call(grid=desc(origin=(0.0, nan, 0.0))) == INVALID_ARGUMENT and call(xf=bad_xf.ctypes.data) == INVALID_ARGUMENT
    assert call(grid=desc(cell=0.0)) == INVALID_ARGUMENT and call(grid=desc(cell=nan)) == INVALID_ARGUMENT
    assert call(counts=out.data_ptr() + 8) == INVALID_ARGUMENT
    assert call(geom=gout.data_ptr() + 2) == INVALID_ARGUMENT
    assert call(grid=desc(dims=(0, 8, 6))) == OUT_OF_RANGE and call(grid=desc(dims=(2049, 1, 1))) == OUT_OF_RANGE
    assert call(grid=desc(dims=(2048, 2048, 33))) == OUT_OF_RANGE
    assert call(grid=desc(origin=(3e38, 0.0, 0.0), cell=1e35, dims=(2048, 1, 1))) == OUT_OF_RANGE
    # the earlier refusal answers: a misaligned pointer before a dimension, a bad cell before a misaligned pointer
    assert call(grid=desc(dims=(0, 8, 6)), counts=out.data_ptr() + 8) == INVALID_ARGUMENT
    assert call(grid=desc(cell=0.0, dims=(0, 8, 6)), counts=out.data_ptr() + 8) == INVALID_ARGUMENT
    assert L.ls_scene_grid_host(h, ctypes.byref(desc(flags=8)), None, None, 0, hc.ctypes.data, hg.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_scene_grid_host(h, ctypes.byref(d), None, None, 2, hc.ctypes.data, hg.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_scene_grid_host(h, ctypes.byref(d), None, None, 0, None, hg.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_scene_grid_host(h, ctypes.byref(desc(dims=(1, 1, 0))), None, None, 0, hc.ctypes.data, hg.ctypes.data) == OUT_OF_RANGE
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(gout.cpu().numpy() == 0xAB)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
    # no commit: the descriptor's refusals still come first; then -1, nothing written
    t2 = make_tracer(capi, s)
    assert call(handle=t2.h, grid=desc(dims=(0, 8, 6))) == OUT_OF_RANGE and call(handle=t2.h, counts=out.data_ptr() + 4) == INVALID_ARGUMENT
    assert t2.sceneGridDevice(d, out.data_ptr(), gout.data_ptr()) == -1
    keep = hc.copy()
    assert t2.L.ls_scene_grid_host(t2.h, ctypes.byref(d), None, None, 0, hc.ctypes.data + o_c, hg.ctypes.data + o_g) == -1
    assert np.array_equal(hc, keep)
    rc, c, gm = t2.sceneGrid(d)
    assert rc == -1 and not c.any() and np.all(gm == INV) and c.shape == (24, 80, 80) and gm.shape == (24, 80, 80)
    t2.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(gout.cpu().numpy() == 0xAB)
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
    g = ref.grid((-30.0, -30.0, -8.0), 1.0, (60, 60, 12))
    d = _desc(capi, g)
    cells = 60 * 60 * 12
    out = torch.full((cells * 4,), 0xAB, dtype=torch.uint8, device="cuda:0")
    gout = torch.full((cells * 4,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != FRAME_EAGER   # the frame is being captured: the graph is open
    assert L.ls_scene_grid(tr.h, None, ctypes.byref(d), None, None, 0, out.data_ptr(), gout.data_ptr()) == INVALID_ARGUMENT
    assert L.ls_scene_grid_host(tr.h, None, None, None, 0, None, None) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(gout.cpu().numpy() == 0xAB)
    # the graph is closed: the call works
    assert tr.sceneGridDevice(d, out.data_ptr(), gout.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    want = _want(oracle, g, ml, s)
    _same((out.cpu().numpy().view(np.uint32).reshape(12, 60, 60), gout.cpu().numpy().view(np.uint32).reshape(12, 60, 60)), want)
    assert want[0].sum() > 1000
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
