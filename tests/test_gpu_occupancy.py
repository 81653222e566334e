"""ls_occupancy_grid / ls_occupancy_grid_host on the MI355X: the free and occupied counts and the lowest geomID per cell of a voxel
grid against the numpy restatement of tests/occupancy_reference.py, byte for byte -- frame records on both engines, caller rays with
the hand-made cases of test_occupancy_cpu.py, shuffled and duplicated records, waves whose lanes share, break and interrupt runs of
cells, accumulation, and the entry points' plumbing.  Nothing here is compared against ls_debug_voxel_walk."""
import ctypes

import numpy as np
import pytest

import occupancy_reference as ref
from conftest import make_tracer
from test_gpu_labels import _geoms, _to_device, _xyz
from test_gpu_rays import INV, _ground_ben, _records, _scene_posed_quads
from test_occupancy_cpu import HAND_GRID, hand_made_rays, rigid_transform, rotation

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = -2                      # LS_ERR_INVALID_ARGUMENT
OUT_OF_RANGE = -9                          # LS_ERR_OUT_OF_RANGE
FRAME_EAGER = 0                            # LS_FRAME_EAGER
GUARD = 256
CARVE, ACCUMULATE = ref.CARVE_MISSES, ref.ACCUMULATE
F = np.float32

# torch fills a new tensor on its own stream, the library works on the handle's: every buffer is filled (a device-wide
# synchronize) before the library gets it


def _desc(capi, g):
    return capi.OccupancyGridDesc.make(g.origin, g.cell, g.dims, g.flags, g.min_range, g.max_range)


def _same(got, want):
    """(counts, geom) pairs, byte for byte"""
    assert got[0].dtype == np.uint32 and got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert np.array_equal(got[0][..., 1], want[0][..., 1]), "n_occ"
    assert np.array_equal(got[1], want[1]), "geom"
    bad = np.argwhere(got[0][..., 0] != want[0][..., 0])
    assert bad.shape[0] == 0, ("n_free", bad[:5], got[0][..., 0][tuple(bad[0])], want[0][..., 0][tuple(bad[0])])
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def _grid_device(tr, capi, g, records=None, rays=None, xf=None, count=None, stream=None, with_geom=True, into=None):
    """ls_occupancy_grid on device buffers, 0xAB behind both outputs -> (counts uint32[nz, ny, nx, 2], geom uint32[nz, ny, nx] or None)"""
    import torch
    nx, ny, nz = g.dims
    cells = nx * ny * nz
    n = 0 if records is None else np.asarray(records).reshape(-1, 4).shape[0]
    d_hits = _to_device(np.asarray(records, np.uint32)) if n else None
    d_rays = None if rays is None else _to_device(np.ascontiguousarray(rays, np.float32))
    d_count = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda:0")
    d_counts = torch.full((cells * 8 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_geom = torch.full((cells * 4 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    if into is not None:
        d_counts[:cells * 8] = _to_device(np.ascontiguousarray(into[0], np.uint32))
        d_geom[:cells * 4] = _to_device(np.ascontiguousarray(into[1], np.uint32))
    torch.cuda.synchronize()
    rc = tr.occupancyGridDevice(_desc(capi, g), d_counts.data_ptr(), d_geom.data_ptr() if with_geom else 0, d_hits.data_ptr() if n else 0, n,
                                0 if rays is None else d_rays.data_ptr(), 0 if rays is None else np.asarray(rays).reshape(-1, 8).shape[0],
                                0 if count is None else d_count.data_ptr(), xf, stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    c, gm = d_counts.cpu().numpy(), d_geom.cpu().numpy()
    assert np.all(c[cells * 8:] == 0xAB) and np.all(gm[cells * 4:] == 0xAB)
    if not with_geom:
        assert np.all(gm == 0xAB)
    return c[:cells * 8].copy().view(np.uint32).reshape(nz, ny, nx, 2), gm[:cells * 4].copy().view(np.uint32).reshape(nz, ny, nx) if with_geom else None


# ---- 1. frame records ------------------------------------------------------------------------------------------------------------

_frame_reference = {}   # the reference of one frame's records on one grid: computed once, whichever engine asks first


def _frame_want(g, rays, rec, geoms):
    key = (rec.tobytes(), tuple(g.origin), g.cell, tuple(g.dims), g.flags, g.min_range, g.max_range)
    if key not in _frame_reference:
        _frame_reference[key] = ref.occupancy(g, rays, rec, geoms, own=True)[:2]
    return _frame_reference[key]


@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_frame_records_carve_the_reference_grid(oracle, capi, sensors, meshes, engine):
    """sensor 0000 (4800 rays) over ground + ben, the grid in the sensor frame.  A 40 x 40 x 12 grid of 0.5 m cells around the sensor,
    with and without the misses, with and without a blind zone, with and without a range gate that cuts half of the hits: the
    sensor stands 5 m above the ground and its nearest return is 13 m away, so this grid is almost all free space (16 returns
    fall in it).  Then an 80 x 80 x 16 grid of 1 m cells, which holds most of the returns."""
    s = sensors["0000"]
    assert s.V * s.H == 4800
    tr = make_tracer(capi, s, engine)
    ml = _ground_ben(tr, oracle, meshes)
    rc, pts, hits = tr.traceScene(0)
    assert rc == 0 and hits.shape[0] == 1781
    rec = _records(hits)
    xyz, t = _xyz(pts), hits["t"]
    rays = ref.own_rays(oracle.ray_dirs(s))
    gate = F(np.sort(t)[t.shape[0] // 2])                 # half of the hits lie beyond it
    assert np.count_nonzero(t > gate) > 500
    small = [(flags, lo, hi) for flags in (0, CARVE) for lo in (0.0, 1.0) for hi in (1e4, gate)]
    seen = 0
    for origin, cell, dims, combos, at_least in (((-10.0, -10.0, -3.0), 0.5, (40, 40, 12), small, 1),
                                                 ((-40.0, -40.0, -10.0), 1.0, (80, 80, 16), [(0, 0.0, 1e4), (CARVE, 1.0, gate)], 400)):
        nx, ny, nz = dims
        for flags, lo, hi in combos:
            g = ref.grid(origin, cell, dims, flags, lo, hi)
            want = _frame_want(g, rays, rec, _geoms(ml))
            rc, counts, geom = tr.occupancyGrid(_desc(capi, g), hits)
            assert rc == 0
            _same((counts, geom), want)
            # the occupied cells are the cells of the frame's own points, and as many
            f = np.floor((xyz - np.float32(origin)) / F(cell))
            inside = np.all((f >= 0) & (f < np.float32(dims)), axis=1) & (t >= F(lo)) & (t <= F(hi))
            assert int(counts[..., 1].sum()) == np.count_nonzero(inside) >= at_least
            ci = f[inside].astype(np.int64)
            n_occ = np.bincount((ci[:, 2] * ny + ci[:, 1]) * nx + ci[:, 0], minlength=nx * ny * nz).reshape(nz, ny, nx)
            assert np.array_equal(counts[..., 1], n_occ)
            assert np.array_equal(geom != INV, n_occ > 0) and set(np.unique(geom[geom != INV])) <= {0, 1}
            # n_free counts rays: no cell more often than there are rays; the sensor's own cell by every ray that carves
            assert counts[..., 0].max() <= 4800
            if lo == 0.0 and flags == CARVE:
                assert counts[int(-origin[2] / cell), int(-origin[1] / cell), int(-origin[0] / cell), 0] == 4800
            seen += int(counts[..., 0].sum())
        _same(_grid_device(tr, capi, g, rec), want)
    assert seen > 100000
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 2. caller rays --------------------------------------------------------------------------------------------------------------

# the hand-made grid and its rays, moved 5 m down in the sensor frame (an exact shift): sensor 0000 stands 5.02 m above the ground,
# which then runs through the grid's second layer of cells
SHIFT = np.float32([0.0, 0.0, -5.0])
HAND_GRID = dict(HAND_GRID, origin=tuple(np.float32(HAND_GRID["origin"]) + SHIFT))


def _caller_rays(rng, n_random):
    """the hand-made rays of test_occupancy_cpu.py, then random ones with origins inside and outside HAND_GRID"""
    hand = np.stack([c[1] for c in hand_made_rays()])
    hand[:, 0:3] += SHIFT
    g = ref.grid(**HAND_GRID)
    lo, ext = np.float64(g.origin), np.float64(g.dims) * 0.5
    r = np.zeros((n_random, 8), np.float32)
    r[:, 0:3] = lo + rng.uniform(-0.5, 1.5, (n_random, 3)) * ext
    d = rng.normal(size=(n_random, 3))
    d[:, 2] -= 0.5                                          # most of them look down, at the ground
    r[:, 4:7] = d * rng.uniform(0.3, 2.0, n_random)[:, None] / np.linalg.norm(d, axis=1)[:, None]
    r[:, 3] = np.where(rng.random(n_random) < 0.2, rng.uniform(0, 2, n_random), 0)
    r[:, 7] = np.where(rng.random(n_random) < 0.2, rng.uniform(2, 20, n_random), np.inf)
    return np.concatenate([hand, r])


def test_caller_rays_with_traced_records(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    geoms = _geoms(ml)
    rays = _caller_rays(np.random.default_rng(17), 270)
    n = rays.shape[0]
    assert n == 301
    rc, hits = tr.traceRays(rays)
    assert rc == 0
    rec = _records(hits)
    f = lambda x: np.float32(x).view(np.uint32)
    hit = np.nonzero(rec[:, 1] != INV)[0]
    assert hit.shape[0] > 60
    # two records that must count nowhere, on rays that have no other: a prim out of range, a ray out of range
    miss = np.nonzero(rec[:, 1] == INV)[0]
    miss = miss[ref.lref.rays_walked(rays)[miss]]
    bad = np.array([[miss[0], 0, geoms[0], f(0.5)], [n, 0, 0, f(0.5)]], np.uint32)
    both = np.concatenate([rec, bad])
    total_occ = 0
    for flags, lo, hi, xf in ((CARVE, 0.0, 1e4, None), (0, 0.0, 1e4, None), (CARVE, 0.75, 6.0, None), (CARVE, 0.0, 1e4, rigid_transform()),
                              (0, 0.5, 9.0, rotation(np.random.default_rng(23)))):
        g = ref.grid(flags=flags, min_range=lo, max_range=hi, **HAND_GRID)
        want = ref.occupancy(g, rays, both, geoms, xf=xf)
        assert ref.occupancy(g, rays, rec, geoms, xf=xf)[0].tobytes() == want[0].tobytes()      # the two bad records change nothing
        rc, counts, geom = tr.occupancyGrid(_desc(capi, g), both, rays, xf)
        assert rc == 0
        _same((counts, geom), want[:2])
        _same(_grid_device(tr, capi, g, both, rays, xf), want[:2])
        assert counts[..., 0].sum() > 200
        total_occ += int(counts[..., 1].sum())
    assert total_occ > 20
    # degenerate rays count nowhere: the grid of the walkable rays alone is the same
    g = ref.grid(flags=CARVE, **HAND_GRID)
    ok = ref.lref.rays_walked(rays)
    assert np.count_nonzero(~ok) == 4
    keep = rays.copy()
    keep[~ok] = [100, 100, 100, 0, 1, 0, 0, np.inf]         # walkable, and nowhere near the grid
    _same(tr.occupancyGrid(_desc(capi, g), rec, rays)[1:], tr.occupancyGrid(_desc(capi, g), rec[ok[rec[:, 0]]], keep)[1:])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 3. shuffled and duplicated records ------------------------------------------------------------------------------------------

def test_closest_record_decides_in_any_order(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    geoms = _geoms(ml)
    rng = np.random.default_rng(29)
    rays = _caller_rays(rng, 270)
    rc, hits = tr.traceRays(rays)
    assert rc == 0
    rec = _records(hits)
    rec = rec[rec[:, 1] != INV]
    t = rec[:, 3].view(np.float32)
    third = rec.shape[0] // 3
    farther = rec[:third].copy()                            # a second record on the same ray, farther away, of another geometry
    farther[:, 1], farther[:, 2] = (farther[:, 1] + 1) % 3, 0
    farther[:, 3] = (t[:third] * F(1.5) + F(0.25)).view(np.uint32)
    nearer = rec[third:2 * third].copy()                    # ... nearer: it decides
    nearer[:, 1], nearer[:, 2] = (nearer[:, 1] + 2) % 3, 0
    nearer[:, 3] = (t[third:2 * third] * F(0.5)).view(np.uint32)
    rec[2 * third:, 1], rec[2 * third:, 2] = 2, 0           # (the rule does not test the triangle: any committed geometry counts)
    tied = rec[2 * third:].copy()                           # ... at the same t: the lower geomID decides
    tied[:, 1] = 1
    allrec = np.concatenate([rec, farther, nearer, tied, rec[::5]])
    g = ref.grid(flags=CARVE, **HAND_GRID)
    want = ref.occupancy(g, rays, allrec, geoms)
    plain = ref.occupancy(g, rays, rec, geoms)
    assert want[0].tobytes() != plain[0].tobytes() and want[1].tobytes() != plain[1].tobytes()
    keys = ref.closest_records(allrec, geoms, rays.shape[0], rays)
    lowest = np.minimum(tied[:, 1], rec[2 * third:, 1])
    assert np.array_equal((keys[tied[:, 0]] & np.uint64(0xFFFFFFFF)).astype(np.uint32), lowest) and np.any(lowest != rec[2 * third:, 1])
    assert np.array_equal((keys[nearer[:, 0]] >> np.uint64(32)).astype(np.uint32), nearer[:, 3])
    for k in range(5):
        perm = rng.permutation(allrec.shape[0])
        _same(_grid_device(tr, capi, g, allrec[perm], rays), want[:2])
    _same(tr.occupancyGrid(_desc(capi, g), allrec[::-1], rays)[1:], want[:2])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 4. wave aggregation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 127, 200])
def test_runs_of_lanes_in_one_cell(oracle, capi, sensors, meshes, n_rays):
    """a 16 x 16 x 4 grid.  identical: every lane of a wave stands in the same cell at every trip; alternate: every second ray misses
    the grid, so every run is one lane long and idle lanes stand between them; inside: identical rays whose records end at different
    cells, so that at most trips one lane of the run stands in its own occupied cell and does not mark; pairs: runs of two; mixed:
    all of it at random"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _ground_ben(tr, oracle, meshes)
    geoms = _geoms(ml)
    f = lambda x: np.float32(x).view(np.uint32)
    base = np.array([-3.9, -3.7, 0.3, 0, 1.0, 0.9, 0.05, np.inf], np.float32)   # (synthetic records: the rule does not test the triangle)
    away = np.array([50.0, 50.0, 50.0, 0, 1.0, 0.0, 0.0, np.inf], np.float32)
    i = np.arange(n_rays)
    rng = np.random.default_rng(n_rays)
    other = np.array([3.9, -3.9, 1.7, 0, -1.0, 0.8, -0.1, np.inf], np.float32)
    cases = {}
    cases["identical"] = (np.tile(base, (n_rays, 1)), np.zeros((0, 4), np.uint32))
    alt = np.tile(base, (n_rays, 1))
    alt[1::2] = away
    cases["alternate"] = (alt, np.zeros((0, 4), np.uint32))
    t_in = (F(0.3) + F(0.11) * (i % 61).astype(np.float32)).astype(np.float32)
    cases["inside"] = (np.tile(base, (n_rays, 1)), np.stack([i, i % 2, np.zeros_like(i), t_in.view(np.uint32)], axis=1).astype(np.uint32))
    pairs = np.tile(base, (n_rays, 1))
    pairs[(i // 2) % 2 == 1] = other
    cases["pairs"] = (pairs, np.stack([i, np.zeros_like(i), np.zeros_like(i), np.full(n_rays, f(3.0))], axis=1).astype(np.uint32)[::3])
    mixed = np.where((rng.random(n_rays) < 0.5)[:, None], base, other)
    mixed[rng.random(n_rays) < 0.2] = away
    mixed[:, 4:7] += (rng.random((n_rays, 3)) < 0.3) * rng.normal(0, 0.02, (n_rays, 3)).astype(np.float32)
    hit = rng.random(n_rays) < 0.6
    cases["mixed"] = (mixed, np.stack([i, rng.integers(0, 2, n_rays), np.zeros_like(i), rng.uniform(0.2, 12, n_rays).astype(np.float32).view(np.uint32)],
                                      axis=1).astype(np.uint32)[hit])
    for name, (rays, rec) in cases.items():
        g = ref.grid((-4.0, -4.0, 0.0), 0.5, (16, 16, 4), CARVE, 0.0, 1e4)
        want = ref.occupancy(g, rays, rec, geoms)
        got = _grid_device(tr, capi, g, rec, rays)
        _same(got, want[:2])
        assert got[0][..., 0].sum() > 0, name
        if name == "identical":
            assert set(np.unique(got[0][..., 0])) == {0, n_rays}
        if name == "inside" and n_rays > 1:
            assert got[0][..., 1].sum() == n_rays and np.count_nonzero(got[0][..., 1]) > 1
            assert np.any((got[0][..., 0] > 0) & (got[0][..., 1] > 0))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 5. accumulation -------------------------------------------------------------------------------------------------------------

def test_accumulate_adds_counts_and_keeps_the_lowest_geom(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    geoms = _geoms(ml)
    rays = _caller_rays(np.random.default_rng(31), 270)
    rc, hits = tr.traceRays(rays)
    assert rc == 0
    rec = _records(hits)
    xa = rigid_transform()
    xb = np.array([np.cos(0.7), -np.sin(0.7), 0, 0.3, np.sin(0.7), np.cos(0.7), 0, -0.2, 0, 0, 1, 0.1], np.float32)   # a turn about z, rounded
    g = ref.grid(flags=CARVE, **HAND_GRID)
    ga = ref.grid(flags=CARVE | ACCUMULATE, **HAND_GRID)
    wa, wb = ref.occupancy(g, rays, rec, geoms, xf=xa), ref.occupancy(g, rays, rec, geoms, xf=xb)
    assert wa[0].tobytes() != wb[0].tobytes() and wa[0][..., 1].sum() > 5 and wb[0][..., 1].sum() > 5
    total = (wa[0] + wb[0], np.minimum(wa[1], wb[1]))
    first = _grid_device(tr, capi, g, rec, rays, xa)
    _same(first, wa[:2])
    _same(_grid_device(tr, capi, ga, rec, rays, xb, into=first), total)
    _same(ref.occupancy(ga, rays, rec, geoms, xf=xb, into=wa[:2])[:2], total)
    # without the flag the second call overwrites what the buffers held
    _same(_grid_device(tr, capi, g, rec, rays, xb, into=first), wb[:2])
    # the host variant: `into` sets the flag, the arrays travel both ways; the caller's arrays stay as they were
    keep = (first[0].copy(), first[1].copy())
    rc, counts, geom = tr.occupancyGrid(_desc(capi, g), rec, rays, xb, into=first)
    assert rc == 0
    _same((counts, geom), total)
    _same(first, keep)
    # accumulating on a cleared pair is the plain call
    rc, counts, geom = tr.occupancyGrid(_desc(capi, g), rec, rays, xa, into=(np.zeros_like(wa[0]), np.full_like(wa[1], INV)))
    assert rc == 0
    _same((counts, geom), wa[:2])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 6. plumbing -----------------------------------------------------------------------------------------------------------------

def test_entry_points(oracle, capi, sensors, meshes):
    """a device count below n; a caller stream; d_geom = NULL; the host variant on unaligned pageable memory; no records at all; the
    refusals of the device entry point in their order, nothing written; a 1 x 1 x 1 grid; 2048 x 1 x 1 with one ray along x; no
    commit: -1 and nothing written"""
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    geoms = _geoms(ml)
    rays = _caller_rays(np.random.default_rng(41), 270)
    n_rays = rays.shape[0]
    built = tr.info(capi.LS_INFO_RAY_QUERY_BUILT)
    rc, hits = tr.traceRays(rays)
    assert rc == 0
    rec = _records(hits)
    n = rec.shape[0]
    g = ref.grid(flags=CARVE, min_range=0.25, max_range=9.0, **HAND_GRID)
    want = ref.occupancy(g, rays, rec, geoms)
    _same(_grid_device(tr, capi, g, rec, rays), want[:2])
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) in (built, 3)           # the call builds nothing: the word is traceRays'
    # a device count below n: the records beyond it are not read; above n: n
    part = ref.occupancy(g, rays, rec[:100], geoms)
    assert part[0].tobytes() != want[0].tobytes()
    _same(_grid_device(tr, capi, g, rec, rays, count=100), part[:2])
    _same(_grid_device(tr, capi, g, rec, rays, count=5000), want[:2])
    # a caller's stream; no geom array
    st = torch.cuda.Stream()
    _same(_grid_device(tr, capi, g, rec, rays, stream=st.cuda_stream), want[:2])
    c, none = _grid_device(tr, capi, g, rec, rays, with_geom=False)
    assert none is None and c.tobytes() == want[0].tobytes()
    # no records: every ray is a miss; without the flag the grid is cleared and nothing else
    miss = ref.occupancy(g, rays, np.zeros((0, 4), np.uint32), geoms)
    _same(_grid_device(tr, capi, g, None, rays), miss[:2])
    assert miss[0][..., 1].sum() == 0 and miss[0][..., 0].sum() > 0
    g0 = ref.grid(flags=0, **HAND_GRID)
    cleared = _grid_device(tr, capi, g0, None, rays)
    assert not cleared[0].any() and np.all(cleared[1] == INV)
    rc, c, gm = tr.occupancyGrid(_desc(capi, g), None, rays)
    assert rc == 0
    _same((c, gm), miss[:2])
    # the handle's own rays without records: 4800 misses
    near = ref.grid((-2.0, -2.0, -1.0), 0.5, (8, 8, 4), CARVE, 0.25, 9.0)
    own = ref.occupancy(near, ref.own_rays(oracle.ray_dirs(s)), np.zeros((0, 4), np.uint32), geoms, own=True)
    assert own[0][..., 0].sum() > 4800          # (the sensor stands on a corner of cells: its rays leave through eight of them)
    _same(_grid_device(tr, capi, near, None, None), own[:2])
    # the host variant on unaligned pageable memory, a guard behind both outputs
    L, h = tr.L, tr.h
    cells = 16 * 8 * 6
    d = _desc(capi, g)

    def unaligned(a, shift):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = np.full(b.size + 64, 0xAB, np.uint8)
        off = (-buf.ctypes.data) % 16 + shift
        buf[off:off + b.size] = b
        return buf, off
    hr, o_r = unaligned(rays, 1)
    hh, o_h = unaligned(rec, 3)
    hc, o_c = unaligned(np.zeros(cells * 2, np.uint32), 5)
    hg, o_g = unaligned(np.zeros(cells, np.uint32), 7)
    hc[:], hg[:] = 0xAB, 0xAB
    assert L.ls_occupancy_grid_host(h, ctypes.byref(d), None, hr.ctypes.data + o_r, n_rays, hh.ctypes.data + o_h, n, hc.ctypes.data + o_c,
                                    hg.ctypes.data + o_g) == 0
    assert hc[o_c:o_c + cells * 8].tobytes() == want[0].tobytes() and hg[o_g:o_g + cells * 4].tobytes() == want[1].tobytes()
    assert np.all(hc[:o_c] == 0xAB) and np.all(hc[o_c + cells * 8:] == 0xAB) and np.all(hg[:o_g] == 0xAB) and np.all(hg[o_g + cells * 4:] == 0xAB)
    # refusals, nothing written
    d_rays, d_hits = _to_device(rays), _to_device(rec)
    out = torch.full((cells * 8 + 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    gout = torch.full((cells * 4 + 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    xf = rigid_transform()

    def call(grid=d, **kw):
        a = dict(xf=None, rays=d_rays.data_ptr(), n_rays=n_rays, hits=d_hits.data_ptr(), count=None, n=n, counts=out.data_ptr(), geom=gout.data_ptr())
        a.update(kw)
        return L.ls_occupancy_grid(h, None, None if grid is None else ctypes.byref(grid), a["xf"], a["rays"], a["n_rays"], a["hits"], a["count"], a["n"],
                                   a["counts"], a["geom"])

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
    assert call(counts=None) == INVALID_ARGUMENT
    assert call(hits=None) == INVALID_ARGUMENT
    assert call(grid=desc(flags=4)) == INVALID_ARGUMENT and call(grid=desc(reserved=(0, 9))) == INVALID_ARGUMENT
    assert call(grid=desc(origin=(0.0, nan, 0.0))) == INVALID_ARGUMENT and call(xf=bad_xf.ctypes.data) == INVALID_ARGUMENT
    assert call(grid=desc(cell=0.0)) == INVALID_ARGUMENT and call(grid=desc(cell=nan)) == INVALID_ARGUMENT
    assert call(grid=desc(min_range=-0.5)) == INVALID_ARGUMENT and call(grid=desc(min_range=nan)) == INVALID_ARGUMENT
    assert call(grid=desc(max_range=0.125)) == INVALID_ARGUMENT and call(grid=desc(max_range=float("inf"))) == INVALID_ARGUMENT
    assert call(rays=d_rays.data_ptr() + 8) == INVALID_ARGUMENT
    assert call(hits=d_hits.data_ptr() + 4) == INVALID_ARGUMENT
    assert call(counts=out.data_ptr() + 8) == INVALID_ARGUMENT
    assert call(geom=gout.data_ptr() + 2) == INVALID_ARGUMENT
    assert call(count=out.data_ptr() + 2) == INVALID_ARGUMENT
    assert call(grid=desc(dims=(0, 8, 6))) == OUT_OF_RANGE and call(grid=desc(dims=(2049, 1, 1))) == OUT_OF_RANGE
    assert call(grid=desc(dims=(2048, 2048, 33))) == OUT_OF_RANGE
    assert call(grid=desc(origin=(3e38, 0.0, 0.0), cell=1e35, dims=(2048, 1, 1))) == OUT_OF_RANGE
    assert call(n=0xFFF00001) == OUT_OF_RANGE and call(n_rays=0xFFF00001) == OUT_OF_RANGE
    # the earlier refusal answers: a misaligned pointer before a dimension, a bad cell before a misaligned pointer
    assert call(grid=desc(dims=(0, 8, 6)), counts=out.data_ptr() + 8) == INVALID_ARGUMENT
    assert call(grid=desc(cell=0.0, dims=(0, 8, 6)), counts=out.data_ptr() + 8) == INVALID_ARGUMENT
    assert L.ls_occupancy_grid_host(h, ctypes.byref(desc(flags=8)), None, rays.ctypes.data, n_rays, rec.ctypes.data, n, hc.ctypes.data, hg.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_occupancy_grid_host(h, ctypes.byref(d), None, rays.ctypes.data, n_rays, None, n, hc.ctypes.data, hg.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_occupancy_grid_host(h, ctypes.byref(desc(dims=(1, 1, 0))), None, rays.ctypes.data, n_rays, rec.ctypes.data, n, hc.ctypes.data, hg.ctypes.data) == OUT_OF_RANGE
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(gout.cpu().numpy() == 0xAB)
    # one cell: every ray that crosses it counts once
    g1 = ref.grid((-1.0, -1.0, -6.0), 2.0, (1, 1, 1), CARVE, 0.0, 1e4)
    w1 = ref.occupancy(g1, rays, rec, geoms)
    assert w1[0][0, 0, 0, 0] > 10 and w1[0][0, 0, 0, 1] > 0
    _same(_grid_device(tr, capi, g1, rec, rays), w1[:2])
    # 2048 cells in a row and one ray along them: the longest walk the call allows; every cell once, the last one occupied
    f = lambda x: np.float32(x).view(np.uint32)
    row = ref.grid((0.0, 0.0, 0.0), 0.25, (2048, 1, 1), 0, 0.0, 1e4)
    one = np.array([[0.125, 0.125, 0.125, 0, 1, 0, 0, np.inf]], np.float32)
    r1 = np.array([[0, 0, 0, f(511.75)]], np.uint32)
    wrow = ref.occupancy(row, one, r1, geoms)
    assert wrow[2].shape[1] == 2048 and wrow[0][0, 0, :, 0].tolist() == [1] * 2047 + [0] and wrow[0][0, 0, 2047].tolist() == [0, 1]
    _same(_grid_device(tr, capi, row, r1, one), wrow[:2])
    back = np.array([[511.9, 0.125, 0.125, 0, -1, 0, 0, np.inf]], np.float32)       # and back, without a record
    rowc = ref.grid((0.0, 0.0, 0.0), 0.25, (2048, 1, 1), CARVE, 0.0, 1e4)
    wback = ref.occupancy(rowc, back, np.zeros((0, 4), np.uint32), geoms)
    assert wback[0][0, 0, :, 0].tolist() == [1] * 2048
    _same(_grid_device(tr, capi, rowc, None, back), wback[:2])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
    # no commit: -1, nothing written
    t2 = make_tracer(capi, s)
    assert t2.occupancyGridDevice(d, out.data_ptr(), gout.data_ptr(), d_hits.data_ptr(), n, d_rays.data_ptr(), n_rays) == -1
    assert t2.L.ls_occupancy_grid_host(t2.h, ctypes.byref(d), None, rays.ctypes.data, n_rays, rec.ctypes.data, n, hc.ctypes.data + o_c, hg.ctypes.data + o_g) == -1
    assert hc[o_c:o_c + cells * 8].tobytes() == want[0].tobytes()                        # (what the earlier call left there)
    rc, c, gm = t2.occupancyGrid(d, rec, rays)
    assert rc == -1 and not c.any() and np.all(gm == INV) and c.shape == (6, 8, 16, 2) and gm.shape == (6, 8, 16)
    t2.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(gout.cpu().numpy() == 0xAB)
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
    g = ref.grid((-30.0, -30.0, -8.0), 1.0, (60, 60, 12), CARVE, 0.5, 40.0)
    d = _desc(capi, g)
    cells = 60 * 60 * 12
    out = torch.full((cells * 8,), 0xAB, dtype=torch.uint8, device="cuda:0")
    gout = torch.full((cells * 4,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != FRAME_EAGER   # the frame is being captured: the graph is open
    assert L.ls_occupancy_grid(tr.h, None, ctypes.byref(d), None, None, 0, h.data_ptr(), c.data_ptr(), cap, out.data_ptr(), gout.data_ptr()) == INVALID_ARGUMENT
    assert L.ls_occupancy_grid_host(tr.h, None, None, None, 0, None, 0, None, None) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(gout.cpu().numpy() == 0xAB)
    # the frame went out, and the handle carves its records where they lie: d_hits, the device count, n = the capacity
    k = int(c[0].item())
    assert k > 0
    assert tr.occupancyGridDevice(d, out.data_ptr(), gout.data_ptr(), h.data_ptr(), cap, d_count=c.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    rec = h.cpu().numpy()[:16 * k].view(np.uint32).reshape(k, 4)
    want = ref.occupancy(g, ref.own_rays(oracle.ray_dirs(s)), rec, _geoms(ml), own=True)
    _same((out.cpu().numpy().view(np.uint32).reshape(12, 60, 60, 2), gout.cpu().numpy().view(np.uint32).reshape(12, 60, 60)), want[:2])
    assert want[0][..., 1].sum() > 100
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
