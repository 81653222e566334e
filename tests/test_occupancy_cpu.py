"""ls_occupancy_grid without a device: the symbols, the header signatures, the descriptor, the refusals that come before any device call
(there is no GPU where `-m "not gpu"` runs), the shared walk through its host hook (ls_debug_voxel_walk) against the numpy
reference, and the reference itself against float64 geometry."""
import ctypes
import os
import re

import numpy as np

import occupancy_reference as ref
from conftest import ROOT

INVALID_ARGUMENT, OUT_OF_RANGE = -2, -9
INV = 0xFFFFFFFF
F = np.float32


def _header(name="lidarshooter_hip.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _desc(capi, g):
    return capi.OccupancyGridDesc.make(g.origin, g.cell, g.dims, g.flags, g.min_range, g.max_range)


# ---- the hand-made rays (test_gpu_occupancy.py casts them too) ---------------------------------------------------------------------

HAND_GRID = dict(origin=(-4.0, -2.0, -1.0), cell=0.5, dims=(16, 8, 6))   # x in [-4, 4), y in [-2, 2), z in [-1, 2)


def hand_made_rays():
    """-> [(name, ray8 float32, t_end)]: t_end the deciding record's t for ls_debug_voxel_walk (NaN: none)"""
    inf, nan = np.inf, np.nan
    cases = [
        ("axis-parallel inside", [-3.75, 0.25, 0.25, 0, 1, 0, 0, inf], 5.0),
        ("axis-parallel along -z", [0.25, 0.25, 1.75, 0, 0, 0, -1, inf], 2.0),
        ("on the lower x face (q == 0: inside)", [-4.0, 0.25, 0.25, 0, 0, 1, 0, inf], 1.0),
        ("on the upper x face (q == E: outside)", [4.0, 0.25, 0.25, 0, 0, 1, 0, inf], 1.0),
        ("on the lower y face", [0.0, -2.0, 0.0, 0, 1, 0, 0, inf], 3.0),
        ("on the upper y face", [0.0, 2.0, 0.0, 0, 1, 0, 0, inf], 3.0),
        ("in a cell face inside the grid", [-3.0, 0.5, 0.0, 0, 1, 0, 0, inf], 4.0),
        ("through the corner from outside: exact ties", [-5.0, -3.0, -2.0, 0, 1, 1, 1, inf], 3.5),
        ("through the corner, no record", [-5.0, -3.0, -2.0, 0, 1, 1, 1, inf], nan),
        ("along a cell edge diagonal: ties at every step", [-4.0, -2.0, 0.25, 0, 0.5, 0.5, 0, inf], 6.0),
        ("misses the grid", [-10.0, 10.0, 10.0, 0, 1, 0, 0, inf], 5.0),
        ("points away from the grid", [-5.0, 0.0, 0.0, 0, -1, 0, 0, inf], nan),
        ("negative directions", [3.9, 1.9, 1.9, 0, -1, -0.5, -0.25, inf], 6.0),
        ("negative direction from outside", [6.0, 3.0, 2.5, 0, -1, -0.5, -0.25, inf], nan),
        ("a denormal direction component", [-3.9, 0.3, 0.3, 0, 1, 1e-42, 0, inf], 7.0),
        ("a negative denormal component on a face", [-3.9, 0.5, 0.3, 0, 1, -1e-42, 0, inf], 7.0),
        ("t_end on a cell boundary", [-3.75, 0.25, 0.25, 0, 1, 0, 0, inf], 1.25),
        ("t_end on a boundary, negative direction", [3.75, 0.25, 0.25, 0, -1, 0, 0, inf], 1.25),
        ("t_end below t_start", [-3.75, 0.25, 0.25, 2.0, 1, 0, 0, inf], 1.0),
        ("t_end equal to t_start", [-3.75, 0.25, 0.25, 1.0, 1, 0, 0, inf], 1.0),
        ("tmax before the far side, no record", [-3.75, 0.25, 0.25, 0.5, 1, 0, 0, 2.5], nan),
        ("the hit on the grid's upper face: not occupied", [3.0, 0.0, 0.0, 0, 1, 0, 0, inf], 1.0),
        ("the hit on the grid's upper z face", [0.1, 0.1, 0.0, 0, 0, 0, 1, inf], 2.0),
        ("the hit on the grid's lower face: occupied", [-5.0, 0.1, 0.1, 0, 1, 0, 0, inf], 1.0),
        ("the hit outside the grid", [3.0, 0.0, 0.0, 0, 1, 0, 0, inf], 3.0),
        ("an origin inside, a skew ray", [0.1, -0.2, 0.3, 0, 0.3, 0.9, -0.2, inf], 2.5),
        ("an origin outside, a skew ray", [-7.0, -4.0, 3.0, 0, 0.8, 0.5, -0.3, inf], 9.0),
        ("degenerate: a zero direction", [0.0, 0.0, 0.0, 0, 0, 0, 0, inf], 1.0),
        ("degenerate: tmin above tmax", [0.0, 0.0, 0.0, 3.0, 1, 0, 0, 2.0], 1.0),
        ("degenerate: a NaN origin", [nan, 0.0, 0.0, 0, 1, 0, 0, inf], 1.0),
        ("degenerate: an infinite direction", [0.0, 0.0, 0.0, 0, inf, 0, 0, inf], 1.0),
    ]
    return [(name, np.array(r, np.float32), F(t)) for name, r, t in cases]


def rigid_transform():
    """a quarter turn about z and a translation: exact in float32"""
    return np.array([0, -1, 0, 0.5, 1, 0, 0, -0.25, 0, 0, 1, 0.125], np.float32)


def rotation(rng):
    """a random rotation and translation, rounded to float32"""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.concatenate([R, rng.uniform(-2, 2, (3, 1))], axis=1).astype(np.float32).reshape(12)


def random_rays(rng, g, n):
    """rays (n, 8) around grid g and a t_end for each: zero direction components, integer directions and origins on cell faces among
    them; a fifth have no record"""
    lo = np.float64(g.origin)
    ext = np.float64(g.dims) * np.float64(g.cell)
    o = lo + rng.uniform(-0.3, 1.3, (n, 3)) * ext + rng.uniform(-2, 2, (n, 3))
    face = rng.random((n, 3)) < 0.15
    o = np.where(face, lo + np.round((o - lo) / np.float64(g.cell)) * np.float64(g.cell), o)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    kind = rng.integers(0, 5, n)
    d = np.where((kind == 1)[:, None], rng.integers(-1, 2, (n, 3)), d)
    d = np.where((kind == 2)[:, None] & (rng.random((n, 3)) < 0.5), 0.0, d)
    toward = (kind == 3)
    target = lo + rng.uniform(0, 1, (n, 3)) * ext
    d = np.where(toward[:, None], (target - o) / np.maximum(np.linalg.norm(target - o, axis=1), 1e-3)[:, None], d)
    d[np.all(d == 0, axis=1)] = [0, 0, 1]
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 4:7] = o, d
    r[:, 3] = np.where(rng.random(n) < 0.2, rng.uniform(0, 3, n), 0)
    r[:, 7] = np.where(rng.random(n) < 0.2, rng.uniform(3, 30, n), np.inf)
    t_end = rng.uniform(0, 30, n).astype(np.float32)
    t_end[rng.random(n) < 0.2] = np.nan
    return r, t_end


# ---- the surface -------------------------------------------------------------------------------------------------------------------

def test_occupancy_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in ("ls_occupancy_grid", "ls_occupancy_grid_host", "ls_occupancy_grid_check"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s
    assert "ls_debug_voxel_walk" in capi.DEBUG_SYMBOLS and hasattr(lib, "ls_debug_voxel_walk")
    assert capi.load().ls_abi_version() == 4


def test_occupancy_header_signatures_and_descriptor(capi):
    hdr = re.sub(r"\s+", " ", _header())
    assert ("int ls_occupancy_grid(ls_tracer *tr, void *hip_stream, const ls_occupancy_grid_desc *grid, const float *sensor_to_grid3x4, "
            "const void *d_rays, uint32_t n_rays, const void *d_hits, const uint32_t *d_count, uint32_t n, void *d_counts, void *d_geom);") in hdr
    assert ("int ls_occupancy_grid_host(ls_tracer *tr, const ls_occupancy_grid_desc *grid, const float *sensor_to_grid3x4, "
            "const void *rays, uint32_t n_rays, const void *hits, uint32_t n, void *counts, void *geom);") in hdr
    assert "int ls_occupancy_grid_check(const ls_occupancy_grid_desc *grid);" in hdr
    assert "#define LS_OCC_CARVE_MISSES 1u" in hdr and "#define LS_OCC_ACCUMULATE 2u" in hdr
    assert capi.LS_OCC_CARVE_MISSES == 1 and capi.LS_OCC_ACCUMULATE == 2
    dbg = re.sub(r"\s+", " ", _header("lidarshooter_hip_debug.h"))
    assert ("int ls_debug_voxel_walk(const ls_occupancy_grid_desc *grid, const float *sensor_to_grid3x4, const float ray32[8], float t_end, "
            "uint32_t *cells_out, uint32_t capacity, uint32_t *n_cells, uint32_t *occupied_cell_out);") in dbg
    D = capi.OccupancyGridDesc
    assert ctypes.sizeof(D) == 48
    body = re.search(r"typedef struct ls_occupancy_grid_desc \{(.*?)\} ls_occupancy_grid_desc;", _header(), re.S).group(1)
    fields = re.findall(r"^\s*(?:uint32_t|float)\s+(\w+)", body, re.M)
    assert fields == [f[0] for f in D._fields_] == ["origin", "cell", "dims", "flags", "min_range", "max_range", "reserved"]
    assert [getattr(D, f).offset for f in fields] == [0, 12, 16, 28, 32, 36, 40]


def test_descriptor_refusals_in_the_stated_order(capi):
    L = capi.load()
    check = lambda d: L.ls_occupancy_grid_check(ctypes.byref(d))

    def make(**kw):
        d = capi.OccupancyGridDesc.make((-1.0, -2.0, -3.0), 0.5, (4, 5, 6), 3, 0.5, 60.0)
        for k, v in kw.items():
            if k in ("origin", "dims", "reserved"):
                for i, x in enumerate(v):
                    getattr(d, k)[i] = x
            else:
                setattr(d, k, v)
        return d
    nan, inf = float("nan"), float("inf")
    assert check(make()) == 0 and check(make(flags=0)) == 0 and check(make(min_range=0.0, max_range=0.0)) == 0
    assert L.ls_occupancy_grid_check(None) == INVALID_ARGUMENT
    # every refusal alone, in the header's order; each one with every LATER fault present as well: the earlier one answers
    faults = [("flags", dict(flags=4), INVALID_ARGUMENT), ("reserved", dict(reserved=(0, 1)), INVALID_ARGUMENT),
              ("origin", dict(origin=(0.0, nan, 0.0)), INVALID_ARGUMENT), ("cell", dict(cell=0.0), INVALID_ARGUMENT),
              ("min_range", dict(min_range=-1.0), INVALID_ARGUMENT), ("max_range", dict(max_range=0.25), INVALID_ARGUMENT),
              ("dims", dict(dims=(0, 5, 6)), OUT_OF_RANGE)]
    for i, (name, kw, rc) in enumerate(faults):
        assert check(make(**kw)) == rc, name
        later = {}
        for _, kw2, _ in faults[i:]:
            later.update(kw2)
        assert check(make(**later)) == rc, name
    for kw in (dict(flags=0x80000001), dict(reserved=(7, 0)), dict(origin=(inf, 0.0, 0.0)), dict(origin=(0.0, 0.0, -inf)), dict(cell=nan), dict(cell=inf),
               dict(cell=-0.5), dict(min_range=nan), dict(min_range=inf), dict(max_range=nan), dict(max_range=inf),
               dict(min_range=2.0, max_range=1.0)):
        assert check(make(**kw)) == INVALID_ARGUMENT, kw
    for kw in (dict(dims=(2049, 1, 1)), dict(dims=(1, 0, 1)), dict(dims=(1, 1, 2049)), dict(dims=(2048, 2048, 33)), dict(dims=(1024, 1024, 129)),
               dict(origin=(3e38, 0.0, 0.0), cell=1e35, dims=(2048, 1, 1))):
        assert check(make(**kw)) == OUT_OF_RANGE, kw
    for kw in (dict(dims=(2048, 1, 1)), dict(dims=(2048, 2048, 32)), dict(dims=(1, 1, 1)), dict(dims=(512, 512, 512))):
        assert check(make(**kw)) == 0, kw


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    buf = (ctypes.c_uint8 * 256)()
    d = capi.OccupancyGridDesc.make((0, 0, 0), 1.0, (2, 2, 2))
    for n in (0, 1):
        p = buf if n else None
        assert L.ls_occupancy_grid(None, None, ctypes.byref(d), None, p, n, p, None, n, buf, buf) == INVALID_ARGUMENT
        assert L.ls_occupancy_grid_host(None, ctypes.byref(d), None, p, n, p, n, buf, buf) == INVALID_ARGUMENT
    assert list(buf) == [0] * 256


# ---- the walk: the host hook against the reference ---------------------------------------------------------------------------------

def _hook(capi, g, ray8, t_end, xf=None):
    L = capi.load()
    d = _desc(capi, g)
    cap = sum(g.dims) + 8
    cells = np.full(cap, 0xABABABAB, np.uint32)
    n, occ = ctypes.c_uint32(0xABABABAB), ctypes.c_uint32(0xABABABAB)
    r = np.ascontiguousarray(ray8, np.float32)
    m = None if xf is None else np.ascontiguousarray(xf, np.float32)
    rc = L.ls_debug_voxel_walk(ctypes.byref(d), None if m is None else m.ctypes.data, r.ctypes.data, ctypes.c_float(float(t_end)), cells.ctypes.data, cap,
                               ctypes.byref(n), ctypes.byref(occ))
    assert rc == 0 and n.value <= sum(g.dims) and np.all(cells[n.value:] == 0xABABABAB)
    return cells[:n.value].copy(), occ.value


def _same_walk(capi, g, rays, t_end, xf=None):
    """the hook, one ray at a time, against the reference over all of them; -> (visited, occupied cells) of the reference"""
    keys = np.where(np.isnan(t_end), np.uint64(0xFFFFFFFFFFFFFFFF), np.ascontiguousarray(t_end, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32))
    st = ref.rays_of(g, rays, keys, False, xf)
    visited = ref.walk(g, st.o, st.d, st.t0, st.t1, st.carve)
    for i in range(rays.shape[0]):
        cells, occ = _hook(capi, g, rays[i], t_end[i], xf)
        want = visited[i][visited[i] >= 0]
        assert np.array_equal(cells, want.astype(np.uint32)), (i, rays[i], t_end[i], cells, want)
        assert occ == (INV if st.occ[i] < 0 else st.occ[i]), (i, rays[i], t_end[i])
        one = ref.one_ray(g, rays[i], t_end[i], xf)
        assert np.array_equal(one[0], cells) and one[1] == occ
    return visited, st.occ


def test_debug_walk_equals_the_reference_on_random_rays(capi):
    rng = np.random.default_rng(11)
    total = 0
    for dims, origin, cell in (((1, 1, 1), (-0.5, -0.5, -0.5), 1.0), ((3, 2, 5), (-1.0, 0.25, -2.0), 0.7), ((33, 17, 9), (-8.0, -4.0, -1.0), 0.5),
                               ((47, 1, 47), (-10.0, 0.0, -10.0), 0.43)):
        for flags, lo, hi in ((1, 0.0, 1e4), (0, 1.0, 12.0), (1, 0.5, 8.0)):
            g = ref.grid(origin, cell, dims, flags, lo, hi)
            rays, t_end = random_rays(rng, g, 42)
            visited, occ = _same_walk(capi, g, rays, t_end, rotation(rng) if flags == 1 and lo > 0 else None)
            total += rays.shape[0]
            assert np.count_nonzero(visited >= 0) > 0
    assert total >= 500


def test_debug_walk_equals_the_reference_on_the_hand_made_rays(capi):
    cases = hand_made_rays()
    rays = np.stack([c[1] for c in cases])
    t_end = np.array([c[2] for c in cases], np.float32)
    name = {c[0]: i for i, c in enumerate(cases)}
    g = ref.grid(flags=1, **HAND_GRID)
    visited, occ = _same_walk(capi, g, rays, t_end)
    cells = lambda k: [int(c) for c in visited[name[k]] if c >= 0]
    idx = lambda x, y, z: (z * 8 + y) * 16 + x
    # what the walk must give, worked out by hand
    assert cells("axis-parallel inside") == [idx(x, 4, 2) for x in range(0, 11)] and occ[name["axis-parallel inside"]] == idx(10, 4, 2)
    assert cells("axis-parallel along -z") == [idx(8, 4, z) for z in (5, 4, 3, 2, 1)]
    assert cells("on the lower x face (q == 0: inside)") == [idx(0, 4, 2), idx(0, 5, 2), idx(0, 6, 2)]
    assert cells("on the upper x face (q == E: outside)") == [] and occ[name["on the upper x face (q == E: outside)"]] == -1
    assert cells("on the lower y face") == [idx(x, 0, 2) for x in range(8, 15)] and cells("on the upper y face") == []
    assert cells("in a cell face inside the grid") == [idx(x, 5, 2) for x in range(2, 11)]
    # the corner: equal boundaries on all three axes, x steps first, then y, then z
    assert cells("through the corner from outside: exact ties")[:7] == [idx(0, 0, 0), idx(1, 0, 0), idx(1, 1, 0), idx(1, 1, 1), idx(2, 1, 1), idx(2, 2, 1),
                                                                       idx(2, 2, 2)]
    assert cells("through the corner, no record")[-1] == idx(6, 6, 5) and len(cells("through the corner, no record")) == 18
    assert cells("along a cell edge diagonal: ties at every step")[:5] == [idx(0, 0, 2), idx(1, 0, 2), idx(1, 1, 2), idx(2, 1, 2), idx(2, 2, 2)]
    assert cells("misses the grid") == [] and cells("points away from the grid") == []
    assert cells("negative directions")[0] == idx(15, 7, 5) and len(cells("negative directions")) == len(set(cells("negative directions")))
    assert cells("a denormal direction component") == [idx(x, 4, 2) for x in range(0, 15)]
    # (it starts on the face y = 0.5 and leaves it downwards at t = -0: the cell above the face first, then the row below)
    assert cells("a negative denormal component on a face") == [idx(0, 5, 2)] + [idx(x, 4, 2) for x in range(0, 15)]
    # a span that ends exactly on a boundary reaches the cell beyond it (b <= t_out), and the point on it belongs to that cell
    assert cells("t_end on a cell boundary") == [idx(0, 4, 2), idx(1, 4, 2), idx(2, 4, 2), idx(3, 4, 2)] and occ[name["t_end on a cell boundary"]] == idx(3, 4, 2)
    assert cells("t_end on a boundary, negative direction") == [idx(15, 4, 2), idx(14, 4, 2), idx(13, 4, 2), idx(12, 4, 2)]
    assert occ[name["t_end on a boundary, negative direction"]] == idx(13, 4, 2)
    assert cells("t_end below t_start") == [] and occ[name["t_end below t_start"]] == idx(2, 4, 2)
    assert cells("t_end equal to t_start") == [idx(2, 4, 2)] and occ[name["t_end equal to t_start"]] == idx(2, 4, 2)
    assert cells("tmax before the far side, no record") == [idx(x, 4, 2) for x in range(1, 6)]
    assert cells("the hit on the grid's upper face: not occupied") == [idx(14, 4, 2), idx(15, 4, 2)]
    assert occ[name["the hit on the grid's upper face: not occupied"]] == -1 and occ[name["the hit on the grid's upper z face"]] == -1
    assert occ[name["the hit on the grid's lower face: occupied"]] == idx(0, 4, 2) and cells("the hit on the grid's lower face: occupied") == [idx(0, 4, 2)]
    assert occ[name["the hit outside the grid"]] == -1 and cells("the hit outside the grid") == [idx(14, 4, 2), idx(15, 4, 2)]
    for k in name:
        if k.startswith("degenerate"):
            assert cells(k) == [] and occ[name[k]] == -1, k
    # the blind zone and the range gate of the header's table; no flag: a ray without a record carves nothing
    for flags, lo, hi in ((0, 0.0, 1e4), (1, 1.5, 4.0), (0, 1.5, 4.0), (1, 1.25, 1.25)):
        _same_walk(capi, ref.grid(flags=flags, min_range=lo, max_range=hi, **HAND_GRID), rays, t_end)
    v0, _ = _same_walk(capi, ref.grid(flags=0, **HAND_GRID), rays, t_end)
    assert not np.any(v0[name["through the corner, no record"]] >= 0)
    v1, o1 = _same_walk(capi, ref.grid(flags=1, min_range=1.5, max_range=4.0, **HAND_GRID), rays, t_end)
    i = name["axis-parallel inside"]            # t = 5 > max_range: free space on [1.5, 4], nothing occupied
    assert [int(c) for c in v1[i] if c >= 0] == [idx(x, 4, 2) for x in range(3, 9)] and o1[i] == -1
    i = name["t_end on a cell boundary"]        # t = 1.25 < min_range: blocked in the blind zone
    assert not np.any(v1[i] >= 0) and o1[i] == -1
    # a rigid transform that is not the identity: the same rays, turned
    vt, ot = _same_walk(capi, g, rays, t_end, rigid_transform())
    assert np.count_nonzero(vt >= 0) > 20 and np.count_nonzero(ot >= 0) > 3
    i = name["axis-parallel inside"]            # o' = (0.25, -4.0, 0.375), d' = (0, 1, 0): enters at t = 2, p' = (0.25, 1.0, 0.375) on a boundary
    assert [int(c) for c in vt[i] if c >= 0] == [idx(8, y, 2) for y in range(0, 7)] and ot[i] == idx(8, 6, 2)
    rng = np.random.default_rng(5)
    _same_walk(capi, g, rays, t_end, rotation(rng))


def test_debug_walk_refuses_bad_arguments(capi):
    L = capi.load()
    g = ref.grid(flags=1, **HAND_GRID)
    d = _desc(capi, g)
    ray = np.array([-5.0, -3.0, -2.0, 0, 1, 1, 1, np.inf], np.float32)
    cells = np.full(32, 0xABABABAB, np.uint32)
    n, occ = ctypes.c_uint32(0), ctypes.c_uint32(0)
    args = lambda **kw: [kw.get(k, v) for k, v in (("grid", ctypes.byref(d)), ("xf", None), ("ray", ray.ctypes.data), ("t", ctypes.c_float(np.nan)),
                                                    ("cells", cells.ctypes.data), ("cap", 32), ("n", ctypes.byref(n)), ("occ", ctypes.byref(occ)))]
    assert L.ls_debug_voxel_walk(*args()) == 0 and n.value == 18
    for kw in (dict(grid=None), dict(ray=None), dict(n=None), dict(occ=None), dict(cells=None)):
        assert L.ls_debug_voxel_walk(*args(**kw)) == INVALID_ARGUMENT, kw
    bad = rigid_transform()
    bad[5] = np.nan
    assert L.ls_debug_voxel_walk(*args(xf=bad.ctypes.data)) == INVALID_ARGUMENT
    zero = _desc(capi, ref.grid((0, 0, 0), 1.0, (0, 1, 1)))
    assert L.ls_debug_voxel_walk(*args(grid=ctypes.byref(zero))) == INVALID_ARGUMENT
    # a capacity below the walk's length: the count comes back, nothing is written past the capacity
    cells[:] = 0xABABABAB
    assert L.ls_debug_voxel_walk(*args(cap=5)) == OUT_OF_RANGE and n.value == 18 and np.all(cells[5:] == 0xABABABAB) and np.all(cells[:5] != 0xABABABAB)
    assert L.ls_debug_voxel_walk(*args(cells=None, cap=0)) == OUT_OF_RANGE and n.value == 18


# ---- the reference against float64 geometry ----------------------------------------------------------------------------------------

def _prototype_cases(rng, n_grids, per_grid):
    """random grids of up to 47 cells per axis at coordinates below 100, each with per_grid rays: random_rays' mix"""
    for _ in range(n_grids):
        dims = [int(x) for x in rng.integers(1, 48, 3)]
        cell = float(rng.choice([0.25, 0.5, 1.0, 0.37, 1.3]))
        origin = rng.uniform(-30.0, 0.0, 3)
        if rng.random() < 0.3:
            origin = np.round(origin)
        g = ref.grid(origin, cell, dims, 1, 0.0, 1e4)
        rays, t_end = random_rays(rng, g, per_grid)
        yield g, rays, t_end


def test_reference_walk_against_float64_segments():
    """every visited cell meets the segment (box inflated by 1e-4), consecutive cells are face neighbours, no cell twice, and no
    float64 sample of the segment that lies more than 1e-3 of a cell from every face falls in a cell the walk did not visit: zero
    exceptions allowed"""
    rng = np.random.default_rng(2)
    n_rays = n_cells = n_samples = 0
    for g, rays, t_end in _prototype_cases(rng, 70, 100):
        keys = np.where(np.isnan(t_end), np.uint64(0xFFFFFFFFFFFFFFFF), t_end.view(np.uint32).astype(np.uint64) << np.uint64(32))
        st = ref.rays_of(g, rays, keys)
        visited = ref.walk(g, st.o, st.d, st.t0, st.t1, st.carve)
        n = rays.shape[0]
        nx, ny, nz = g.dims
        cell, lo = np.float64(g.cell), np.float64(g.origin)
        o, d, t0, t1 = np.float64(st.o), np.float64(st.d), np.float64(st.t0), np.float64(st.t1)
        assert np.all(np.isfinite(t1))
        assert np.all(visited[~st.carve] < 0)
        got = visited >= 0
        c = np.stack([visited % nx, (visited // nx) % ny, visited // (nx * ny)], axis=2)          # (n, trips, 3)
        # no cell twice
        for i in range(n):
            v = visited[i][got[i]]
            assert np.unique(v).shape[0] == v.shape[0], (g, rays[i])
        # face neighbours
        both = got[:, 1:] & got[:, :-1]
        step = np.abs(c[:, 1:] - c[:, :-1]).sum(axis=2)
        assert np.all(step[both] == 1)
        assert not np.any(got[:, 1:] & ~got[:, :-1])
        # every visited cell meets the float64 segment, its box inflated by 1e-4
        blo = lo + c * cell - 1e-4
        bhi = lo + (c + 1) * cell + 1e-4
        with np.errstate(all="ignore"):
            ta = (blo - o[:, None, :]) / d[:, None, :]
            tb = (bhi - o[:, None, :]) / d[:, None, :]
            par = (d == 0)[:, None, :] & np.ones_like(got)[:, :, None]
            inside_slab = (o[:, None, :] >= blo) & (o[:, None, :] <= bhi)
            near = np.where(par, np.where(inside_slab, -np.inf, np.inf), np.minimum(ta, tb)).max(axis=2)
            far = np.where(par, np.where(inside_slab, np.inf, -np.inf), np.maximum(ta, tb)).min(axis=2)
        meets = np.maximum(near, t0[:, None]) <= np.minimum(far, t1[:, None])
        assert np.all(meets[got]), (g, rays[np.nonzero((~meets & got).any(axis=1))[0][:3]])
        # no missed cell: 400 samples of the segment
        walked = st.carve & (t0 <= t1)
        s = t0[:, None] + (t1 - t0)[:, None] * np.linspace(0.0, 1.0, 400)[None, :]
        p = (o[:, None, :] + s[:, :, None] * d[:, None, :] - lo) / cell                              # in cells
        fl = np.floor(p)
        deep = np.all((p - fl > 1e-3) & (fl + 1 - p > 1e-3), axis=2) & np.all((fl >= 0) & (fl < np.float64(g.dims)), axis=2) & walked[:, None]
        ci = (fl[:, :, 2] * ny + fl[:, :, 1]) * nx + fl[:, :, 0]
        for i in np.nonzero(deep.any(axis=1))[0]:
            want = np.unique(ci[i][deep[i]].astype(np.int64))
            missed = np.setdiff1d(want, visited[i][got[i]])
            assert missed.shape[0] == 0, (g, rays[i], t_end[i], missed)
            n_samples += int(deep[i].sum())
        n_rays += n
        n_cells += int(got.sum())
    assert n_rays == 7000 and n_cells > 20000 and n_samples > 100000


def test_reference_counts_follow_the_table_and_the_tie_rule():
    """a hand-made case of the whole reference: the closest record decides, then the lowest geomID; n_free counts rays and leaves
    out the ray's own occupied cell; accumulation adds and takes the minimum"""
    f = lambda x: int(np.float32(x).view(np.uint32))
    g = ref.grid((0, 0, 0), 1.0, (4, 1, 1), 1, 0.0, 10.0)
    rays = np.zeros((3, 8), np.float32)
    rays[:, 0:3] = [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [3.5, 0.5, 0.5]]
    rays[:, 4:7] = [[1, 0, 0], [1, 0, 0], [-1, 0, 0]]
    rays[:, 7] = np.inf
    rec = np.array([[0, 2, 0, f(2.0)], [0, 1, 0, f(2.0)], [0, 0, 0, f(3.0)],       # ray 0: t = 2 decides, geom 1 before geom 2
                    [1, 2, 0, f(1.0)], [1, 0, 5, f(0.5)],                            # ray 1: the closer record's prim is out of range
                    [7, 0, 0, f(1.0)], [2, 3, 0, f(1.0)]], np.uint32)                # a ray out of range, an unknown geometry: ray 2 is a miss
    counts, geom, visited = ref.occupancy(g, rays, rec, {0: 1, 1: 1, 2: 1})
    assert counts[0, 0, :, 0].tolist() == [3, 2, 1, 1] and counts[0, 0, :, 1].tolist() == [0, 1, 1, 0]
    assert geom[0, 0].tolist() == [INV, 2, 1, INV]
    perm = np.random.default_rng(3).permutation(rec.shape[0])
    again = ref.occupancy(g, rays, rec[perm], {0: 1, 1: 1, 2: 1})
    assert again[0].tobytes() == counts.tobytes() and again[1].tobytes() == geom.tobytes()
    acc = ref.occupancy(g, rays, rec, {0: 1, 1: 1, 2: 1}, into=(counts, np.minimum(geom, 1)))
    assert np.array_equal(acc[0], 2 * counts) and acc[1][0, 0].tolist() == [1, 1, 1, 1]
    g0 = ref.grid((0, 0, 0), 1.0, (4, 1, 1), 0, 0.0, 10.0)                           # without the flag the miss carves nothing
    assert ref.occupancy(g0, rays, rec, {0: 1, 1: 1, 2: 1})[0][0, 0, :, 0].tolist() == [2, 1, 0, 0]
