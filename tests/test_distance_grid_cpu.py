"""ls_scene_distance_grid without a device: the symbols and the descriptor, the check's refusals in their order (there is no GPU where
`-m "not gpu"` runs), the numpy restatement of closest_on_triangle against the library's (ls_debug_closest_on_triangle) bit for bit,
the numpy reference against the shared arithmetic's host hook (ls_debug_distance_grid_triangle), cell list and distance bits, the
widened range against the whole grid, and the reference's distances against float64."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np

import distance_grid_reference as ref
from conftest import ROOT
from test_closest_cpu import _check, _min_angle_deg
from test_scene_grid_cpu import random_triangles

INVALID_ARGUMENT, OUT_OF_RANGE = -2, -9
F = np.float32


def _desc(capi, g):
    return capi.DistanceGridDesc.make(g.origin, g.cell, g.dims, g.flags, g.trunc)


def _header(name="lidarshooter_hip.h"):
    return open(os.path.join(ROOT, "include", name)).read()


# ---- the surface -----------------------------------------------------------------------------------------------------------------

def test_symbols_signatures_and_descriptor(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in ("ls_scene_distance_grid", "ls_scene_distance_grid_host", "ls_scene_distance_grid_check"):
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    for s in ("ls_debug_distance_grid_triangle", "ls_debug_distance_grid_queued"):
        assert s in capi.DEBUG_SYMBOLS and hasattr(lib, s), s
    hdr = re.sub(r"\s+", " ", _header())
    assert ("int ls_scene_distance_grid(ls_tracer *tr, void *hip_stream, const ls_distance_grid_desc *grid, const float *sensor_to_grid3x4, "
            "const uint8_t *d_select, uint32_t n_select, void *d_cells);") in hdr
    assert ("int ls_scene_distance_grid_host(ls_tracer *tr, const ls_distance_grid_desc *grid, const float *sensor_to_grid3x4, "
            "const uint8_t *select, uint32_t n_select, void *cells);") in hdr
    assert "int ls_scene_distance_grid_check(const ls_distance_grid_desc *grid);" in hdr
    assert "#define LS_DIST_GRID_ACCUMULATE 1u" in hdr
    dbg = re.sub(r"\s+", " ", _header("lidarshooter_hip_debug.h"))
    assert ("int ls_debug_distance_grid_triangle(const ls_distance_grid_desc *grid, const float tri9[9], uint32_t *cells_out, float *dist_out, "
            "uint32_t capacity, uint32_t *n_cells);") in dbg
    assert "int ls_debug_distance_grid_queued(ls_tracer *tr, uint32_t *n_queued);" in dbg
    D = capi.DistanceGridDesc
    assert ctypes.sizeof(D) == 48 and capi.LS_DIST_GRID_ACCUMULATE == 1
    assert [getattr(D, k).offset for k in ("origin", "cell", "dims", "flags", "trunc", "reserved")] == [0, 12, 16, 28, 32, 36]
    assert capi.DIST_GRID_DTYPE.itemsize == 8 and [capi.DIST_GRID_DTYPE.fields[k][1] for k in ("geom", "dist")] == [0, 4]
    rest = np.zeros(1, capi.DIST_GRID_DTYPE)
    rest["geom"], rest["dist"] = 0xFFFFFFFF, np.inf
    assert rest.view(np.uint64)[0] == capi.DIST_GRID_REST == 0x7F800000FFFFFFFF == int(ref.REST)
    assert capi.load().ls_abi_version() == 4


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    buf = (ctypes.c_uint8 * 64)(*([0xAB] * 64))
    d = capi.DistanceGridDesc.make((0.0, 0.0, 0.0), 1.0, (2, 2, 2), 0, 1.0)
    assert L.ls_scene_distance_grid(None, None, ctypes.byref(d), None, None, 0, buf) == INVALID_ARGUMENT
    assert L.ls_scene_distance_grid_host(None, ctypes.byref(d), None, None, 0, buf) == INVALID_ARGUMENT
    assert bytes(buf) == b"\xab" * 64   # nothing written


def test_the_check_and_its_order(capi):
    L = capi.load()
    make = capi.DistanceGridDesc.make
    check = lambda d: L.ls_scene_distance_grid_check(ctypes.byref(d))

    def desc(origin=(0.0, 0.0, 0.0), cell=1.0, dims=(4, 4, 4), flags=0, trunc=1.0, reserved=(0, 0, 0)):
        d = make(origin, cell, dims, flags, trunc)
        for k in range(3):
            d.reserved[k] = reserved[k]
        return d
    assert L.ls_scene_distance_grid_check(None) == INVALID_ARGUMENT
    assert check(desc()) == 0
    assert check(desc((-3.0, -2.5, -1.5), 0.25, (24, 20, 12), capi.LS_DIST_GRID_ACCUMULATE, 0.6)) == 0
    assert check(desc(cell=0.1, dims=(2048, 2048, 32), trunc=0.0)) == 0
    assert check(desc(dims=(1, 1, 1))) == 0
    for flags in (2, 4, 0x80000000, 3):
        assert check(desc(flags=flags)) == INVALID_ARGUMENT
    for k in range(3):
        assert check(desc(reserved=[int(j == k) for j in range(3)])) == INVALID_ARGUMENT
    for origin in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf)):
        assert check(desc(origin=origin)) == INVALID_ARGUMENT
    for cell in (0.0, -1.0, np.nan, np.inf):
        assert check(desc(cell=cell)) == INVALID_ARGUMENT
    for trunc in (np.nan, -1.0, np.inf, -np.inf, -1e-30):
        assert check(desc(trunc=trunc)) == INVALID_ARGUMENT
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (2049, 1, 1), (1, 2049, 1), (1, 1, 2049), (2048, 2048, 33)):
        assert check(desc(dims=dims)) == OUT_OF_RANGE
    assert check(desc(origin=(3e38, 0.0, 0.0), cell=1e35, dims=(2048, 1, 1))) == OUT_OF_RANGE
    # trunc at 32 cells, the float32 product, and the next float above it
    for cell in (0.3, 0.25, 1.7):
        limit = F(32.0) * F(cell)
        assert check(desc(cell=cell, trunc=limit)) == 0
        assert check(desc(cell=cell, trunc=np.nextafter(limit, F(np.inf)))) == OUT_OF_RANGE
    # the earlier refusal answers: an invalid argument before anything out of range
    assert check(desc(dims=(0, 4, 4), trunc=np.nan)) == INVALID_ARGUMENT
    assert check(desc(dims=(0, 4, 4), trunc=-1.0)) == INVALID_ARGUMENT
    assert check(desc(cell=0.0, dims=(0, 4, 4), trunc=100.0)) == INVALID_ARGUMENT
    assert check(desc(flags=2, trunc=100.0)) == INVALID_ARGUMENT
    assert check(desc(reserved=(0, 0, 7), dims=(4, 4, 0))) == INVALID_ARGUMENT


# ---- closest_on_triangle: numpy against the library ------------------------------------------------------------------------------

def _library_closest(capi, p, a, b, c):
    """ls_debug_closest_on_triangle case by case -> (q (m, 3), d2 (m))"""
    lib = ctypes.CDLL(capi.LIB_PATH)
    fn = lib.ls_debug_closest_on_triangle
    fn.restype = ctypes.c_int
    arrs = [np.ascontiguousarray(x, np.float32) for x in (p, a, b, c)]
    m = arrs[0].shape[0]
    q, d2 = np.zeros((m, 3), np.float32), np.zeros(m, np.float32)
    base = [x.ctypes.data for x in arrs]
    qb, db = q.ctypes.data, d2.ctypes.data
    vp = ctypes.c_void_p
    for i in range(m):
        o = 12 * i
        assert fn(vp(base[0] + o), vp(base[1] + o), vp(base[2] + o), vp(base[3] + o), vp(qb + o), vp(db + 4 * i)) == 0
    return q, d2


def _same_bits(capi, p, a, b, c):
    q, d2, region = ref.closest_on_triangle(p, a, b, c)
    lq, ld2 = _library_closest(capi, p, a, b, c)
    bad = np.nonzero((d2.view(np.uint32) != ld2.view(np.uint32)) | np.any(q.view(np.uint32) != lq.view(np.uint32), axis=1))[0]
    assert bad.shape[0] == 0, (bad.shape[0], bad[:5], q[bad[:2]], lq[bad[:2]], d2[bad[:2]], ld2[bad[:2]], region[bad[:5]])
    return d2, region


def test_numpy_closest_on_triangle_equals_the_library_bit_for_bit(capi):
    """60 000 random cases at each of the scales 1 and 100 (q and d2, four outputs, bit for bit), every one of the seven regions at
    least 1 000 times; then triangles without area, non-finite corners and needles"""
    rng = np.random.default_rng(31)
    seen = np.zeros(7, np.int64)
    for S in (1.0, 100.0):
        m = 60000
        centre = rng.uniform(-0.5, 0.5, (m, 1, 3)) * S
        L = S * 10 ** rng.uniform(-2, -0.3, (m, 1, 1))
        t = centre + rng.uniform(-0.5, 0.5, (m, 3, 3)) * L
        w = rng.uniform(-1.0, 2.0, (m, 3))
        w /= np.where(np.abs(w.sum(axis=1)) > 0.2, w.sum(axis=1), 1.0)[:, None]
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        p = np.einsum("mk,mkj->mj", w, t) + nrm * (rng.uniform(-4, 4, (m, 1)) * L[:, 0] * rng.integers(0, 2, (m, 1)))
        d2, region = _same_bits(capi, F(p), F(t[:, 0]), F(t[:, 1]), F(t[:, 2]))
        assert np.all(region >= 0) and np.all(np.isfinite(d2))
        seen += np.bincount(region, minlength=7)
    assert seen.sum() >= 100000 and seen.min() >= 1000, dict(zip(ref.REGIONS, seen.tolist()))
    # no area, a corner that is not a number, an area that underflows: skipped, q = 0 and d2 = +inf
    z = F([1, 2, 3])
    odd = [(z, z, z), (z, z + 1, z + 2), (z, F([np.nan, 0, 0]), z + 1), (z, F([np.inf, 0, 0]), z + 1), (F([0, 0, 0]), F([1e-30, 0, 0]), F([0, 1e-30, 0])),
           (z, z, z + 1), (F([3e38, 0, 0]), F([-3e38, 0, 0]), F([0, 3e38, 0]))]
    p = np.tile(F([0.5, 0.1, -2]), (len(odd), 1))
    d2, region = _same_bits(capi, p, *[np.stack([t[k] for t in odd]) for k in range(3)])
    assert np.all(region == -1) and np.all(np.isposinf(d2))
    # needles: whatever they give, the same bits
    m = 20000
    S = 10 ** rng.uniform(-1, 3, (m, 1))
    a = rng.uniform(-1, 1, (m, 3)) * S
    e = rng.normal(size=(m, 3))
    e *= S * 10 ** rng.uniform(-3, 0, (m, 1)) / np.linalg.norm(e, axis=1)[:, None]
    b = a + e
    c = a + e * rng.uniform(-0.5, 1.5, (m, 1)) + rng.normal(size=(m, 3)) * np.linalg.norm(e, axis=1)[:, None] * 10 ** rng.uniform(-9, -2, (m, 1))
    p = a + rng.normal(size=(m, 3)) * np.linalg.norm(e, axis=1)[:, None] * 10 ** rng.uniform(-3, 1, (m, 1))
    d2, region = _same_bits(capi, F(p), F(a), F(b), F(c))
    assert np.count_nonzero(region >= 0) > 10000 and np.count_nonzero(region == -1) > 10


# ---- the reference against the host hook -----------------------------------------------------------------------------------------

GRID = dict(origin=(-3.0, -2.5, -1.5), cell=0.25, dims=(24, 20, 12))


def _hook(L, d, tri9, capacity):
    t = np.ascontiguousarray(tri9, np.float32).reshape(9)
    cells = np.full(capacity + 4, 0xABABABAB, np.uint32)
    dist = np.full(capacity + 4, -7.0, np.float32)
    n = ctypes.c_uint32(0xFFFFFFFF)
    rc = L.ls_debug_distance_grid_triangle(ctypes.byref(d), t.ctypes.data, cells.ctypes.data if capacity else None, dist.ctypes.data if capacity else None,
                                           capacity, ctypes.byref(n))
    assert np.all(cells[capacity:] == 0xABABABAB) and np.all(dist[capacity:] == -7.0)
    return rc, n.value, cells[:capacity], dist[:capacity]


def _hook_equals_reference(capi, g, tris):
    """-> the number of counting cells of every triangle"""
    L = capi.load()
    d = _desc(capi, g)
    tri, cell, dist, _ = ref.counted(g, tris)
    order = np.lexsort((cell, tri))
    tri, cell, dist = tri[order], cell[order], dist[order]
    first = np.searchsorted(tri, np.arange(tris.shape[0] + 1))
    cap = g.dims[0] * g.dims[1] * g.dims[2]
    for i in range(tris.shape[0]):
        want_c, want_d = cell[first[i]:first[i + 1]], dist[first[i]:first[i + 1]]
        rc, n, got_c, got_d = _hook(L, d, tris[i], cap)
        assert rc == 0 and n == want_c.shape[0], (i, n, want_c.shape[0])
        assert np.array_equal(got_c[:n], want_c.astype(np.uint32)), i
        assert np.array_equal(got_d[:n].view(np.uint32), want_d.view(np.uint32)), i
    return np.diff(first)


def test_host_hook_equals_the_reference(capi):
    """cell list and distance bits over 1 200 random triangles (some reach over the grid's sides, some lie outside it, one in 17 has
    no area and never counts, one in 23 lies in a cell-face plane), at a band of 2.4 cells and of 0.9"""
    rng = np.random.default_rng(77)
    for trunc, n in ((0.6, 700), (0.225, 500)):
        g = ref.grid(trunc=trunc, **GRID)
        tris = random_triangles(rng, g, n, 0.02, 2.0)
        counts = _hook_equals_reference(capi, g, tris)
        flat = np.arange(n) % 17 == 5
        assert np.all(counts[flat] == 0) and np.count_nonzero(counts) > n // 2


def _cells(x, y, z):
    """a point given in cells of GRID (exact: the cell is a power of two)"""
    return [-3.0 + 0.25 * x, -2.5 + 0.25 * y, -1.5 + 0.25 * z]


def test_hand_made_triangles(capi):
    """vertices exactly on cell planes and at cell centres (dist == 0); triangles outside the grid but within trunc of it contribute,
    triangles farther than trunc contribute nothing; trunc = 0; a capacity too small; the hook's refusals"""
    L = capi.load()
    nx, ny, nz = GRID["dims"]
    at = lambda x, y, z: (z * ny + y) * nx + x
    g = ref.grid(trunc=0.5, **GRID)
    centres = [_cells(3.5, 4.5, 5.5), _cells(7.5, 4.5, 5.5), _cells(3.5, 9.5, 6.5)]
    planes = [_cells(10.0, 10.0, 4.0), _cells(14.0, 10.0, 4.0), _cells(10.0, 13.0, 4.0)]
    below = [_cells(5.0, 5.0, -1.5), _cells(9.0, 5.0, -1.5), _cells(5.0, 9.0, -1.5)]        # 2 cells below the lowest centres: dist == trunc
    beside = [_cells(-1.25, 3.0, 3.0), _cells(-1.25, 8.0, 3.0), _cells(-1.25, 3.0, 8.0)]    # 1.75 cells left of the first centres
    above = [_cells(24.5, 20.5, 12.5), _cells(26.5, 20.5, 12.5), _cells(24.5, 22.5, 12.5)]  # beyond the far corner, within reach of its cell
    far = [[_cells(5.0, 5.0, -1.75), _cells(9.0, 5.0, -1.75), _cells(5.0, 9.0, -1.75)],     # a quarter cell too far below
           [_cells(-2.0, 3.0, 3.0), _cells(-2.0, 8.0, 3.0), _cells(-2.0, 3.0, 8.0)],
           [_cells(30.0, 3.0, 3.0), _cells(30.0, 8.0, 3.0), _cells(33.0, 3.0, 8.0)],
           [_cells(5.0, -4.0, 3.0), _cells(9.0, -4.0, 3.0), _cells(5.0, -4.0, 8.0)],
           [_cells(5.0, 24.0, 3.0), _cells(9.0, 24.0, 3.0), _cells(5.0, 24.0, 8.0)],
           [_cells(5.0, 5.0, 15.0), _cells(9.0, 5.0, 15.0), _cells(5.0, 9.0, 15.0)]]
    tris = np.array([centres, planes, below, beside, above] + far, np.float32)
    counts = _hook_equals_reference(capi, g, tris)
    assert np.all(counts[:5] > 0) and np.all(counts[5:] == 0), counts
    c, d = ref.triangle_cells(g, tris[0])
    for x, y, z in ((3, 4, 5), (7, 4, 5), (3, 9, 6)):
        assert d[np.nonzero(c == at(x, y, z))[0][0]] == 0.0
    c, d = ref.triangle_cells(g, tris[2])
    assert np.all(d == F(0.5)) and set(c.tolist()) <= {at(x, y, 0) for x in range(24) for y in range(20)} and at(5, 5, 0) in c.tolist()
    c, d = ref.triangle_cells(g, tris[3])
    assert np.all(c % nx == 0) and d.min() == F(0.4375) and d.max() <= F(0.5)
    c, d = ref.triangle_cells(g, tris[4])
    assert c.tolist() == [at(23, 19, 11)]
    # trunc = 0: only the cells whose centre lies on the triangle
    g0 = ref.grid(trunc=0.0, **GRID)
    inplane = [_cells(3.5, 4.5, 5.5), _cells(7.5, 4.5, 5.5), _cells(3.5, 8.5, 5.5)]
    counts = _hook_equals_reference(capi, g0, np.array([centres, planes, inplane], np.float32))
    assert counts[1] == 0 and counts[0] >= 3 and counts[2] >= 5 + 4 + 3 + 2 + 1
    c, d = ref.triangle_cells(g0, inplane)
    assert np.all(d == 0.0) and {at(3, 4, 5), at(7, 4, 5), at(3, 8, 5), at(5, 6, 5)} <= set(c.tolist())
    # a capacity too small: the count is the full one, the lists are cut, nothing behind them is written
    d_ = _desc(capi, g)
    want_c, want_d = ref.triangle_cells(g, tris[3])
    rc, n, got_c, got_d = _hook(L, d_, tris[3], 3)
    assert rc == OUT_OF_RANGE and n == want_c.shape[0] and got_c.tolist() == want_c[:3].tolist() and got_d.tolist() == want_d[:3].tolist()
    rc, n, _, _ = _hook(L, d_, tris[3], 0)
    assert rc == OUT_OF_RANGE and n == want_c.shape[0]
    # non-finite vertices: nothing
    for bad in (np.nan, np.inf, -np.inf):
        t = tris[0].copy()
        t[1, 2] = bad
        rc, n, _, _ = _hook(L, d_, t, 16)
        assert rc == 0 and n == 0 and ref.triangle_cells(g, t)[0].size == 0
    # refusals
    nn = ctypes.c_uint32(0)
    tt = np.ascontiguousarray(tris[0]).reshape(9)
    oc, od = np.zeros(8, np.uint32), np.zeros(8, np.float32)
    hook = L.ls_debug_distance_grid_triangle
    assert hook(None, tt.ctypes.data, oc.ctypes.data, od.ctypes.data, 8, ctypes.byref(nn)) == INVALID_ARGUMENT
    assert hook(ctypes.byref(d_), None, oc.ctypes.data, od.ctypes.data, 8, ctypes.byref(nn)) == INVALID_ARGUMENT
    assert hook(ctypes.byref(d_), tt.ctypes.data, oc.ctypes.data, od.ctypes.data, 8, None) == INVALID_ARGUMENT
    assert hook(ctypes.byref(d_), tt.ctypes.data, None, od.ctypes.data, 8, ctypes.byref(nn)) == INVALID_ARGUMENT
    assert hook(ctypes.byref(d_), tt.ctypes.data, oc.ctypes.data, None, 8, ctypes.byref(nn)) == INVALID_ARGUMENT
    bad = capi.DistanceGridDesc.make((0.0, 0.0, 0.0), 1.0, (4, 4, 4), 0, 33.0)
    assert hook(ctypes.byref(bad), tt.ctypes.data, oc.ctypes.data, od.ctypes.data, 8, ctypes.byref(nn)) == INVALID_ARGUMENT


# ---- the range is conservative ---------------------------------------------------------------------------------------------------

def test_the_widened_range_leaves_out_no_counting_cell():
    """The reference run over ALL cells of the grid gives the same bytes as the reference over the widened ranges: 2 000 random
    triangles on a 16 x 14 x 12 grid of 0.25 m cells at a band of 2.4 cells and 1 000 on a 12 x 12 x 8 grid of 0.5 m cells far from the
    origin at a band of 1.3.  This holds for coordinates with |q| / cell < 2^20: beyond that the rounding of (q -+ trunc) / cell and of
    the centre's product reaches the half cell that the range keeps in hand (a float32 has 24 bits: at 2^20 cells an ulp of the
    quotient is 1/16 of a cell)."""
    sets = ((dict(origin=(-2.0, -1.75, -1.5), cell=0.25, dims=(16, 14, 12)), 0.6, 2000, 0.02, 1.5, 11),
            (dict(origin=(37.0, -52.0, 3.0), cell=0.5, dims=(12, 12, 8)), 0.65, 1000, 0.06, 4.0, 12))
    for gd, trunc, n, a, b, seed in sets:
        g = ref.grid(trunc=trunc, **gd)
        tris = random_triangles(np.random.default_rng(seed), g, n, a, b)
        q, ok, _, _ = ref.ranges(g, tris)
        assert np.abs(q[np.isfinite(q)]).max() / g.cell < 2 ** 20
        geom = (np.arange(n) % 5).astype(np.uint32)
        by_range = ref.distance_grid(g, tris, geom)
        by_all = ref.distance_grid(g, tris, geom, all_cells=True)
        assert by_range.tobytes() == by_all.tobytes()
        assert np.count_nonzero(by_range != ref.REST) > by_range.size // 2 and np.count_nonzero(~ok) > 20


# ---- the reference against float64 -----------------------------------------------------------------------------------------------

def test_reference_distances_against_float64():
    """The distances the reference sends, against test_closest_cpu's float64 brute force within that file's own bound (2e-6 * S on
    dist and q, S the largest |coordinate| among the centre and the corners, derived there for triangles whose smallest angle is at
    least 20 degrees): its _check, given the numpy restatement in the library's place, over 3 000 of the counting pairs."""
    rng = np.random.default_rng(5)
    g = ref.grid(trunc=0.6, **GRID)
    tris = random_triangles(rng, g, 900, 0.05, 2.0)
    q, ok, _, _ = ref.ranges(g, tris)
    with np.errstate(all="ignore"):   # (a triangle without area has no angles: left out)
        keep = np.array([bool(ok[i]) and np.ptp(q[i], axis=0).max() > 0 and _min_angle_deg(*q[i]) >= 20.0 for i in range(tris.shape[0])])
    tris, q = tris[keep], q[keep]
    assert tris.shape[0] > 400
    tri, cell, dist, tested = ref.counted(g, tris)
    assert tested > 100000 and tri.shape[0] > 30000
    nx, ny, _ = g.dims
    c = np.stack([cell % nx, (cell // nx) % ny, cell // (nx * ny)], axis=1)
    ctr = (c.astype(np.float32) + F(0.5)) * g.cell

    def restated(p, a, b, cc):
        qq, d2, _ = ref.closest_on_triangle(p[None], a[None], b[None], cc[None])
        return qq[0], d2[0]
    shim = SimpleNamespace(closest_on_triangle=restated)
    seen = set()
    for k in rng.choice(tri.shape[0], 3000, replace=False):
        region, d2 = _check(shim, ctr[k], q[tri[k], 0], q[tri[k], 1], q[tri[k], 2])
        assert np.sqrt(F(d2)).view(np.uint32) == dist[k].view(np.uint32)
        seen.add(region)
    assert seen == {"A", "B", "C", "AB", "AC", "BC", "F"}
