"""ls_scene_grid without a device: the descriptor's refusals (there is no GPU where `-m "not gpu"` runs), the shared arithmetic
through its host hook (ls_debug_scene_grid_triangle) against the numpy reference, cell list for cell list, and the reference itself
against float64 geometry."""
import ctypes

import numpy as np

import scene_grid_reference as ref

INVALID_ARGUMENT, OUT_OF_RANGE = -2, -9
F = np.float32

# the two sets of the float64 check: (grid, triangles, smallest and largest size in metres, seed)
SETS = ((dict(origin=(-3.0, -2.5, -1.5), cell=0.25, dims=(24, 20, 12)), 1500, 0.02, 2.0, 101),
        (dict(origin=(37.0, -52.0, 3.0), cell=0.5, dims=(16, 16, 8)), 600, 0.06, 6.0, 202))


def _desc(capi, g):
    return capi.SceneGridDesc.make(g.origin, g.cell, g.dims, g.flags)


def random_triangles(rng, g, n, smallest, largest):
    """n triangles float32 (n, 3, 3) around grid g, vertices within a uniform size in [smallest, largest] of a centre: one in 17 collapsed to a segment, one in
    23 snapped into a cell-face plane; some reach over the grid's sides and some lie wholly outside"""
    lo = np.float64(g.origin)
    ext = np.float64(g.dims) * np.float64(g.cell)
    centre = lo + rng.uniform(-0.15, 1.15, (n, 3)) * ext
    size = rng.uniform(smallest, largest, n)
    v = centre[:, None, :] + size[:, None, None] * rng.uniform(-1.0, 1.0, (n, 3, 3))
    seg = np.arange(n) % 17 == 5
    v[seg, 2] = v[seg, 1]                                   # a segment: two vertices coincide
    snap = np.nonzero(np.arange(n) % 23 == 7)[0]
    axis = rng.integers(0, 3, snap.shape[0])
    plane = np.round((v[snap, 0, axis] - lo[axis]) / np.float64(g.cell))
    v[snap, :, axis] = (lo[axis] + plane * np.float64(g.cell))[:, None]
    return v.astype(np.float32)


_sets = {}


def _set(k):
    """grid, triangles and the reference's marked pairs of set k: computed once"""
    if k not in _sets:
        gd, n, a, b, seed = SETS[k]
        g = ref.grid(**gd)
        tris = random_triangles(np.random.default_rng(seed), g, n, a, b)
        tri, cell, tested = ref.marked(g, tris)
        _sets[k] = (g, tris, tri, cell, tested)
    return _sets[k]


def _sat64(q, c, cell, grow):
    """the 13 axes in float64 for pairs q (m, 3, 3), c (m, 3), the box grown by `grow` per side -> overlaps bool (m)"""
    h = 0.5 * cell + grow
    p = q - ((c + 0.5) * cell)[:, None, :]
    sep = np.zeros(q.shape[0], bool)
    for a in range(3):
        sep |= (p[:, :, a].min(axis=1) > h) | (p[:, :, a].max(axis=1) < -h)
    e = [q[:, 1] - q[:, 0], q[:, 2] - q[:, 1], q[:, 0] - q[:, 2]]
    for ej in e:
        for i in range(3):
            u = np.zeros(3)
            u[i] = 1.0
            ax = np.cross(u[None, :], ej)
            proj = np.einsum("mkj,mj->mk", p, ax)
            r = h * np.abs(ax).sum(axis=1)
            sep |= (proj.min(axis=1) > r) | (proj.max(axis=1) < -r)
    n = np.cross(e[0], e[1])
    d = np.einsum("mj,mj->m", n, p[:, 0])
    r = h * np.abs(n).sum(axis=1)
    sep |= (d > r) | (d < -r)
    return ~sep


def test_reference_against_float64_geometry():
    """Condition 1: no cell is missed in which a float64 sample of the triangle lies at least 1e-3 of a cell deep.  Condition 2: no
    cell is marked whose box, grown by 1e-3 of a cell per side, a float64 run of the same 13 axes finds disjoint from the triangle.
    Both without exception, over 1 500 triangles of 0.02 - 2 m on a 24 x 20 x 12 grid of 0.25 m cells and 600 of 0.06 - 6 m on a 16 x
    16 x 8 grid of 0.5 m cells far from the origin."""
    rng = np.random.default_rng(5)
    pairs_tested = pairs_marked = samples_checked = 0
    for k in range(len(SETS)):
        g, tris, tri, cell, tested = _set(k)
        nx, ny, nz = g.dims
        cw = np.float64(g.cell)
        q64 = tris.astype(np.float64) - np.float64(g.origin)[None, None, :]
        pairs_tested += tested
        pairs_marked += tri.shape[0]
        marked = set(zip(tri.tolist(), cell.tolist()))
        # 1. samples: the vertices, points on the edges and in the interior
        S = 48
        w = rng.dirichlet([1.0, 1.0, 1.0], (tris.shape[0], S))
        w[:, 0:3] = np.eye(3)[None]
        w[:, 3:12, :] = 0.0
        t = rng.random((tris.shape[0], 9))
        for j in range(9):                                   # three points on each edge
            a, b = j % 3, (j + 1) % 3
            w[:, 3 + j, a], w[:, 3 + j, b] = t[:, j], 1.0 - t[:, j]
        pts = np.einsum("nsk,nkj->nsj", w, q64)
        f = np.floor(pts / cw)
        depth = np.minimum(pts / cw - f, f + 1.0 - pts / cw).min(axis=2)
        inside = np.all((f >= 0) & (f < np.float64(g.dims)), axis=2) & (depth >= 1e-3)
        ti, si = np.nonzero(inside)
        ci = f[ti, si].astype(np.int64)
        word = (ci[:, 2] * ny + ci[:, 1]) * nx + ci[:, 0]
        missed = [(a, b) for a, b in set(zip(ti.tolist(), word.tolist())) if (a, b) not in marked]
        assert not missed, ("missed", k, missed[:5])
        samples_checked += ti.shape[0]
        # 2. the marked cells, grown, in float64
        c = np.stack([cell % nx, (cell // nx) % ny, cell // (nx * ny)], axis=1).astype(np.float64)
        ok = _sat64(q64[tri], c, cw, 1e-3 * cw)
        assert np.all(ok), ("marked, but disjoint in float64", k, tri[~ok][:5], cell[~ok][:5])
    print("pairs tested", pairs_tested, "marked", pairs_marked, "samples inside", samples_checked)
    assert pairs_tested > 100000 and pairs_marked > 10000 and samples_checked > 30000


def test_reference_marks_what_a_coarser_look_expects():
    """hand-made triangles on a 4 x 4 x 4 grid of unit cells: an axis-aligned one inside one layer, vertices on cell-boundary planes, a segment, a point, one wholly outside"""
    g = ref.grid((0.0, 0.0, 0.0), 1.0, (4, 4, 4))
    w = lambda x, y, z: (z * 4 + y) * 4 + x
    flat = [0.25, 0.25, 0.5, 1.5, 0.25, 0.5, 0.25, 1.5, 0.5]
    assert ref.triangle_cells(g, flat).tolist() == sorted([w(0, 0, 0), w(1, 0, 0), w(0, 1, 0)])   # the hypotenuse misses cell (1, 1, 0)
    touch = [0.25, 0.25, 0.5, 1.75, 0.25, 0.5, 0.25, 1.75, 0.5]                                  # ... and here touches its corner
    assert ref.triangle_cells(g, touch).tolist() == sorted([w(0, 0, 0), w(1, 0, 0), w(0, 1, 0), w(1, 1, 0)])
    point = [2.0, 2.0, 2.0] * 3
    assert ref.triangle_cells(g, point).tolist() == [w(2, 2, 2)]   # the range is floor's: a face plane belongs to the cell above it
    upto = [1.25, 1.25, 1.5, 2.0, 1.25, 1.5, 1.25, 2.0, 1.5]       # ... and a range that ends on one reaches that cell: it touches
    assert ref.triangle_cells(g, upto).tolist() == sorted([w(1, 1, 1), w(2, 1, 1), w(1, 2, 1)])
    corner = [0.0, 0.0, 0.0] * 3                             # the range is clamped: only the grid's own cell
    assert ref.triangle_cells(g, corner).tolist() == [0]
    seg = [0.5, 0.5, 0.5, 3.5, 0.5, 0.5, 3.5, 0.5, 0.5]
    assert ref.triangle_cells(g, seg).tolist() == [w(x, 0, 0) for x in range(4)]
    assert ref.triangle_cells(g, [5.0, 0.5, 0.5, 6.0, 0.5, 0.5, 5.0, 1.5, 0.5]).size == 0
    assert ref.triangle_cells(g, [-2.0, 0.5, 0.5, -1.0, 0.5, 0.5, -2.0, 1.5, 0.5]).size == 0
    half = [-1.5, 0.5, 0.5, 1.5, 0.5, 0.5, 1.5, 0.6, 0.5]    # half outside: clipped by the grid
    assert ref.triangle_cells(g, half).tolist() == [w(0, 0, 0), w(1, 0, 0)]
    assert ref.triangle_cells(g, [np.nan, 0.5, 0.5, 1.5, 0.5, 0.5, 1.5, 0.6, 0.5]).size == 0
    assert ref.triangle_cells(g, [np.inf, 0.5, 0.5, 1.5, 0.5, 0.5, 1.5, 0.6, 0.5]).size == 0


def _hook(capi, L, d, tri9, capacity):
    t = np.ascontiguousarray(tri9, np.float32).reshape(9)
    out = np.full(capacity + 4, 0xABABABAB, np.uint32)
    n = ctypes.c_uint32(0xFFFFFFFF)
    rc = L.ls_debug_scene_grid_triangle(ctypes.byref(d), t.ctypes.data, out.ctypes.data if capacity else None, capacity, ctypes.byref(n))
    assert np.all(out[capacity:] == 0xABABABAB)
    return rc, n.value, out[:capacity]


def test_host_hook_equals_the_reference(capi):
    """ls_debug_scene_grid_triangle against the reference, cell list for cell list, over the triangles of the float64 check (ranges
    clipped by the grid and triangles wholly outside among them), the hand-made ones, a non-finite vertex and a capacity too small"""
    L = capi.load()
    lists = with_cells = clipped = outside = 0
    for k in range(len(SETS)):
        g, tris, tri, cell, _ = _set(k)
        d = _desc(capi, g)
        order = np.lexsort((cell, tri))
        tri_s, cell_s = tri[order], cell[order]
        first = np.searchsorted(tri_s, np.arange(tris.shape[0] + 1))
        q, ok, lo, hi = ref.ranges(g, tris)
        ext = np.float32(g.dims) * g.cell
        for i in range(tris.shape[0]):
            want = cell_s[first[i]:first[i + 1]]
            rc, n, got = _hook(capi, L, d, tris[i], 4096)
            assert rc == 0 and n == want.shape[0], (k, i)
            assert np.array_equal(got[:n], want.astype(np.uint32)), (k, i)
            lists += 1
            with_cells += n > 0
            outside += not ok[i]
            clipped += bool(ok[i] and (np.any(q[i] < 0) or np.any(q[i] >= ext[None, :])))
    assert lists == 2100 and with_cells > 1200 and clipped > 100 and outside > 50
    g = ref.grid((0.0, 0.0, 0.0), 1.0, (4, 4, 4))
    d = _desc(capi, g)
    nan, inf = np.nan, np.inf
    for t in ([0.25, 0.25, 0.5, 1.75, 0.25, 0.5, 0.25, 1.75, 0.5], [2.0, 2.0, 2.0] * 3, [0.0, 0.0, 0.0] * 3, [4.0, 4.0, 4.0] * 3,
              [0.5, 0.5, 0.5, 3.5, 0.5, 0.5, 3.5, 0.5, 0.5], [5.0, 0.5, 0.5, 6.0, 0.5, 0.5, 5.0, 1.5, 0.5], [-1.5, 0.5, 0.5, 1.5, 0.5, 0.5, 1.5, 0.6, 0.5],
              [nan, 0.5, 0.5, 1.5, 0.5, 0.5, 1.5, 0.6, 0.5], [0.5, 0.5, -inf, 1.5, 0.5, 0.5, 1.5, 0.6, 0.5], [3e38, 0.5, 0.5, -3e38, 0.5, 0.5, 0.0, 3e38, 0.5],
              [-1.0, -1.0, -1.0, 9.0, -1.0, 2.0, -1.0, 9.0, 5.0]):
        want = ref.triangle_cells(g, t)
        rc, n, got = _hook(capi, L, d, t, 64)
        assert rc == 0 and n == want.shape[0] and np.array_equal(got[:n], want), t
    # a capacity too small: the count is the full one, the list is cut, nothing behind it is written
    t = [0.5, 0.5, 0.5, 3.5, 0.5, 0.5, 3.5, 0.5, 0.5]
    rc, n, got = _hook(capi, L, d, t, 3)
    assert rc == OUT_OF_RANGE and n == 4 and got.tolist() == [0, 1, 2]
    rc, n, got = _hook(capi, L, d, t, 0)
    assert rc == OUT_OF_RANGE and n == 4
    rc, n, got = _hook(capi, L, d, t, 4)
    assert rc == 0 and n == 4
    # refusals
    nn = ctypes.c_uint32(0)
    tt = np.array(t, np.float32)
    out = np.zeros(8, np.uint32)
    assert L.ls_debug_scene_grid_triangle(None, tt.ctypes.data, out.ctypes.data, 8, ctypes.byref(nn)) == INVALID_ARGUMENT
    assert L.ls_debug_scene_grid_triangle(ctypes.byref(d), None, out.ctypes.data, 8, ctypes.byref(nn)) == INVALID_ARGUMENT
    assert L.ls_debug_scene_grid_triangle(ctypes.byref(d), tt.ctypes.data, out.ctypes.data, 8, None) == INVALID_ARGUMENT
    assert L.ls_debug_scene_grid_triangle(ctypes.byref(d), tt.ctypes.data, None, 8, ctypes.byref(nn)) == INVALID_ARGUMENT
    bad = capi.SceneGridDesc.make((0.0, 0.0, 0.0), 1.0, (4, 4, 0))
    assert L.ls_debug_scene_grid_triangle(ctypes.byref(bad), tt.ctypes.data, out.ctypes.data, 8, ctypes.byref(nn)) == INVALID_ARGUMENT


def test_descriptor_and_its_check(capi):
    L = capi.load()
    assert ctypes.sizeof(capi.SceneGridDesc) == 32 and capi.LS_SCENE_GRID_ACCUMULATE == 1
    make = capi.SceneGridDesc.make
    check = lambda d: L.ls_scene_grid_check(ctypes.byref(d))
    assert L.ls_scene_grid_check(None) == INVALID_ARGUMENT
    assert check(make((-3.0, -2.5, -1.5), 0.25, (24, 20, 12))) == 0
    assert check(make((0.0, 0.0, 0.0), 0.1, (2048, 2048, 32), capi.LS_SCENE_GRID_ACCUMULATE)) == 0
    assert check(make((0.0, 0.0, 0.0), 1.0, (1, 1, 1))) == 0
    for flags in (2, 4, 0x80000000, 3):
        assert check(make((0.0, 0.0, 0.0), 1.0, (4, 4, 4), flags)) == INVALID_ARGUMENT
    for origin in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf)):
        assert check(make(origin, 1.0, (4, 4, 4))) == INVALID_ARGUMENT
    for cell in (0.0, -1.0, np.nan, np.inf):
        assert check(make((0.0, 0.0, 0.0), cell, (4, 4, 4))) == INVALID_ARGUMENT
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (2049, 1, 1), (1, 2049, 1), (1, 1, 2049), (2048, 2048, 33)):
        assert check(make((0.0, 0.0, 0.0), 1.0, dims)) == OUT_OF_RANGE
    assert check(make((3e38, 0.0, 0.0), 1e35, (2048, 1, 1))) == OUT_OF_RANGE
    # the earlier refusal answers: flags before the cell, the cell before a dimension
    assert check(make((0.0, 0.0, 0.0), 0.0, (0, 4, 4), 2)) == INVALID_ARGUMENT
    assert check(make((0.0, 0.0, 0.0), 0.0, (0, 4, 4))) == INVALID_ARGUMENT
