"""The numpy reference of ls_occupancy_grid (include/lidarshooter_hip.h): the counting rule (labels_reference's), the closest record per
ray, the affine, the header's per-ray table and the walk, restated over float32 arrays -- every operation one numpy operation on
float32, so every operation rounds once -- and vectorised over the rays: one trip of the loop moves every ray that still walks."""
from types import SimpleNamespace

import numpy as np

import labels_reference as lref

INV = 0xFFFFFFFF
CARVE_MISSES, ACCUMULATE = 1, 2
F = np.float32


def grid(origin, cell, dims, flags=0, min_range=0.0, max_range=1e4):
    """the descriptor's fields as the reference reads them (a capi.OccupancyGridDesc has the same names)"""
    return SimpleNamespace(origin=[F(x) for x in origin], cell=F(cell), dims=[int(x) for x in dims], flags=int(flags), min_range=F(min_range),
                           max_range=F(max_range))


def own_rays(dirs):
    """the handle's own rays as 32-byte records: origin 0, tmin 0, the nominal direction, tmax +inf"""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    r = np.zeros((d.shape[0], 8), np.float32)
    r[:, 4:7], r[:, 7] = d, np.inf
    return r


def to_grid(m, o, d):
    """ls_cloud_to_world's order: ((m0 x + m1 y) + m2 z) + m3 for the origin, the direction without the translation"""
    m = np.ascontiguousarray(m, np.float32).reshape(3, 4)
    with np.errstate(all="ignore"):
        o2 = np.stack([((m[i, 0] * o[:, 0] + m[i, 1] * o[:, 1]) + m[i, 2] * o[:, 2]) + m[i, 3] for i in range(3)], axis=1)
        d2 = np.stack([(m[i, 0] * d[:, 0] + m[i, 1] * d[:, 1]) + m[i, 2] * d[:, 2] for i in range(3)], axis=1)
    assert o2.dtype == np.float32 and d2.dtype == np.float32
    return o2, d2


def closest_records(records, geoms, ray_bound, rays=None):
    """-> uint64[ray_bound]: per ray the smallest (t bits << 32) | geom among its counted records, ~0 where it has none.
    rays: the caller's (for the walkable test), None for the handle's own"""
    rec = np.asarray(records, np.uint32).reshape(-1, 4)
    keys = np.full(ray_bound, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    if rec.shape[0] == 0 or ray_bound == 0 or not geoms:
        return keys
    ok = lref.counted(rec, geoms, max(geoms) + 1, ray_bound, rays)
    k = ((rec[ok, 3] & np.uint32(0x7FFFFFFF)).astype(np.uint64) << np.uint64(32)) | rec[ok, 1].astype(np.uint64)
    np.minimum.at(keys, rec[ok, 0].astype(np.int64), k)
    return keys


def cell_of(g, p):
    """(index int64, inside bool) of points p (n, 3): floor((p - origin) / cell) per axis, compared as floats against [0, n)"""
    with np.errstate(all="ignore"):
        f = np.stack([np.floor((p[:, a] - g.origin[a]) / g.cell) for a in range(3)], axis=1)
        inside = np.all((f >= 0) & (f < np.float32(g.dims)[None, :]), axis=1)
    c = np.where(inside[:, None], f, 0).astype(np.int64)
    return (c[:, 2] * g.dims[1] + c[:, 1]) * g.dims[0] + c[:, 0], inside


def walk(g, o, d, t0, t1, go):
    """the walk of csrc/ls_voxel.h for every ray with go set, on [t0, t1] -> int64 (n, trips): the cells in the order visited, -1 behind
    a ray's last one"""
    n = o.shape[0]
    cell = g.cell
    dims = np.array(g.dims, np.int64)
    with np.errstate(all="ignore"):
        q = np.stack([o[:, a] - g.origin[a] for a in range(3)], axis=1)
        E = [F(g.dims[a]) * cell for a in range(3)]
        t_in, t_out = t0.copy(), t1.copy()
        live = go.copy()
        for a in range(3):
            zero = d[:, a] == 0
            live &= ~(zero & ~((q[:, a] >= 0) & (q[:, a] < E[a])))
            ta, tb = (F(0) - q[:, a]) / d[:, a], (E[a] - q[:, a]) / d[:, a]
            t_in = np.where(zero, t_in, np.fmax(t_in, np.fmin(ta, tb)))
            t_out = np.where(zero, t_out, np.fmin(t_out, np.fmax(ta, tb)))
        live &= t_in <= t_out
        c = np.zeros((n, 3), np.int64)
        for a in range(3):
            e = q[:, a] + t_in * d[:, a]
            f = np.floor(e / cell)
            f = np.fmin(np.fmax(f, F(0)), F(g.dims[a] - 1))
            c[:, a] = np.where(live, f, 0).astype(np.int64)
        up = (d > 0).astype(np.int64)

        def boundary(cc, a, rows):
            return ((cc + up[rows, a]).astype(np.float32) * cell - q[rows, a]) / d[rows, a]
        every = np.arange(n)
        b = np.stack([np.where(d[:, a] == 0, F(np.inf), boundary(c[:, a], a, every)) for a in range(3)], axis=1).astype(np.float32)
        assert q.dtype == np.float32 and b.dtype == np.float32 and t_in.dtype == np.float32 and t_out.dtype == np.float32
        out = []
        while np.any(live):
            out.append(np.where(live, (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0], -1))
            assert len(out) <= sum(g.dims), "the walk takes at most nx + ny + nz trips"
            a = np.zeros(n, np.int64)
            bb = b[:, 0].copy()
            s = b[:, 1] < bb
            a[s], bb[s] = 1, b[s, 1]
            s = b[:, 2] < bb
            a[s], bb[s] = 2, b[s, 2]
            live &= bb <= t_out
            rows = np.nonzero(live)[0]
            ar = a[rows]
            c[rows, ar] += np.where(d[rows, ar] > 0, 1, -1)
            inside = (c[rows, ar] >= 0) & (c[rows, ar] < dims[ar])
            live[rows[~inside]] = False
            rows, ar = rows[inside], ar[inside]
            b[rows, ar] = boundary(c[rows, ar], ar, rows)
    return np.stack(out, axis=1) if out else np.full((n, 0), -1, np.int64)


def rays_of(g, rays, keys, own=False, xf=None):
    """the header's per-ray table -> SimpleNamespace(o, d: the ray in the grid's frame; t0, t1, carve: the span and whether anything is
    carved; occ: the occupied cell or -1; geom: the deciding record's geomID)"""
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    walkable = np.ones(r.shape[0], bool) if own else lref.rays_walked(r)
    o, d, tmin, tmax = r[:, 0:3].copy(), r[:, 4:7].copy(), r[:, 3].copy(), r[:, 7].copy()
    if xf is not None:
        o, d = to_grid(xf, o, d)
    has_t = keys != np.uint64(0xFFFFFFFFFFFFFFFF)
    t = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    geom = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    with np.errstate(all="ignore"):
        t0 = np.fmax(tmin, g.min_range)
        t1 = np.fmin(tmax, g.max_range)
        carve = walkable & np.where(has_t, t >= g.min_range, bool(g.flags & CARVE_MISSES))
        marks = walkable & has_t & (t >= g.min_range) & (t <= g.max_range)
        t1 = np.where(marks, t, t1).astype(np.float32)
        prod = t[:, None] * d
        p = prod if (own and xf is None) else o + prod     # an own ray without a transform: t d with no sum
    assert p.dtype == np.float32 and t0.dtype == np.float32
    cell, inside = cell_of(g, p)
    occ = np.where(marks & inside, cell, -1)
    return SimpleNamespace(o=o, d=d, t0=t0, t1=t1, carve=carve, occ=occ, geom=geom)


def occupancy(g, rays, records, geoms, own=False, xf=None, into=None):
    """-> (counts uint32[nz, ny, nx, 2], geom uint32[nz, ny, nx], visited int64 (n_rays, trips)): rays (n, 8) float32 (own_rays(dirs)
    with own=True for the handle's), records (k, 4) uint32, geoms {geomID: element count}; into: a pair to accumulate on"""
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    nx, ny, nz = g.dims
    keys = closest_records(records, geoms, r.shape[0], None if own else r)
    st = rays_of(g, r, keys, own, xf)
    visited = walk(g, st.o, st.d, st.t0, st.t1, st.carve)
    counts = np.zeros((nx * ny * nz, 2), np.uint32) if into is None else np.array(into[0], np.uint32).reshape(-1, 2)
    geom = np.full(nx * ny * nz, INV, np.uint32) if into is None else np.array(into[1], np.uint32).reshape(-1)
    free = (visited >= 0) & (visited != st.occ[:, None])
    counts[:, 0] += np.bincount(visited[free], minlength=nx * ny * nz).astype(np.uint32)
    hit = st.occ >= 0
    counts[:, 1] += np.bincount(st.occ[hit], minlength=nx * ny * nz).astype(np.uint32)
    np.minimum.at(geom, st.occ[hit], st.geom[hit])
    return counts.reshape(nz, ny, nx, 2), geom.reshape(nz, ny, nx), visited


def one_ray(g, ray8, t_end, xf=None):
    """what ls_debug_voxel_walk returns for one ray: (the visited cells uint32[k], the occupied cell or INV); t_end NaN: no record"""
    r = np.ascontiguousarray(ray8, np.float32).reshape(1, 8)
    tb = np.uint64(np.float32(t_end).view(np.uint32))
    keys = np.array([0xFFFFFFFFFFFFFFFF if np.isnan(t_end) else (int(tb) << 32)], np.uint64)
    st = rays_of(g, r, keys, False, xf)
    v = walk(g, st.o, st.d, st.t0, st.t1, st.carve)[0]
    return v[v >= 0].astype(np.uint32), np.uint32(INV if st.occ[0] < 0 else st.occ[0])
