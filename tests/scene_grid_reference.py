"""The numpy reference of ls_scene_grid (include/lidarshooter_hip.h): the definition of csrc/ls_scene_grid.h restated over float32
arrays -- every operation one numpy operation on float32, so every operation rounds once -- and vectorised over the (triangle, cell)
pairs of the triangles' clamped ranges.

Per triangle, v_k its vertices in the grid's frame: q_k = v_k - origin (a non-finite q: skipped); per axis lo = floor(min q / cell),
hi = floor(max q / cell) as floats (hi < 0 or lo >= n: skipped), clamped to [0, n - 1]; per cell c of the range ctr = (c + 0.5) cell,
h = 0.5 cell, p_k = q_k - ctr, the edges e0 = q1 - q0, e1 = q2 - q1, e2 = q0 - q2; the cell overlaps unless one of 13 axes separates:
the 3 box axes (every p_k[a] > h, or every one < -h), the 9 axes unit_i x e_j (i = x: (e_y p_k.z) - (e_z p_k.y) against r = h (|e_z| +
|e_y|), cyclically; every projection > r, or every one < -r) and the plane (n = cross(e0, e1), d = ((n.x p_0.x) + (n.y p_0.y)) + (n.z
p_0.z) against r = h ((|n.x| + |n.y|) + |n.z|): d > r or d < -r).  No comparison with a NaN separates."""
from types import SimpleNamespace

import numpy as np

INV = 0xFFFFFFFF
ACCUMULATE = 1
F = np.float32
CHUNK = 1 << 21          # (triangle, cell) pairs tested at once


def grid(origin, cell, dims, flags=0):
    """the descriptor's fields as the reference reads them (a capi.SceneGridDesc has the same names)"""
    return SimpleNamespace(origin=[F(x) for x in origin], cell=F(cell), dims=[int(x) for x in dims], flags=int(flags))


def to_grid(m, v):
    """sensor-frame vertices (n, 3) through sensor_to_grid: ((m0 x + m1 y) + m2 z) + m3 per row"""
    m = np.ascontiguousarray(m, np.float32).reshape(3, 4)
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        out = np.stack([((m[i, 0] * v[:, 0] + m[i, 1] * v[:, 1]) + m[i, 2] * v[:, 2]) + m[i, 3] for i in range(3)], axis=1)
    assert out.dtype == np.float32
    return out


def ranges(g, tris):
    """-> (q float32 (n, 3, 3) [triangle, vertex, axis], ok bool (n), lo int64 (n, 3), hi int64 (n, 3)): steps 1 to 3"""
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        q = np.stack([t[:, :, a] - g.origin[a] for a in range(3)], axis=2)
        assert q.dtype == np.float32
        ok = np.all(np.isfinite(q), axis=(1, 2))
        qq = np.where(ok[:, None, None], q, F(0))
        lo = np.stack([np.floor(qq[:, :, a].min(axis=1) / g.cell) for a in range(3)], axis=1)
        hi = np.stack([np.floor(qq[:, :, a].max(axis=1) / g.cell) for a in range(3)], axis=1)
        assert lo.dtype == np.float32 and hi.dtype == np.float32
        n = np.float32(g.dims)[None, :]
        ok &= ~np.any((hi < 0) | (lo >= n), axis=1)
        lo = np.fmin(np.fmax(lo, F(0)), n - F(1))
        hi = np.fmin(np.fmax(hi, F(0)), n - F(1))
    lo = np.where(ok[:, None], lo, 0).astype(np.int64)
    hi = np.where(ok[:, None], hi, -1).astype(np.int64)
    return q, ok, lo, hi


def _separates(a, b, c, r):
    m = -r
    return ((a > r) & (b > r) & (c > r)) | ((a < m) & (b < m) & (c < m))


def overlaps(g, q, c):
    """steps 4 and 5 for pairs: q float32 (m, 3, 3), c int64 (m, 3) -> bool (m)"""
    cell = g.cell
    h = F(0.5) * cell
    with np.errstate(all="ignore"):
        ctr = (c.astype(np.float32) + F(0.5)) * cell
        p = q - ctr[:, None, :]
        assert p.dtype == np.float32
        sep = np.zeros(q.shape[0], bool)
        for a in range(3):
            sep |= _separates(p[:, 0, a], p[:, 1, a], p[:, 2, a], h)
        e = [q[:, 1] - q[:, 0], q[:, 2] - q[:, 1], q[:, 0] - q[:, 2]]
        X, Y, Z = 0, 1, 2
        for ej in e:
            ex, ey, ez = ej[:, X], ej[:, Y], ej[:, Z]
            sep |= _separates(*[(ey * p[:, k, Z]) - (ez * p[:, k, Y]) for k in range(3)], h * (np.abs(ez) + np.abs(ey)))
            sep |= _separates(*[(ez * p[:, k, X]) - (ex * p[:, k, Z]) for k in range(3)], h * (np.abs(ex) + np.abs(ez)))
            sep |= _separates(*[(ex * p[:, k, Y]) - (ey * p[:, k, X]) for k in range(3)], h * (np.abs(ey) + np.abs(ex)))
        e0, e1 = e[0], e[1]
        nx = (e0[:, Y] * e1[:, Z]) - (e0[:, Z] * e1[:, Y])
        ny = (e0[:, Z] * e1[:, X]) - (e0[:, X] * e1[:, Z])
        nz = (e0[:, X] * e1[:, Y]) - (e0[:, Y] * e1[:, X])
        d = ((nx * p[:, 0, X]) + (ny * p[:, 0, Y])) + (nz * p[:, 0, Z])
        r = h * ((np.abs(nx) + np.abs(ny)) + np.abs(nz))
        assert d.dtype == np.float32 and r.dtype == np.float32
        sep |= (d > r) | (d < -r)
    return ~sep


def pairs(g, tris):
    """every (triangle, cell) pair of the clamped ranges, in chunks -> yields (tri int64 (m), c int64 (m, 3), q float32 (m, 3, 3))"""
    q, ok, lo, hi = ranges(g, tris)
    w = hi - lo + 1                                     # (0 along x for a skipped triangle)
    w[~ok] = 0
    cnt = w[:, 0] * w[:, 1] * w[:, 2]
    order = np.nonzero(cnt)[0]
    at = 0
    while at < order.shape[0]:
        end, total = at, 0
        while end < order.shape[0] and (total == 0 or total + cnt[order[end]] <= CHUNK):
            total += cnt[order[end]]
            end += 1
        sel = order[at:end]
        tri = np.repeat(sel, cnt[sel])
        k = np.arange(total) - np.repeat(np.cumsum(cnt[sel]) - cnt[sel], cnt[sel])
        wx, wy = w[tri, 0], w[tri, 1]
        c = np.stack([lo[tri, 0] + k % wx, lo[tri, 1] + (k // wx) % wy, lo[tri, 2] + k // (wx * wy)], axis=1)
        yield tri, c, q[tri]
        at = end


def marked(g, tris):
    """-> (tri int64 (m), cell int64 (m), tested): the overlapping (triangle, cell word index) pairs and the number of pairs tested"""
    nx, ny, _ = g.dims
    T, C, tested = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0
    for tri, c, q in pairs(g, tris):
        hit = overlaps(g, q, c)
        tested += tri.shape[0]
        T.append(tri[hit])
        C.append((c[hit, 2] * ny + c[hit, 1]) * nx + c[hit, 0])
    return np.concatenate(T), np.concatenate(C), tested


def triangle_cells(g, tri9):
    """what ls_debug_scene_grid_triangle returns for one triangle: the overlapping cells, ascending"""
    return np.sort(marked(g, np.ascontiguousarray(tri9, np.float32).reshape(1, 3, 3))[1]).astype(np.uint32)


def scene_grid(g, tris, geom_ids, into=None):
    """-> (counts uint32[nz, ny, nx], geom uint32[nz, ny, nx]): tris float32 (n, 3, 3) in the grid's frame, geom_ids (n); into: a pair
    to accumulate on"""
    nx, ny, nz = g.dims
    cells = nx * ny * nz
    counts = np.zeros(cells, np.uint32) if into is None else np.array(into[0], np.uint32).reshape(-1)
    geom = np.full(cells, INV, np.uint32) if into is None else np.array(into[1], np.uint32).reshape(-1)
    tri, cell, _ = marked(g, tris)
    counts += np.bincount(cell, minlength=cells).astype(np.uint32)
    np.minimum.at(geom, cell, np.asarray(geom_ids, np.uint32)[tri])
    return counts.reshape(nz, ny, nx), geom.reshape(nz, ny, nx)


def scene_triangles(oracle, ml, sensor, xf=None, select=None):
    """the triangles of a mesh list [(geomID, verts, elems, affine)] as the call sees them: vertices through the frame's transform
    (the oracle's, bit-equal to the device's) and sensor_to_grid, a quad as its two triangles; select: bytes by geomID or None
    -> (tris float32 (n, 3, 3), geom uint32 (n))"""
    T, G = [np.zeros((0, 3, 3), np.float32)], [np.zeros(0, np.uint32)]
    for m in ml:
        gid, verts, elems, A = int(m[0]), np.asarray(m[1]), np.asarray(m[2]), m[3]
        if select is not None and gid < len(select) and not select[gid]:
            continue
        v = oracle.transform_vertices(np.ascontiguousarray(verts, np.float32), A, sensor)
        if xf is not None:
            v = to_grid(xf, v)
        idx = oracle.quads_to_triangles(elems) if elems.shape[1] == 4 else elems
        T.append(v[np.asarray(idx, np.int64)])
        G.append(np.full(idx.shape[0], gid, np.uint32))
    return np.concatenate(T), np.concatenate(G)
