"""The numpy reference of ls_scene_distance_grid (include/lidarshooter_hip.h): the definition of csrc/ls_distance_grid.h restated over
float32 arrays -- every operation one numpy operation on float32, so every operation rounds once -- and vectorised over the
(triangle, cell) pairs of the triangles' widened, clamped ranges.

Per triangle, v_k its vertices in the grid's frame: q_k = v_k - origin (a non-finite q: skipped); per axis lo = floor((min q - trunc) /
cell), hi = floor((max q + trunc) / cell) as floats (hi < 0 or lo >= n: skipped), clamped to [0, n - 1]; per cell c of the range ctr =
(c + 0.5) cell and closest_on_triangle(ctr, q_0, q_1, q_2) -- csrc/ls_closest.h restated below: Ericson's seven regions in the header's
order by np.where, true divisions, the face numerators clamped at 0 -- gives d2; the pair counts iff d2 is finite and dist = sqrt(d2)
<= trunc, and sends (bits(dist) << 32) | geomID to its cell, whose word becomes the 64-bit unsigned minimum."""
from types import SimpleNamespace

import numpy as np

from scene_grid_reference import scene_triangles, to_grid  # noqa: F401  (the scene as ls_scene_grid sees it: the same triangles)

INV = 0xFFFFFFFF
REST = np.uint64(0x7F800000FFFFFFFF)     # {0xFFFFFFFF, +inf}: no surface within trunc
ACCUMULATE = 1
F = np.float32
CHUNK = 1 << 20          # (triangle, cell) pairs tested at once
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "F")


def grid(origin, cell, dims, trunc, flags=0):
    """the descriptor's fields as the reference reads them (a capi.DistanceGridDesc has the same names)"""
    return SimpleNamespace(origin=[F(x) for x in origin], cell=F(cell), dims=[int(x) for x in dims], flags=int(flags), trunc=F(trunc))


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def closest_on_triangle(p, a, b, c):
    """csrc/ls_closest.h for m cases at once: p, a, b, c float32 (m, 3) -> (q float32 (m, 3), d2 float32 (m), region int8 (m): the
    index into REGIONS, -1 for a skipped triangle: q = 0, d2 = +inf)"""
    p, a, b, c = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (p, a, b, c))
    X, Y, Z = 0, 1, 2
    zero = F(0)
    with np.errstate(all="ignore"):
        abx, aby, abz = b[:, X] - a[:, X], b[:, Y] - a[:, Y], b[:, Z] - a[:, Z]
        acx, acy, acz = c[:, X] - a[:, X], c[:, Y] - a[:, Y], c[:, Z] - a[:, Z]
        nx, ny, nz = aby * acz - abz * acy, abz * acx - abx * acz, abx * acy - aby * acx
        nn = _dot(nx, ny, nz, nx, ny, nz)
        live = (nn > zero) & (nn < F(np.inf))
        apx, apy, apz = p[:, X] - a[:, X], p[:, Y] - a[:, Y], p[:, Z] - a[:, Z]
        d1 = _dot(abx, aby, abz, apx, apy, apz)
        d2a = _dot(acx, acy, acz, apx, apy, apz)
        bpx, bpy, bpz = p[:, X] - b[:, X], p[:, Y] - b[:, Y], p[:, Z] - b[:, Z]
        d3 = _dot(abx, aby, abz, bpx, bpy, bpz)
        d4 = _dot(acx, acy, acz, bpx, bpy, bpz)
        cpx, cpy, cpz = p[:, X] - c[:, X], p[:, Y] - c[:, Y], p[:, Z] - c[:, Z]
        d5 = _dot(abx, aby, abz, cpx, cpy, cpz)
        d6 = _dot(acx, acy, acz, cpx, cpy, cpz)
        vc = d1 * d4 - d3 * d2a
        vb = d5 * d2a - d1 * d6
        va = d3 * d6 - d5 * d4
        # the tests of the seven regions, each taken only where none before it was
        tests = [(d1 <= zero) & (d2a <= zero),
                 (d3 >= zero) & (d4 <= d3),
                 (vc <= zero) & (d1 >= zero) & (d3 <= zero),
                 (d6 >= zero) & (d5 <= d6),
                 (vb <= zero) & (d2a >= zero) & (d6 <= zero),
                 (va <= zero) & ((d4 - d3) >= zero) & ((d5 - d6) >= zero)]
        region = np.full(p.shape[0], 6, np.int8)
        for k in range(5, -1, -1):
            region = np.where(tests[k], np.int8(k), region)
        # every region's point (computed everywhere, chosen by region)
        v_ab = d1 / (d1 - d3)
        w_ac = d2a / (d2a - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        fa, fb, fc = np.where(va > zero, va, zero), np.where(vb > zero, vb, zero), np.where(vc > zero, vc, zero)
        denom = F(1) / ((fa + fb) + fc)
        v, w = fb * denom, fc * denom
        cand = [(a[:, X], a[:, Y], a[:, Z]),
                (b[:, X], b[:, Y], b[:, Z]),
                (a[:, X] + abx * v_ab, a[:, Y] + aby * v_ab, a[:, Z] + abz * v_ab),
                (c[:, X], c[:, Y], c[:, Z]),
                (a[:, X] + acx * w_ac, a[:, Y] + acy * w_ac, a[:, Z] + acz * w_ac),
                (b[:, X] + (c[:, X] - b[:, X]) * w_bc, b[:, Y] + (c[:, Y] - b[:, Y]) * w_bc, b[:, Z] + (c[:, Z] - b[:, Z]) * w_bc),
                ((a[:, X] + abx * v) + acx * w, (a[:, Y] + aby * v) + acy * w, (a[:, Z] + abz * v) + acz * w)]
        qx, qy, qz = cand[6]
        for k in range(5, -1, -1):
            at = region == k
            qx, qy, qz = np.where(at, cand[k][0], qx), np.where(at, cand[k][1], qy), np.where(at, cand[k][2], qz)
        dx, dy, dz = p[:, X] - qx, p[:, Y] - qy, p[:, Z] - qz
        d2 = _dot(dx, dy, dz, dx, dy, dz)
        assert d2.dtype == np.float32 and qx.dtype == np.float32 and nn.dtype == np.float32
        q = np.stack([np.where(live, qx, zero), np.where(live, qy, zero), np.where(live, qz, zero)], axis=1)
        d2 = np.where(live, d2, F(np.inf))
        region = np.where(live, region, np.int8(-1))
    return q, d2, region


def ranges(g, tris, all_cells=False):
    """-> (q float32 (n, 3, 3) [triangle, vertex, axis], ok bool (n), lo int64 (n, 3), hi int64 (n, 3)): steps 1 and 2.  all_cells:
    every triangle with a finite q gets the whole grid instead of its range (what the range must not differ from)"""
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        q = np.stack([t[:, :, a] - g.origin[a] for a in range(3)], axis=2)
        assert q.dtype == np.float32
        ok = np.all(np.isfinite(q), axis=(1, 2))
        qq = np.where(ok[:, None, None], q, F(0))
        lo = np.stack([np.floor((qq[:, :, a].min(axis=1) - g.trunc) / g.cell) for a in range(3)], axis=1)
        hi = np.stack([np.floor((qq[:, :, a].max(axis=1) + g.trunc) / g.cell) for a in range(3)], axis=1)
        assert lo.dtype == np.float32 and hi.dtype == np.float32
        n = np.float32(g.dims)[None, :]
        if all_cells:
            lo, hi = np.zeros_like(lo), np.zeros_like(hi) + (n - F(1))
        else:
            ok &= ~np.any((hi < 0) | (lo >= n), axis=1)
            lo = np.fmin(np.fmax(lo, F(0)), n - F(1))
            hi = np.fmin(np.fmax(hi, F(0)), n - F(1))
    lo = np.where(ok[:, None], lo, 0).astype(np.int64)
    hi = np.where(ok[:, None], hi, -1).astype(np.int64)
    return q, ok, lo, hi


def range_cells(g, tris):
    """the number of cells of every triangle's widened, clamped range (0: skipped)"""
    _, ok, lo, hi = ranges(g, tris)
    return np.where(ok, np.prod(hi - lo + 1, axis=1), 0)


def pairs(g, tris, all_cells=False):
    """every (triangle, cell) pair of the ranges, in chunks -> yields (tri int64 (m), c int64 (m, 3), q float32 (m, 3, 3))"""
    q, ok, lo, hi = ranges(g, tris, all_cells)
    w = hi - lo + 1
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


def cell_distance(g, q, c):
    """step 3 for pairs: q float32 (m, 3, 3), c int64 (m, 3) -> (counts bool (m), dist float32 (m))"""
    with np.errstate(all="ignore"):
        ctr = (c.astype(np.float32) + F(0.5)) * g.cell
        assert ctr.dtype == np.float32
        _, d2, _ = closest_on_triangle(ctr, q[:, 0], q[:, 1], q[:, 2])
        dist = np.sqrt(d2)
        assert dist.dtype == np.float32
        return np.isfinite(d2) & (dist <= g.trunc), dist


def counted(g, tris, all_cells=False):
    """-> (tri int64 (m), cell int64 (m), dist float32 (m), tested): the counting (triangle, cell record index) pairs with their
    distances, and the number of pairs tested"""
    nx, ny, _ = g.dims
    T, C, D, tested = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.float32)], 0
    for tri, c, q in pairs(g, tris, all_cells):
        hit, dist = cell_distance(g, q, c)
        tested += tri.shape[0]
        T.append(tri[hit])
        C.append((c[hit, 2] * ny + c[hit, 1]) * nx + c[hit, 0])
        D.append(dist[hit])
    return np.concatenate(T), np.concatenate(C), np.concatenate(D), tested


def triangle_cells(g, tri9):
    """what ls_debug_distance_grid_triangle returns for one triangle: the counting cells, ascending, and their distances"""
    _, cell, dist, _ = counted(g, np.ascontiguousarray(tri9, np.float32).reshape(1, 3, 3))
    order = np.argsort(cell, kind="stable")
    return cell[order].astype(np.uint32), dist[order]


def words(dist, geom):
    """(dist float32, geom uint32) arrays -> the records as 64-bit words (bits(dist) << 32) | geom"""
    return (np.ascontiguousarray(dist, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(geom, np.uint32).astype(np.uint64)


def split(w):
    """64-bit words -> (dist float32, geom uint32), same shape"""
    w = np.ascontiguousarray(w, np.uint64)
    return (w >> np.uint64(32)).astype(np.uint32).view(np.float32), (w & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def distance_grid(g, tris, geom_ids, into=None, all_cells=False):
    """-> uint64[nz, ny, nx], the records as words: tris float32 (n, 3, 3) in the grid's frame, geom_ids (n); into: words to take the
    minimum with (compared as 64-bit words, whatever their bits)"""
    nx, ny, nz = g.dims
    out = np.full(nx * ny * nz, REST, np.uint64) if into is None else np.array(into, np.uint64).reshape(-1)
    tri, cell, dist, _ = counted(g, tris, all_cells)
    np.minimum.at(out, cell, words(dist, np.asarray(geom_ids, np.uint32)[tri]))
    return out.reshape(nz, ny, nx)
