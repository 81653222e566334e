"""The definition of ls_cloud_nearest (include/lidarshooter_hip.h; csrc/ls_cloud_nearest.h) in numpy, twice:

  brute()  the definition as it stands: every query against every cloud point, in chunks, the minimum of the 64-bit key
           (bits(d2) << 32) | i over the candidates.  About 2^25 pairs a second: for inputs up to 2^26 pairs;
  grid()   for larger inputs: the cloud sorted by cell, and per query `searchsorted` over the 3 x 3 x 3 cells around its own, in the
           same float32 arithmetic.  tests/test_cloud_nearest_cpu.py holds it to brute() byte for byte.

Everything float is float32 and every numpy operation rounds once; numpy fuses nothing.  Neither path uses the library."""
import numpy as np

F = np.float32
U32 = np.uint32
U64 = np.uint64
INV = 0xFFFFFFFF
SKIP_SAME_INDEX = 1
DTYPE = np.dtype([("index", "<u4"), ("dist2", "<f4"), ("dist", "<f4"), ("flags", "<u4")])
INFO_DTYPE = np.dtype([("n_found", "<u4"), ("n_query_outside", "<u4"), ("n_cloud_indexed", "<u4"), ("reserved", "<u4")])
NONE = U64(0xFFFFFFFFFFFFFFFF)             # no candidate yet: above every key (a key's high word is at most bits(r2))
RADIUS_MIN, RADIUS_MAX = F(2.0 ** -20), F(2.0 ** 20)


def constants(radius):
    """step 1 and the cell edge -> (D, r2, h) as float32"""
    r = F(radius)
    return r * F(65536.0), r * r, r * F(1.015625)


def transform(q, xf):
    """step 2's transform of the queries (m, 3): ((m0 x + m1 y) + m2 z) + m3 per row"""
    q = np.ascontiguousarray(q, F).reshape(-1, 3)
    if xf is None:
        return q
    m = np.ascontiguousarray(xf, F).reshape(3, 4)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=1).astype(F)


def takes_part(D, p):
    """step 2: finite and |c| <= D per coordinate (NaN and +-inf fail the comparison)"""
    with np.errstate(invalid="ignore"):
        return np.all(np.abs(p) <= D, axis=1)


def cells(h, p):
    """the cell of points that take part: floorf(c / h) per axis -> int64 (n, 3)"""
    return np.floor(p / h).astype(np.int64)


def _keys(r2, q, p, idx, own):
    """steps 4 and 5 for the pairs of q and p (xyz along the last axis; the shapes broadcast), idx the cloud indices, own the queries' own
    indices or None -> uint64 keys, NONE for a pair that is no candidate"""
    dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    ok = d2 <= r2
    if own is not None:
        ok &= idx != own
    key = (d2.view(U32).astype(U64) << U64(32)) | idx.astype(U64)
    return np.where(ok, key, NONE)


def _records(best, outside, n_indexed):
    m = best.shape[0]
    out = np.zeros(m, DTYPE)
    found = best != NONE
    out["index"] = np.where(found, (best & U64(INV)).astype(U32), U32(INV))
    d2 = np.where(found, (best >> U64(32)).astype(U32), U32(0x7F800000)).view(F)
    out["dist2"] = d2
    out["dist"] = np.sqrt(d2)
    out["flags"] = np.where(outside, U32(2), found.astype(U32))
    assert not np.any(found & outside)
    info = np.zeros(1, INFO_DTYPE)
    info["n_found"], info["n_query_outside"], info["n_cloud_indexed"] = np.count_nonzero(found), np.count_nonzero(outside), n_indexed
    return out, info[0]


def _prepare(cloud, queries, radius, xf):
    D, r2, h = constants(radius)
    cloud = np.ascontiguousarray(cloud, F).reshape(-1, 3)
    q = transform(queries, xf)
    part = np.nonzero(takes_part(D, cloud))[0]
    return D, r2, h, cloud[part], part.astype(U32), q, ~takes_part(D, q)


def brute(cloud, queries, radius, flags=0, xf=None, pairs_per_chunk=1 << 22):
    """the definition: cloud (n, 3), queries (m, 3) float32 -> (records DTYPE[m], info INFO_DTYPE[()])"""
    D, r2, h, p, idx, q, outside = _prepare(cloud, queries, radius, xf)
    m, n = q.shape[0], p.shape[0]
    best = np.full(m, NONE, U64)
    inside = np.nonzero(~outside)[0]
    step = max(1, pairs_per_chunk // max(n, 1))
    for a in range(0, inside.shape[0] if n else 0, step):
        k = inside[a:a + step]
        own = k.astype(U32)[:, None] if flags & SKIP_SAME_INDEX else None
        best[k] = _keys(r2, q[k][:, None, :], p[None, :, :], idx[None, :], own).min(axis=1)
    return _records(best, outside, n)


def grid(cloud, queries, radius, flags=0, xf=None, pairs_per_chunk=1 << 22):
    """the same records through a cell grid: the cloud sorted by a linear cell number, per query the ranges of the 27 cells around its
    own (searchsorted), every point of them tested as brute() tests it"""
    D, r2, h, p, idx, q, outside = _prepare(cloud, queries, radius, xf)
    m, n = q.shape[0], p.shape[0]
    best = np.full(m, NONE, U64)
    inside = np.nonzero(~outside)[0]
    if n and inside.shape[0]:
        S = np.int64(1 << 18)                                         # a cell lies in -65536 .. 65536: + 65537 (a neighbour's too) fits 18 bits
        lin = lambda c: ((c[:, 2] + 65537) * S + (c[:, 1] + 65537)) * S + (c[:, 0] + 65537)
        pk = lin(cells(h, p))
        order = np.argsort(pk, kind="stable")
        pk, ps, pidx = pk[order], p[order], idx[order]
        qc = cells(h, q[inside])
        for oz in (-1, 0, 1):
            for oy in (-1, 0, 1):
                for ox in (-1, 0, 1):
                    key = lin(qc + np.int64([ox, oy, oz]))
                    lo, hi = np.searchsorted(pk, key, "left"), np.searchsorted(pk, key, "right")
                    has = np.nonzero(hi > lo)[0]
                    cnt = (hi - lo)[has]
                    cum = np.cumsum(cnt)
                    a = 0
                    while a < has.shape[0]:   # chunks of queries whose ranges add up to about pairs_per_chunk pairs
                        done = int(cum[a - 1]) if a else 0
                        b = max(a + 1, int(np.searchsorted(cum, done + pairs_per_chunk, "right")))
                        c, k = cnt[a:b], inside[has[a:b]]
                        start = np.cumsum(c) - c
                        which = np.repeat(np.arange(b - a), c)
                        j = lo[has[a:b]][which] + (np.arange(int(c.sum())) - start[which])
                        own = k[which].astype(U32) if flags & SKIP_SAME_INDEX else None
                        keys = _keys(r2, q[k][which], ps[j], pidx[j], own)
                        best[k] = np.minimum(best[k], np.minimum.reduceat(keys, start))
                        a = b
    return _records(best, outside, n)


def strided(points, stride, fill=0xAB):
    """points (n, 3) float32 as n records of `stride` bytes: x, y, z at bytes 0, 4, 8 and `fill` in every other byte -> uint8 (n, stride)"""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    out = np.full((p.shape[0], int(stride)), fill, np.uint8)
    out[:, :12] = p.view(np.uint8).reshape(-1, 12)
    return out
