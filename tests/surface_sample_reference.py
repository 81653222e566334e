"""The numpy reference of ls_sample_surface (include/lidarshooter_hip.h): the definition of csrc/ls_surface_sample.h restated -- every
float operation one numpy operation on float32, so every operation rounds once; the weights, their prefix and the pick in uint64;
Philox4x32-10 and the 64 x 64 -> high 64 product through 32-bit halves held in uint64.

Per triangle, q_k its vertices in the output frame: a non-finite coordinate gives weight 0; N = (q1 - q0) x (q2 - q0) as products and
differences, m = max |N_k| (weight 0 unless m > 0 and finite), g = N / m, len = sqrt((gx gx + gy gy) + gz gz), n = g / len, a = (0.5 m)
len (weight 0 unless finite); A = max a, e = ilogb(A) - 30 (A == 0: e = 0), w = floor(ldexp(a, -e)); P the exclusive prefix, W its
last entry.  Sample j: x = Philox(key (seed, 1), counter (lo32 j, hi32 j, 0, 0)); T = hi64(((x0 << 32) | x1) W); the triangle is the
largest i with P[i] <= T; alpha = x2 >> 8, beta = x3 >> 8, folded when alpha + beta > 2^24; p = ((w q0 + u q1) + v q2)."""
import numpy as np

INV = 0xFFFFFFFF
F = np.float32
U64 = np.uint64
M32 = U64(0xFFFFFFFF)
DTYPE = np.dtype([("p", "<f4", 3), ("geom", "<u4"), ("n", "<f4", 3), ("prim", "<u4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4"), ("flags", "<u4")])
INFO_DTYPE = np.dtype([("weight_total", "<u8"), ("exponent", "<i4"), ("n_weighted", "<u4")])
assert DTYPE.itemsize == 48 and INFO_DTYPE.itemsize == 16


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays (or scalars) of counters and keys -> four uint32 arrays"""
    c0, c1, c2, c3, k0, k1 = (np.atleast_1d(np.asarray(x, U64)) & M32 for x in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2          # (32 x 32 bits: no overflow in 64)
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> U64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + U64(0x9E3779B9)) & M32, (k1 + U64(0xBB67AE85)) & M32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def mulhi64(a, b):
    """the high 64 bits of the 128-bit products of uint64 arrays"""
    a, b = np.asarray(a, U64), np.asarray(b, U64)
    al, ah, bl, bh = a & M32, a >> U64(32), b & M32, b >> U64(32)
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> U64(32)) + (lh & M32) + (hl & M32)
    return hh + (lh >> U64(32)) + (hl >> U64(32)) + (mid >> U64(32))


def areas(tris):
    """step 2: tris float32 (n, 3, 3) [triangle, vertex, axis] -> (a float32 (n), +0 where the weight is 0; normal float32 (n, 3))"""
    q = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        finite = np.all(np.isfinite(q), axis=(1, 2))
        A, B = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
        N = np.stack([(A[:, 1] * B[:, 2]) - (A[:, 2] * B[:, 1]), (A[:, 2] * B[:, 0]) - (A[:, 0] * B[:, 2]), (A[:, 0] * B[:, 1]) - (A[:, 1] * B[:, 0])],
                     axis=1)
        m = np.fmax(np.fmax(np.abs(N[:, 0]), np.abs(N[:, 1])), np.abs(N[:, 2]))
        ok = finite & (m > 0) & np.isfinite(m)
        g = N / m[:, None]
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        a = (F(0.5) * m) * ln
        ok &= np.isfinite(a)
        n = g / ln[:, None]
    assert a.dtype == np.float32 and n.dtype == np.float32
    return np.where(ok, a, F(0)), np.where(ok[:, None], n, F(0))


def exponent(a):
    """step 3: e from the largest area"""
    top = a.view(np.uint32).max() if a.size else 0
    if top == 0:
        return 0
    _, ex = np.frexp(np.array([top], np.uint32).view(np.float32)[0])     # A = f 2^ex, f in [0.5, 1)
    return int(ex) - 1 - 30


def weights(a, e):
    """step 4"""
    with np.errstate(all="ignore"):
        s = np.ldexp(a, np.int32(-e))
    assert s.dtype == np.float32
    return np.floor(s).astype(U64)


def prefix(w):
    """step 5: P (n + 1)"""
    P = np.zeros(w.shape[0] + 1, U64)
    np.cumsum(w, out=P[1:])
    return P


def table(tris):
    """steps 2 to 5 -> (a, w, P, info)"""
    a, _ = areas(tris)
    e = exponent(a)
    w = weights(a, e)
    P = prefix(w)
    info = np.zeros(1, INFO_DTYPE)
    info["weight_total"], info["exponent"], info["n_weighted"] = P[-1], e, np.count_nonzero(w)
    return a, w, P, info[0]


def words(seed, first, n):
    """step 6 for samples first .. first + n - 1 (mod 2^64)"""
    j = (np.arange(n, dtype=U64) + U64(int(first) & 0xFFFFFFFFFFFFFFFF))
    return philox4x32(j & M32, j >> U64(32), 0, 0, int(seed), 1)


def pick(P, r64):
    """step 7: the largest i < n with P[i] <= T, T = hi64(r64 W); INV where W == 0"""
    r64 = np.atleast_1d(np.asarray(r64, U64))
    if P[-1] == 0:
        return np.full(r64.shape, INV, np.uint32)
    T = mulhi64(r64, P[-1])
    i = np.searchsorted(P, T, side="right") - 1
    assert np.all(i < P.shape[0] - 1) and np.all(P[i] <= T) and np.all(P[i + 1] > T)
    return i.astype(np.uint32)


def bary(x2, x3):
    """step 8 -> (u, v, w) float32"""
    al, be = (np.asarray(x2, np.uint32) >> 8).astype(np.int64), (np.asarray(x3, np.uint32) >> 8).astype(np.int64)
    fold = al + be > (1 << 24)
    al, be = np.where(fold, (1 << 24) - al, al), np.where(fold, (1 << 24) - be, be)
    ga = (1 << 24) - al - be
    s = F(2.0 ** -24)
    return al.astype(np.float32) * s, be.astype(np.float32) * s, ga.astype(np.float32) * s


def point(q, u, v, w):
    """step 9: q float32 (m, 3, 3) -> p float32 (m, 3)"""
    with np.errstate(all="ignore"):
        p = ((w[:, None] * q[:, 0] + u[:, None] * q[:, 1]) + v[:, None] * q[:, 2])
    assert p.dtype == np.float32
    return p


def samples(tris, geom, prim, tri, seed, first, n):
    """the records of samples first .. first + n - 1 over the triangles (in the output frame, in the flat index's order), with their
    geomID, prim and triangle-in-geometry words -> (records DTYPE (n), info)"""
    q = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    _, _, P, info = table(q)
    out = np.zeros(n, DTYPE)
    out["geom"] = INV
    if P[-1] == 0 or n == 0:
        return out, info
    x0, x1, x2, x3 = words(seed, first, n)
    i = pick(P, (x0.astype(U64) << U64(32)) | x1.astype(U64))
    u, v, w = bary(x2, x3)
    _, nrm = areas(q[i])
    out["p"], out["n"], out["u"], out["v"] = point(q[i], u, v, w), nrm, u, v
    out["geom"], out["prim"], out["tri"] = np.asarray(geom, np.uint32)[i], np.asarray(prim, np.uint32)[i], np.asarray(tri, np.uint32)[i]
    out["flags"] = 1
    return out, info


def scene_triangles(oracle, ml, sensor, xf=None, select=None):
    """the selected triangles of a mesh list [(geomID, verts, elems, affine)] as the call sees them, in the flat index's order
    (ascending geomID; an unselected geometry's triangles have weight 0 and move no pick, so they are left out): vertices through
    the frame's transform (the oracle's, bit-equal to the device's) and sensor_to_out, a quad as its triangles 2q, 2q + 1
    -> (tris float32 (n, 3, 3), geom, prim, tri uint32 (n))"""
    from scene_grid_reference import to_grid
    T, G, Pr, Tr = [np.zeros((0, 3, 3), np.float32)], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    for m in sorted(ml, key=lambda m: int(m[0])):
        gid, verts, elems, A = int(m[0]), np.asarray(m[1]), np.asarray(m[2]), m[3]
        if select is not None and gid < len(select) and not select[gid]:
            continue
        v = oracle.transform_vertices(np.ascontiguousarray(verts, np.float32), A, sensor)
        if xf is not None:
            v = to_grid(xf, v)
        quad = elems.shape[1] == 4
        idx = oracle.quads_to_triangles(elems) if quad else elems
        k = np.arange(idx.shape[0], dtype=np.uint32)
        T.append(v[np.asarray(idx, np.int64)])
        G.append(np.full(idx.shape[0], gid, np.uint32))
        Pr.append(k >> 1 if quad else k)
        Tr.append(k)
    return np.concatenate(T), np.concatenate(G), np.concatenate(Pr), np.concatenate(Tr)


def scene_samples(oracle, ml, sensor, xf, select, desc):
    """what ls_sample_surface gives for the mesh list: desc has first_sample, n_samples and seed -> (records, info)"""
    T, G, Pr, Tr = scene_triangles(oracle, ml, sensor, xf, select)
    return samples(T, G, Pr, Tr, int(desc.seed), int(desc.first_sample), int(desc.n_samples))
