"""ls_closest_points / ls_closest_points_host without a device: the symbols, the record layouts, the argument checks that
come before any device call, and the library's point-triangle arithmetic (ls_debug_closest_on_triangle, the host compilation
of what k_closest_points runs per triangle) against an independent float64 derivation."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT


def _header(name="lidarshooter_hip.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_closest_point_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in ("ls_closest_points", "ls_closest_points_host"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s
    assert "ls_debug_closest_on_triangle" in capi.DEBUG_SYMBOLS and hasattr(lib, "ls_debug_closest_on_triangle")
    hdr = _header()
    assert re.search(r"int ls_closest_points\(ls_tracer \*tr, void \*hip_stream, const void \*d_points, uint32_t n, void \*d_out\);", hdr)
    assert re.search(r"int ls_closest_points_host\(ls_tracer \*tr, const void \*points, uint32_t n, void \*out\);", hdr)
    dbg = _header("lidarshooter_hip_debug.h")
    assert re.search(r"int ls_debug_closest_on_triangle\(const float p\[3\], const float v0\[3\], const float v1\[3\], const float v2\[3\], "
                     r"float q\[3\], float \*d2\);", dbg)


def test_record_layouts(capi):
    assert capi.POINT_QUERY_DTYPE.itemsize == 16
    assert [capi.POINT_QUERY_DTYPE.fields[k][1] for k in ("point", "radius")] == [0, 12]
    assert capi.CLOSEST_DTYPE.itemsize == 32
    assert [capi.CLOSEST_DTYPE.fields[k][1] for k in ("q", "dist", "geom", "prim", "index", "pad")] == [0, 12, 16, 20, 24, 28]
    p = np.zeros(2, capi.POINT_QUERY_DTYPE)
    p["point"] = [[1, 2, 3]] * 2
    p["radius"] = 4
    assert np.array_equal(p.view(np.float32).reshape(2, 4), np.tile(np.float32([1, 2, 3, 4]), (2, 1)))


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    buf = (ctypes.c_uint8 * 64)(*([0xAB] * 64))
    INVALID_ARGUMENT = -2
    assert L.ls_closest_points(None, None, buf, 1, buf) == INVALID_ARGUMENT
    assert L.ls_closest_points(None, None, None, 0, None) == INVALID_ARGUMENT
    assert L.ls_closest_points_host(None, buf, 1, buf) == INVALID_ARGUMENT
    assert L.ls_closest_points_host(None, None, 0, None) == INVALID_ARGUMENT
    assert bytes(buf) == b"\xab" * 64   # nothing written


def test_abi_version_unchanged(capi):
    assert capi.load().ls_abi_version() == 4


# ---- the arithmetic ---------------------------------------------------------------------------------------------------

def _closest64(p, a, b, c):
    """float64, not Ericson's form: the projection onto the plane where it falls inside the triangle, else the nearest of the
    three clamped segment projections.  -> (q, dist, region) with region in A B C AB AC BC F"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    n = np.cross(b - a, c - a)
    cands = []
    nn = n @ n
    if nn > 0:
        proj = p - n * ((p - a) @ n) / nn
        # inside test by the three signed areas
        s0 = np.cross(b - a, proj - a) @ n
        s1 = np.cross(c - b, proj - b) @ n
        s2 = np.cross(a - c, proj - c) @ n
        if s0 >= 0 and s1 >= 0 and s2 >= 0:
            cands.append((np.linalg.norm(p - proj), proj, "F"))
    for (u, v, nu, nv) in ((a, b, "A", "B"), (a, c, "A", "C"), (b, c, "B", "C")):
        e = v - u
        t = np.clip(((p - u) @ e) / (e @ e), 0.0, 1.0)
        qq = u + t * e
        name = nu if t == 0.0 else nv if t == 1.0 else nu + nv
        cands.append((np.linalg.norm(p - qq), qq, name))
    d, qq, name = min(cands, key=lambda x: x[0])
    if name != "F" and cands[0][2] == "F" and cands[0][0] <= d:
        d, qq, name = cands[0]
    return qq, d, name


def _min_angle_deg(a, b, c):
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    out = 180.0
    for (u, v, w) in ((a, b, c), (b, c, a), (c, a, b)):
        e, f = v - u, w - u
        out = min(out, np.degrees(np.arccos(np.clip((e @ f) / (np.linalg.norm(e) * np.linalg.norm(f)), -1, 1))))
    return out


def _check(capi, p, a, b, c):
    """2e-6 * S on dist and q (S = the largest |coordinate| among p and the corners): a numpy float32 restatement of the
    operation sequence deviated from float64 by at most 2.6e-7 * S (4.4 float32 ulps of S) over 2 x 2 000 000 random cases at
    S = 1 and S = 100 with edges 0.01 - 1 x S and points up to 4 edge lengths away, all with smallest angle >= 20 degrees;
    2e-6 keeps a factor of 7.7 over that."""
    p, a, b, c = (np.asarray(x, np.float32) for x in (p, a, b, c))
    q, d2 = capi.closest_on_triangle(p, a, b, c)
    q64, d64, region = _closest64(p, a, b, c)
    S = float(max(np.abs(x).max() for x in (p, a, b, c)))
    assert np.isfinite(d2) and d2 >= 0
    dist = float(np.sqrt(np.float32(d2)))
    assert abs(dist - d64) <= 2e-6 * S, (p, a, b, c, dist, d64, region)
    assert np.abs(q.astype(np.float64) - q64).max() <= 2e-6 * S, (p, a, b, c, q, q64, region)
    return region, d2


def test_closest_on_triangle_against_float64(capi):
    rng = np.random.default_rng(2024)
    seen = {}
    n_checked = 0
    for S in (1.0, 100.0):
        for _ in range(4000):
            center = rng.uniform(-0.5, 0.5, 3) * S
            L = S * 10 ** rng.uniform(-2, -0.3)
            a, b, c = (center + rng.uniform(-0.5, 0.5, 3) * L for _ in range(3))
            if _min_angle_deg(np.float32(a), np.float32(b), np.float32(c)) < 20.0:
                continue
            # points around the triangle, up to 4 edge lengths away, biased to lie over every region
            w = rng.uniform(-1.0, 2.0, 3)
            w /= w.sum() if abs(w.sum()) > 0.2 else 1.0
            nrm = np.cross(b - a, c - a)
            nrm /= np.linalg.norm(nrm)
            p = w[0] * a + w[1] * b + w[2] * c + nrm * rng.uniform(-4, 4) * L * rng.integers(0, 2)
            if np.abs(p).max() > S:
                continue
            region, _ = _check(capi, p, a, b, c)
            seen[region] = seen.get(region, 0) + 1
            n_checked += 1
    assert n_checked > 3000
    assert set(seen) == {"A", "B", "C", "AB", "AC", "BC", "F"}, seen
    assert min(seen.values()) >= 50, seen


def test_points_on_the_triangle_have_distance_zero(capi):
    rng = np.random.default_rng(7)
    for S in (1.0, 100.0):
        for _ in range(300):
            a, b, c = (np.float32(rng.uniform(-1, 1, 3) * S) for _ in range(3))
            if _min_angle_deg(a, b, c) < 20.0:
                continue
            # exactly on a vertex
            for v in (a, b, c):
                q, d2 = capi.closest_on_triangle(v, a, b, c)
                assert d2 == 0.0 and np.array_equal(q, v)
            # exactly on an edge, exactly on the face: a triangle in the plane z = const with corners on a dyadic grid, so that
            # midpoints and centroid-like points are exact float32 values of the plane and the segments
            g = np.float32(S / 64)
            ia = rng.integers(-20, 20, 2)
            ib = ia + np.array([rng.integers(4, 12) * 2, rng.integers(0, 4) * 2])
            ic = ia + np.array([rng.integers(0, 4) * 2, rng.integers(4, 12) * 2])
            z = np.float32(rng.integers(-8, 8)) * g
            fa, fb, fc = (np.float32([i[0] * g, i[1] * g, z]) for i in (ia, ib, ic))
            if _min_angle_deg(fa, fb, fc) < 20.0:
                continue
            for (u, v) in ((fa, fb), (fa, fc), (fb, fc)):
                m = np.float32((u.astype(np.float64) + v.astype(np.float64)) / 2)
                assert np.array_equal(m.astype(np.float64), (u.astype(np.float64) + v.astype(np.float64)) / 2)
                region, d2 = _check(capi, m, fa, fb, fc)
                assert d2 == 0.0, (u, v, m, d2)
            # on the face: the reciprocal of the face region rounds unless the doubled area squared is a power of two -- a right
            # triangle with power-of-two legs, the point at dyadic barycentric coordinates
            k1, k2 = rng.integers(1, 5, 2)
            ax = rng.permutation(3)
            ra = np.zeros(3)
            ra[ax[0]], ra[ax[1]], ra[ax[2]] = ia[0] * float(g), ia[1] * float(g), float(z)
            rb, rc = ra.copy(), ra.copy()
            rb[ax[0]] += float(g) * 2 ** k1
            rc[ax[1]] += float(g) * 2 ** k2
            ra, rb, rc = np.float32(ra), np.float32(rb), np.float32(rc)
            inner = np.float32((2 * ra.astype(np.float64) + rb.astype(np.float64) + rc.astype(np.float64)) / 4)
            region, d2 = _check(capi, inner, ra, rb, rc)
            assert region == "F" and d2 == 0.0


def test_needles_and_degenerate_triangles(capi):
    """A needle's answer is not held to 2e-6 * S, but it is either skipped (d2 not finite) or the distance of a point of the
    triangle: never nearer than the true distance by more than the rounding of the coordinates (what the hierarchy walk's
    pruning relies on; 4e-6 * S = half of the margin the walk keeps for it)."""
    rng = np.random.default_rng(99)
    finite = 0
    for _ in range(6000):
        S = 10 ** rng.uniform(-1, 3)
        a = rng.uniform(-1, 1, 3) * S
        e = rng.normal(size=3)
        e *= S * 10 ** rng.uniform(-3, 0) / np.linalg.norm(e)
        b = a + e
        c = a + e * rng.uniform(-0.5, 1.5) + rng.normal(size=3) * np.linalg.norm(e) * 10 ** rng.uniform(-9, -2)
        p = a + rng.normal(size=3) * np.linalg.norm(e) * 10 ** rng.uniform(-3, 1)
        a, b, c, p = (np.float32(x) for x in (a, b, c, p))
        q, d2 = capi.closest_on_triangle(p, a, b, c)
        if not np.isfinite(d2):
            continue
        finite += 1
        _, d64, _ = _closest64(p, a, b, c)
        Sc = float(max(np.abs(x).max() for x in (p, a, b, c)))
        assert float(np.sqrt(np.float32(d2))) >= d64 - 4e-6 * Sc, (p, a, b, c, d2, d64)
    assert finite > 3000
    # no area, or a corner that is not a number: skipped, whatever the point
    z = np.float32([1, 2, 3])
    for tri in ((z, z, z), (z, z + 1, z + 2), (z, np.float32([np.nan, 0, 0]), z + 1), (z, np.float32([np.inf, 0, 0]), z + 1),
                (np.float32([0, 0, 0]), np.float32([1e-30, 0, 0]), np.float32([0, 1e-30, 0]))):
        q, d2 = capi.closest_on_triangle(np.float32([0.5, 0.1, -2]), *tri)
        assert not np.isfinite(d2) and np.array_equal(q, np.zeros(3, np.float32))
