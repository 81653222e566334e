"""ls_hit_attributes / ls_hit_attributes_host without a device: the symbols, the record layout, the argument checks that come
before any device call, and the library's hit-attribute arithmetic (ls_debug_hit_attributes_on_triangle, the host compilation
of what k_hit_attributes runs per record): t against the oracle's test bit for bit, normal / incidence / barycentrics against
an independent float64 derivation, finiteness on tiny and huge triangles."""
import ctypes
import os
import re
import types

import numpy as np

from conftest import ROOT

INVALID_ARGUMENT = -2
EPS = 2.0 ** -24


def _header(name="lidarshooter_hip.h"):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", name)).read())


def test_hit_attribute_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert capi.load().ls_abi_version() == 4      # the new entry points do not step the ABI version
    for s in ("ls_hit_attributes", "ls_hit_attributes_host"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s
    assert "ls_debug_hit_attributes_on_triangle" in capi.DEBUG_SYMBOLS and hasattr(lib, "ls_debug_hit_attributes_on_triangle")
    hdr = _header()
    assert re.search(r"int ls_hit_attributes\(ls_tracer \*tr, void \*hip_stream, const void \*d_rays, uint32_t n_rays, "
                     r"const void \*d_hits, const uint32_t \*d_count, uint32_t n, void \*d_out\);", hdr)
    assert re.search(r"int ls_hit_attributes_host\(ls_tracer \*tr, const void \*rays, uint32_t n_rays, const void \*hits, uint32_t n, "
                     r"void \*out\);", hdr)
    dbg = _header("lidarshooter_hip_debug.h")
    assert re.search(r"int ls_debug_hit_attributes_on_triangle\(const float o\[3\], const float d\[3\], const float v0\[3\], "
                     r"const float v1\[3\], const float v2\[3\], float \*t, float out9\[9\]", dbg)


def test_record_layout(capi):
    dt = capi.HIT_ATTR_DTYPE
    assert dt.itemsize == 48
    assert [dt.fields[k][1] for k in ("n", "cos_inc", "u", "v", "tri", "flags", "p", "ray")] == [0, 12, 16, 20, 24, 28, 32, 44]
    assert dt.fields["n"][0].shape == (3,) and dt.fields["p"][0].shape == (3,)
    assert dt.fields["tri"][0] == np.dtype("<u4") and dt.fields["flags"][0] == np.dtype("<u4") and dt.fields["ray"][0] == np.dtype("<u4")


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    buf = (ctypes.c_uint8 * 64)(*([0xAB] * 64))
    assert L.ls_hit_attributes(None, None, None, 0, buf, None, 1, buf) == INVALID_ARGUMENT
    assert L.ls_hit_attributes(None, None, buf, 1, buf, None, 1, buf) == INVALID_ARGUMENT
    assert L.ls_hit_attributes(None, None, None, 0, None, None, 0, None) == INVALID_ARGUMENT
    assert L.ls_hit_attributes_host(None, None, 0, buf, 1, buf) == INVALID_ARGUMENT
    assert L.ls_hit_attributes_host(None, None, 0, None, 0, None) == INVALID_ARGUMENT
    assert bytes(buf) == b"\xab" * 64   # nothing written
    f32p = ctypes.POINTER(ctypes.c_float)
    assert L.ls_debug_hit_attributes_on_triangle(None, None, None, None, None, None, ctypes.cast(buf, f32p)) == INVALID_ARGUMENT
    assert bytes(buf) == b"\xab" * 64


# ---- the arithmetic ---------------------------------------------------------------------------------------------------

def _pairs(rng, n, origin_scale):
    """n seeded ray / triangle pairs: a triangle, an origin (off zero by origin_scale), a ray aimed at a point of the triangle's
    plane -- inside, outside, ON an edge, ON a corner (the target rounded to float32, so that the decision is the rounding's)"""
    out = []
    for i in range(n):
        S = 10 ** rng.uniform(-1, 2)
        a = rng.uniform(-1, 1, 3) * S
        b = a + rng.normal(size=3) * S * 10 ** rng.uniform(-2, 0)
        c = a + rng.normal(size=3) * S * 10 ** rng.uniform(-2, 0)
        a, b, c = (np.float32(x) for x in (a, b, c))
        o = np.float32(rng.normal(size=3) * origin_scale * S)
        kind = i % 5
        if kind == 0:      # anywhere around the triangle
            w = rng.uniform(-0.5, 1.5, 2)
            target = a + w[0] * (b - a) + w[1] * (c - a)
        elif kind == 1:    # inside
            w = rng.dirichlet([1, 1, 1])
            target = w[0] * a + w[1] * b + w[2] * c
        elif kind == 2:    # on an edge
            u, v = [(a, b), (b, c), (c, a)][i // 5 % 3]
            target = u + rng.uniform(0, 1) * (v.astype(np.float64) - u)
        elif kind == 3:    # on a corner
            target = [a, b, c][i // 5 % 3].astype(np.float64)
        else:              # the midpoint of an edge
            u, v = [(a, b), (b, c), (c, a)][i // 5 % 3]
            target = (u.astype(np.float64) + v) / 2
        d = np.float32((np.asarray(target, np.float64) - o) * (1.0 if i % 7 else rng.uniform(0.1, 10)))
        if i % 11 == 0:
            d = -d         # behind the origin: no hit
        out.append((o, d, a, b, c))
    return out


def test_t_is_bit_equal_to_the_oracle(capi, oracle):
    """pass / fail and t of >= 20 000 pairs with origins off zero are lso_tri_intersect's; with o = 0 they are the frame test's
    as the oracle's brute force over a one-triangle scene gives it"""
    L = oracle.lib()
    f32p = ctypes.POINTER(ctypes.c_float)
    rng = np.random.default_rng(4242)
    pairs = _pairs(rng, 20500, 3.0)
    passed = 0
    for (o, d, a, b, c) in pairs:
        t = ctypes.c_float(0)
        want = L.lso_tri_intersect(*[x.ctypes.data_as(f32p) for x in (o, d, a, b, c)], ctypes.byref(t))
        got = capi.hit_attributes_on_triangle(o, d, a, b, c)
        assert (got is not None) == bool(want), (o, d, a, b, c)
        if want:
            passed += 1
            assert got[0].view(np.uint32) == np.float32(t.value).view(np.uint32), (o, d, a, b, c, got[0], t.value)
    assert 0.3 * len(pairs) < passed < 0.9 * len(pairs)
    # o = 0: the frame's test
    zero = np.zeros(3, np.float32)
    hits = 0
    for (_, d, a, b, c) in _pairs(np.random.default_rng(77), 3000, 0.0):
        scene = types.SimpleNamespace(verts=np.stack([a, b, c]).astype(np.float32), tris=np.array([[0, 1, 2]], np.uint32))
        t, gid = oracle.trace_bruteforce(d.reshape(1, 3), scene, 1)
        got = capi.hit_attributes_on_triangle(zero, d, a, b, c)
        assert (got is not None) == (gid[0] == 0), (d, a, b, c)
        if got is not None:
            hits += 1
            assert got[0].view(np.uint32) == t[0].view(np.uint32), (d, a, b, c, got[0], t[0])
    assert hits > 900


def _min_angle(a, b, c):
    out = np.pi
    for (u, v, w) in ((a, b, c), (b, c, a), (c, a, b)):
        e, f = v - u, w - u
        out = min(out, np.arccos(np.clip((e @ f) / (np.linalg.norm(e) * np.linalg.norm(f)), -1, 1)))
    return out


def test_attributes_against_float64(capi):
    """Well-conditioned cases (|C| / e_min <= 10, |cos| >= 0.2, smallest angle alpha >= 20 degrees), with B = k 2^-24 / sin(alpha), k = 16:
    | |n| - 1 | and |n . e| / |e| for both edges within B; n along (v1 - v0) x (v2 - v0); |cos_inc - cos64| within B; the point
    (1 - u - v) v0 + u v1 + v v2, formed in float64 from the float32 u, v, within k 2^-24 (|C| / e_min) / (|cos| sin(alpha)) e_max
    + 4 ulps of the largest corner coordinate of the float64 ray / plane point -- which is what says that u goes with v1 and v with v2.
    Largest error / bound ratios observed over the 6 000 cases of this seed (printed with -s): | |n| - 1 | 0.088, n . e 0.072,
    cos_inc 0.137, the point 0.043 -- k = 16 holds with a factor of 7 in hand, so it stays."""
    rng = np.random.default_rng(31337)
    k = 16.0
    worst = dict(norm=0.0, edge=0.0, cos=0.0, point=0.0)
    n_checked = 0
    while n_checked < 6000:
        S = 10 ** rng.uniform(-1, 2)
        a = rng.uniform(-1, 1, 3) * S
        L = S * 10 ** rng.uniform(-2, 0)
        b, c = a + rng.normal(size=3) * L, a + rng.normal(size=3) * L
        a, b, c = (np.float32(x).astype(np.float64) for x in (a, b, c))
        alpha = _min_angle(a, b, c)
        if alpha < np.radians(20.0):
            continue
        edges = [np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b)]
        e_min, e_max = min(edges), max(edges)
        w = rng.dirichlet([1, 1, 1])
        target = w[0] * a + w[1] * b + w[2] * c
        nrm = np.cross(b - a, c - a)
        nrm /= np.linalg.norm(nrm)
        # an origin within a few edge lengths, on either side, the ray at any incidence down to cos = 0.2
        side = rng.choice([-1.0, 1.0])
        tang = np.cross(nrm, rng.normal(size=3))
        tang /= np.linalg.norm(tang)
        cosv = rng.uniform(0.22, 1.0)
        back = side * nrm * cosv + tang * np.sqrt(1 - cosv * cosv)
        o = np.float32(target + back * e_min * rng.uniform(0.5, 8.0)).astype(np.float64)
        d = np.float32((target - o) * 10 ** rng.uniform(-1, 1)).astype(np.float64)
        C = a - o
        cos64 = -(nrm @ d) / np.linalg.norm(d)
        if np.linalg.norm(C) / e_min > 10.0 or abs(cos64) < 0.2:
            continue
        t64 = (nrm @ C) / (nrm @ d)
        P = o + t64 * d
        # inside with a margin, so that the float32 test passes
        ww = np.linalg.solve(np.stack([b - a, c - a, nrm], 1), P - a)
        if ww[0] < 0.02 or ww[1] < 0.02 or ww[0] + ww[1] > 0.98:
            continue
        got = capi.hit_attributes_on_triangle(o, d, a, b, c)
        assert got is not None, (o, d, a, b, c)
        t, r = got
        n32, cos32, u, v, p = r[0:3].astype(np.float64), float(r[3]), float(r[4]), float(r[5]), r[6:9].astype(np.float64)
        B = k * EPS / np.sin(alpha)
        worst["norm"] = max(worst["norm"], abs(np.linalg.norm(n32) - 1.0) / B)
        assert abs(np.linalg.norm(n32) - 1.0) <= B
        for e in (b - a, c - a):
            worst["edge"] = max(worst["edge"], abs(n32 @ e) / np.linalg.norm(e) / B)
            assert abs(n32 @ e) / np.linalg.norm(e) <= B, (a, b, c, n32)
        assert n32 @ np.cross(b - a, c - a) > 0
        worst["cos"] = max(worst["cos"], abs(cos32 - cos64) / B)
        assert abs(cos32 - cos64) <= B, (cos32, cos64)
        assert (cos32 > 0) == (side > 0)
        Q = (1.0 - u - v) * a + u * b + v * c
        S_c = max(np.abs(x).max() for x in (a, b, c))
        bound = k * EPS * (np.linalg.norm(C) / e_min) / (abs(cos64) * np.sin(alpha)) * e_max + 4 * float(np.spacing(np.float32(S_c)))
        worst["point"] = max(worst["point"], np.abs(Q - P).max() / bound)
        assert np.abs(Q - P).max() <= bound, (o, d, a, b, c, u, v, Q, P)
        # p = o + t d, one product and one sum per axis
        t32 = np.float32(t)
        assert np.array_equal(r[6:9], np.float32(o) + t32 * np.float32(d))
        n_checked += 1
    print("largest error / bound:", worst)
    assert max(worst.values()) <= 1.0


def test_tiny_and_huge_triangles_stay_finite(capi):
    """edge 1e-18 (Ng . Ng underflows to 0 in float32) and edge 1e15 (it overflows), hit head-on: the pre-scaled normal is unit"""
    for L in (1e-18, 1e15):
        a, b, c = np.float32([-L, -L, 0]), np.float32([L, -L, 0]), np.float32([0, L, 0])
        for (o, d, front) in ((np.float32([0, 0, 1]), np.float32([0, 0, -1]), True), (np.float32([0, 0, -2]), np.float32([0, 0, 4]), False)):
            got = capi.hit_attributes_on_triangle(o, d, a, b, c)
            assert got is not None, L
            t, r = got
            assert np.all(np.isfinite(r))
            assert abs(float(np.linalg.norm(r[0:3].astype(np.float64))) - 1.0) <= 4 * EPS
            assert r[2] == 1.0 and r[3] == (1.0 if front else -1.0)
            assert t == (1.0 if front else 0.5)
            assert abs(float(r[4]) - 0.25) <= 1e-6 and abs(float(r[5]) - 0.5) <= 1e-6   # the origin's foot: 1/4 v0 + 1/4 v1 + 1/2 v2
