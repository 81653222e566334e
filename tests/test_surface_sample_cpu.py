"""ls_sample_surface without a device: the symbols and the descriptor, the check's refusals (there is no GPU where `-m "not gpu"`
runs), the numpy reference (tests/surface_sample_reference.py) against the three host hooks of the shared arithmetic
(ls_debug_surface_weights, ls_debug_surface_pick, ls_debug_surface_point) byte for byte, Philox against the paper's known answers,
the points against float64, and the distribution of the reference's draws."""
import ctypes
import os
import re

import numpy as np

import surface_sample_reference as ref
from conftest import ROOT

INVALID_ARGUMENT = -2
F = np.float32
U64 = np.uint64
M32 = 0xFFFFFFFF


# ---- the hooks ------------------------------------------------------------------------------------------------------------------

def hook_weights(capi, tris):
    """ls_debug_surface_weights -> (area float32 (n), weight uint64 (n), prefix uint64 (n + 1), info)"""
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    n = t.shape[0]
    a, w, P, info = np.full(n, 7, np.float32), np.full(n, 7, U64), np.full(n + 1, 7, U64), np.zeros(1, ref.INFO_DTYPE)
    assert capi.load().ls_debug_surface_weights(t.ctypes.data, n, a.ctypes.data, w.ctypes.data, P.ctypes.data, info.ctypes.data) == 0
    return a, w, P, info[0]


def hook_pick(capi, P, r64):
    P = np.ascontiguousarray(P, U64)
    out = ctypes.c_uint32(12345)
    assert capi.load().ls_debug_surface_pick(P.ctypes.data, P.shape[0] - 1, int(r64), ctypes.byref(out)) == 0
    return out.value


def hook_point(capi, tri9, x2, x3):
    t = np.ascontiguousarray(tri9, np.float32).reshape(9)
    out = np.full(9, 7, np.float32)
    assert capi.load().ls_debug_surface_point(t.ctypes.data, int(x2), int(x3), out.ctypes.data) == 0
    return out


def same_table(capi, tris):
    """the reference's steps 2 to 5 against the hook, byte for byte -> (a, w, P, info) of the reference"""
    a, w, P, info = ref.table(tris)
    ha, hw, hP, hinfo = hook_weights(capi, tris)
    bad = np.nonzero(a.view(np.uint32) != ha.view(np.uint32))[0]
    assert bad.size == 0, ("area", bad[:5], a[bad[:5]], ha[bad[:5]])
    assert info.tobytes() == hinfo.tobytes(), (info, hinfo)
    assert w.tobytes() == hw.tobytes() and P.tobytes() == hP.tobytes()
    if P[-1]:
        assert (1 << 30) <= int(w.max()) < (1 << 31) and int(P[-1]) < (1 << 63)
    return a, w, P, info


# ---- the surface -----------------------------------------------------------------------------------------------------------------

def test_symbols_descriptor_and_records(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in ("ls_sample_surface", "ls_sample_surface_host", "ls_surface_sample_check"):
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    for s in ("ls_debug_surface_weights", "ls_debug_surface_pick", "ls_debug_surface_point"):
        assert s in capi.DEBUG_SYMBOLS and hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "lidarshooter_hip.h")).read()
    assert ("int ls_sample_surface(ls_tracer *tr, void *hip_stream, const ls_surface_sample_desc *desc, const float *sensor_to_out3x4,\n"
            "                      const uint8_t *d_select, uint32_t n_select, void *d_samples, void *d_info);") in hdr
    assert ("int ls_sample_surface_host(ls_tracer *tr, const ls_surface_sample_desc *desc, const float *sensor_to_out3x4,\n"
            "                           const uint8_t *select, uint32_t n_select, void *samples, void *info);") in hdr
    assert "int ls_surface_sample_check(const ls_surface_sample_desc *desc);" in hdr
    assert re.search(r"#define LS_SURFACE_SAMPLE_FLAGS 0u", hdr)
    assert ctypes.sizeof(capi.SurfaceSampleDesc) == 32
    assert capi.SURFACE_SAMPLE_DTYPE == ref.DTYPE and capi.SURFACE_SAMPLE_DTYPE.itemsize == 48
    assert [capi.SURFACE_SAMPLE_DTYPE.fields[k][1] for k in ("p", "geom", "n", "prim", "u", "v", "tri", "flags")] == [0, 12, 16, 28, 32, 36, 40, 44]
    assert capi.SURFACE_INFO_DTYPE == ref.INFO_DTYPE and capi.SURFACE_INFO_DTYPE.itemsize == 16
    assert capi.ABI_VERSION == 4
    d = capi.SurfaceSampleDesc.make(10, seed=3, first_sample=(1 << 40) + 5)
    assert (d.first_sample, d.n_samples, d.seed, d.flags, list(d.reserved)) == ((1 << 40) + 5, 10, 3, 0, [0, 0, 0])


def test_check_refusals(capi):
    L = capi.load()
    make = capi.SurfaceSampleDesc.make
    assert L.ls_surface_sample_check(None) == INVALID_ARGUMENT
    assert L.ls_surface_sample_check(ctypes.byref(make(0))) == 0
    assert L.ls_surface_sample_check(ctypes.byref(make(0xFFFFFFFF, seed=0xFFFFFFFF, first_sample=(1 << 64) - 1))) == 0
    for flags in (1, 2, 0x80000000):
        assert L.ls_surface_sample_check(ctypes.byref(make(16, flags=flags))) == INVALID_ARGUMENT
    for k in range(3):
        d = make(16)
        d.reserved[k] = 1
        assert L.ls_surface_sample_check(ctypes.byref(d)) == INVALID_ARGUMENT
    # the hooks refuse a missing input or result
    buf = np.zeros(32, np.float32)
    out = ctypes.c_uint32(0)
    assert L.ls_debug_surface_weights(None, 1, None, None, None, None) == INVALID_ARGUMENT
    assert L.ls_debug_surface_weights(None, 0, None, None, None, None) == 0
    assert L.ls_debug_surface_pick(None, 0, 0, ctypes.byref(out)) == INVALID_ARGUMENT
    assert L.ls_debug_surface_pick(buf.ctypes.data, 0, 0, None) == INVALID_ARGUMENT
    assert L.ls_debug_surface_point(None, 0, 0, buf.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_debug_surface_point(buf.ctypes.data, 0, 0, None) == INVALID_ARGUMENT


# ---- Philox ----------------------------------------------------------------------------------------------------------------------

# the known answers of Random123's kat_vectors for philox4x32-10 (tests/test_returns_cpu.py holds the library's generator to them)
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def test_philox_known_answers_and_the_sample_counter(capi):
    for ctr, key, want in KAT:
        assert tuple(int(x[0]) for x in ref.philox4x32(*ctr, *key)) == want
    rng = np.random.default_rng(5)
    ctr, key = rng.integers(0, 1 << 32, (300, 4), dtype=np.uint64), rng.integers(0, 1 << 32, (300, 2), dtype=np.uint64)
    got = np.stack(ref.philox4x32(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1]), axis=1)
    for k in range(300):
        assert tuple(int(x) for x in capi.philox4x32(ctr[k], key[k])) == tuple(int(x) for x in got[k])
    # sample j: key (seed, 1), counter (lo32 j, hi32 j, 0, 0); the counter's high word counts on past 2^32, and j wraps at 2^64
    first = (1 << 32) - 3
    x = np.stack(ref.words(77, first, 8), axis=1)
    for k in range(8):
        j = first + k
        assert tuple(int(v) for v in x[k]) == tuple(int(v) for v in capi.philox4x32((j & M32, j >> 32, 0, 0), (77, 1)))
    x = np.stack(ref.words(9, (1 << 64) - 2, 4), axis=1)
    for k, j in enumerate(((1 << 64) - 2, (1 << 64) - 1, 0, 1)):
        assert tuple(int(v) for v in x[k]) == tuple(int(v) for v in capi.philox4x32((j & M32, j >> 32, 0, 0), (9, 1)))
    # the 64 x 64 -> high 64 product
    a, b = rng.integers(0, 1 << 64, 2000, dtype=np.uint64), rng.integers(0, 1 << 63, 2000, dtype=np.uint64)
    a[:4], b[:4] = (0, (1 << 64) - 1, (1 << 64) - 1, 1 << 32), (5, (1 << 63) - 1, 1, 1 << 32)
    assert [int(v) for v in ref.mulhi64(a, b)] == [(int(p) * int(q)) >> 64 for p, q in zip(a, b)]


# ---- areas, weights, prefix ------------------------------------------------------------------------------------------------------

def random_triangles(rng, n, lo=-3.0, hi=1.5):
    """n triangles with sizes log-uniform in 10^lo .. 10^hi around centres within 50 m"""
    centre = rng.uniform(-50.0, 50.0, (n, 1, 3))
    size = 10.0 ** rng.uniform(lo, hi, (n, 1, 1))
    return (centre + size * rng.uniform(-1.0, 1.0, (n, 3, 3))).astype(np.float32)


def odd_triangles():
    """needles, segments and points, non-finite corners, edges of 1e-18 and 1e15 next to ordinary ones"""
    t = []
    t.append([[0, 0, 0], [1, 0, 0], [0, 1, 0]])                               # ordinary
    t.append([[0, 0, 0], [100, 0, 0], [50, 1e-6, 0]])                         # needles
    t.append([[3, 3, 3], [3 + 1e-4, 3, 3], [3, 3 + 40, 3 + 40]])
    t.append([[1, 2, 3], [4, 5, 6], [4, 5, 6]])                               # segments
    t.append([[1, 2, 3], [2, 4, 6], [3, 6, 9]])                               # (collinear)
    t.append([[7, 7, 7]] * 3)                                                 # a point
    t.append([[0, 0, 0]] * 3)
    for bad in (np.nan, np.inf, -np.inf):                                     # non-finite corners, in every position
        for k in range(9):
            q = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64).reshape(9)
            q[k] = bad
            t.append(q.reshape(3, 3))
    t.append([[0, 0, 0], [1e-18, 0, 0], [0, 1e-18, 0]])                       # N underflows to a subnormal: 1e-36
    t.append([[5, 5, 5], [5 + 1e-18, 5, 5], [5, 5 + 1e-18, 5]])               # the edge is below the coordinate's ulp: a point
    t.append([[0, 0, 0], [1e15, 0, 0], [0, 1e15, 0]])                         # 5e29: finite
    t.append([[0, 0, 0], [1e15, 1e15, 0], [0, 1e15, 1e15]])
    t.append([[0, 0, 0], [1e25, 0, 0], [0, 1e25, 0]])                         # the product overflows: weight 0
    t.append([[3e38, 0, 0], [-3e38, 0, 0], [0, 1, 0]])                        # the edge overflows
    t.append([[0, 0, 0], [2, 0, 0], [0, 3, 0]])
    return np.array(t, np.float64).astype(np.float32)


def test_weights_against_the_hook(capi):
    """>= 100 000 random triangles, sizes over four and a half decades, in sets of their own largest area; the odd cases alone, among
    ordinary triangles, and scaled; a largest area that is an exact power of two and one an ulp below; subnormal areas"""
    rng = np.random.default_rng(20261)
    total = 0
    for n in (1, 2, 255, 256, 257, 4099, 100000):
        a, w, P, info = same_table(capi, random_triangles(rng, n))
        assert info["n_weighted"] == np.count_nonzero(w) > 0
        total += n
    assert total >= 100000
    odd = odd_triangles()
    a, w, P, info = same_table(capi, odd)
    assert int(np.argmax(a)) == 37 and info["exponent"] == 99 - 30      # sqrt(3) / 2 * 1e30 lies in [2^99, 2^100)
    assert np.count_nonzero(a) == 7 and info["n_weighted"] == 2          # the 1e15 pair alone is within 2^30 of the largest
    assert not a[3:34].any() and not a[35] and not a[38] and not a[39]
    # without the giants the ordinary ones weigh, the needles too; the subnormal one is too small
    a, w, P, info = same_table(capi, np.concatenate([odd[:36], odd[40:]]))
    assert w[0] > 0 and w[1] > 0 and w[2] > 0 and w[34] == 0 and a[34] > 0 and info["n_weighted"] == 4
    # among random ones, in runs
    mixed = np.concatenate([odd, random_triangles(rng, 300), odd, random_triangles(rng, 5), odd])
    same_table(capi, mixed)
    # a power of two: legs 2 and 1 give a = 1.0 exactly; an ulp below: legs 2 - 2^-22 ... the float below 2, and 1
    pow2 = np.array([[[0, 0, 0], [2, 0, 0], [0, 1, 0]], [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]]], np.float32)
    a, w, P, info = same_table(capi, pow2)
    assert a[0] == F(1.0) and info["exponent"] == -30 and w[0] == 1 << 30 and w[1] == 1 << 29
    below = pow2.copy()
    below[0, 1, 0] = np.nextafter(F(2), F(0))
    a, w, P, info = same_table(capi, below)
    assert a[0] == np.nextafter(F(1), F(0)) and info["exponent"] == -31 and w[0] == (1 << 31) - 128 and w[1] == 1 << 30
    # subnormal areas: alone (the largest is subnormal too), and under a normal one
    tiny = (rng.uniform(-1, 1, (500, 3, 3)) * 10.0 ** rng.uniform(-20.5, -19.5, (500, 1, 1))).astype(np.float32)
    a, w, P, info = same_table(capi, tiny)
    assert 0 < a.max() < F(1.1754944e-38) and info["n_weighted"] > 400 and info["exponent"] < -126 - 30
    one = np.array([[[0, 0, 0], [2 ** -149, 0, 0], [0, 1, 0]]], np.float32)                  # N = 2^-149, a = 0.5 * 2^-149 -> +0
    a, w, P, info = same_table(capi, one)
    assert a[0] == 0 and P[-1] == 0 and info["exponent"] == 0 and info["n_weighted"] == 0
    least = np.array([[[0, 0, 0], [2 ** -148, 0, 0], [0, 1, 0]]], np.float32)                # a = 2^-149, the least area there is
    a, w, P, info = same_table(capi, least)
    assert a.view(np.uint32)[0] == 1 and info["exponent"] == -149 - 30 and w[0] == 1 << 30
    a, w, P, info = same_table(capi, np.concatenate([tiny[:50] * F(2.0 ** 14), pow2[2:] * F(2.0 ** -50)]))
    assert info["n_weighted"] >= 1
    # nothing to weigh
    a, w, P, info = same_table(capi, odd[3:34])
    assert P[-1] == 0 and not w.any() and info["exponent"] == 0 and info["n_weighted"] == 0
    a, w, P, info = same_table(capi, np.zeros((0, 3, 3), np.float32))
    assert P.shape == (1,) and P[0] == 0


# ---- the pick --------------------------------------------------------------------------------------------------------------------

def _r_for(T, W):
    """the least 64-bit word r with hi64(r W) == T"""
    r = -((-T << 64) // W)
    assert (r * W) >> 64 == T and (r == 0 or ((r - 1) * W) >> 64 < T)
    return r


def test_pick_on_every_prefix_entry_and_at_both_ends(capi):
    """a table with runs of zero weights at the start, in the middle and at the end: r64 = 0 and 2^64 - 1, T exactly on every P[i]
    (and one below it); a table of one; W = 0"""
    w = np.array([0, 0, 0, 5, 1, 0, 0, 0, 0, 7, 1 << 30, 0, 3, 3, 0, (1 << 31) - 1, 1, 0, 0], U64)
    P = ref.prefix(w)
    W = int(P[-1])
    nz = np.nonzero(w)[0]
    assert hook_pick(capi, P, 0) == nz[0] == int(ref.pick(P, 0)[0])
    assert hook_pick(capi, P, (1 << 64) - 1) == nz[-1] == int(ref.pick(P, (1 << 64) - 1)[0])
    for i in range(w.shape[0]):
        T = int(P[i])
        if T >= W:
            continue
        want = max(k for k in range(w.shape[0]) if int(P[k]) <= T)          # the last of a run of equal entries: the one with a weight
        assert w[want] > 0
        for r in (_r_for(T, W), _r_for(T + 1, W) - 1 if T + 1 < W else (1 << 64) - 1):
            assert hook_pick(capi, P, r) == want == int(ref.pick(P, r)[0]), (i, r)
        if T:
            below = max(k for k in range(w.shape[0]) if int(P[k]) <= T - 1)
            assert hook_pick(capi, P, _r_for(T, W) - 1) == below == int(ref.pick(P, _r_for(T, W) - 1)[0])
    rng = np.random.default_rng(3)
    big = ref.prefix(rng.integers(0, 1 << 31, 5000, dtype=np.uint64) * (rng.uniform(size=5000) < 0.6))
    r = rng.integers(0, 1 << 64, 3000, dtype=np.uint64)
    want = ref.pick(big, r)
    assert [hook_pick(capi, big, int(x)) for x in r] == [int(x) for x in want]
    one = ref.prefix(np.array([9], U64))
    assert hook_pick(capi, one, 0) == 0 and hook_pick(capi, one, (1 << 64) - 1) == 0
    for none in (ref.prefix(np.zeros(4, U64)), np.zeros(1, U64)):
        assert hook_pick(capi, none, 123) == ref.INV == int(ref.pick(none, 123)[0])


# ---- the barycentrics and the point ----------------------------------------------------------------------------------------------

def _same_point(capi, tri, x2, x3):
    u, v, w = ref.bary([x2], [x3])
    _, n = ref.areas(tri[None])
    want = np.concatenate([ref.point(tri[None], u, v, w)[0], n[0], u, v, w]).astype(np.float32)
    got = hook_point(capi, tri, x2, x3)
    assert got.tobytes() == want.tobytes(), (tri, x2, x3, got, want)
    return got


def test_fold_and_the_point_against_the_hook(capi):
    tri = np.array([[1.25, -2.5, 0.75], [4.5, 0.125, 1.0], [2.0, 3.5, -1.5]], np.float32)
    one = 1 << 24
    S = F(2.0 ** -24)
    for al, be, u, v in ((one - 5, 5, one - 5, 5),                       # alpha + beta = 2^24: no fold, gamma = 0
                         (one - 5, 6, 5, one - 6),                       # 2^24 + 1: folded
                         (0, 12345, 0, 12345), (54321, 0, 54321, 0), (0, 0, 0, 0),
                         (one - 1, one - 1, 1, 1), (one - 1, 0, one - 1, 0), (0, one - 1, 0, one - 1), (one >> 1, (one >> 1) + 1, one >> 1, (one >> 1) - 1)):
        for low in (0, 0xFF):                                            # the low eight bits of the words do not count
            got = _same_point(capi, tri, (al << 8) | low, (be << 8) | low)
            assert got[6] == F(u) * S and got[7] == F(v) * S and got[8] == F(one - u - v) * S
            assert float(got[6]) + float(got[7]) + float(got[8]) == 1.0 and got[6:].min() >= 0
    got = _same_point(capi, tri, 0, 0)
    assert got[:3].tobytes() == tri[0].tobytes()                          # u = v = 0: the first corner, bit for bit
    assert _same_point(capi, tri, (one - 1) << 8 | 0xFF, 0)[6] == F(one - 1) * S
    rng = np.random.default_rng(8)
    odd = odd_triangles()
    tris = np.concatenate([random_triangles(rng, 3000), odd[np.all(np.isfinite(odd), axis=(1, 2))]])   # (which NaN a NaN corner leaves is nobody's promise)
    x = rng.integers(0, 1 << 32, (tris.shape[0], 2), dtype=np.uint64)
    for t, (x2, x3) in zip(tris, x):
        _same_point(capi, t, int(x2), int(x3))


def test_points_and_normals_against_float64():
    """test_closest_cpu's bound, 2e-6 * S (S the largest |coordinate| of the triangle): the point against a float64 evaluation of its own
    barycentrics -- which are >= 0 and add up to 1 exactly, so that evaluation is a point of the triangle and every sample lies within
    the bound of its triangle; the normal unit to 1e-6 and along the float64 cross product"""
    rng = np.random.default_rng(31)
    n = 200000
    tris = random_triangles(rng, n)
    x2, x3 = rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 1 << 32, n, dtype=np.uint64)
    u, v, w = ref.bary(x2, x3)
    p = ref.point(tris, u, v, w)
    u64, v64, w64 = (z.astype(np.float64) for z in (u, v, w))
    assert np.all(u64 + v64 + w64 == 1.0) and min(u.min(), v.min(), w.min()) >= 0
    q = tris.astype(np.float64)
    p64 = w64[:, None] * q[:, 0] + u64[:, None] * q[:, 1] + v64[:, None] * q[:, 2]
    S = np.abs(q).max(axis=(1, 2))
    err = np.abs(p - p64).max(axis=1) / S
    print("largest |p - p64| / S", err.max())
    assert err.max() <= 2e-6
    a, nrm = ref.areas(tris)
    N = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    L = np.linalg.norm(N, axis=1)
    fat = L > 1e-3 * np.linalg.norm(q[:, 1] - q[:, 0], axis=1) * np.linalg.norm(q[:, 2] - q[:, 0], axis=1)   # (a sliver's cross product cancels)
    assert fat.mean() > 0.99
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert np.abs(nrm[fat] - (N / L[:, None])[fat]).max() <= 1e-3
    assert np.abs(a[fat] / (0.5 * L[fat]) - 1.0).max() <= 1e-3


# ---- the distribution ------------------------------------------------------------------------------------------------------------

DISTRIBUTION_SEED = 2026


def test_draws_follow_the_weights():
    """50 triangles whose areas span 1 : 1000, 200 000 samples of the reference under a fixed seed: every triangle's count within
    5 sqrt(n p (1 - p)) + 1 of n p, p = w_i / W; the fold leaves the barycentrics' centroid within 0.005 of (1/3, 1/3)"""
    k, n = 50, 200000
    side = np.sqrt(10.0 ** np.linspace(0.0, 3.0, k)) * 0.01                  # legs: areas 0.5 * side^2, 1 : 1000
    tris = np.zeros((k, 3, 3), np.float32)
    tris[:, 0] = np.stack([np.arange(k), np.zeros(k), np.zeros(k)], axis=1)
    tris[:, 1] = tris[:, 0] + np.stack([side, np.zeros(k), np.zeros(k)], axis=1).astype(np.float32)
    tris[:, 2] = tris[:, 0] + np.stack([np.zeros(k), side, np.zeros(k)], axis=1).astype(np.float32)
    a, w, P, info = ref.table(tris)
    assert 900 < a.max() / a.min() < 1100 and w.min() > 0
    rec, _ = ref.samples(tris, np.zeros(k, np.uint32), np.arange(k), np.arange(k), DISTRIBUTION_SEED, 0, n)
    assert np.all(rec["flags"] == 1)
    count = np.bincount(rec["tri"], minlength=k)
    p = w.astype(np.float64) / float(P[-1])
    dev = np.abs(count - n * p) / (5 * np.sqrt(n * p * (1 - p)) + 1)
    print("largest deviation in units of the bound", dev.max())
    assert dev.max() <= 1.0
    cu, cv = rec["u"].astype(np.float64).mean(), rec["v"].astype(np.float64).mean()
    print("centroid", cu, cv)
    assert abs(cu - 1 / 3) <= 0.005 and abs(cv - 1 / 3) <= 0.005
    # inside the triangles: x - x0 and y - y0 within the legs, and under the hypotenuse to rounding
    t = rec["tri"]
    dx, dy = (rec["p"][:, 0] - tris[t, 0, 0]) / side[t], rec["p"][:, 1] / side[t]
    assert dx.min() >= -1e-3 and dy.min() >= 0 and (dx + dy).max() <= 1 + 1e-3      # (x near 49 rounds to 4e-6, a leg is 0.01 and more)
