"""ls_hit_velocities / ls_hit_velocities_host / ls_twist_table_constant without a device: the symbols and their signatures, the
refusal of a NULL handle, the one new operation sequence -- the rigid-body velocity field of a twist at a hit point, the velocity of
the sensor's origin and the range rate (ls_debug_hit_velocity, the host compilation of what k_hit_velocities runs) -- against a
restatement written here in np.float32 operations, bit for bit, and against float64 within a derived bound; and the constant-twist
table against its double formula and against a central difference of ls_motion_constant_twist's own motion."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

INVALID_ARGUMENT = -2
F = np.float32
EPS = 2.0 ** -24
QNAN = 0x7FC00000


def _header(name="lidarshooter_hip.h"):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", name)).read())


# ---- the restatement and the bound (shared with test_gpu_velocity.py) ----------------------------------------------------------

def _restate_field(tw, x, n):
    if tw is None:
        return [np.zeros(n, np.float32) for _ in range(3)]
    return [tw[:, 3] + (tw[:, 1] * x[2] - tw[:, 2] * x[1]),
            tw[:, 4] + (tw[:, 2] * x[0] - tw[:, 0] * x[2]),
            tw[:, 5] + (tw[:, 0] * x[1] - tw[:, 1] * x[0])]


def restate_hit_velocity(cast, t, sensor_twist, geom_twist):
    """the 32-byte records, uint32 (n, 8), of valid hits at t (n,) along the cast ray records (n, 8) with the twist records (n, 6) =
    [w | u] of the sensor and of the geometry (None: at rest, +0): P_i = o_i + t c_i; v(x)_0 = u_0 + (w_1 x_2 - w_2 x_1) and its
    cyclic siblings at P and at o; rel = v_s - v_o; radial = ((rel_0 c_0 + rel_1 c_1) + rel_2 c_2) / sqrt((c_0 c_0 + c_1 c_1) + c_2
    c_2) -- every product, difference, sum, root and quotient rounded to float32; flags = 1"""
    r, t = np.asarray(cast, np.float32), np.asarray(t, np.float32)
    n = r.shape[0]
    st, gt = (None if x is None else np.asarray(x, np.float32) for x in (sensor_twist, geom_twist))
    with np.errstate(all="ignore"):
        o, c = [r[:, i] for i in range(3)], [r[:, 4 + i] for i in range(3)]
        P = [o[i] + t * c[i] for i in range(3)]
        vs, vo = _restate_field(gt, P, n), _restate_field(st, o, n)
        rel = [vs[i] - vo[i] for i in range(3)]
        length = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        radial = ((rel[0] * c[0] + rel[1] * c[1]) + rel[2] * c[2]) / length
    out = np.zeros((n, 8), np.uint32)
    for i in range(3):
        out[:, i], out[:, 4 + i] = vs[i].astype(F).view(np.uint32), vo[i].astype(F).view(np.uint32)
    out[:, 3], out[:, 7] = radial.astype(F).view(np.uint32), 1
    return out


def same_floats(got, want):
    """uint32 words of float32 values: equal bit for bit, a NaN equal to any NaN (its sign and payload depend on the machine)"""
    g, w = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    nan_g, nan_w = np.isnan(g.view(F)), np.isnan(w.view(F))
    return g.shape == w.shape and np.array_equal(nan_g, nan_w) and np.array_equal(np.where(nan_g, QNAN, g), np.where(nan_w, QNAN, w))


def float64_velocity(cast, t, sensor_twist, geom_twist):
    """the same quantities in float64 from the float32 inputs taken as doubles -> (v_s (n, 3), v_o (n, 3), radial (n,))"""
    r, t = np.asarray(cast, np.float64), np.asarray(t, np.float64)
    o, c = r[:, 0:3], r[:, 4:7]
    P = o + t[:, None] * c
    z = np.zeros_like(P)
    vs = z if geom_twist is None else np.asarray(geom_twist, np.float64)[:, 3:6] + np.cross(np.asarray(geom_twist, np.float64)[:, 0:3], P)
    vo = z if sensor_twist is None else np.asarray(sensor_twist, np.float64)[:, 3:6] + np.cross(np.asarray(sensor_twist, np.float64)[:, 0:3], o)
    return vs, vo, np.einsum("ki,ki->k", vs - vo, c) / np.linalg.norm(c, axis=1)


def velocity_bound(cast, t, sensor_twist, geom_twist):
    """how far the float32 sequence may be from float64_velocity, per record, from the operation count; e = 2^-24, every rounding
    at most e times the magnitude of its result, second-order terms covered by the final factor 1.01 -> (bound on each component of
    v_s (n, 3), on radial (n,)):
      P_i = fl(o_i + fl(t c_i)):                 dP_i <= e (|t c_i| + |P_i|)
      a product w_j P_k:                          |w_j| dP_k + e |w_j P_k|
      their difference, then the sum with u_i:    e (|w_j P_k| + |w_k P_j|), then e (|u_i| + |w_j P_k| + |w_k P_j|)
      -> dv_s,i <= |w_j| dP_k + |w_k| dP_j + e (|u_i| + 3 (|w_j P_k| + |w_k P_j|));  dv_o,i likewise at o, which is exact (dP = 0)
      rel_i = fl(v_s,i - v_o,i):                  drel_i <= dv_s,i + dv_o,i + e |rel_i|
      the dot product, three products and two sums: sum_i |c_i| drel_i + 3 e sum_i |rel_i c_i|
      len: three products, two sums, a root:      relative 3 e / 2 + e;  the quotient: relative e
      -> dradial <= (sum_i |c_i| drel_i + 3 e sum_i |rel_i c_i|) / |c| + 4 e |radial|"""
    r, t = np.asarray(cast, np.float64), np.asarray(t, np.float64)
    n = r.shape[0]
    o, c = r[:, 0:3], r[:, 4:7]
    tc = np.abs(t[:, None] * c)
    P = o + t[:, None] * c
    dP = EPS * (tc + np.abs(P))

    def field(tw, x, dx):
        if tw is None:
            return np.zeros((n, 3))
        tw = np.abs(np.asarray(tw, np.float64))
        w, u, x = tw[:, 0:3], tw[:, 3:6], np.abs(x)
        out = np.zeros((n, 3))
        for i, (j, k) in enumerate(((1, 2), (2, 0), (0, 1))):
            out[:, i] = w[:, j] * dx[:, k] + w[:, k] * dx[:, j] + EPS * (u[:, i] + 3.0 * (w[:, j] * x[:, k] + w[:, k] * x[:, j]))
        return out

    dvs, dvo = field(geom_twist, P, dP), field(sensor_twist, o, np.zeros((n, 3)))
    vs, vo, radial = float64_velocity(cast, t, sensor_twist, geom_twist)
    rel = vs - vo
    drel = dvs + dvo + EPS * np.abs(rel)
    length = np.linalg.norm(c, axis=1)
    drad = (np.sum(np.abs(c) * drel, axis=1) + 3.0 * EPS * np.sum(np.abs(rel * c), axis=1)) / length + 4.0 * EPS * np.abs(radial)
    return 1.01 * dvs, 1.01 * drad


def rodrigues(w, tau):
    """the rotation by w * tau, float64 (3, 3)"""
    w = np.asarray(w, np.float64)
    wn = np.linalg.norm(w)
    a = wn * tau
    if a == 0.0:
        return np.eye(3)
    k = w / wn
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def body_motion(lin, ang, pivot, tau):
    """ls_motion_constant_twist's own motion in float64: x(tau) = Q x_0 + c with Q = rodrigues(ang, tau), c = pivot - Q pivot + lin tau"""
    lin, ang, pivot = (np.asarray(np.float32(x), np.float64) for x in (lin, ang, pivot))
    Q = rodrigues(ang, tau)
    return Q, pivot - Q @ pivot + lin * tau


def _hook(capi, cast, t, st, gt):
    n = cast.shape[0]
    return np.stack([capi.hit_velocity(cast[k], t[k], None if st is None else st[k], None if gt is None else gt[k]) for k in range(n)])


def _random_hits(rng, n):
    """cast rays as a sweep casts them -- origins within a few metres, directions near unit length --, ranges up to 120 m, twists of
    road traffic: up to 2 rad/s and 40 m/s"""
    cast = np.zeros((n, 8), np.float32)
    cast[:, 0:3] = rng.uniform(-3, 3, (n, 3))
    d = rng.normal(size=(n, 3))
    cast[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.999, 1.001, (n, 1))
    cast[:, 7] = 1e16
    t = rng.uniform(0.5, 120.0, n).astype(np.float32)
    tw = [np.concatenate([rng.uniform(-2, 2, (n, 3)), rng.uniform(-40, 40, (n, 3))], axis=1).astype(np.float32) for _ in range(2)]
    return cast, t, tw[0], tw[1]


# ---- exports and refusals ---------------------------------------------------------------------------------------------

def test_velocity_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert capi.load().ls_abi_version() == 4      # the new entry points do not step the ABI version
    for s in ("ls_hit_velocities", "ls_hit_velocities_host", "ls_twist_table_constant"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s
    assert "ls_debug_hit_velocity" in capi.DEBUG_SYMBOLS and hasattr(lib, "ls_debug_hit_velocity")
    for name in ("hitVelocities", "hitVelocitiesDevice"):
        assert callable(getattr(capi.Tracer, name))
    assert callable(capi.twist_table_constant) and callable(capi.hit_velocity)
    assert ctypes.sizeof(capi.GeometryTwist) == 16 and capi.HIT_VELOCITY_DTYPE.itemsize == 32
    hdr = _header()
    assert "#define LS_ABI_VERSION 4" in hdr
    assert re.search(r"typedef struct ls_geometry_twist \{ uint32_t geom; /\*.*?\*/ uint32_t reserved; /\*.*?\*/ const float \*col_twist; /\*.*?\*/ \} "
                     r"ls_geometry_twist;", hdr)
    tables = (r"const float \*{p}col_pose, uint32_t n_cols, const ls_geometry_motion \*motions, uint32_t n_motions, const float \*{p}sensor_twist, "
              r"const ls_geometry_twist \*twists, uint32_t n_twists, uint32_t flags, ")
    assert re.search(r"int ls_hit_velocities\(ls_tracer \*tr, void \*hip_stream, " + tables.format(p="d_") +
                     r"const void \*d_hits, const uint32_t \*d_count, uint32_t n, void \*d_out, float \*d_radial\);", hdr)
    assert re.search(r"int ls_hit_velocities_host\(ls_tracer \*tr, " + tables.format(p="") +
                     r"const void \*hits, uint32_t n, void \*out, float \*radial\);", hdr)
    assert re.search(r"int ls_twist_table_constant\(const float lin_vel\[3\], const float ang_vel\[3\], const float pivot\[3\], double t0, double dt, "
                     r"uint32_t n_cols, float \*col_twist\);", hdr)
    assert re.search(r"int ls_debug_hit_velocity\(const float cast8\[8\], float t, const float sensor_twist6\[6\], const float geom_twist6\[6\], "
                     r"float out8\[8\]\);", _header("lidarshooter_hip_debug.h"))


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    H = 4
    pose = np.tile(F([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), (H, 1))
    twist = np.zeros((H, 6), np.float32)
    mo = (capi.GeometryMotion * 1)()
    mo[0].geom, mo[0].col_motion = 0, pose.ctypes.data
    tw = (capi.GeometryTwist * 1)()
    tw[0].geom, tw[0].col_twist = 0, twist.ctypes.data
    hits = np.zeros(4, capi.HIT_DTYPE)
    out, rad = np.zeros(4 * 32, np.uint8), np.zeros(4, np.float32)
    P, T, Hh = pose.ctypes.data, twist.ctypes.data, hits.ctypes.data
    assert L.ls_hit_velocities(None, None, P, H, mo, 1, T, tw, 1, 0, Hh, None, 4, out.ctypes.data, rad.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_hit_velocities_host(None, P, H, mo, 1, T, tw, 1, 0, Hh, 4, out.ctypes.data, rad.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_hit_velocities_host(None, None, 0, None, 0, None, None, 0, 0, Hh, 4, out.ctypes.data, None) == INVALID_ARGUMENT
    assert not out.any() and not rad.any()
    f32p = ctypes.POINTER(ctypes.c_float)
    res = np.full(8, 7.0, np.float32)
    cast = np.zeros(8, np.float32)
    assert L.ls_debug_hit_velocity(None, 1.0, None, None, res.ctypes.data_as(f32p)) == INVALID_ARGUMENT
    assert L.ls_debug_hit_velocity(cast.ctypes.data_as(f32p), 1.0, None, None, None) == INVALID_ARGUMENT
    assert np.all(res == 7.0)


# ---- the operation sequence --------------------------------------------------------------------------------------------------

def test_hit_velocity_equals_the_restatement(capi):
    rng = np.random.default_rng(20262)
    n = 10000
    cast, t, st, gt = _random_hits(rng, n)
    cast[::17, 0:3] = 0                                              # no pose table: the ray from the origin
    st[::19, 0:3] = 0                                                # pure translations
    gt[::23, 0:3] = 0
    for k in range(0, n, 97):                                        # non-finite entries in either twist, the ray and t
        (st, gt)[k % 2][k, rng.integers(0, 6)] = (np.nan, np.inf, -np.inf)[k % 3]
    cast[5::301, 4 + 1] = np.inf
    t[7::401] = np.nan
    got = _hook(capi, cast, t, st, gt)
    assert same_floats(got[:, 0:7], restate_hit_velocity(cast, t, st, gt)[:, 0:7]) and np.all(got[:, 7] == 1)
    assert np.count_nonzero(~np.isfinite(got[:, 0:7].view(F)).all(axis=1)) >= n // 97
    # both NULL-twist cases, and neither twist: zeros that carry a plus sign, a radial that is a zero
    m = 2000
    no_s, no_g, none = (_hook(capi, cast[:m], t[:m], a, b) for a, b in ((None, gt[:m]), (st[:m], None), (None, None)))
    assert same_floats(no_s[:, 0:7], restate_hit_velocity(cast[:m], t[:m], None, gt[:m])[:, 0:7]) and not no_s[:, 4:7].any()
    assert same_floats(no_g[:, 0:7], restate_hit_velocity(cast[:m], t[:m], st[:m], None)[:, 0:7]) and not no_g[:, 0:3].any()
    assert same_floats(none[:, 0:7], restate_hit_velocity(cast[:m], t[:m], None, None)[:, 0:7])
    assert not none[:, 0:3].any() and not none[:, 4:7].any() and np.all(none[:, 7] == 1)
    fin = np.isfinite(none[:, 3].view(F))
    assert np.count_nonzero(fin) > m // 2 and np.all(none[fin, 3].view(F) == 0)
    # with the geometry's twist alone and a pure translation, v_s is u
    still = gt[:m].copy()
    still[:, 0:3] = 0
    fin = np.isfinite(still).all(axis=1) & np.isfinite(cast[:m]).all(axis=1) & np.isfinite(t[:m])
    assert np.array_equal(_hook(capi, cast[:m], t[:m], None, still)[fin, 0:3].view(F), still[fin, 3:6])


def test_hit_velocity_against_float64(capi):
    """the float32 sequence against the float64 evaluation of the same float32 inputs (float64_velocity), for rays and twists as a
    sweep over road traffic has them (_random_hits): every component of v_s and the radial velocity within velocity_bound, whose
    docstring derives it from the operation count -- it is evaluated per record from the magnitudes of the operands and is about
    1e-5 m/s at 100 m, 2 rad/s and 40 m/s.  Measured over these 20 000 records: the largest error is 0.80 of the bound for v_s and
    0.37 for the radial velocity."""
    rng = np.random.default_rng(78)
    n = 20000
    cast, t, st, gt = _random_hits(rng, n)
    got = _hook(capi, cast, t, st, gt).view(F).astype(np.float64)
    vs, vo, radial = float64_velocity(cast, t, st, gt)
    bvs, brad = velocity_bound(cast, t, st, gt)
    evs, erad = np.abs(got[:, 0:3] - vs), np.abs(got[:, 3] - radial)
    print("largest error / bound: v_s %.3f, radial %.3f; largest bound: v_s %.3g m/s, radial %.3g m/s" %
          ((evs / bvs).max(), (erad / brad).max(), bvs.max(), brad.max()))
    assert np.all(evs <= bvs) and np.all(erad <= brad)
    # a bound that says something: at 120 m, 2 rad/s and 40 m/s its terms add up to at most 2^-24 * (40 + 10 * 2 * 120) = 1.5e-4 m/s
    # per component, three components in the radial velocity -- far below the 0.1 m/s of a table difference
    assert bvs.max() < 2e-4 and brad.max() < 6e-4
    # the wrong sign of the cross product is far outside it
    flipped = gt.copy()
    flipped[:, 0:3] = -flipped[:, 0:3]
    bad = _hook(capi, cast[::10], t[::10], st[::10], flipped[::10]).view(F).astype(np.float64)
    assert np.count_nonzero((np.abs(bad[:, 0:3] - vs[::10]) > bvs[::10]).any(axis=1)) > n // 10 * 0.9


# ---- ls_twist_table_constant ---------------------------------------------------------------------------------------------------

CASES = [((12.0, -9.0, 0.5), (0.05, -0.1, 0.5), (6.0, 2.0, -0.5), 0.0, 0.1 / 16, 16),
         ((3.0, -4.0, 1.0), (0.0, 0.0, 4.0), (7.0, 1.5, -2.0), -0.05, 0.1 / 64, 64),
         ((0.0, 0.0, 0.0), (1.0, 2.0, -0.5), (0.0, 0.0, 0.0), 0.25, 1e-3, 7),
         ((-30.0, 0.1, 0.0), (-0.3, 0.2, 0.1), (-40.0, 25.0, 1.0), 1.0, 2.4e-5, 33)]


@pytest.mark.parametrize("lin,ang,pivot,t0,dt,n", CASES)
def test_twist_table_equals_the_double_formula(capi, lin, ang, pivot, t0, dt, n):
    got = capi.twist_table_constant(lin, ang, pivot, t0, dt, n)
    v, w, p = (np.asarray(np.float32(x), np.float64) for x in (lin, ang, pivot))
    want = np.zeros((n, 6), np.float32)
    for h in range(n):
        tau = t0 + h * dt
        a = p + v * tau
        cross = np.array([w[1] * a[2] - w[2] * a[1], w[2] * a[0] - w[0] * a[2], w[0] * a[1] - w[1] * a[0]])
        want[h, 0:3] = np.float32(ang)
        want[h, 3:6] = np.where(cross != 0.0, (v - cross).astype(np.float32), np.float32(lin))
    assert got.shape == (n, 6) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_zero_angular_velocity_gives_the_linear_velocity_exactly(capi):
    for lin in ((12.0, -9.0, 0.5), (-0.0, 1e-30, 3e7), (0.1, 0.2, 0.3)):
        for pivot in ((0, 0, 0), (5.0, -7.0, 1.0)):
            got = capi.twist_table_constant(lin, (0, 0, 0), pivot, -0.3, 0.01, 50)
            want = np.tile(np.concatenate([np.zeros(3, np.float32), np.float32(lin)]), (50, 1))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_twist_table_is_the_rate_of_the_motion_table(capi):
    """ls_twist_table_constant against a float64 central difference of ls_motion_constant_twist's own motion x(tau) = Q(tau) x_0 +
    c(tau) (body_motion: Rodrigues in double) at tau_h +- d, d = 1e-6 s: for material points x_0, the point is at x = x(tau_h) and
    the table says v = u_h + w_h x x.  Tolerance per component, with m = max(|lin|, |w| r) and r = |x| + |pivot| + |lin tau|:
      the table's single rounding:   2^-24 |u_h| + 2^-24 |w| |x|   (u_h and w_h are each one rounding off the double value)
      the difference's truncation:   d^2 / 6 |x'''| = d^2 / 6 |w|^3 r           (x''' = w x (w x (w x (x - pivot - lin tau))))
      the difference's own rounding: 4 * 2^-53 r / d                             (two values of size r, each a few roundings, over 2 d)
    which is about 1e-5 m/s here, the first term by far the largest."""
    rng = np.random.default_rng(4)
    d = 1e-6
    worst = 0.0
    for lin, ang, pivot, t0, dt, n in CASES:
        tab = capi.twist_table_constant(lin, ang, pivot, t0, dt, n).astype(np.float64)
        v, w, p = (np.asarray(np.float32(x), np.float64) for x in (lin, ang, pivot))
        for h in range(0, n, max(1, n // 8)):
            tau = t0 + h * dt
            for x0 in rng.uniform(-50, 50, (6, 3)):
                (Qa, ca), (Qb, cb), (Q, c) = body_motion(lin, ang, pivot, tau + d), body_motion(lin, ang, pivot, tau - d), body_motion(lin, ang, pivot, tau)
                rate = ((Qa @ x0 + ca) - (Qb @ x0 + cb)) / (2 * d)
                x = Q @ x0 + c
                got = tab[h, 3:6] + np.cross(tab[h, 0:3], x)
                wn, r = np.linalg.norm(w), np.linalg.norm(x) + np.linalg.norm(p) + np.linalg.norm(v * tau)
                tol = EPS * (np.abs(tab[h, 3:6]).max() + wn * np.linalg.norm(x)) + d * d / 6 * wn ** 3 * r + 4 * 2.0 ** -53 * r / d
                err = np.abs(got - rate).max()
                worst = max(worst, err / tol)
                assert err <= tol, (lin, ang, pivot, h, err, tol)
    print("largest error / tolerance: %.3f" % worst)


def test_twist_table_refuses_bad_input(capi):
    L = capi.load()
    f32p = ctypes.POINTER(ctypes.c_float)
    out = np.full((4, 6), 7.0, np.float32)
    good = [np.float32(x) for x in ((1, 2, 3), (0.1, 0.2, 0.3), (4, 5, 6))]

    def call(lin, ang, piv, t0=0.0, dt=0.01, n=4, dst=out):
        ptr = [None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(f32p) for a in (lin, ang, piv)]
        return L.ls_twist_table_constant(*ptr, t0, dt, n, None if dst is None else dst.ctypes.data_as(f32p))

    assert call(None, good[1], good[2]) == INVALID_ARGUMENT and call(good[0], None, good[2]) == INVALID_ARGUMENT
    assert call(good[0], good[1], None) == INVALID_ARGUMENT and call(*good, dst=None) == INVALID_ARGUMENT
    for k in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            a = [g.copy() for g in good]
            a[k][1] = bad
            assert call(*a) == INVALID_ARGUMENT
    assert call(*good, t0=np.nan) == INVALID_ARGUMENT and call(*good, dt=np.inf) == INVALID_ARGUMENT
    assert np.all(out == 7.0)
    assert call(*good, n=0, dst=None) == 0 and call(*good) == 0 and np.all(out[:, 0:3] == good[1])
