"""ls_trace_scene_beams / ls_trace_scene_beams_host / ls_beam_pattern_rings without a device: the symbols, the refusal of a NULL
handle, the sub-ray of a sample (ls_debug_beam_ray, the host compilation of what k_beam_rays runs) and the echoes of a beam
(ls_debug_beam_echoes: the keys, the echo starts and the selection k_beam_reduce runs) against restatements written here --
np.float32 operations in the stated order and a plain Python reduction, bit for bit --, the ring pattern against numpy float64,
and every refusal of a model through ls_debug_beam_model_check."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

INVALID_ARGUMENT, OUT_OF_RANGE = -2, -9
FIRST, LAST, STRONGEST = 1, 2, 4
F = np.float32
INF = float("inf")


def _header(name="lidarshooter_hip.h"):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", name)).read())


# ---- the restatements (shared with test_gpu_beams.py) -------------------------------------------------------------------

def restate_beam_rays(st, ct, cphi, sphi, a, b):
    """the sub-ray records, float32 (n, 8), of samples (a, b) of rays with the factor-table entries st, ct, (cphi, sphi), all float32
    (n,): origin 0, tmin 0, d_i = (d_i + a u_i) + b w_i with d = (st cphi, st sphi, ct), u = (-sphi, cphi, 0), w = (-(ct cphi),
    -(ct sphi), st) -- every product and sum rounded to float32 --, a component -0 made +0, tmax 1e16"""
    st, ct, cphi, sphi, a, b = (np.asarray(x, np.float32) for x in (st, ct, cphi, sphi, a, b))
    d = (st * cphi, st * sphi, ct)
    u = (-sphi, cphi, np.zeros_like(st))
    w = (-(ct * cphi), -(ct * sphi), st)
    r = np.zeros((st.shape[0], 8), np.float32)
    for i in range(3):
        x = (d[i] + a * u[i]) + b * w[i]
        assert x.dtype == np.float32
        r[:, 4 + i] = np.where(x == 0, F(0.0), x)
    r[:, 7] = F(1e16)
    return r


def reduce_beam(r, hit, returns, min_count, separation):
    """the returns of one beam: r float32[S] reported ranges, hit bool[S] -> [(bits of r_e, echo word)] in ascending range.  The
    sub-hits by (r, s) ascending; an echo starts at the first and wherever the float32 difference to the one before exceeds the
    separation; it carries its nearest member and its member count; detectable from min_count members on; FIRST the nearest,
    LAST the farthest, STRONGEST the largest (the nearer of equals); distinct selected echoes, one record each."""
    r = np.asarray(r, np.float32)
    order = sorted((s for s in range(len(r)) if hit[s]), key=lambda s: (float(r[s]), s))
    echoes = []
    with np.errstate(invalid="ignore"):
        for j, s in enumerate(order):
            if j == 0 or F(r[s] - r[order[j - 1]]) > F(separation):
                echoes.append([s, 0])
            echoes[-1][1] += 1
    det = [e for e in echoes if e[1] >= min_count]
    if not det:
        return []
    best = det[0]
    for e in det[1:]:
        if e[1] > best[1]:
            best = e
    out = []
    for e in det:
        kinds = (FIRST if e is det[0] else 0) | (LAST if e is det[-1] else 0) | (STRONGEST if e is best else 0)
        kinds &= returns
        if kinds:
            out.append((int(r[e[0]].view(np.uint32)), kinds | (e[1] << 8) | (e[0] << 16)))
    return out


def rings_f64(half_az, half_el, n_rings, per_ring):
    """ls_beam_pattern_rings in float64: (a, b) unrounded, and k from the float32-rounded a and b"""
    ha, he = float(F(half_az)), float(F(half_el))
    ab = [(0.0, 0.0)]
    for j in range(1, n_rings + 1):
        for i in range(per_ring):
            rho, phi = j / n_rings, 2.0 * np.pi * (i + 0.5 * (j - 1)) / per_ring
            ab.append((ha * rho * np.cos(phi), he * rho * np.sin(phi)))
    ab = np.array(ab, np.float64)
    ab32 = ab.astype(np.float32).astype(np.float64)
    return ab, np.sqrt(1.0 + (ab32[:, 0] ** 2 + ab32[:, 1] ** 2))


# ---- exports and refusals ---------------------------------------------------------------------------------------------

def test_beam_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert capi.load().ls_abi_version() == 4      # the new entry points do not step the ABI version
    for s in ("ls_trace_scene_beams", "ls_trace_scene_beams_host", "ls_beam_pattern_rings"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s
    for s in ("ls_debug_beam_ray", "ls_debug_beam_echoes", "ls_debug_beam_model_check"):
        assert s in capi.DEBUG_SYMBOLS and hasattr(lib, s), s
    hdr = _header()
    assert "#define LS_ABI_VERSION 4" in hdr
    assert "#define LS_BEAM_FIRST 1u" in hdr and "#define LS_BEAM_LAST 2u" in hdr and "#define LS_BEAM_STRONGEST 4u" in hdr
    assert (capi.LS_BEAM_FIRST, capi.LS_BEAM_LAST, capi.LS_BEAM_STRONGEST) == (1, 2, 4)
    assert re.search(r"typedef struct ls_beam_model \{ const float \*pattern; .* uint32_t n_samples; .* uint32_t returns; .* uint32_t min_count; "
                     r".* float echo_separation; .* uint32_t reserved\[4\]; .* \} ls_beam_model;", hdr)
    assert ctypes.sizeof(capi.BeamModel) == 40
    assert re.search(r"int ls_trace_scene_beams\(ls_tracer \*tr, void \*hip_stream, const ls_beam_model \*model, void \*d_points32, void \*d_hits, "
                     r"uint32_t \*d_echo, uint32_t \*d_n_points, uint32_t capacity\);", hdr)
    assert re.search(r"int ls_trace_scene_beams_host\(ls_tracer \*tr, const ls_beam_model \*model, void \*points32, void \*hits, uint32_t \*echo, "
                     r"uint32_t \*n_points, uint32_t capacity\);", hdr)
    assert re.search(r"int ls_beam_pattern_rings\(float half_angle_az, float half_angle_el, uint32_t n_rings, uint32_t per_ring, float \*pattern\);", hdr)
    dbg = _header("lidarshooter_hip_debug.h")
    assert re.search(r"int ls_debug_beam_ray\(float sin_theta, float cos_theta, float cos_phi, float sin_phi, const float abk\[3\], float ray8\[8\]\);", dbg)
    assert re.search(r"int ls_debug_beam_echoes\(const ls_beam_model \*model, const float \*r, const uint8_t \*hit, uint32_t \*out /\*.*?\*/, "
                     r"uint32_t \*n_out\);", dbg)
    assert re.search(r"int ls_debug_beam_model_check\(const ls_beam_model \*model, uint32_t shard_rays, uint32_t capacity\);", dbg)


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    m = capi.BeamModel()
    n = ctypes.c_uint32(77)
    buf = np.zeros(64, np.uint8)
    assert L.ls_trace_scene_beams(None, None, ctypes.byref(m), None, None, None, buf.ctypes.data, 4) == INVALID_ARGUMENT
    assert L.ls_trace_scene_beams_host(None, ctypes.byref(m), None, None, None, ctypes.byref(n), 4) == INVALID_ARGUMENT
    assert n.value == 77 and not buf.any()
    assert L.ls_debug_beam_ray(0.5, 0.5, 0.5, 0.5, None, None) == INVALID_ARGUMENT
    assert L.ls_debug_beam_echoes(None, None, None, None, None) == INVALID_ARGUMENT


# ---- the sub-ray of a sample ------------------------------------------------------------------------------------------

def test_beam_ray_equals_the_restatement(capi):
    rng = np.random.default_rng(20251)
    n = 10000
    theta, phi = rng.uniform(0.2, 2.9, n), rng.uniform(-np.pi, np.pi, n)
    st, ct, sp, cp = (x.astype(np.float32) for x in (np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)))
    abk = np.stack([rng.normal(0, 0.01, n), rng.normal(0, 0.01, n), 1.0 + rng.uniform(0, 1e-3, n)], axis=1).astype(np.float32)
    abk[::9, :2] *= F(30.0)          # wide offsets too: the arithmetic does not care
    abk[::13, 0] = 0.0
    abk[::17, 1] = 0.0
    cp[::101], sp[::101] = 1.0, 0.0  # exact axes: zeros among the products
    st[::103], ct[::103] = 1.0, 0.0
    want = restate_beam_rays(st, ct, cp, sp, abk[:, 0], abk[:, 1])
    got = np.stack([capi.beam_ray(st[k], ct[k], cp[k], sp[k], abk[k]) for k in range(n)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(got[:, 0:4] == 0) and np.all(got[:, 7] == F(1e16))
    assert not np.any(np.signbit(got[:, 4:7]) & (got[:, 4:7] == 0))      # no negative zero leaves the library


def test_centre_sample_returns_the_nominal_direction(capi):
    rng = np.random.default_rng(4)
    for theta, phi in zip(rng.uniform(0.2, 2.9, 300), rng.uniform(-np.pi, np.pi, 300)):
        st, ct, sp, cp = F(np.sin(theta)), F(np.cos(theta)), F(np.sin(phi)), F(np.cos(phi))
        r = capi.beam_ray(st, ct, cp, sp, [0.0, 0.0, 1.0])
        assert np.array_equal(r[4:7].view(np.uint32), np.float32([st * cp, st * sp, ct]).view(np.uint32))
    # a nominal component -0 comes out as +0
    r = capi.beam_ray(F(1.0), F(-0.0), F(1.0), F(-0.0), [0.0, 0.0, 1.0])
    assert np.array_equal(r[4:7].view(np.uint32), np.float32([1.0, 0.0, 0.0]).view(np.uint32))


# ---- the echoes of a beam -----------------------------------------------------------------------------------------------

def _beam_case(rng, S, kind):
    """ranges (float32[S]) and hit flags of one beam: clustered surfaces with planted exact ties, random misses"""
    centres = rng.uniform(2.0, 60.0, int(rng.integers(1, 5)))
    r = (centres[rng.integers(0, len(centres), S)] + rng.normal(0, 0.03, S)).astype(np.float32)
    if S > 1:      # exact ties: the lower sample index leads
        dup = rng.integers(0, S, max(1, S // 4))
        r[dup] = r[(dup + 1) % S]
    if kind == "all_miss":
        hit = np.zeros(S, bool)
    elif kind == "all_hit":
        hit = np.ones(S, bool)
    else:
        hit = rng.random(S) < rng.uniform(0.2, 0.95)
    return r, hit


@pytest.mark.parametrize("separation", [0.0, 0.05, INF])
def test_beam_echoes_equal_the_reduction(capi, separation):
    rng = np.random.default_rng(int(separation * 100) + 77 if separation != INF else 5)
    seen_counts, seen_ties, merged = set(), 0, 0
    for S in range(1, 65):
        cases = [_beam_case(rng, S, kind) for kind in ("all_miss", "all_hit", "random", "random")]
        for min_count in sorted({1, min(2, S), S}):
            for returns in range(1, 8):
                m = capi.BeamModel(np.tile(F([0, 0, 1]), (S, 1)), returns, min_count, separation)
                for r, hit in cases:
                    want = reduce_beam(r, hit, returns, min_count, separation)
                    got = [tuple(int(x) for x in rec) for rec in capi.beam_echoes(m, r, hit)]
                    assert got == want, (S, min_count, returns, r, hit)
                    seen_counts.add(len(got))
                    assert len(got) <= bin(returns).count("1")
                    merged += sum(1 for _, w in got if bin(w & 7).count("1") > 1)
                    hs = r[hit]
                    seen_ties += int(len(np.unique(hs)) < len(hs))
    assert seen_ties > 100 and merged > 100
    assert seen_counts == ({0, 1} if separation == INF else {0, 1, 2, 3})


def test_beam_echoes_by_hand(capi):
    # two surfaces 4 m apart, three and two sub-hits, one miss: FIRST and STRONGEST coincide, LAST is the far one
    r, hit = F([5.0, 9.05, 5.1, 9.0, 5.05, 1.0]), [1, 1, 1, 1, 1, 0]
    m = capi.BeamModel(np.tile(F([0, 0, 1]), (6, 1)), 7, 1, 0.25)
    assert [tuple(x) for x in capi.beam_echoes(m, r, hit)] == [(F(5.0).view(np.uint32), 5 | 3 << 8 | 0 << 16), (F(9.0).view(np.uint32), 2 | 2 << 8 | 3 << 16)]
    m.min_count = 3      # the far surface is not detectable any more: one record of all three kinds
    assert [tuple(x) for x in capi.beam_echoes(m, r, hit)] == [(F(5.0).view(np.uint32), 7 | 3 << 8)]
    m.min_count, m.echo_separation = 1, 0.0   # every distinct range its own echo; the tie below stays one echo of two
    r[4] = r[0]
    got = capi.beam_echoes(m, r, hit)
    assert [tuple(x) for x in got] == [(F(5.0).view(np.uint32), 5 | 2 << 8), (F(9.05).view(np.uint32), 2 | 1 << 8 | 1 << 16)]
    # equal counts: the nearer echo is the strongest
    m.returns = STRONGEST
    assert [tuple(x) for x in capi.beam_echoes(m, F([7.0, 3.0, 7.0, 3.0, 1.0, 1.0]), [1, 1, 1, 1, 0, 0])] == [(F(3.0).view(np.uint32), 4 | 2 << 8 | 1 << 16)]
    for bad in (dict(returns=0), dict(returns=8), dict(min_count=0), dict(min_count=7), dict(echo_separation=-1.0), dict(echo_separation=float("nan"))):
        mm = capi.BeamModel(np.tile(F([0, 0, 1]), (6, 1)), 7, 1, 0.25)
        for k, v in bad.items():
            setattr(mm, k, v)
        with pytest.raises(capi.LidarShooterHipError):
            capi.beam_echoes(mm, r, hit)


# ---- the ring pattern -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("half_az,half_el,n_rings,per_ring", [(0.01, 0.01, 1, 4), (0.0015, 0.0008, 2, 6), (0.02, 0.005, 3, 21), (0.003, 0.003, 7, 9),
                                                              (0.01, 0.0, 1, 63), (0.5, 0.25, 9, 7)])
def test_pattern_rings_equal_float64(capi, half_az, half_el, n_rings, per_ring):
    """every entry within 1 float32 ulp of the float64 evaluation: one rounding of a double result whose libm sin / cos / sqrt may
    differ from numpy's in the last double bit; sample 0 exactly (0, 0, 1)"""
    got = capi.beam_pattern_rings(half_az, half_el, n_rings, per_ring)
    S = 1 + n_rings * per_ring
    assert got.shape == (S, 3) and got.dtype == np.float32
    assert np.array_equal(got[0].view(np.uint32), F([0, 0, 1]).view(np.uint32))
    ab, k = rings_f64(half_az, half_el, n_rings, per_ring)
    ref = np.concatenate([ab, k[:, None]], axis=1)
    ref32 = ref.astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(ref32), np.abs(got)))
    assert np.all(np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= ulp)
    # k from the ROUNDED a and b: within an ulp of the float64 value of the entries the library returned
    g = got.astype(np.float64)
    kk = np.sqrt(1.0 + (g[:, 0] ** 2 + g[:, 1] ** 2)).astype(np.float32)
    assert np.all(np.abs(got[:, 2].astype(np.float64) - kk.astype(np.float64)) <= np.spacing(kk))
    assert np.all(got[:, 2] >= 1.0) and np.all(np.hypot(got[1:, 0] / max(half_az, 1e-30), got[1:, 1] / max(half_el, 1e-30)) <= 1.0 + 1e-6)


def test_pattern_rings_refuses_bad_input(capi):
    L = capi.load()
    f32p = ctypes.POINTER(ctypes.c_float)
    out = np.full((80, 3), 7.0, np.float32)
    dst = out.ctypes.data_as(f32p)
    assert L.ls_beam_pattern_rings(0.01, 0.01, 7, 9, dst) == 0 and np.array_equal(out[0], F([0, 0, 1])) and np.all(out[64:] == 7.0)   # S = 64
    assert L.ls_beam_pattern_rings(0.01, 0.01, 0, 0, dst) == 0 and L.ls_beam_pattern_rings(0.01, 0.01, 0, 9, dst) == 0              # S = 1
    out[:] = 7.0
    for n_rings, per_ring in ((8, 8), (1, 64), (64, 1), (3, 22), (0xFFFFFFFF, 0xFFFFFFFF), (0x10000, 0x10000)):
        assert L.ls_beam_pattern_rings(0.01, 0.01, n_rings, per_ring, dst) == INVALID_ARGUMENT
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.ls_beam_pattern_rings(bad, 0.01, 1, 4, dst) == INVALID_ARGUMENT and L.ls_beam_pattern_rings(0.01, bad, 1, 4, dst) == INVALID_ARGUMENT
    assert L.ls_beam_pattern_rings(0.01, 0.01, 1, 4, None) == INVALID_ARGUMENT
    assert np.all(out == 7.0)      # a refusal writes nothing
    with pytest.raises(capi.LidarShooterHipError):
        capi.beam_pattern_rings(0.01, 0.01, 8, 8)


# ---- the refusals of a model --------------------------------------------------------------------------------------------

def test_every_refusal_of_a_model(capi):
    L = capi.load()
    rays = 32 * 150
    pat = capi.beam_pattern_rings(0.01, 0.01, 1, 4)

    def check(m, n=rays, capacity=None):
        cap = m.n_returns * n if capacity is None else capacity
        return L.ls_debug_beam_model_check(ctypes.byref(m) if m is not None else None, n, cap)

    def model(**kw):
        m = capi.BeamModel(pat, 7, 2, 0.25)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    assert check(model()) == 0
    assert check(model(echo_separation=INF)) == 0 and check(model(echo_separation=0.0)) == 0 and check(model(min_count=5)) == 0
    assert L.ls_debug_beam_model_check(None, rays, 3 * rays) == INVALID_ARGUMENT                      # a NULL model
    m = model()
    m.pattern = None
    assert check(m) == INVALID_ARGUMENT                                                                # a NULL pattern
    assert check(model(n_samples=0)) == INVALID_ARGUMENT
    big = capi.BeamModel(np.tile(F([0, 0, 1]), (65, 1)), 1, 1, 0.0)
    assert check(big) == INVALID_ARGUMENT                                                              # S = 65
    big.n_samples = 64
    assert check(big) == 0
    for returns in (0, 8, 9, 0x80000001, 0xFFFFFFFF):                                                  # no bit, unknown bits
        assert check(model(returns=returns), capacity=3 * rays) == INVALID_ARGUMENT
    assert check(model(min_count=0)) == INVALID_ARGUMENT and check(model(min_count=6)) == INVALID_ARGUMENT
    assert check(model(echo_separation=float("nan"))) == INVALID_ARGUMENT and check(model(echo_separation=-1e-9)) == INVALID_ARGUMENT
    assert check(model(echo_separation=-INF)) == INVALID_ARGUMENT
    for s in (0, 2, 4):                                                                                # the pattern's entries
        for col in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                p = pat.copy()
                p[s, col] = bad
                assert check(capi.BeamModel(p, 7, 2, 0.25)) == INVALID_ARGUMENT
        for bad in (0.0, -0.0, -1.0):
            p = pat.copy()
            p[s, 2] = bad
            assert check(capi.BeamModel(p, 7, 2, 0.25)) == INVALID_ARGUMENT
    p = pat.copy()
    p[3] = (-0.3, 0.2, 1e-30)                                                                          # (any finite offsets and positive k pass)
    assert check(capi.BeamModel(p, 7, 2, 0.25)) == 0
    for i in range(4):                                                                                 # the reserved words
        m = model()
        m.reserved[i] = 1
        assert check(m) == INVALID_ARGUMENT
    for returns, K in ((1, 1), (2, 1), (4, 1), (3, 2), (5, 2), (6, 2), (7, 3)):                        # the capacity: K x the shard's rays
        assert check(model(returns=returns), capacity=K * rays) == 0
        assert check(model(returns=returns), capacity=K * rays - 1) == INVALID_ARGUMENT
    # more than 2^27 sub-rays: out of range once everything else is in order, invalid argument otherwise
    n = (1 << 27) // 5 + 1
    assert check(model(returns=1), n=n - 1) == 0 and check(model(returns=1), n=n) == OUT_OF_RANGE
    assert check(model(returns=1), n=n, capacity=n - 1) == INVALID_ARGUMENT
    assert check(big, n=(1 << 21) + 1) == OUT_OF_RANGE and check(big, n=1 << 21) == 0
    assert check(model(returns=7), n=0xFFFFFFFF, capacity=0xFFFFFFFF) == INVALID_ARGUMENT              # 3 x 2^32 does not wrap round
