"""ls_trace_scene_beams_sweep / ls_trace_scene_beams_sweep_host / ls_beam_weights_gaussian without a device: the symbols, the
refusal of a NULL handle, the sub-ray of a sample under a pose (ls_debug_beam_sweep_ray, the host compilation of what
k_beam_sweep_rays runs) against the two restatements of the calls it joins, the weighted echoes of a beam
(ls_debug_beam_echoes_weighted: what k_beam_reduce_weighted runs) against a plain Python reduction written here -- bit for bit --,
the Gaussian weights against numpy float64, and every refusal of a model or a weight through ls_debug_beam_sweep_check."""
import ctypes
import re

import numpy as np
import pytest

from test_beams_cpu import FIRST, LAST, STRONGEST, INF, INVALID_ARGUMENT, OUT_OF_RANGE, _beam_case, _header, reduce_beam, restate_beam_rays
from test_sweep_cpu import IDENTITY_POSE, restate_rays

F = np.float32
U32P = ctypes.POINTER(ctypes.c_uint32)


# ---- the restatements (shared with test_gpu_beams_sweep.py) ---------------------------------------------------------------

def restate_beam_sweep_rays(st, ct, cphi, sphi, a, b, pose):
    """the sub-ray records, float32 (n, 8): restate_beam_rays' direction carried through the pose records (n, 12) by restate_rays"""
    return restate_rays(restate_beam_rays(st, ct, cphi, sphi, a, b)[:, 4:7], pose)


def reduce_beam_weighted(r, hit, returns, min_count, separation, weights=None, min_weight=0):
    """the returns of one beam: [(bits of r_e, echo word, W_e)] in ascending range.  The echoes as reduce_beam forms them; the
    strength of an echo is the sum of its members' weights (None: 1 each); detectable with at least min_count members AND a
    strength of at least min_weight; FIRST the nearest, LAST the farthest, STRONGEST the largest strength (the nearer of equals)"""
    r = np.asarray(r, np.float32)
    w = [1] * len(r) if weights is None else [int(x) for x in weights]
    order = sorted((s for s in range(len(r)) if hit[s]), key=lambda s: (float(r[s]), s))
    echoes = []                                                   # [nearest sample, members, strength]
    with np.errstate(invalid="ignore"):
        for j, s in enumerate(order):
            if j == 0 or F(r[s] - r[order[j - 1]]) > F(separation):
                echoes.append([s, 0, 0])
            echoes[-1][1] += 1
            echoes[-1][2] += w[s]
    det = [e for e in echoes if e[1] >= min_count and e[2] >= min_weight]
    if not det:
        return []
    best = det[0]
    for e in det[1:]:
        if e[2] > best[2]:
            best = e
    out = []
    for e in det:
        kinds = (FIRST if e is det[0] else 0) | (LAST if e is det[-1] else 0) | (STRONGEST if e is best else 0)
        kinds &= returns
        if kinds:
            out.append((int(r[e[0]].view(np.uint32)), kinds | (e[1] << 8) | (e[0] << 16), e[2]))
    return out


def _got(capi, m, weights, min_weight, r, hit):
    return [tuple(int(x) for x in rec) for rec in capi.beam_echoes_weighted(m, weights, min_weight, r, hit)]


def _model(capi, S, returns, min_count, separation):
    return capi.BeamModel(np.tile(F([0, 0, 1]), (S, 1)), returns, min_count, separation)


# ---- exports and refusals ---------------------------------------------------------------------------------------------

def test_beams_sweep_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert capi.load().ls_abi_version() == 4      # the new entry points do not step the ABI version
    for s in ("ls_trace_scene_beams_sweep", "ls_trace_scene_beams_sweep_host", "ls_beam_weights_gaussian"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s
    for s in ("ls_debug_beam_sweep_ray", "ls_debug_beam_echoes_weighted", "ls_debug_beam_sweep_check"):
        assert s in capi.DEBUG_SYMBOLS and hasattr(lib, s), s
    hdr = _header()
    assert re.search(r"int ls_trace_scene_beams_sweep\(ls_tracer \*tr, void \*hip_stream, const ls_beam_model \*model, const uint32_t \*weights, "
                     r"uint32_t min_weight, const float \*d_col_pose, uint32_t n_cols, uint32_t flags, void \*d_points32, void \*d_hits, "
                     r"uint32_t \*d_echo, uint32_t \*d_n_points, uint32_t capacity\);", hdr)
    assert re.search(r"int ls_trace_scene_beams_sweep_host\(ls_tracer \*tr, const ls_beam_model \*model, const uint32_t \*weights, "
                     r"uint32_t min_weight, const float \*col_pose, uint32_t n_cols, uint32_t flags, void \*points32, void \*hits, uint32_t \*echo, "
                     r"uint32_t \*n_points, uint32_t capacity\);", hdr)
    assert re.search(r"int ls_beam_weights_gaussian\(const float \*pattern, uint32_t n_samples, float sigma_az, float sigma_el, uint32_t \*weights\);", hdr)
    assert "Not offered: per-sample weights" not in hdr and "ls_trace_scene_beams_sweep below" in hdr   # the beams' comment points here now
    dbg = _header("lidarshooter_hip_debug.h")
    assert re.search(r"int ls_debug_beam_sweep_ray\(float sin_theta, float cos_theta, float cos_phi, float sin_phi, const float abk\[3\], "
                     r"const float pose12\[12\], float ray8\[8\]\);", dbg)
    assert re.search(r"int ls_debug_beam_echoes_weighted\(const ls_beam_model \*model, const uint32_t \*weights, uint32_t min_weight, const float \*r, "
                     r"const uint8_t \*hit, uint32_t \*out /\*.*?\*/, uint32_t \*n_out\);", dbg)
    assert re.search(r"int ls_debug_beam_sweep_check\(const ls_beam_model \*model, const uint32_t \*weights, uint32_t shard_rays, uint32_t capacity\);", dbg)


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    m = capi.BeamModel()
    n = ctypes.c_uint32(77)
    buf = np.zeros(64, np.uint8)
    pose = np.tile(IDENTITY_POSE, (4, 1))
    assert L.ls_trace_scene_beams_sweep(None, None, ctypes.byref(m), None, 0, None, 0, 0, None, None, None, buf.ctypes.data, 4) == INVALID_ARGUMENT
    assert L.ls_trace_scene_beams_sweep_host(None, ctypes.byref(m), None, 0, pose.ctypes.data, 4, 0, None, None, None, ctypes.byref(n), 4) == INVALID_ARGUMENT
    assert n.value == 77 and not buf.any()
    assert L.ls_debug_beam_sweep_ray(0.5, 0.5, 0.5, 0.5, None, None, None) == INVALID_ARGUMENT
    assert L.ls_debug_beam_echoes_weighted(None, None, 0, None, None, None, None) == INVALID_ARGUMENT


# ---- the sub-ray of a sample under a pose -------------------------------------------------------------------------------

def _ray_cases(n, seed):
    rng = np.random.default_rng(seed)
    theta, phi = rng.uniform(0.2, 2.9, n), rng.uniform(-np.pi, np.pi, n)
    st, ct, sp, cp = (x.astype(np.float32) for x in (np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)))
    abk = np.stack([rng.normal(0, 0.01, n), rng.normal(0, 0.01, n), 1.0 + rng.uniform(0, 1e-3, n)], axis=1).astype(np.float32)
    abk[::13, 0] = 0.0
    abk[::17, 1] = 0.0
    cp[::101], sp[::101] = 1.0, 0.0  # exact axes: zeros among the products
    st[::103], ct[::103] = 1.0, 0.0
    pose = rng.normal(0, 1, (n, 12)).astype(np.float32)          # any matrix: the arithmetic does not care
    pose[::7] = IDENTITY_POSE
    pose[::11, 0:3] = 0.0                                        # zeros among the products here too
    return st, ct, sp, cp, abk, pose


def test_beam_sweep_ray_equals_the_two_restatements_composed(capi):
    st, ct, sp, cp, abk, pose = _ray_cases(6000, 20252)
    want = restate_beam_sweep_rays(st, ct, cp, sp, abk[:, 0], abk[:, 1], pose)
    got = np.stack([capi.beam_sweep_ray(st[k], ct[k], cp[k], sp[k], abk[k], pose[k]) for k in range(len(st))])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, 0:3].view(np.uint32), pose[:, [3, 7, 11]].view(np.uint32)) and np.all(got[:, 3] == 0) and np.all(got[:, 7] == F(1e16))


def test_identity_pose_gives_the_beam_ray_and_the_centre_sample_the_sweep_ray(capi):
    st, ct, sp, cp, abk, pose = _ray_cases(1500, 9)
    for k in range(len(st)):
        got = capi.beam_sweep_ray(st[k], ct[k], cp[k], sp[k], abk[k], IDENTITY_POSE)
        assert np.array_equal(got.view(np.uint32), capi.beam_ray(st[k], ct[k], cp[k], sp[k], abk[k]).view(np.uint32))
    # the centre sample: the nominal direction through the pose -- the beam's step from a component -0 to +0 included, which the
    # sweep's sequence cannot tell from -0 unless all three products of a row are zeros
    rng = np.random.default_rng(10)
    zeros = 0
    for k in range(len(st)):
        d = np.float32([st[k] * cp[k], st[k] * sp[k], ct[k]])
        zeros += int(np.any(d == 0))
        d = np.where(d == 0, F(0.0), d)
        got = capi.beam_sweep_ray(st[k], ct[k], cp[k], sp[k], [0.0, 0.0, 1.0 + rng.uniform(0, 1e-3)], pose[k])
        assert np.array_equal(got.view(np.uint32), capi.sweep_ray(d, pose[k]).view(np.uint32))
    assert zeros > 10


# ---- the weighted echoes of a beam --------------------------------------------------------------------------------------

@pytest.mark.parametrize("separation", [0.0, 0.05, INF])
def test_weighted_echoes_equal_the_reduction(capi, separation):
    rng = np.random.default_rng(int(separation * 100) + 311 if separation != INF else 6)
    seen_counts, moved, thresholded = set(), 0, 0
    for S in (1, 2, 3, 5, 8, 33, 64):
        cases = [_beam_case(rng, S, kind) for kind in ("all_miss", "all_hit", "random", "random", "random")]
        for weights in (None, rng.integers(1, 65536, S).astype(np.uint32), np.full(S, 65535, np.uint32)):
            total = S if weights is None else int(weights.astype(np.int64).sum())
            for min_weight in (0, total // 3, total + 1):
                for min_count in sorted({1, min(2, S)}):
                    for returns in range(1, 8):
                        m = _model(capi, S, returns, min_count, separation)
                        for r, hit in cases:
                            want = reduce_beam_weighted(r, hit, returns, min_count, separation, weights, min_weight)
                            got = _got(capi, m, weights, min_weight, r, hit)
                            assert got == want, (S, weights, min_weight, min_count, returns, r, hit)
                            seen_counts.add(len(got))
                            assert all(1 <= W <= total for _, _, W in got)
                            if min_weight > total:
                                assert got == []
                            plain = reduce_beam(r, hit, returns, min_count, separation)
                            if weights is None and min_weight == 0:      # the first two words are ls_debug_beam_echoes'
                                assert [g[:2] for g in got] == plain == [tuple(int(x) for x in rec) for rec in capi.beam_echoes(m, r, hit)]
                                assert all(W == (w >> 8) & 0x7F for _, w, W in got)
                            elif min_weight == 0:
                                moved += [g[:2] for g in got] != plain
                            else:
                                thresholded += len(got) < len(plain)
    # not vacuous: the threshold removes echoes, and where a beam can have several echoes the weights move a selection
    assert thresholded > 0 and (moved > 0 or separation == INF)
    assert seen_counts == ({0, 1} if separation == INF else {0, 1, 2, 3})


def test_weighted_echoes_by_hand(capi):
    bits = lambda x: int(F(x).view(np.uint32))   # noqa: E731
    # a near surface under three weak edge samples, a far one under the bright centre and a neighbour: STRONGEST by weight is not the
    # echo with the most members
    r, hit = F([9.0, 5.0, 5.05, 5.1, 9.05, 1.0]), [1, 1, 1, 1, 1, 0]
    w = np.uint32([65535, 9000, 9000, 9000, 20000, 30000])
    m = _model(capi, 6, 7, 1, 0.25)
    assert _got(capi, m, w, 0, r, hit) == [(bits(5.0), FIRST | 3 << 8 | 1 << 16, 27000), (bits(9.0), LAST | STRONGEST | 2 << 8 | 0 << 16, 85535)]
    assert _got(capi, m, None, 0, r, hit) == [(bits(5.0), FIRST | STRONGEST | 3 << 8 | 1 << 16, 3), (bits(9.0), LAST | 2 << 8, 2)]
    # the missed sample's weight counts nowhere: W_total is not a bound that a beam reaches without it
    assert sum(W for _, _, W in _got(capi, m, w, 0, r, hit)) == int(w.sum()) - 30000
    # equal strengths: the nearer echo is the strongest, whatever the member counts
    m.returns = STRONGEST
    assert _got(capi, m, np.uint32([10, 40, 10, 10, 10, 1]), 0, F([7.0, 3.0, 7.0, 7.05, 7.1, 1.0]), [1, 1, 1, 1, 1, 0]) == \
        [(bits(3.0), STRONGEST | 1 << 8 | 1 << 16, 40)]
    # an echo that min_count admits and min_weight removes: FIRST moves on to the next one
    m.returns, m.min_count = 7, 2
    r, hit = F([4.0, 4.05, 8.0, 8.05, 12.0, 12.05]), [1] * 6
    w = np.uint32([100, 100, 5000, 5000, 3000, 3000])
    assert _got(capi, m, w, 0, r, hit) == [(bits(4.0), FIRST | 2 << 8, 200), (bits(8.0), STRONGEST | 2 << 8 | 2 << 16, 10000),
                                            (bits(12.0), LAST | 2 << 8 | 4 << 16, 6000)]
    assert _got(capi, m, w, 201, r, hit) == [(bits(8.0), FIRST | STRONGEST | 2 << 8 | 2 << 16, 10000), (bits(12.0), LAST | 2 << 8 | 4 << 16, 6000)]
    assert _got(capi, m, w, 200, r, hit)[0] == (bits(4.0), FIRST | 2 << 8, 200)                     # (>=: the threshold itself passes)
    assert _got(capi, m, w, 6001, r, hit) == [(bits(8.0), 7 | 2 << 8 | 2 << 16, 10000)]
    assert _got(capi, m, w, 10001, r, hit) == []
    # sixty-four samples of the largest weight: the strength is exact at its upper bound
    m64 = _model(capi, 64, 7, 1, INF)
    assert _got(capi, m64, np.full(64, 65535, np.uint32), 64 * 65535, np.linspace(3, 4, 64).astype(np.float32), [1] * 64) == \
        [(bits(3.0), 7 | 64 << 8, 64 * 65535)]
    for bad in (np.uint32([0, 1, 1, 1, 1, 1]), np.uint32([1, 1, 1, 1, 1, 65536]), np.uint32([1, 1, 0xFFFFFFFF, 1, 1, 1])):
        with pytest.raises(capi.LidarShooterHipError):
            capi.beam_echoes_weighted(m, bad, 0, r, hit)


# ---- the Gaussian weights -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rings,per_ring,sigma_az,sigma_el", [(1, 4, 0.01, 0.01), (2, 6, 0.0007, 0.0011), (7, 9, 0.004, 0.02), (3, 21, 1e-4, 1e-4)])
def test_weights_gaussian_equal_float64(capi, n_rings, per_ring, sigma_az, sigma_el):
    """one rounding of a double result whose libm exp may differ from numpy's in the last double bit: within 1 of the float64
    evaluation, the centre exactly 65535, never below 1"""
    pat = capi.beam_pattern_rings(0.0015, 0.001, n_rings, per_ring)
    got = capi.beam_weights_gaussian(pat, sigma_az, sigma_el)
    p = pat.astype(np.float64)
    ref = 65535.0 * np.exp(-0.5 * ((p[:, 0] / float(F(sigma_az))) ** 2 + (p[:, 1] / float(F(sigma_el))) ** 2))
    want = np.maximum(1, np.round(ref)).astype(np.int64)
    assert got.dtype == np.uint32 and got.shape == (pat.shape[0],)
    assert got[0] == 65535 and np.all(got >= 1) and np.all(got <= 65535)
    assert np.all(np.abs(got.astype(np.int64) - want) <= 1)
    exact = np.abs(ref - np.round(ref)) < 0.49                   # away from a rounding boundary the two agree exactly
    assert np.array_equal(got[exact], want[exact])
    if sigma_az == 1e-4:
        assert np.count_nonzero(got == 1) > 20                    # far tails are clamped to 1, not 0


def test_weights_gaussian_refuses_bad_input(capi):
    L = capi.load()
    f32p = ctypes.POINTER(ctypes.c_float)
    pat = capi.beam_pattern_rings(0.01, 0.01, 7, 9)
    out = np.full(80, 7, np.uint32)
    src, dst = pat.ctypes.data_as(f32p), out.ctypes.data_as(U32P)
    assert L.ls_beam_weights_gaussian(src, 64, 0.01, 0.01, dst) == 0 and out[0] == 65535 and np.all(out[64:] == 7)
    out[:] = 7
    assert L.ls_beam_weights_gaussian(None, 5, 0.01, 0.01, dst) == INVALID_ARGUMENT and L.ls_beam_weights_gaussian(src, 5, 0.01, 0.01, None) == INVALID_ARGUMENT
    assert L.ls_beam_weights_gaussian(src, 0, 0.01, 0.01, dst) == INVALID_ARGUMENT and L.ls_beam_weights_gaussian(src, 65, 0.01, 0.01, dst) == INVALID_ARGUMENT
    for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -0.0, -0.01):
        assert L.ls_beam_weights_gaussian(src, 5, bad, 0.01, dst) == INVALID_ARGUMENT and L.ls_beam_weights_gaussian(src, 5, 0.01, bad, dst) == INVALID_ARGUMENT
    for col in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            p = pat.copy()
            p[3, col] = bad
            assert L.ls_beam_weights_gaussian(p.ctypes.data_as(f32p), 5, 0.01, 0.01, dst) == INVALID_ARGUMENT
            assert L.ls_beam_weights_gaussian(p.ctypes.data_as(f32p), 3, 0.01, 0.01, dst) == 0          # (sample 3 is not among the first three)
            out[:] = 7
    assert np.all(out == 7)      # a refusal writes nothing
    with pytest.raises(capi.LidarShooterHipError):
        capi.beam_weights_gaussian(pat, 0.0, 0.01)


# ---- the refusals of the call ---------------------------------------------------------------------------------------------

def test_every_refusal_of_a_model_or_a_weight(capi):
    L = capi.load()
    rays = 32 * 150
    pat = capi.beam_pattern_rings(0.01, 0.01, 1, 4)
    good_w = np.uint32([65535, 20000, 20000, 9000, 9000])

    def check(m, w=good_w, n=rays, capacity=None):
        cap = m.n_returns * n if capacity is None else capacity
        return L.ls_debug_beam_sweep_check(ctypes.byref(m) if m is not None else None, None if w is None else w.ctypes.data_as(U32P), n, cap)

    def model(**kw):
        m = capi.BeamModel(kw.pop("pattern", pat), 7, 2, 0.25)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    assert check(model()) == 0 and check(model(), None) == 0
    assert check(model(), np.uint32([1, 1, 1, 1, 1])) == 0 and check(model(), np.full(5, 65535, np.uint32)) == 0       # the bounds themselves
    for s in range(5):                                                                                                   # weight 0, weight 65536
        for bad in (0, 65536, 0x10001, 0xFFFFFFFF):
            w = good_w.copy()
            w[s] = bad
            assert check(model(), w) == INVALID_ARGUMENT
    w = np.uint32([1, 1, 1, 1, 1, 0, 65536])                                                                             # only n_samples of them are read
    assert check(model(), w) == 0
    # the model's errors, with good weights, with none and with bad ones
    assert L.ls_debug_beam_sweep_check(None, good_w.ctypes.data_as(U32P), rays, 3 * rays) == INVALID_ARGUMENT
    null_pattern = model()
    null_pattern.pattern = None
    reserved = model()
    reserved.reserved[1] = 1
    nan_entry, zero_k = pat.copy(), pat.copy()
    nan_entry[2, 0], zero_k[4, 2] = np.nan, 0.0
    big = capi.BeamModel(np.tile(F([0, 0, 1]), (65, 1)), 1, 1, 0.0)
    for m in (null_pattern, reserved, model(n_samples=0), big, model(returns=0), model(returns=8), model(min_count=0), model(min_count=6),
              model(echo_separation=float("nan")), model(echo_separation=-1e-9), model(pattern=nan_entry), model(pattern=zero_k)):
        for w in (good_w, None, np.zeros(5, np.uint32)):
            assert check(m, w, capacity=3 * rays) == INVALID_ARGUMENT
    for returns, K in ((1, 1), (2, 1), (4, 1), (3, 2), (5, 2), (6, 2), (7, 3)):                                          # the capacity: K x the shard's rays
        assert check(model(returns=returns), capacity=K * rays) == 0
        assert check(model(returns=returns), capacity=K * rays - 1) == INVALID_ARGUMENT
    # more than 2^27 sub-rays: out of range once the model is in order, as for ls_trace_scene_beams
    n = (1 << 27) // 5 + 1
    assert check(model(returns=1), n=n - 1) == 0 and check(model(returns=1), n=n) == OUT_OF_RANGE
    assert check(model(returns=1), n=n, capacity=n - 1) == INVALID_ARGUMENT
    big.n_samples = 64
    w64 = np.full(64, 3, np.uint32)
    assert check(big, w64, n=(1 << 21) + 1) == OUT_OF_RANGE and check(big, w64, n=1 << 21) == 0
    # with NULL weights the status is ls_debug_beam_model_check's
    for m, nn, cap in ((model(), rays, 3 * rays), (model(), rays, 3 * rays - 1), (model(returns=1), n, n), (model(min_count=0), rays, 3 * rays)):
        assert L.ls_debug_beam_sweep_check(ctypes.byref(m), None, nn, cap) == L.ls_debug_beam_model_check(ctypes.byref(m), nn, cap)
