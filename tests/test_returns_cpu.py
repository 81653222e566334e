"""ls_apply_return_model / ls_apply_return_model_host without a device: the symbols, the layout of ls_return_model, the refusals
that come before any device call, Philox4x32-10 against known answers, and the library's return model (ls_debug_return_model,
the host compilation of what k_returns_eval runs per record) against a restatement written here -- Python-integer Philox,
np.float32 scalar operations in the stated order -- bit for bit; then the statistics of its noise and drop-out."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

INVALID_ARGUMENT = -2
M32 = 0xFFFFFFFF
F = np.float32


def _header(name="lidarshooter_hip.h"):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", name)).read())


# ---- the restatement (shared with test_gpu_returns.py) ----------------------------------------------------------------

def philox4x32(ctr, key):
    """Philox4x32-10 from its definition, on Python integers"""
    c0, c1, c2, c3 = (int(x) for x in ctr)
    k0, k1 = (int(x) for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def restate(m, ray, frame, t, length, cos_inc, rho):
    """steps 2-8 of ls_apply_return_model in np.float32 scalars, one rounding per operation -> (kept, t', I)"""
    with np.errstate(all="ignore"):
        t, length, cos_inc, rho = F(t), F(length), F(cos_inc), F(rho)
        r = t * length
        c = F(1)
        if m.flags & 1:
            if m.flags & 2:
                c = -cos_inc if cos_inc < 0 else cos_inc
            else:
                c = cos_inc if cos_inc > 0 else F(0)
        f = F(1)
        r0 = F(m.ref_range)
        if r0 > 0:
            q = r0 / (r if r > r0 else r0)
            f = q * q
        inten = ((F(m.intensity_scale) * rho) * c) * f
        if inten > F(m.intensity_max):
            inten = F(m.intensity_max)
        a = philox4x32((ray, frame, 0, 0), (m.seed, 0))
        b = philox4x32((ray, frame, 1, 0), (m.seed, 0))
        dropped = bool(F(m.dropout) > 0 and F(b[2] >> 8) * F(2.0 ** -24) < F(m.dropout))
        S = sum((w & 0xFFFF) + (w >> 16) for w in (a[0], a[1], a[2], a[3], b[0], b[1]))
        z = F(S - 393210) * F(1.0 / 65536)
        tp = t
        if not (F(m.noise_sigma0) == 0 and F(m.noise_sigma1) == 0):
            sigma = F(m.noise_sigma0) + F(m.noise_sigma1) * r
            tp = t + (sigma * z) / length
        kept = bool(F(m.range_min) <= r and r <= F(m.range_max) and inten >= F(m.intensity_floor) and not dropped and tp > 0)
    return kept, F(tp), F(inten)


def _bits(x):
    return int(np.float32(x).view(np.uint32))


# ---- exports, layout, refusals ----------------------------------------------------------------------------------------

def test_return_model_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert capi.load().ls_abi_version() == 4      # the new entry points do not step the ABI version
    for s in ("ls_apply_return_model", "ls_apply_return_model_host"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s
    for s in ("ls_debug_philox4x32", "ls_debug_return_model"):
        assert s in capi.DEBUG_SYMBOLS and hasattr(lib, s), s
    hdr = _header()
    assert re.search(r"int ls_apply_return_model\(ls_tracer \*tr, void \*hip_stream, const ls_return_model \*model, uint32_t frame_index, "
                     r"const void \*d_rays, uint32_t n_rays, const void \*d_hits, const uint32_t \*d_count, uint32_t n, "
                     r"const float \*d_reflectivity, uint32_t n_reflectivity, void \*d_points32, void \*d_hits_out, uint32_t \*d_n_out\);", hdr)
    assert re.search(r"int ls_apply_return_model_host\(ls_tracer \*tr, const ls_return_model \*model, uint32_t frame_index, "
                     r"const void \*rays, uint32_t n_rays, const void \*hits, uint32_t n, const float \*reflectivity, "
                     r"uint32_t n_reflectivity, void \*points32, void \*hits_out, uint32_t \*n_out\);", hdr)
    assert "#define LS_RETURN_LAMBERT 1u" in hdr and "#define LS_RETURN_TWO_SIDED 2u" in hdr
    dbg = _header("lidarshooter_hip_debug.h")
    assert re.search(r"int ls_debug_philox4x32\(const uint32_t ctr\[4\], const uint32_t key\[2\], uint32_t out\[4\]\);", dbg)
    assert re.search(r"int ls_debug_return_model\(const ls_return_model \*m, uint32_t ray, uint32_t frame_index, float t, float len, "
                     r"float cos_inc, float rho, float \*t_out, float \*intensity\);", dbg)


def test_model_layout(capi):
    M = capi.ReturnModel
    assert ctypes.sizeof(M) == 64
    names = ["range_min", "range_max", "intensity_scale", "ref_range", "intensity_floor", "intensity_max", "noise_sigma0", "noise_sigma1",
             "dropout", "seed", "flags", "reserved"]
    assert [getattr(M, k).offset for k in names] == [4 * i for i in range(12)]
    assert M.reserved.size == 20 and (capi.LS_RETURN_LAMBERT, capi.LS_RETURN_TWO_SIDED) == (1, 2)
    # the header declares the fields in that order: nine floats, seed, flags, five reserved words
    body = re.search(r"typedef struct ls_return_model \{(.*?)\} ls_return_model;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    decl = [d.strip() for d in body.split(";") if d.strip()]
    assert decl == ["float range_min, range_max", "float intensity_scale", "float ref_range", "float intensity_floor", "float intensity_max",
                    "float noise_sigma0, noise_sigma1", "float dropout", "uint32_t seed", "uint32_t flags", "uint32_t reserved[5]"]
    # and the library reads them where the binding puts them: each field's effect shows in ls_debug_return_model
    m = M()
    assert capi.return_model(m, 1, 0, 10.0, 1.0, 0.5, 1.0) == (True, F(10.0), F(64.0))
    assert capi.return_model(M(range_min=10.5), 1, 0, 10.0, 1.0, 0.5, 1.0)[0] is False
    assert capi.return_model(M(range_max=9.5), 1, 0, 10.0, 1.0, 0.5, 1.0)[0] is False
    assert capi.return_model(M(intensity_scale=3.0), 1, 0, 10.0, 1.0, 0.5, 1.0)[2] == F(3.0)
    assert capi.return_model(M(ref_range=5.0), 1, 0, 10.0, 1.0, 0.5, 1.0)[2] == F(16.0)
    assert capi.return_model(M(intensity_floor=65.0), 1, 0, 10.0, 1.0, 0.5, 1.0)[0] is False
    assert capi.return_model(M(intensity_max=7.0), 1, 0, 10.0, 1.0, 0.5, 1.0)[2] == F(7.0)
    assert capi.return_model(M(noise_sigma0=0.5), 1, 0, 10.0, 1.0, 0.5, 1.0)[1] != F(10.0)
    assert capi.return_model(M(noise_sigma1=0.05), 1, 0, 10.0, 1.0, 0.5, 1.0)[1] != F(10.0)
    assert capi.return_model(M(dropout=1.0), 1, 0, 10.0, 1.0, 0.5, 1.0)[0] is False
    assert capi.return_model(M(noise_sigma0=0.5, seed=1), 1, 0, 10.0, 1.0, 0.5, 1.0)[1] != capi.return_model(M(noise_sigma0=0.5), 1, 0, 10.0, 1.0, 0.5, 1.0)[1]
    assert capi.return_model(M(flags=1), 1, 0, 10.0, 1.0, 0.5, 1.0)[2] == F(32.0)


def bad_models(capi):
    """every model the entry points refuse (shared with test_gpu_returns.py)"""
    M = capi.ReturnModel
    nan, inf = float("nan"), float("inf")
    out = [(f"NaN {k}", M(**{k: nan})) for k in ("range_min", "range_max", "intensity_scale", "ref_range", "intensity_floor", "intensity_max",
                                                   "noise_sigma0", "noise_sigma1", "dropout")]
    out += [("range_min > range_max", M(range_min=5.0, range_max=4.0)), ("range_min = inf > range_max", M(range_min=inf, range_max=100.0))]
    out += [(f"negative {k}", M(**{k: -1e-3})) for k in ("intensity_scale", "intensity_floor", "noise_sigma0", "noise_sigma1", "ref_range", "range_min")]
    out += [("dropout < 0", M(dropout=-1e-6)), ("dropout > 1", M(dropout=1.0 + 2.0 ** -23)), ("unknown flag", M(flags=4)),
            ("unknown high flag", M(flags=0x80000001))]
    for i in range(5):
        m = M()
        m.reserved[i] = 1
        out.append((f"reserved[{i}]", m))
    return out


def test_refusals_without_a_device(capi):
    L = capi.load()
    buf = (ctypes.c_uint8 * 64)(*([0xAB] * 64))
    n_out = ctypes.c_uint32(0xABABABAB)
    good = capi.ReturnModel()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    # a NULL handle, whatever the rest
    for model in (ctypes.byref(good), None):
        assert L.ls_apply_return_model(None, None, model, 0, None, 0, buf, None, 1, None, 0, buf, buf, ctypes.cast(buf, ctypes.c_void_p)) == INVALID_ARGUMENT
        assert L.ls_apply_return_model_host(None, model, 0, None, 0, buf, 1, None, 0, buf, buf, ctypes.byref(n_out)) == INVALID_ARGUMENT
    assert L.ls_apply_return_model(None, None, ctypes.byref(good), 0, None, 0, None, None, 0, None, 0, None, None, None) == INVALID_ARGUMENT
    for name, m in bad_models(capi):
        assert L.ls_apply_return_model_host(None, ctypes.byref(m), 0, None, 0, buf, 1, None, 0, buf, buf, ctypes.byref(n_out)) == INVALID_ARGUMENT, name
    assert bytes(buf) == b"\xab" * 64 and n_out.value == 0xABABABAB   # nothing written
    # the model check itself, which needs no handle: ls_debug_return_model refuses what the entry points refuse
    f32p = ctypes.POINTER(ctypes.c_float)
    t_out, inten = ctypes.c_float(-7.0), ctypes.c_float(-7.0)
    assert L.ls_debug_return_model(ctypes.byref(good), 0, 0, 1.0, 1.0, 1.0, 1.0, ctypes.byref(t_out), ctypes.byref(inten)) == 1
    t_out.value = inten.value = -7.0
    for name, m in bad_models(capi):
        assert L.ls_debug_return_model(ctypes.byref(m), 0, 0, 1.0, 1.0, 1.0, 1.0, ctypes.byref(t_out), ctypes.byref(inten)) == INVALID_ARGUMENT, name
    assert L.ls_debug_return_model(None, 0, 0, 1.0, 1.0, 1.0, 1.0, ctypes.byref(t_out), ctypes.byref(inten)) == INVALID_ARGUMENT
    assert L.ls_debug_return_model(ctypes.byref(good), 0, 0, 1.0, 1.0, 1.0, 1.0, None, ctypes.byref(inten)) == INVALID_ARGUMENT
    assert L.ls_debug_return_model(ctypes.byref(good), 0, 0, 1.0, 1.0, 1.0, 1.0, ctypes.byref(t_out), None) == INVALID_ARGUMENT
    assert t_out.value == -7.0 and inten.value == -7.0
    assert L.ls_debug_philox4x32(None, ctypes.cast(buf, u32p), ctypes.cast(buf, u32p)) == INVALID_ARGUMENT
    assert L.ls_debug_philox4x32(ctypes.cast(buf, u32p), None, ctypes.cast(buf, u32p)) == INVALID_ARGUMENT
    assert L.ls_debug_philox4x32(ctypes.cast(buf, u32p), ctypes.cast(buf, u32p), None) == INVALID_ARGUMENT
    assert bytes(buf) == b"\xab" * 64
    # the limits themselves are fine
    M = capi.ReturnModel
    for m in (M(dropout=0.0), M(dropout=1.0), M(range_min=3.0, range_max=3.0), M(range_min=0.0, range_max=0.0), M(flags=2), M(flags=3),
              M(intensity_max=0.0), M(intensity_floor=float("inf")), M(intensity_scale=0.0), M(seed=0xFFFFFFFF)):
        assert L.ls_debug_return_model(ctypes.byref(m), 0, 0, 1.0, 1.0, 1.0, 1.0, ctypes.byref(t_out), ctypes.byref(inten)) in (0, 1)


# ---- Philox -----------------------------------------------------------------------------------------------------------

KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def test_philox_known_answers(capi):
    for ctr, key, want in KAT:
        assert tuple(int(x) for x in capi.philox4x32(ctr, key)) == want
        assert philox4x32(ctr, key) == want       # the restatement's generator too
    rng = np.random.default_rng(1)
    for _ in range(200):
        ctr, key = rng.integers(0, 2 ** 32, 4, dtype=np.uint64), rng.integers(0, 2 ** 32, 2, dtype=np.uint64)
        assert tuple(int(x) for x in capi.philox4x32(ctr, key)) == philox4x32(ctr, key)


# ---- the model against its restatement ----------------------------------------------------------------------------------

def _same(capi, m, ray, frame, t, length, cos_inc, rho):
    got = capi.return_model(m, ray, frame, t, length, cos_inc, rho)
    want = restate(m, ray, frame, t, length, cos_inc, rho)
    assert got[0] == want[0] and _bits(got[1]) == _bits(want[1]) and _bits(got[2]) == _bits(want[2]), \
        ([(k, getattr(m, k)) for k, _ in m._fields_[:11]], ray, frame, t, length, cos_inc, rho, got, want)
    return got


def test_model_is_the_restatement_bit_for_bit(capi):
    M = capi.ReturnModel
    rng = np.random.default_rng(2024)
    kept = lost = 0
    for i in range(4000):
        flags = i % 4
        t = F(10 ** rng.uniform(-1, 2))
        length = F(1.0) if i % 3 == 0 else F(10 ** rng.uniform(-1, 1))
        cos_inc = F(rng.uniform(-1, 1))
        rho = F(rng.uniform(0.05, 1.5))
        r = float(t * length)
        m = M(flags=flags, seed=int(rng.integers(0, 2 ** 32)), intensity_scale=float(F(rng.uniform(1, 200))))
        if i % 2:
            m.ref_range = float(F(r * rng.uniform(0.2, 3.0)))            # on both sides of r
        if i % 5 == 1:
            m.range_min, m.range_max = float(F(r * rng.uniform(0.5, 1.2))), float(F(r * rng.uniform(1.2, 2.0)))   # r on both sides of the lower gate
        elif i % 5 == 2:
            m.range_min, m.range_max = float(F(r * rng.uniform(0.1, 0.5))), float(F(r * rng.uniform(0.8, 1.5)))   # ... of the upper gate
        if i % 7 == 3:
            m.intensity_floor = float(F(rng.uniform(0, 60)))
        if i % 7 == 4:
            m.intensity_max = float(F(rng.uniform(1, 100)))
        if i % 3 != 1:
            m.noise_sigma0 = float(F(rng.uniform(0, 0.05))) if i % 6 < 4 else 0.0
            m.noise_sigma1 = float(F(rng.uniform(0, 0.01))) if i % 4 < 2 else 0.0
        if i % 11 == 5:
            m.noise_sigma0 = float(F(t * length * 0.3))     # t' <= 0 happens
        m.dropout = (0.0, 0.0, 0.3, 1.0, float(F(rng.uniform(0, 1))))[i % 5 if i % 13 else 3]
        got = _same(capi, m, int(rng.integers(0, 2 ** 32)) if i % 9 else i, int(rng.integers(0, 2 ** 32)) if i % 8 else 0, t, length, cos_inc, rho)
        kept += got[0]
        lost += not got[0]
    assert kept > 1000 and lost > 1000

    # r exactly on each gate: kept on it, lost one ulp outside
    for t, length in ((F(10.0), F(1.0)), (F(3.0), F(2.5)), (F(0.7), F(1.3))):
        r = t * length
        up, down = np.nextafter(r, F(np.inf)), np.nextafter(r, F(0))
        for lo, hi, want in ((r, np.inf, True), (0.0, r, True), (r, r, True), (up, np.inf, False), (0.0, down, False)):
            got = _same(capi, M(range_min=float(lo), range_max=float(hi)), 3, 1, t, length, 0.5, 1.0)
            assert got[0] is want, (t, length, lo, hi)
    # intensity exactly at the floor (kept), a floor one ulp above (lost); exactly at the maximum (unchanged), one ulp below (clamped)
    for flags, ref in ((0, 0.0), (1, 0.0), (3, 4.0), (1, 4.0)):
        base = M(flags=flags, ref_range=ref, intensity_scale=77.0)
        _, _, inten = _same(capi, base, 9, 2, 7.5, 1.25, -0.625 if flags == 3 else 0.625, 0.3)
        assert inten > 0
        for floor, want in ((inten, True), (np.nextafter(inten, F(np.inf)), False)):
            m = M(flags=flags, ref_range=ref, intensity_scale=77.0, intensity_floor=float(floor))
            assert _same(capi, m, 9, 2, 7.5, 1.25, -0.625 if flags == 3 else 0.625, 0.3)[0] is want
        for mx in (inten, np.nextafter(inten, F(0))):
            m = M(flags=flags, ref_range=ref, intensity_scale=77.0, intensity_max=float(mx))
            assert _same(capi, m, 9, 2, 7.5, 1.25, -0.625 if flags == 3 else 0.625, 0.3)[2] == mx
    # a negative incidence cosine: nothing with LAMBERT (kept at floor 0, lost at any floor above), its magnitude with TWO_SIDED
    assert _same(capi, M(flags=1), 4, 0, 5.0, 1.0, -0.5, 1.0) == (True, F(5.0), F(0.0))
    assert _same(capi, M(flags=1, intensity_floor=1e-30), 4, 0, 5.0, 1.0, -0.5, 1.0)[0] is False
    assert _same(capi, M(flags=3), 4, 0, 5.0, 1.0, -0.5, 1.0) == (True, F(5.0), F(32.0))
    assert _same(capi, M(flags=2), 4, 0, 5.0, 1.0, -0.5, 1.0) == (True, F(5.0), F(64.0))     # TWO_SIDED alone: no incidence term
    # a NaN reflectivity: a NaN intensity, lost whatever the floor; saturation does not catch it
    for m in (M(), M(intensity_max=10.0), M(flags=1, ref_range=2.0)):
        got = _same(capi, m, 4, 0, 5.0, 1.0, 0.5, float("nan"))
        assert got[0] is False and np.isnan(got[2])
    # sigma 0: t' is t's bits whatever the seed and the frame; dropout 0 keeps, dropout 1 loses, every ray
    for ray in range(300):
        assert _same(capi, M(seed=ray * 7919), ray, ray % 5, 12.5, 1.0, 0.3, 1.0) == (True, F(12.5), F(64.0))
        assert _same(capi, M(dropout=1.0), ray, 0, 12.5, 1.0, 0.3, 1.0)[0] is False


# ---- statistics -------------------------------------------------------------------------------------------------------

def _z(capi, m, n, frame=0):
    """z of rays 0 .. n-1: (t' - t) / sigma with len = 1, sigma1 = 0; with t = 64 and sigma = 1 the sum 64 + z is exact (z lies on
    a 2^-16 grid within +-6, the floats around 64 on a 2^-18 one), so t' - t is z itself"""
    out = np.empty(n)
    kept = np.empty(n, bool)
    for ray in range(n):
        k, tp, _ = capi.return_model(m, ray, frame, 64.0, 1.0, 1.0, 1.0)
        out[ray], kept[ray] = float(tp) - 64.0, k
    return out, kept


def test_noise_and_dropout_statistics(capi):
    """100 000 consecutive rays of one frame.  Standard errors at n = 100 000: the mean of unit draws n^-1/2 = 0.0032, their
    standard deviation (2n)^-1/2 = 0.0022, a share of 0.3 (0.21 / n)^1/2 = 0.0014 -- the bounds 0.02, 0.02 and 0.01 are six to
    nine of them wide."""
    n = 100000
    M = capi.ReturnModel
    z, kept = _z(capi, M(noise_sigma0=1.0, seed=12345), n)
    print("z: mean", z.mean(), "std", z.std(), "min", z.min(), "max", z.max())
    assert np.all(kept)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    assert np.abs(z).max() <= 6.0 and np.abs(z).max() > 3.5
    assert np.all(z * 2 ** 16 == np.round(z * 2 ** 16))
    _, kept = _z(capi, M(dropout=0.3, seed=12345), n)
    share = 1.0 - kept.mean()
    print("lost share at dropout 0.3:", share)
    assert abs(share - 0.3) < 0.01
    # another seed, another frame: other noise (equal only by the chance of the 2^-16 grid: ~1e-5 of the draws)
    few = 20000
    z_seed, _ = _z(capi, M(noise_sigma0=1.0, seed=12346), few)
    z_frame, _ = _z(capi, M(noise_sigma0=1.0, seed=12345), few, frame=1)
    assert np.mean(z_seed != z[:few]) > 0.99 and np.mean(z_frame != z[:few]) > 0.99 and np.mean(z_frame != z_seed) > 0.99
    z_again, _ = _z(capi, M(noise_sigma0=1.0, seed=12345), 2000)
    assert np.array_equal(z_again, z[:2000])
