"""ls_cloud_nearest without a device: the symbols, the descriptor and the records; the check's refusals (there is no GPU where
`-m "not gpu"` runs); the numpy reference (tests/cloud_nearest_reference.py) -- its grid path against its brute force byte for byte, and
the brute force against a float64 nearest neighbour --; the 27-cell claim of csrc/ls_cloud_nearest.h against the compiled sequence
(ls_debug_cloud_cell) on adversarial pairs at seven radii; the domain rule at its edge."""
import ctypes
import os
import re

import numpy as np

import cloud_nearest_reference as ref
from conftest import ROOT

INVALID_ARGUMENT = -2
F = np.float32
RADII = (2.0 ** -20, 0.013, 0.05, 1.0, 3.7, 1000.0, 2.0 ** 20)
U = 2.0 ** -24                                     # the unit roundoff of float32


def hook_cells(capi, radius, pts):
    """ls_debug_cloud_cell -> (cell int32 (n, 3), takes_part bool (n))"""
    p = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = p.shape[0]
    cell, part = np.full((n, 3), 7, np.int32), np.full(n, 7, np.uint8)
    assert capi.load().ls_debug_cloud_cell(float(F(radius)), p.ctypes.data, n, cell.ctypes.data, part.ctypes.data) == 0
    assert np.all(part <= 1)
    return cell, part.astype(bool)


def hook_bucket(capi, cell, log2_buckets):
    c = np.ascontiguousarray(cell, np.int32).reshape(3)
    return int(capi.load().ls_debug_cloud_bucket(c.ctypes.data, log2_buckets))


# ---- the surface -----------------------------------------------------------------------------------------------------------------

def test_symbols_descriptor_and_records(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in ("ls_cloud_nearest", "ls_cloud_nearest_host", "ls_cloud_nearest_check"):
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    for s in ("ls_debug_cloud_cell", "ls_debug_cloud_bucket"):
        assert s in capi.DEBUG_SYMBOLS and hasattr(lib, s), s
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lidarshooter_hip.h")).read())
    assert ("int ls_cloud_nearest(ls_tracer *tr, void *hip_stream, const ls_cloud_nearest_desc *desc, const float *query_to_cloud3x4, "
            "const void *d_cloud, uint32_t n_cloud, const void *d_queries, uint32_t n_queries, void *d_out, void *d_info);") in hdr
    assert ("int ls_cloud_nearest_host(ls_tracer *tr, const ls_cloud_nearest_desc *desc, const float *query_to_cloud3x4, "
            "const void *cloud, uint32_t n_cloud, const void *queries, uint32_t n_queries, void *out, void *info);") in hdr
    assert "int ls_cloud_nearest_check(const ls_cloud_nearest_desc *desc);" in hdr
    assert "#define LS_CLOUD_NEAREST_SKIP_SAME_INDEX 1u" in hdr
    D = capi.CloudNearestDesc
    assert ctypes.sizeof(D) == 32 and capi.LS_CLOUD_NEAREST_SKIP_SAME_INDEX == 1 == ref.SKIP_SAME_INDEX
    assert [getattr(D, k).offset for k in ("radius", "flags", "cloud_stride", "query_stride", "reserved")] == [0, 4, 8, 12, 16]
    assert capi.CLOUD_NEAREST_DTYPE == ref.DTYPE and ref.DTYPE.itemsize == 16
    assert [ref.DTYPE.fields[k][1] for k in ("index", "dist2", "dist", "flags")] == [0, 4, 8, 12]
    assert capi.CLOUD_NEAREST_INFO_DTYPE == ref.INFO_DTYPE and ref.INFO_DTYPE.itemsize == 16
    assert [ref.INFO_DTYPE.fields[k][1] for k in ("n_found", "n_query_outside", "n_cloud_indexed", "reserved")] == [0, 4, 8, 12]
    d = D.make(0.25, 32, 48, flags=1)
    assert (d.radius, d.flags, d.cloud_stride, d.query_stride, list(d.reserved)) == (0.25, 1, 32, 48, [0, 0, 0, 0])
    assert capi.load().ls_abi_version() == 4 == capi.ABI_VERSION


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    buf = (ctypes.c_uint8 * 64)(*([0xAB] * 64))
    pts = np.zeros((4, 3), F)
    d = capi.CloudNearestDesc.make(1.0)
    assert L.ls_cloud_nearest(None, None, ctypes.byref(d), None, pts.ctypes.data, 4, pts.ctypes.data, 4, buf, buf) == INVALID_ARGUMENT
    assert L.ls_cloud_nearest_host(None, ctypes.byref(d), None, pts.ctypes.data, 4, pts.ctypes.data, 4, buf, buf) == INVALID_ARGUMENT
    assert bytes(buf) == b"\xab" * 64   # nothing written


def test_check_refusals(capi):
    L = capi.load()
    check = lambda d: L.ls_cloud_nearest_check(ctypes.byref(d))

    def desc(radius=1.0, cloud_stride=12, query_stride=12, flags=0, reserved=None):
        d = capi.CloudNearestDesc.make(radius, cloud_stride, query_stride, flags)
        if reserved is not None:
            d.reserved[reserved] = 1
        return d
    assert L.ls_cloud_nearest_check(None) == INVALID_ARGUMENT
    assert check(desc()) == 0
    assert check(desc(0.2, 32, 48, capi.LS_CLOUD_NEAREST_SKIP_SAME_INDEX)) == 0
    for flags in (2, 3, 4, 0x80000000):
        assert check(desc(flags=flags)) == INVALID_ARGUMENT
    for k in range(4):
        assert check(desc(reserved=k)) == INVALID_ARGUMENT
    lo, hi = F(2.0 ** -20), F(2.0 ** 20)
    for radius in (lo, hi, np.nextafter(lo, F(1)), np.nextafter(hi, F(0)), 0.013, 1000.0):
        assert check(desc(radius)) == 0, radius
    for radius in (np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, np.nextafter(lo, F(0)), np.nextafter(hi, F(np.inf)), 1e-30, 1e30, 2.0 ** -149):
        assert check(desc(radius)) == INVALID_ARGUMENT, radius
    for stride in (12, 16, 20, 32, 48, 124, 128):
        assert check(desc(cloud_stride=stride)) == 0 and check(desc(query_stride=stride)) == 0
    for stride in (0, 4, 8, 11, 13, 14, 15, 30, 127, 129, 132, 256, 0x80000010, 0xFFFFFFFC):
        assert check(desc(cloud_stride=stride)) == INVALID_ARGUMENT, stride
        assert check(desc(query_stride=stride)) == INVALID_ARGUMENT, stride
    # the hooks refuse what the call refuses of a radius, a missing pointer, a table the call never makes
    pts, cell, part = np.zeros(3, F), np.zeros(3, np.int32), np.zeros(1, np.uint8)
    assert L.ls_debug_cloud_cell(1.0, None, 0, None, None) == 0
    assert L.ls_debug_cloud_cell(1.0, None, 1, cell.ctypes.data, part.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_debug_cloud_cell(1.0, pts.ctypes.data, 1, None, part.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_debug_cloud_cell(1.0, pts.ctypes.data, 1, cell.ctypes.data, None) == INVALID_ARGUMENT
    for radius in (0.0, float("nan"), float("inf"), 2.0 ** -21, 2.0 ** 21):
        assert L.ls_debug_cloud_cell(radius, pts.ctypes.data, 1, cell.ctypes.data, part.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_debug_cloud_bucket(None, 10) == 0xFFFFFFFF
    assert L.ls_debug_cloud_bucket(cell.ctypes.data, 9) == 0xFFFFFFFF and L.ls_debug_cloud_bucket(cell.ctypes.data, 28) == 0xFFFFFFFF
    for k in (10, 17, 27):
        assert L.ls_debug_cloud_bucket(cell.ctypes.data, k) < (1 << k)


# ---- the reference against itself ------------------------------------------------------------------------------------------------

def _same(a, b):
    (ra, ia), (rb, ib) = a, b
    assert ra.tobytes() == rb.tobytes(), np.nonzero(ra != rb)[0][:5]
    assert ia.tobytes() == ib.tobytes(), (ia, ib)


def scan_like(rng, n, box=100.0, power=3.0):
    """n points clustered as a scan is: dense near the origin (the more the larger `power`), within a box of +-box / 2"""
    r = (box / 2) * rng.uniform(0.0, 1.0, (n, 1)) ** power
    d = rng.normal(size=(n, 3))
    d[:, 2] *= 0.15
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (r * d).astype(F)


def lattice(n_side, spacing=0.5, origin=-2.0):
    g = np.arange(n_side) * spacing + origin
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(F)


def test_grid_path_equals_brute_force_on_random_inputs():
    rng = np.random.default_rng(41)
    for radius, n, m in ((0.05, 6000, 4000), (0.3, 6000, 4000), (1.0, 3000, 3000), (2.0, 3000, 2000)):
        cloud = np.concatenate([rng.uniform(-4, 4, (n // 2, 3)), scan_like(rng, n - n // 2, 12.0)]).astype(F)
        q = np.concatenate([rng.uniform(-4.5, 4.5, (m - m // 4, 3)).astype(F), cloud[rng.integers(0, n, m // 4)]])
        cloud[rng.integers(0, n, 20)] = np.nan
        cloud[rng.integers(0, n, 5), 1] = np.inf
        cloud[rng.integers(0, n, 5), 2] = F(radius) * F(70000.0)
        q[rng.integers(0, m, 10), 0] = -np.inf
        q[rng.integers(0, m, 10)] = F(radius) * F(-65537.0)
        for flags in (0, ref.SKIP_SAME_INDEX):
            for xf in (None, np.float32([0.8, -0.6, 0, 0.25, 0.6, 0.8, 0, -0.5, 0, 0, 1.5, 0.125])):
                want = ref.brute(cloud, q, radius, flags, xf)
                _same(ref.grid(cloud, q, radius, flags, xf), want)
                _same(ref.grid(cloud, q, radius, flags, xf, pairs_per_chunk=777), want)
                assert 0 < want[1]["n_found"] < m and want[1]["n_query_outside"] >= 10 and want[1]["n_cloud_indexed"] < n
    # a cloud against itself: with the flag nobody finds itself, without it everybody does, at distance 0
    cloud = rng.uniform(-1, 1, (3000, 3)).astype(F)
    rec, info = ref.brute(cloud, cloud, 0.1)
    assert np.array_equal(rec["index"], np.arange(3000)) and not rec["dist2"].any() and info["n_found"] == 3000
    rec, info = ref.brute(cloud, cloud, 0.1, ref.SKIP_SAME_INDEX)
    assert not np.any(rec["index"] == np.arange(3000)) and 0 < info["n_found"] < 3000 and rec["dist2"][rec["flags"] == 1].min() > 0
    _same(ref.grid(cloud, cloud, 0.1, ref.SKIP_SAME_INDEX), (rec, info))
    # nothing to search, nothing to ask
    rec, info = ref.brute(np.zeros((0, 3), F), cloud[:5], 0.1)
    assert np.all(rec["index"] == ref.INV) and np.all(np.isinf(rec["dist"])) and not rec["flags"].any() and info["n_cloud_indexed"] == 0
    _same(ref.grid(np.zeros((0, 3), F), cloud[:5], 0.1), (rec, info))
    _same(ref.grid(cloud, np.zeros((0, 3), F), 0.1), ref.brute(cloud, np.zeros((0, 3), F), 0.1))


def test_grid_path_equals_brute_force_on_lattices_and_ties():
    """a lattice of spacing 0.5 (exact in float32), queries at its points, edge, face and cell midpoints -- 1, 2, 4 and 8 points at equal
    d2 --: the lowest index wins, in every order of the cloud; the radius on the spacing, on the diagonals and an ulp either side"""
    rng = np.random.default_rng(43)
    cloud = lattice(9)
    base = cloud[rng.integers(0, cloud.shape[0], 600)]
    q = np.concatenate([base, base + F([0.25, 0, 0]), base + F([0, 0.25, 0.25]), base + F([0.25, 0.25, 0.25])]).astype(F)
    for radius in (0.25, np.nextafter(F(0.25), F(0)), 0.5, np.nextafter(F(0.5), F(1)), np.sqrt(F(0.125)), np.sqrt(F(0.1875)), 0.45, 1.1):
        for trial in range(3):
            perm = rng.permutation(cloud.shape[0]) if trial else np.arange(cloud.shape[0])
            c = cloud[perm]
            want = ref.brute(c, q, radius)
            _same(ref.grid(c, q, radius), want)
            _same(ref.grid(c, c, radius, ref.SKIP_SAME_INDEX), ref.brute(c, c, radius, ref.SKIP_SAME_INDEX))
            if ref.constants(radius)[1] >= F(0.1875):   # every kind of query finds its ring of equidistant points: the lowest index of them
                rec = want[0]
                d2 = ((c[None, :, :].astype(np.float64) - q[:, None, :]) ** 2).sum(axis=2)
                ties = d2 == d2.min(axis=1, keepdims=True)
                inside = np.all(np.abs(q) <= 2.0, axis=1)
                assert set(ties[inside].sum(axis=1)) == {1, 2, 4, 8}
                assert np.array_equal(rec["index"][inside], np.argmax(ties, axis=1)[inside])


# ---- the reference against float64 -----------------------------------------------------------------------------------------------

def test_reference_against_float64():
    """The float32 d2 of step 4 is dx, dy, dz rounded once each (relative U = 2^-24; the coordinates are exact), their squares rounded
    once and two sums rounded once, all of terms >= 0: d2 = D2 (1 + e), |e| <= (1 + U)^5 - 1 < 6 U, D2 the float64 value (distances
    here are far above the underflow threshold).  So for the float32 winner w and the float64 winner t, d2(w) <= d2(t) gives
    D(w) <= D(t) sqrt((1 + 6 U) / (1 - 6 U)) < D(t) (1 + 7 U): the same index wins, or the float64 distances of the two winners
    differ by less than 7 U D(t).  The radius likewise: r2 is within U of r^2, so a pair found has D <= r (1 + 4 U) and a query
    that found nothing has D(t) > r (1 - 4 U)."""
    rng = np.random.default_rng(47)
    worst = 0.0
    for radius, scale in ((0.05, 1.0), (0.5, 6.0), (3.7, 40.0), (1000.0, 20000.0), (2.0 ** -20, 2.0 ** -16)):
        cloud = (rng.uniform(-1, 1, (4000, 3)) * scale).astype(F)
        q = (rng.uniform(-1, 1, (3000, 3)) * scale).astype(F)
        rec, info = ref.brute(cloud, q, radius)
        D = np.sqrt(((cloud[None, :, :].astype(np.float64) - q[:, None, :].astype(np.float64)) ** 2).sum(axis=2))
        t = np.argmin(D, axis=1)
        Dt = D[np.arange(q.shape[0]), t]
        r = float(F(radius))
        found = rec["flags"] == 1
        assert 100 < np.count_nonzero(found) < q.shape[0] - 100, np.count_nonzero(found)
        Dw = D[np.nonzero(found)[0], rec["index"][found]]
        worst = max(worst, float(((Dw - Dt[found]) / (U * Dt[found])).max()))
        assert np.all(Dw <= Dt[found] * (1 + 7 * U)) and np.all(Dw <= r * (1 + 4 * U))
        assert np.all(Dt[~found] > r * (1 - 4 * U))
        assert np.count_nonzero(rec["index"][found] != t[found]) <= 5            # (almost always the same index)
        assert np.abs(rec["dist"][found].astype(np.float64) / Dw - 1).max() <= 4 * U + 1e-12   # sqrt(1 + 6 U) (1 + U) - 1 < 4 U + 3 U^2
    print("largest (D(w) - D(t)) / (U D(t))", worst)


# ---- the 27-cell claim against the compiled sequence ---------------------------------------------------------------------------

def _adversarial_pairs(rng, radius, n):
    """queries log-uniform up to D, on cell faces k h and exactly at +-D; the cloud point one radius (a few ulp either side) along one
    axis, and on or near the other axes' faces"""
    D, r2, h = ref.constants(radius)
    r = F(radius)
    mag = np.exp(rng.uniform(np.log(float(r) * 2.0 ** -10), np.log(float(D)), (n, 3)))
    q = (mag * rng.choice([-1.0, 1.0], (n, 3))).astype(F)
    faces = (rng.integers(-64500, 64501, (n, 3)).astype(F) * h).astype(F)               # the rounded k h
    on_face = rng.uniform(size=(n, 3)) < 0.5
    q = np.where(on_face, faces, q)
    edge = rng.uniform(size=(n, 3)) < 0.02
    q = np.where(edge, np.where(rng.uniform(size=(n, 3)) < 0.5, D, -D), q).astype(F)
    for _ in range(2):                                                                  # a few ulp either side of all of these
        step = rng.integers(-2, 3, (n, 3))
        q = np.where(step > 0, np.nextafter(q, F(np.inf)), np.where(step < 0, np.nextafter(q, F(-np.inf)), q)).astype(F)
    q = np.clip(q, -D, D)
    # the offset: the radius along one axis, within a few ulp and within 3e-7 of it; nothing, a sliver or a face-sized step on the others
    axis = rng.integers(0, 3, n)
    off = np.zeros((n, 3), F)
    along = r * (F(1) + rng.integers(-6, 3, n).astype(F) * F(2.0 ** -23)) * rng.choice([-1.0, 1.0], n).astype(F)
    off[np.arange(n), axis] = along
    other = rng.uniform(size=(n, 3)) < 0.3
    small = (r * F(2.0 ** -12) * rng.uniform(-1, 1, (n, 3))).astype(F)
    off = np.where((off == 0) & other, small, off).astype(F)
    p = (q + off).astype(F)
    return q, p


def test_every_passing_pair_has_cells_at_most_one_apart(capi):
    """>= 10^6 adversarial pairs at each of seven radii through ls_debug_cloud_cell: every pair that passes step 4 (both points take part,
    d2 <= r2 in float32) has cells at most 1 apart per axis; the compiled cells are numpy's"""
    rng = np.random.default_rng(53)
    n = 1 << 20
    for radius in RADII:
        D, r2, h = ref.constants(radius)
        q, p = _adversarial_pairs(rng, radius, n)
        cq, part_q = hook_cells(capi, radius, q)
        cp, part_p = hook_cells(capi, radius, p)
        assert np.array_equal(part_q, ref.takes_part(D, q)) and np.array_equal(part_p, ref.takes_part(D, p))
        both = part_q & part_p
        assert np.array_equal(cq[both], ref.cells(h, q[both])) and np.array_equal(cp[both], ref.cells(h, p[both]))
        assert np.abs(cq).max() <= 65536 and np.abs(cp).max() <= 65536
        passes = both & (ref._keys(r2, q, p, np.zeros(n, np.uint32), None) != ref.NONE)
        apart = np.abs(cq.astype(np.int64) - cp.astype(np.int64))[passes].max(axis=1)
        print("radius", radius, "pairs", n, "pass", int(passes.sum()), "a cell apart", int((apart == 1).sum()), "worst", int(apart.max()))
        assert passes.sum() > n // 10 and (apart == 1).sum() > n // 20   # (the pairs are not vacuous: many pass, most of them across a face)
        assert apart.max() <= 1, (radius, q[passes][apart > 1][:3], p[passes][apart > 1][:3])


def test_domain_rule_at_its_edge(capi):
    for radius in RADII:
        D, r2, h = ref.constants(radius)
        assert D == F(radius) * F(65536.0) and float(D) == float(F(radius)) * 65536.0          # exact
        above = np.nextafter(D, F(np.inf))
        rows = []
        for a in range(3):
            for v, want in ((D, True), (-D, True), (above, False), (-above, False), (np.nan, False), (np.inf, False), (-np.inf, False),
                            (F(0), True), (F(-0.0), True), (np.nextafter(D, F(0)), True)):
                p = np.zeros(3, F)
                p[a] = v
                rows.append((p, want))
        pts = np.array([p for p, _ in rows], F)
        want = np.array([w for _, w in rows])
        cell, part = hook_cells(capi, radius, pts)
        assert np.array_equal(part, want) and np.array_equal(ref.takes_part(D, pts), want)
        assert not cell[~want].any()
        assert np.array_equal(cell[want], ref.cells(h, pts[want]))
        assert cell.max() == 64527 and cell.min() == -64528                                    # floor(+-65536 / 1.015625)
        # a query at D finds a cloud point at D and is blind to one an ulp beyond
        cloud = np.array([[D, 0, 0], [above, 0, 0], [np.nan, 0, 0]], F)
        rec, info = ref.brute(cloud, cloud, radius)
        assert list(rec["flags"]) == [1, 2, 2] and list(rec["index"]) == [0, ref.INV, ref.INV] and info["n_cloud_indexed"] == 1
        assert info["n_query_outside"] == 2 and np.isinf(rec["dist2"][1]) and np.isinf(rec["dist"][2])


def test_bucket_hash_spreads_and_collides(capi):
    """the hook the GPU tests construct collisions with: every bucket of a table is in range, neighbouring cells spread over a large
    table, and a small table makes neighbours of one cell share a bucket"""
    cellsx = [(x, y, z) for x in range(-8, 9) for y in range(-8, 9) for z in range(-8, 9)]
    big = [hook_bucket(capi, c, 20) for c in cellsx]
    assert max(big) < 1 << 20 and len(set(big)) > 0.99 * len(cellsx)
    small = [hook_bucket(capi, c, 10) for c in cellsx]
    assert max(small) < 1 << 10 and 900 < len(set(small)) <= 1024
    assert hook_bucket(capi, (65536, -65536, 0), 27) < 1 << 27
