"""ls_cloud_nearest / ls_cloud_nearest_host on the MI355X: for each query the nearest point of a cloud within a radius, against the numpy
restatement of tests/cloud_nearest_reference.py, byte for byte -- the counts around the sort's tile and the wave, exact ties, the radius
itself, the faces of the index's cells, long and colliding buckets, the domain rule, strides and the library's own records, transforms,
a scan-sized cloud, and the entry points' plumbing.  The index (ls_debug_cloud_cell / _bucket) is used to CONSTRUCT inputs only:
nothing the device returns is compared with a hook."""
import ctypes

import numpy as np
import pytest

import cloud_nearest_reference as ref
from conftest import make_tracer
from test_cloud_nearest_cpu import hook_bucket, hook_cells, lattice, scan_like
from test_gpu_labels import _to_device
from test_gpu_rays import _ground_ben

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, OUT_OF_RANGE = -2, -9    # LS_ERR_INVALID_ARGUMENT, LS_ERR_OUT_OF_RANGE
FRAME_EAGER = 0                            # LS_FRAME_EAGER
GUARD = 256
F = np.float32
SKIP = ref.SKIP_SAME_INDEX

# torch fills a new tensor on its own stream, the library works on the handle's: every buffer is filled (a device-wide
# synchronize) before the library gets it


def _same(got, want, what=""):
    (rec, info), (wrec, winfo) = got, want
    assert rec.dtype == ref.DTYPE and rec.shape == wrec.shape, what
    if rec.tobytes() != wrec.tobytes():
        bad = np.nonzero(rec.view(np.uint32).reshape(-1, 4) != wrec.view(np.uint32).reshape(-1, 4))[0]
        assert bad.size == 0, (what, bad.size, bad[:5], rec[bad[:3]], wrec[bad[:3]])
    if info is not None:
        assert info.tobytes() == winfo.tobytes(), (what, info, winfo)


def _xyz(records, stride):
    """x, y, z of whole records of `stride` bytes -> float32 (n, 3)"""
    b = np.ascontiguousarray(records).reshape(-1).view(np.uint8).reshape(-1, stride)
    return b[:, :12].copy().view(F).reshape(-1, 3)


def _device(tr, capi, desc, cloud, queries, xf=None, stream=None, with_info=True):
    """ls_cloud_nearest on device copies of whole records, 0xAB behind both outputs -> (records, info or None)"""
    import torch
    c, n_cloud = tr._strided_points(cloud, desc.cloud_stride)
    q, n_queries = tr._strided_points(queries, desc.query_stride)
    d_c, d_q = _to_device(c), _to_device(q)
    d_out = torch.full((n_queries * 16 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_info = torch.full((16 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = tr.cloudNearestDevice(desc, d_c.data_ptr() if n_cloud else 0, n_cloud, d_q.data_ptr() if n_queries else 0, n_queries,
                               d_out.data_ptr(), d_info.data_ptr() if with_info else 0, xf, stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    o, i = d_out.cpu().numpy(), d_info.cpu().numpy()
    assert np.all(o[n_queries * 16:] == 0xAB) and np.all(i[16:] == 0xAB)
    if not with_info:
        assert np.all(i == 0xAB)
    return o[:n_queries * 16].copy().view(ref.DTYPE), i[:16].copy().view(ref.INFO_DTYPE)[0] if with_info else None


def _check(tr, capi, cloud, queries, radius, flags=0, xf=None, want=None, host=False, what=""):
    """packed float32 points through the device call (and the host variant) against the reference -> the reference's (records, info)"""
    d = capi.CloudNearestDesc.make(radius, 12, 12, flags)
    if want is None:
        want = ref.brute(cloud, queries, radius, flags, xf)
    _same(_device(tr, capi, d, np.ascontiguousarray(cloud, F), np.ascontiguousarray(queries, F), xf), want, what)
    if host:
        rc, rec, info = tr.cloudNearest(d, np.ascontiguousarray(cloud, F), np.ascontiguousarray(queries, F), xf)
        assert rc == 0
        _same((rec, info), want, (what, "host"))
    return want


@pytest.fixture(scope="module")
def bare(capi, sensors):
    """a handle without a commit: the call needs none"""
    tr = make_tracer(capi, sensors["0000"])
    yield tr
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 1. counts -------------------------------------------------------------------------------------------------------------------

N_CLOUD = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8193)    # the sort's tile is 4 096
N_QUERIES = (0, 1, 63, 64, 65, 257)
_counts = {}   # the references, computed once, whichever case asks first


def _counts_reference():
    if not _counts:
        rng = np.random.default_rng(61)
        cloud, q = rng.uniform(-1, 1, (max(N_CLOUD), 3)).astype(F), rng.uniform(-1.1, 1.1, (max(N_QUERIES), 3)).astype(F)
        q[5], q[70, 1] = np.nan, 1e7
        _counts["in"] = (cloud, q)
        for n in N_CLOUD:
            for m in N_QUERIES:
                radius = 0.6 if n < 100 else 0.08
                _counts[n, m] = (radius, ref.brute(cloud[:n], q[:m], radius))
    return _counts


@pytest.mark.parametrize("committed", [False, True])
def test_counts_with_and_without_a_committed_scene(oracle, capi, sensors, meshes, committed):
    """every n_cloud x n_queries: the device call with and without d_info and the host variant; on a handle with no commit, and on
    one with the golden scene committed and frames traced -- the same reference for both"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    if committed:
        _ground_ben(tr, oracle, meshes)
        for k in range(2):
            rc, pts, hits = tr.traceScene(k)
            assert rc == 0 and len(pts) == 1781
    golden = _counts_reference()
    cloud, q = golden["in"]
    for n in N_CLOUD:
        for m in N_QUERIES:
            radius, want = golden[n, m]
            d = capi.CloudNearestDesc.make(radius)
            _same(_device(tr, capi, d, cloud[:n], q[:m]), want, (n, m))
            _same(_device(tr, capi, d, cloud[:n], q[:m], with_info=False), want, (n, m))
            rc, rec, info = tr.cloudNearest(d, cloud[:n], q[:m])
            assert rc == 0
            _same((rec, info), want, (n, m, "host"))
            assert want[1]["n_cloud_indexed"] == n and want[1]["n_query_outside"] == (m > 5) + (m > 70)
            if n == 0:
                assert np.all(want[0]["flags"] != 1) and np.all(want[0]["index"] == ref.INV) and np.all(np.isinf(want[0]["dist"]))
    assert 0 < golden[8193, 257][1][1]["n_found"] < 255
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 2. exact ties ---------------------------------------------------------------------------------------------------------------

def test_exact_ties_go_to_the_lowest_index_in_every_order(capi, bare):
    """a lattice of spacing 0.5, queries at edge, face and cell midpoints: 2, 4 and 8 points at equal d2; three orders of the cloud"""
    rng = np.random.default_rng(67)
    cloud = lattice(9)
    base = cloud[rng.integers(0, cloud.shape[0], 500)]
    q = np.concatenate([base, base + F([0.25, 0, 0]), base + F([0, 0.25, 0.25]), base + F([0.25, 0.25, 0.25])]).astype(F)
    inside = np.all(np.abs(q) <= 2.0, axis=1)
    for trial in range(3):
        c = cloud[rng.permutation(cloud.shape[0])] if trial else cloud
        for radius in (0.45, 0.5):
            rec, info = _check(bare, capi, c, q, radius, host=trial == 0, what=(trial, radius))
            d2 = ((c[None, :, :].astype(np.float64) - q[:, None, :]) ** 2).sum(axis=2)
            ties = d2 == d2.min(axis=1, keepdims=True)
            assert set(ties[inside].sum(axis=1)) == {1, 2, 4, 8}
            assert np.array_equal(rec["index"][inside], np.argmax(ties, axis=1)[inside])      # the reference itself: the lowest index
        _check(bare, capi, c, c, 0.5, SKIP, what=(trial, "self"))                               # six neighbours at 0.5: the lowest


# ---- 3. the radius itself --------------------------------------------------------------------------------------------------------

def test_the_radius_itself(capi, bare):
    up = np.nextafter(F(0.5), F(1))
    for a in range(3):
        for sign in (1, -1):
            on, beyond = np.zeros(3, F), np.zeros(3, F)
            on[a], beyond[a] = sign * F(0.5), sign * up
            rec, info = _check(bare, capi, [on], [[0, 0, 0]], 0.5, host=True)
            assert rec["flags"][0] == 1 and rec["dist"][0] == F(0.5) and rec["dist2"][0] == F(0.25)
            rec, info = _check(bare, capi, [beyond], [[0, 0, 0]], 0.5, host=True)
            assert rec["flags"][0] == 0 and rec["index"][0] == ref.INV and np.isinf(rec["dist"][0]) and info["n_cloud_indexed"] == 1
            rec, info = _check(bare, capi, [beyond, on], [[0, 0, 0]], 0.5)
            assert rec["index"][0] == 1
    # diagonals: queries on a shell around one cloud point at the origin, their float32 d2 within a few ulp of r2 -- equal to it among them
    rng = np.random.default_rng(71)
    for radius in (0.3, 0.05, 3.7):
        D, r2, h = ref.constants(radius)
        d = rng.normal(size=(40000, 3))
        q = (d / np.linalg.norm(d, axis=1, keepdims=True) * float(F(radius)) * (1 + rng.integers(-3, 4, (40000, 1)) * 2.0 ** -24)).astype(F)
        rec, info = _check(bare, capi, [[0, 0, 0]], q, radius)
        on = rec["dist2"] == r2
        print("radius", radius, "found", int(info["n_found"]), "with d2 == r2", int(on.sum()))
        assert on.sum() > 20 and 4000 < info["n_found"] < 36000 and rec["dist2"][rec["flags"] == 1].max() == r2
    # coincident points, points one ulp apart, a subnormal d2
    a = F(2.0 ** -5)                                              # (inside the domain of the smallest radius: D = 2^-4)
    one = np.nextafter(a, F(1))
    cloud = np.array([[a, a, a], [one, a, a], [a, a, a], [0, 0, 0], [1e-20, 0, 0]], F)
    for radius in (2.0 ** -20, 0.05):
        rec, info = _check(bare, capi, cloud, cloud, radius, host=True)
        assert list(rec["index"]) == [0, 1, 0, 3, 4] and not rec["dist2"].any()
        rec, info = _check(bare, capi, cloud, cloud, radius, SKIP, host=True)
        assert list(rec["index"]) == [2, 0, 0, 4, 3]
        assert rec["dist2"][0] == 0 and rec["dist2"][1] == (one - a) * (one - a) > 0 and 0 < rec["dist2"][3] < F(1.1754944e-38)


# ---- 4. cell faces ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [2.0 ** -20, 0.05, 2.0 ** 20])
def test_points_on_and_next_to_cell_faces(capi, bare, radius):
    """points and queries at k h and one ulp either side, per axis and in corners (the faces beyond the domain take no part): every
    pair an ulp apart straddles a face or lies on it"""
    D, r2, h = ref.constants(radius)
    pts = []
    for k in (-65536, -1, 0, 1, 4095, 65535):
        face = F(k) * h
        around = (np.nextafter(face, F(-np.inf)), face, np.nextafter(face, F(np.inf)))
        for v in around:
            for a in range(3):
                p = np.zeros(3, F)
                p[a] = v
                pts.append(p)
            pts.append(np.full(3, v, F))
        pts.append(np.array([around[0], around[1], around[2]], F))
        pts.append(np.array([around[2], around[0], around[1]], F))
    pts = np.array(pts, F)
    part = ref.takes_part(D, pts)
    cell, hook_part = hook_cells(capi, radius, pts)
    assert np.array_equal(part, hook_part) and 0 < np.count_nonzero(~part) <= pts.shape[0] // 2
    assert len({tuple(c) for c in cell[part]}) > 20                                      # the points do lie on both sides of their faces
    rng = np.random.default_rng(73)
    for flags in (0, SKIP):
        rec, info = _check(bare, capi, pts, pts, radius, flags, host=True, what=(radius, flags))
        assert info["n_query_outside"] == np.count_nonzero(~part) == pts.shape[0] - info["n_cloud_indexed"]
        assert info["n_found"] == np.count_nonzero(part)                                 # everybody has a neighbour an ulp away
        c = pts[rng.permutation(pts.shape[0])]
        _check(bare, capi, c, pts, radius, flags, what=(radius, flags, "shuffled"))
    # queries most of a radius from the faces' points, along every axis
    q = np.concatenate([pts + F(radius) * F(s) * np.eye(3, dtype=F)[a] for a in range(3) for s in (-0.999, 0.999, -1.0, 1.0)]).astype(F)
    rec, info = _check(bare, capi, pts, q, radius)
    assert info["n_found"] > q.shape[0] // 4


# ---- 5. long and colliding buckets -----------------------------------------------------------------------------------------------

def test_long_buckets_colliding_buckets_and_a_cloud_that_takes_no_part(capi, bare):
    # 4 097 duplicates of one point -- more than a tile of the sort, one bucket -- and one nearer point with a higher index
    cloud = np.concatenate([np.tile(F([0.3, 0, 0]), (4097, 1)), F([[0, 0.1, 0]])])
    q = F([[0, 0, 0], [0.3, 0, 0], [0.3, 0.01, 0], [5, 5, 5]])
    rec, info = _check(bare, capi, cloud, q, 0.5, host=True)
    assert list(rec["index"]) == [4097, 0, 0, ref.INV]
    rec, info = _check(bare, capi, cloud, cloud, 0.5, SKIP)
    assert rec["index"][0] == 1 and np.all(rec["index"][1:4097] == 0) and rec["index"][4097] == 0
    # 5 000 occupied cells in a table of 2^14 buckets (n_cloud just above and just below 5 000): neighbouring cells of one query share
    # a bucket, and cells far away share buckets with them
    rng = np.random.default_rng(79)
    radius = 1.0
    D, r2, h = ref.constants(radius)
    side = 18
    chosen = rng.permutation(side ** 3)[:5000]
    cells = np.stack([chosen % side, (chosen // side) % side, chosen // (side * side)], axis=1) - side // 2
    centre = ((cells + 0.5 + rng.uniform(-0.4, 0.4, cells.shape)) * float(h)).astype(F)
    got, part = hook_cells(capi, radius, centre)
    assert part.all() and np.array_equal(got, cells)                                       # one point per chosen cell
    q = rng.uniform(-8.5, 8.5, (2000, 3)).astype(F) * h
    qc, _ = hook_cells(capi, radius, q)
    shared = 0
    for c in qc[:400]:
        b = [hook_bucket(capi, c + np.array([x, y, z]), 14) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]
        shared += len(set(b)) < 27
    assert shared >= 2, shared                                                             # (27 cells, 351 pairs, 2^14 buckets: one query in 47)
    for n in (5010, 4990):
        cloud = np.concatenate([centre, centre[:10] + F(0.01)])[:n]
        assert 1 << 14 >= 2 * n > 1 << 13
        rec, info = _check(bare, capi, cloud, q, radius, what=n)
        assert 500 < info["n_found"] < 2000
    # a cloud whose points all fail the domain rule: every record has flags 0
    cloud = np.array([[70000, 0, 0], [np.nan, 0, 0], [0, -np.inf, 0], [0, 0, 65537]], F)
    rec, info = _check(bare, capi, cloud, q[:300] / h, 1.0, host=True)
    assert not rec["flags"].any() and info["n_cloud_indexed"] == 0 and info["n_found"] == 0 and np.all(rec["index"] == ref.INV)


# ---- 6. the domain and non-finite coordinates ------------------------------------------------------------------------------------

def test_domain_and_non_finite_points_among_valid_ones(capi, bare):
    rng = np.random.default_rng(83)
    radius = 0.01                                                # D = 655.36
    D, r2, h = ref.constants(radius)
    cloud = rng.uniform(-0.2, 0.2, (3000, 3)).astype(F)
    q = rng.uniform(-0.2, 0.2, (1500, 3)).astype(F)
    bad = [np.nan, np.inf, -np.inf, np.nextafter(D, F(np.inf)), -np.nextafter(D, F(np.inf)), 1e30, -700.0]
    for k, v in enumerate(bad * 3):
        cloud[10 + 7 * k, k % 3] = v
        q[3 + 5 * k, (k + 1) % 3] = v
    cloud[2000], q[1000] = [D, -D, D], [D, -D, D]                # on the domain's corner: takes part
    q[1001] = [np.nan, np.nan, np.nan]
    for flags in (0, SKIP):
        rec, info = _check(bare, capi, cloud, q, radius, flags, host=True)
        assert info["n_query_outside"] == 22 and info["n_cloud_indexed"] == 3000 - 21 and 100 < info["n_found"] < 1400
        assert rec["index"][1000] == 2000 and rec["dist"][1000] == 0
    bad_rows = np.nonzero(~ref.takes_part(D, cloud))[0]
    assert not np.isin(rec["index"], bad_rows).any()


# ---- 7. strides and the library's own records ------------------------------------------------------------------------------------

def test_strides_with_filler_between_the_coordinates(capi, bare):
    rng = np.random.default_rng(89)
    cloud, q = rng.uniform(-1, 1, (5000, 3)).astype(F), rng.uniform(-1, 1, (700, 3)).astype(F)
    want = ref.brute(cloud, q, 0.1)
    for cs, qs in ((12, 12), (16, 48), (32, 16), (48, 128), (128, 32), (20, 124)):
        d = capi.CloudNearestDesc.make(0.1, cs, qs)
        c, qq = ref.strided(cloud, cs), ref.strided(q, qs)
        _same(_device(bare, capi, d, c, qq), want, (cs, qs))
        rc, rec, info = bare.cloudNearest(d, c, qq)
        assert rc == 0
        _same((rec, info), want, (cs, qs, "host"))
    # the host variant reads 12 bytes of the last record and nothing behind them
    d = capi.CloudNearestDesc.make(0.1, 48, 128)
    c, qq = ref.strided(cloud, 48).reshape(-1)[:-36].copy(), ref.strided(q, 128).reshape(-1)[:-116].copy()
    out, info = np.full(700 * 16 + 32, 0xAB, np.uint8), np.full(48, 0xAB, np.uint8)
    assert bare.L.ls_cloud_nearest_host(bare.h, ctypes.byref(d), None, c.ctypes.data, 5000, qq.ctypes.data, 700, out.ctypes.data + 16, info.ctypes.data + 16) == 0
    assert out[16:-16].tobytes() == want[0].tobytes() and info[16:32].tobytes() == want[1].tobytes()
    assert np.all(out[:16] == 0xAB) and np.all(out[-16:] == 0xAB) and np.all(info[:16] == 0xAB) and np.all(info[32:] == 0xAB)


def test_the_frame_cloud_the_surface_samples_and_the_closest_points(oracle, capi, sensors, meshes):
    """the golden scene's frame cloud (32-byte points) against 4 096 records of ls_sample_surface (48 bytes) and back: the closest
    surface points of the frame's points (ls_closest_points' 32-byte records) against the sample cloud; the frame cloud against itself"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    rc, pts, hits = tr.traceScene(0)
    assert rc == 0 and pts.shape == (1781, 32)
    rc, samples, _ = tr.sampleSurface(capi.SurfaceSampleDesc.make(4096, seed=5))
    assert rc == 0 and samples.dtype.itemsize == 48 and np.all(samples["flags"] == 1)
    P, S = _xyz(pts, 32), _xyz(samples, 48)
    assert np.array_equal(S, samples["p"])
    radius = 0.5
    # completeness: sample -> cloud
    d = capi.CloudNearestDesc.make(radius, 32, 48)
    want = ref.brute(P, S, radius)
    print("samples that find a return within", radius, ":", int(want[1]["n_found"]), "of 4096")
    assert 0 < want[1]["n_found"] < 4096 and want[1]["n_cloud_indexed"] == 1781
    _same(_device(tr, capi, d, pts, samples), want)
    rc, rec, info = tr.cloudNearest(d, pts, samples)
    assert rc == 0
    _same((rec, info), want)
    # accuracy's other form: the frame points' closest surface points -> the sample cloud
    rc, near = tr.closestPoints(np.concatenate([P, np.full((P.shape[0], 1), np.inf, F)], axis=1))
    assert rc == 0 and near.dtype.itemsize == 32
    d = capi.CloudNearestDesc.make(radius, 48, 32)
    want = ref.brute(S, near["q"], radius)
    assert want[1]["n_found"] > 0
    _same(_device(tr, capi, d, samples, near), want)
    # the frame cloud against itself: everybody finds a point at distance 0; with the flag, its nearest other return
    d = capi.CloudNearestDesc.make(radius, 32, 32)
    want = ref.brute(P, P, radius)
    assert not want[0]["dist2"].any() and want[1]["n_found"] == 1781
    _same(_device(tr, capi, d, pts, pts), want)
    d = capi.CloudNearestDesc.make(radius, 32, 32, SKIP)
    want = ref.brute(P, P, radius, SKIP)
    assert not np.any(want[0]["index"] == np.arange(1781)) and want[1]["n_found"] > 100
    _same(_device(tr, capi, d, pts, pts), want)
    rc, again, _ = tr.traceScene(0)                                          # the frames go on as before
    assert rc == 0 and np.array_equal(again, pts)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 8. the transform ------------------------------------------------------------------------------------------------------------

def test_rigid_and_scaling_transforms_and_queries_that_leave_the_domain(capi, bare):
    rng = np.random.default_rng(97)
    cloud = rng.uniform(-3, 3, (4000, 3)).astype(F)
    q = rng.uniform(-3, 3, (1500, 3)).astype(F)
    c, s_ = np.cos(0.7), np.sin(0.7)
    rigid = np.float32([c, -s_, 0, 0.5, s_, c, 0, -0.25, 0, 0, 1, 0.125])
    scaling = np.float32([2.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, -1.5, 1])
    plain = ref.brute(cloud, q, 0.3)
    for xf in (rigid, scaling):
        want = _check(bare, capi, cloud, q, 0.3, xf=xf, host=True)
        assert want[0].tobytes() != plain[0].tobytes() and 100 < want[1]["n_found"] < 1500
        _check(bare, capi, cloud, cloud, 0.3, SKIP, xf=xf)                  # (the query's own index, not its place, is what is skipped)
    # radius 2^-10: D = 64.  The queries lie inside the domain and some leave it under the transform
    radius = 2.0 ** -10
    cloud = rng.uniform(-60, 60, (2000, 3)).astype(F)
    q = np.concatenate([cloud[:500] * F(0.5), rng.uniform(-60, 60, (500, 3)).astype(F)])
    grow = np.float32([2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0])
    shift = np.float32([1, 0, 0, 40, 0, 1, 0, 0, 0, 0, 1, 0])
    assert ref.brute(cloud, q, radius)[1]["n_query_outside"] == 0
    for xf in (grow, shift):
        want = _check(bare, capi, cloud, q, radius, xf=xf, host=True)
        assert 100 < want[1]["n_query_outside"] < 900
    assert ref.brute(cloud, q, radius, xf=grow)[1]["n_found"] == 500        # 2 * (0.5 p) is p again, exactly


# ---- 9. a scan-sized cloud -------------------------------------------------------------------------------------------------------

_large = {}


def _large_inputs():
    if not _large:
        rng = np.random.default_rng(101)
        _large["cloud"] = scan_like(rng, 1 << 17, 100.0, power=1.0)
        q = scan_like(rng, 1 << 15, 100.0, power=1.0)
        q[::3] += rng.normal(scale=0.3, size=q[::3].shape).astype(F)
        _large["q"] = q
    return _large["cloud"], _large["q"]


@pytest.mark.parametrize("radius", [0.2, 2.0])
def test_a_scan_sized_cloud_against_the_grid_path(capi, bare, radius):
    """2^17 points in a 100 m box, dense near the origin as a scan is, 2^15 queries: against the reference's grid path, which
    tests/test_cloud_nearest_cpu.py holds to the brute force"""
    cloud, q = _large_inputs()
    want = ref.grid(cloud, q, radius)
    assert 1000 < want[1]["n_found"] and want[1]["n_cloud_indexed"] == 1 << 17
    _check(bare, capi, cloud, q, radius, want=want, what=radius)
    if radius == 0.2:
        _check(bare, capi, cloud, q, radius, want=want, host=True, what="host")


# ---- 10. plumbing ----------------------------------------------------------------------------------------------------------------

def test_entry_points(oracle, capi, sensors, meshes):
    """a caller's stream; two calls back to back with different radii (the scratch is reused); every refusal in its order, nothing
    written; a frame traced between two calls still equals the oracle"""
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _ground_ben(tr, oracle, meshes)
    rng = np.random.default_rng(103)
    cloud, q = rng.uniform(-1, 1, (6000, 3)).astype(F), rng.uniform(-1, 1, (1000, 3)).astype(F)
    want = {r: ref.brute(cloud, q, r) for r in (0.05, 0.4)}
    st = torch.cuda.Stream()
    _same(_device(tr, capi, capi.CloudNearestDesc.make(0.05), cloud, q, stream=st.cuda_stream), want[0.05])
    # back to back on one handle, nothing waited for in between: the second call's index replaces the first one's in stream order
    d_c, d_q = _to_device(cloud), _to_device(q)
    outs = [torch.full((1000 * 16 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    infos = [torch.full((16,), 0xAB, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    order = (0.05, 0.4, 0.05)
    for k, r in enumerate(order):
        n = 6000 if k != 1 else 3000                                         # (a smaller cloud in between: a smaller table)
        assert tr.cloudNearestDevice(capi.CloudNearestDesc.make(r), d_c.data_ptr(), n, d_q.data_ptr(), 1000, outs[k].data_ptr(), infos[k].data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    for k, r in enumerate(order):
        w = want[r] if k != 1 else ref.brute(cloud[:3000], q, r)
        o = outs[k].cpu().numpy()
        assert np.all(o[16000:] == 0xAB)
        _same((o[:16000].copy().view(ref.DTYPE), infos[k].cpu().numpy().view(ref.INFO_DTYPE)[0]), w, k)
    # a frame between two calls equals the oracle; the call after it is unchanged
    rc, pts, hits = tr.traceScene(0)
    assert rc == 0 and np.array_equal(pts, oracle.trace_frame(s, ml)["points"])
    _same(_device(tr, capi, capi.CloudNearestDesc.make(0.4), cloud, q), want[0.4])
    # refusals, nothing written
    L, h = tr.L, tr.h
    out = torch.full((1000 * 16 + 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    iout = torch.full((32,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def desc(radius=0.1, cs=12, qs=12, flags=0, reserved=None):
        d = capi.CloudNearestDesc.make(radius, cs, qs, flags)
        if reserved is not None:
            d.reserved[reserved] = 1
        return d

    def call(handle=h, d=desc(), **kw):
        a = dict(xf=None, cloud=d_c.data_ptr(), n_cloud=6000, queries=d_q.data_ptr(), n_queries=1000, out=out.data_ptr(), info=iout.data_ptr())
        a.update(kw)
        return L.ls_cloud_nearest(handle, None, None if d is None else ctypes.byref(d), a["xf"], a["cloud"], a["n_cloud"], a["queries"],
                                  a["n_queries"], a["out"], a["info"])
    bad_xf = np.float32([1, 0, 0, 0, 0, 1, 0, np.inf, 0, 0, 1, 0])
    nan_xf = np.float32([np.nan, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    assert call(d=None) == INVALID_ARGUMENT
    assert call(out=None) == INVALID_ARGUMENT and call(cloud=None) == INVALID_ARGUMENT and call(queries=None) == INVALID_ARGUMENT
    assert call(d=desc(flags=2)) == INVALID_ARGUMENT and call(d=desc(flags=0x80000000)) == INVALID_ARGUMENT
    assert call(d=desc(reserved=0)) == INVALID_ARGUMENT and call(d=desc(reserved=3)) == INVALID_ARGUMENT
    for radius in (np.nan, np.inf, 0.0, -1.0, 2.0 ** -21, 2.0 ** 21):
        assert call(d=desc(radius)) == INVALID_ARGUMENT
    for stride in (0, 8, 14, 132):
        assert call(d=desc(cs=stride)) == INVALID_ARGUMENT and call(d=desc(qs=stride)) == INVALID_ARGUMENT
    assert call(xf=bad_xf.ctypes.data) == INVALID_ARGUMENT and call(xf=nan_xf.ctypes.data) == INVALID_ARGUMENT
    assert call(cloud=d_c.data_ptr() + 2) == INVALID_ARGUMENT and call(queries=d_q.data_ptr() + 1) == INVALID_ARGUMENT
    assert call(out=out.data_ptr() + 8) == INVALID_ARGUMENT and call(info=iout.data_ptr() + 4) == INVALID_ARGUMENT
    assert call(n_cloud=(1 << 27) + 1) == OUT_OF_RANGE and call(n_queries=0xFFFFFF01) == OUT_OF_RANGE
    # an invalid argument answers before anything out of range
    assert call(n_cloud=(1 << 27) + 1, d=desc(flags=4)) == INVALID_ARGUMENT and call(n_queries=0xFFFFFF01, out=out.data_ptr() + 4) == INVALID_ARGUMENT
    hb = np.full(1000 * 16, 0xAB, np.uint8)
    assert L.ls_cloud_nearest_host(h, ctypes.byref(desc(flags=8)), None, cloud.ctypes.data, 6000, q.ctypes.data, 1000, hb.ctypes.data, None) == INVALID_ARGUMENT
    assert L.ls_cloud_nearest_host(h, ctypes.byref(desc()), None, None, 6000, q.ctypes.data, 1000, hb.ctypes.data, None) == INVALID_ARGUMENT
    assert L.ls_cloud_nearest_host(h, ctypes.byref(desc()), None, cloud.ctypes.data, 6000, q.ctypes.data, 1000, None, None) == INVALID_ARGUMENT
    assert L.ls_cloud_nearest_host(h, ctypes.byref(desc()), bad_xf.ctypes.data, cloud.ctypes.data, 6000, q.ctypes.data, 1000, hb.ctypes.data, None) == INVALID_ARGUMENT
    assert L.ls_cloud_nearest_host(h, ctypes.byref(desc()), None, cloud.ctypes.data, (1 << 27) + 1, q.ctypes.data, 1000, hb.ctypes.data, None) == OUT_OF_RANGE
    assert np.all(hb == 0xAB)
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(iout.cpu().numpy() == 0xAB)
    # nothing to do is not an error: no queries with and without an info, no buffers at all
    assert call(n_queries=0, queries=None, out=None) == 0 and call(n_queries=0, queries=None, out=None, info=None) == 0
    assert call(n_cloud=0, cloud=None, n_queries=0, queries=None, out=None, info=None) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert iout.cpu().numpy()[:16].view(np.uint32).tolist() == [0, 0, 6000, 0] and np.all(out.cpu().numpy() == 0xAB)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_open_frame_graph_is_refused(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0001"]
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    tr.setOption(capi.LS_OPT_FRAME_GRAPH, 1)
    _ground_ben(tr, oracle, meshes)
    cap = s.V * s.H
    p, h, c = (torch.zeros(32 * cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * cap, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), cap)
    rng = np.random.default_rng(107)
    cloud, q = rng.uniform(-1, 1, (3000, 3)).astype(F), rng.uniform(-1, 1, (500, 3)).astype(F)
    d_c, d_q = _to_device(cloud), _to_device(q)
    d = capi.CloudNearestDesc.make(0.1)
    out = torch.full((500 * 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    iout = torch.full((16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != FRAME_EAGER   # the frame is being captured: the graph is open
    assert L.ls_cloud_nearest(tr.h, None, ctypes.byref(d), None, d_c.data_ptr(), 3000, d_q.data_ptr(), 500, out.data_ptr(), iout.data_ptr()) == INVALID_ARGUMENT
    assert L.ls_cloud_nearest_host(tr.h, None, None, None, 0, None, 0, None, None) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(iout.cpu().numpy() == 0xAB)
    # the graph is closed: the call works
    assert tr.cloudNearestDevice(d, d_c.data_ptr(), 3000, d_q.data_ptr(), 500, out.data_ptr(), iout.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    _same((out.cpu().numpy().view(ref.DTYPE), iout.cpu().numpy().view(ref.INFO_DTYPE)[0]), ref.brute(cloud, q, 0.1))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
