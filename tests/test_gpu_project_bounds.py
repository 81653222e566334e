"""The footprint bounds of k_project against the oracle's exhaustive closest hit, every ray compared (t bits, geometry, primitive),
with one frame in flight and with LS_OPT_PIPELINE 2: elevation tables that stress the channel band's guess-and-verify start
(csrc/ls_band_map.h), triangles whose edges lie in the vertical plane of a column's (cos, sin) pair and one ulp either side,
the 0 / 360 degree seam, a reversed sweep, a triangle the vertical axis pierces, and footprints on both sides of the
big-footprint threshold.  The bounds only have to be supersets: whatever they are, the frame must be the oracle's."""
import ctypes

import numpy as np
import pytest

from conftest import grazing_mesh, make_tracer

pytestmark = pytest.mark.gpu

f32p = ctypes.POINTER(ctypes.c_float)
I3 = np.eye(3, dtype=np.float32).reshape(9)


def _sensor(oracle, vertical, H, begin=0.0, end=360.0):
    return oracle.Sensor(uid="bounds", vertical=np.asarray(vertical, np.float32), h_begin=np.float32(begin), h_end=np.float32(end),
                         h_count=H, R=I3, Rinv=I3, t=np.zeros(3, np.float32))


def _soup(rng, n, scale):
    c = rng.normal(0.0, scale, size=(n, 1, 3))
    size = np.exp(rng.uniform(np.log(0.02), np.log(scale), size=(n, 1, 1)))
    return (c + rng.normal(0.0, 1.0, size=(n, 3, 3)) * size).reshape(-1, 3).astype(np.float32)


def _mesh(*vertex_blocks):
    v = np.concatenate([np.asarray(b, np.float32).reshape(-1, 3) for b in vertex_blocks])
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)


def _ulp_variants(v, axis):
    """the vertices, and the same with coordinate `axis` one ulp up / one ulp down"""
    up, dn = v.copy(), v.copy()
    up[:, axis] = np.nextafter(v[:, axis], np.float32(np.inf))
    dn[:, axis] = np.nextafter(v[:, axis], np.float32(-np.inf))
    return [v, up, dn]


def _check_both_modes(oracle, capi, s, v, t, min_hits):
    """the frame through k_project with one frame in flight, then with three (the synchronous call on a pipelined handle, once
    per slot stream): every ray's (t bits, global triangle) equal to the oracle's"""
    ref = oracle.trace_frame(s, [(0, v, t, oracle.IDENTITY_AFFINE)])
    assert int((ref["gid"] != oracle.INVALID).sum()) >= min_hits
    tr = make_tracer(capi, s, "projection")
    tr.addGeometry("m", v.shape[0], t.shape[0])
    tr.updateGeometry("m", oracle.IDENTITY_AFFINE, v, t)
    assert tr.commitScene() == 0

    def one(frame):
        rc, pts, hits = tr.traceScene(frame)
        assert rc == 0
        tt, gid = tr.denseHits()
        assert np.array_equal(gid, ref["gid"]), "hit triangle ids / hit-miss set differ from the oracle"
        assert np.array_equal(tt.view(np.uint32), ref["t"].view(np.uint32)), "t not bit-equal"
        got = np.stack([hits["ray"], hits["geom"], hits["prim"], hits["t"].view(np.uint32)], axis=1)
        assert np.array_equal(got, ref["hits"]) and np.array_equal(pts, ref["points"])
    one(0)
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    for k in range(3):
        one(1 + k)
    return tr


def _band_walk(capi, tr):
    m = np.zeros(8, np.float32)
    assert capi.load().ls_debug_tracer_band_map(tr.h, m.ctypes.data_as(f32p)) == 0
    return int(m[6:].view(np.int32)[1])


BAND_TABLES = {
    "v1": [3.0],
    "v2": [-1.0, 2.0],
    "uniform16": list(np.linspace(-15.0, 15.0, 16)),
    "clusters16": list(np.linspace(-20.0, -12.0, 8)) + list(np.linspace(8.0, 15.0, 8)),                  # one gap of 20 degrees
    "repeated16": [-15, -13, -11, -9, -7, -5, -3, -1, -1, 1, 3, 5, 7, 9, 11, 13],
    "nonuniform33": list(np.sign(np.linspace(-1, 1, 33)) * np.abs(np.linspace(-1, 1, 33)) ** 5 * 60.0),   # keeps the bisection
    "descending16": list(np.linspace(15.0, -15.0, 16)),
}


@pytest.mark.parametrize("name", list(BAND_TABLES))
def test_band_start_by_guess_and_verify(oracle, capi, name):
    """a few hundred random triangles, and grazing triangles whose highest or lowest corner sits on a ray of the raster (the
    construction of test_triangles_whose_corner_lies_on_a_ray: conftest.grazing_mesh, identity pose here) and one ulp of z above
    and below it: a vertex elevation on a channel, and either side of it"""
    s = _sensor(oracle, BAND_TABLES[name], 64)
    rng = np.random.default_rng(len(name) * 131)
    gv, _ = grazing_mesh(oracle, s, n=96, seed=5)
    v, t = _mesh(_soup(rng, 300, 8.0), *_ulp_variants(gv, 2))
    tr = _check_both_modes(oracle, capi, s, v, t, 40 if len(BAND_TABLES[name]) > 2 else 5)
    walk = _band_walk(capi, tr)
    if name in ("v1", "nonuniform33"):
        assert walk < 0        # the handle bisects
    elif name != "v2":
        assert 0 <= walk <= 3  # the handle starts from its map
    tr.close()


def _column_plane_triangles(oracle, s, rng, n):
    """triangles with an edge IN the vertical plane of a column's (cos phi, sin phi) as the tables hold it -- both ends r * (cos, sin)
    in float32 -- the third corner towards the next column; then the same with y one ulp up and one ulp down"""
    st, ct, sp, cp = oracle.ray_tables(s)
    tris = []
    for k in range(n):
        h = int(rng.integers(0, s.H))
        r1, r2 = np.float32(rng.uniform(3.0, 40.0)), np.float32(rng.uniform(3.0, 40.0))
        a = np.array([r1 * cp[h], r1 * sp[h], np.float32(-0.25) * r1], np.float32)
        b = np.array([r2 * cp[h], r2 * sp[h], np.float32(0.2) * r2], np.float32)
        hn = (h + (1 if k % 2 else -1)) % s.H
        r3 = np.float32(rng.uniform(3.0, 40.0))
        c = np.array([r3 * cp[hn], r3 * sp[hn], np.float32(rng.uniform(-0.2, 0.15)) * r3], np.float32)
        tris.append([a, b, c])
    v = np.array(tris, np.float32).reshape(-1, 3)
    return _ulp_variants(v, 1) + _ulp_variants(v, 0)[1:]


@pytest.mark.parametrize("H,begin,end", [(360, 0.0, 360.0), (4096, 0.0, 360.0), (360, 300.0, -60.0), (4096, -170.0, 35.0)])
def test_column_intervals_on_and_beside_a_column_plane(oracle, capi, H, begin, end):
    """V = 4; edges in a column's plane and one ulp beside it, triangles across the 0 / 360 seam and across the sweep's own
    begin / end, a reversed sweep with h_begin != 0, triangles the vertical axis pierces above and below"""
    s = _sensor(oracle, [-10.0, -3.0, 2.0, 8.0], H, begin, end)
    rng = np.random.default_rng(H + int(begin))
    seam = []
    for phi0 in (0.0, float(begin), float(end)):
        for half in (0.02, 0.4, 3.0):   # degrees either side of the seam
            a0, a1 = np.radians(phi0 - half), np.radians(phi0 + half)
            r = 12.0
            seam.append([[r * np.cos(a0), r * np.sin(a0), -3.0], [r * np.cos(a1), r * np.sin(a1), -3.0], [r * np.cos(a0), r * np.sin(a0), 2.5]])
    axis = [[[-1, -1, 3], [2, -1, 3], [-1, 2, 3]], [[-1, -1, -2], [2, -1, -2], [-1, 2, -2]], [[-30, -25, -4], [35, -20, -4], [0, 40, -4]]]
    v, t = _mesh(_soup(rng, 200, 8.0), *_column_plane_triangles(oracle, s, rng, 60), seam, axis)
    _check_both_modes(oracle, capi, s, v, t, 200).close()


def test_footprints_around_the_big_footprint_threshold(oracle, capi):
    """footprints of 100 to 160 cells in three shapes -- one ring wide, one column wide, a block -- around the 128 cells above which
    a footprint goes to the gather queue instead of the wave's own trips, and a few of many thousand cells"""
    from lidarshooter_amd import synth
    s = _sensor(oracle, synth.syn_vertical(128), 512)
    step, ring = 360.0 / 512.0, 40.0 / 127.0
    tris = []
    r = 20.0

    def at(az_deg, el_deg):
        a, e = np.radians(az_deg), np.radians(el_deg)
        return [r * np.cos(a), r * np.sin(a), r * np.tan(e)]
    for k, cols in enumerate(range(100, 161, 4)):       # one ring (at most two) x cols columns
        az, el = 5.0 + 11.0 * k, -5.0 + 0.31 * k
        tris.append([at(az, el), at(az + cols * step, el), at(az + 0.5 * cols * step, el + 0.2 * ring)])
    for k, chans in enumerate(range(100, 129, 4)):      # chans rings x one column (at most two)
        az = 190.0 + 9.0 * k
        tris.append([at(az, -25.0), at(az + 0.3 * step, -25.0), at(az + 0.15 * step, -25.0 + chans * ring)])
    for k, cols in enumerate(range(12, 21)):            # 8 rings x cols columns
        az = 280.0 + 8.0 * k
        tris.append([at(az, 2.0), at(az + cols * step, 2.0), at(az, 2.0 + 7.2 * ring)])
    tris.append([[-200, -200, -3], [200, -200, -3], [200, 200, -3]])   # thousands of cells: the queue
    v, t = _mesh(tris, _soup(np.random.default_rng(3), 150, 6.0))
    _check_both_modes(oracle, capi, s, v, t, 3000).close()
