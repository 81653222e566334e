"""Group culling (k_group_bounds, k_cull, k_project<CULLED>: csrc/ls_project.hip) on meshes of one to 67 600 triangles -- culling
forced onto them with ls_debug_force_group_cull -- against tests/cull_reference.py, which restates what the pass may and may not do
with numpy and the CPU oracle.  Every case asserts
  (a) the downloaded group and block boxes hold their vertices (float64), and mark non-finite ones unbounded;
  (b) every group that some ray of the raster (of the shard) hits when it stands alone survives the pass: the exact necessary
      condition for a frame that is bit for bit the oracle's, whether or not the group's hits are the closest ones;
  (c) no group survives whose float64 bound, doubled, lies between two rings (moderate coordinates only);
  (d) the frame is bit for bit oracle.trace_frame's, with one frame in flight and with LS_OPT_PIPELINE 2;
  (e) the scene is not vacuous: at least 10 % of the groups must survive and at least 10 % are rejected (tiny meshes: a hit).
The k_cull instantiation the hook reports is asserted wherever a case is about it."""
import numpy as np
import pytest

import cull_reference as cr
from conftest import make_tracer
from test_gpu_project_bounds import BAND_TABLES

pytestmark = pytest.mark.gpu

I3 = np.eye(3, dtype=np.float32).reshape(9)
LUT, LDS, SECTOR, COUNT, UNCULLED = 1, 2, 4, 8, 16


def _sensor(oracle, vertical, H, begin=0.0, end=360.0, t=(0.0, 0.0, 0.0), Rinv=I3, R=I3):
    return oracle.Sensor(uid="cull", vertical=np.asarray(vertical, np.float32), h_begin=np.float32(begin), h_end=np.float32(end), h_count=H,
                         R=np.asarray(R, np.float32), Rinv=np.asarray(Rinv, np.float32), t=np.asarray(t, np.float32))


UNIFORM16 = BAND_TABLES["uniform16"]
V33 = list(np.linspace(-24.0, 8.0, 33))


def _tracer(capi, s, geoms, shard=None, count=False):
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_BLOCK_CULL, 1)
    tr.forceGroupCull(True)
    if count:
        tr.setOption(capi.LS_OPT_COUNT_VISITS, 1)
    for name, v, e, A, indexed in geoms:
        e = np.asarray(e, np.uint32)
        tr.addGeometry(name, v.shape[0], e.shape[0], capi.LS_GEOMETRY_TYPE_QUAD if e.shape[1] == 4 else capi.LS_GEOMETRY_TYPE_TRIANGLE)
        tr.updateGeometry(name, A, v, e if indexed else None)   # (a geometry without indices has an id and no place in the scene)
    if shard is not None:
        tr.setShard(*shard)
    assert tr.commitScene() == 0
    return tr


def _frames(oracle, capi, tr, s, geoms, shard, min_hits, use_bvh=False):
    """(d): the synchronous frame, then three with LS_OPT_PIPELINE 2 (once per slot stream): every ray of the shard with the oracle's
    (t bits, triangle); on the full turn the hit records and points too"""
    ref = oracle.trace_frame(s, [(tr.getGeometryId(name), v, e, A) for name, v, e, A, indexed in geoms if indexed], use_bvh=use_bvh)
    cols = cr.shard_columns(s.H, shard)
    want_gid = ref["gid"].reshape(s.V, s.H)[:, cols].reshape(-1)
    want_t = ref["t"].reshape(s.V, s.H)[:, cols].reshape(-1)
    n_hit = int((want_gid != oracle.INVALID).sum())
    assert n_hit >= min_hits, n_hit

    if any(np.asarray(e).shape[1] == 4 for _, _, e, _, indexed in geoms if indexed):
        # (the dense view names a quad's first triangle for both; the hit records below carry the quad)
        want_gid = np.where(want_gid == oracle.INVALID, want_gid, want_gid & ~np.uint32(1))

    def one(frame):
        rc, pts, hits = tr.traceScene(frame)
        assert rc == 0
        tt, gid = tr.denseHits()
        assert np.array_equal(gid, want_gid), "hit triangle ids / hit-miss set differ from the oracle"
        assert np.array_equal(tt.view(np.uint32), want_t.view(np.uint32)), "t not bit-equal"
        assert len(pts) == n_hit and len(hits) == n_hit
        if shard is None:
            got = np.stack([hits["ray"], hits["geom"], hits["prim"], hits["t"].view(np.uint32)], axis=1)
            assert np.array_equal(got, ref["hits"]) and np.array_equal(pts, ref["points"])
    one(0)
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    for k in range(3):
        one(1 + k)
    tr.setOption(capi.LS_OPT_PIPELINE, 0)
    return n_hit


def _check_cull(oracle, tr, s, geoms, shard=None, moderate=True, floors=True, variant=None):
    """(a), (b), (c), (e) for every culled geometry of the scene -> {name: (must_survive, survivors, variant, boxes)}"""
    up, dn, _, _ = tr.cullTables()
    out = {}
    for gname, v, e, A, indexed in geoms:
        if not indexed:
            continue
        perm, gb, bb = tr.downloadCull(gname)
        assert cr.box_contains(v, e, perm, gb, bb) == []                                       # (a)
        surv, var = tr.cullSurvivors(gname)
        if variant is not None:
            assert var == variant, (gname, var, variant)
        ng = gb.shape[0]
        assert surv.shape[0] == np.unique(surv).shape[0] and (surv.shape[0] == 0 or surv.max() < ng)
        kept = np.zeros(ng, bool)
        kept[surv] = True
        ms = cr.must_survive(oracle, s, v, e, A, perm, shard)
        lost = np.flatnonzero(ms & ~kept)
        assert lost.size == 0, f"{gname}: groups {lost[:8]} of {ng} are hit by a ray and were rejected"     # (b)
        if moderate:
            clear = cr.clearly_between_rings(s, A, gb, up, dn)
            wrong = np.flatnonzero(clear & kept)
            assert wrong.size == 0, f"{gname}: groups {wrong[:8]} lie between two rings and survived"    # (c)
        if floors:
            assert ms.mean() >= 0.1 and 1.0 - kept.mean() >= 0.1, (gname, ms.mean(), kept.mean())           # (e)
        else:
            assert ms.any(), gname
        out[gname] = (ms, kept, var, gb, bb, perm)
    return out


def _case(oracle, capi, s, geoms, shard=None, moderate=True, floors=True, variant=None, min_hits=1, count=False, use_bvh=False):
    geoms = [g if len(g) == 5 else (*g, True) for g in geoms]
    tr = _tracer(capi, s, geoms, shard, count)
    got = _check_cull(oracle, tr, s, geoms, shard, moderate, floors, variant)
    if count:
        tr.setOption(capi.LS_OPT_COUNT_VISITS, 0)
    _frames(oracle, capi, tr, s, geoms, shard, min_hits, use_bvh)
    tr.close()
    return got


def _ground(n_tris, seed=0, cell=0.3, centre=(12.0, 0.0)):
    """a relief beside the sensor, 2 m below it, cut to n_tris triangles (odd counts: a partial last quad and a partial last group),
    in square cells of `cell` metres: a group of four triangles is then a fraction of the ring spacing deep (2.6 m out there for
    rings 2 degrees apart), so that most groups fall between two rings, and as wide as a column of a 256-column raster, so that those on a
    ring are hit"""
    cells = (n_tris + 1) // 2
    ny = max(1, int(round(np.sqrt(cells))))
    nx = (cells + ny - 1) // ny
    v, t = cr.relief_grid(nx + 1, ny + 1, 1.0, amp=0.1, seed=seed)
    v[:, 0] = v[:, 0] * np.float32(0.5 * nx * cell) + np.float32(centre[0])
    v[:, 1] = v[:, 1] * np.float32(0.5 * ny * cell) + np.float32(centre[1])
    return v, t[:n_tris].copy()


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_tiny_meshes(oracle, capi, n):
    """one group, partial or full, and one group plus one triangle: a k_cull workgroup with one or two live lanes"""
    s = _sensor(oracle, UNIFORM16, 64)
    v, t = cr.soup(n, 0.5, seed=n, size=(1.0, 2.0))
    v = (v + np.array([6.0, 1.0, -0.5], np.float32)).astype(np.float32)
    got = _case(oracle, capi, s, [("m", v, t, oracle.IDENTITY_AFFINE)], floors=False, variant=LUT | LDS)
    assert got["m"][1].shape[0] == (n + 3) // 4


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1025, 2052])
def test_sizes_around_a_block_and_a_workgroup(oracle, capi, n):
    """64 groups are a block (256 triangles), 512 groups a k_cull workgroup at two rounds (2 048 triangles): one group short of,
    exactly and one triangle past a block; a partial last group; 513 groups -- a second workgroup with one live lane"""
    s = _sensor(oracle, V33, 256)
    v, t = _ground(n, seed=n, cell=0.15)
    got = _case(oracle, capi, s, [("m", v, t, oracle.IDENTITY_AFFINE)], variant=LUT | LDS, min_hits=8)
    assert got["m"][1].shape[0] == (n + 3) // 4


def test_grid_of_67600_triangles(oracle, capi):
    """16 900 groups: 34 k_cull workgroups -- more than the 32 list segments, so every segment is used and the first two take a
    second workgroup's survivors"""
    s = _sensor(oracle, V33, 256)
    v, t = cr.annulus(131, 260, 5.0, 31.0, amp=0.1, seed=9)   # ground all round, cells 0.2 m deep and 1.4 degrees wide
    assert t.shape[0] == 67600
    _case(oracle, capi, s, [("m", v, t, oracle.IDENTITY_AFFINE)], variant=LUT | LDS, min_hits=3000, use_bvh=True)   # (the oracle's own BVH: the same hits, sooner)


# ---- channel tables --------------------------------------------------------------------------------------------------------------
TABLES = {
    "uniform16": (UNIFORM16, 256, LUT | LDS),
    "descending16": (BAND_TABLES["descending16"], 256, LUT | LDS),
    "clusters16": (BAND_TABLES["clusters16"], 256, LUT | LDS),
    "repeated16": (BAND_TABLES["repeated16"], 256, LUT | LDS),
    "pairs16": ([e for e in np.linspace(-16.0, -2.0, 8) for _ in range(2)], 256, LUT | LDS),          # both compare-and-steps of the look-up
    "triples12": ([e for e in np.linspace(-15.0, -3.0, 4) for _ in range(3)], 256, LDS),              # three channels in a bucket: the search
    "v1": ([-8.0], 256, LDS),
    "poles5": ([-90.0, -30.0, -5.0, 20.0, 90.0], 256, LDS),                                          # infinite tangents
    "v2049": (list(np.linspace(-40.0, 40.0, 2049)), 8, 0),                                          # tables in global memory
}


def _table_scene(name):
    if name == "v2049":
        return _ground(300, seed=7)
    if name == "v1":   # one ring, which meets the ground 14.2 m out: a strip of ground around that circle
        return cr.annulus(9, 200, 12.2, 16.2, seed=5)
    return _ground(1500, seed=len(name), centre={"clusters16": (7.5, 0.0), "poles5": (0.0, 0.0)}.get(name, (12.0, 0.0)))


@pytest.mark.parametrize("name", list(TABLES))
def test_channel_tables(oracle, capi, name):
    vertical, H, variant = TABLES[name]
    s = _sensor(oracle, vertical, H)
    v, t = _table_scene(name)
    # (v2049: 0.04 degrees between rings -- every group meets one: the case is about the variant, (a), (b) and (d))
    _case(oracle, capi, s, [("m", v, t, oracle.IDENTITY_AFFINE)], variant=variant, floors=name != "v2049", min_hits=20)


def _query_values(up, dn):
    x = np.unique(np.concatenate([up, dn]))
    x = x[np.isfinite(x)]
    inf = np.float32(np.inf)
    parts = [x, np.nextafter(x, inf), np.nextafter(x, -inf), (0.5 * (x[1:].astype(np.float64) + x[:-1])).astype(np.float32),
             np.array([-np.inf, np.inf, np.nan, -3e38, 3e38, 0.0], np.float32)]
    if x.size:
        span = max(float(x[-1]) - float(x[0]), 1.0)
        parts.append(np.array([x[0] - 0.01 * span, x[0] - 10.0 * span, x[-1] + 0.01 * span, x[-1] + 10.0 * span], np.float32))
    return np.concatenate(parts).astype(np.float32)


@pytest.mark.parametrize("name", list(TABLES))
def test_channel_query_on_the_device(oracle, capi, name):
    """chan_query<LUT> and chan_query<SEARCH> with the tables staged as k_cull stages them, against the reference: every table
    value, one ulp either side, midpoints, +-inf, NaN and values beyond both ends, as tan_lo and as tan_hi"""
    vertical, H, variant = TABLES[name]
    s = _sensor(oracle, vertical, H)
    tr = make_tracer(capi, s, "projection")
    up, dn, chan, lut_ok = tr.cullTables()
    assert lut_ok == bool(variant & LUT)
    assert np.all(np.diff(up) >= 0) and np.all(np.diff(dn) >= 0) and np.all(dn <= up)
    assert np.array_equal(np.asarray(vertical, np.float32)[chan], np.sort(np.asarray(vertical, np.float32)))
    x = _query_values(up, dn)
    rng = np.random.default_rng(1)
    if x.size <= 400:
        lo, hi = [a.reshape(-1) for a in np.meshgrid(x, x, indexing="ij")]
    else:
        i, j = rng.integers(0, x.size, 60000), rng.integers(0, x.size, 60000)
        lo, hi = np.concatenate([x, x, x[i]]), np.concatenate([x, np.roll(x, -1), x[j]])
    want = cr.chan_query_ref(up, dn, lo, hi)
    ok = ~np.isnan(lo)
    assert np.array_equal(want[ok], cr.chan_query_exists(up, dn, lo[ok], hi[ok]))
    assert 0.05 < want.mean() < 0.95
    lut, search = tr.chanQuery(lo, hi)
    assert np.array_equal(search, want), np.flatnonzero(search != want)[:8]
    if lut_ok:
        assert np.array_equal(lut, want), [(lo[k], hi[k]) for k in np.flatnonzero(lut != want)[:8]]
    else:
        assert np.all(lut == 2)
    tr.close()


def test_every_k_cull_instantiation(oracle, capi):
    """every instantiation launch_project can pick is run and reported by the hook: {look-up, search in LDS, search in global
    memory} x {full turn, sector} x {plain, LS_OPT_COUNT_VISITS} -- the look-up needs the tables in LDS: twelve, not sixteen"""
    v, t = _ground(300, seed=3)
    geoms = [("m", v, t, oracle.IDENTITY_AFFINE)]
    seen = set()
    for table, shard in (("uniform16", (0, 9)), ("triples12", (0, 9)), ("v2049", (0, 1))):
        vertical, H, variant = TABLES[table]
        s = _sensor(oracle, vertical, H)
        for sh in (None, shard):
            for count in (False, True):
                want = variant | (SECTOR if sh else 0) | (COUNT if count else 0)
                got = _case(oracle, capi, s, geoms, shard=sh, floors=False, variant=want, min_hits=1, count=count)
                seen.add(got["m"][2])
    assert len(seen) == 12


# ---- shards ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shard,begin", [((40, 12), 0.0), ((236, 20), 0.0), ((112, 20), -170.0), ((240, 16), -170.0), ((0, 128), 0.0), ((77, 1), 0.0)],
                         ids=["narrow", "up-to-360", "across-0", "across-180", "half-turn", "one-column"])
def test_shards(oracle, capi, shard, begin):
    """uniform16 x 256.  A half turn has no sector (k_cull without SECTOR).  'up-to-360': the raster's last columns, whose padded
    sector crosses 360 degrees; 'across-0' / 'across-180': a raster from -170 to 190 degrees, whose columns 112 .. 131 straddle
    azimuth 0 and whose last ones cross +-180, where atan2 wraps."""
    s = _sensor(oracle, UNIFORM16, 256, begin, begin + 360.0)
    v, t = cr.annulus(14, 180, 9.0, 15.0, amp=0.1, seed=21)   # 4 680 triangles all round the sensor
    half = shard[1] >= 128
    # (the floors of (e) are the full turn's: under a narrow sector nearly every group is rejected and few must survive)
    got = _case(oracle, capi, s, [("m", v, t, oracle.IDENTITY_AFFINE)], shard=shard, floors=half, variant=LUT | LDS | (0 if half else SECTOR),
                min_hits=1)
    ms, kept = got["m"][0], got["m"][1]
    if not half:
        assert 1.0 - kept.mean() >= 0.5


def test_geometry_outside_the_sector(oracle, capi):
    """every k_cull workgroup takes the early out: no survivor, an empty frame"""
    s = _sensor(oracle, UNIFORM16, 256)
    v, t = _ground(2052, seed=22, centre=(-20.0, 0.0))   # around azimuth 180
    geoms = [("m", v, t, oracle.IDENTITY_AFFINE, True)]
    tr = _tracer(capi, s, geoms, shard=(0, 12))                      # azimuth 0 .. 15.5
    surv, var = tr.cullSurvivors("m")
    assert var == LUT | LDS | SECTOR and surv.shape[0] == 0
    perm, gb, bb = tr.downloadCull("m")
    assert cr.box_contains(v, t, perm, gb, bb) == []
    assert not cr.must_survive(oracle, s, v, t, oracle.IDENTITY_AFFINE, perm, (0, 12)).any()
    for mode in (0, 2):
        tr.setOption(capi.LS_OPT_PIPELINE, mode)
        rc, pts, hits = tr.traceScene(mode)
        assert rc == 0 and len(pts) == 0 and len(hits) == 0
    tr.close()


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def test_walls(oracle, capi):
    """a wall ring about the sensor that leans outwards by 1 in 10: the least-squares plane of a group rises 10 m per metre, along x
    where the wall faces x -- beyond the clamp at 8, the box is the plain axis-aligned one -- and 7 m along both x and y on the
    diagonals, where the box stays sheared"""
    s = _sensor(oracle, UNIFORM16, 64)
    v, t = cr.wall_ring(160, 51, 20.0, z_range=(-12.0, 12.0), taper=0.1)   # the rings reach 5.4 m up and down
    got = _case(oracle, capi, s, [("m", v, t, oracle.IDENTITY_AFFINE)], variant=LUT | LDS, min_hits=500)
    gb = got["m"][3]
    flat = np.all(gb[:, 6:8] == 0, axis=1)
    assert np.all(np.abs(gb[:, 6:8]) <= 8.0) and 0.2 < flat.mean() < 0.8 and np.abs(gb[~flat, 6:8]).max() > 6.0


def test_degenerate_and_special_groups(oracle, capi):
    """zero-area and collinear triangles, a group of twelve identical vertices, groups the vertical axis pierces, a group through the
    sensor's origin, between reliefs that keep the scene honest; every special group is found by its vertices"""
    s = _sensor(oracle, UNIFORM16, 256)
    gv, gt = _ground(1200, seed=31)
    p = np.array([7.0, 2.0, -1.0])
    special = {
        "point": np.tile(p, (12, 1)),                                                                                   # hx = hy = hz = 0
        "zero-area": np.array([[5, 5, -1], [5, 5, -1], [6, 5, -1]] * 4, float),
        "collinear": np.array([[4, -6, -1], [5, -6, -1.2], [6, -6, -1.4]] * 4, float) + np.repeat(np.arange(4), 3)[:, None] * [0, 0.2, 0],
        "axis-above": np.array([[-1, -1, 3], [2, -1, 3], [-1, 2, 3]] * 4, float) + np.repeat(np.arange(4), 3)[:, None] * [0, 0, 0.3],
        "axis-below": np.array([[-1, -1, -1.5], [2, -1, -1.5], [-1, 2, -1.5]] * 4, float) + np.repeat(np.arange(4), 3)[:, None] * [0.1, 0, 0],
        "origin": np.array([[-1, -1, -0.2], [1, -1, 0.0], [0, 1.5, 0.2]] * 4, float) + np.repeat(np.arange(4), 3)[:, None] * [0.01, 0, 0],
    }
    blocks = np.concatenate(list(special.values())).astype(np.float32)
    v = np.concatenate([gv, blocks])
    t = np.concatenate([gt, gv.shape[0] + np.arange(blocks.shape[0], dtype=np.uint32).reshape(-1, 3)])
    got = _case(oracle, capi, s, [("m", v, t, oracle.IDENTITY_AFFINE)], variant=LUT | LDS, min_hits=60)
    ms, kept, _, gb, _, perm = got["m"]
    # twelve identical vertices sort next to each other: their group (if the Morton order kept them together) is a point
    first = gt.shape[0]
    for g in range(gb.shape[0]):
        tri = cr.group_triangles(perm, g)
        if np.all((tri >= first) & (tri < first + 4)):
            assert np.all(gb[g, 3:6] < 1e-5) and np.allclose(gb[g, 0:3], p)
    # the groups the axis pierces are kept whatever the rings (no first-order bound next to the axis); the one through the origin
    # is hit by rays of every column
    for k, name in enumerate(special):
        tris = first + 4 * k + np.arange(4)
        groups = np.unique(np.flatnonzero(np.isin(perm, tris)) // 4)
        if name in ("axis-above", "axis-below", "origin"):
            assert kept[groups].all(), name
        if name == "origin":
            assert ms[groups].any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_vertex(oracle, capi, bad):
    """one NaN / infinite vertex: its groups and their block are unbounded (kept, never rejected); the block next door and the
    groups without it are bounded as ever, and the frame is still the oracle's"""
    s = _sensor(oracle, UNIFORM16, 256)
    v, t = _ground(1500, seed=33)
    k = int(t[700, 1])
    v[k, 2] = bad
    got = _case(oracle, capi, s, [("m", v, t, oracle.IDENTITY_AFFINE)], variant=LUT | LDS, min_hits=60)
    ms, kept, _, gb, bb, perm = got["m"]
    touched = np.unique(np.flatnonzero((t[perm] == k).any(axis=1)) // 4)
    unb, b_unb = cr.is_unbounded(gb), cr.is_unbounded(bb)
    assert touched.size >= 1 and unb[touched].all() and kept[touched].all()
    assert unb.sum() == touched.size                                  # nobody else
    assert b_unb.sum() == np.unique(touched // 64).size and b_unb[touched // 64].all()
    assert not b_unb.all()


def test_quads(oracle, capi):
    """a quad geometry: two triangles per element, (v0, v1, v3), (v2, v3, v1); groups and the permutation are over the triangles"""
    s = _sensor(oracle, UNIFORM16, 256)
    nx, ny = 28, 29
    v, _ = cr.relief_grid(nx, ny, 2.8, amp=0.1, seed=41, centre=(12.0, 0.0))
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).reshape(-1)
    q = np.stack([a, a + ny, a + ny + 1, a + 1], axis=1).astype(np.uint32)
    got = _case(oracle, capi, s, [("m", v, q, oracle.IDENTITY_AFFINE)], variant=LUT | LDS, min_hits=30)
    assert got["m"][1].shape[0] == (2 * q.shape[0] + 3) // 4


def _corner_patches(oracle, s, n, seed, z0=-2.0, eps=0.01):
    """n flat rectangles of four triangles (the corners and the middle) on the plane z = z0, each with a corner just outside the point
    where a ray of the raster meets the plane -- alternately the corner furthest from the axis and the nearest: tan(elevation) takes
    its extreme over the rectangle's box AT that corner, so the ring through the point lies in the last few percent of the interval
    the bound gives the group, and a ray of the ring hits it there"""
    rng = np.random.default_rng(seed)
    dirs = oracle.ray_dirs(s).reshape(s.V, s.H, 3).astype(np.float64)
    low = np.flatnonzero(s.vertical < -2.0)
    verts, cells = [], set()
    while len(verts) < n:
        d = dirs[int(rng.choice(low)), int(rng.integers(0, s.H))]
        p = d * (z0 / d[2])
        if min(abs(p[0]), abs(p[1])) < 1.0 or np.hypot(p[0], p[1]) > 30.0 or (round(p[0]), round(p[1])) in cells:
            continue
        cells.add((round(p[0]), round(p[1])))   # (a metre apart: the rectangles are at most 0.2 m long)
        h = rng.uniform(0.04, 0.1, 2)
        out = np.sign(p[:2])
        far = len(verts) % 2 == 0
        corner = p[:2] + out * h * 2.0 * eps * (1.0 if far else -1.0)
        c = corner - out * h * (1.0 if far else -1.0)
        q = [[c[0] + a * h[0], c[1] + b * h[1], z0] for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1))] + [[c[0], c[1], z0]]
        verts.append(np.array([q[i] for tri in ((0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)) for i in tri]))
    v = np.concatenate(verts).astype(np.float32)
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)


def _sharpness(s, A, gb, up, dn):
    """how far into its bound the nearest ring lies: (distance from fc to the nearest channel interval) / (w + rem), float64"""
    q = cr.bound_f64(s, A, gb)
    gap = np.maximum(np.maximum(dn[None, :].astype(np.float64) - q["fc"][:, None], q["fc"][:, None] - up[None, :].astype(np.float64)), 0.0).min(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(q["eps"] < 0.25, gap / (q["w"] + q["rem"]), 0.0)


@pytest.mark.parametrize("pose", ["identity", "scaled"])
def test_rings_in_the_last_tenth_of_the_bound(oracle, capi, pose):
    """(b) where the bound is tight: at least sixty groups that a ray hits and whose nearest ring lies beyond 0.92 of the float64
    half width w + rem from the centre's tangent -- a bound a tenth too narrow rejects them"""
    s = _sensor(oracle, UNIFORM16, 256)
    # (scaled and shifted: the full vertex transform, with the axes kept -- under a rotation the rectangles' boxes are loose and
    # nothing is sharp)
    A = oracle.IDENTITY_AFFINE if pose == "identity" else np.array([2.0, 0, 0, 0.5, 0, 2.0, 0, -1.0, 0, 0, 2.0, 0.25], np.float32)
    gv, t = _corner_patches(oracle, s, 400, seed=17)
    M = np.asarray(A, np.float64).reshape(3, 4)
    v = np.linalg.solve(M[:, :3], (gv.astype(np.float64) - M[:, 3]).T).T.astype(np.float32)
    geoms = [("m", v, t, A, True)]
    tr = _tracer(capi, s, geoms)
    ms, kept, _, gb, _, perm = _check_cull(oracle, tr, s, geoms, floors=False, variant=LUT | LDS)["m"]
    up, dn, _, _ = tr.cullTables()
    sharp = _sharpness(s, A, gb, up, dn)
    assert int((ms & (sharp > 0.92) & (sharp <= 1.0)).sum()) >= 60, np.sort(sharp[ms])[-80:]
    _frames(oracle, capi, tr, s, geoms, None, 300)
    tr.close()


# ---- several geometries ----------------------------------------------------------------------------------------------------------
def _patches(n, tris_each, seed):
    """n reliefs side by side on a ring around the sensor"""
    out = []
    for k in range(n):
        az = 2.0 * np.pi * k / n
        v, t = _ground(tris_each, seed=seed + k, centre=(11.0, 0.0))
        c, sn = np.float32(np.cos(az)), np.float32(np.sin(az))
        v = np.stack([c * v[:, 0] - sn * v[:, 1], sn * v[:, 0] + c * v[:, 1], v[:, 2]], axis=1).astype(np.float32)
        out.append((f"g{k:02d}", v, t, np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.02 * k], np.float32)))
    return out


def test_three_culled_and_two_without_indices(oracle, capi):
    """five geometries, the second and the fourth with vertices and no indices: they hold a geomID and no place in the committed
    scene, so the scene's slots, the cull batch and the geomIDs all count differently"""
    s = _sensor(oracle, UNIFORM16, 256)
    geoms = [(*g, k not in (1, 3)) for k, g in enumerate(_patches(5, 301, 50))]
    tr = _tracer(capi, s, geoms)
    assert [tr.getGeometryId(g[0]) for g in geoms] == [0, 1, 2, 3, 4]
    got = _check_cull(oracle, tr, s, geoms, floors=False, variant=LUT | LDS)
    assert sorted(got) == ["g00", "g02", "g04"]
    _frames(oracle, capi, tr, s, geoms, None, 40)
    tr.close()


@pytest.mark.parametrize("n", [16, 17])
def test_sixteen_and_seventeen_culled(oracle, capi, n):
    """sixteen culled geometries are one k_cull launch; seventeen are more than a launch takes: the frame projects all of them
    unculled (the hook says so), and is the oracle's either way"""
    s = _sensor(oracle, UNIFORM16, 256)
    geoms = [(*g, True) for g in _patches(n, 203, 60)]
    tr = _tracer(capi, s, geoms)
    got = _check_cull(oracle, tr, s, geoms, floors=False, moderate=n == 16, variant=LUT | LDS if n == 16 else UNCULLED)
    if n == 17:
        assert all(kept.all() for _, kept, *_ in got.values())
    else:
        assert sum(int((~kept).sum()) for _, kept, *_ in got.values()) > 0.1 * sum(kept.shape[0] for _, kept, *_ in got.values())
    _frames(oracle, capi, tr, s, geoms, None, 100)
    tr.close()


# ---- poses -----------------------------------------------------------------------------------------------------------------------
def _posed(oracle, A, seed, n=1500):
    """a relief that lies around the sensor's foot AFTER the pose A: its mesh-space vertices are the relief through A's inverse"""
    gv, gt = _ground(n, seed=seed)
    M = np.asarray(A, np.float64).reshape(3, 4)
    v = np.linalg.solve(M[:, :3], (gv.astype(np.float64) - M[:, 3]).T).T
    return v.astype(np.float32), gt


POSES = {
    "rigid": lambda o: o.affine_from_components(np.array((1.5, -2.0, 0.3), np.float32), np.array((0.05, -0.08, 1.1), np.float32)),
    "mirrored-sheared": lambda o: np.array([-1.2, 0.3, 0.0, 0.5, 0.2, 0.8, 0.1, -1.0, 0.1, -0.2, 1.1, 0.2], np.float32),
    "scale-1e3": lambda o: np.array([1e3, 0, 0, 0.5, 0, 1e3, 0, -1.0, 0, 0, 1e3, 0.2], np.float32),
    "scale-1e-3": lambda o: np.array([1e-3, 0, 0, 0.5, 0, 1e-3, 0, -1.0, 0, 0, 1e-3, 0.2], np.float32),
}


@pytest.mark.parametrize("name", list(POSES))
def test_poses(oracle, capi, name):
    s = _sensor(oracle, UNIFORM16, 256, t=(0.3, -0.2, 0.1))
    A = POSES[name](oracle)
    v, t = _posed(oracle, A, seed=len(name))
    # (c) asks for coordinates below 1e3 m: at scale 1e-3 the mesh's are 1.6e4
    _case(oracle, capi, s, [("m", v, t, A)], moderate=name != "scale-1e-3", variant=LUT | LDS, min_hits=60)


def test_rank_deficient_pose(oracle, capi):
    """A flattens the mesh onto the plane z = -2 (its third column is zero)"""
    s = _sensor(oracle, UNIFORM16, 256)
    v, t = _ground(1500, seed=71)
    A = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, -2.0], np.float32)
    _case(oracle, capi, s, [("m", v, t, A)], variant=LUT | LDS, min_hits=60)


GEOREF = {"xyz": (5.0e5, 4.2e6, 300.0), "x-only": (5.0e5, 0.0, 0.0)}


@pytest.mark.parametrize("name", list(GEOREF))
@pytest.mark.parametrize("scene", ["ground-60m", "patch-5cm"])
def test_georeferenced_pose(oracle, capi, name, scene):
    """a mesh in small local coordinates whose pose carries a georeferenced offset, the sensor a few metres from it: the vertex path
    rounds A v at the ulp of the offset (0.5 m at 4.2e6, 0.03 m at 5e5) before it subtracts t, so the triangles the exact test sees
    are not the ideal ones the bound is made for.  Ground 4 - 60 m from the sensor in cells of 3.4 m, and a patch 10 m out in cells
    of 5 cm -- far below the rounding.  (a), (b) and (d) apply."""
    A, s, R = _georef(oracle, name, UNIFORM16, 64 if scene == "ground-60m" else 256)
    if scene == "ground-60m":
        gv, gt = cr.relief_grid(36, 36, 60.0, z0=-0.2, amp=0.3, seed=81, centre=(3.0, -7.0))
    else:
        gv, gt = cr.relief_grid(100, 100, 2.5, z0=-0.2, amp=0.3, seed=81, centre=(11.0, -1.0))
    v = (gv.astype(np.float64) @ R).astype(np.float32)     # R^T g: A v = g + T
    assert np.abs(v).max() < 100.0
    _case(oracle, capi, s, [("m", v, gt, A)], moderate=False, floors=False, variant=LUT | LDS, min_hits=50)


def _georef(oracle, name, vertical=UNIFORM16, H=64):
    T = np.array(GEOREF[name], np.float64)
    A = oracle.affine_from_components(T.astype(np.float32), np.array((0.3, 0.1, -2.2), np.float32))
    s = _sensor(oracle, vertical, H, t=(T + np.array([3.0, -7.0, 1.8])).astype(np.float32))
    return A, s, np.asarray(A, np.float64).reshape(3, 4)[:, :3]


def test_georeferenced_groups_that_the_rounding_moves_onto_a_ring(oracle, capi):
    """The georeferenced pose (5.0e5, 4.2e6, 300) with sixteen geometries of ONE group each -- four triangles a few centimetres
    across, 5 - 15 m from the sensor -- chosen on the CPU, from 3 000 candidates, as those that a ray of the raster hits (the oracle,
    whose vertex path rounds A v to the 0.5 m grid of float32 at 4.2e6) although the float64 bound of the IDEAL box, with half
    again as much room as DESIGN 3.1 gives it, meets no ring: the rounding carried the group onto a ring.  (a), (b) and (d)."""
    A, s, R = _georef(oracle, "xyz", V33, 256)
    rng = np.random.default_rng(5)
    n = 3000
    az, rho = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(5.0, 15.0, n)
    c = np.stack([3.0 + rho * np.cos(az), -7.0 + rho * np.sin(az), np.full(n, -0.2)], axis=1)
    g = c[:, None, :] + rng.uniform(-1.0, 1.0, (n, 12, 3)) * np.array([0.05, 0.05, 0.01])
    v = (g.reshape(-1, 3) @ R).astype(np.float32)
    t = np.arange(12 * n, dtype=np.uint32).reshape(-1, 3)
    ms = cr.must_survive(oracle, s, v, t, A, np.arange(4 * n, dtype=np.uint32))
    boxes = np.array([cr.sheared_box_f64(v[12 * k:12 * k + 12].astype(np.float64)) for k in range(n)])
    boxes[:, 3:6] = boxes[:, 3:6] * 1.00001 + 1e-5
    chi = np.sort(s.vertical.astype(np.float64))
    up, dn = np.tan(np.radians(chi + 2e-4)), np.tan(np.radians(chi - 2e-4))        # the rings with their elevation margin
    q = cr.bound_f64(s, A, boxes)
    half = 1.5 * (q["w"] + q["rem"]) + 1e-5
    meets = ((up[None, :] >= (q["fc"] - half)[:, None]) & (dn[None, :] <= (q["fc"] + half)[:, None])).any(axis=1)
    moved = np.flatnonzero(ms & ~meets & (q["eps"] < 0.2))
    assert moved.size >= 8, moved.size
    pick = np.concatenate([moved, np.flatnonzero(ms & meets)])[:16]
    geoms = [(f"c{i:02d}", v[12 * k:12 * k + 12].copy(), np.arange(12, dtype=np.uint32).reshape(4, 3), A, True) for i, k in enumerate(pick)]
    tr = _tracer(capi, s, geoms)
    got = _check_cull(oracle, tr, s, geoms, moderate=False, floors=False, variant=LUT | LDS)
    assert all(m.all() and k.all() for m, k, *_ in got.values())
    _frames(oracle, capi, tr, s, geoms, None, 16)
    tr.close()


# ---- updates ---------------------------------------------------------------------------------------------------------------------
def test_updates_between_frames(oracle, capi):
    """a vertex upload (bounds stale, rebuilt by the commit), the same topology with permuted coordinates (the Morton order is stale
    but valid: perm stays, the boxes follow the vertices), a pose-only update (the mesh-space boxes travel through the new matrix)"""
    s = _sensor(oracle, UNIFORM16, 256)
    v, t = _ground(1500, seed=91)
    A0 = oracle.IDENTITY_AFFINE
    tr = _tracer(capi, s, [("m", v, t, A0, True)])
    first = _check_cull(oracle, tr, s, [("m", v, t, A0, True)], variant=LUT | LDS)["m"]
    _frames(oracle, capi, tr, s, [("m", v, t, A0, True)], None, 60)
    v2 = v.copy()
    v2[:, 2] += (0.4 * np.sin(0.5 * v[:, 0])).astype(np.float32)
    v2[:, 0] += np.float32(1.5)
    v3 = v[:, [1, 0, 2]].copy()
    A4 = oracle.affine_from_components(np.array((2.0, 1.0, -0.3), np.float32), np.array((0.02, 0.04, 0.7), np.float32))
    for vk, Ak in ((v2, A0), (v3, A0), (v3, A4)):
        if Ak is A0:
            tr.updateGeometry("m", Ak, vk, None)
        else:
            tr.updateGeometryTransform("m", Ak)
        assert tr.commitScene() == 0
        g = [("m", vk, t, Ak, True)]
        now = _check_cull(oracle, tr, s, g, variant=LUT | LDS)["m"]
        assert np.array_equal(now[5], first[5])                       # the order is the topology's
        _frames(oracle, capi, tr, s, g, None, 60)
    assert not np.array_equal(now[1], first[1])
    tr.close()
