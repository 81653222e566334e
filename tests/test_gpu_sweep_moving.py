"""ls_trace_scene_sweep_moving / ls_trace_scene_sweep_moving_host on the MI355X: sweep frames whose geometries move during the
turn.  The degenerate cases against ls_trace_scene_sweep and ls_trace_scene; a real motion against the definition -- the rays
restated in numpy (test_sweep_cpu.restate_rays, test_sweep_moving_cpu.restate_motion_rays), the brute force of test_gpu_rays over
one single-geometry scene per geometry, merged by (t, geom, prim) --; the meaning of a record against a geometry re-posed per
column, exactly for translations and a half turn, within the parity bound for a general rotation; azimuth shards, non-finite
records, two launch batches, unaligned tables, host against device, return codes, the state a call leaves.  Everything is compared
bit for bit unless said otherwise."""
import ctypes

import numpy as np
import pytest

from conftest import make_tracer
from test_gpu_rays import INV, _add, _brute, _ground_ben, _records
from test_gpu_sweep import FILL, _all_rays, _expect, _same_bits, _sweep, _twist_poses
from test_sweep_cpu import IDENTITY_POSE, restate_rays
from test_sweep_moving_cpu import compose, contributions, merge, parity_misses, small_sensor, yaw_case

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, UNKNOWN_GEOMETRY = -2, -3
F = np.float32
MISS = (INV, INV, int(F(-1.0).view(np.uint32)))
TURN = 0.1


# ---- the device entry point ------------------------------------------------------------------------------------------------

def _moving(tr, pose, motions, flags=0, points=True, hits=True, stream=None, skew=0):
    """ls_trace_scene_sweep_moving with capacity exactly the shard's ray count and one canary record behind every buffer; pose None:
    the sensor at rest; motions {geomID: float32 (H, 12)}; skew: every table starts that many bytes past a 16-byte boundary -> (k,
    points uint8 (k, 32) | None, hits uint32 (k, 4) | None); whatever lies past record k, the canary included, must still hold the
    fill pattern"""
    import torch
    n = tr.getTotalRays()

    def table(a):
        raw = np.ascontiguousarray(a, np.float32).view(np.uint8).reshape(-1)
        buf = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        buf[skew:skew + raw.size] = torch.from_numpy(raw.copy()).to("cuda:0")
        return buf

    d_pose = None if pose is None else table(pose)
    d_tabs = {g: table(t) for g, t in motions.items()}
    p = torch.full(((n + 1) * 32,), FILL, dtype=torch.uint8, device="cuda:0") if points else None
    h = torch.full(((n + 1) * 16,), FILL, dtype=torch.uint8, device="cuda:0") if hits else None
    c = torch.full((16,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = tr.traceSweepMovingDevice(0 if pose is None else d_pose.data_ptr() + skew, 0 if pose is None else pose.shape[0],
                                   {g: b.data_ptr() + skew for g, b in d_tabs.items()}, c.data_ptr(), n, p.data_ptr() if points else 0,
                                   h.data_ptr() if hits else 0, flags=flags, stream=stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    cw = c.cpu().numpy()
    k = int(cw[:4].view(np.uint32)[0])
    assert 0 <= k <= n and np.all(cw[4:] == FILL)
    out = [k, None, None]
    if points:
        a = p.cpu().numpy().reshape(n + 1, 32)
        assert np.all(a[k:] == FILL), "a point record written past the count"
        out[1] = a[:k].copy()
    if hits:
        a = h.cpu().numpy().reshape(n + 1, 16)
        assert np.all(a[k:] == FILL), "a hit record written past the count"
        out[2] = a[:k].copy().view(np.uint32).reshape(k, 4)
    return tuple(out)


def _dense(h, n):
    """packed ls_hit records -> one record per ray of the full raster"""
    d = np.zeros((n, 4), np.uint32)
    d[:, 0] = np.arange(n)
    d[:, 1:] = MISS
    d[h[:, 0]] = h
    return d


def _identity_tables(tr, s, names=("ground", "face")):
    return {tr.L.ls_geometry_id(tr.h, n.encode()): np.tile(IDENTITY_POSE, (s.H, 1)) for n in names}


_cache = {}


def _scene(oracle, capi, sensors, meshes):
    """XT-32 0000 over ground + ben: the sensor on the sweep tests' twist, ground at rest, ben on a constant twist about its own
    centroid (about 15 m/s and 0.5 rad/s) -- the poses, ben's motion table, the sweep's rays and every geometry's contribution by
    definition: computed once, shared by the tests that need them, never changed"""
    if "scene" not in _cache:
        s = sensors["0000"]
        ml = [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], oracle.IDENTITY_AFFINE)]
        pose = _twist_poses(capi, s)
        rays = _all_rays(oracle, s, pose)
        pivot = oracle.transform_vertices(meshes["ben"][0], oracle.IDENTITY_AFFINE, s).astype(np.float64).mean(0)
        motion = capi.motion_constant_twist((12.0, -9.0, 0.5), (0.05, -0.1, 0.5), pivot, 0.0, TURN / s.H, s.H)
        contrib = contributions(oracle, _brute, s, ml, rays, {1: motion})
        for a in (pose, rays, motion, *contrib.values()):
            a.setflags(write=False)
        _cache["scene"] = (s, ml, pose, rays, motion, contrib)
    return _cache["scene"]


# ---- 1. the degenerate cases -------------------------------------------------------------------------------------------------

def test_no_motion_and_identity_tables_reproduce_the_sweep_and_the_frame(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    pose = _twist_poses(capi, s)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    ident = _identity_tables(tr, s)
    assert sorted(ident) == [0, 1]
    for flags in (0, capi.LS_SWEEP_DESKEW):
        k, p, h, _ = _sweep(tr, pose, flags=flags)
        assert k > 1000
        for motions in ({}, ident, {1: ident[1]}):
            k2, p2, h2 = _moving(tr, pose, motions, flags=flags)
            assert k2 == k and np.array_equal(h2, h) and _same_bits(p2, p)
    # no pose table and no motions: the frame (the reference's 1781 points); LS_SWEEP_DESKEW changes nothing at rest
    rc, pts, hits = tr.traceScene(0)
    assert rc == 0 and len(pts) == 1781
    for motions in ({}, ident):
        for flags in (0, capi.LS_SWEEP_DESKEW):
            k, p, h = _moving(tr, None, motions, flags=flags)
            assert k == 1781 and _same_bits(p, np.asarray(pts).reshape(-1, 32)) and np.array_equal(h, _records(hits))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 2. the definition -------------------------------------------------------------------------------------------------------

def test_moving_ben_equals_the_merged_brute_force(oracle, capi, sensors, meshes):
    s, ml, pose, rays, motion, contrib = _scene(oracle, capi, sensors, meshes)
    dense = merge(contrib)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for flags in (0, capi.LS_SWEEP_DESKEW):
        k, p, h = _moving(tr, pose, {1: motion}, flags=flags)
        want_h, want_p = _expect(oracle, s, dense, rays, deskew=bool(flags))
        assert k == len(want_h) and set(want_h[:, 1]) == {0, 1}
        assert np.array_equal(h, want_h)
        assert _same_bits(p, want_p)
    # the motion matters: the static sweep's records on ben differ
    ks, ps, hs, _ = _sweep(tr, pose)
    static = _dense(hs, s.V * s.H)
    on_ben = (dense[:, 1] == 1) | (static[:, 1] == 1)
    assert np.count_nonzero(np.any(static != dense, axis=1) & on_ben) >= 1
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 3. the meaning of a record, exactly ---------------------------------------------------------------------------------------

def _box():
    """a closed box of half size 1 about the origin: corners at +-1, 12 triangles"""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([tri for a, b, c, d in q for tri in ((a, b, c), (a, c, d))], np.uint32)


PLATE = (np.float32([[12, -12, -12], [12, 12, -12], [12, 12, 12], [12, -12, 12]]), np.uint32([[0, 1, 2], [0, 2, 3]]))


def _reposed_per_column(tr, s, name, A0, motion, rays):
    """the reference of tests 3 and 4: for every column h the geometry re-posed to [Q A | Q a + c], committed, and that column's
    rays through ls_trace_rays_host -> dense records; the committed pose is restored"""
    n, cols = s.V * s.H, np.arange(s.V * s.H) % s.H
    ref = np.zeros((n, 4), np.uint32)
    for h in range(s.H):
        tr.updateGeometryTransform(name, compose(motion[h], A0))
        assert tr.commitScene() == 0
        mine = np.nonzero(cols == h)[0]
        rc, hits = tr.traceRays(rays[mine])
        assert rc == 0
        ref[mine] = _records(hits)
        ref[mine, 0] = mine
    tr.updateGeometryTransform(name, A0)
    assert tr.commitScene() == 0
    return ref


@pytest.mark.parametrize("half_turn", [False, True])
def test_a_record_means_the_geometry_reposed_exactly(oracle, capi, half_turn):
    """V = 8, H = 16, the sensor frame the world frame, the sensor at rest; a box whose corners are multiples of 2^-4 below 16, a
    plate behind it; c_h = (h / 16, -h / 32, 0), Q the identity or a half turn about z.  Every sum of corners and offsets is exact
    and a half turn only negates components, so geom, prim and the bits of t equal those of the box re-posed to [Q | Q a + c]."""
    s = small_sensor(oracle, begin=4.0, end=36.0)
    n = s.V * s.H
    Q = np.diag([-1.0, -1.0, 1.0]) if half_turn else np.eye(3)
    a = np.float32([-6, -2, 0]) if half_turn else np.float32([6, 2, 0])      # Q a = (6, 2, 0): in front of the sensor either way
    A0 = np.float32([1, 0, 0, a[0], 0, 1, 0, a[1], 0, 0, 1, a[2]])
    motion = np.zeros((s.H, 3, 4), np.float32)
    motion[:, :, :3] = Q
    motion[:, 0, 3], motion[:, 1, 3] = np.arange(s.H) / 16.0, -np.arange(s.H) / 32.0
    motion = motion.reshape(s.H, 12)
    rays = restate_rays(oracle.ray_dirs(s), np.tile(IDENTITY_POSE, (n, 1)))
    tr = make_tracer(capi, s)
    box = _box()
    _add(tr, "box", *box)
    _add(tr, "plate", *PLATE)
    tr.updateGeometry("box", A0, *box)
    tr.updateGeometry("plate", oracle.IDENTITY_AFFINE, *PLATE)
    assert tr.commitScene() == 0
    ref = _reposed_per_column(tr, s, "box", A0, motion, rays)
    assert np.count_nonzero(ref[:, 1] == 0) >= 16 and np.count_nonzero(ref[:, 1] == 1) >= 16
    assert len(set(ref[ref[:, 1] == 0, 0] % s.H)) >= 8            # the box is seen in many columns, each with its own offset
    k, p, h = _moving(tr, None, {0: motion})
    got = _dense(h, n)
    assert np.array_equal(got[:, 1:], ref[:, 1:])
    # forward against inverse, Q^T (o - c) against Q^T o - c: the box moved the other way is another cloud
    back = motion.copy()
    back[:, [3, 7]] = -back[:, [3, 7]]
    assert not np.array_equal(_dense(_moving(tr, None, {0: back})[2], n)[:, 1:], ref[:, 1:])
    tr.close()


# ---- 4. the meaning of a general rotation, within the parity bound --------------------------------------------------------------

def test_general_rotation_equals_reposing(oracle, capi, meshes):
    """ben yawing by 0.4 rad over the turn while it drives on, against ben re-posed per column: (geom, prim) agree and |t - t_ref|
    <= 1e-4 t_ref for all rays but at most 1 %.  The reference alone (both sides through the oracle's brute force,
    test_sweep_moving_cpu.test_definition_against_reposed_geometry_in_the_oracle_alone) differs in 0 of 128 rays, and so does the
    device: measured share 0 %."""
    s, ml, motion, rays = yaw_case(oracle, capi, meshes)
    n = s.V * s.H
    tr = make_tracer(capi, s)
    _add(tr, "ben", *ml[0][1:3])
    _add(tr, "plate", *ml[1][1:3])
    tr.updateGeometry("ben", ml[0][3], *ml[0][1:3])
    tr.updateGeometry("plate", ml[1][3], *ml[1][1:3])
    assert tr.commitScene() == 0
    ref = _reposed_per_column(tr, s, "ben", ml[0][3], motion, rays)
    assert np.count_nonzero(ref[:, 1] == 0) >= n // 2 and np.count_nonzero(ref[:, 1] == 1) >= 8
    got = _dense(_moving(tr, None, {0: motion})[2], n)
    miss = np.count_nonzero(parity_misses(got, ref))
    print("rays outside the parity bound:", miss, "of", n)
    assert miss <= n // 100
    # a transposed Q misses by a wide margin
    wrong = motion.copy().reshape(-1, 3, 4)
    wrong[:, :, :3] = wrong[:, :, :3].transpose(0, 2, 1)
    bad = _dense(_moving(tr, None, {0: wrong.reshape(-1, 12)})[2], n)
    assert np.count_nonzero(parity_misses(bad, ref)) > n // 4
    tr.close()


# ---- 5. shards -----------------------------------------------------------------------------------------------------------------

def test_two_unaligned_shards_are_the_full_turn(oracle, capi, sensors, meshes):
    s, ml, pose, rays, motion, contrib = _scene(oracle, capi, sensors, meshes)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for flags in (0, capi.LS_SWEEP_DESKEW):
        tr.setShard(0, s.H)
        kf, pf, hf = _moving(tr, pose, {1: motion}, flags=flags)
        want_h, want_p = _expect(oracle, s, merge(contrib), rays, deskew=bool(flags))
        assert np.array_equal(hf, want_h) and _same_bits(pf, want_p)
        # two shards that part the columns in which ben is seen; neither width is a multiple of 64, the second starts past column 0
        ben_cols = np.unique(hf[hf[:, 1] == 1, 0] % s.H)
        split = int(ben_cols[len(ben_cols) // 2])
        assert len(ben_cols) >= 4 and split % 64 != 0 and (s.H - split) % 64 != 0
        total = 0
        for first, count in ((0, split), (split, s.H - split)):
            tr.setShard(first, count)
            assert tr.getTotalRays() == s.V * count
            k, p, h = _moving(tr, pose, {1: motion}, flags=flags)      # the tables are still indexed by the global column
            col = hf[:, 0] % s.H
            inside = (col >= first) & (col < first + count)
            assert 100 < np.count_nonzero(inside) < kf and np.any(hf[inside, 1] == 1)
            assert k == np.count_nonzero(inside) and np.array_equal(h, hf[inside]) and _same_bits(p, pf[inside])
            total += k
        assert total == kf
    tr.close()


# ---- 6. non-finite records ---------------------------------------------------------------------------------------------------

def test_nan_record_hides_that_geometry_in_that_column_only(oracle, capi, sensors, meshes):
    s, ml, pose, rays, motion, contrib = _scene(oracle, capi, sensors, meshes)
    n, cols = s.V * s.H, np.arange(s.V * s.H) % s.H
    full = merge(contrib)
    ben_per_col = np.bincount(full[full[:, 1] == 1, 0] % s.H, minlength=s.H)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for col, entry, bad_value in ((int(np.argmax(ben_per_col)), 5, np.nan), (int(np.argmax(ben_per_col)), 3, np.inf),
                                  (int(np.nonzero(ben_per_col)[0][0]), 0, np.nan)):
        assert ben_per_col[col] > 0
        bad = motion.copy()
        bad[col, entry] = bad_value
        want = merge(contrib, hidden={1: cols == col})
        assert np.all(want[cols == col, 1] != 1) and np.any(want[cols == col, 1] == 0)      # the ground is still hit there
        assert np.array_equal(want[cols != col], full[cols != col])
        k, p, h = _moving(tr, pose, {1: bad})
        want_h, want_p = _expect(oracle, s, want, rays)
        assert k == len(want_h) and np.array_equal(h, want_h) and _same_bits(p, want_p)
    # a NaN sensor pose still yields misses for the whole column
    col = int(np.argmax(ben_per_col))
    bad_pose = pose.copy()
    bad_pose[col, 6] = np.nan
    want = full.copy()
    want[cols == col, 1:] = MISS
    k, p, h = _moving(tr, bad_pose, {1: motion})
    want_h, want_p = _expect(oracle, s, want, rays)
    assert k == len(want_h) and np.array_equal(h, want_h) and _same_bits(p, want_p)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 7. seventeen geometries: two launch batches ---------------------------------------------------------------------------------

def _seventeen(oracle, capi, s):
    """seventeen small plates (6 x 4 cells, tilted, posed) around the sensor: 1 .. 15 on a ring 10 m away, at rest; 0 and 16 nearer,
    in front of 5 and of 8, each on a twist of its own (about 20 m/s across the line of sight, turning about its centroid).
    Geometry 16 belongs to the second launch batch.  -> (geometries, {geomID: motion table})"""
    xs, ys = np.meshgrid(np.linspace(-3, 3, 7), np.linspace(-2, 2, 5), indexing="xy")
    pv = np.stack([xs, ys, 0.3 * xs], -1).reshape(-1, 3).astype(np.float32)
    pq = np.array([[j * 7 + i, j * 7 + i + 1, j * 7 + i + 8, j * 7 + i + 7] for j in range(4) for i in range(6)], np.uint32)
    pt = oracle.quads_to_triangles(pq)
    rng = np.random.default_rng(17)
    geoms, motions = [], {}
    for k in range(17):
        at, dist = {0: (5, 6.0), 16: (8, 6.0)}.get(k, (k, 10.0))
        ang = 2 * np.pi * at / 15
        lin = np.float32([s.t[0] + dist * np.cos(ang), s.t[1] + dist * np.sin(ang), s.t[2] - 1.0 + rng.uniform(-0.5, 0.5)])
        A = oracle.affine_from_components(lin, np.float32([rng.uniform(-0.3, 0.3), 1.2 + rng.uniform(-0.3, 0.3), ang]))
        geoms.append((f"g{k}", pv, pt, A))
        if k in (0, 16):
            c = oracle.transform_vertices(pv, A, s).astype(np.float64).mean(0)
            across = np.cross([0.0, 0.0, 1.0], c / np.linalg.norm(c)) * (20.0 if k == 0 else -20.0)
            motions[k] = capi.motion_constant_twist(across, (0.2, -0.1, 1.5 if k == 0 else -1.0), c, -0.5 * TURN, TURN / s.H, s.H)
    return geoms, motions


def test_seventeen_geometries_two_batches(oracle, capi, sensors):
    s = sensors["0000"]
    geoms, motions = _seventeen(oracle, capi, s)
    ml = [(i, v, e, A) for i, (name, v, e, A) in enumerate(geoms)]
    pose = _twist_poses(capi, s)
    rays = _all_rays(oracle, s, pose)
    # 0 and 16 by definition; 1 .. 15 are at rest and see one and the same record: one pass over their union -- ascending global
    # id, a strictly closer hit replaces -- is their merge
    contrib = contributions(oracle, _brute, s, [ml[0], ml[16]], rays, motions)
    rest = _brute(oracle, oracle.assemble_scene(s, ml[1:16]), rays)
    dense = merge({0: contrib[0], 1: rest, 16: contrib[16]})
    seen = set(dense[:, 1]) - {INV}
    assert {0, 16} <= seen and len(seen) >= 12                    # both batches
    # a moving geometry passes in front of a static one of a higher id (0 before 5) and of a lower id (16 before 8)
    assert np.count_nonzero((dense[:, 1] == 0) & (rest[:, 1] == 5)) >= 5
    assert np.count_nonzero((dense[:, 1] == 16) & (rest[:, 1] == 8)) >= 5
    tr = make_tracer(capi, s)
    for name, v, e, A in geoms:
        _add(tr, name, v, e)
        tr.updateGeometry(name, A, v, e)
    assert tr.commitScene() == 0
    for flags in (0, capi.LS_SWEEP_DESKEW):
        k, p, h = _moving(tr, pose, motions, flags=flags)
        want_h, want_p = _expect(oracle, s, dense, rays, deskew=bool(flags))
        assert k == len(want_h) and np.array_equal(h, want_h) and _same_bits(p, want_p)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 8. alignment, the host variant, a caller stream ---------------------------------------------------------------------------

def test_unaligned_tables_host_variant_and_caller_stream(oracle, capi, sensors, meshes):
    import torch
    s, ml, pose, rays, motion, contrib = _scene(oracle, capi, sensors, meshes)
    dense = merge(contrib)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    ident = np.tile(IDENTITY_POSE, (s.H, 1))
    qs = torch.cuda.Stream()
    for first, count in ((0, s.H), (37, 61)):
        tr.setShard(first, count)
        for flags in (0, capi.LS_SWEEP_DESKEW):
            want_h, want_p = _expect(oracle, s, dense, rays, deskew=bool(flags))
            inside = (want_h[:, 0] % s.H >= first) & (want_h[:, 0] % s.H < first + count)
            for skew, stream in ((0, None), (4, None), (12, None), (4, qs.cuda_stream)):      # 4-byte but not 16-byte aligned tables
                k, p, h = _moving(tr, pose, {1: motion, 0: ident}, flags=flags, skew=skew, stream=stream)
                assert k == np.count_nonzero(inside) and np.array_equal(h, want_h[inside]) and _same_bits(p, want_p[inside])
            for want_pts in (True, False):
                for want_hits in (True, False):
                    rc, kh, ph, hh = tr.traceSweepMoving(pose, {1: motion}, flags=flags, points=want_pts, hits=want_hits)
                    assert rc == 0 and kh == k
                    assert (ph is None) if not want_pts else _same_bits(ph, p)
                    assert (hh is None) if not want_hits else np.array_equal(_records(hh), h)
    # the host variant at rest and without motions: the frame
    tr.setShard(0, s.H)
    rc, kh, ph, hh = tr.traceSweepMoving(None, {})
    rc2, pts, hits = tr.traceScene(0)
    assert rc == 0 and rc2 == 0 and kh == len(pts) == 1781 and _same_bits(ph, np.asarray(pts).reshape(-1, 32)) and np.array_equal(_records(hh), _records(hits))
    tr.close()
    t2 = make_tracer(capi, s)
    rc, k, p, h = t2.traceSweepMoving(pose, {})
    assert rc == -1 and k == 0 and len(p) == 0 and len(h) == 0
    t2.close()


# ---- 9. return codes -------------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order(oracle, capi, sensors, meshes):
    """every refusal of the header, alone and together with the one after it (the earlier one answers: ls_last_error says which),
    with nothing written.  A removal commits the remaining scene itself (ls_remove_geometry), so LS_ERR_NOT_COMMITTED -- a layout
    entry whose geometry is gone -- is not reachable through the public entry points, for this call as for ls_trace_scene_sweep:
    the call follows the remaining scene, and a motion that names the removed geometry is LS_ERR_UNKNOWN_GEOMETRY."""
    import torch
    s = sensors["0000"]
    n = s.V * s.H
    pose = _twist_poses(capi, s)
    ident = np.tile(IDENTITY_POSE, (s.H, 1))
    d_pose = torch.from_numpy(pose).to("cuda:0")
    d_tab = torch.from_numpy(ident).to("cuda:0")
    bufs = {k: torch.full((size,), FILL, dtype=torch.uint8, device="cuda:0") for k, size in (("p", n * 32 + 64), ("h", n * 16 + 64), ("c", 64))}
    torch.cuda.synchronize()
    P, H_, C_ = (bufs[k].data_ptr() for k in "phc")
    host_n = ctypes.c_uint32(0xABABABAB)
    host_p, host_h = np.full((n, 32), FILL, np.uint8), np.full((n, 16), FILL, np.uint8)

    def untouched():
        torch.cuda.synchronize()
        return all(np.all(b.cpu().numpy() == FILL) for b in bufs.values()) and host_n.value == 0xABABABAB and \
            np.all(host_p == FILL) and np.all(host_h == FILL)

    def motions(entries):
        arr = (capi.GeometryMotion * max(1, len(entries)))()
        for m, (g, r, t) in zip(arr, entries):
            m.geom, m.reserved, m.col_motion = g, r, t
        return arr

    TAB, HTAB = d_tab.data_ptr(), ident.ctypes.data
    base = dict(pose=d_pose.data_ptr(), n_cols=s.H, entries=[(1, 0, TAB)], null_motions=False, n_motions=None, flags=0, p=P, h=H_, c=C_, cap=n)

    def device(tr, **kw):
        a = {**base, **kw}
        nm = len(a["entries"]) if a["n_motions"] is None else a["n_motions"]
        return tr.L.ls_trace_scene_sweep_moving(tr.h, None, a["pose"], a["n_cols"], None if a["null_motions"] else motions(a["entries"]), nm,
                                                a["flags"], a["p"], a["h"], a["c"], a["cap"])

    def host(tr, **kw):
        a = {**dict(base, pose=pose.ctypes.data, entries=[(1, 0, HTAB)], p=host_p.ctypes.data, h=host_h.ctypes.data, c=ctypes.byref(host_n)), **kw}
        nm = len(a["entries"]) if a["n_motions"] is None else a["n_motions"]
        return tr.L.ls_trace_scene_sweep_moving_host(tr.h, a["pose"], a["n_cols"], None if a["null_motions"] else motions(a["entries"]), nm,
                                                     a["flags"], a["p"], a["h"], a["c"], a["cap"])

    tr = make_tracer(capi, s)
    assert (device(tr, entries=[]), host(tr, entries=[])) == (-1, -1) and untouched()          # before a commit
    _add(tr, "ground", *meshes["ground"])
    _add(tr, "face", *meshes["ben"])
    assert (device(tr), host(tr)) == (-1, -1) and untouched()                                  # geometries without a commit
    assert device(tr, cap=n - 1) == INVALID_ARGUMENT and device(tr, entries=[(7, 0, TAB)]) == -1 and untouched()   # 10 before 11 before 12
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
    tr.updateGeometry("face", oracle.IDENTITY_AFFINE, *meshes["ben"])
    assert tr.commitScene() == 0
    # the refusals 2 .. 10 in the header's order: (arguments, what ls_last_error says); every one is combined with the next
    steps = [
        (dict(c=None), "null count"),
        (dict(n_cols=s.H - 1), "one pose per azimuth column"),
        (dict(flags=2), "unknown sweep flags"),
        (dict(null_motions=True, n_motions=1), "null motions"),
        (dict(entries=[(1, 0, None)]), "without a table"),
        (dict(entries=[(1, 1, TAB)]), "reserved"),
        (dict(entries=[(1, 0, TAB), (1, 0, TAB)]), "two motions"),
        (dict(p=P + 8), "aligned"),
        (dict(cap=n - 1), "capacity"),
    ]
    together = {3: dict(null_motions=True, n_motions=1, entries=[]),               # NULL motions, and a table that would be NULL
                4: dict(entries=[(1, 1, None)]),                                   # a NULL table in an entry whose reserved is set
                5: dict(entries=[(1, 1, TAB), (1, 0, TAB)])}                       # reserved set in one of two entries for one geometry
    for i, (kw, says) in enumerate(steps):
        assert device(tr, **kw) == INVALID_ARGUMENT and says in tr.last_error(), (i, tr.last_error())
        if i + 1 < len(steps):
            both = together.get(i, {**kw, **steps[i + 1][0]})
            assert device(tr, **both) == INVALID_ARGUMENT and says in tr.last_error(), (i, tr.last_error())
    more = [
        device(tr, n_cols=s.H + 1), device(tr, pose=None, n_cols=s.H), device(tr, pose=None, n_cols=1),       # the table and n_cols
        device(tr, flags=0x80000001),
        device(tr, entries=[(0, 0, TAB), (1, 0, TAB), (2, 0, TAB)]),                                          # more motions than geometries
        device(tr, h=H_ + 8), device(tr, c=C_ + 2), device(tr, pose=d_pose.data_ptr() + 2), device(tr, entries=[(1, 0, TAB + 2)]),
        host(tr, c=None), host(tr, n_cols=s.H - 1), host(tr, flags=4), host(tr, null_motions=True, n_motions=1),
        host(tr, entries=[(1, 0, None)]), host(tr, entries=[(1, 7, HTAB)]), host(tr, entries=[(0, 0, HTAB), (0, 0, HTAB)]), host(tr, cap=n - 1),
    ]
    assert more == [INVALID_ARGUMENT] * len(more) and untouched()
    # 12, after the commit state: a geometry that is not in the committed scene
    assert device(tr, entries=[(2, 0, TAB)]) == UNKNOWN_GEOMETRY and host(tr, entries=[(0xFFFFFFFF, 0, HTAB)]) == UNKNOWN_GEOMETRY and untouched()
    assert tr.last_error()
    # a shard: the capacity that counts is the shard's, the tables keep H records
    tr.setShard(10, 20)
    assert device(tr, cap=s.V * 20 - 1) == INVALID_ARGUMENT and device(tr, n_cols=20) == INVALID_ARGUMENT and untouched()
    tr.setShard(0, s.H)
    # the handle still answers; host memory may have any alignment
    k, p, hh = _moving(tr, pose, {1: ident})
    ks, ps, hs, _ = _sweep(tr, pose)
    assert k == ks and np.array_equal(hh, hs) and _same_bits(p, ps)
    odd = np.zeros(s.H * 48 + 1, np.uint8)
    odd[1:] = ident.view(np.uint8).reshape(-1)
    assert host(tr, entries=[(1, 0, odd.ctypes.data + 1)]) == 0 and host_n.value == k
    host_n.value = 0xABABABAB
    host_p[:], host_h[:] = FILL, FILL
    # a removal commits the remaining scene: the call follows it, the removed geometry is unknown, an emptied scene is -1
    assert tr.removeGeometry("face") >= 0
    assert device(tr, entries=[(1, 0, TAB)]) == UNKNOWN_GEOMETRY and untouched()
    k2, p2, h2 = _moving(tr, pose, {0: ident})
    assert 0 < k2 < k and np.all(h2[:, 1] == 0)
    assert tr.removeGeometry("ground") >= 0
    assert (device(tr, entries=[]), host(tr, entries=[])) == (-1, -1) and untouched()
    tr.close()


def test_open_frame_graph_is_refused_first(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0001"]
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    tr.setOption(capi.LS_OPT_FRAME_GRAPH, 1)
    _ground_ben(tr, oracle, meshes)
    n = s.V * s.H
    p, h, c = (torch.zeros(32 * n, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * n, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), n)
    out = torch.full((n * 16 + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    host_n = ctypes.c_uint32(7)
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != 0   # the frame is being captured: the graph is open
    # (a NULL count as well: the open graph answers first)
    assert L.ls_trace_scene_sweep_moving(tr.h, None, None, 0, None, 0, 0, None, out.data_ptr() + 16, out.data_ptr(), n) == INVALID_ARGUMENT
    assert L.ls_trace_scene_sweep_moving(tr.h, None, None, 0, None, 0, 0, None, None, None, n) == INVALID_ARGUMENT and "frame graph" in tr.last_error()
    assert L.ls_trace_scene_sweep_moving_host(tr.h, None, 0, None, 0, 0, None, None, ctypes.byref(host_n), n) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == FILL) and host_n.value == 7
    # the frame went out, and the handle answers again: at rest and without motions, that frame
    k_frame = int(c[0].item())
    assert k_frame > 0
    k, _, hh = _moving(tr, None, {})
    assert k == k_frame and _same_bits(hh, h.cpu().numpy()[:16 * k].view(np.uint32).reshape(k, 4))
    tr.close()


# ---- 10. the state a call leaves ---------------------------------------------------------------------------------------------

def test_state_after_a_call(oracle, capi, sensors, meshes):
    s, ml, pose, rays, motion, contrib = _scene(oracle, capi, sensors, meshes)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    rc, pts0, hits0 = tr.traceScene(0)
    assert rc == 0 and len(pts0) == 1781
    pts0, hits0 = np.array(pts0), np.array(hits0)
    k, p, h = _moving(tr, pose, {1: motion})
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 2
    want_h, want_p = _expect(oracle, s, merge(contrib), rays)
    assert np.array_equal(h, want_h) and _same_bits(p, want_p)
    rc, pts1, hits1 = tr.traceScene(1)
    assert rc == 0 and _same_bits(np.asarray(pts1), pts0) and np.array_equal(_records(hits1), _records(hits0))
    k2, p2, h2 = _moving(tr, pose, {1: motion})
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0 and np.array_equal(h2, h)
    # a commit after which only a pose changed builds nothing: the hierarchies are in mesh space
    A = oracle.affine_from_components(np.float32([0.4, -0.3, 0.1]), np.float32([0.0, 0.0, 0.6]))
    tr.updateGeometryTransform("face", A)
    assert tr.commitScene() == 0
    k3, p3, h3 = _moving(tr, pose, {1: motion})
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0 and k3 > 1000 and not np.array_equal(h3, h)
    tr.updateGeometryTransform("face", oracle.IDENTITY_AFFINE)
    assert tr.commitScene() == 0
    rc, pts2, hits2 = tr.traceScene(2)
    assert rc == 0 and _same_bits(np.asarray(pts2), pts0) and np.array_equal(_records(hits2), _records(hits0))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
