"""ls_hit_velocities / ls_hit_velocities_host on the MI355X: the surface velocity, the velocity of the sensor's origin and the Doppler
range rate at the hit records of a frame.  A real motion against the definition restated on the host -- the rays and the validity as
test_gpu_attr_moving._define restates them, the values through ls_debug_hit_velocity --; the valid bits against
ls_hit_attributes_moving's, record for record; pure translations, no twists and a snapshot frame exactly; the meaning of a record
against float64 finite differences of the material point's trajectory and of its range; a sensor that only spins; count words,
optional outputs, unaligned tables, streams, host against device, shards, many geometries, block edges, refusals.  Everything is
compared bit for bit unless said otherwise.  The sensor is V = 8, H = 16 (test_sweep_moving_cpu.small_sensor) unless noted."""
import ctypes

import numpy as np
import pytest

from conftest import make_tracer
from test_attr_moving_cpu import box
from test_gpu_attr import _hits_u32
from test_gpu_attr_moving import _attr_device, _define, _dev, _tables
from test_gpu_rays import INV, _add, _records
from test_gpu_sweep import FILL
from test_gpu_sweep_moving import _moving
from test_sweep_cpu import IDENTITY_POSE
from test_sweep_moving_cpu import small_sensor
from test_velocity_cpu import EPS, QNAN, body_motion, same_floats, velocity_bound

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, UNKNOWN_GEOMETRY, OUT_OF_RANGE = -2, -3, -9
F = np.float32
TURN = 0.1
KBLOCK = 256                                                     # csrc/ls_device.h: kBlock
# the definition frame: the sensor drives and yaws, the box turns about a pivot off its centre while it drives on, the ground rests
SENSOR_LIN, SENSOR_ANG = (2.0, -1.0, 0.1), (0.02, -0.03, 0.3)
BOX_LIN, BOX_ANG, BOX_PIVOT = (8.0, -5.0, 0.5), (0.1, -0.2, 1.5), (6.5, 2.5, 0.2)
BOX_POSE = F([1.5, 0, 0, 6, 0, 1.5, 0, 2, 0, 0, 1.5, 0])         # half size 1.5 at (6, 2, 0)
GROUND = (F([[0, -10, -1.5], [40, -10, -1.5], [40, 30, -1.5], [0, 30, -1.5]]), np.uint32([[0, 1, 2], [0, 2, 3]]))
BOX, GND = 0, 1                                                  # geomIDs


# ---- the scene and the definition, restated ---------------------------------------------------------------------------------------

def _box_ground(tr, oracle, box_pose=BOX_POSE):
    bx = box()
    assert _add(tr, "box", *bx) == BOX and _add(tr, "ground", *GROUND) == GND
    tr.updateGeometry("box", box_pose, *bx)
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *GROUND)
    assert tr.commitScene() == 0
    return [(BOX, *bx, box_pose), (GND, *GROUND, oracle.IDENTITY_AFFINE)]


def define_velocities(capi, scene, dirs, H, hits, pose, motions, sensor_twist, twists):
    """per hit: the ray its column cast and the valid bit as test_gpu_attr_moving._define restates them (the ray the geometry saw,
    the named triangle through ls_debug_hit_attributes_on_triangle, t bit-equal to hit.t), the values of a valid record through
    ls_debug_hit_velocity with the column's twist records; an invalid one is zeros -> (records uint32 (n, 8), the radial array
    uint32 (n,) with 0x7FC00000 for an invalid record, the rays the columns cast float32 (n, 8))"""
    h = _hits_u32(hits)
    attr, cast = _define(capi, scene, dirs, H, h, pose, motions, False)
    out = np.zeros((h.shape[0], 8), np.uint32)
    radial = np.full(h.shape[0], QNAN, np.uint32)
    for i in np.nonzero(attr[:, 7] == 1)[0]:
        col, geom = int(h[i, 0]) % H, int(h[i, 1])
        out[i] = capi.hit_velocity(cast[i], h[i, 3:4].view(F)[0], None if sensor_twist is None else sensor_twist[col],
                                   twists[geom][col] if geom in twists else None)
        radial[i] = out[i, 3]
    return out, radial, cast


def _twist_tables(sensor_twist, twists, skew=0):
    """the twist tables in device memory, each `skew` bytes past a 16-byte boundary -> (d_sensor_twist, {geomID: address}, what keeps
    them alive)"""
    d_s, _, tabs, keep = _tables(sensor_twist, twists, skew)
    return d_s, tabs, keep


def _vel_device(tr, hits, pose, motions, sensor_twist, twists, flags=0, n=None, count=None, stream=None, skew=0, records=True, radial=True):
    """ls_hit_velocities on uploaded copies, both outputs filled with 0xAB and one canary record behind each -> (records uint32
    (handled, 8) | None, radial uint32 (handled,) | None); everything past the handled records must still be 0xAB"""
    import torch
    h = _hits_u32(hits)
    n = h.shape[0] if n is None else n
    d_h = _dev(h) if h.shape[0] else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    d_c = _dev(np.array([count], np.uint32)) if count is not None else None
    d_o = torch.full(((n + 1) * 32,), FILL, dtype=torch.uint8, device="cuda:0")
    d_r = torch.full(((n + 1) * 4,), FILL, dtype=torch.uint8, device="cuda:0")
    d_pose, n_cols, tabs, keep = _tables(pose, motions, skew)
    d_st, tws, keep2 = _twist_tables(sensor_twist, twists, skew)
    torch.cuda.synchronize()
    rc = tr.hitVelocitiesDevice(d_h.data_ptr(), n, d_out=d_o.data_ptr() if records else 0, d_radial=d_r.data_ptr() if radial else 0,
                                d_col_pose=d_pose, n_cols=n_cols, motions=tabs, d_sensor_twist=d_st, twists=tws, flags=flags,
                                d_count=d_c.data_ptr() if d_c is not None else 0, stream=stream)
    assert rc == 0, tr.last_error()
    tr.synchronize()
    torch.cuda.synchronize()
    handled = n if count is None else min(n, count)
    o, r = d_o.cpu().numpy(), d_r.cpu().numpy()
    assert np.all(o[(handled if records else 0) * 32:] == FILL), "a velocity record written past the handled ones"
    assert np.all(r[(handled if radial else 0) * 4:] == FILL), "a radial velocity written past the handled ones"
    return (o[:handled * 32].view(np.uint32).reshape(handled, 8).copy() if records else None,
            r[:handled * 4].view(np.uint32).copy() if radial else None)


def _vel_host(tr, hits, pose, motions, sensor_twist, twists, **kw):
    rc, rec, rad = tr.hitVelocities(hits, pose, motions, sensor_twist, twists, **kw)
    assert rc == 0
    return (None if rec is None else np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 8)), (None if rad is None else rad.view(np.uint32))


def _same(got, want):
    """records (n, 8) or radial arrays (n,): equal bit for bit (test_velocity_cpu.same_floats: a NaN equals any NaN)"""
    g, w = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    assert g.shape == w.shape, (g.shape, w.shape)
    if g.ndim == 2:
        assert np.array_equal(g[:, 7], w[:, 7]), np.nonzero(g[:, 7] != w[:, 7])[0][:10]
        g, w = g[:, 0:7], w[:, 0:7]
    bad = np.nonzero((g != w).reshape(g.shape[0], max(1, g.size // max(1, g.shape[0]))).any(axis=1))[0]
    assert same_floats(g, w), (bad[:10], g[bad[:3]], w[bad[:3]])


_cache = {}


def _case(oracle, capi):
    """the definition frame -- the small sensor on a constant twist, the box on a constant twist about an off-centre pivot, the
    ground at rest --, traced once with ls_trace_scene_sweep_moving, and the restatement of its records' velocities: computed once,
    shared by the tests that need them, never changed"""
    if "case" not in _cache:
        s = small_sensor(oracle)
        dt = TURN / s.H
        pose = capi.sweep_poses_constant_twist(SENSOR_LIN, SENSOR_ANG, 0.0, dt, s.H)
        motion = capi.motion_constant_twist(BOX_LIN, BOX_ANG, BOX_PIVOT, 0.0, dt, s.H)
        st = capi.twist_table_constant(SENSOR_LIN, SENSOR_ANG, (0, 0, 0), 0.0, dt, s.H)
        bt = capi.twist_table_constant(BOX_LIN, BOX_ANG, BOX_PIVOT, 0.0, dt, s.H)
        tr = make_tracer(capi, s)
        ml = _box_ground(tr, oracle)
        scene = oracle.assemble_scene(s, ml)
        k, p, h = _moving(tr, pose, {BOX: motion})
        tr.close()
        want, radial, cast = define_velocities(capi, scene, oracle.ray_dirs(s), s.H, h, pose, {BOX: motion}, st, {BOX: bt})
        for a in (pose, motion, st, bt, h, want, radial, cast):
            a.setflags(write=False)
        _cache["case"] = dict(s=s, scene=scene, pose=pose, motion=motion, st=st, bt=bt, hits=h, want=want, radial=radial, cast=cast, dt=dt)
    return _cache["case"]


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------

def test_moving_box_equals_the_restatement(oracle, capi):
    c = _case(oracle, capi)
    h, want, radial = c["hits"], c["want"], c["radial"]
    valid = want[:, 7] == 1
    assert np.count_nonzero(valid & (h[:, 1] == BOX)) >= 20 and np.count_nonzero(valid & (h[:, 1] == GND)) >= 20
    tr = make_tracer(capi, c["s"])
    _box_ground(tr, oracle)
    rec, rad = _vel_device(tr, h, c["pose"], {BOX: c["motion"]}, c["st"], {BOX: c["bt"]})
    _same(rec, want)
    _same(rad, radial)
    assert np.array_equal(rad[valid], rec[valid, 3])                    # the dense field is the records' radial velocity
    v = rec[:, 0:7].view(F)
    assert np.all(np.isfinite(v)) and not rec[h[:, 1] == GND, 0:3].any()           # the ground rests: +0
    assert np.all(np.linalg.norm(v[h[:, 1] == BOX, 0:3], axis=1) > 5.0) and np.all(np.linalg.norm(v[:, 4:7], axis=1) > 2.0)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 2. validity: the valid bit is ls_hit_attributes_moving's ---------------------------------------------------------------------

def test_valid_bits_equal_the_attributes(oracle, capi):
    c = _case(oracle, capi)
    s, h, pose, motion = c["s"], c["hits"], c["pose"], c["motion"]
    tr = make_tracer(capi, s)
    _box_ground(tr, oracle)
    odd = h[:6].copy()
    odd[0, 1:] = (INV, INV, int(F(-1.0).view(np.uint32)))              # a miss record
    odd[1, 0] = s.V * s.H                                               # a ray past the raster
    odd[2, 1] = 7                                                       # an unknown geometry
    odd[3, 2] = 12 if odd[3, 1] == BOX else 2                           # the first element past the geometry's
    odd[4, 3] += 1                                                      # t one ulp off
    odd[5, 0] = 0xFFFFFFFF
    records = np.concatenate([h, odd])
    other = capi.motion_constant_twist((-3.0, 4.0, 2.0), (0.5, 0.0, -1.0), (0, 0, 0), 0.0, c["dt"], s.H)
    seen_invalid = 0
    for p, m in ((pose, {BOX: motion}), (pose, {}), (None, {BOX: motion}), (pose, {BOX: other}), (pose, {BOX: motion, GND: other})):
        attr = _attr_device(tr, records, p, m)
        rec, rad = _vel_device(tr, records, p, m, c["st"], {BOX: c["bt"]})
        assert np.array_equal(rec[:, 7], attr[:, 7])
        gone = rec[:, 7] == 0
        assert not rec[gone].any() and np.all(rad[gone] == QNAN) and not np.any(np.isnan(rad[~gone].view(F)))
        assert np.all(rec[h.shape[0]:, 7] == 0)
        seen_invalid += np.count_nonzero(gone[:h.shape[0]])
    assert np.all(_vel_device(tr, records, pose, {BOX: motion}, None, {})[0][:h.shape[0], 7] == c["want"][:, 7])
    assert seen_invalid > 40                                            # tables that do not belong to the frame did invalidate records
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 3. exactness -----------------------------------------------------------------------------------------------------------------

def test_pure_translations_no_twists_and_a_snapshot(oracle, capi):
    s = small_sensor(oracle)
    dt = TURN / s.H
    dirs = oracle.ray_dirs(s)
    tr = make_tracer(capi, s)
    ml = _box_ground(tr, oracle)
    scene = oracle.assemble_scene(s, ml)
    # the box recedes straight along x, the sensor drives sideways: no rotation anywhere
    lin_b, lin_s = F([5.0, 0.0, 0.0]), F([0.25, -1.5, 0.125])
    pose = capi.sweep_poses_constant_twist(lin_s, (0, 0, 0), 0.0, dt, s.H)
    motion = capi.motion_constant_twist(lin_b, (0, 0, 0), (6.0, 2.0, 0.0), 0.0, dt, s.H)
    st = capi.twist_table_constant(lin_s, (0, 0, 0), (0, 0, 0), 0.0, dt, s.H)
    bt = capi.twist_table_constant(lin_b, (0, 0, 0), (6.0, 2.0, 0.0), 0.0, dt, s.H)
    k, p, h = _moving(tr, pose, {BOX: motion})
    rec, rad = _vel_device(tr, h, pose, {BOX: motion}, st, {BOX: bt})
    on_box = h[:, 1] == BOX
    assert np.all(rec[:, 7] == 1) and np.count_nonzero(on_box) >= 20 and np.count_nonzero(~on_box) >= 20
    assert np.all(rec[on_box, 0:3] == lin_b.view(np.uint32)) and not rec[~on_box, 0:3].any()      # v_s: lin_vel's bits, +0 at rest
    assert np.all(rec[:, 4:7] == lin_s.view(np.uint32))                                           # v_o: the sensor's lin_vel
    want, radial, cast = define_velocities(capi, scene, dirs, s.H, h, pose, {BOX: motion}, st, {BOX: bt})
    _same(rec, want)
    # with the sensor at rest the box only recedes: on the ray nearest the x axis the radial velocity is the sequence's value, positive
    k0, p0, h0 = _moving(tr, None, {BOX: motion})
    rec0, rad0 = _vel_device(tr, h0, None, {BOX: motion}, None, {BOX: bt})
    want0, radial0, cast0 = define_velocities(capi, scene, dirs, s.H, h0, None, {BOX: motion}, None, {BOX: bt})
    _same(rec0, want0)
    _same(rad0, radial0)
    b0 = np.nonzero(h0[:, 1] == BOX)[0]
    centre = b0[np.argmax(dirs[h0[b0, 0], 0])]
    d = dirs[h0[centre, 0]]
    seq = ((F(5.0) * d[0] + F(0.0) * d[1]) + F(0.0) * d[2]) / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    assert rad0[centre] == F(seq).view(np.uint32) and rad0[centre:centre + 1].view(F)[0] > 4.5
    assert np.all(rad0[b0].view(F) > 0) and not rec0[:, 4:7].any()
    # no twists at all: zero vectors, a radial velocity that is a zero, whatever the frame
    for hh, pp, mm in ((h, pose, {BOX: motion}), (h0, None, {BOX: motion})):
        r, a = _vel_device(tr, hh, pp, mm, None, {})
        assert np.all(r[:, 7] == 1) and not r[:, 0:3].any() and not r[:, 4:7].any() and np.all(r[:, 3].view(F) == 0) and np.all(a.view(F) == 0)
    # twists without motions: the Doppler field of a snapshot, a frame of ls_trace_scene
    rc, pts, hits = tr.traceScene(0)
    assert rc == 0 and len(pts) > 40
    hs = _records(hits)
    spin = capi.twist_table_constant((1.0, 2.0, 0.0), (0.0, 0.0, 2.0), (6.0, 2.0, 0.0), 0.0, 0.0, s.H)      # every column: tau = 0
    rs, as_ = _vel_device(tr, hs, None, {}, st, {BOX: spin, GND: bt})
    ws, wr, _ = define_velocities(capi, scene, dirs, s.H, hs, None, {}, st, {BOX: spin, GND: bt})
    assert np.all(ws[:, 7] == 1) and set(hs[:, 1]) == {BOX, GND}
    _same(rs, ws)
    _same(as_, wr)
    assert np.all(rs[hs[:, 1] == GND, 0:3] == lin_b.view(np.uint32))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 4. meaning: finite differences of the trajectory and of the range ----------------------------------------------------------------

FD_STEP = 1e-6


def _finite_differences(c, lin_s, ang_s):
    """for the valid records of the definition frame, in float64: the hit point P = o + t c' of the float32 cast ray taken as
    doubles is the material point's position at tau_h; the material point x_0 = Q(tau_h)^T (P - c(tau_h)) rides the box's motion
    (test_velocity_cpu.body_motion, Rodrigues in double), the ground's rests; the sensor's origin rides lin_s from the pose table's
    own origin (a sensor turns about its origin: pivot 0).  Central differences at tau_h +- 1e-6 s of x(tau) and of |x(tau) -
    o(tau)| -> (indices, v_s (k, 3), radial (k,), the twist records used (k, 6) x 2)"""
    s, h, cast = c["s"], c["hits"], c["cast"].astype(np.float64)
    idx = np.nonzero(c["want"][:, 7] == 1)[0]
    vs, rad = np.zeros((idx.size, 3)), np.zeros(idx.size)
    ls = np.asarray(F(lin_s), np.float64)
    for j, i in enumerate(idx):
        col = int(h[i, 0]) % s.H
        tau = col * c["dt"]
        o = cast[i, 0:3]
        P = o + float(h[i, 3:4].view(F)[0]) * cast[i, 4:7]
        pos = []
        for sign in (+1.0, -1.0):
            if h[i, 1] == BOX:
                Q0, c0 = body_motion(BOX_LIN, BOX_ANG, BOX_PIVOT, tau)
                Q1, c1 = body_motion(BOX_LIN, BOX_ANG, BOX_PIVOT, tau + sign * FD_STEP)
                x = Q1 @ (Q0.T @ (P - c0)) + c1
            else:
                x = P
            pos.append((x, o + ls * (sign * FD_STEP)))
        vs[j] = (pos[0][0] - pos[1][0]) / (2 * FD_STEP)
        rad[j] = (np.linalg.norm(pos[0][0] - pos[0][1]) - np.linalg.norm(pos[1][0] - pos[1][1])) / (2 * FD_STEP)
    return idx, vs, rad


def _meaning_bound(c, idx, st, twists):
    """velocity_bound (test_velocity_cpu: the float32 sequence against float64, from the operation count) for these records, plus
    what separates the float64 evaluation of the TABLES from the finite differences:
      the tables' single rounding: each entry of u and w is one rounding off its double value -- e (|u_i| + |w_j| |x_k| + |w_k|
        |x_j|) per component for either body, and through rel . c^ into the radial velocity;
      the central difference: truncation d^2 / 6 |x'''| <= d^2 / 6 |w|^3 (|x| + |pivot| + |lin| tau) < 1e-11 m/s, and for the range
        d^2 / 6 |rho'''| with rho''' a sum of a few products of |w|, |rel| / rho and |rel| < 1e3 m/s^3: < 2e-10 m/s; its own rounding
        4 * 2^-53 * 50 m / d = 2.3e-8 m/s.  FD_ALLOWANCE = 5e-8 m/s covers the three.
    -> (bound on each component of v_s (k, 3), on radial (k,))"""
    FD_ALLOWANCE = 5e-8
    s, h = c["s"], c["hits"][idx]
    cast, t = c["cast"][idx], h[:, 3].copy().view(F)
    cols = h[:, 0] % s.H
    gt = np.zeros((idx.size, 6), np.float32)
    for g, tab in twists.items():
        gt[h[:, 1] == g] = tab[cols[h[:, 1] == g]]
    sv = None if st is None else st[cols]
    bvs, brad = velocity_bound(cast, t, sv, gt)
    r = cast.astype(np.float64)
    o, cc = r[:, 0:3], r[:, 4:7]
    P = np.abs(o + t.astype(np.float64)[:, None] * cc)

    def rounding(tw, x):
        a = np.abs(tw.astype(np.float64))
        return EPS * np.stack([a[:, 3 + i] + a[:, j] * x[:, k] + a[:, k] * x[:, j] for i, (j, k) in enumerate(((1, 2), (2, 0), (0, 1)))], axis=1)

    tvs = rounding(gt, P)
    tvo = rounding(sv, np.abs(o)) if sv is not None else 0.0
    unit = np.abs(cc) / np.linalg.norm(cc, axis=1, keepdims=True)
    return bvs + tvs + FD_ALLOWANCE, brad + np.sum(unit * (tvs + tvo), axis=1) + FD_ALLOWANCE


def test_velocities_mean_the_rate_of_the_trajectory(oracle, capi):
    """v_s and the radial velocity of the definition frame's valid records -- the device's, which test 1 pins to the restatement --
    against float64 central differences of the material point's trajectory and of its range to the sensor's origin (_finite_differences),
    within _meaning_bound, whose docstring derives it: at most 5e-6 m/s for v_s and 8e-6 m/s for the radial velocity here.  Measured
    on the MI355X: the largest error is 0.56 of the bound for v_s and 0.18 for the radial velocity."""
    c = _case(oracle, capi)
    tr = make_tracer(capi, c["s"])
    _box_ground(tr, oracle)
    rec, rad = _vel_device(tr, c["hits"], c["pose"], {BOX: c["motion"]}, c["st"], {BOX: c["bt"]})
    tr.close()
    idx, vs, radial = _finite_differences(c, SENSOR_LIN, SENSOR_ANG)
    bvs, brad = _meaning_bound(c, idx, c["st"], {BOX: c["bt"]})
    got = rec[idx, 0:4].view(F).astype(np.float64)
    evs, erad = np.abs(got[:, 0:3] - vs), np.abs(got[:, 3] - radial)
    print("largest error / bound: v_s %.3f, radial %.3f; largest bound: v_s %.3g m/s, radial %.3g m/s; largest |radial| %.3g m/s" %
          ((evs / bvs).max(), (erad / brad).max(), bvs.max(), brad.max(), np.abs(radial).max()))
    assert idx.size >= 40 and np.all(evs <= bvs) and np.all(erad <= brad)
    assert np.abs(radial).max() > 3.0 and brad.max() < 1e-4             # metres per second against a bound of micrometres per second


# ---- 5. a sensor that only spins ----------------------------------------------------------------------------------------------------

def test_a_spinning_sensor_adds_no_range_rate(oracle, capi):
    """lin 0, ang != 0 about the sensor's own origin: the frame is another one (the rays turn), but v_o is zero and the radial
    velocity of every record is what the same record gets with the sensor's twist left out, within the bound of the float32
    sequence (velocity_bound, both evaluations against the one float64 value): a turning sensor changes no range."""
    s = small_sensor(oracle)
    dt = TURN / s.H
    spin = (0.3, -0.2, 2.5)
    pose = capi.sweep_poses_constant_twist((0, 0, 0), spin, 0.0, dt, s.H)
    st = capi.twist_table_constant((0, 0, 0), spin, (0, 0, 0), 0.0, dt, s.H)
    motion = capi.motion_constant_twist(BOX_LIN, BOX_ANG, BOX_PIVOT, 0.0, dt, s.H)
    bt = capi.twist_table_constant(BOX_LIN, BOX_ANG, BOX_PIVOT, 0.0, dt, s.H)
    assert np.all(pose[:, [3, 7, 11]] == 0) and np.any(pose[:, 1] != 0) and not st[:, 3:6].any()
    tr = make_tracer(capi, s)
    _box_ground(tr, oracle)
    k, p, h = _moving(tr, pose, {BOX: motion})
    spun, _ = _vel_device(tr, h, pose, {BOX: motion}, st, {BOX: bt})
    rest, _ = _vel_device(tr, h, pose, {BOX: motion}, None, {BOX: bt})
    tr.close()
    assert np.all(spun[:, 7] == 1) and np.count_nonzero(h[:, 1] == BOX) >= 20
    assert np.all(spun[:, 4:7].view(F) == 0)                            # w x 0: the origin stays where it is
    cast = np.zeros((k, 8), np.float32)
    cast[:, 4:7] = np.einsum("kij,kj->ki", pose[h[:, 0] % s.H].reshape(-1, 3, 4)[:, :, :3].astype(np.float64), oracle.ray_dirs(s)[h[:, 0]])
    gt = np.where((h[:, 1] == BOX)[:, None], bt[h[:, 0] % s.H], F(0))
    _, brad = velocity_bound(cast, h[:, 3].copy().view(F), st[h[:, 0] % s.H], gt)
    diff = np.abs(spun[:, 3].view(F).astype(np.float64) - rest[:, 3].view(F).astype(np.float64))
    print("largest difference / bound: %.3f" % (diff[brad > 0] / (2 * brad[brad > 0])).max())      # (no bound, no difference: a ground record)
    assert np.all(diff <= 2 * brad) and np.abs(rest[h[:, 1] == BOX, 3].view(F)).max() > 3.0


# ---- 6. plumbing --------------------------------------------------------------------------------------------------------------------

def test_count_word_optional_outputs_alignment_streams_host_and_shards(oracle, capi):
    import torch
    c = _case(oracle, capi)
    s, h, pose, want, radial = c["s"], c["hits"], c["pose"], c["want"], c["radial"]
    mo, tw = {BOX: c["motion"]}, {BOX: c["bt"]}
    n = h.shape[0]
    tr = make_tracer(capi, s)
    _box_ground(tr, oracle)
    # a device count below n, equal to it and above it: canaries behind both outputs (the helper checks them)
    for count in (0, 1, 63, 64, n - 1, n, n + 9):
        rec, rad = _vel_device(tr, h, pose, mo, c["st"], tw, count=count)
        _same(rec, want[:min(count, n)])
        _same(rad, radial[:min(count, n)])
    # one output without the other
    rec, rad = _vel_device(tr, h, pose, mo, c["st"], tw, radial=False)
    assert rad is None
    _same(rec, want)
    rec, rad = _vel_device(tr, h, pose, mo, c["st"], tw, records=False, count=n - 3)
    assert rec is None
    _same(rad, radial[:n - 3])
    # n = 0: LS_OK, nothing written, no output needed
    assert _vel_device(tr, h[:0], pose, mo, c["st"], tw)[0].shape == (0, 8)
    assert tr.hitVelocitiesDevice(0, 0) == 0
    # tables 4 bytes past a 16-byte boundary, an identity motion and a zero twist for the ground next to the box's, a caller stream
    ident, zero = np.tile(IDENTITY_POSE, (s.H, 1)), np.zeros((s.H, 6), np.float32)
    qs = torch.cuda.Stream()
    for skew, stream in ((4, None), (12, qs.cuda_stream), (0, qs.cuda_stream)):
        rec, rad = _vel_device(tr, h, pose, {BOX: c["motion"], GND: ident}, c["st"], {BOX: c["bt"], GND: zero}, skew=skew, stream=stream)
        assert np.array_equal(rec.view(F), want.view(F)[:, :])            # (0 + 0 x P is a zero of either sign: equal numerically)
        assert np.array_equal(rec[:, 7], want[:, 7]) and np.array_equal(rad.view(F), radial.view(F))
        _same(rec[h[:, 1] == BOX], want[h[:, 1] == BOX])
    # the host variant equals the device's; host memory may have any alignment
    rec, rad = _vel_host(tr, h, pose, mo, c["st"], tw)
    _same(rec, want)
    _same(rad, radial)
    rec, rad = _vel_host(tr, h, pose, mo, c["st"], tw, radial=False)
    assert rad is None
    _same(rec, want)
    rec, rad = _vel_host(tr, h, pose, mo, c["st"], tw, records=False)
    assert rec is None
    _same(rad, radial)
    odd = np.zeros(s.H * 24 + 1, np.uint8)
    odd[1:] = c["bt"].view(np.uint8).reshape(-1)
    tws = (capi.GeometryTwist * 1)()
    tws[0].geom, tws[0].col_twist = BOX, odd.ctypes.data + 1
    mos = (capi.GeometryMotion * 1)()
    mos[0].geom, mos[0].col_motion = BOX, c["motion"].ctypes.data
    out = np.full((n + 1, 8), 0xABABABAB, np.uint32)
    assert tr.L.ls_hit_velocities_host(tr.h, pose.ctypes.data, s.H, mos, 1, c["st"].ctypes.data, tws, 1, 0, h.ctypes.data, n, out.ctypes.data, None) == 0
    _same(out[:n], want)
    assert np.all(out[n] == 0xABABABAB)
    assert _vel_host(tr, h[:0], pose, mo, c["st"], tw)[0].shape == (0, 8)
    # the result does not depend on the shard: the tables keep H records, hit.ray is global
    tr.setShard(5, 7)
    rec, rad = _vel_device(tr, h, pose, mo, c["st"], tw)
    _same(rec, want)
    _same(rad, radial)
    k, p, hs = _moving(tr, pose, mo)
    inside = (h[:, 0] % s.H >= 5) & (h[:, 0] % s.H < 12)
    assert 10 < k < n and np.array_equal(hs, h[inside])
    _same(_vel_device(tr, hs, pose, mo, c["st"], tw)[0], want[inside])
    _same(_vel_host(tr, hs, pose, mo, c["st"], tw)[0], want[inside])
    tr.setShard(0, s.H)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_forty_geometries_block_edges_and_a_nan_twist(oracle, capi):
    """forty plates on a 5 x 8 wall in front of the small sensor with free ids between them (every fourth geometry added is removed
    before the commit), twists for every third; 3 * kBlock + 17 records drawn from the frame in shuffled order, so that block edges
    fall inside the input and the lanes of a wave name different geometries; then a non-finite twist entry."""
    s = small_sensor(oracle)
    dt = TURN / s.H
    dirs = oracle.ray_dirs(s)
    tr = make_tracer(capi, s)
    plate = (F([[0, -0.5, -0.5], [0, 0.5, -0.5], [0, 0.5, 0.5], [0, -0.5, 0.5]]), np.uint32([[0, 1, 2], [0, 2, 3]]))
    rng = np.random.default_rng(40)
    ml, twists, kept = [], {}, []
    for k in range(54):
        assert _add(tr, f"g{k}", *plate) == k
        j = len(kept)
        A = F([1, 0, 0, 8.0 + 0.1 * j, 0, 1, 0, 0.4 + (j % 8), 0, 0, 1, -2.0 + (j // 8)])
        tr.updateGeometry(f"g{k}", A, *plate)
        if k % 4 == 3 or j >= 40:
            continue
        ml.append((k, *plate, A))
        kept.append(k)
        if j % 3 == 0:
            twists[k] = capi.twist_table_constant(rng.uniform(-9, 9, 3), rng.uniform(-1, 1, 3), A[[3, 7, 11]], 0.0, dt, s.H)
    for k in range(54):
        if k not in kept:
            assert tr.removeGeometry(f"g{k}") >= 0
    assert tr.commitScene() == 0 and tr.getGeometryCount() == 40 and len(twists) == 14
    scene = oracle.assemble_scene(s, ml)
    pose = capi.sweep_poses_constant_twist(SENSOR_LIN, SENSOR_ANG, 0.0, dt, s.H)
    st = capi.twist_table_constant(SENSOR_LIN, SENSOR_ANG, (0, 0, 0), 0.0, dt, s.H)
    k, p, h = _moving(tr, pose, {})
    assert k >= 50 and len(set(h[:, 1])) >= 20 and len(set(h[:, 1]) & set(twists)) >= 6
    want, radial, cast = define_velocities(capi, scene, dirs, s.H, h, pose, {}, st, twists)
    assert np.all(want[:, 7] == 1)
    pick = rng.integers(0, k, 3 * KBLOCK + 17)
    rec, rad = _vel_device(tr, h[pick], pose, {}, st, twists)
    _same(rec, want[pick])
    _same(rad, radial[pick])
    _same(_vel_host(tr, h[pick], pose, {}, st, twists)[0], want[pick])
    moving = np.isin(h[pick, 1], list(twists))
    assert np.count_nonzero(moving) > 100 and np.all(rec[moving, 0:3].view(F).any(axis=1)) and not rec[~moving, 0:3].any()
    # records that name a free id between two geometries, or an id past the table: invalid, nothing read
    odd = h[:3].copy()
    odd[0, 1], odd[1, 1], odd[2, 1] = 3, 54, INV
    r, a = _vel_device(tr, odd, pose, {}, st, twists)
    assert not r.any() and np.all(a == QNAN)
    # a non-finite entry in one column of one twist table: non-finite values, and the record stays valid
    g = int(np.bincount(h[np.isin(h[:, 1], list(twists)), 1]).argmax())
    col = int(h[h[:, 1] == g][0, 0] % s.H)
    bad = dict(twists)
    bad[g] = twists[g].copy()
    bad[g][col, 1] = np.nan
    bad[g][(col + 1) % s.H, 4] = np.inf
    rec, rad = _vel_device(tr, h, pose, {}, st, bad)
    wb, rb, _ = define_velocities(capi, scene, dirs, s.H, h, pose, {}, st, bad)
    _same(rec, wb)
    _same(rad, rb)
    hit = (h[:, 1] == g) & (h[:, 0] % s.H == col)
    assert np.count_nonzero(hit) >= 1 and np.all(rec[:, 7] == 1) and np.all(np.isnan(rec[hit, 0:3].view(F)).any(axis=1))
    assert np.all(np.isnan(rad[hit].view(F)))
    _same(rec[~np.isin(h[:, 1], [g])], want[~np.isin(h[:, 1], [g])])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order_with_nothing_written(oracle, capi):
    """every refusal of the header, alone and together with the one after it (the earlier one answers: ls_last_error says which),
    for the device call, and the host variant's; nothing is written.  A removal commits the remaining scene itself, so a twist that
    names the removed geometry is LS_ERR_UNKNOWN_GEOMETRY."""
    import torch
    s = small_sensor(oracle)
    n = 8
    ident, zero = np.tile(IDENTITY_POSE, (s.H, 1)), np.zeros((s.H, 6), np.float32)
    d_pose, d_tab, d_tw = (torch.from_numpy(a.copy()).to("cuda:0") for a in (ident, ident, zero))
    d_h = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    bufs = {k: torch.full((size,), FILL, dtype=torch.uint8, device="cuda:0") for k, size in (("o", n * 32 + 64), ("r", n * 4 + 64), ("c", 64))}
    torch.cuda.synchronize()
    O_, R_, C_ = (bufs[k].data_ptr() for k in "orc")
    hits = np.zeros(n, capi.HIT_DTYPE)
    host_o, host_r = np.full((n, 32), FILL, np.uint8), np.full(n * 4, FILL, np.uint8)

    def untouched():
        torch.cuda.synchronize()
        return all(np.all(b.cpu().numpy() == FILL) for b in bufs.values()) and np.all(host_o == FILL) and np.all(host_r == FILL)

    def array(kind, entries):
        arr = (kind * max(1, len(entries)))()
        for e, (g, r, t) in zip(arr, entries):
            e.geom, e.reserved = g, r
            setattr(e, kind._fields_[2][0], t)
        return arr

    TAB, TW = d_tab.data_ptr(), d_tw.data_ptr()
    base = dict(pose=d_pose.data_ptr(), n_cols=s.H, entries=[(BOX, 0, TAB)], null_motions=False, n_motions=None, st=TW, tw_entries=[(BOX, 0, TW)],
                null_twists=False, n_twists=None, flags=0, hits=d_h.data_ptr(), count=None, n=n, o=O_, r=R_)
    host_base = dict(base, pose=ident.ctypes.data, entries=[(BOX, 0, ident.ctypes.data)], st=zero.ctypes.data, tw_entries=[(BOX, 0, zero.ctypes.data)],
                     hits=hits.ctypes.data, o=host_o.ctypes.data, r=host_r.ctypes.data)

    def args(a):
        nm = len(a["entries"]) if a["n_motions"] is None else a["n_motions"]
        nt = len(a["tw_entries"]) if a["n_twists"] is None else a["n_twists"]
        return (a["pose"], a["n_cols"], None if a["null_motions"] else array(capi.GeometryMotion, a["entries"]), nm, a["st"],
                None if a["null_twists"] else array(capi.GeometryTwist, a["tw_entries"]), nt, a["flags"])

    def vel(tr, **kw):
        a = {**base, **kw}
        return tr.L.ls_hit_velocities(tr.h, None, *args(a), a["hits"], a["count"], a["n"], a["o"], a["r"])

    def vel_host(tr, **kw):
        a = {**host_base, **kw}
        return tr.L.ls_hit_velocities_host(tr.h, *args(a), a["hits"], a["n"], a["o"], a["r"])

    tr = make_tracer(capi, s)
    # -1 with no commit writes nothing; the argument checks and the record limit come before it, an unknown geometry after it
    assert vel(tr, entries=[], tw_entries=[]) == -1 and vel_host(tr, entries=[], tw_entries=[]) == -1 and untouched()
    bx = box()
    _add(tr, "box", *bx)
    _add(tr, "ground", *GROUND)
    assert vel(tr) == -1 and vel_host(tr) == -1 and vel(tr, tw_entries=[(7, 0, TW)]) == -1 and untouched()
    assert vel(tr, n_cols=s.H - 1) == INVALID_ARGUMENT and vel(tr, n=0xFFF00001) == OUT_OF_RANGE and untouched()
    tr.updateGeometry("box", BOX_POSE, *bx)
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *GROUND)
    assert tr.commitScene() == 0
    rc, _ = tr.traceRays(np.float32([[0, 0, 0, 0, 1.0, 0.3, 0.0, np.inf]]))
    assert rc == 0
    built = tr.info(capi.LS_INFO_RAY_QUERY_BUILT)
    steps = [
        (dict(hits=None), "null hit records"),
        (dict(n_cols=s.H - 1), "one pose per azimuth column"),
        (dict(flags=capi.LS_SWEEP_DESKEW), "unknown flags"),
        (dict(null_motions=True, n_motions=1), "null motions"),
        (dict(entries=[(BOX, 0, None)]), "a motion without a table"),
        (dict(entries=[(BOX, 1, TAB)]), "ls_geometry_motion.reserved"),
        (dict(entries=[(BOX, 0, TAB), (BOX, 0, TAB)]), "two motions"),
        (dict(null_twists=True, n_twists=1), "null twists"),
        (dict(tw_entries=[(BOX, 0, None)]), "a twist without a table"),
        (dict(tw_entries=[(BOX, 1, TW)]), "ls_geometry_twist.reserved"),
        (dict(tw_entries=[(BOX, 0, TW), (BOX, 0, TW)]), "two twists"),
        (dict(hits=d_h.data_ptr() + 8), "aligned"),
        (dict(n=0xFFF00001), "too many"),
        (dict(entries=[(2, 0, TAB)]), "a motion names"),
        (dict(tw_entries=[(2, 0, TW)]), "a twist names"),
    ]
    codes = [INVALID_ARGUMENT] * 12 + [OUT_OF_RANGE, UNKNOWN_GEOMETRY, UNKNOWN_GEOMETRY]
    together = {3: dict(null_motions=True, n_motions=1, entries=[]),               # NULL motions, and a table that would be NULL
                4: dict(entries=[(BOX, 1, None)]),                                 # a NULL table in an entry whose reserved is set
                5: dict(entries=[(BOX, 1, TAB), (BOX, 0, TAB)]),                   # reserved set in one of two entries for one geometry
                7: dict(null_twists=True, n_twists=1, tw_entries=[]),
                8: dict(tw_entries=[(BOX, 1, None)]),
                9: dict(tw_entries=[(BOX, 1, TW), (BOX, 0, TW)])}
    for i, (kw, says) in enumerate(steps):
        assert vel(tr, **kw) == codes[i] and says in tr.last_error(), (i, tr.last_error())
        if i + 1 < len(steps):
            both = together.get(i, {**kw, **steps[i + 1][0]})
            assert vel(tr, **both) == codes[i] and says in tr.last_error(), (i, tr.last_error())
    assert untouched()
    more = [
        vel(tr, o=None, r=None), vel_host(tr, hits=None), vel_host(tr, o=None, r=None),
        vel(tr, n_cols=s.H + 1), vel(tr, pose=None, n_cols=s.H), vel(tr, flags=2), vel(tr, flags=0x80000000),
        vel(tr, entries=[(0, 0, TAB), (1, 0, TAB), (2, 0, TAB)]), vel(tr, tw_entries=[(0, 0, TW), (1, 0, TW), (2, 0, TW)]),      # more than geometries
        vel(tr, o=O_ + 8), vel(tr, r=R_ + 2), vel(tr, count=C_ + 2), vel(tr, pose=d_pose.data_ptr() + 2), vel(tr, entries=[(BOX, 0, TAB + 2)]),
        vel(tr, st=TW + 2), vel(tr, tw_entries=[(BOX, 0, TW + 1)]),
        vel_host(tr, n_cols=s.H - 1), vel_host(tr, flags=1), vel_host(tr, null_motions=True, n_motions=1), vel_host(tr, null_twists=True, n_twists=2),
        vel_host(tr, tw_entries=[(BOX, 0, None)]), vel_host(tr, tw_entries=[(GND, 9, zero.ctypes.data)]),
        vel_host(tr, tw_entries=[(GND, 0, zero.ctypes.data), (GND, 0, zero.ctypes.data)]),
    ]
    assert more == [INVALID_ARGUMENT] * len(more) and untouched()
    assert vel_host(tr, tw_entries=[(0xFFFFFFFF, 0, zero.ctypes.data)]) == UNKNOWN_GEOMETRY and vel_host(tr, n=0xFFF00001) == OUT_OF_RANGE
    assert untouched()
    # a shard changes nothing: the tables keep H records
    tr.setShard(3, 5)
    assert vel(tr, n_cols=5) == INVALID_ARGUMENT and untouched()
    tr.setShard(0, s.H)
    # 16 bytes are enough for the records, 4 for the words and the tables; eight zero records are invalid
    assert vel(tr, o=O_ + 16, r=R_ + 4, count=C_ + 4) == 0        # (the count word holds 0xABABABAB: min(n, count) = n)
    tr.synchronize()
    torch.cuda.synchronize()
    o, r = bufs["o"].cpu().numpy(), bufs["r"].cpu().numpy()
    assert np.all(o[:16] == FILL) and not o[16:16 + n * 32].any() and np.all(o[16 + n * 32:] == FILL)
    assert np.all(r[:4] == FILL) and np.all(r[4:4 + n * 4].view(np.uint32) == QNAN) and np.all(r[4 + n * 4:] == FILL)
    for b in bufs.values():
        b.fill_(FILL)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0 and tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == built
    # a removal commits the remaining scene: a twist of the removed geometry is unknown, an emptied scene is -1
    assert tr.removeGeometry("ground") >= 0
    assert vel(tr, entries=[], tw_entries=[(GND, 0, TW)]) == UNKNOWN_GEOMETRY and "a twist names" in tr.last_error()
    assert vel(tr, entries=[(GND, 0, TAB)], tw_entries=[(GND, 0, TW)]) == UNKNOWN_GEOMETRY and "a motion names" in tr.last_error()
    assert vel(tr, entries=[], tw_entries=[(BOX, 0, TW)]) == 0
    tr.synchronize()
    for b in bufs.values():
        b.fill_(FILL)
    assert tr.removeGeometry("box") >= 0
    assert vel(tr, entries=[], tw_entries=[]) == -1 and vel_host(tr, entries=[], tw_entries=[]) == -1 and untouched()
    tr.close()


def test_open_frame_graph_is_refused_first(oracle, capi, sensors, meshes):
    import torch
    from test_gpu_rays import _ground_ben
    s = sensors["0001"]
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    tr.setOption(capi.LS_OPT_FRAME_GRAPH, 1)
    _ground_ben(tr, oracle, meshes)
    cap = s.V * s.H
    p, h, c = (torch.zeros(32 * cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * cap, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), cap)
    out = torch.full((cap * 32,), FILL, dtype=torch.uint8, device="cuda:0")
    rad = torch.full((cap * 4,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != 0   # the frame is being captured: the graph is open
    assert L.ls_hit_velocities(tr.h, None, None, 0, None, 0, None, None, 0, 0, h.data_ptr(), c.data_ptr(), cap, out.data_ptr(),
                               rad.data_ptr()) == INVALID_ARGUMENT and "frame graph" in tr.last_error()
    # (NULL records and a wrong n_cols as well: the open graph answers first)
    assert L.ls_hit_velocities(tr.h, None, None, 3, None, 0, None, None, 0, 1, None, None, cap, None, None) == INVALID_ARGUMENT
    assert "frame graph" in tr.last_error()
    assert L.ls_hit_velocities_host(tr.h, None, 3, None, 0, None, None, 0, 0, None, cap, None, None) == INVALID_ARGUMENT and "frame graph" in tr.last_error()
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert bool(torch.all(out == FILL)) and bool(torch.all(rad == FILL))
    # the frame went out, and the handle answers again: straight from the frame's device buffers through its count word
    k = int(c[0].item())
    assert k > 0
    assert tr.hitVelocitiesDevice(h.data_ptr(), cap, d_out=out.data_ptr(), d_radial=rad.data_ptr(), d_count=c.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    o, r = out.cpu().numpy(), rad.cpu().numpy()
    rec = o[:k * 32].view(np.uint32).reshape(k, 8)
    # a frame at rest: valid, zero vectors, a radial velocity that is a zero
    assert np.all(rec[:, 7] == 1) and not rec[:, 0:3].any() and not rec[:, 4:7].any()
    assert np.all(rec[:, 3].view(F) == 0) and np.all(r[:k * 4].view(F) == 0)
    assert np.all(o[k * 32:] == FILL) and np.all(r[k * 4:] == FILL)
    tr.close()
