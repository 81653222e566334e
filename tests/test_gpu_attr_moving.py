"""ls_hit_attributes_moving / ls_apply_return_model_moving (and their _host variants) on the MI355X: surface attributes and sensor
returns for the records of a frame whose sensor and geometries move during the turn.  The degenerate cases against
ls_hit_attributes / ls_apply_return_model; a real motion against the definition restated on the host -- the column's ray
(test_sweep_cpu.restate_rays), the ray the geometry saw (test_sweep_moving_cpu.restate_motion_rays), the oracle's sensor-frame
corners through ls_debug_hit_attributes_on_triangle, the normal through ls_debug_motion_normal, the model through
ls_debug_return_model --; the meaning of a record against a geometry re-posed per column, exactly for a translation and a half turn;
tables that do not belong to the frame, many geometries, shards, buffer variants, canaries, refusals.  Everything is compared bit
for bit unless said otherwise."""
import ctypes

import numpy as np
import pytest

from conftest import make_tracer
from test_attr_moving_cpu import box, box_case
from test_gpu_attr import _hits_u32, _u32
from test_gpu_rays import INV, _add, _ground_ben, _records
from test_gpu_returns import _full_model
from test_gpu_sweep import FILL, _same_bits, _sweep, _twist_poses
from test_gpu_sweep_moving import PLATE, TURN, _identity_tables, _moving, _scene
from test_returns_cpu import bad_models
from test_sweep_cpu import IDENTITY_POSE, restate_rays
from test_sweep_moving_cpu import compose, restate_motion_rays

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, UNKNOWN_GEOMETRY, OUT_OF_RANGE = -2, -3, -9
F = np.float32
REFL = [0.8, 0.6]


# ---- the definition, restated -----------------------------------------------------------------------------------------------

def _define(capi, scene, dirs, H, hits, pose, motions, deskew):
    """per hit (ray, geom, prim, t bits): the ray its column cast -- (0, d) without a pose table --, the ray its geometry saw, the
    named triangle of the oracle's scene (a quad: its two triangles in order) through ls_debug_hit_attributes_on_triangle; valid
    when it passes with t bit-equal to hit.t.  The normal of a moving geometry through ls_debug_motion_normal; p = t * d, or o_h +
    t * d' when deskewing under a pose table.  -> (records uint32 (n, 12), the rays the columns cast float32 (n, 8))"""
    h = _hits_u32(hits)
    out = np.zeros((h.shape[0], 12), np.uint32)
    out[:, 11] = h[:, 0]
    cast_all = np.zeros((h.shape[0], 8), np.float32)
    slot_of = {int(g): i for i, g in enumerate(scene.geom_ids)}
    first = [int(x) for x in scene.geom_first] + [scene.tris.shape[0]]
    for i in range(h.shape[0]):
        ray, geom, prim, tbits = (int(x) for x in h[i])
        if ray >= dirs.shape[0] or geom not in slot_of:
            continue
        slot = slot_of[geom]
        quad = bool(scene.geom_quad[slot])
        n_tris = first[slot + 1] - first[slot]
        if prim >= (n_tris // 2 if quad else n_tris):
            continue
        col, d = ray % H, dirs[ray].astype(F)
        cast = np.zeros(8, np.float32)
        cast[4:7], cast[7] = d, F(1e16)
        if pose is not None:
            cast = restate_rays(d[None], pose[col][None])[0]
        cast_all[i] = cast
        seen = restate_motion_rays(cast[None], motions[geom][col][None])[0] if geom in motions else cast
        if not (np.all(np.isfinite(seen[[0, 1, 2, 4, 5, 6]])) and np.any(seen[4:7] != 0)):
            continue
        for k in ((2 * prim, 2 * prim + 1) if quad else (prim,)):
            c = scene.verts[scene.tris[first[slot] + k]]
            got = capi.hit_attributes_on_triangle(seen[0:3], seen[4:7], c[0], c[1], c[2])
            if got is not None and int(got[0].view(np.uint32)) == tbits:
                t, r = got
                nrm = capi.motion_normal(r[0:3], motions[geom][col]) if geom in motions else r[0:3]
                p = cast[0:3] + t * cast[4:7] if deskew and pose is not None else t * d
                out[i, 0:3] = nrm.view(np.uint32)
                out[i, 3:6] = r[3:6].view(np.uint32)
                out[i, 6], out[i, 7] = k, 1
                out[i, 8:11] = p.astype(F).view(np.uint32)
                break
    return out, cast_all


def _define_returns(capi, model, hits, rec, cast, dirs, H, deskew, refl=None, frame=0):
    """the kept returns of the valid records, in input order: len of the ray the column cast, ls_debug_return_model, the point t' *
    d or o_h + t' * d', ring = ray // H -> (points uint8 (k, 32), records uint32 (k, 4))"""
    h = _hits_u32(hits)
    pts, out = [], []
    for i in np.nonzero(rec[:, 7] == 1)[0]:
        ray, geom, prim = (int(x) for x in h[i, 0:3])
        c = cast[i, 4:7]
        length = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        rho = F(refl[geom]) if refl is not None and geom < len(refl) else F(1)
        kept, tp, inten = capi.return_model(model, ray, frame, h[i, 3:4].view(F)[0], length, rec[i, 3:4].view(F)[0], rho)
        if not kept:
            continue
        xyz = cast[i, 0:3] + tp * c if deskew else tp * dirs[ray].astype(F)
        p = np.zeros(8, np.uint32)
        p[0:3] = xyz.astype(F).view(np.uint32)
        p[4] = F(inten).view(np.uint32)
        p[5] = ray // H
        pts.append(p)
        out.append((ray, geom, prim, int(F(tp).view(np.uint32))))
    return np.array(pts, np.uint32).reshape(-1, 8).view(np.uint8).reshape(-1, 32), np.array(out, np.uint32).reshape(-1, 4)


# ---- the device entry points ------------------------------------------------------------------------------------------------

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _tables(pose, motions, skew=0):
    """the pose table and the motion tables in device memory, each `skew` bytes past a 16-byte boundary -> (d_col_pose, n_cols,
    {geomID: address}, what keeps them alive)"""
    import torch

    def table(a):
        raw = np.ascontiguousarray(a, np.float32).view(np.uint8).reshape(-1)
        buf = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        buf[skew:skew + raw.size] = torch.from_numpy(raw.copy()).to("cuda:0")
        return buf

    d_pose = None if pose is None else table(pose)
    d_tabs = {g: table(t) for g, t in motions.items()}
    return (0 if pose is None else d_pose.data_ptr() + skew, 0 if pose is None else pose.shape[0],
            {g: b.data_ptr() + skew for g, b in d_tabs.items()}, (d_pose, d_tabs))


def _attr_device(tr, hits, pose, motions, flags=0, n=None, count=None, stream=None, skew=0):
    """ls_hit_attributes_moving on uploaded copies, the output filled with 0xAB and one canary record behind it -> uint32 (handled,
    12); everything past the handled records must still be 0xAB"""
    import torch
    h = _hits_u32(hits)
    n = h.shape[0] if n is None else n
    d_h = _dev(h) if h.shape[0] else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    d_c = _dev(np.array([count], np.uint32)) if count is not None else None
    d_o = torch.full(((n + 1) * 48,), FILL, dtype=torch.uint8, device="cuda:0")
    d_pose, n_cols, tabs, keep = _tables(pose, motions, skew)
    torch.cuda.synchronize()
    rc = tr.hitAttributesMovingDevice(d_h.data_ptr(), n, d_o.data_ptr(), d_col_pose=d_pose, n_cols=n_cols, motions=tabs, flags=flags,
                                      d_count=d_c.data_ptr() if d_c is not None else 0, stream=stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    handled = n if count is None else min(n, count)
    o = d_o.cpu().numpy()
    assert np.all(o[handled * 48:] == FILL), "an attribute record written past the handled ones"
    return o[:handled * 48].view(np.uint32).reshape(handled, 12).copy()


def _returns_device(tr, model, hits, pose, motions, flags=0, refl=None, frame=0, n=None, count=None, points=True, records=True, stream=None,
                    skew=0):
    """ls_apply_return_model_moving on uploaded copies, outputs filled with 0xAB -> (points uint8 (k, 32) | None, records uint32 (k,
    4) | None, k); everything past record k, one canary record behind the capacity included, must still be 0xAB"""
    import torch
    h = _hits_u32(hits)
    n = h.shape[0] if n is None else n
    d_h = _dev(h) if h.shape[0] else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    d_f = _dev(np.asarray(refl, np.float32)) if refl is not None else None
    d_c = _dev(np.array([count], np.uint32)) if count is not None else None
    d_p = torch.full(((n + 1) * 32,), FILL, dtype=torch.uint8, device="cuda:0")
    d_o = torch.full(((n + 1) * 16,), FILL, dtype=torch.uint8, device="cuda:0")
    d_n = torch.full((16,), FILL, dtype=torch.uint8, device="cuda:0")
    d_pose, n_cols, tabs, keep = _tables(pose, motions, skew)
    torch.cuda.synchronize()
    rc = tr.applyReturnModelMovingDevice(model, d_h.data_ptr(), n, d_n.data_ptr(), d_points32=d_p.data_ptr() if points else 0,
                                         d_hits_out=d_o.data_ptr() if records else 0, d_col_pose=d_pose, n_cols=n_cols, motions=tabs, flags=flags,
                                         d_count=d_c.data_ptr() if d_c is not None else 0, d_reflectivity=d_f.data_ptr() if d_f is not None else 0,
                                         n_reflectivity=len(refl) if refl is not None else 0, frame_index=frame, stream=stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    word = d_n.cpu().numpy()
    k = int(word[:4].view(np.uint32)[0])
    assert np.all(word[4:] == FILL) and k <= n
    p, o = d_p.cpu().numpy(), d_o.cpu().numpy()
    assert np.all(p[(k if points else 0) * 32:] == FILL) and np.all(o[(k if records else 0) * 16:] == FILL)      # nothing past record k
    return (p[:k * 32].reshape(k, 32).copy() if points else None), (o[:k * 16].view(np.uint32).reshape(k, 4).copy() if records else None), k


def _attr_host(tr, hits, pose, motions, flags=0):
    rc, rec = tr.hitAttributesMoving(hits, pose, motions, flags)
    assert rc == 0
    return _u32(rec)


def _returns_host(tr, model, hits, pose, motions, flags=0, refl=None, frame=0):
    rc, p, h = tr.applyReturnModelMoving(model, hits, pose, motions, flags, refl, frame)
    assert rc == 0
    return p, _hits_u32(h)


def _same(got, want):
    bad = np.nonzero(np.any(got != want, axis=1))[0] if got.shape == want.shape else None
    assert bad is not None and bad.size == 0, (got.shape, want.shape, None if bad is None else (bad[:10], got[bad[:3]], want[bad[:3]]))


def _same_returns(got, want):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (got[0].shape, want[0].shape, got[1].shape, want[1].shape)
    bad = np.nonzero(np.any(got[0] != want[0], axis=1) | np.any(got[1] != want[1], axis=1))[0]
    assert bad.size == 0, (bad[:10], got[0][bad[:2]].view(np.uint32), want[0][bad[:2]].view(np.uint32), got[1][bad[:3]], want[1][bad[:3]])


_cache = {}


def _frames(oracle, capi, sensors, meshes):
    """_scene of test_gpu_sweep_moving -- the sensor on a twist, ben on a twist -- traced once per flag, and the restatement of its
    records' attributes: computed once, shared by the tests that need them, never changed -> (tracer, {flags: (hits uint32 (k, 4),
    points uint8 (k, 32), the restated records, the rays the columns cast)})"""
    if "frames" not in _cache:
        s, ml, pose, rays, motion, contrib = _scene(oracle, capi, sensors, meshes)
        tr = make_tracer(capi, s)
        _ground_ben(tr, oracle, meshes)
        scene = oracle.assemble_scene(s, ml)
        per_flag = {}
        for flags in (0, capi.LS_SWEEP_DESKEW):
            k, p, h = _moving(tr, pose, {1: motion}, flags=flags)
            want, cast = _define(capi, scene, oracle.ray_dirs(s), s.H, h, pose, {1: motion}, bool(flags))
            for a in (p, h, want, cast):
                a.setflags(write=False)
            per_flag[flags] = (h, p, want, cast)
        tr.close()
        _cache["frames"] = per_flag
    return _cache["frames"]


# ---- 1. degenerate: the sensor and the scene at rest --------------------------------------------------------------------------

def test_at_rest_equals_the_static_calls(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    rc, pts, hits = tr.traceScene(0)
    assert rc == 0 and len(pts) == 1781
    rc, rec = tr.hitAttributes(hits)
    assert rc == 0 and np.all(rec["flags"] == 1)
    m = _full_model(capi)
    rc, wp, wh = tr.applyReturnModel(m, hits, None, REFL, 5)
    assert rc == 0 and 100 < wh.shape[0] < 1781
    for flags in (0, capi.LS_SWEEP_DESKEW):                       # at rest the flag changes nothing
        _same(_attr_host(tr, hits, None, {}, flags), _u32(rec))
        _same(_attr_device(tr, hits, None, {}, flags), _u32(rec))
        _same_returns(_returns_host(tr, m, hits, None, {}, flags, REFL, 5), (wp, _hits_u32(wh)))
        p, h, k = _returns_device(tr, m, hits, None, {}, flags, REFL, 5)
        assert k == wh.shape[0]
        _same_returns((p, h), (wp, _hits_u32(wh)))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 2. degenerate: the sensor on a twist, the scene at rest ------------------------------------------------------------------

def test_sweep_without_motion_equals_the_caller_ray_detour(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    pose = _twist_poses(capi, s)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    ident = _identity_tables(tr, s)
    k, p, h, r = _sweep(tr, pose, flags=capi.LS_SWEEP_DESKEW, rays=True)
    k0, p0, h0, _ = _sweep(tr, pose, flags=0)
    assert k > 1000 and k0 == k and np.array_equal(h0, h)
    rc, rec = tr.hitAttributes(h, r)                             # the detour: the sweep's rays as caller rays
    assert rc == 0 and np.all(rec["flags"] == 1)
    want = _u32(rec)
    m = _full_model(capi, range_min=0.0)
    rc, wp, wh = tr.applyReturnModel(m, h, r, REFL, 3)
    assert rc == 0 and 100 < wh.shape[0] < k
    ringed = wp.copy()
    ringed[:, 20:24] = (_hits_u32(wh)[:, 0] // s.H).astype(np.uint32).view(np.uint8).reshape(-1, 4)      # the ring is v here, 0 there
    assert np.all(wp[:, 20:24] == 0) and np.any(ringed[:, 20:24] != 0)
    for motions in ({}, ident):
        for run in (_attr_host, _attr_device):
            got = run(tr, h, pose, motions, capi.LS_SWEEP_DESKEW)
            if motions:      # an identity record gives the normal back numerically: a -0 may come back as +0
                assert np.array_equal(got[:, 0:3].view(F), want[:, 0:3].view(F))
                _same(got[:, 3:], want[:, 3:])
            else:
                _same(got, want)
            # flags 0: the point the sensor reports, the bits of the skewed frame
            got0 = run(tr, h, pose, motions, 0)
            _same(got0[:, 0:8], got[:, 0:8])
            assert _same_bits(got0[:, 8:11], p0[:, 0:12].copy().view(np.uint32).reshape(k, 3)) and np.array_equal(got0[:, 11], h[:, 0])
        _same_returns(_returns_host(tr, m, h, pose, motions, capi.LS_SWEEP_DESKEW, REFL, 3), (ringed, _hits_u32(wh)))
        gp, gh, gk = _returns_device(tr, m, h, pose, motions, capi.LS_SWEEP_DESKEW, REFL, 3)
        assert gk == wh.shape[0]
        _same_returns((gp, gh), (ringed, _hits_u32(wh)))
        # the identity model with flags 0: the skewed frame itself, ring included
        ip, ih, ik = _returns_device(tr, capi.ReturnModel(), h, pose, motions, 0)
        assert ik == k and _same_bits(ip, p0) and np.array_equal(ih, h)
        ip, ih, ik = _returns_device(tr, capi.ReturnModel(), h, pose, motions, capi.LS_SWEEP_DESKEW)
        assert ik == k and _same_bits(ip, p) and np.array_equal(ih, h)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 3. the definition under real motion ------------------------------------------------------------------------------------

def test_moving_ben_equals_the_restatement(oracle, capi, sensors, meshes):
    s, ml, pose, rays, motion, contrib = _scene(oracle, capi, sensors, meshes)
    frames = _frames(oracle, capi, sensors, meshes)
    dirs = oracle.ray_dirs(s)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    m = _full_model(capi, range_min=0.0)
    for flags in (0, capi.LS_SWEEP_DESKEW):
        h, p, want, cast = frames[flags]
        assert np.all(want[:, 7] == 1) and set(h[:, 1]) == {0, 1}           # every record the frame emitted is valid
        got = _attr_device(tr, h, pose, {1: motion}, flags)
        _same(got, want)
        _same(_attr_host(tr, h, pose, {1: motion}, flags), want)
        assert _same_bits(got[:, 8:11], p[:, 0:12].copy().view(np.uint32).reshape(-1, 3))      # p: the frame's own points32 xyz
        nrm = got[:, 0:3].view(F).astype(np.float64)
        assert np.all(np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-6)
        # ground is at rest: its normals are those ls_hit_attributes finds with the sweep's rays as caller rays
        ground = h[:, 1] == 0
        rc, rec = tr.hitAttributes(h[ground], rays)
        assert rc == 0 and np.all(rec["flags"] == 1) and np.array_equal(got[ground, 0:3], _u32(rec)[:, 0:3])
        wr = _define_returns(capi, m, h, want, cast, dirs, s.H, bool(flags), REFL, 9)
        assert 100 < wr[1].shape[0] < h.shape[0] and set(wr[1][:, 1]) == {0, 1}
        _same_returns(_returns_host(tr, m, h, pose, {1: motion}, flags, REFL, 9), wr)
        gp, gh, gk = _returns_device(tr, m, h, pose, {1: motion}, flags, REFL, 9)
        assert gk == wr[1].shape[0]
        _same_returns((gp, gh), wr)
        # the identity model keeps every record: the frame's own cloud, ring included
        ip, ih, ik = _returns_device(tr, capi.ReturnModel(), h, pose, {1: motion}, flags)
        assert ik == h.shape[0] and _same_bits(ip, p) and np.array_equal(ih, h)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 4. the meaning of a record, exactly ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("half_turn", [False, True])
def test_attributes_mean_the_geometry_reposed_exactly(oracle, capi, half_turn):
    """the box and plate of test_gpu_sweep_moving, the box displaced by c_h = (h / 16, -h / 32, 0) and Q the identity or a half turn
    about z: the attributes of the moving frame's records against ls_trace_rays + ls_hit_attributes on the box re-posed per column
    (test_gpu_sweep_moving._reposed_per_column's loop, with the attributes taken inside it).  t, cos_inc, u, v and tri by bits, the
    normal numerically; test_attr_moving_cpu.test_translation_and_half_turn_are_exact_on_the_host says the reference alone is exact."""
    s, A0, motion, rays = box_case(oracle, half_turn)
    n, cols = s.V * s.H, np.arange(s.V * s.H) % s.H
    tr = make_tracer(capi, s)
    bx = box()
    _add(tr, "box", *bx)
    _add(tr, "plate", *PLATE)
    tr.updateGeometry("box", A0, *bx)
    tr.updateGeometry("plate", oracle.IDENTITY_AFFINE, *PLATE)
    assert tr.commitScene() == 0
    ref_h, ref_a = np.zeros((n, 4), np.uint32), np.zeros((n, 12), np.uint32)
    for h in range(s.H):
        tr.updateGeometryTransform("box", compose(motion[h], A0))
        assert tr.commitScene() == 0
        mine = np.nonzero(cols == h)[0]
        rc, hits = tr.traceRays(rays[mine])
        assert rc == 0
        rc2, rec = tr.hitAttributes(hits, rays[mine])
        assert rc2 == 0
        ref_h[mine], ref_a[mine] = _records(hits), _u32(rec)
        ref_h[mine, 0] = mine
    tr.updateGeometryTransform("box", A0)
    assert tr.commitScene() == 0
    hit = ref_h[:, 1] != INV
    assert np.count_nonzero(ref_h[:, 1] == 0) >= 16 and np.count_nonzero(ref_h[:, 1] == 1) >= 16
    k, p, h = _moving(tr, None, {0: motion})
    assert np.array_equal(h, ref_h[hit])                                 # ray, geom, prim and the bits of t
    want = ref_a[hit]
    for got in (_attr_host(tr, h, None, {0: motion}), _attr_device(tr, h, None, {0: motion})):
        assert np.all(got[:, 7] == 1) and np.all(want[:, 7] == 1)
        _same(got[:, 3:8], want[:, 3:8])                                 # cos_inc, u, v, tri, flags
        assert np.array_equal(got[:, 0:3].view(F), want[:, 0:3].view(F))       # the normal: Q n_g, numerically
        assert np.array_equal(got[:, 8:11].view(F), want[:, 8:11].view(F))     # t * d against 0 + t * d
        assert _same_bits(got[:, 8:11], p[:, 0:12].copy().view(np.uint32).reshape(-1, 3))
    if half_turn:      # the normals did turn: without the way back they would point the other way in x and y
        on_box = h[:, 1] == 0
        static = _u32(tr.hitAttributes(h[on_box], restate_motion_rays(rays, motion[cols]))[1])
        assert np.all(static[:, 7] == 1)
        sn, gn = static[:, 0:3].view(F), got[on_box, 0:3].view(F)
        assert np.array_equal(gn[:, 0:2], -sn[:, 0:2]) and np.array_equal(gn[:, 2], sn[:, 2]) and np.any(sn[:, 0:2] != 0)
    tr.close()


# ---- 5. tables that do not belong to the frame ----------------------------------------------------------------------------------

def test_wrong_tables_invalidate_the_geometries_concerned(oracle, capi, sensors, meshes):
    s, ml, pose, rays, motion, contrib = _scene(oracle, capi, sensors, meshes)
    h, p, want, cast = _frames(oracle, capi, sensors, meshes)[0]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    ben = h[:, 1] == 1
    # ben's table omitted: ben is taken to be at rest, and the exact test from the column's ray fails for most of its records
    got = _attr_device(tr, h, pose, {})
    assert np.count_nonzero(got[ben, 7] == 0) > np.count_nonzero(ben) // 2 and np.all(got[~ben, 7] == 1)
    _same(got[~ben], want[~ben])
    gone = got[ben & (got[:, 7] == 0)]
    assert not gone[:, 0:11].any() and np.array_equal(gone[:, 11], h[ben & (got[:, 7] == 0), 0])      # zeros everywhere but `ray`
    m = capi.ReturnModel()
    gp, gh, gk = _returns_device(tr, m, h, pose, {})
    assert gk == np.count_nonzero(got[:, 7] == 1) and np.array_equal(gh, h[got[:, 7] == 1])
    # a NaN record in one column: ben's records of that column are invalid, every other record is unchanged
    col = int(np.argmax(np.bincount(h[ben, 0] % s.H, minlength=s.H)))
    for entry, value in ((5, np.nan), (3, np.inf)):
        bad = motion.copy()
        bad[col, entry] = value
        hidden = ben & (h[:, 0] % s.H == col)
        assert np.count_nonzero(hidden) > 0
        got = _attr_device(tr, h, pose, {1: bad})
        assert np.all(got[hidden, 7] == 0) and not got[hidden, 0:11].any()
        _same(got[~hidden], want[~hidden])
        gp, gh, gk = _returns_device(tr, m, h, pose, {1: bad})
        assert gk == np.count_nonzero(~hidden) and np.array_equal(gh, h[~hidden]) and _same_bits(gp, p[~hidden])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 6. many geometries ---------------------------------------------------------------------------------------------------------

def test_eighteen_geometries_a_quad_and_an_id_gap(oracle, capi, sensors):
    """nineteen plates on a ring around the sensor, the last one a quad mesh; g7 is removed before the commit: eighteen geometries,
    geomIDs 0 .. 18 without 7.  Five of them, the quad among them, move on twists of their own; the sensor is on a twist too."""
    s = sensors["0000"]
    xs, ys = np.meshgrid(np.linspace(-3, 3, 7), np.linspace(-2, 2, 5), indexing="xy")
    pv = np.stack([xs, ys, 0.3 * xs], -1).reshape(-1, 3).astype(np.float32)
    pq = np.array([[j * 7 + i, j * 7 + i + 1, j * 7 + i + 8, j * 7 + i + 7] for j in range(4) for i in range(6)], np.uint32)
    pt = oracle.quads_to_triangles(pq)
    rng = np.random.default_rng(18)
    tr = make_tracer(capi, s)
    ml, motions = [], {}
    for k in range(19):
        ang = 2 * np.pi * k / 19
        lin = np.float32([s.t[0] + 10.0 * np.cos(ang), s.t[1] + 10.0 * np.sin(ang), s.t[2] - 1.0 + rng.uniform(-0.5, 0.5)])
        A = oracle.affine_from_components(lin, np.float32([rng.uniform(-0.3, 0.3), 1.2 + rng.uniform(-0.3, 0.3), ang]))
        elems, gtype = (pq, capi.LS_GEOMETRY_TYPE_QUAD) if k == 18 else (pt, 0)
        assert _add(tr, f"g{k}", pv, elems, gtype) == k
        tr.updateGeometry(f"g{k}", A, pv, elems)
        if k != 7:
            ml.append((k, pv, elems, A))
        if k in (0, 5, 11, 16, 18):
            c = oracle.transform_vertices(pv, A, s).astype(np.float64).mean(0)
            across = np.cross([0.0, 0.0, 1.0], c / np.linalg.norm(c)) * rng.uniform(-8.0, 8.0)
            motions[k] = capi.motion_constant_twist(across, (0.2, -0.1, rng.uniform(-1.5, 1.5)), c, -0.5 * TURN, TURN / s.H, s.H)
    assert tr.removeGeometry("g7") >= 0
    assert tr.commitScene() == 0 and tr.getGeometryCount() == 18
    scene = oracle.assemble_scene(s, ml)
    assert sorted(int(g) for g in scene.geom_ids) == [k for k in range(19) if k != 7] and bool(scene.geom_quad[-1])
    pose = _twist_poses(capi, s)
    dirs = oracle.ray_dirs(s)
    m = _full_model(capi, range_min=0.0)
    refl = [0.05 + 0.05 * k for k in range(19)]
    for flags in (0, capi.LS_SWEEP_DESKEW):
        k, p, h = _moving(tr, pose, motions, flags=flags)
        seen = set(int(g) for g in h[:, 1])
        assert set(motions) <= seen and len(seen) >= 12 and 7 not in seen
        want, cast = _define(capi, scene, dirs, s.H, h, pose, motions, bool(flags))
        assert np.all(want[:, 7] == 1)
        quad = h[:, 1] == 18
        assert set(want[quad, 6] - 2 * h[quad, 2]) == {0, 1}               # both halves of the quads are met
        _same(_attr_device(tr, h, pose, motions, flags), want)
        _same(_attr_host(tr, h, pose, motions, flags), want)
        assert _same_bits(want[:, 8:11], p[:, 0:12].copy().view(np.uint32).reshape(-1, 3))
        wr = _define_returns(capi, m, h, want, cast, dirs, s.H, bool(flags), refl, 2)
        assert 50 < wr[1].shape[0] < k
        gp, gh, gk = _returns_device(tr, m, h, pose, motions, flags, refl, 2)
        assert gk == wr[1].shape[0]
        _same_returns((gp, gh), wr)
        _same_returns(_returns_host(tr, m, h, pose, motions, flags, refl, 2), wr)
    # records that name the gap, an id past the table, an element or a ray out of range: invalid, nothing read
    odd = h[:5].copy()
    odd[0, 1], odd[1, 1], odd[2, 2], odd[3, 0], odd[4, 1] = 7, 19, 10 ** 6, s.V * s.H, INV
    got = _attr_device(tr, odd, pose, motions)
    assert not got[:, 0:11].any() and np.array_equal(got[:, 11], odd[:, 0])
    assert _returns_device(tr, m, odd, pose, motions)[2] == 0
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 7. shards ------------------------------------------------------------------------------------------------------------------

def test_a_shard_handle_gives_the_full_handles_bytes(oracle, capi, sensors, meshes):
    s, ml, pose, rays, motion, contrib = _scene(oracle, capi, sensors, meshes)
    frames = _frames(oracle, capi, sensors, meshes)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    m = _full_model(capi, range_min=0.0)
    for flags in (0, capi.LS_SWEEP_DESKEW):
        hf, pf, want, cast = frames[flags]
        tr.setShard(0, s.H)
        fp, fh, fk = _returns_device(tr, m, hf, pose, {1: motion}, flags, REFL, 4)
        assert 100 < fk < hf.shape[0]
        first, count = 37, 61
        tr.setShard(first, count)
        k, p, h = _moving(tr, pose, {1: motion}, flags=flags)           # the shard's records: global ray indices, global columns
        inside = (hf[:, 0] % s.H >= first) & (hf[:, 0] % s.H < first + count)
        assert k == np.count_nonzero(inside) > 100 and np.array_equal(h, hf[inside]) and np.any(h[:, 1] == 1) and h[:, 0].max() >= s.H
        _same(_attr_device(tr, h, pose, {1: motion}, flags), want[inside])
        _same(_attr_host(tr, h, pose, {1: motion}, flags), want[inside])
        kept = (fh[:, 0] % s.H >= first) & (fh[:, 0] % s.H < first + count)
        assert 10 < np.count_nonzero(kept) < fk
        gp, gh, gk = _returns_device(tr, m, h, pose, {1: motion}, flags, REFL, 4)     # the noise of the full turn: keyed by the ray
        assert gk == np.count_nonzero(kept)
        _same_returns((gp, gh), (fp[kept], fh[kept]))
        # the calls do not depend on the shard: the full frame's records through the shard handle
        _same(_attr_device(tr, hf, pose, {1: motion}, flags), want)
    tr.close()


# ---- 8. buffer variants -----------------------------------------------------------------------------------------------------------

def test_count_word_empty_input_optional_outputs_alignment_and_streams(oracle, capi, sensors, meshes):
    import torch
    s, ml, pose, rays, motion, contrib = _scene(oracle, capi, sensors, meshes)
    h, p, want, cast = _frames(oracle, capi, sensors, meshes)[capi.LS_SWEEP_DESKEW]
    flags = capi.LS_SWEEP_DESKEW
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    ident = np.tile(IDENTITY_POSE, (s.H, 1))
    m = _full_model(capi, range_min=0.0)
    wr = _returns_host(tr, m, h, pose, {1: motion}, flags, REFL, 1)
    n = h.shape[0]
    assert 100 < wr[1].shape[0] < n
    # a device count below n, at a block boundary and off it; a count above n
    for count in (0, 1, 255, 256, 257, 1000, n + 7):
        c = min(count, n)
        _same(_attr_device(tr, h, pose, {1: motion}, flags, count=count), want[:c])
        part = wr[1][:, 0] <= h[c - 1, 0] if c else np.zeros(wr[1].shape[0], bool)      # (ascending ray indices: a prefix of the kept ones)
        gp, gh, gk = _returns_device(tr, m, h, pose, {1: motion}, flags, REFL, 1, count=count)
        assert gk == np.count_nonzero(part)
        _same_returns((gp, gh), (wr[0][part], wr[1][part]))
    # n = 0: LS_OK, *d_n_out = 0, nothing else written
    assert _attr_device(tr, h[:0], pose, {1: motion}, flags).shape == (0, 12)
    assert _returns_device(tr, m, h[:0], pose, {1: motion}, flags)[2] == 0
    assert _attr_host(tr, h[:0], pose, {1: motion}, flags).shape == (0, 12)
    gp, gh = _returns_host(tr, m, h[:0], pose, {1: motion}, flags)
    assert gp.shape[0] == 0 and gh.shape[0] == 0
    # optional outputs
    gp, gh, gk = _returns_device(tr, m, h, pose, {1: motion}, flags, REFL, 1, records=False)
    assert gk == wr[1].shape[0] and gh is None and np.array_equal(gp, wr[0])
    gp, gh, gk = _returns_device(tr, m, h, pose, {1: motion}, flags, REFL, 1, points=False)
    assert gk == wr[1].shape[0] and gp is None and np.array_equal(gh, wr[1])
    assert _returns_device(tr, m, h, pose, {1: motion}, flags, REFL, 1, points=False, records=False)[2] == wr[1].shape[0]
    # tables 4-byte but not 16-byte aligned, an identity table for the ground next to ben's, a caller stream
    qs = torch.cuda.Stream()
    for skew, stream in ((4, None), (12, None), (8, qs.cuda_stream), (0, qs.cuda_stream)):
        got = _attr_device(tr, h, pose, {1: motion, 0: ident}, flags, skew=skew, stream=stream)
        assert np.array_equal(got[:, 0:3].view(F), want[:, 0:3].view(F))
        _same(got[:, 3:], want[:, 3:])
        gp, gh, gk = _returns_device(tr, m, h, pose, {1: motion}, flags, REFL, 1, skew=skew, stream=stream)
        assert gk == wr[1].shape[0]
        _same_returns((gp, gh), wr)
    # the host variants equal the device's (host memory may have any alignment)
    _same(_attr_host(tr, h, pose, {1: motion}, flags), want)
    odd = np.zeros(s.H * 48 + 1, np.uint8)
    odd[1:] = motion.view(np.uint8).reshape(-1)
    mo = (capi.GeometryMotion * 1)()
    mo[0].geom, mo[0].col_motion = 1, odd.ctypes.data + 1
    out = np.zeros((n, 12), np.uint32)
    assert tr.L.ls_hit_attributes_moving_host(tr.h, pose.ctypes.data, s.H, mo, 1, flags, h.ctypes.data, n, out.ctypes.data) == 0
    _same(out, want)
    pts, k_out = np.full((n, 32), FILL, np.uint8), ctypes.c_uint32(0)
    refl = np.float32(REFL)
    assert tr.L.ls_apply_return_model_moving_host(tr.h, ctypes.byref(m), 1, pose.ctypes.data, s.H, mo, 1, flags, h.ctypes.data, n, refl.ctypes.data, 2,
                                                  pts.ctypes.data, None, ctypes.byref(k_out)) == 0
    assert k_out.value == wr[1].shape[0] and np.array_equal(pts[:k_out.value], wr[0]) and np.all(pts[k_out.value:] == FILL)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 9. the overrun guard -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 64, 255, 256, 257, 513])
def test_canaries_behind_every_output(oracle, capi, sensors, meshes, n):
    """record counts around the wave and workgroup sizes: one canary record behind every output -- and everything between the kept
    records and it -- stays untouched (the helpers check it), with the tables, with a count word equal to n, and without outputs"""
    s, ml, pose, rays, motion, contrib = _scene(oracle, capi, sensors, meshes)
    h, p, want, cast = _frames(oracle, capi, sensors, meshes)[0]
    assert h.shape[0] >= 513
    pick = np.linspace(0, h.shape[0] - 1, n).astype(np.int64)            # ground and ben, ascending ray index
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    _same(_attr_device(tr, h[pick], pose, {1: motion}), want[pick])
    _same(_attr_device(tr, h[pick], pose, {1: motion}, count=n), want[pick])
    gp, gh, gk = _returns_device(tr, capi.ReturnModel(), h[pick], pose, {1: motion})
    assert gk == n and np.array_equal(gh, h[pick]) and _same_bits(gp, p[pick])
    gp, gh, gk = _returns_device(tr, capi.ReturnModel(dropout=0.5, seed=3), h[pick], pose, {1: motion}, count=n)
    assert gk <= n and np.all(np.isin(gh[:, 0], h[pick, 0])) and np.all(np.diff(gh[:, 0].astype(np.int64)) > 0)
    tr.close()


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order_and_the_state_a_call_leaves(oracle, capi, sensors, meshes):
    """every refusal of the header, alone and together with the one after it (the earlier one answers: ls_last_error says which),
    with nothing written.  A removal commits the remaining scene itself (ls_remove_geometry), so LS_ERR_NOT_COMMITTED -- a layout
    entry whose geometry is gone -- is not reachable through the public entry points, for these calls as for ls_hit_attributes and
    ls_trace_scene_sweep_moving: the calls follow the remaining scene, the removed geometry's records are invalid and a motion that
    names it is LS_ERR_UNKNOWN_GEOMETRY."""
    import torch
    s = sensors["0000"]
    n = 8
    pose = _twist_poses(capi, s)
    ident = np.tile(IDENTITY_POSE, (s.H, 1))
    d_pose, d_tab = torch.from_numpy(pose).to("cuda:0"), torch.from_numpy(ident).to("cuda:0")
    d_h = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    d_f = torch.ones(4, dtype=torch.float32, device="cuda:0")
    bufs = {k: torch.full((size,), FILL, dtype=torch.uint8, device="cuda:0") for k, size in (("a", n * 48 + 64), ("p", n * 32 + 64), ("o", n * 16 + 64),
                                                                                             ("c", 64))}
    torch.cuda.synchronize()
    A_, P_, O_, C_ = (bufs[k].data_ptr() for k in "apoc")
    hits = np.zeros(n, capi.HIT_DTYPE)
    host_a, host_p, host_n = np.full((n, 48), FILL, np.uint8), np.full((n, 32), FILL, np.uint8), ctypes.c_uint32(0xABABABAB)
    m = capi.ReturnModel()

    def untouched():
        torch.cuda.synchronize()
        return all(np.all(b.cpu().numpy() == FILL) for b in bufs.values()) and host_n.value == 0xABABABAB and \
            np.all(host_a == FILL) and np.all(host_p == FILL)

    def motions(entries):
        arr = (capi.GeometryMotion * max(1, len(entries)))()
        for mo, (g, r, t) in zip(arr, entries):
            mo.geom, mo.reserved, mo.col_motion = g, r, t
        return arr

    TAB, HTAB = d_tab.data_ptr(), ident.ctypes.data
    base = dict(model=m, pose=d_pose.data_ptr(), n_cols=s.H, entries=[(1, 0, TAB)], null_motions=False, n_motions=None, flags=0, hits=d_h.data_ptr(),
                count=None, n=n, refl=None, n_refl=0, a=A_, p=P_, o=O_, c=C_)

    def args(a):
        nm = len(a["entries"]) if a["n_motions"] is None else a["n_motions"]
        return a["pose"], a["n_cols"], None if a["null_motions"] else motions(a["entries"]), nm, a["flags"]

    def model_of(a):
        return None if a["model"] is None else ctypes.byref(a["model"])

    def attr(tr, **kw):
        a = {**base, **kw}
        return tr.L.ls_hit_attributes_moving(tr.h, None, *args(a), a["hits"], a["count"], a["n"], a["a"])

    def rets(tr, **kw):
        a = {**base, **kw}
        return tr.L.ls_apply_return_model_moving(tr.h, None, model_of(a), 0, *args(a), a["hits"], a["count"], a["n"], a["refl"], a["n_refl"],
                                                 a["p"], a["o"], a["c"])

    host_base = dict(base, pose=pose.ctypes.data, entries=[(1, 0, HTAB)], hits=hits.ctypes.data, a=host_a.ctypes.data, p=host_p.ctypes.data, o=None,
                     c=ctypes.byref(host_n))

    def attr_host(tr, **kw):
        a = {**host_base, **kw}
        return tr.L.ls_hit_attributes_moving_host(tr.h, *args(a), a["hits"], a["n"], a["a"])

    def rets_host(tr, **kw):
        a = {**host_base, **kw}
        return tr.L.ls_apply_return_model_moving_host(tr.h, model_of(a), 0, *args(a), a["hits"], a["n"], a["refl"], a["n_refl"], a["p"], a["o"], a["c"])

    every = (attr, rets, attr_host, rets_host)
    tr = make_tracer(capi, s)
    # -1 with no commit writes nothing; the argument checks and the record limit come before it, an unknown geometry after it
    assert [f(tr, entries=[]) for f in every] == [-1] * 4 and untouched()
    _add(tr, "ground", *meshes["ground"])
    _add(tr, "face", *meshes["ben"])
    assert [f(tr) for f in every] == [-1] * 4 and [f(tr, entries=[(7, 0, TAB)]) for f in (attr, rets)] == [-1] * 2 and untouched()
    assert attr(tr, n_cols=s.H - 1) == INVALID_ARGUMENT and rets(tr, flags=2) == INVALID_ARGUMENT
    assert attr(tr, n=0xFFF00001) == OUT_OF_RANGE and rets(tr, n=0xFFF00001) == OUT_OF_RANGE and untouched()
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
    tr.updateGeometry("face", oracle.IDENTITY_AFFINE, *meshes["ben"])
    assert tr.commitScene() == 0
    rc, pts0, hits0 = tr.traceScene(0)
    assert rc == 0 and len(pts0) == 1781
    rc, _ = tr.traceRays(np.float32([[0, 0, 0, 0, 0.3, 0.2, -1.0, np.inf]]))
    assert rc == 0
    built = tr.info(capi.LS_INFO_RAY_QUERY_BUILT)
    assert built == 2
    # the return model checks its model and the reflectivities first
    for name, bad in bad_models(capi):
        assert rets(tr, model=bad, hits=None) == INVALID_ARGUMENT and "return model" in tr.last_error(), name
        assert rets_host(tr, model=bad, c=None) == INVALID_ARGUMENT and "return model" in tr.last_error(), name
    assert rets(tr, model=None, hits=None) == INVALID_ARGUMENT and rets_host(tr, model=None, n_cols=3) == INVALID_ARGUMENT
    assert rets(tr, n_refl=3, hits=None) == INVALID_ARGUMENT and "reflectivities" in tr.last_error()
    assert rets_host(tr, n_refl=3, c=None) == INVALID_ARGUMENT and "reflectivities" in tr.last_error()
    # then, for both calls, in the header's order: (arguments, what ls_last_error says); every one is combined with the next
    steps = [
        (dict(hits=None), "null hit records"),
        (dict(n_cols=s.H - 1), "one pose per azimuth column"),
        (dict(flags=2), "unknown sweep flags"),
        (dict(null_motions=True, n_motions=1), "null motions"),
        (dict(entries=[(1, 0, None)]), "without a table"),
        (dict(entries=[(1, 1, TAB)]), "reserved"),
        (dict(entries=[(1, 0, TAB), (1, 0, TAB)]), "two motions"),
        (dict(hits=d_h.data_ptr() + 8), "aligned"),
        (dict(n=0xFFF00001), "too many"),
        (dict(entries=[(2, 0, TAB)]), "not in the committed scene"),
    ]
    codes = [INVALID_ARGUMENT] * 8 + [OUT_OF_RANGE, UNKNOWN_GEOMETRY]
    together = {3: dict(null_motions=True, n_motions=1, entries=[]),               # NULL motions, and a table that would be NULL
                4: dict(entries=[(1, 1, None)]),                                   # a NULL table in an entry whose reserved is set
                5: dict(entries=[(1, 1, TAB), (1, 0, TAB)])}                       # reserved set in one of two entries for one geometry
    for f in (attr, rets):
        for i, (kw, says) in enumerate(steps):
            assert f(tr, **kw) == codes[i] and says in tr.last_error(), (f.__name__, i, tr.last_error())
            if i + 1 < len(steps):
                both = together.get(i, {**kw, **steps[i + 1][0]})
                assert f(tr, **both) == codes[i] and says in tr.last_error(), (f.__name__, i, tr.last_error())
    more = [
        attr(tr, a=None), rets(tr, c=None), attr_host(tr, hits=None), attr_host(tr, a=None), rets_host(tr, hits=None), rets_host(tr, c=None),
        attr(tr, n_cols=s.H + 1), attr(tr, pose=None, n_cols=s.H), rets(tr, pose=None, n_cols=1), attr(tr, flags=0x80000001),
        attr(tr, entries=[(0, 0, TAB), (1, 0, TAB), (2, 0, TAB)]),                                              # more motions than geometries
        attr(tr, a=A_ + 8), attr(tr, count=C_ + 2), attr(tr, pose=d_pose.data_ptr() + 2), attr(tr, entries=[(1, 0, TAB + 2)]),
        rets(tr, p=P_ + 8), rets(tr, o=O_ + 8), rets(tr, c=C_ + 2), rets(tr, count=C_ + 2), rets(tr, refl=d_f.data_ptr() + 2, n_refl=2),
        rets(tr, pose=d_pose.data_ptr() + 2), rets(tr, entries=[(1, 0, TAB + 2)]),
        attr_host(tr, n_cols=s.H - 1), attr_host(tr, flags=4), rets_host(tr, null_motions=True, n_motions=1), rets_host(tr, entries=[(1, 0, None)]),
        attr_host(tr, entries=[(1, 7, HTAB)]), rets_host(tr, entries=[(0, 0, HTAB), (0, 0, HTAB)]),
    ]
    assert more == [INVALID_ARGUMENT] * len(more) and untouched()
    assert attr_host(tr, entries=[(0xFFFFFFFF, 0, HTAB)]) == UNKNOWN_GEOMETRY and rets_host(tr, entries=[(2, 0, HTAB)]) == UNKNOWN_GEOMETRY
    assert attr_host(tr, n=0xFFF00001) == OUT_OF_RANGE and untouched() and tr.last_error()
    # a shard changes nothing: the tables keep H records
    tr.setShard(10, 20)
    assert attr(tr, n_cols=20) == INVALID_ARGUMENT and untouched()
    tr.setShard(0, s.H)
    # 16 bytes are enough for the records, 4 for the words and the tables; eight zero records (ray 0, geom 0, prim 0, t 0) are invalid
    assert attr(tr, a=A_ + 16) == 0 and rets(tr, p=P_ + 16, o=O_ + 16, c=C_ + 4, refl=d_f.data_ptr() + 4, n_refl=2) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    a, c = bufs["a"].cpu().numpy(), bufs["c"].cpu().numpy()
    assert np.all(a[:16] == FILL) and not a[16:16 + n * 48].any() and np.all(a[16 + n * 48:] == FILL)
    assert np.all(c[:4] == FILL) and not c[4:8].any() and np.all(c[8:] == FILL)
    assert all(np.all(bufs[k].cpu().numpy() == FILL) for k in "po")
    for b in bufs.values():
        b.fill_(FILL)
    torch.cuda.synchronize()
    # the state the calls leave: the device status, the query hierarchies, the frame
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0 and tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == built
    rc, pts1, hits1 = tr.traceScene(1)
    assert rc == 0 and len(pts1) == 1781 and _same_bits(np.asarray(pts1), np.asarray(pts0)) and np.array_equal(_records(hits1), _records(hits0))
    # a removal commits the remaining scene: the calls follow it, the removed geometry is unknown, an emptied scene is -1
    h0 = _records(hits0)
    rec = _attr_host(tr, h0, None, {})
    assert np.all(rec[:, 7] == 1)
    assert tr.removeGeometry("face") >= 0
    assert attr(tr, entries=[(1, 0, TAB)]) == UNKNOWN_GEOMETRY and rets(tr, entries=[(1, 0, TAB)]) == UNKNOWN_GEOMETRY and untouched()
    after = _attr_device(tr, h0, None, {0: ident})
    assert np.array_equal(after[:, 7] == 1, h0[:, 1] == 0) and np.array_equal(after[h0[:, 1] == 0, 3:], rec[h0[:, 1] == 0, 3:])
    assert _returns_device(tr, m, h0, None, {})[2] == np.count_nonzero(h0[:, 1] == 0)
    assert tr.removeGeometry("ground") >= 0
    assert [f(tr, entries=[]) for f in every] == [-1] * 4 and untouched()
    tr.close()


def test_open_frame_graph_is_refused_first(oracle, capi, sensors, meshes):
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
    out = torch.full((cap * 48,), FILL, dtype=torch.uint8, device="cuda:0")
    word = torch.full((4,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    m, bad = capi.ReturnModel(), capi.ReturnModel(dropout=2.0)
    host_n = ctypes.c_uint32(77)
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != 0   # the frame is being captured: the graph is open
    assert L.ls_hit_attributes_moving(tr.h, None, None, 0, None, 0, 0, h.data_ptr(), c.data_ptr(), cap, out.data_ptr()) == INVALID_ARGUMENT
    # (NULL records and a wrong n_cols as well: the open graph answers first -- but a return model's own refusal comes before it)
    assert L.ls_hit_attributes_moving(tr.h, None, None, 3, None, 0, 0, None, None, cap, None) == INVALID_ARGUMENT and "frame graph" in tr.last_error()
    assert L.ls_hit_attributes_moving_host(tr.h, None, 3, None, 0, 0, None, cap, None) == INVALID_ARGUMENT and "frame graph" in tr.last_error()
    assert L.ls_apply_return_model_moving(tr.h, None, ctypes.byref(m), 0, None, 0, None, 0, 0, h.data_ptr(), c.data_ptr(), cap, None, 0, out.data_ptr(),
                                          None, word.data_ptr()) == INVALID_ARGUMENT and "frame graph" in tr.last_error()
    assert L.ls_apply_return_model_moving_host(tr.h, ctypes.byref(m), 0, None, 0, None, 0, 0, None, 0, None, 0, None, None,
                                               ctypes.byref(host_n)) == INVALID_ARGUMENT and "frame graph" in tr.last_error()
    assert L.ls_apply_return_model_moving(tr.h, None, ctypes.byref(bad), 0, None, 0, None, 0, 0, h.data_ptr(), c.data_ptr(), cap, None, 0, out.data_ptr(),
                                          None, word.data_ptr()) == INVALID_ARGUMENT and "return model" in tr.last_error()
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert bool(torch.all(out == FILL)) and bool(torch.all(word == FILL)) and host_n.value == 77
    # the frame went out, and the handle answers again: straight from the frame's device buffers through its count word
    k = int(c[0].item())
    assert k > 0
    assert tr.applyReturnModelMovingDevice(m, h.data_ptr(), cap, word.data_ptr(), d_points32=out.data_ptr(), d_count=c.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert int(word.cpu().numpy().view(np.uint32)[0]) == k and torch.equal(out[:k * 32], p[:k * 32]) and bool(torch.all(out[k * 32:] == FILL))
    tr.close()
