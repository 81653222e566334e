"""ls_trace_scene_beams_sweep / ls_trace_scene_beams_sweep_host on the MI355X: weighted beams from a moving sensor.  Against the
two calls it joins (ls_trace_scene_beams at rest and under identity poses, ls_trace_scene_sweep with one centre sample); against an
expectation that restates the sub-rays in numpy float32 (test_beams_sweep_cpu.restate_beam_sweep_rays), runs the brute force of
test_gpu_rays on them over the oracle's scene and reduces every beam in plain Python (test_beams_sweep_cpu.reduce_beam_weighted);
lane-group shapes on an odd shard, tiny rasters, a NaN pose column, two launch batches, NULL outputs, return codes, frames around
a call, host against device.  Everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest

from conftest import make_tracer
from test_beams_cpu import FIRST, STRONGEST, INF
from test_beams_sweep_cpu import reduce_beam_weighted, restate_beam_sweep_rays
from test_gpu_beams import CENTRE, FILL, _beams, _rings5, _same_bits
from test_gpu_rays import INV, _add, _brute, _ground_ben
from test_gpu_sweep import _eighteen, _holed_grid, _sweep, _twist_poses
from test_sweep_cpu import IDENTITY_POSE, restate_rays

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, OUT_OF_RANGE = -2, -9
FRAME_EAGER = 0
F = np.float32
WEIGHTS5 = np.uint32([65535, 20000, 20000, 9000, 9000])


# ---- expectations ----------------------------------------------------------------------------------------------------------

def _subhits(oracle, s, scene, pat, pose, first=0, count=None):
    """the sub-rays of the columns [first, first + count) of the full raster (index (v * H + h) * S + s) under the per-column poses,
    through the brute force -> (r float32 (V * H, S): the reported ranges t * k, hit bool (V * H, S), dense ls_hit records uint32
    (V * H * S, 4)); the beams of the other columns stay all-miss and are not asked for"""
    st, ct, sp, cp = oracle.ray_tables(s)
    n, S = s.V * s.H, pat.shape[0]
    count = s.H - first if count is None else count
    q = np.array([v * s.H + h for v in range(s.V) for h in range(first, first + count)])
    vv, hh, ss = np.repeat(q // s.H, S), np.repeat(q % s.H, S), np.tile(np.arange(S), len(q))
    rays = restate_beam_sweep_rays(st[vv], ct[vv], cp[hh], sp[hh], pat[ss, 0], pat[ss, 1], pose[hh])
    rec = _brute(oracle, scene, rays)
    t = rec[:, 3].copy().view(np.float32)
    r, hit, dense = np.zeros((n, S), np.float32), np.zeros((n, S), bool), np.zeros((n * S, 4), np.uint32)
    rr = t * pat[ss, 2]
    assert rr.dtype == np.float32
    r[q], hit[q] = rr.reshape(-1, S), (rec[:, 1] != INV).reshape(-1, S)
    dense.reshape(n, S, 4)[q] = rec.reshape(-1, S, 4)
    for a in (r, hit, dense):
        a.setflags(write=False)
    return r, hit, dense


def _expect(oracle, s, sub, S, returns, min_count, separation, weights=None, min_weight=0, pose=None, deskew=False, first=0, count=None):
    """-> (hits uint32 (k, 4), points uint8 (k, 32), echo uint32 (k,), records per beam int (rays,), strengths int (k,)) of the
    columns [first, first + count): ascending global ray index, ascending range inside a beam; xyz = r_e * d, or o_h + r_e * d'
    (one product, one sum) when deskewing; intensity (64 W_e) / W_total; ring v"""
    r, hit, dense = sub
    count = s.H - first if count is None else count
    st, ct, sp, cp = oracle.ray_tables(s)
    v_of, h_of = np.arange(s.V * s.H) // s.H, np.arange(s.V * s.H) % s.H
    dirs = np.stack([st[v_of] * cp[h_of], st[v_of] * sp[h_of], ct[v_of]], axis=1)      # the nominal d: the frame's factor-table products
    assert dirs.dtype == np.float32
    hits, echo, strength, per_beam = [], [], [], np.zeros(s.V * s.H, np.int64)
    for q in range(s.V * s.H):
        if not first <= q % s.H < first + count:
            continue
        recs = reduce_beam_weighted(r[q], hit[q], returns, min_count, separation, weights, min_weight)
        per_beam[q] = len(recs)
        for bits, word, W in recs:
            d = dense[q * S + (word >> 16)]
            hits.append((q, d[1], d[2], bits))
            echo.append(word)
            strength.append(W)
    hits = np.array(hits, np.uint32).reshape(-1, 4)
    echo, strength = np.array(echo, np.uint32), np.array(strength, np.int64)
    k = len(echo)
    p = np.zeros((k, 8), np.uint32)
    ray = hits[:, 0].astype(np.int64)
    re = hits[:, 3].copy().view(np.float32)
    if deskew and pose is not None:
        carried = restate_rays(dirs[ray], pose[ray % s.H])
        xyz = carried[:, 0:3] + re[:, None] * carried[:, 4:7]
    else:
        xyz = re[:, None] * dirs[ray]
    assert xyz.dtype == np.float32
    p[:, 0:3] = xyz.view(np.uint32)
    total = S if weights is None else int(np.asarray(weights, np.int64).sum())
    p[:, 4] = ((F(64.0) * strength.astype(np.float32)) / F(total)).astype(np.float32).view(np.uint32)
    p[:, 5] = ray // s.H
    return hits, p.view(np.uint8).reshape(-1, 32), echo, per_beam, strength


_cache = {}


def _xt32(oracle, capi, sensors, meshes):
    """XT-32 0000 over ground + ben under the twist with the five-sample pattern: the scene, the poses and the brute force's
    sub-hits -- computed once, shared by the tests that need them, never changed"""
    if "xt32" not in _cache:
        s = sensors["0000"]
        ml = [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], oracle.IDENTITY_AFFINE)]
        scene = oracle.assemble_scene(s, ml)
        pose, pat = _twist_poses(capi, s), _rings5(capi)
        pose.setflags(write=False)
        _cache["xt32"] = (s, ml, scene, pose, pat, _subhits(oracle, s, scene, pat, pose))
    return _cache["xt32"]


# ---- the device entry point ------------------------------------------------------------------------------------------------

def _bs(tr, model, weights=None, min_weight=0, pose=None, flags=0, points=True, hits=True, echo=True, stream=None):
    """ls_trace_scene_beams_sweep with capacity exactly K x the shard's ray count and one canary record behind every buffer (the
    scheme of test_gpu_beams._beams) -> (k, points uint8 (k, 32) | None, hits uint32 (k, 4) | None, echo uint32 (k,) | None);
    whatever lies past record k, the canary included, must still hold the fill pattern"""
    import torch
    cap = model.n_returns * tr.getTotalRays()
    d_pose = None if pose is None else torch.from_numpy(np.array(pose, np.float32)).to("cuda:0")
    p = torch.full(((cap + 1) * 32,), FILL, dtype=torch.uint8, device="cuda:0") if points else None
    h = torch.full(((cap + 1) * 16,), FILL, dtype=torch.uint8, device="cuda:0") if hits else None
    e = torch.full(((cap + 1) * 4,), FILL, dtype=torch.uint8, device="cuda:0") if echo else None
    c = torch.full((16,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = tr.traceBeamsSweepDevice(model, c.data_ptr(), cap, p.data_ptr() if points else 0, h.data_ptr() if hits else 0, e.data_ptr() if echo else 0,
                                  weights=weights, min_weight=min_weight, d_col_pose=0 if pose is None else d_pose.data_ptr(),
                                  n_cols=0 if pose is None else pose.shape[0], flags=flags, stream=stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    cw = c.cpu().numpy()
    k = int(cw[:4].view(np.uint32)[0])
    assert 0 <= k <= cap and np.all(cw[4:] == FILL)
    out = [k, None, None, None]
    for i, (buf, size) in enumerate(((p, 32), (h, 16), (e, 4)), start=1):
        if buf is not None:
            a = buf.cpu().numpy().reshape(cap + 1, size)
            assert np.all(a[k:] == FILL), "a record written past the count"
            out[i] = a[:k].copy()
    if hits:
        out[2] = out[2].view(np.uint32).reshape(k, 4)
    if echo:
        out[3] = out[3].view(np.uint32).reshape(k)
    return tuple(out)


def _check(got, want):
    k, p, h, e = got
    wh, wp, we = want[0], want[1], want[2]
    assert k == len(we)
    assert np.array_equal(h, wh)
    assert np.array_equal(e, we)
    assert _same_bits(p, wp)


def _same(a, b):
    """two (k, points, hits, echo) results, byte for byte"""
    return a[0] == b[0] and _same_bits(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


# ---- 1. unit weights, at rest or under identity poses: the beams call ------------------------------------------------------

def test_equals_the_beams_call(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    pat = _rings5(capi)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    identity = np.tile(IDENTITY_POSE, (s.H, 1))
    for returns, min_count, separation in ((7, 1, 0.25), (5, 2, 0.05)):
        model = capi.BeamModel(pat, returns, min_count, separation)
        want = _beams(tr, model)
        assert want[0] > 1500
        assert _same(_bs(tr, model), want)                                                # d_col_pose NULL
        assert _same(_bs(tr, model, flags=capi.LS_SWEEP_DESKEW), want)                    # at rest the flag changes nothing
        assert _same(_bs(tr, model, pose=identity), want)                                 # an identity table
        assert _same(_bs(tr, model, pose=identity, flags=capi.LS_SWEEP_DESKEW), want)     # an identity table with DESKEW
        assert _same(_bs(tr, model, weights=np.ones(5, np.uint32)), want)                 # weights of 1 are no weights
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 2. one centre sample: the sweep call ----------------------------------------------------------------------------------

def test_equals_the_sweep_call(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    pose = _twist_poses(capi, s)
    model = capi.BeamModel(CENTRE, FIRST, 1, INF)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for flags in (0, capi.LS_SWEEP_DESKEW):
        k, p, h, _ = _sweep(tr, pose, flags=flags)
        kb, pb, hb, eb = _bs(tr, model, pose=pose, flags=flags)
        assert k == kb > 1000 and np.array_equal(hb, h) and _same_bits(pb, p)
        assert np.all(eb == (1 | 1 << 8))
    tr.close()


# ---- 3. the general case against the brute force ---------------------------------------------------------------------------

def test_general_case_equals_the_brute_force(oracle, capi, sensors, meshes):
    """twist poses, five samples, weights (65535, 20000, 20000, 9000, 9000), min_weight 25000, separation 0.05, every return mask,
    both flags, over the full raster"""
    s, ml, scene, pose, pat, sub = _xt32(oracle, capi, sensors, meshes)
    # the expectation itself first, so that the test cannot pass vacuously
    full = _expect(oracle, s, sub, 5, 7, 1, 0.05, WEIGHTS5, 25000)
    unit = _expect(oracle, s, sub, 5, 7, 1, 0.05)
    assert np.count_nonzero(full[3] >= 2) >= 1                                   # a beam with two returns
    strongest = {int(h[0]): (int(h[3]), int(e >> 16)) for h, e in zip(full[0], full[2]) if e & STRONGEST}
    strongest_unit = {int(h[0]): (int(h[3]), int(e >> 16)) for h, e in zip(unit[0], unit[2]) if e & STRONGEST}
    assert any(strongest[q] != strongest_unit[q] for q in strongest if q in strongest_unit)     # the weights move a STRONGEST
    assert len(full[2]) < len(unit[2])                                           # the threshold removes echoes
    assert set(full[0][:, 1]) == {0, 1} and len(set(full[4])) > 5
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for returns in range(1, 8):
        model = capi.BeamModel(pat, returns, 1, 0.05)
        for flags in (0, capi.LS_SWEEP_DESKEW):
            want = _expect(oracle, s, sub, 5, returns, 1, 0.05, WEIGHTS5, 25000, pose, bool(flags))
            _check(_bs(tr, model, WEIGHTS5, 25000, pose, flags), want)
    a, b = (_expect(oracle, s, sub, 5, 7, 1, 0.05, WEIGHTS5, 25000, pose, dk)[1] for dk in (False, True))
    assert not _same_bits(a, b)                                                  # deskewing moves the points
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 4. lane-group shapes on an odd shard -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rings,per_ring", [(1, 6), (3, 5), (7, 9)])
def test_lane_group_shapes_on_an_odd_shard(oracle, capi, sensors, n_rings, per_ring):
    """S = 7 (eight lanes per beam, one idle), 16 and 64 on a 5 x 257 raster over the holed grid; the shard starts at an odd column
    and has an odd number of them: its output is the full turn's expectation restricted to its columns"""
    s0 = sensors["0000"]
    V, H, first, count = 5, 257, 37, 21
    s = oracle.Sensor(uid="odd", vertical=np.linspace(-3.0, -28.0, V).astype(np.float32), h_begin=np.float32(0.0), h_end=np.float32(360.0), h_count=H,
                      R=s0.R, Rinv=s0.Rinv, t=s0.t)
    mesh = _holed_grid()
    scene = oracle.assemble_scene(s, [(0, *mesh, oracle.IDENTITY_AFFINE)])
    pat = capi.beam_pattern_rings(0.03, 0.03, n_rings, per_ring)
    S = pat.shape[0]
    assert S in (7, 16, 64)
    weights = capi.beam_weights_gaussian(pat, 0.015, 0.015)
    total = int(weights.sum())
    pose = _twist_poses(capi, s)
    sub = _subhits(oracle, s, scene, pat, pose, first, count)
    tr = make_tracer(capi, s)
    _add(tr, "mesh", *mesh)
    tr.updateGeometry("mesh", oracle.IDENTITY_AFFINE, *mesh)
    assert tr.commitScene() == 0
    tr.setShard(first, count)
    assert tr.getTotalRays() == V * count
    seen = set()
    for returns, min_count, min_weight, separation in ((7, 1, 0, 0.02), (7, 2, total // 8, 0.5), (6, 1, total // 3, INF)):
        for flags in (0, capi.LS_SWEEP_DESKEW):
            want = _expect(oracle, s, sub, S, returns, min_count, separation, weights, min_weight, pose, bool(flags), first, count)
            _check(_bs(tr, capi.BeamModel(pat, returns, min_count, separation), weights, min_weight, pose, flags), want)
        seen |= set(want[3])
    assert {0, 1, 2} <= seen
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 5. tiny rasters: the compaction across lane-group, wave and workgroup boundaries --------------------------------------

@pytest.mark.parametrize("V,H", [(1, 1), (3, 70), (5, 257)])
def test_tiny_rasters(oracle, capi, sensors, V, H):
    s0 = sensors["0000"]
    vertical = np.linspace(-3.0, -28.0, V).astype(np.float32) if V > 1 else np.float32([-12.0])
    from lidarshooter_amd import synth
    # (no sensor of fewer than two columns: the raster of ONE ray is a two-column sensor on the shard of its first column, as in
    # test_gpu_beams.test_tiny_rasters)
    cols = max(H, 2)
    s = oracle.Sensor(uid="tiny", vertical=vertical, h_begin=np.float32(0.0 if H > 1 else 30.0), h_end=np.float32(360.0 if H > 1 else 40.0),
                      h_count=cols, R=s0.R, Rinv=s0.Rinv, t=s0.t)
    mesh = _holed_grid() if H > 1 else synth.grid_mesh(48, 40)      # (the single ray must not look through a hole)
    scene = oracle.assemble_scene(s, [(0, *mesh, oracle.IDENTITY_AFFINE)])
    pat = capi.beam_pattern_rings(0.03, 0.02, 1, 2)
    weights = np.uint32([40000, 30000, 500])
    pose = _twist_poses(capi, s)
    sub = _subhits(oracle, s, scene, pat, pose, 0, H)
    tr = make_tracer(capi, s)
    _add(tr, "mesh", *mesh)
    tr.updateGeometry("mesh", oracle.IDENTITY_AFFINE, *mesh)
    assert tr.commitScene() == 0
    tr.setShard(0, H)
    assert tr.getTotalRays() == V * H
    seen = set()
    for returns, min_count, min_weight, separation in ((7, 1, 0, 0.02), (7, 1, 501, 0.02), (3, 2, 0, 0.5)):
        for flags in (0, capi.LS_SWEEP_DESKEW):
            want = _expect(oracle, s, sub, 3, returns, min_count, separation, weights, min_weight, pose, bool(flags), 0, H)
            _check(_bs(tr, capi.BeamModel(pat, returns, min_count, separation), weights, min_weight, pose, flags), want)
        seen |= set(want[3][np.arange(V * cols) % cols < H])
    assert seen == ({0, 1, 2, 3} if V * H > 1 else {1, 2, 3})      # lanes with 0, 1, 2 and 3 records; the last block's count
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 6. a NaN in one column's pose -----------------------------------------------------------------------------------------

def test_nan_pose_column_gives_no_returns(oracle, capi, sensors, meshes):
    s, ml, scene, pose, pat, sub = _xt32(oracle, capi, sensors, meshes)
    model = capi.BeamModel(pat, 7, 1, 0.05)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for flags in (0, capi.LS_SWEEP_DESKEW):
        wh, wp, we, per_beam, _ = _expect(oracle, s, sub, 5, 7, 1, 0.05, WEIGHTS5, 25000, pose, bool(flags))
        per_col = np.bincount(wh[:, 0] % s.H, minlength=s.H)
        for col, entry in ((int(np.argmax(per_col)), 5), (s.H - 1, 3)):
            assert per_col[col] > 0
            bad = pose.copy()
            bad[col, entry] = np.nan
            keep = wh[:, 0] % s.H != col
            _check(_bs(tr, model, WEIGHTS5, 25000, bad, flags), (wh[keep], wp[keep], we[keep]))     # the other columns are unchanged
            assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 7. eighteen geometries: two launch batches of the walk ----------------------------------------------------------------

def test_eighteen_geometries_two_batches_and_the_canary(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    geoms = _eighteen(oracle, capi, s, meshes)
    scene = oracle.assemble_scene(s, [(i, v, e, A) for i, (name, v, e, A, gt) in enumerate(geoms)])
    pat = capi.beam_pattern_rings(0.01, 0.01, 1, 2)
    weights = np.uint32([65535, 30000, 30000])
    pose = _twist_poses(capi, s)
    sub = _subhits(oracle, s, scene, pat, pose)
    seen = set(sub[2][:, 1]) - {INV}
    assert {0, 16, 17} <= seen and len(seen) >= 12     # both batches, the quad mesh among them
    tr = make_tracer(capi, s)
    for name, v, e, A, gt in geoms:
        _add(tr, name, v, e, gt)
        tr.updateGeometry(name, A, v, e)
    assert tr.commitScene() == 0
    want = _expect(oracle, s, sub, 3, 7, 1, 0.25, weights, 40000, pose, True)
    assert {0, 16, 17} <= set(want[0][:, 1])
    # (_bs: capacity is exactly K x the ray count, one canary record lies behind every buffer and is checked)
    _check(_bs(tr, capi.BeamModel(pat, 7, 1, 0.25), weights, 40000, pose, capi.LS_SWEEP_DESKEW), want)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 18
    tr.close()


# ---- 8. plumbing -----------------------------------------------------------------------------------------------------------

def test_each_output_null_in_turn(oracle, capi, sensors, meshes):
    s, ml, scene, pose, pat, sub = _xt32(oracle, capi, sensors, meshes)
    want = _expect(oracle, s, sub, 5, 6, 1, 0.05, WEIGHTS5, 25000, pose, True)
    model = capi.BeamModel(pat, 6, 1, 0.05)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for points, hits, echo in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        k, p, h, e = _bs(tr, model, WEIGHTS5, 25000, pose, capi.LS_SWEEP_DESKEW, points=points, hits=hits, echo=echo)
        assert k == len(want[2])
        assert (p is None) if not points else _same_bits(p, want[1])
        assert (h is None) if not hits else np.array_equal(h, want[0])
        assert (e is None) if not echo else np.array_equal(e, want[2])
    tr.close()


def test_return_codes(oracle, capi, sensors, meshes):
    import torch
    s, ml, scene, pose, pat, sub = _xt32(oracle, capi, sensors, meshes)
    n = s.V * s.H
    cap = 3 * n
    d_pose = torch.from_numpy(np.array(pose, np.float32)).to("cuda:0")
    bufs = {k: torch.full((size,), FILL, dtype=torch.uint8, device="cuda:0") for k, size in
            (("p", cap * 32 + 64), ("h", cap * 16 + 64), ("e", cap * 4 + 64), ("c", 64))}
    torch.cuda.synchronize()
    P, H_, E, C_ = (bufs[k].data_ptr() for k in "phec")
    PD, PH = d_pose.data_ptr(), pose.ctypes.data
    host_n = ctypes.c_uint32(0xABABABAB)
    host_p, host_h, host_e = np.full((cap, 32), FILL, np.uint8), np.full((cap, 16), FILL, np.uint8), np.full((cap, 4), FILL, np.uint8)
    good = capi.BeamModel(pat, 7, 1, 0.05)
    u32p = ctypes.POINTER(ctypes.c_uint32)

    def untouched():
        torch.cuda.synchronize()
        return all(np.all(b.cpu().numpy() == FILL) for b in bufs.values()) and host_n.value == 0xABABABAB and \
            np.all(host_p == FILL) and np.all(host_h == FILL) and np.all(host_e == FILL)

    def dev(tr, m=good, w=WEIGHTS5, min_weight=25000, pd=PD, n_cols=s.H, flags=0, p=P, h=H_, e=E, c=C_, capacity=cap):
        return tr.L.ls_trace_scene_beams_sweep(tr.h, None, ctypes.byref(m) if m is not None else None, None if w is None else w.ctypes.data_as(u32p),
                                               min_weight, pd, n_cols, flags, p, h, e, c, capacity)

    def host(tr, m=good, w=WEIGHTS5, min_weight=25000, ph=PH, n_cols=s.H, flags=0, c=True, capacity=cap):
        return tr.L.ls_trace_scene_beams_sweep_host(tr.h, ctypes.byref(m) if m is not None else None, None if w is None else w.ctypes.data_as(u32p),
                                                    min_weight, ph, n_cols, flags, host_p.ctypes.data, host_h.ctypes.data, host_e.ctypes.data,
                                                    ctypes.byref(host_n) if c else None, capacity)

    tr = make_tracer(capi, s)
    assert (dev(tr), host(tr)) == (-1, -1) and untouched()                       # before a commit
    _add(tr, "ground", *meshes["ground"])
    _add(tr, "face", *meshes["ben"])
    assert (dev(tr), host(tr)) == (-1, -1) and untouched()                       # geometries without a commit
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
    tr.updateGeometry("face", oracle.IDENTITY_AFFINE, *meshes["ben"])
    assert tr.commitScene() == 0

    def model(**kw):
        m = capi.BeamModel(kw.pop("pattern", pat), 7, 1, 0.05)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    null_pattern = model()
    null_pattern.pattern = None
    reserved = model()
    reserved.reserved[2] = 5
    nan_entry, neg_k = pat.copy(), pat.copy()
    nan_entry[3, 1], neg_k[2, 2] = np.nan, 0.0
    bad_models = [None, null_pattern, reserved, model(n_samples=0), model(n_samples=65), model(returns=0), model(returns=8), model(min_count=0),
                  model(min_count=6), model(echo_separation=float("nan")), model(echo_separation=-0.5), model(pattern=nan_entry),
                  model(pattern=neg_k)]
    w0, w65536 = WEIGHTS5.copy(), WEIGHTS5.copy()
    w0[4], w65536[0] = 0, 65536
    refused = [dev(tr, m) for m in bad_models] + [host(tr, m) for m in bad_models]
    refused += [dev(tr, w=w0), host(tr, w=w0), dev(tr, w=w65536), host(tr, w=w65536),   # a weight outside 1..65535
                dev(tr, c=None), host(tr, c=False),                                      # a NULL count
                dev(tr, capacity=cap - 1), host(tr, capacity=cap - 1),                  # a small capacity (K = 3)
                dev(tr, model(returns=3), capacity=2 * n - 1),
                dev(tr, n_cols=s.H - 1), dev(tr, n_cols=s.H + 1), host(tr, n_cols=s.H - 1), dev(tr, n_cols=0), host(tr, n_cols=0),   # n_cols != H
                dev(tr, pd=None), host(tr, ph=None),                                     # no table, yet columns
                dev(tr, flags=2), dev(tr, flags=0x80000001), host(tr, flags=4), dev(tr, pd=None, n_cols=0, flags=2),   # unknown flags
                dev(tr, p=P + 8), dev(tr, h=H_ + 8), dev(tr, e=E + 2), dev(tr, c=C_ + 2), dev(tr, pd=PD + 2),         # misaligned
                dev(tr, p=P + 4, h=None, e=None)]
    assert refused == [INVALID_ARGUMENT] * len(refused) and untouched()
    assert tr.last_error()
    assert dev(tr, model(returns=3), capacity=2 * n) == 0                           # (K = 2: twice the rays are enough)
    assert dev(tr, w=None, min_weight=0) == 0 and dev(tr, pd=None, n_cols=0, flags=1) == 0
    tr.synchronize()
    bufs["p"].fill_(FILL), bufs["h"].fill_(FILL), bufs["e"].fill_(FILL), bufs["c"].fill_(FILL)
    torch.cuda.synchronize()
    # a shard: the capacity that counts is the shard's, the table still has a record per global column
    tr.setShard(10, 20)
    assert dev(tr, capacity=3 * s.V * 20 - 1) == INVALID_ARGUMENT and dev(tr, n_cols=20) == INVALID_ARGUMENT and untouched()
    tr.setShard(0, s.H)
    # the handle still answers
    want = _expect(oracle, s, sub, 5, 7, 1, 0.05, WEIGHTS5, 25000, pose)
    _check(_bs(tr, good, WEIGHTS5, 25000, pose), want)
    # a table that is only 4-byte aligned: the same bytes through the 4-byte loads
    shifted = torch.zeros(s.H * 12 + 1, dtype=torch.float32, device="cuda:0")
    shifted[1:] = d_pose.reshape(-1)
    for flags in (0, 1):
        bufs["p"].fill_(FILL), bufs["h"].fill_(FILL), bufs["e"].fill_(FILL), bufs["c"].fill_(FILL)
        torch.cuda.synchronize()
        assert (shifted.data_ptr() + 4) % 16 == 4 and dev(tr, pd=shifted.data_ptr() + 4, flags=flags) == 0
        tr.synchronize()
        w = _expect(oracle, s, sub, 5, 7, 1, 0.05, WEIGHTS5, 25000, pose, bool(flags))
        k = int(bufs["c"].cpu().numpy()[:4].view(np.uint32)[0])
        assert k == len(w[2]) and _same_bits(bufs["p"].cpu().numpy()[:32 * k].reshape(k, 32), w[1])
        assert np.array_equal(bufs["h"].cpu().numpy()[:16 * k].view(np.uint32).reshape(k, 4), w[0])
    bufs["p"].fill_(FILL), bufs["h"].fill_(FILL), bufs["e"].fill_(FILL), bufs["c"].fill_(FILL)
    torch.cuda.synchronize()
    # an emptied scene gives -1 (a removal commits the remaining scene itself, as for the calls this one joins)
    assert tr.removeGeometry("face") >= 0
    k2, p2, h2, e2 = _bs(tr, good, WEIGHTS5, 25000, pose)
    assert k2 > 0 and np.all(h2[:, 1] == 0) and np.any(want[0][:, 1] == 1)
    assert tr.removeGeometry("ground") >= 0
    assert (dev(tr), host(tr)) == (-1, -1) and untouched()
    tr.close()


def test_out_of_range_without_allocating(oracle, capi, sensors):
    """a handle whose rays x 64 exceed 2^27 -- 128 x 16 400 rays; nothing is committed, no output is given, only the count word"""
    import torch
    from lidarshooter_amd import synth
    s0 = sensors["0000"]
    s = oracle.Sensor(uid="wide", vertical=synth.syn_vertical(128), h_begin=np.float32(0.0), h_end=np.float32(360.0), h_count=16400,
                      R=s0.R, Rinv=s0.Rinv, t=s0.t)
    tr = make_tracer(capi, s)
    n = tr.getTotalRays()
    assert n * 64 > 1 << 27 >= n * 63
    c = torch.full((16,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    host_n = ctypes.c_uint32(7)
    m64, m63 = capi.BeamModel(np.tile(CENTRE, (64, 1)), FIRST, 1, 0.0), capi.BeamModel(np.tile(CENTRE, (63, 1)), FIRST, 1, 0.0)
    w = np.full(64, 9, np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    L = tr.L
    assert L.ls_trace_scene_beams_sweep(tr.h, None, ctypes.byref(m64), w, 0, None, 0, 0, None, None, None, c.data_ptr(), n) == OUT_OF_RANGE
    assert L.ls_trace_scene_beams_sweep_host(tr.h, ctypes.byref(m64), w, 0, None, 0, 0, None, None, None, ctypes.byref(host_n), n) == OUT_OF_RANGE
    assert L.ls_trace_scene_beams_sweep(tr.h, None, ctypes.byref(m64), w, 0, None, 0, 0, None, None, None, c.data_ptr(), n - 1) == INVALID_ARGUMENT
    assert L.ls_debug_beam_sweep_check(ctypes.byref(m64), w, n, n) == OUT_OF_RANGE
    assert L.ls_trace_scene_beams_sweep(tr.h, None, ctypes.byref(m63), w, 0, None, 0, 0, None, None, None, c.data_ptr(), n) == -1   # in range: no commit
    torch.cuda.synchronize()
    assert np.all(c.cpu().numpy() == FILL) and host_n.value == 7
    tr.close()


def test_open_frame_graph_is_refused(oracle, capi, sensors, meshes):
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
    m = capi.BeamModel(CENTRE, FIRST, 1, INF)
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != FRAME_EAGER   # the frame is being captured: the graph is open
    assert L.ls_trace_scene_beams_sweep(tr.h, None, ctypes.byref(m), None, 0, None, 0, 0, None, out.data_ptr() + 16, None, out.data_ptr(), n) == INVALID_ARGUMENT
    assert L.ls_trace_scene_beams_sweep_host(tr.h, ctypes.byref(m), None, 0, None, 0, 0, None, None, None, ctypes.byref(host_n), n) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == FILL) and host_n.value == 7
    # the frame went out, and the handle answers again: one centre sample at rest gives that frame
    k_frame = int(c[0].item())
    assert k_frame > 0
    k, _, hh, _ = _bs(tr, m)
    assert k == k_frame and _same_bits(hh, h.cpu().numpy()[:16 * k].view(np.uint32).reshape(k, 4))
    tr.close()


def test_frames_around_a_call_on_a_caller_stream(oracle, capi, sensors, meshes):
    """LS_OPT_PIPELINE = 2: frames of ls_trace_scene_async, a call on a caller stream between them -- every frame the oracle's
    cloud, the call the same call on the handle's stream"""
    import torch
    s, ml, scene, pose, pat, sub = _xt32(oracle, capi, sensors, meshes)
    ref = oracle.trace_frame(s, ml)
    n = s.V * s.H
    model = capi.BeamModel(pat, 7, 1, 0.05)
    cap = 3 * n
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    _ground_ben(tr, oracle, meshes)
    qs = torch.cuda.Stream()
    d_pose = torch.from_numpy(np.array(pose, np.float32)).to("cuda:0")
    frames = [(torch.zeros(32 * n, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * n, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0")) for _ in range(4)]
    bp, bh, be, bc = (torch.full((32 * cap,), FILL, dtype=torch.uint8, device="cuda:0"), torch.full((16 * cap,), FILL, dtype=torch.uint8, device="cuda:0"),
                      torch.full((4 * cap,), FILL, dtype=torch.uint8, device="cuda:0"), torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    torch.cuda.synchronize()
    for i, (p, h, c) in enumerate(frames):
        tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), n)
        tr.traceSceneAsync(i)
        if i == 1:
            assert tr.traceBeamsSweepDevice(model, bc.data_ptr(), cap, bp.data_ptr(), bh.data_ptr(), be.data_ptr(), weights=WEIGHTS5, min_weight=25000,
                                            d_col_pose=d_pose.data_ptr(), n_cols=s.H, flags=capi.LS_SWEEP_DESKEW, stream=qs.cuda_stream) == 0
            assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 2
    tr.flush()
    tr.synchronize()
    torch.cuda.synchronize()
    for p, h, c in frames:
        k = int(c[0].item())
        assert k == len(ref["points"]) and np.array_equal(p.cpu().numpy()[:32 * k].reshape(k, 32), ref["points"])
    k = int(bc[0].item())
    want = _expect(oracle, s, sub, 5, 7, 1, 0.05, WEIGHTS5, 25000, pose, True)
    got = _bs(tr, model, WEIGHTS5, 25000, pose, capi.LS_SWEEP_DESKEW)      # the handle's stream
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0
    _check(got, want)
    assert k == got[0] and _same_bits(bp.cpu().numpy()[:32 * k].reshape(k, 32), got[1])
    assert _same_bits(bh.cpu().numpy()[:16 * k].view(np.uint32).reshape(k, 4), got[2])
    assert _same_bits(be.cpu().numpy()[:4 * k].view(np.uint32), got[3])
    assert np.all(bp.cpu().numpy()[32 * k:] == FILL) and np.all(be.cpu().numpy()[4 * k:] == FILL)
    # a frame after it, synchronously: still the oracle's cloud
    rc, pts, hits = tr.traceScene(9)
    assert rc == 0 and np.array_equal(np.asarray(pts).reshape(-1, 32), ref["points"])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_host_entry_point_equals_device_entry_point(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    pat, pose = _rings5(capi), _twist_poses(capi, s)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for first, count in ((0, s.H), (37, 51)):
        tr.setShard(first, count)
        for returns, min_count, weights, min_weight, table, flags in ((7, 1, WEIGHTS5, 25000, pose, capi.LS_SWEEP_DESKEW), (2, 2, None, 0, pose, 0),
                                                                      (5, 1, WEIGHTS5, 0, None, 0)):
            model = capi.BeamModel(pat, returns, min_count, 0.05)
            k, p, h, e = _bs(tr, model, weights, min_weight, table, flags)
            assert k > 100
            for want_p, want_h, want_e in ((True, True, True), (False, True, False), (True, False, False), (False, False, True), (False, False, False)):
                rc, kh, ph, hh, eh = tr.traceBeamsSweep(model, weights, min_weight, table, flags, points=want_p, hits=want_h, echo=want_e)
                assert rc == 0 and kh == k
                assert (ph is None) if not want_p else _same_bits(ph, p)
                assert (hh is None) if not want_h else np.array_equal(np.stack([hh["ray"], hh["geom"], hh["prim"], hh["t"].view(np.uint32)], axis=1), h)
                assert (eh is None) if not want_e else np.array_equal(eh, e)
    tr.close()
    t2 = make_tracer(capi, s)
    rc, k, p, h, e = t2.traceBeamsSweep(capi.BeamModel(pat, 7, 1, 0.25), WEIGHTS5, 0, pose)
    assert rc == -1 and k == 0 and len(p) == 0 and len(h) == 0 and len(e) == 0
    t2.close()
