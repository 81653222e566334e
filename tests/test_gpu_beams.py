"""ls_trace_scene_beams / ls_trace_scene_beams_host on the MI355X: frames of diverging beams with multi-echo returns.  The
expectation restates the sub-rays in numpy float32 (test_beams_cpu.restate_beam_rays), runs the oracle's brute force on them over
the oracle's scene and reduces every beam in plain Python (test_beams_cpu.reduce_beam).  One sample against the frame; the full
raster; the seven return masks; other sample counts; range ties; azimuth shards; tiny rasters (the compaction across lane-group,
wave and workgroup boundaries); two launch batches; NULL outputs; return codes; frames around a call; host against device.
Everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest

from conftest import make_tracer
from test_beams_cpu import FIRST, LAST, STRONGEST, INF, reduce_beam, restate_beam_rays
from test_gpu_rays import INV, _add, _from_gid, _ground_ben
from test_gpu_sweep import _eighteen, _holed_grid

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, OUT_OF_RANGE = -2, -9
FRAME_EAGER = 0
FILL = 0xAB
F = np.float32
CENTRE = np.float32([[0.0, 0.0, 1.0]])


# ---- expectations ----------------------------------------------------------------------------------------------------------

def _subhits(oracle, s, scene, pat):
    """the sub-rays of the full raster (index (v * H + h) * S + s) through the oracle's brute force -> (r float32 (V * H, S): the
    reported ranges t * k, hit bool (V * H, S), dense ls_hit records uint32 (V * H * S, 4))"""
    st, ct, sp, cp = oracle.ray_tables(s)
    n, S = s.V * s.H, pat.shape[0]
    vv, hh, ss = np.repeat(np.arange(n) // s.H, S), np.repeat(np.arange(n) % s.H, S), np.tile(np.arange(S), n)
    rays = restate_beam_rays(st[vv], ct[vv], cp[hh], sp[hh], pat[ss, 0], pat[ss, 1])
    t, gid = oracle.trace_bruteforce(np.ascontiguousarray(rays[:, 4:7]), scene)
    r = t * pat[ss, 2]
    assert r.dtype == np.float32
    out = (r.reshape(n, S), (gid != INV).reshape(n, S), _from_gid(scene, t, gid))
    for a in out:
        a.setflags(write=False)
    return out


def _expect(oracle, s, sub, S, returns, min_count, separation, first=0, count=None):
    """-> (hits uint32 (k, 4), points uint8 (k, 32), echo uint32 (k,), records per beam int (rays,)) of the columns [first, first +
    count): ascending global ray index, ascending range inside a beam; xyz = r_e * d, intensity (64 n_e) / S, ring v"""
    r, hit, dense = sub
    count = s.H - first if count is None else count
    st, ct, sp, cp = oracle.ray_tables(s)
    v_of, h_of = np.arange(s.V * s.H) // s.H, np.arange(s.V * s.H) % s.H
    dirs = np.stack([st[v_of] * cp[h_of], st[v_of] * sp[h_of], ct[v_of]], axis=1)      # the nominal d: the frame's factor-table products
    assert dirs.dtype == np.float32
    hits, echo, per_beam = [], [], np.zeros(s.V * s.H, np.int64)
    for q in range(s.V * s.H):
        if not first <= q % s.H < first + count:
            continue
        recs = reduce_beam(r[q], hit[q], returns, min_count, separation)
        per_beam[q] = len(recs)
        for bits, word in recs:
            d = dense[q * S + (word >> 16)]
            hits.append((q, d[1], d[2], bits))
            echo.append(word)
    hits = np.array(hits, np.uint32).reshape(-1, 4)
    echo = np.array(echo, np.uint32)
    k = len(echo)
    p = np.zeros((k, 8), np.uint32)
    ray = hits[:, 0].astype(np.int64)
    p[:, 0:3] = (hits[:, 3].copy().view(np.float32)[:, None] * dirs[ray]).astype(np.float32).view(np.uint32)
    p[:, 4] = ((F(64.0) * ((echo >> 8) & 0x7F).astype(np.float32)) / F(S)).astype(np.float32).view(np.uint32)
    p[:, 5] = ray // s.H
    return hits, p.view(np.uint8).reshape(-1, 32), echo, per_beam


_cache = {}


def _xt32(oracle, sensors, meshes, capi, key, pat):
    """XT-32 0000 over ground + ben and the sub-hits of a pattern: computed once per pattern, shared, never changed"""
    if "scene" not in _cache:
        s = sensors["0000"]
        ml = [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], oracle.IDENTITY_AFFINE)]
        _cache["scene"] = (s, ml, oracle.assemble_scene(s, ml))
    s, ml, scene = _cache["scene"]
    if key not in _cache:
        _cache[key] = _subhits(oracle, s, scene, pat)
    return s, ml, scene, _cache[key]


def _rings5(capi):
    return capi.beam_pattern_rings(0.01, 0.01, 1, 4)


# ---- the device entry point ------------------------------------------------------------------------------------------------

def _beams(tr, model, points=True, hits=True, echo=True, stream=None):
    """ls_trace_scene_beams with capacity exactly K x the shard's ray count and one canary record behind every buffer -> (k, points
    uint8 (k, 32) | None, hits uint32 (k, 4) | None, echo uint32 (k,) | None); whatever lies past record k, the canary included,
    must still hold the fill pattern"""
    import torch
    cap = model.n_returns * tr.getTotalRays()
    p = torch.full(((cap + 1) * 32,), FILL, dtype=torch.uint8, device="cuda:0") if points else None
    h = torch.full(((cap + 1) * 16,), FILL, dtype=torch.uint8, device="cuda:0") if hits else None
    e = torch.full(((cap + 1) * 4,), FILL, dtype=torch.uint8, device="cuda:0") if echo else None
    c = torch.full((16,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = tr.traceBeamsDevice(model, c.data_ptr(), cap, p.data_ptr() if points else 0, h.data_ptr() if hits else 0, e.data_ptr() if echo else 0,
                             stream=stream)
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


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check(got, want):
    k, p, h, e = got
    wh, wp, we, _ = want
    assert k == len(we)
    assert np.array_equal(h, wh)
    assert np.array_equal(e, we)
    assert _same_bits(p, wp)


# ---- 1. one centre sample reproduces the frame -----------------------------------------------------------------------------

@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_one_sample_reproduces_the_frame(oracle, capi, sensors, meshes, engine):
    """S = 1, the sample (0, 0, 1), FIRST, min_count 1: points32, hits and count of ls_trace_scene on both engines of the frame side
    -- the reference's 1668 points over the ground, 1781 over ground + ben; every echo word FIRST with one member of sample 0"""
    s = sensors["0000"]
    for with_ben, known in ((False, 1668), (True, 1781)):
        tr = make_tracer(capi, s, engine)
        if with_ben:
            _ground_ben(tr, oracle, meshes)
        else:
            _add(tr, "ground", *meshes["ground"])
            tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
            assert tr.commitScene() == 0
        rc, pts, hits = tr.traceScene(0)
        assert rc == 0 and len(pts) == known
        for separation in (INF, 0.0):
            k, p, h, e = _beams(tr, capi.BeamModel(CENTRE, FIRST, 1, separation))
            assert k == known
            assert _same_bits(p, np.asarray(pts).reshape(-1, 32))
            assert np.array_equal(h, np.stack([hits["ray"], hits["geom"], hits["prim"], hits["t"].view(np.uint32)], axis=1))
            assert np.all(e == (1 | 1 << 8))
        tr.close()


# ---- 2. the full raster against the expectation ----------------------------------------------------------------------------

def test_full_raster_equals_the_expectation(oracle, capi, sensors, meshes):
    """S = 5 (no power of two), half-angle 0.01 rad, separation 0.25 m, all three returns"""
    pat = _rings5(capi)
    s, ml, scene, sub = _xt32(oracle, sensors, meshes, capi, "rings5", pat)
    r, hit, dense = sub
    # the expectation itself first: the centre sample is the frame, and the echo structure is rich
    ref = oracle.trace_frame(s, ml)
    centre = dense[0::5]
    assert np.array_equal(centre[:, 1] != INV, ref["gid"] != INV) and np.count_nonzero(centre[:, 1] != INV) == 1781
    assert np.array_equal(centre[centre[:, 1] != INV][:, 3], ref["t"][ref["gid"] != INV].view(np.uint32))
    echoes = np.zeros(s.V * s.H, np.int64)
    for q in range(s.V * s.H):
        rs = np.sort(r[q][hit[q]])
        echoes[q] = 0 if len(rs) == 0 else 1 + np.count_nonzero((rs[1:] - rs[:-1]) > F(0.25))
    assert [int(np.count_nonzero(echoes == i)) for i in range(5)] == [2948, 251, 137, 1458, 6]
    partial = (hit.sum(1) > 0) & (hit.sum(1) < 5)
    assert np.count_nonzero(partial) == 179
    want = _expect(oracle, s, sub, 5, 7, 1, 0.25)
    wh, wp, we, per_beam = want
    assert np.all(per_beam <= np.minimum(echoes, 3)) and np.array_equal(per_beam == 0, echoes == 0)   # (min_count 1: every echo is detectable)
    assert np.count_nonzero(per_beam == 3) > 1000 and np.count_nonzero(per_beam == 2) > 100                # beams emitting 3 and 2 records
    assert np.count_nonzero(we & 7 == 7) > 100                      # the three selections in one record
    assert set(wh[:, 1]) == {0, 1} and len(set((we >> 16) & 0x3F)) == 5
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    _check(_beams(tr, capi.BeamModel(pat, 7, 1, 0.25)), want)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 2 and tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 3. the seven return masks, capacity exactly K x rays ------------------------------------------------------------------

def test_every_return_mask(oracle, capi, sensors, meshes):
    pat = _rings5(capi)
    s, ml, scene, sub = _xt32(oracle, sensors, meshes, capi, "rings5", pat)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    counts = {}
    for returns in range(1, 8):
        want = _expect(oracle, s, sub, 5, returns, 1, 0.25)
        got = _beams(tr, capi.BeamModel(pat, returns, 1, 0.25))      # (_beams: capacity is exactly K x rays, the canary behind it)
        _check(got, want)
        e = got[3]
        assert np.all(e & (7 ^ returns) == 0) and np.all(e & 7 != 0)
        for bit in (FIRST, LAST, STRONGEST):                          # one record of every asked kind per beam with a detectable echo
            assert np.count_nonzero(e & bit) == (1852 if returns & bit else 0)
        counts[returns] = got[0]
    assert counts[1] == counts[2] == counts[4] == 1852 and counts[3] > counts[1] and counts[7] > counts[3] and counts[7] > counts[5]
    tr.close()


# ---- 4. other sample counts ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rings,per_ring", [(1, 7), (3, 5)])
def test_other_sample_counts_over_the_full_raster(oracle, capi, sensors, meshes, n_rings, per_ring):
    """S = 8 and 16, separation 0.05 m and +inf, min_count 2"""
    pat = capi.beam_pattern_rings(0.012, 0.008, n_rings, per_ring)
    S = pat.shape[0]
    s, ml, scene, sub = _xt32(oracle, sensors, meshes, capi, f"rings{S}", pat)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for separation in (0.05, INF):
        want = _expect(oracle, s, sub, S, 7, 2, separation)
        assert len(want[2]) > 1500 and np.all((want[2] >> 8) & 0x7F >= 2)
        if separation == INF:
            assert np.all(want[2] & 7 == 7) and np.max(want[3]) == 1
        else:
            assert np.max(want[3]) == 3
        _check(_beams(tr, capi.BeamModel(pat, 7, 2, separation)), want)
    tr.close()


def test_sixty_four_samples_on_a_shard(oracle, capi, sensors, meshes):
    pat = capi.beam_pattern_rings(0.01, 0.01, 7, 9)
    assert pat.shape[0] == 64
    s = sensors["0000"]
    ml = [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], oracle.IDENTITY_AFFINE)]
    scene = oracle.assemble_scene(s, ml)
    # (the sub-hits of the shard's columns only: the other beams stay all-miss in this expectation and are not asked for)
    st, ct, sp, cp = oracle.ray_tables(s)
    n, S, first, count = s.V * s.H, 64, 0, 16
    q = np.array([v * s.H + h for v in range(s.V) for h in range(first, first + count)])
    vv, hh, ss = np.repeat(q // s.H, S), np.repeat(q % s.H, S), np.tile(np.arange(S), len(q))
    rays = restate_beam_rays(st[vv], ct[vv], cp[hh], sp[hh], pat[ss, 0], pat[ss, 1])
    t, gid = oracle.trace_bruteforce(np.ascontiguousarray(rays[:, 4:7]), scene)
    r, hit, dense = np.zeros((n, S), np.float32), np.zeros((n, S), bool), np.zeros((n * S, 4), np.uint32)
    r[q], hit[q] = (t * pat[ss, 2]).reshape(-1, S), (gid != INV).reshape(-1, S)
    dense.reshape(n, S, 4)[q] = _from_gid(scene, t, gid).reshape(-1, S, 4)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    tr.setShard(first, count)
    for returns, min_count, separation in ((7, 1, 0.1), (5, 8, 0.02), (2, 64, INF)):
        want = _expect(oracle, s, (r, hit, dense), S, returns, min_count, separation, first, count)
        assert len(want[2]) > 100 and np.max((want[2] >> 16) & 0x3F) > 32
        if returns == 7:
            assert np.max(want[3]) == 3
        _check(_beams(tr, capi.BeamModel(pat, returns, min_count, separation)), want)
    tr.close()


# ---- 5. range ties: the lower sample index leads ---------------------------------------------------------------------------

def test_duplicated_samples_tie_and_the_lower_index_wins(oracle, capi, sensors, meshes):
    base = _rings5(capi)
    pat = np.ascontiguousarray(base[[1, 0, 1, 2, 0, 3, 2, 4, 4, 3, 0]])          # every sample at least twice
    lowest = {1: 0, 0: 1, 2: 3, 3: 5, 4: 7}                                        # base sample -> its first index in pat
    s, ml, scene, sub = _xt32(oracle, sensors, meshes, capi, "dup11", pat)
    r, hit, dense = sub
    assert np.array_equal(r[:, 0], r[:, 2]) and np.array_equal(r[:, 1], r[:, 10]) and np.array_equal(hit[:, 7], hit[:, 8])
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for separation in (0.0, 0.25):
        want = _expect(oracle, s, sub, 11, 7, 1, separation)
        got = _beams(tr, capi.BeamModel(pat, 7, 1, separation))
        _check(got, want)
        e = got[3]
        assert set((e >> 16) & 0x3F) <= set(lowest.values())                       # never the later copy of a sample
        assert np.all((e >> 8) & 0x7F >= 2)                                        # a tie is never split, even at separation 0
    tr.close()


# ---- 6. azimuth shards -----------------------------------------------------------------------------------------------------

def test_shards_are_the_full_turn_restricted(oracle, capi, sensors, meshes):
    pat = _rings5(capi)
    s, ml, scene, sub = _xt32(oracle, sensors, meshes, capi, "rings5", pat)
    model = capi.BeamModel(pat, 7, 1, 0.25)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    kf, pf, hf, ef = _beams(tr, model)
    col = hf[:, 0] % s.H
    pieces = []
    for first, count in ((0, 64), (64, 86), (37, 50)):
        tr.setShard(first, count)
        assert tr.getTotalRays() == s.V * count
        got = _beams(tr, model)
        _check(got, _expect(oracle, s, sub, 5, 7, 1, 0.25, first, count))
        inside = (col >= first) & (col < first + count)
        assert got[0] == np.count_nonzero(inside) > 100
        assert np.array_equal(got[2], hf[inside]) and np.array_equal(got[3], ef[inside]) and _same_bits(got[1], pf[inside])   # global ray indices
        pieces.append(got)
    assert pieces[0][0] + pieces[1][0] == kf
    both = np.concatenate([pieces[0][2], pieces[1][2]])
    assert np.array_equal(both[np.argsort(both[:, 0], kind="stable")], hf)
    tr.close()


# ---- 7. tiny rasters: the compaction across lane-group, wave and workgroup boundaries --------------------------------------

@pytest.mark.parametrize("V,H", [(1, 1), (3, 70), (5, 257)])
def test_tiny_rasters(oracle, capi, sensors, V, H):
    s0 = sensors["0000"]
    vertical = np.linspace(-3.0, -28.0, V).astype(np.float32) if V > 1 else np.float32([-12.0])
    from lidarshooter_amd import synth
    # The library (like the reference) takes no sensor of fewer than two columns -- its azimuth step is (end - begin) / (H - 1) --, so
    # the raster of ONE ray is a one-channel, two-column sensor whose handle is put on the shard of its first column.
    cols = max(H, 2)
    s = oracle.Sensor(uid="tiny", vertical=vertical, h_begin=np.float32(0.0 if H > 1 else 30.0), h_end=np.float32(360.0 if H > 1 else 40.0),
                      h_count=cols, R=s0.R, Rinv=s0.Rinv, t=s0.t)
    mesh = _holed_grid() if H > 1 else synth.grid_mesh(48, 40)      # (the single ray must not look through a hole)
    scene = oracle.assemble_scene(s, [(0, *mesh, oracle.IDENTITY_AFFINE)])
    tr = make_tracer(capi, s)
    _add(tr, "mesh", *mesh)
    tr.updateGeometry("mesh", oracle.IDENTITY_AFFINE, *mesh)
    assert tr.commitScene() == 0
    tr.setShard(0, H)
    assert tr.getTotalRays() == V * H
    seen = set()
    for pat in (CENTRE, capi.beam_pattern_rings(0.02, 0.02, 1, 2), capi.beam_pattern_rings(0.03, 0.02, 1, 5), capi.beam_pattern_rings(0.03, 0.03, 2, 6)):
        S = pat.shape[0]
        sub = _subhits(oracle, s, scene, pat)
        for returns, min_count, separation in ((7, 1, 0.02), (3, min(2, S), 0.5)):
            want = _expect(oracle, s, sub, S, returns, min_count, separation, 0, H)
            _check(_beams(tr, capi.BeamModel(pat, returns, min_count, separation)), want)
            seen |= set(want[3][np.arange(V * cols) % cols < H])
    assert seen == ({0, 1, 2, 3} if V * H > 1 else {1, 2, 3})       # lanes with 0, 1, 2 and 3 records
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 8. eighteen geometries: two launch batches of the walk ----------------------------------------------------------------

def test_eighteen_geometries_two_batches(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    geoms = _eighteen(oracle, capi, s, meshes)
    scene = oracle.assemble_scene(s, [(i, v, e, A) for i, (name, v, e, A, gt) in enumerate(geoms)])
    pat = capi.beam_pattern_rings(0.01, 0.01, 1, 2)
    sub = _subhits(oracle, s, scene, pat)
    seen = set(sub[2][:, 1]) - {INV}
    assert {0, 16, 17} <= seen and len(seen) >= 12     # both batches, the quad mesh among them
    tr = make_tracer(capi, s)
    for name, v, e, A, gt in geoms:
        _add(tr, name, v, e, gt)
        tr.updateGeometry(name, A, v, e)
    assert tr.commitScene() == 0
    want = _expect(oracle, s, sub, 3, 7, 1, 0.25)
    assert {0, 16, 17} <= set(want[0][:, 1])
    _check(_beams(tr, capi.BeamModel(pat, 7, 1, 0.25)), want)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 18
    tr.close()


# ---- 9. each output NULL in turn -------------------------------------------------------------------------------------------

def test_each_output_null_in_turn(oracle, capi, sensors, meshes):
    pat = _rings5(capi)
    s, ml, scene, sub = _xt32(oracle, sensors, meshes, capi, "rings5", pat)
    want = _expect(oracle, s, sub, 5, 6, 1, 0.25)
    model = capi.BeamModel(pat, 6, 1, 0.25)
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for points, hits, echo in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        k, p, h, e = _beams(tr, model, points=points, hits=hits, echo=echo)
        assert k == len(want[2])
        assert (p is None) if not points else _same_bits(p, want[1])
        assert (h is None) if not hits else np.array_equal(h, want[0])
        assert (e is None) if not echo else np.array_equal(e, want[2])
    tr.close()


# ---- 10. return codes ------------------------------------------------------------------------------------------------------

def test_return_codes(oracle, capi, sensors, meshes):
    import torch
    pat = _rings5(capi)
    s, ml, scene, sub = _xt32(oracle, sensors, meshes, capi, "rings5", pat)
    n = s.V * s.H
    cap = 3 * n
    bufs = {k: torch.full((size,), FILL, dtype=torch.uint8, device="cuda:0") for k, size in
            (("p", cap * 32 + 64), ("h", cap * 16 + 64), ("e", cap * 4 + 64), ("c", 64))}
    torch.cuda.synchronize()
    P, H_, E, C_ = (bufs[k].data_ptr() for k in "phec")
    host_n = ctypes.c_uint32(0xABABABAB)
    host_p, host_h, host_e = np.full((cap, 32), FILL, np.uint8), np.full((cap, 16), FILL, np.uint8), np.full((cap, 4), FILL, np.uint8)
    good = capi.BeamModel(pat, 7, 1, 0.25)

    def untouched():
        torch.cuda.synchronize()
        return all(np.all(b.cpu().numpy() == FILL) for b in bufs.values()) and host_n.value == 0xABABABAB and \
            np.all(host_p == FILL) and np.all(host_h == FILL) and np.all(host_e == FILL)

    def dev(tr, m=good, p=P, h=H_, e=E, c=C_, capacity=cap):
        return tr.L.ls_trace_scene_beams(tr.h, None, ctypes.byref(m) if m is not None else None, p, h, e, c, capacity)

    def host(tr, m=good, c=True, capacity=cap):
        return tr.L.ls_trace_scene_beams_host(tr.h, ctypes.byref(m) if m is not None else None, host_p.ctypes.data, host_h.ctypes.data,
                                              host_e.ctypes.data, ctypes.byref(host_n) if c else None, capacity)

    tr = make_tracer(capi, s)
    assert (dev(tr), host(tr)) == (-1, -1) and untouched()                       # before a commit
    _add(tr, "ground", *meshes["ground"])
    _add(tr, "face", *meshes["ben"])
    assert (dev(tr), host(tr)) == (-1, -1) and untouched()                       # geometries without a commit
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
    tr.updateGeometry("face", oracle.IDENTITY_AFFINE, *meshes["ben"])
    assert tr.commitScene() == 0

    def model(**kw):
        m = capi.BeamModel(kw.pop("pattern", pat), 7, 1, 0.25)
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
    refused = [dev(tr, m) for m in bad_models] + [host(tr, m) for m in bad_models]
    refused += [dev(tr, c=None), host(tr, c=False),                                  # a NULL count
                dev(tr, capacity=cap - 1), host(tr, capacity=cap - 1),              # a small capacity (K = 3)
                dev(tr, model(returns=3), capacity=2 * n - 1),
                dev(tr, p=P + 8), dev(tr, h=H_ + 8), dev(tr, e=E + 2), dev(tr, c=C_ + 2), dev(tr, p=P + 4, h=None, e=None)]   # misaligned
    assert refused == [INVALID_ARGUMENT] * len(refused) and untouched()
    assert tr.last_error()
    assert dev(tr, model(returns=3), capacity=2 * n) == 0                           # (K = 2: twice the rays are enough)
    tr.synchronize()
    bufs["p"].fill_(FILL), bufs["h"].fill_(FILL), bufs["e"].fill_(FILL), bufs["c"].fill_(FILL)
    torch.cuda.synchronize()
    # a shard: the capacity that counts is the shard's
    tr.setShard(10, 20)
    assert dev(tr, capacity=3 * s.V * 20 - 1) == INVALID_ARGUMENT and untouched()
    tr.setShard(0, s.H)
    # the handle still answers
    want = _expect(oracle, s, sub, 5, 7, 1, 0.25)
    _check(_beams(tr, good), want)
    # A removal commits the remaining scene itself (ls_remove_geometry), as for the sweep: the call follows the remaining scene, and
    # an emptied scene gives -1
    assert tr.removeGeometry("face") >= 0
    k2, p2, h2, e2 = _beams(tr, good)
    assert k2 > 0 and np.all(h2[:, 1] == 0) and np.any(want[0][:, 1] == 1)     # (the ground behind the face shows now)
    assert tr.removeGeometry("ground") >= 0
    assert (dev(tr), host(tr)) == (-1, -1) and untouched()                       # an empty scene
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
    L = tr.L
    assert L.ls_trace_scene_beams(tr.h, None, ctypes.byref(m64), None, None, None, c.data_ptr(), n) == OUT_OF_RANGE
    assert L.ls_trace_scene_beams_host(tr.h, ctypes.byref(m64), None, None, None, ctypes.byref(host_n), n) == OUT_OF_RANGE
    assert L.ls_trace_scene_beams(tr.h, None, ctypes.byref(m64), None, None, None, c.data_ptr(), n - 1) == INVALID_ARGUMENT
    assert L.ls_debug_beam_model_check(ctypes.byref(m64), n, n) == OUT_OF_RANGE
    assert L.ls_trace_scene_beams(tr.h, None, ctypes.byref(m63), None, None, None, c.data_ptr(), n) == -1       # in range: no commit
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
    assert L.ls_trace_scene_beams(tr.h, None, ctypes.byref(m), None, out.data_ptr() + 16, None, out.data_ptr(), n) == INVALID_ARGUMENT
    assert L.ls_trace_scene_beams_host(tr.h, ctypes.byref(m), None, None, None, ctypes.byref(host_n), n) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == FILL) and host_n.value == 7
    # the frame went out, and the handle traces beams again: one centre sample gives that frame
    k_frame = int(c[0].item())
    assert k_frame > 0
    k, _, hh, _ = _beams(tr, m)
    assert k == k_frame and _same_bits(hh, h.cpu().numpy()[:16 * k].view(np.uint32).reshape(k, 4))
    tr.close()


# ---- 11. frames are unaffected ---------------------------------------------------------------------------------------------

def test_frames_around_a_beam_call_on_a_caller_stream(oracle, capi, sensors, meshes):
    """LS_OPT_PIPELINE = 2: frames, a beam call on a caller stream between them -- every frame the oracle's cloud, the beam call the
    same call on the handle's stream; LS_INFO_RAY_QUERY_BUILT counts the first call's hierarchies and then nothing"""
    import torch
    pat = _rings5(capi)
    s, ml, scene, sub = _xt32(oracle, sensors, meshes, capi, "rings5", pat)
    ref = oracle.trace_frame(s, ml)
    n = s.V * s.H
    model = capi.BeamModel(pat, 7, 1, 0.25)
    cap = 3 * n
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    _ground_ben(tr, oracle, meshes)
    qs = torch.cuda.Stream()
    frames = [(torch.zeros(32 * n, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * n, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0")) for _ in range(4)]
    bp, bh, be, bc = (torch.full((32 * cap,), FILL, dtype=torch.uint8, device="cuda:0"), torch.full((16 * cap,), FILL, dtype=torch.uint8, device="cuda:0"),
                      torch.full((4 * cap,), FILL, dtype=torch.uint8, device="cuda:0"), torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    torch.cuda.synchronize()
    for i, (p, h, c) in enumerate(frames):
        tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), n)
        tr.traceSceneAsync(i)
        if i == 1:
            assert tr.traceBeamsDevice(model, bc.data_ptr(), cap, bp.data_ptr(), bh.data_ptr(), be.data_ptr(), stream=qs.cuda_stream) == 0
            assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 2
    tr.flush()
    tr.synchronize()
    torch.cuda.synchronize()
    for p, h, c in frames:
        k = int(c[0].item())
        assert k == len(ref["points"]) and np.array_equal(p.cpu().numpy()[:32 * k].reshape(k, 32), ref["points"])
    k = int(bc[0].item())
    want = _expect(oracle, s, sub, 5, 7, 1, 0.25)
    got = _beams(tr, model)                                         # the handle's stream
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


# ---- 12. the host entry point equals the device entry point ----------------------------------------------------------------

def test_host_entry_point_equals_device_entry_point(oracle, capi, sensors, meshes):
    pat = _rings5(capi)
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    for first, count in ((0, s.H), (37, 50)):
        tr.setShard(first, count)
        for returns, min_count, separation in ((7, 1, 0.25), (2, 2, 0.05)):
            model = capi.BeamModel(pat, returns, min_count, separation)
            k, p, h, e = _beams(tr, model)
            assert k > 100
            for want_p, want_h, want_e in ((True, True, True), (False, True, False), (True, False, False), (False, False, True), (False, False, False)):
                rc, kh, ph, hh, eh = tr.traceBeamsHost(model, points=want_p, hits=want_h, echo=want_e)
                assert rc == 0 and kh == k
                assert (ph is None) if not want_p else _same_bits(ph, p)
                assert (hh is None) if not want_h else np.array_equal(np.stack([hh["ray"], hh["geom"], hh["prim"], hh["t"].view(np.uint32)], axis=1), h)
                assert (eh is None) if not want_e else np.array_equal(eh, e)
    tr.close()
    t2 = make_tracer(capi, s)
    rc, k, p, h, e = t2.traceBeamsHost(capi.BeamModel(pat, 7, 1, 0.25))
    assert rc == -1 and k == 0 and len(p) == 0 and len(h) == 0 and len(e) == 0
    t2.close()
