"""ls_format_cloud / ls_format_cloud_host on the MI355X: clouds in a driver's own PointCloud2 record.  The reference's own layout
against the frame; Velodyne's 22-byte XYZIRT over a sweep frame; an Ouster-like organized image, on the full turn and on a shard;
tile boundaries, ranks and layers, foreign rays on synthetic records without any scene; return codes; host against device; frames
around a call.  Everything is compared byte for byte, NaNs included, against the numpy restatement of tests/test_format_cpu.py.
Output buffers are pre-filled with a pattern and one record longer than needed: whatever lies past the last byte due keeps it."""
import ctypes

import numpy as np
import pytest

from conftest import make_tracer
from test_format_cpu import NAN32, NAN64, _golden_message, restate_cloud, restate_organized
from test_gpu_rays import _ground_ben, _records
from test_gpu_sweep import _sweep, _twist_poses

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, OUT_OF_RANGE = -2, -9
FILL = 0xAB
F = np.float32
TURN = 0.1                                     # seconds per turn of the sensor (test_gpu_sweep's twist)


# ---- formats ---------------------------------------------------------------------------------------------------------------

def _velodyne(capi):
    """XYZIRT, 22 bytes: the float `time` at byte 18"""
    return capi.CloudFormat(22, [(capi.LS_FIELD_X, 7, 0), (capi.LS_FIELD_Y, 7, 4), (capi.LS_FIELD_Z, 7, 8), (capi.LS_FIELD_INTENSITY, 7, 12),
                                 (capi.LS_FIELD_RING, 4, 16), (capi.LS_FIELD_TIME, 7, 18)])


def _ouster(capi, organized=True, layer=0, echo=False):
    """48 bytes with gaps at 12, 25 and 36: xyz, intensity, t in ns, ring u8, label u16, range in mm, ray, a float64 range"""
    fields = [(capi.LS_FIELD_X, 7, 0), (capi.LS_FIELD_Y, 7, 4), (capi.LS_FIELD_Z, 7, 8), (capi.LS_FIELD_INTENSITY, 7, 16),
              (capi.LS_FIELD_TIME, 6, 20, 1e9, 0.0), (capi.LS_FIELD_RING, 2, 24), (capi.LS_FIELD_GEOM, 4, 26),
              (capi.LS_FIELD_RANGE, 6, 28, 1000.0, 0.0), (capi.LS_FIELD_RAY, 6, 32), (capi.LS_FIELD_RANGE, 8, 40)]
    if echo:
        fields.append((capi.LS_FIELD_ECHO, 6, 36))
    return capi.CloudFormat(48, fields, organized=organized, layer=layer)


def _reference(capi):
    msg = _golden_message()
    return capi.cloud_format_from_point_fields(msg["pointFields"], msg["pointStep"])


def _step_format(capi, step, organized=False):
    """one format per record size of the tile test"""
    c = capi
    if step == 1:
        fields = [(c.LS_FIELD_RING, 1, 0)]
    elif step == 5:
        fields = [(c.LS_FIELD_RING, 2, 0), (c.LS_FIELD_X, 7, 1)]                  # an unaligned float behind one byte
    elif step == 22:
        return c.CloudFormat(22, [(f.source, f.datatype, f.offset) for f in list(_velodyne(c).fields)[:6]], organized=organized)
    elif step == 32:
        return c.CloudFormat(32, [(f.source, f.datatype, f.offset) for f in list(_reference(c).fields)[:5]], organized=organized)
    elif step == 48:
        return _ouster(c, organized=organized)
    else:
        fields = [(c.LS_FIELD_X, 8, 0), (c.LS_FIELD_Y, 7, 9), (c.LS_FIELD_Z, 3, 14, 100.0, 0.0), (c.LS_FIELD_RANGE, 8, 17, 0.5, 1.0),
                  (c.LS_FIELD_TIME, 7, 30), (c.LS_FIELD_GEOM, 8, 40), (c.LS_FIELD_PRIM, 5, 63), (c.LS_FIELD_COLUMN, 4, 67),
                  (c.LS_FIELD_INTENSITY, 1, 70, 1.0, -64.0), (c.LS_FIELD_ECHO, 6, 100), (c.LS_FIELD_RAY, 6, 124)]
    return c.CloudFormat(step, fields, organized=organized)


# ---- the device entry point ------------------------------------------------------------------------------------------------

def _to_device(a):
    import torch
    if a is None:
        return None
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(b.copy()).to("cuda:0") if b.size else torch.zeros(16, dtype=torch.uint8, device="cuda:0")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _format(tr, fmt, hits, points=None, echo=None, col_time=None, chan_time=None, count=None, stream=None):
    """ls_format_cloud over host arrays put on the device: `count` None, or the value of a device count word (the arrays are the
    capacity) -> uint8 (records, point_step); everything behind them, a canary record included, must keep the fill pattern"""
    import torch
    hits = np.ascontiguousarray(hits, np.uint32).reshape(-1, 4)
    n = hits.shape[0]
    d = [_to_device(a) for a in (hits, points, echo, col_time, chan_time)]
    d_count = None if count is None else torch.from_numpy(np.array([count, 0, 0, 0], np.uint32).view(np.int32)).to("cuda:0")
    step = fmt.point_step
    cap = tr.V * tr.H if fmt.organized else n
    records = cap if fmt.organized else (n if count is None else min(n, count))
    out = torch.full(((cap + 1) * step + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = tr.formatCloudDevice(fmt, _ptr(d[0]) if n else 0, n, out.data_ptr(), d_points32=_ptr(d[1]) if n else 0, d_echo=_ptr(d[2]) if n else 0,
                              d_count=_ptr(d_count), d_col_time=_ptr(d[3]), d_chan_time=_ptr(d[4]), stream=stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert np.all(a[records * step:] == FILL), "a byte written past the last record due"
    return a[:records * step].reshape(records, step).copy()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _times(capi, s):
    """the columns' firing times of one turn, and a firing offset per channel"""
    return capi.column_times(0.0, TURN / s.H, s.H), (np.arange(s.V, dtype=np.float64) * 1.512e-6 + 3e-7).astype(F)


def _synthetic(rng, n, rays):
    """n records with the given rays: random points (the words no field reads are random too), geom, prim and t"""
    points = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint32)
    points[:, [0, 1, 2, 4]] = (rng.normal(size=(n, 4)) * 40.0).astype(F).view(np.uint32)
    hits = np.stack([np.asarray(rays, np.uint32), rng.integers(0, 70000, n, dtype=np.uint32), rng.integers(0, 2 ** 31, n, dtype=np.uint32),
                     rng.uniform(0.3, 200.0, n).astype(F).view(np.uint32)], axis=1).astype(np.uint32)
    echo = rng.integers(0, 2 ** 22, n, dtype=np.uint32)
    return points.view(np.uint8).reshape(n, 32), np.ascontiguousarray(hits), echo


# ---- 1. the reference's own layout reproduces the frame ------------------------------------------------------------------------

@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_reference_layout_reproduces_the_frame(oracle, capi, sensors, meshes, engine):
    """the format the golden config declares (ring as UINT16 over the int32 the frame writes), the records of ls_trace_scene_async
    with its device count word and n = the capacity, on a caller's stream with no host wait in between: points32 byte for byte.  The
    reference's 1668 points over the ground, 1781 over ground + ben."""
    import torch
    s = sensors["0000"]
    fmt = _reference(capi)
    assert fmt.point_step == 32
    n = s.V * s.H
    for with_ben, known in ((False, 1668), (True, 1781)):
        tr = make_tracer(capi, s, engine)
        if with_ben:
            _ground_ben(tr, oracle, meshes)
        else:
            tr.addGeometry("ground", meshes["ground"][0].shape[0], meshes["ground"][1].shape[0])
            tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
            assert tr.commitScene() == 0
        rc, pts, _ = tr.traceScene(0)
        assert rc == 0 and len(pts) == known
        p, h, c = (torch.zeros(32 * n, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * n, dtype=torch.uint8, device="cuda:0"),
                   torch.zeros(4, dtype=torch.int32, device="cuda:0"))
        out = torch.full(((n + 1) * 32,), FILL, dtype=torch.uint8, device="cuda:0")
        qs = torch.cuda.Stream()
        torch.cuda.synchronize()
        tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), n)
        tr.traceSceneAsync(0)
        assert tr.formatCloudDevice(fmt, h.data_ptr(), n, out.data_ptr(), d_points32=p.data_ptr(), d_count=c.data_ptr(), stream=qs.cuda_stream) == 0
        tr.synchronize()
        torch.cuda.synchronize()
        a = out.cpu().numpy()
        assert int(c[0].item()) == known
        assert np.array_equal(a[:known * 32].reshape(known, 32), np.asarray(pts).reshape(known, 32))
        assert np.all(a[known * 32:] == FILL)
        assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
        tr.close()


# ---- 2. Velodyne XYZIRT over a sweep frame -------------------------------------------------------------------------------------

def _sweep_records(oracle, capi, sensors, meshes):
    """the records of ls_trace_scene_sweep under test_gpu_sweep's twist over ground + ben -> (tracer, sensor, points, hits)"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    k, p, h, _ = _sweep(tr, _twist_poses(capi, s))
    assert k > 1000
    return tr, s, p, h


def test_velodyne_xyzirt_over_a_sweep_frame(oracle, capi, sensors, meshes):
    tr, s, p, h = _sweep_records(oracle, capi, sensors, meshes)
    k = h.shape[0]
    col_time, chan_time = _times(capi, s)
    fmt = _velodyne(capi)
    got = _format(tr, fmt, h, points=p, col_time=col_time, chan_time=chan_time)
    assert _same(got, restate_cloud(fmt, p, h, None, col_time, chan_time, s.V, s.H))
    # what a deskewing consumer reads: the time of every point is its column's plus its channel's
    t = got[:, 18:22].copy().view(F).reshape(-1)
    assert np.array_equal(t, col_time[h[:, 0] % s.H] + chan_time[h[:, 0] // s.H]) and len(set(t.tolist())) > 500
    assert np.array_equal(got[:, 16:18].copy().view(np.uint16).reshape(-1), (h[:, 0] // s.H).astype(np.uint16))
    if (k * 22) % 16 == 0:   # the narrowed tail: a count whose bytes do not end on a 16-byte boundary
        got = _format(tr, fmt, h[:k - 1], points=p[:k - 1], col_time=col_time, chan_time=chan_time)
        assert _same(got, restate_cloud(fmt, p[:k - 1], h[:k - 1], None, col_time, chan_time, s.V, s.H))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 3. Ouster-like, organized, on the full turn and on a shard ----------------------------------------------------------------

def _check_miss_cells(got, miss, s, col_time, chan_time):
    """the miss cells of _ouster's record: NaN, 0, 0xFFFF, and the cell's own ring, ray and time"""
    cells = np.nonzero(miss)[0]
    m = got[miss]
    w = lambda a, b, t: np.ascontiguousarray(m[:, a:b]).view(t).reshape(-1)
    assert np.all(w(0, 4, np.uint32) == NAN32) and np.all(w(4, 8, np.uint32) == NAN32) and np.all(w(8, 12, np.uint32) == NAN32)
    assert np.all(w(16, 20, np.uint32) == NAN32) and np.all(w(40, 48, np.uint64) == NAN64)
    assert np.all(w(28, 32, np.uint32) == 0) and np.all(w(26, 28, np.uint16) == 0xFFFF)
    assert np.array_equal(m[:, 24], (cells // s.H).astype(np.uint8)) and np.array_equal(w(32, 36, np.uint32), cells.astype(np.uint32))
    tau = (col_time[cells % s.H] + chan_time[cells // s.H]).astype(F)
    assert np.array_equal(w(20, 24, np.uint32), np.rint((tau * F(1e9)).astype(F)).astype(np.uint32))
    assert np.all(m[:, 12:16] == 0) and np.all(m[:, 25] == 0) and np.all(m[:, 36:40] == 0)


def test_ouster_like_organized_image_and_a_shard(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    col_time, chan_time = _times(capi, s)
    fmt = _ouster(capi)
    for first, count in ((0, s.H), (37, 61)):
        tr.setShard(first, count)
        rc, pts, hits = tr.traceScene(0)
        assert rc == 0 and len(pts) > 300
        p, h = np.asarray(pts).reshape(-1, 32), _records(hits)
        got = _format(tr, fmt, h, points=p, col_time=col_time, chan_time=chan_time)
        want, miss = restate_organized(fmt, p, h, None, col_time, chan_time, s.V, s.H)
        assert got.shape == (s.V * s.H, 48) and _same(got, want)
        assert np.count_nonzero(~miss) == len(pts)
        _check_miss_cells(got, miss, s, col_time, chan_time)
        cols = np.arange(s.V * s.H) % s.H
        assert np.all(miss[(cols < first) | (cols >= first + count)])          # the cells of other shards are misses
        # a filled cell holds its record: the label and the range in millimetres
        at = h[:, 0].astype(np.int64)
        assert np.array_equal(np.ascontiguousarray(got[at, 26:28]).view(np.uint16).reshape(-1), h[:, 1].astype(np.uint16))
        assert np.array_equal(np.ascontiguousarray(got[at, 28:32]).view(np.uint32).reshape(-1),
                              np.rint((h[:, 3].view(F) * F(1000.0)).astype(F)).astype(np.uint32))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 4. tile boundaries, without a scene ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", [1, 5, 22, 32, 48, 128])
def test_tile_boundaries_without_a_scene(capi, sensors, step):
    """a handle with no geometry at all; record counts around the 64-lane wave, the 256-record tile (128 records at step 128) and its
    multiples; every second call through a device count word below the capacity"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    col_time, chan_time = _times(capi, s)
    rng = np.random.default_rng(400 + step)
    for j, n in enumerate((0, 1, 63, 64, 255, 256, 257, 511, 513)):
        cap = n + 7 if j % 2 else n
        rays = rng.choice(s.V * s.H, cap, replace=False).astype(np.uint32)       # distinct rays
        p, h, e = _synthetic(rng, cap, rays)
        count = n if j % 2 else None
        for organized in (False, True):
            fmt = _step_format(capi, step, organized)
            assert capi.cloud_format_check(fmt) == 0
            got = _format(tr, fmt, h, points=p, echo=e, col_time=col_time, chan_time=chan_time, count=count)
            if organized:
                want, miss = restate_organized(fmt, p[:n], h[:n], e[:n], col_time, chan_time, s.V, s.H)
                assert np.count_nonzero(~miss) == n
            else:
                want = restate_cloud(fmt, p[:n], h[:n], e[:n], col_time, chan_time, s.V, s.H)
            assert _same(got, want), (step, n, organized)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 5. ranks and layers -------------------------------------------------------------------------------------------------------

def test_ranks_and_layers_on_synthetic_runs(capi, sensors):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    rng = np.random.default_rng(55)
    lengths = np.array([1, 2, 3, 4, 5, 5, 4, 3, 2, 1] * 40)
    run_rays = rng.choice(s.V * s.H, lengths.size, replace=False).astype(np.uint32)
    rays = np.repeat(run_rays, lengths)
    n = rays.size
    p, h, e = _synthetic(rng, n, rays)
    h[:, 1] = np.arange(n, dtype=np.uint32)                                       # geom names the record
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    fields = [(capi.LS_FIELD_GEOM, 6, 0), (capi.LS_FIELD_RAY, 6, 4), (capi.LS_FIELD_X, 7, 8), (capi.LS_FIELD_ECHO, 6, 12)]
    for layer in (0, 1, 2):
        fmt = capi.CloudFormat(16, fields, organized=True, layer=layer)
        got = _format(tr, fmt, h, points=p, echo=e)
        who = np.ascontiguousarray(got[:, 0:4]).view(np.uint32).reshape(-1)
        expect = np.full(s.V * s.H, 0xFFFFFFFF, np.uint32)
        has = lengths > layer                                                     # the fourth and fifth of a run are never used
        expect[run_rays[has]] = (starts[has] + layer).astype(np.uint32)
        assert np.array_equal(who, expect), layer
        want, miss = restate_organized(fmt, p, h, e, None, None, s.V, s.H)
        assert _same(got, want) and np.count_nonzero(~miss) == np.count_nonzero(has)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_layers_of_a_beam_frame_are_its_first_and_second_return(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    model = capi.BeamModel(capi.beam_pattern_rings(0.01, 0.01, 1, 4), capi.LS_BEAM_FIRST | capi.LS_BEAM_LAST, 1, 0.25)
    rc, k, p, hits, e = tr.traceBeamsHost(model)
    assert rc == 0 and k > 1000
    h = _records(hits)
    second = np.count_nonzero(h[1:, 0] == h[:-1, 0])
    assert second > 10                                                            # beams with two echoes
    col_time, chan_time = _times(capi, s)
    filled = []
    for layer in (0, 1):
        fmt = _ouster(capi, layer=layer, echo=True)
        got = _format(tr, fmt, h, points=p, echo=e, col_time=col_time, chan_time=chan_time)
        want, miss = restate_organized(fmt, p, h, e, col_time, chan_time, s.V, s.H)
        assert _same(got, want)
        filled.append(np.count_nonzero(~miss))
    assert filled == [k - second, second]
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 6. foreign rays -----------------------------------------------------------------------------------------------------------

def test_foreign_rays(capi, sensors):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    cells = s.V * s.H
    rng = np.random.default_rng(66)
    n = 700
    rays = rng.choice(cells, n, replace=False).astype(np.uint32)
    foreign = np.zeros(n, bool)
    foreign[rng.choice(n, 90, replace=False)] = True
    foreign[[0, 255, 256, n - 1]] = True
    rays[foreign] = np.resize(np.array([cells, cells + 1, 0xFFFFFFFF], np.uint32), np.count_nonzero(foreign))
    p, h, e = _synthetic(rng, n, rays)
    col_time, chan_time = _times(capi, s)
    c = capi
    fmt = c.CloudFormat(40, [(c.LS_FIELD_X, 7, 0), (c.LS_FIELD_RING, 6, 4), (c.LS_FIELD_COLUMN, 6, 8), (c.LS_FIELD_TIME, 7, 12), (c.LS_FIELD_RAY, 6, 16),
                             (c.LS_FIELD_GEOM, 6, 20), (c.LS_FIELD_PRIM, 6, 24), (c.LS_FIELD_RANGE, 7, 28), (c.LS_FIELD_ECHO, 6, 32),
                             (c.LS_FIELD_TIME, 5, 36, 1e6, 0.0)])
    got = _format(tr, fmt, h, points=p, echo=e, col_time=col_time, chan_time=chan_time)
    assert _same(got, restate_cloud(fmt, p, h, e, col_time, chan_time, s.V, s.H))
    assert np.all(got[foreign, 4:16] == 0) and np.all(got[foreign, 36:40] == 0)                       # ring, column and both times
    assert np.array_equal(np.ascontiguousarray(got[:, 16:28]).view(np.uint32).reshape(n, 3), h[:, 0:3])   # the rest is formatted
    assert np.array_equal(got[:, 0:4], p[:, 0:4]) and np.array_equal(np.ascontiguousarray(got[:, 32:36]).view(np.uint32).reshape(-1), e)
    org = c.CloudFormat(40, [(f.source, f.datatype, f.offset, f.scale, f.bias) for f in list(fmt.fields)[:10]], organized=True)
    got = _format(tr, org, h, points=p, echo=e, col_time=col_time, chan_time=chan_time)
    want, miss = restate_organized(org, p, h, e, col_time, chan_time, s.V, s.H)
    assert _same(got, want) and np.count_nonzero(~miss) == n - np.count_nonzero(foreign)                # they are left out
    assert tr.info(c.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 7. return codes -----------------------------------------------------------------------------------------------------------

def test_return_codes(capi, sensors):
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)                                       # no geometry at all: the call needs no commit
    L, hd = tr.L, tr.h
    n = 300
    rng = np.random.default_rng(77)
    p, h, e = _synthetic(rng, n, rng.choice(s.V * s.H, n, replace=False))
    col_time, chan_time = _times(capi, s)
    d = {k: _to_device(a) for k, a in (("p", p), ("h", h), ("e", e), ("ct", col_time), ("ch", chan_time))}
    d["c"] = torch.from_numpy(np.array([n, 0, 0, 0], np.int32)).to("cuda:0")
    out = torch.full((s.V * s.H * 48 + 64,), FILL, dtype=torch.uint8, device="cuda:0")
    host_out = np.full(s.V * s.H * 48, FILL, np.uint8)
    torch.cuda.synchronize()
    P, H_, E, CT, CH, C_, O = [d[k].data_ptr() for k in ("p", "h", "e", "ct", "ch", "c")] + [out.data_ptr()]
    ok, org = _ouster(capi, organized=False, echo=True), _ouster(capi, echo=True)
    ref = ctypes.byref

    def dev(fmt=ok, points=P, hits=H_, echo=E, count=C_, n_=n, ct=CT, ch=CH, o=O, handle=hd):
        return L.ls_format_cloud(handle, None, None if fmt is None else ref(fmt), points, hits, echo, count, n_, ct, ch, o)

    def host(fmt=ok, points=p.ctypes.data, hits=h.ctypes.data, echo=e.ctypes.data, n_=n, ct=col_time.ctypes.data, ch=chan_time.ctypes.data,
             o=host_out.ctypes.data, handle=hd):
        return L.ls_format_cloud_host(handle, None if fmt is None else ref(fmt), points, hits, echo, n_, ct, ch, o)

    def untouched():
        torch.cuda.synchronize()
        return bool(np.all(out.cpu().numpy() == FILL) and np.all(host_out == FILL))

    bad_step, bad_layer = _ouster(capi, organized=False), _ouster(capi, organized=False)
    bad_step.point_step, bad_layer.layer = 47, 1
    no_points = capi.CloudFormat(8, [(capi.LS_FIELD_RAY, 6, 0), (capi.LS_FIELD_RANGE, 7, 4)])
    refused = {
        "null handle": dev(handle=None), "null handle, host": host(handle=None),
        "null format": dev(fmt=None), "null format, host": host(fmt=None),
        "a field outside the step": dev(fmt=bad_step), "a field outside the step, host": host(fmt=bad_step),
        "a layer without organized": dev(fmt=bad_layer),
        "null hits": dev(hits=None), "null hits, host": host(hits=None),
        "null output": dev(o=None), "null output, host": host(o=None),
        "null output, organized, n = 0": dev(fmt=org, o=None, n_=0), "null output, organized, n = 0, host": host(fmt=org, o=None, n_=0),
        "x named without points": dev(points=None), "x named without points, host": host(points=None),
        "time named without column times": dev(ct=None), "time named without column times, host": host(ct=None),
        "time named without column times, n = 0": dev(fmt=org, ct=None, n_=0),
        "misaligned output": dev(o=O + 8), "misaligned points": dev(points=P + 8), "misaligned hits": dev(hits=H_ + 8),
        "misaligned echo": dev(echo=E + 2), "misaligned count": dev(count=C_ + 2), "misaligned column times": dev(ct=CT + 2),
        "misaligned channel times": dev(ch=CH + 1),
    }
    assert refused == {k: INVALID_ARGUMENT for k in refused} and untouched()
    assert tr.last_error()
    assert dev(n_=0xFFF00001) == OUT_OF_RANGE and host(n_=0xFFF00001) == OUT_OF_RANGE and untouched()
    # what is not refused: n = 0 unorganized writes nothing, NULL points for a format that names none, NULL echo and channel times
    assert dev(n_=0, hits=None, points=None, o=None) == 0 and host(n_=0, hits=None, points=None, o=None) == 0
    tr.synchronize()
    assert untouched()
    assert dev(fmt=no_points, points=None, echo=None, ch=None, ct=None, count=None) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert _same(a[:n * 8].reshape(n, 8), restate_cloud(no_points, None, h, None, None, None, s.V, s.H)) and np.all(a[n * 8:] == FILL)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
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
    out = torch.full((n * 32 + 32,), FILL, dtype=torch.uint8, device="cuda:0")
    host_out = np.full(32 * 4, FILL, np.uint8)
    hp, hh = np.zeros((4, 32), np.uint8), np.zeros((4, 4), np.uint32)
    torch.cuda.synchronize()
    L = tr.L
    fmt = _reference(capi)
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != 0   # the frame is being captured: the graph is open
    assert L.ls_format_cloud(tr.h, None, ctypes.byref(fmt), p.data_ptr(), h.data_ptr(), None, c.data_ptr(), n, None, None, out.data_ptr()) == INVALID_ARGUMENT
    assert L.ls_format_cloud(tr.h, None, None, p.data_ptr(), h.data_ptr(), None, c.data_ptr(), n, None, None, out.data_ptr()) == INVALID_ARGUMENT
    assert "frame graph" in tr.last_error()                          # the graph comes before the NULL format
    assert L.ls_format_cloud_host(tr.h, ctypes.byref(fmt), hp.ctypes.data, hh.ctypes.data, None, 4, None, None, host_out.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == FILL) and np.all(host_out == FILL)
    # the frame went out, and the handle formats again: that frame's cloud
    k = int(c[0].item())
    assert k > 0
    assert tr.formatCloudDevice(fmt, h.data_ptr(), n, out.data_ptr(), d_points32=p.data_ptr(), d_count=c.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert np.array_equal(a[:32 * k], p.cpu().numpy()[:32 * k]) and np.all(a[32 * k:] == FILL)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 8. the host variant equals the device call ----------------------------------------------------------------------------------

def _unaligned(a, shift):
    """a copy of the array's bytes at an address that is `shift` past a 16-byte boundary -> (its address, the keeper)"""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = np.zeros(b.size + 32, np.uint8)
    off = (-buf.ctypes.data) % 16 + shift
    buf[off:off + b.size] = b
    return buf.ctypes.data + off, buf


def test_host_variant_equals_the_device_call(oracle, capi, sensors, meshes):
    tr, s, p, h = _sweep_records(oracle, capi, sensors, meshes)
    col_time, chan_time = _times(capi, s)
    rc, pts, hits = tr.traceScene(0)
    frame_p, frame_h = np.asarray(pts).reshape(-1, 32), _records(hits)
    for fmt, pp, hh in ((_velodyne(capi), p, h), (_ouster(capi), frame_p, frame_h)):
        dev = _format(tr, fmt, hh, points=pp, col_time=col_time, chan_time=chan_time)
        assert _same(tr.formatCloud(fmt, hh, points=pp, col_time=col_time, chan_time=chan_time), dev)
        # pointers that are aligned to nothing, the output included
        keep = [_unaligned(a, sh) for a, sh in ((pp, 1), (hh, 3), (col_time, 1), (chan_time, 2))]
        out = np.full(dev.size + 48, FILL, np.uint8)
        o = (-out.ctypes.data) % 16 + 5
        assert tr.L.ls_format_cloud_host(tr.h, ctypes.byref(fmt), keep[0][0], keep[1][0], None, hh.shape[0], keep[2][0], keep[3][0],
                                         out.ctypes.data + o) == 0
        assert np.array_equal(out[o:o + dev.size], dev.reshape(-1)) and np.all(out[:o] == FILL) and np.all(out[o + dev.size:] == FILL)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 9. frames are unaffected --------------------------------------------------------------------------------------------------

def test_frames_around_a_format_call(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    col_time, chan_time = _times(capi, s)
    rc, pts0, hits0 = tr.traceScene(0)
    assert rc == 0 and len(pts0) == 1781
    p, h = np.asarray(pts0).reshape(-1, 32).copy(), _records(hits0)
    for fmt in (_velodyne(capi), _ouster(capi)):
        _format(tr, fmt, h, points=p, col_time=col_time, chan_time=chan_time)
        rc, pts1, hits1 = tr.traceScene(0)
        assert rc == 0 and np.array_equal(np.asarray(pts1), p.reshape(np.asarray(pts1).shape)) and np.array_equal(_records(hits1), h)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0               # left as it is: nothing was built
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
