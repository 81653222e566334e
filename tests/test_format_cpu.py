"""ls_format_cloud without a GPU: the record's operation sequence on the host (ls_debug_format_record, csrc/ls_cloud_format.h) against
a numpy restatement of the record rules, byte for byte; ls_cloud_format_check; ls_cloud_format_from_point_fields on the golden
sensor config; ls_column_times.  The restatement (restate_cloud, restate_organized) is what tests/test_gpu_format.py compares the
device against as well."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import DATA

F = np.float32
NAN32, NAN64 = 0x7FC00000, 0x7FF8000000000000
INVALID_ARGUMENT, UNSUPPORTED_TYPE = -2, -5
FLOAT_SOURCES = (1, 2, 3, 4, 5, 6)            # X, Y, Z, INTENSITY, RANGE, TIME
WORD_SOURCES = (7, 8, 9, 10, 11, 12)          # RING, COLUMN, RAY, GEOM, PRIM, ECHO
BYTES = {1: 1, 2: 1, 3: 2, 4: 2, 5: 4, 6: 4, 7: 4, 8: 8}
RANGE = {1: (-128, 127), 2: (0, 255), 3: (-32768, 32767), 4: (0, 65535), 5: (-2 ** 31, 2 ** 31 - 1), 6: (0, 2 ** 32 - 1)}


# ---- the restatement -----------------------------------------------------------------------------------------------------------

def restate_sources(points, hits, echo, col_time, chan_time, V, H, miss=None):
    """the twelve sources of n records as uint32 arrays (float sources as their bits), keyed by LS_FIELD_*.  points uint8 (n, 32) or
    None, hits uint32 (n, 4), echo uint32 (n,) or None, col_time float32 (H,) or None, chan_time float32 (V,) or None; miss: a bool
    mask of records that are miss cells of the ray hits[:, 0]"""
    hits = np.ascontiguousarray(hits, np.uint32).reshape(-1, 4)
    n = hits.shape[0]
    ray = hits[:, 0]
    mine = ray.astype(np.int64) < V * H
    safe = np.where(mine, ray, 0).astype(np.int64)
    ring, column = safe // H, safe % H
    ct = np.zeros(H, F) if col_time is None else np.asarray(col_time, F)
    ch = np.zeros(V, F) if chan_time is None else np.asarray(chan_time, F)
    time = np.where(mine, ct[column] + ch[ring], F(0.0)).astype(F)          # one float32 sum
    p = np.zeros((n, 8), np.uint32) if points is None else np.ascontiguousarray(points, np.uint8).reshape(n, 32).view(np.uint32)
    e = np.zeros(n, np.uint32) if echo is None else np.asarray(echo, np.uint32)
    s = {1: p[:, 0].copy(), 2: p[:, 1].copy(), 3: p[:, 2].copy(), 4: p[:, 4].copy(), 5: hits[:, 3].copy(), 6: time.view(np.uint32).copy(),
         7: np.where(mine, ring, 0).astype(np.uint32), 8: np.where(mine, column, 0).astype(np.uint32), 9: ray.copy(),
         10: hits[:, 1].copy(), 11: hits[:, 2].copy(), 12: e.copy()}
    if miss is not None:
        m = np.asarray(miss, bool)
        for k in (1, 2, 3, 4, 5):
            s[k][m] = NAN32
        s[10][m] = s[11][m] = 0xFFFFFFFF
        s[12][m] = 0
    return s


def _field_bytes(source, datatype, scale, bias, v):
    """the bytes one field stores for the source words v: uint8 (n, BYTES[datatype]), little-endian"""
    nb = BYTES[datatype]
    if source in WORD_SOURCES:
        if datatype == 7:
            return v.astype(F).astype("<f4").view(np.uint8).reshape(-1, 4)
        if datatype == 8:
            return v.astype(np.float64).astype("<f8").view(np.uint8).reshape(-1, 8)
        return (v.astype(np.uint64) & np.uint64(2 ** (8 * nb) - 1)).astype(f"<u{nb}").view(np.uint8).reshape(-1, nb)
    plain = F(scale) == F(1.0) and F(bias) == F(0.0)
    if plain and datatype == 7:
        return v.astype("<u4").view(np.uint8).reshape(-1, 4)               # the bits untouched
    f = v.view(F)
    with np.errstate(all="ignore"):
        g = f if plain else ((f * F(scale)).astype(F) + F(bias)).astype(F)  # float32, two roundings
    nan = np.isnan(g)
    if datatype == 7:
        return np.where(nan, np.uint32(NAN32), g.view(np.uint32)).astype("<u4").view(np.uint8).reshape(-1, 4)
    if datatype == 8:
        with np.errstate(all="ignore"):
            wide = g.astype(np.float64).view(np.uint64)
        return np.where(nan, np.uint64(NAN64), wide).astype("<u8").view(np.uint8).reshape(-1, 8)
    lo, hi = RANGE[datatype]
    with np.errstate(all="ignore"):
        r = np.rint(np.where(nan, F(0.0), g)).astype(np.float64)            # ties to even, then the exact widening
    r = np.clip(r, float(lo), float(hi)).astype(np.int64)
    return (r.astype(np.uint64) & np.uint64(2 ** (8 * nb) - 1)).astype(f"<u{nb}").view(np.uint8).reshape(-1, nb)


def restate_format(fmt, sources):
    """the records of the sources under the format: uint8 (n, point_step), every byte no field covers 0"""
    n = sources[9].shape[0]
    out = np.zeros((n, fmt.point_step), np.uint8)
    for k in range(fmt.n_fields):
        fd = fmt.fields[k]
        out[:, fd.offset:fd.offset + BYTES[fd.datatype]] = _field_bytes(fd.source, fd.datatype, fd.scale, fd.bias, sources[fd.source])
    return out


def restate_cloud(fmt, points, hits, echo, col_time, chan_time, V, H):
    """the unorganized cloud: record i of the output is record i of the input"""
    return restate_format(fmt, restate_sources(points, hits, echo, col_time, chan_time, V, H))


def ranks(rays):
    """how many of the immediately preceding records i-1, i-2, i-3 carry the same ray, up to the first that differs"""
    rays = np.asarray(rays, np.uint32)
    n = rays.shape[0]
    rank = np.zeros(n, np.int64)
    for j in (1, 2, 3):
        same = np.zeros(n, bool)
        same[j:] = rays[j:] == rays[:-j]
        rank += (same & (rank == j - 1)).astype(np.int64)
    return rank


def restate_organized(fmt, points, hits, echo, col_time, chan_time, V, H):
    """the organized cloud: V * H cells, cell c holds the record of ray c whose rank equals fmt.layer, or the miss of cell c; the
    inputs must claim every cell at most once (what is unspecified otherwise is not restated)"""
    hits = np.ascontiguousarray(hits, np.uint32).reshape(-1, 4)
    cells = V * H
    pick = (ranks(hits[:, 0]) == fmt.layer) & (hits[:, 0].astype(np.int64) < cells)
    who = np.nonzero(pick)[0]
    assert len(set(hits[who, 0].tolist())) == who.size, "two records claim one cell"
    cell_hits = np.zeros((cells, 4), np.uint32)
    cell_hits[:, 0] = np.arange(cells, dtype=np.uint32)
    miss = np.ones(cells, bool)
    at = hits[who, 0].astype(np.int64)
    cell_hits[at] = hits[who]
    miss[at] = False
    cell_points = np.zeros((cells, 32), np.uint8)
    if points is not None and who.size:
        cell_points[at] = np.ascontiguousarray(points, np.uint8).reshape(-1, 32)[who]
    cell_echo = np.zeros(cells, np.uint32)
    if echo is not None and who.size:
        cell_echo[at] = np.asarray(echo, np.uint32)[who]
    return restate_format(fmt, restate_sources(cell_points, cell_hits, cell_echo, col_time, chan_time, V, H, miss=miss)), miss


# ---- ls_debug_format_record against it -------------------------------------------------------------------------------------------

def _special_floats():
    bits = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFC00001, 0x7F800001]          # +-0, +-inf, NaNs with payloads
    vals = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, -128.5, 254.5, 255.5, 32766.5, 32767.5, 65534.5, 65535.5, -1e30, 1e30, 3.0, -7.25]
    for p in (2.0 ** 31, 2.0 ** 32, 2.0 ** 7, 2.0 ** 8, 2.0 ** 15, 2.0 ** 16):
        vals += [p, float(np.nextafter(F(p), F(0))), float(np.nextafter(F(p), F(np.inf))),
                 -p, float(np.nextafter(F(-p), F(0))), float(np.nextafter(F(-p), F(-np.inf)))]
    return np.concatenate([np.array(bits, np.uint32), np.array(vals, F).view(np.uint32)])


def _special_words():
    return np.array([0, 1, 127, 128, 255, 256, 32767, 32768, 65535, 65536, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 129, 0xFFFFFF7F,
                     0xFFFFFFFF], np.uint32)


def _run_records(capi, fmt, points, hits, echo, ct_val, ch_val, V, H):
    """ls_debug_format_record for every record, with the table entries given per record -> uint8 (n, point_step), 0xEE before"""
    L = capi.load()
    n = hits.shape[0]
    out = np.full((n, fmt.point_step), 0xEE, np.uint8)
    pb, hb, ob = points.ctypes.data, hits.ctypes.data, out.ctypes.data
    ref = ctypes.byref(fmt)
    for i in range(n):
        assert L.ls_debug_format_record(ref, pb + 32 * i, hb + 16 * i, int(echo[i]), float(ct_val[i]), float(ch_val[i]), V, H, 0, ob + fmt.point_step * i) == 0
    return out


def _restate_records(fmt, points, hits, echo, ct_val, ch_val, V, H):
    """the restatement with per-record table entries: sources from restate_sources, TIME replaced by the per-record sum"""
    s = restate_sources(points, hits, echo, None, None, V, H)
    mine = hits[:, 0].astype(np.int64) < V * H
    with np.errstate(all="ignore"):
        s[6] = np.where(mine, ct_val.astype(F) + ch_val.astype(F), F(0.0)).astype(F).view(np.uint32)
    return restate_format(fmt, s)


def _all_sources_format(capi, dt, scale=1.0, bias=0.0):
    """the twelve sources in one record, every one as datatype dt, back to back"""
    nb = BYTES[dt]
    fields = [(src, dt, nb * k) + ((scale, bias) if src in FLOAT_SOURCES else ()) for k, src in enumerate(FLOAT_SOURCES + WORD_SOURCES)]
    return capi.CloudFormat(12 * nb, fields)


def _records_from(values_f, values_w, V, H, rng):
    """records whose float sources run through values_f and whose word sources through values_w (ring and column follow the ray)"""
    n = max(values_f.size, values_w.size)
    vf, vw = np.resize(values_f, n), np.resize(values_w, n)
    points = np.zeros((n, 8), np.uint32)
    points[:, 0], points[:, 1], points[:, 2], points[:, 4] = vf, np.roll(vf, 1), np.roll(vf, 2), np.roll(vf, 3)
    points[:, 3], points[:, 5] = 0xDEADBEEF, rng.integers(0, 2 ** 32, n, dtype=np.uint32)     # words no source reads
    hits = np.stack([vw, np.roll(vw, 1), np.roll(vw, 2), np.roll(vf, 4)], axis=1).astype(np.uint32)
    hits[::3, 0] = rng.integers(0, V * H, hits[::3, 0].size, dtype=np.uint32)                  # a third of the rays are of the raster
    echo = np.roll(vw, 3)
    ct_val, ch_val = np.roll(vf, 5).view(F).copy(), np.roll(vf, 6).view(F).copy()
    return points.view(np.uint8).reshape(n, 32), np.ascontiguousarray(hits), echo, ct_val, ch_val


@pytest.mark.parametrize("dt", range(1, 9))
def test_record_equals_the_restatement_for_every_source(capi, dt):
    V, H = 32, 150
    rng = np.random.default_rng(100 + dt)
    # the special values, passed through (scale 1, bias 0) and under a scale and a bias
    for scale, bias in ((1.0, 0.0), (1.0, 0.5), (-2.0, 0.0), (1000.0, -0.5)):
        fmt = _all_sources_format(capi, dt, scale, bias)
        assert capi.cloud_format_check(fmt) == 0
        rec = _records_from(_special_floats(), _special_words(), V, H, rng)
        got, want = _run_records(capi, fmt, *rec, V, H), _restate_records(fmt, *rec, V, H)
        assert np.array_equal(got, want), (dt, scale, bias, np.argwhere(got != want)[:5])
    # 10^4 random draws: 50 random scales and biases, 200 records each
    for _ in range(50):
        mag = float(10.0 ** rng.uniform(-3, 10))
        scale, bias = float(F(rng.normal() * 10.0 ** rng.uniform(-3, 4))), float(F(rng.normal() * 10.0 ** rng.uniform(-2, 5)))
        fmt = _all_sources_format(capi, dt, scale, bias)
        vf = np.concatenate([(rng.normal(size=150) * mag).astype(F).view(np.uint32), rng.integers(0, 2 ** 32, 50, dtype=np.uint32)])
        vw = rng.integers(0, 2 ** 32, 200, dtype=np.uint32) >> rng.integers(0, 32, 200).astype(np.uint32)
        rec = _records_from(vf, vw, V, H, rng)
        got, want = _run_records(capi, fmt, *rec, V, H), _restate_records(fmt, *rec, V, H)
        assert np.array_equal(got, want), (dt, scale, bias, np.argwhere(got != want)[:5])


def test_pass_through_canonical_nan_gaps_unaligned_offset_and_a_miss_cell(capi):
    V, H = 32, 150
    # Velodyne's XYZIRT: FLOAT32 `time` at byte 18 of a 22-byte step
    velodyne = capi.CloudFormat(22, [(capi.LS_FIELD_X, 7, 0), (capi.LS_FIELD_Y, 7, 4), (capi.LS_FIELD_Z, 7, 8), (capi.LS_FIELD_INTENSITY, 7, 12),
                                     (capi.LS_FIELD_RING, 4, 16), (capi.LS_FIELD_TIME, 7, 18)])
    assert capi.cloud_format_check(velodyne) == 0
    p = np.zeros(8, np.uint32)
    p[0], p[1], p[2], p[4] = 0x80000000, 0x7FC12345, F(1.25).view(np.uint32), 0xFFC00001          # -0 and two NaN payloads pass through
    hit = np.array([7 * H + 31, 5, 6, F(9.5).view(np.uint32)], np.uint32)
    got = capi.format_record(velodyne, p, hit, 0, 0.125, 0.5, V, H)
    assert got[0:4].view(np.uint32)[0] == 0x80000000 and got[4:8].view(np.uint32)[0] == 0x7FC12345
    assert got[12:16].view(np.uint32)[0] == 0xFFC00001 and got[16:18].view(np.uint16)[0] == 7
    assert got[18:22].copy().view(F)[0] == F(0.625)
    # the same NaNs under a bias, or as FLOAT64: canonical; as integers: 0.  Gaps: 0 whatever the buffer held
    gaps = capi.CloudFormat(40, [(capi.LS_FIELD_Y, 7, 1, 1.0, 1.0), (capi.LS_FIELD_INTENSITY, 8, 9), (capi.LS_FIELD_Y, 5, 20), (capi.LS_FIELD_X, 8, 30)])
    got = capi.format_record(gaps, p, hit, 0, 0.0, 0.0, V, H)
    assert got[1:5].copy().view(np.uint32)[0] == NAN32 and got[9:17].copy().view(np.uint64)[0] == NAN64
    assert got[30:38].copy().view(np.uint64)[0] == 0x8000000000000000              # (double)-0
    covered = np.zeros(40, bool)
    for a, b in ((1, 5), (9, 17), (20, 24), (30, 38)):
        covered[a:b] = True
    assert np.all(got[~covered] == 0) and np.all(got[20:24] == 0)
    s = restate_sources(p.view(np.uint8).reshape(1, 32), hit.reshape(1, 4), None, None, None, V, H)
    assert np.array_equal(got, restate_format(gaps, s)[0])
    # a foreign ray: ring, column and time are 0, the rest is formatted
    far = hit.copy()
    far[0] = V * H
    got = capi.format_record(velodyne, p, far, 0, 0.125, 0.5, V, H)
    assert got[16:18].view(np.uint16)[0] == 0 and np.all(got[18:22] == 0) and got[8:12].copy().view(F)[0] == F(1.25)
    # a miss cell: NaN for the float types, 0 for the integers, all ones for geom and prim, its own ring, ray and time
    ouster = capi.CloudFormat(48, [(capi.LS_FIELD_X, 7, 0), (capi.LS_FIELD_RANGE, 6, 4, 1000.0, 0.0), (capi.LS_FIELD_GEOM, 4, 8), (capi.LS_FIELD_PRIM, 5, 12),
                                   (capi.LS_FIELD_RING, 2, 16), (capi.LS_FIELD_COLUMN, 4, 18), (capi.LS_FIELD_RAY, 6, 20), (capi.LS_FIELD_TIME, 7, 24),
                                   (capi.LS_FIELD_ECHO, 6, 28), (capi.LS_FIELD_INTENSITY, 8, 32), (capi.LS_FIELD_Z, 3, 40, 100.0, 0.0)], organized=True)
    cell = 9 * H + 17
    got = capi.format_record(ouster, None, None, 0x77, 0.25, 0.5, V, H, cell_ray=cell)
    w = lambda a, b, t: got[a:b].copy().view(t)[0]
    assert w(0, 4, np.uint32) == NAN32 and w(4, 8, np.uint32) == 0 and w(8, 10, np.uint16) == 0xFFFF and w(12, 16, np.uint32) == 0xFFFFFFFF
    assert got[16] == 9 and w(18, 20, np.uint16) == 17 and w(20, 24, np.uint32) == cell and w(24, 28, F) == F(0.75) and w(28, 32, np.uint32) == 0
    assert w(32, 40, np.uint64) == NAN64 and w(40, 42, np.int16) == 0 and np.all(got[42:] == 0)
    cell_hit = np.array([[cell, 1, 2, 3]], np.uint32)
    s = restate_sources(None, cell_hit, None, None, None, V, H, miss=[True])
    s[6] = np.array([F(0.25) + F(0.5)], F).view(np.uint32)
    assert np.array_equal(got, restate_format(ouster, s)[0])


# ---- ls_cloud_format_check -------------------------------------------------------------------------------------------------------

def test_format_check_passes_a_valid_format_and_refuses_each_rule(capi):
    X, RING, TIME = capi.LS_FIELD_X, capi.LS_FIELD_RING, capi.LS_FIELD_TIME
    ok = lambda: capi.CloudFormat(22, [(X, 7, 0), (RING, 4, 16), (TIME, 7, 18, 1e9, 0.5)])
    assert capi.cloud_format_check(ok()) == 0
    assert capi.cloud_format_check(capi.CloudFormat(128, [(X, 8, 120)], organized=True, layer=2)) == 0
    assert capi.cloud_format_check(capi.CloudFormat(1, [(RING, 1, 0)])) == 0
    assert capi.load().ls_cloud_format_check(None) == INVALID_ARGUMENT

    def bad(change):
        f = ok()
        change(f)
        return capi.cloud_format_check(f)

    def setf(k, **kw):
        def change(f):
            for name, v in kw.items():
                setattr(f.fields[k], name, v)
        return change
    refused = {
        "step 0": bad(lambda f: setattr(f, "point_step", 0)),
        "step 129": bad(lambda f: setattr(f, "point_step", 129)),
        "no field": bad(lambda f: setattr(f, "n_fields", 0)),
        "17 fields": bad(lambda f: setattr(f, "n_fields", 17)),
        "source 0": bad(setf(0, source=0)),
        "source 13": bad(setf(0, source=13)),
        "datatype 0": bad(setf(0, datatype=0)),
        "datatype 9": bad(setf(0, datatype=9)),
        "flag bits": bad(lambda f: setattr(f, "flags", 2)),
        "layer 3": bad(lambda f: (setattr(f, "flags", 1), setattr(f, "layer", 3))),
        "layer without organized": bad(lambda f: setattr(f, "layer", 1)),
        "does not fit": bad(setf(2, offset=19)),
        "overlap": bad(setf(1, offset=3)),
        "overlap inside": bad(setf(1, offset=19)),
        "scale inf": bad(setf(2, scale=float("inf"))),
        "bias nan": bad(setf(0, bias=float("nan"))),
        "word scale": bad(setf(1, scale=2.0)),
        "word bias": bad(setf(1, bias=1.0)),
    }
    assert refused == {k: INVALID_ARGUMENT for k in refused}


# ---- ls_cloud_format_from_point_fields -------------------------------------------------------------------------------------------

def _golden_message():
    txt = open(os.path.join(DATA, "config", "hesai-pandar-XT-32-lidar_0000.json")).read()
    txt = re.sub(r"^\s*//.*$", "", txt, flags=re.M)          # the config carries whole-line comments
    return json.loads(txt)["message"]


def test_format_from_the_golden_config(capi):
    msg = _golden_message()
    fmt = capi.cloud_format_from_point_fields(msg["pointFields"], msg["pointStep"])
    assert fmt.point_step == 32 and fmt.n_fields == 5 and fmt.flags == 0 and fmt.layer == 0
    got = [(f.source, f.datatype, f.offset, f.scale, f.bias) for f in list(fmt.fields)[:5]]
    assert got == [(capi.LS_FIELD_X, 7, 0, 1.0, 0.0), (capi.LS_FIELD_Y, 7, 4, 1.0, 0.0), (capi.LS_FIELD_Z, 7, 8, 1.0, 0.0),
                   (capi.LS_FIELD_INTENSITY, 7, 16, 1.0, 0.0), (capi.LS_FIELD_RING, 4, 20, 1.0, 0.0)]      # ring as UINT16
    assert capi.cloud_format_check(fmt) == 0
    # every name of the table
    for name, source in capi.CLOUD_FIELD_NAMES.items():
        f = capi.cloud_format_from_point_fields([{"name": name, "offset": 3, "datatype": 6, "count": 1}], 8)
        assert (f.fields[0].source, f.fields[0].offset, f.fields[0].datatype) == (source, 3, 6)


def test_format_from_point_fields_refusals(capi):
    L = capi.load()
    u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)

    def call(names, offsets, datatypes, counts, step):
        n = len(names)
        arr = (ctypes.c_char_p * n)(*[s.encode() for s in names])
        o, d, c = np.array(offsets, np.uint32), np.array(datatypes, np.uint8), np.array(counts, np.uint32)
        out = capi.CloudFormat(7, [(1, 7, 0)])
        rc = L.ls_cloud_format_from_point_fields(arr, o.ctypes.data_as(u32p), d.ctypes.data_as(u8p), c.ctypes.data_as(u32p), n, step, ctypes.byref(out))
        assert rc == 0 or (out.point_step, out.n_fields) == (7, 1), "a refused call leaves the output alone"
        return rc
    assert call(["x", "ring"], [0, 4], [7, 4], [1, 1], 8) == 0
    assert call(["x", "rgb"], [0, 4], [7, 6], [1, 1], 8) == UNSUPPORTED_TYPE          # an unknown name
    assert call(["x", "Ring"], [0, 4], [7, 4], [1, 1], 8) == UNSUPPORTED_TYPE         # case-sensitive
    assert call(["x", "ring"], [0, 4], [7, 4], [1, 2], 8) == UNSUPPORTED_TYPE         # count 2
    assert call(["x", "ring"], [0, 4], [7, 4], [0, 1], 8) == UNSUPPORTED_TYPE
    assert call(["x", "ring"], [0, 2], [7, 4], [1, 1], 8) == INVALID_ARGUMENT         # the check's status: an overlap
    assert call(["x", "ring"], [0, 7], [7, 4], [1, 1], 8) == INVALID_ARGUMENT         # does not fit
    assert call(["x"], [0], [9], [1], 8) == INVALID_ARGUMENT                          # an unknown datatype
    assert call(["x"], [70000], [7], [1], 8) == INVALID_ARGUMENT
    assert call(["x"] * 17, list(range(0, 68, 4)), [7] * 17, [1] * 17, 128) == INVALID_ARGUMENT


# ---- ls_column_times -------------------------------------------------------------------------------------------------------------

def test_column_times_are_the_tau_of_the_constant_twist(capi):
    for t0, dt, n in ((0.0, 0.1 / 150, 150), (-0.05, 0.1 / 1024, 1024), (1e6 + 0.3, 55.5e-6, 2048), (0.25, 0.0, 3)):
        got = capi.column_times(t0, dt, n)
        want = (t0 + np.arange(n, dtype=np.float64) * dt).astype(np.float32)       # double, rounded once
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        # the tau ls_sweep_poses_constant_twist implies: o_h = lin_vel * tau_h, in double from the unrounded tau, rounded once
        lin = np.array([8.0, -5.0, 0.5], np.float32)
        pose = capi.sweep_poses_constant_twist(lin, (0.1, -0.15, 1.0), t0, dt, n)
        tau = t0 + np.arange(n, dtype=np.float64) * dt
        o = (lin.astype(np.float64)[None, :] * tau[:, None]).astype(np.float32)
        assert np.array_equal(pose[:, [3, 7, 11]].view(np.uint32), o.view(np.uint32))
        assert np.array_equal(tau.astype(np.float32).view(np.uint32), got.view(np.uint32))
    assert capi.column_times(0.0, 1.0, 0).size == 0
    L = capi.load()
    one = np.zeros(1, np.float32)
    f32p = ctypes.POINTER(ctypes.c_float)
    assert L.ls_column_times(0.0, 1.0, 1, None) == INVALID_ARGUMENT
    assert L.ls_column_times(float("nan"), 1.0, 1, one.ctypes.data_as(f32p)) == INVALID_ARGUMENT
    assert L.ls_column_times(0.0, float("inf"), 1, one.ctypes.data_as(f32p)) == INVALID_ARGUMENT
