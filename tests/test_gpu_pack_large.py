"""The ordered pack (csrc/ls_pack.h) beyond 256 and beyond 2048 workgroups, on the MI355X.  Every workgroup of a pack kernel adds up
the counts of the workgroups before it, eight guarded loads per lane and trip: one trip covers 2048 workgroups, and the per-call
suites stop at the XT-32's 250.  Here a synthetic raster of 131 x 6907 rays (3535 workgroups; neither V * H a multiple of 256 nor H
one of 64) turns inside a box without its top and without one side face, so that hits and misses, and 256-record blocks that are
neither empty nor full, occur below workgroup 256, between 256 and 2048, and above 2048.

No oracle run: the reference is the same call on pieces of fewer than 65 536 items -- azimuth shards for the scan frames, slices of
the input for the return model --, the path the per-call suites check against the oracle.  Whole and pieces must agree bit for
bit: count, points, hit records, echo words.  Every output has a canary record behind it (the sibling suites' helpers check it)."""
import numpy as np
import pytest

from conftest import make_tracer
from test_gpu_beams import _beams
from test_gpu_beams_sweep import _bs
from test_gpu_rays import _add
from test_gpu_returns import _device, _full_model
from test_gpu_sweep import _box_around, _same_bits, _sweep, _twist_poses

pytestmark = pytest.mark.gpu

V, H = 131, 6907
NAZ = 500                               # columns per shard: V * NAZ = 65 500 rays, 256 workgroups
SLICE = 65_000                          # records per slice of the return model's input
TRIP = 2048                             # workgroups one trip of the counts loop covers
RANGES = ((0, 256), (256, TRIP), (TRIP, None))
WEIGHTS3 = np.array([3, 1, 2], np.uint32)

_cache = {}


def _setup(oracle, capi, sensors):
    """the sensor, the mesh and the twist table: made once, never changed"""
    if "setup" not in _cache:
        from lidarshooter_amd import synth
        s0 = sensors["0000"]
        # elevations 58 .. -34 degrees, the odd channels ascending and then the even ones descending: the first and the last rings
        # look at the walls, the rings in the middle over them
        a = synth.syn_vertical(V, 58.0, 92.0)
        vertical = np.concatenate([a[1::2][::-1], a[0::2]]).astype(np.float32)
        s = oracle.Sensor(uid="large", vertical=vertical, h_begin=np.float32(0.0), h_end=np.float32(360.0), h_count=H, R=s0.R, Rinv=s0.Rinv, t=s0.t)
        assert s.V * s.H > TRIP * 256 and (s.V * s.H) % 256 != 0 and s.H % 64 != 0 and s.V * NAZ < 65_536
        verts, tris = _box_around(s.t, 40.0)
        keep = np.ones(12, bool)
        keep[[2, 3, 10, 11]] = False    # the face x = +half and the top
        pose = _twist_poses(capi, s)
        pose.setflags(write=False)
        _cache["setup"] = (s, (verts, np.ascontiguousarray(tris[keep])), pose)
    return _cache["setup"]


def _tracer(oracle, capi, sensors):
    s, mesh, pose = _setup(oracle, capi, sensors)
    tr = make_tracer(capi, s)
    _add(tr, "box", *mesh)
    tr.updateGeometry("box", oracle.IDENTITY_AFFINE, *mesh)
    assert tr.commitScene() == 0
    return tr, s, pose


def _assert_three_ranges(has):
    """has[i]: item i of a pack (a ray, a beam, an input record) produced a record.  Items with and without one, and 256-item
    blocks that are neither empty nor full, below workgroup 256, between 256 and 2048, and above 2048"""
    n = has.shape[0]
    assert n > TRIP * 256
    blocks = -(-n // 256)
    padded = np.zeros(blocks * 256, bool)
    padded[:n] = has
    per_block = padded.reshape(blocks, 256).sum(1)
    size = np.full(blocks, 256)
    size[-1] = n - (blocks - 1) * 256
    for lo, hi in RANGES:
        hi = blocks if hi is None else hi
        items = has[lo * 256:hi * 256]
        assert items.any() and not items.all(), (lo, hi)
        assert np.count_nonzero((per_block[lo:hi] > 0) & (per_block[lo:hi] < size[lo:hi])) > 0, (lo, hi)


def _per_ray(s, hits):
    return np.bincount(hits[:, 0].astype(np.int64), minlength=s.V * s.H)


def _merged(tr, s, call):
    """call() on every shard of NAZ columns, merged in ascending ray index (stable: a beam's records keep their order) -> (k, points,
    hits, ...) as call returns them"""
    parts = []
    for az0 in range(0, s.H, NAZ):
        tr.setShard(az0, min(NAZ, s.H - az0))
        assert tr.getTotalRays() < 65_536
        parts.append(call())
    tr.setShard(0, s.H)
    arrays = [np.concatenate([p[i] for p in parts]) for i in range(1, len(parts[0]))]
    order = np.argsort(arrays[1][:, 0], kind="stable")
    return (sum(p[0] for p in parts), *[a[order] for a in arrays])


def _assert_same(full, merged):
    assert full[0] == merged[0]
    for a, b in zip(full[1:], merged[1:]):
        assert _same_bits(a, b)


@pytest.mark.parametrize("deskew", [False, True])
def test_sweep_full_turn_equals_its_shards(oracle, capi, sensors, deskew):
    tr, s, pose = _tracer(oracle, capi, sensors)
    flags = capi.LS_SWEEP_DESKEW if deskew else 0
    full = _sweep(tr, pose, flags=flags)[:3]
    per_ray = _per_ray(s, full[2])
    assert per_ray.max() == 1 and np.all(np.diff(full[2][:, 0].astype(np.int64)) > 0)
    _assert_three_ranges(per_ray > 0)
    assert np.count_nonzero(per_ray.reshape(s.V, s.H).sum(1) == 0) >= 4       # upper rings miss whole
    _assert_same(full, _merged(tr, s, lambda: _sweep(tr, pose, flags=flags)[:3]))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_beams_full_turn_equals_its_shards(oracle, capi, sensors):
    """S = 3, K = 2 (FIRST | LAST): 0, 1 or 2 records per beam"""
    tr, s, pose = _tracer(oracle, capi, sensors)
    model = capi.BeamModel(capi.beam_pattern_rings(0.01, 0.01, 1, 2), 3, 1, 0.05)
    assert model.n_samples == 3 and model.n_returns == 2
    full = _beams(tr, model)
    per_beam = _per_ray(s, full[2])
    assert set(per_beam) == {0, 1, 2} and np.all(np.diff(full[2][:, 0].astype(np.int64)) >= 0)
    _assert_three_ranges(per_beam > 0)
    _assert_same(full, _merged(tr, s, lambda: _beams(tr, model)))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_beams_sweep_full_turn_equals_its_shards(oracle, capi, sensors):
    """the same with weights 3, 1, 2, a threshold a lone sample of weight 1 misses, the twist table and deskewed points"""
    tr, s, pose = _tracer(oracle, capi, sensors)
    model = capi.BeamModel(capi.beam_pattern_rings(0.01, 0.01, 1, 2), 3, 1, 0.05)
    call = lambda: _bs(tr, model, WEIGHTS3, 2, pose, capi.LS_SWEEP_DESKEW)   # noqa: E731
    full = call()
    per_beam = _per_ray(s, full[2])
    assert set(per_beam) == {0, 1, 2} and np.all(np.diff(full[2][:, 0].astype(np.int64)) >= 0)
    _assert_three_ranges(per_beam > 0)
    _assert_same(full, _merged(tr, s, call))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_return_model_equals_its_slices(oracle, capi, sensors):
    """ls_apply_return_model over the full turn's hit records with their rays: drop-out, a range gate and an intensity floor that
    bite; the whole input, then the input cut short by a device count word just above 2048 x 256"""
    tr, s, pose = _tracer(oracle, capi, sensors)
    k, _, hits, rays = _sweep(tr, pose, points=False, rays=True)
    count = TRIP * 256 + 77
    assert k > count + 256
    model = _full_model(capi, range_max=55.0)
    ray = hits[:, 0].astype(np.int64)
    pieces = [_device(capi, tr, model, hits[i:i + SLICE], rays=rays) for i in range(0, k, SLICE)]
    want_p, want_h = np.concatenate([p[0] for p in pieces]), np.concatenate([p[1] for p in pieces])
    at = np.searchsorted(ray, want_h["ray"].astype(np.int64))               # the input position of every kept record
    assert np.array_equal(ray[at], want_h["ray"]) and np.all(np.diff(at) > 0)
    kept = np.zeros(k, bool)
    kept[at] = True
    _assert_three_ranges(kept)
    got_p, got_h, got_k = _device(capi, tr, model, hits, rays=rays)
    assert got_k == len(want_h) and _same_bits(got_p, want_p) and _same_bits(got_h, want_h)
    inside = at < count
    assert 0 < np.count_nonzero(inside) < len(at)
    got_p, got_h, got_k = _device(capi, tr, model, hits, rays=rays, count=count)
    assert got_k == np.count_nonzero(inside) and _same_bits(got_p, want_p[inside]) and _same_bits(got_h, want_h[inside])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
