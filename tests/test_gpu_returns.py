"""ls_apply_return_model / ls_apply_return_model_host on the MI355X: sensor returns from hit records, against an expectation built
on the host -- validity and the incidence cosine from ls_hit_attributes_host, the model as restated in test_returns_cpu.py
(Python-integer Philox, np.float32 scalars), a numpy stable selection -- byte for byte: the 32-byte points, the 16-byte records
and the count."""
import ctypes
import dataclasses

import numpy as np
import pytest

from conftest import make_tracer
from test_returns_cpu import bad_models, restate

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
INVALID_ARGUMENT = -2
F = np.float32


def _add(tr, name, verts, elems, gtype=0):
    gid = tr.addGeometry(name, verts.shape[0], elems.shape[0], gtype)
    assert gid >= 0
    return gid


def _ground_ben(tr, oracle, meshes, A_ben=None):
    A_ben = oracle.IDENTITY_AFFINE if A_ben is None else A_ben
    _add(tr, "ground", *meshes["ground"])
    _add(tr, "face", *meshes["ben"])
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
    tr.updateGeometry("face", A_ben, *meshes["ben"])
    assert tr.commitScene() == 0


def _expect(capi, tr, model, hits, rays=None, dirs=None, H=0, refl=None, frame=0):
    """The kept returns of `hits`, in input order -> (points uint8[k, 32], HIT_DTYPE[k]).  rays: float32 (n_rays, 8) caller rays,
    or None with dirs = the sensor's table directions (origin 0, the point t' * d without a sum, ring = ray // H)."""
    rc, rec = tr.hitAttributes(hits, rays)
    assert rc == 0
    pts, out = [], []
    for i in np.nonzero(rec["flags"] == 1)[0]:
        h = hits[i]
        ray, geom = int(h["ray"]), int(h["geom"])
        o, d = (None, dirs[ray]) if rays is None else (rays[ray, 0:3], rays[ray, 4:7])
        d = d.astype(F)
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        rho = F(refl[geom]) if refl is not None and geom < len(refl) else F(1)
        kept, tp, inten = restate(model, ray, frame, h["t"], length, rec["cos_inc"][i], rho)
        if not kept:
            continue
        with np.errstate(all="ignore"):
            xyz = tp * d if rays is None else o.astype(F) + tp * d
        p = np.zeros(8, np.uint32)
        p[0:3] = xyz.astype(F).view(np.uint32)
        p[4] = F(inten).view(np.uint32)
        p[5] = ray // H if rays is None else 0
        pts.append(p)
        out.append((ray, geom, int(h["prim"]), tp))
    pts = np.array(pts, np.uint32).reshape(-1, 8).view(np.uint8).reshape(-1, 32)
    return pts, np.array(out, capi.HIT_DTYPE)


def _device(capi, tr, model, hits, rays=None, refl=None, frame=0, n=None, count=None, points=True, records=True, stream=None):
    """the device entry point on uploaded copies, outputs filled with 0xAB beforehand -> (points or None, records or None, k);
    everything past record k, and 64 bytes past the capacity, must still be 0xAB"""
    import torch
    n = hits.shape[0] if n is None else n
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")   # noqa: E731
    d_h = dev(hits) if hits.shape[0] else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    d_r = dev(rays) if rays is not None else None
    d_f = dev(np.asarray(refl, np.float32)) if refl is not None else None
    d_c = dev(np.array([count], np.uint32)) if count is not None else None
    d_p = torch.full((n * 32 + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_o = torch.full((n * 16 + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_n = torch.full((16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = tr.applyReturnModelDevice(model, d_h.data_ptr(), n, d_n.data_ptr(), d_points32=d_p.data_ptr() if points else 0,
                                   d_hits_out=d_o.data_ptr() if records else 0, d_rays=d_r.data_ptr() if d_r is not None else 0,
                                   n_rays=rays.shape[0] if rays is not None else 0, d_count=d_c.data_ptr() if d_c is not None else 0,
                                   d_reflectivity=d_f.data_ptr() if d_f is not None else 0, n_reflectivity=len(refl) if refl is not None else 0,
                                   frame_index=frame, stream=stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    word = d_n.cpu().numpy()
    k = int(word[:4].view(np.uint32)[0])
    assert np.all(word[4:] == 0xAB) and k <= n
    p, o = d_p.cpu().numpy(), d_o.cpu().numpy()
    assert np.all(p[(k if points else 0) * 32:] == 0xAB) and np.all(o[(k if records else 0) * 16:] == 0xAB)   # nothing past record k
    return (p[:k * 32].reshape(k, 32) if points else None), (o[:k * 16].view(capi.HIT_DTYPE) if records else None), k


def _same(got, want):
    """(points, records) pairs equal byte for byte"""
    gp, gh = got[0], got[1]
    wp, wh = want[0], want[1]
    assert gp.shape == wp.shape and gh.shape == wh.shape, (gp.shape, wp.shape, gh.shape, wh.shape)
    bad = np.nonzero(np.any(gp != wp, axis=1) | (gh.view(np.uint32).reshape(-1, 4) != wh.view(np.uint32).reshape(-1, 4)).any(axis=1))[0]
    assert bad.size == 0, (bad[:10], gp[bad[:2]].view(np.uint32), wp[bad[:2]].view(np.uint32), gh[bad[:3]], wh[bad[:3]])


def _both(capi, tr, model, hits, want, rays=None, refl=None, frame=0):
    """the host variant and the device variant give `want`"""
    rc, p, h = tr.applyReturnModel(model, hits, rays, refl, frame)
    assert rc == 0
    _same((p, h), want)
    p, h, k = _device(capi, tr, model, hits, rays, refl, frame)
    assert k == want[1].shape[0]
    _same((p, h), want)


def _full_model(capi, **kw):
    """every mechanism at once, each of them biting on the XT-32 over ground + ben (ranges 1 - 40 m)"""
    f = dict(flags=capi.LS_RETURN_LAMBERT | capi.LS_RETURN_TWO_SIDED, range_min=1.5, range_max=30.0, intensity_scale=200.0, ref_range=4.0,
             intensity_floor=0.8, intensity_max=60.0, noise_sigma0=0.01, noise_sigma1=0.002, dropout=0.2, seed=20261017)
    f.update(kw)
    return capi.ReturnModel(**f)


@pytest.mark.parametrize("engine", ["bvh", "projection"])
def test_identity_reproduces_the_frame(oracle, capi, sensors, meshes, engine):
    """flags 0, scale 64, no gate, floor, noise or drop-out: the frame's own points32, hit records and count, byte for byte -- from
    host copies, and straight from the frame's device buffers through its count word with n = the capacity"""
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s, engine)
    _ground_ben(tr, oracle, meshes)
    rc, pts32, hits = tr.traceScene(0)
    assert rc == 0 and tr.getTotalRays() == 4800 and hits.shape[0] == 1781
    ident = capi.ReturnModel()
    assert (ident.flags, ident.intensity_scale, ident.range_min, ident.range_max, ident.dropout) == (0, 64.0, 0.0, float("inf"), 0.0)
    rc, p, h = tr.applyReturnModel(ident, hits)
    assert rc == 0
    _same((p, h), (pts32, hits))
    p, h, k = _device(capi, tr, ident, hits)
    assert k == 1781
    _same((p, h), (pts32, hits))
    # the frame's device buffers, no read-back in between
    cap = s.V * s.H
    fp, fh, fc = (torch.zeros(32 * cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * cap, dtype=torch.uint8, device="cuda:0"),
                  torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    op = torch.full((32 * cap,), 0xAB, dtype=torch.uint8, device="cuda:0")
    oh = torch.full((16 * cap,), 0xAB, dtype=torch.uint8, device="cuda:0")
    on = torch.full((4,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    tr.setOutputBuffers(fp.data_ptr(), fh.data_ptr(), fc.data_ptr(), cap)
    tr.traceSceneAsync(1)
    assert tr.applyReturnModelDevice(ident, fh.data_ptr(), cap, on.data_ptr(), d_points32=op.data_ptr(), d_hits_out=oh.data_ptr(),
                                     d_count=fc.data_ptr(), frame_index=1) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert int(fc[0].item()) == 1781 and on.cpu().numpy().tolist() == [1781, -1, -1, -1]
    assert torch.equal(op[:1781 * 32], fp[:1781 * 32]) and torch.equal(oh[:1781 * 16], fh[:1781 * 16])
    assert np.array_equal(op[:1781 * 32].cpu().numpy().reshape(-1, 32), pts32)
    assert bool(torch.all(op[1781 * 32:] == 0xAB)) and bool(torch.all(oh[1781 * 16:] == 0xAB))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_full_model_on_frame_hits(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    rc, pts32, hits = tr.traceScene(0)
    assert rc == 0 and hits.shape[0] == 1781 and set(hits["geom"]) == {0, 1}
    dirs = oracle.ray_dirs(s)
    refl = [0.55]     # shorter than the geometry count: geometry 1 has reflectivity 1
    # the gate, the floor and the saturation are put where this scene's ranges and intensities lie, so that each of them bites
    open_ = dict(range_min=0.0, range_max=float("inf"), intensity_floor=0.0, intensity_max=float("inf"), dropout=0.0, noise_sigma0=0.0,
                 noise_sigma1=0.0)
    w0 = _expect(capi, tr, _full_model(capi, **open_), hits, dirs=dirs, H=s.H, refl=refl)
    assert w0[1].shape[0] == 1781
    i0, r0 = w0[0].view(np.float32)[:, 4], w0[1]["t"]
    cut = dict(range_min=float(np.percentile(r0, 5)), range_max=float(np.percentile(r0, 90)), intensity_floor=float(np.percentile(i0, 15)),
               intensity_max=float(np.percentile(i0, 85)))
    for flags in (capi.LS_RETURN_LAMBERT | capi.LS_RETURN_TWO_SIDED, capi.LS_RETURN_LAMBERT):
        m = _full_model(capi, flags=flags, **cut)
        want = _expect(capi, tr, m, hits, dirs=dirs, H=s.H, refl=refl, frame=3)
        k = want[1].shape[0]
        assert 300 < k < 1500 and set(want[1]["geom"]) == {0, 1}
        _both(capi, tr, m, hits, want, refl=refl, frame=3)
        _both(capi, tr, m, hits, want, refl=refl, frame=3)        # again: the same bytes
        inten = want[0].view(np.float32)[:, 4]
        assert inten.max() == F(cut["intensity_max"]) and np.count_nonzero(inten == inten.max()) > 10      # saturated ...
        assert inten.min() >= F(cut["intensity_floor"]) and np.unique(inten).size > 100                      # ... floored, and varying
        t_in = hits["t"][np.searchsorted(hits["ray"], want[1]["ray"])]
        assert np.count_nonzero(want[1]["t"] != t_in) > 0.9 * k                                     # noisy
        assert np.array_equal(want[0].view(np.int32)[:, 5], want[1]["ray"] // s.H)
    # every mechanism loses some returns of its own
    base = dict(range_min=0.0, range_max=float("inf"), intensity_floor=0.0, dropout=0.0)
    for one in (dict(range_min=cut["range_min"]), dict(range_max=cut["range_max"]), dict(intensity_floor=cut["intensity_floor"]), dict(dropout=0.2)):
        mm = _full_model(capi, **{**base, **one})
        w = _expect(capi, tr, mm, hits, dirs=dirs, H=s.H, refl=refl, frame=3)
        assert 0 < 1781 - w[1].shape[0] < 1781, one
        _both(capi, tr, mm, hits, w, refl=refl, frame=3)
    # another frame index: other bytes
    m = _full_model(capi, **cut)
    want3 = _expect(capi, tr, m, hits, dirs=dirs, H=s.H, refl=refl, frame=3)
    want4 = _expect(capi, tr, m, hits, dirs=dirs, H=s.H, refl=refl, frame=4)
    _both(capi, tr, m, hits, want4, refl=refl, frame=4)
    assert want3[1].shape != want4[1].shape or not np.array_equal(want3[0], want4[0])
    # no noise, no drop-out: the frame index does not matter
    quiet = _full_model(capi, **{**cut, "noise_sigma0": 0.0, "noise_sigma1": 0.0, "dropout": 0.0})
    wq = _expect(capi, tr, quiet, hits, dirs=dirs, H=s.H, refl=refl, frame=0)
    assert 300 < wq[1].shape[0] < 1781
    for frame in (0, 7, 0xFFFFFFFF):
        _both(capi, tr, quiet, hits, wq, refl=refl, frame=frame)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def _interleaved_rays(rng, n, lo, hi):
    """caller rays with origins off zero: two of three aimed at a point of the scene's box from above, every third one leaving upwards"""
    o = rng.uniform(lo + [0, 0, 2.0], hi + [0, 0, 6.0], (n, 3))
    target = rng.uniform(lo, hi, (n, 3))
    d = (target - o) * rng.uniform(0.3, 2.0, (n, 1))
    up = np.arange(n) % 3 == 2
    d[up] = rng.normal(size=(int(up.sum()), 3)) * 0.2 + [0, 0, 1.0]
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = o, d, np.inf
    return rays


def test_caller_rays_across_block_boundaries(oracle, capi, sensors, meshes):
    """3 * 256 + 17 records, hits and misses interleaved, some stale (ben moved after the trace), some corrupted: the kept ones in
    input order, the lost ones absent, ring 0; then n = 1, n = 0 and a device count below n"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    A = oracle.affine_from_components(np.float32([1.0, -1.0, 0.2]), np.float32([0.1, 0.0, 0.7]))
    _ground_ben(tr, oracle, meshes, A)
    n = 3 * 256 + 17
    scene = oracle.assemble_scene(s, [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], A)])    # sensor frame
    ben_pts = scene.verts[scene.tris[int(scene.geom_first[1]):]].reshape(-1, 3).astype(np.float64)[::11]
    lo, hi = np.maximum(scene.verts.min(0), -12.0).astype(np.float64), np.minimum(scene.verts.max(0), 12.0).astype(np.float64)
    rays = _interleaved_rays(np.random.default_rng(41), n, lo, hi)
    # a sixth of the rays at ben itself, so that some hits go stale when it moves
    at = np.arange(0, n, 6)
    rays[at, 4:7] = (ben_pts[np.arange(at.size) % ben_pts.shape[0]] - rays[at, 0:3]) * 1.5
    rc, hits = tr.traceRays(rays)
    assert rc == 0
    hit = hits["geom"] != INV
    assert 100 < np.count_nonzero(hit) < n - 200 and np.count_nonzero(hits["geom"] == 1) > 10
    for b in (256, 512, 768):       # hits and misses on both sides of every block boundary
        assert 0 < np.count_nonzero(hit[b - 8:b]) < 8 and 0 < np.count_nonzero(hit[b:b + 8]) < 8
    m = _full_model(capi, range_min=0.0, range_max=200.0, intensity_floor=0.05, intensity_max=150.0, dropout=0.15)
    refl = [0.7, 0.9]
    want = _expect(capi, tr, m, hits, rays, refl=refl, frame=2)
    assert 50 < want[1].shape[0] < np.count_nonzero(hit) and np.all(np.diff(want[1]["ray"].astype(np.int64)) > 0)
    assert np.all(want[0].view(np.int32)[:, 5] == 0)
    _both(capi, tr, m, hits, want, rays, refl, 2)
    # corrupted records among them: a bad geometry id, a bad element, a ray index out of range, t one ulp off
    batch = hits.copy()
    good = np.nonzero(hit)[0]
    for j, i in enumerate(good[::3]):
        kind = j % 4
        if kind == 0:
            batch["geom"][i] = 5 if j % 8 else 1000000
        elif kind == 1:
            batch["prim"][i] = 0x7FFFFFFF
        elif kind == 2:
            batch["ray"][i] = n
        else:
            batch["t"][i] = np.nextafter(batch["t"][i], F(np.inf if j % 8 == 3 else 0))
    want_b = _expect(capi, tr, m, batch, rays, refl=refl, frame=2)
    assert want_b[1].shape[0] < want[1].shape[0] and np.all(np.isin(want_b[1]["ray"], want[1]["ray"]))
    _both(capi, tr, m, batch, want_b, rays, refl, 2)
    # a permuted subset: the order of the input, the noise of the ray
    order = np.random.default_rng(42).permutation(n)[:600]
    sub = np.ascontiguousarray(hits[order])
    want_s = _expect(capi, tr, m, sub, rays, refl=refl, frame=2)
    _both(capi, tr, m, sub, want_s, rays, refl, 2)
    full = {int(r): (bytes(p), bytes(h)) for r, p, h in zip(want[1]["ray"], want[0], want[1].view(np.uint8).reshape(-1, 16))}
    assert all(full[int(r)] == (bytes(p), bytes(h)) for r, p, h in zip(want_s[1]["ray"], want_s[0], want_s[1].view(np.uint8).reshape(-1, 16)))
    # n = 1 (a kept record, a lost one), n = 0
    first_kept = int(np.nonzero(hits["ray"] == want[1]["ray"][0])[0][0])
    first_miss = int(np.nonzero(~hit)[0][0])
    p, h, k = _device(capi, tr, m, hits[first_kept:first_kept + 1], rays, refl, 2)
    assert k == 1 and bytes(p[0]) == bytes(want[0][0]) and h[0] == want[1][0]
    assert _device(capi, tr, m, hits[first_miss:first_miss + 1], rays, refl, 2)[2] == 0
    assert _device(capi, tr, m, hits[:0], rays, refl, 2)[2] == 0
    rc, p, h = tr.applyReturnModel(m, hits[:0], rays, refl, 2)
    assert rc == 0 and p.shape[0] == 0 and h.shape[0] == 0
    # a device count below n (and one above it): only min(n, count) records are handled, nothing is written past *n_out
    for count in (300, 256, 1, 0, n + 100):
        c = min(count, n)
        w = _expect(capi, tr, m, hits[:c], rays, refl=refl, frame=2)
        p, h, k = _device(capi, tr, m, hits, rays, refl, 2, count=count)
        assert k == w[1].shape[0]
        _same((p, h), w)
    # ben moves after the trace: its hits are stale wherever ls_hit_attributes says so
    tr.updateGeometryTransform("face", oracle.affine_from_components(np.float32([1.1, -1.0, 0.2]), np.float32([0.1, 0.0, 0.9])))
    assert tr.commitScene() == 0
    want_m = _expect(capi, tr, m, hits, rays, refl=refl, frame=2)
    assert want_m[1].shape[0] < want[1].shape[0] and np.count_nonzero(want_m[1]["geom"] == 1) < np.count_nonzero(want[1]["geom"] == 1)
    _both(capi, tr, m, hits, want_m, rays, refl, 2)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_a_shard_sees_the_noise_of_the_full_turn(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    m = _full_model(capi, range_min=0.0)
    refl = [0.8, 0.6]
    full = make_tracer(capi, s)
    _ground_ben(full, oracle, meshes)
    rc, _, fh = full.traceScene(0)
    assert rc == 0
    rc, fp, fo = full.applyReturnModel(m, fh, None, refl, 5)
    assert rc == 0 and 100 < fo.shape[0] < 1781
    full.close()
    tr = make_tracer(capi, s)
    first, n = s.H // 3 + 1, s.H // 4
    tr.setShard(first, n)
    _ground_ben(tr, oracle, meshes)
    rc, _, hits = tr.traceScene(0)
    assert rc == 0 and hits.shape[0] > 100 and hits["ray"].max() >= s.H      # global ray indices
    want = _expect(capi, tr, m, hits, dirs=oracle.ray_dirs(s), H=s.H, refl=refl, frame=5)
    _both(capi, tr, m, hits, want, refl=refl, frame=5)
    col = fo["ray"] % s.H
    inside = (col >= first) & (col < first + n)
    assert 10 < np.count_nonzero(inside) < fo.shape[0]
    _same(want, (fp[inside], fo[inside]))
    tr.close()


def test_eighteen_geometries_and_a_quad(oracle, capi, sensors):
    """more geometries than one launch of the ray queries takes (16), each with a reflectivity of its own, and a quad hit on the
    edge its two triangles share"""
    ident = np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1])
    s = dataclasses.replace(sensors["0000"], R=ident, Rinv=ident, t=np.zeros(3, np.float32))
    tr = make_tracer(capi, s)
    rng = np.random.default_rng(9)
    sq = np.float32([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]])
    st = np.array([[0, 1, 3], [2, 3, 1]], np.uint32)
    centres = []
    for k in range(18):
        c = np.float32([(k % 6) * 5.0 - 12.0, (k // 6) * 5.0 - 5.0, 1.0 + 0.1 * k])
        A = oracle.affine_from_components(c, np.float32(rng.uniform(-0.5, 0.5, 3)))
        assert _add(tr, f"g{k}", sq, st) == k
        tr.updateGeometry(f"g{k}", A, sq, st)
        centres.append(c)
    qv = np.float32([[30, 0, 2], [31, 0, 2], [31, 1, 2], [30, 1, 2]])
    qi = np.array([[0, 1, 2, 3]], np.uint32)
    assert _add(tr, "quad", qv, qi, capi.LS_GEOMETRY_TYPE_QUAD) == 18
    tr.updateGeometry("quad", capi.IDENTITY_AFFINE, qv, qi)
    assert tr.commitScene() == 0
    rays = np.zeros((18 * 3 + 6, 8), np.float32)
    rays[:, 7] = np.inf
    for j in range(18 * 3):
        o = centres[j // 3] + np.float32([0.3 * (j % 3) - 0.2, 0.1, 4.0 + j % 3])
        rays[j, 0:3], rays[j, 4:7] = o, (centres[j // 3] + np.float32([0.1, -0.1 * (j % 3), 0]) - o) * 0.5
    xs = np.float32([0.5, 0.25, 0.75, 0.125, 0.875, 0.375])
    rays[54:, 0], rays[54:, 1], rays[54:, 2], rays[54:, 6] = 30 + xs, 1 - xs, -1.0, 1.0     # below the edge v1 - v3
    rc, hits = tr.traceRays(rays)
    assert rc == 0 and np.array_equal(hits["geom"][:54], np.repeat(np.arange(18), 3)) and np.all(hits["geom"][54:] == 18)
    assert np.all(hits["prim"][54:] == 0) and np.all(hits["t"][54:] == 3.0)
    rc, rec = tr.hitAttributes(hits, rays)
    assert rc == 0 and np.all(rec["flags"] == 1) and np.all(rec["tri"][54:] == 0) and np.all(rec["cos_inc"][54:] == -1.0)
    refl = [0.05 + 0.05 * k for k in range(19)]
    m = capi.ReturnModel(flags=3, intensity_scale=100.0, ref_range=2.0, noise_sigma0=0.01, seed=7)
    want = _expect(capi, tr, m, hits, rays, refl=refl, frame=1)
    assert want[1].shape[0] == 60
    inten = want[0].view(np.float32)[:, 4]
    plain = _expect(capi, tr, m, hits, rays, frame=1)[0].view(np.float32)[:, 4]
    assert np.allclose(inten / plain, np.repeat(F(refl), 3)[:54].tolist() + [refl[18]] * 6, rtol=1e-6)   # a reflectivity per geometry
    q = F(2.0) / F(3.0)
    assert np.all(inten[54:] == ((F(100.0) * F(refl[18])) * F(1.0)) * (q * q))   # the quad: |cos_inc| = 1, r = 3
    _both(capi, tr, m, hits, want, rays, refl, 1)
    # one-sided Lambert: the quad is hit from behind, its intensity is 0 and a floor loses it
    one = capi.ReturnModel(flags=1, intensity_scale=100.0, intensity_floor=1e-6)
    w1 = _expect(capi, tr, one, hits, rays, refl=refl, frame=1)
    assert not np.any(w1[1]["geom"] == 18) and w1[1].shape[0] >= 40
    _both(capi, tr, one, hits, w1, rays, refl, 1)
    tr.close()


def test_optional_outputs(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    rc, _, hits = tr.traceScene(0)
    assert rc == 0
    m = _full_model(capi)
    want = _expect(capi, tr, m, hits, dirs=oracle.ray_dirs(s), H=s.H)
    k = want[1].shape[0]
    p, h, kk = _device(capi, tr, m, hits, records=False)
    assert kk == k and h is None and np.array_equal(p, want[0])
    p, h, kk = _device(capi, tr, m, hits, points=False)
    assert kk == k and p is None and np.array_equal(h, want[1])
    assert _device(capi, tr, m, hits, points=False, records=False)[2] == k
    # the host variant
    L = tr.L
    pts, out, n_out = np.full((1781, 32), 0xAB, np.uint8), np.zeros(1781, capi.HIT_DTYPE), ctypes.c_uint32(0)
    assert L.ls_apply_return_model_host(tr.h, ctypes.byref(m), 0, None, 0, hits.ctypes.data, 1781, None, 0, pts.ctypes.data, None, ctypes.byref(n_out)) == 0
    assert n_out.value == k and np.array_equal(pts[:k], want[0]) and np.all(pts[k:] == 0xAB)
    assert L.ls_apply_return_model_host(tr.h, ctypes.byref(m), 0, None, 0, hits.ctypes.data, 1781, None, 0, None, out.ctypes.data, ctypes.byref(n_out)) == 0
    assert n_out.value == k and np.array_equal(out[:k], want[1]) and np.all(out[k:] == np.zeros(1, capi.HIT_DTYPE))
    # a caller stream
    import torch
    qs = torch.cuda.Stream()
    p, h, kk = _device(capi, tr, m, hits, stream=qs.cuda_stream)
    assert kk == k
    _same((p, h), want)
    tr.close()


def test_return_codes(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    L = tr.L
    m = capi.ReturnModel()
    hits = np.zeros(4, capi.HIT_DTYPE)
    d_h = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    d_f = torch.ones(4, dtype=torch.float32, device="cuda:0")
    out = torch.full((4 * 32 + 32,), 0xAB, dtype=torch.uint8, device="cuda:0")
    word = torch.full((16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def untouched():
        tr.synchronize()
        torch.cuda.synchronize()
        return bool(torch.all(out == 0xAB)) and bool(torch.all(word == 0xAB))
    # before any commit: -1, nothing written
    assert tr.applyReturnModelDevice(m, d_h.data_ptr(), 4, word.data_ptr(), d_points32=out.data_ptr()) == -1
    n_out = ctypes.c_uint32(77)
    assert L.ls_apply_return_model_host(tr.h, ctypes.byref(m), 0, None, 0, hits.ctypes.data, 4, None, 0, None, None, ctypes.byref(n_out)) == -1
    assert tr.applyReturnModel(m, hits)[0] == -1 and n_out.value == 77 and untouched()
    _ground_ben(tr, oracle, meshes)
    rays = np.zeros((16, 8), np.float32)
    rays[:, 4:7], rays[:, 7] = [0.3, 0.2, -1.0], np.inf
    rc, rh = tr.traceRays(rays)
    assert rc == 0
    built = tr.info(capi.LS_INFO_RAY_QUERY_BUILT)
    # the models the entry points refuse, a NULL model, reflectivities announced but not given: before anything else
    args = (None, 0, d_h.data_ptr(), None, 4, None, 0, out.data_ptr(), None, word.data_ptr())
    for name, bad in bad_models(capi):
        assert L.ls_apply_return_model(tr.h, None, ctypes.byref(bad), 0, *args) == INVALID_ARGUMENT, name
        assert L.ls_apply_return_model_host(tr.h, ctypes.byref(bad), 0, None, 0, hits.ctypes.data, 4, None, 0, None, None, ctypes.byref(n_out)) == INVALID_ARGUMENT, name
        assert "return model" in tr.last_error()
    assert L.ls_apply_return_model(tr.h, None, None, 0, *args) == INVALID_ARGUMENT
    assert L.ls_apply_return_model_host(tr.h, None, 0, None, 0, hits.ctypes.data, 4, None, 0, None, None, ctypes.byref(n_out)) == INVALID_ARGUMENT
    assert L.ls_apply_return_model(tr.h, None, ctypes.byref(m), 0, None, 0, d_h.data_ptr(), None, 4, None, 3, out.data_ptr(), None, word.data_ptr()) == INVALID_ARGUMENT
    assert L.ls_apply_return_model_host(tr.h, ctypes.byref(m), 0, None, 0, hits.ctypes.data, 4, None, 3, None, None, ctypes.byref(n_out)) == INVALID_ARGUMENT
    # NULL records with n > 0, a NULL count output, misaligned pointers
    for a in ((None, 0, None, None, 4, None, 0, out.data_ptr(), None, word.data_ptr()),
              (None, 0, d_h.data_ptr(), None, 4, None, 0, out.data_ptr(), None, None),
              (None, 0, d_h.data_ptr() + 8, None, 4, None, 0, out.data_ptr(), None, word.data_ptr()),
              (None, 0, d_h.data_ptr(), None, 4, None, 0, out.data_ptr() + 8, None, word.data_ptr()),
              (None, 0, d_h.data_ptr(), None, 4, None, 0, None, out.data_ptr() + 8, word.data_ptr()),
              (None, 0, d_h.data_ptr(), None, 4, None, 0, out.data_ptr(), None, word.data_ptr() + 2),
              (None, 0, d_h.data_ptr(), word.data_ptr() + 2, 4, None, 0, out.data_ptr(), None, word.data_ptr()),
              (None, 0, d_h.data_ptr(), None, 4, d_f.data_ptr() + 2, 2, out.data_ptr(), None, word.data_ptr()),
              (d_h.data_ptr() + 4, 1, d_h.data_ptr(), None, 4, None, 0, out.data_ptr(), None, word.data_ptr())):
        assert L.ls_apply_return_model(tr.h, None, ctypes.byref(m), 0, *a) == INVALID_ARGUMENT, a
    assert L.ls_apply_return_model_host(tr.h, ctypes.byref(m), 0, None, 0, None, 4, None, 0, None, None, ctypes.byref(n_out)) == INVALID_ARGUMENT
    assert L.ls_apply_return_model_host(tr.h, ctypes.byref(m), 0, None, 0, hits.ctypes.data, 4, None, 0, None, None, None) == INVALID_ARGUMENT
    assert n_out.value == 77 and untouched()
    # 16 bytes are enough for the records, 4 for the words; four zero records (ray 0, geom 0, prim 0, t 0) are invalid: no return
    assert L.ls_apply_return_model(tr.h, None, ctypes.byref(m), 0, None, 0, d_h.data_ptr(), None, 4, d_f.data_ptr() + 4, 2, out.data_ptr() + 16, None,
                                   word.data_ptr() + 4) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    w = word.cpu().numpy()
    assert np.all(w[:4] == 0xAB) and np.all(w[4:8] == 0) and np.all(w[8:] == 0xAB) and bool(torch.all(out == 0xAB))
    word.fill_(0xAB)
    rc, p, h = tr.applyReturnModel(m, rh, rays)
    assert rc == 0 and h.shape[0] == 16 and np.array_equal(h, rh)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == built       # left alone
    # a geometry removed: ls_remove_geometry commits what is left (EmbreeTracer.cpp:252), so the query answers for the remaining
    # scene as ls_hit_attributes does -- the removed geometry's hits are lost -- and LS_ERR_NOT_COMMITTED, which the entry point
    # shares with it (a registry that no longer matches the committed layout), cannot be reached through the public calls
    assert tr.removeGeometry("face") >= 0
    stale = rh.copy()
    stale["geom"][::2] = 1
    want = _expect(capi, tr, m, stale, rays)
    assert want[1].shape[0] == np.count_nonzero(stale["geom"] == 0) and np.all(want[1]["geom"] == 0)
    _both(capi, tr, m, stale, want, rays)
    # every geometry removed: an empty scene
    assert tr.removeGeometry("ground") >= 0
    assert tr.applyReturnModelDevice(m, d_h.data_ptr(), 4, word.data_ptr(), d_points32=out.data_ptr()) == -1
    assert tr.applyReturnModel(m, hits)[0] == -1
    assert n_out.value == 77 and untouched()
    tr.close()


def test_open_frame_graph_is_refused(oracle, capi, sensors, meshes):
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
    out = torch.full((cap * 32,), 0xAB, dtype=torch.uint8, device="cuda:0")
    word = torch.full((4,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    m = capi.ReturnModel()
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != 0   # not LS_FRAME_EAGER: the frame is being captured, the graph is open
    assert L.ls_apply_return_model(tr.h, None, ctypes.byref(m), 0, None, 0, h.data_ptr(), c.data_ptr(), cap, None, 0, out.data_ptr(), None,
                                   word.data_ptr()) == INVALID_ARGUMENT
    n_out = ctypes.c_uint32(77)
    assert L.ls_apply_return_model_host(tr.h, ctypes.byref(m), 0, None, 0, None, 0, None, 0, None, None, ctypes.byref(n_out)) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert bool(torch.all(out == 0xAB)) and bool(torch.all(word == 0xAB)) and n_out.value == 77
    k = int(c[0].item())
    assert k > 0
    assert tr.applyReturnModelDevice(m, h.data_ptr(), cap, word.data_ptr(), d_points32=out.data_ptr(), d_count=c.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert int(word.cpu().numpy().view(np.uint32)[0]) == k and torch.equal(out[:k * 32], p[:k * 32])
    tr.close()
