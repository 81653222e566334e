"""ls_hit_attributes / ls_hit_attributes_host on the MI355X: surface attributes of hit records, against the definition restated
on the host -- the named triangle's corners with the frame transform's bits (the oracle's scene, as the brute force of
test_gpu_closest.py obtains them) through ls_debug_hit_attributes_on_triangle, the validity rule and the quad rule: all 48 bytes
of every record must be equal."""
import dataclasses

import numpy as np
import pytest

from conftest import make_tracer

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
INVALID_ARGUMENT = -2


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
    return [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], A_ben)]


def _plate():
    xs, ys = np.meshgrid(np.linspace(-3, 3, 7), np.linspace(-2, 2, 5), indexing="xy")
    pv = np.stack([xs, ys, 0.3 * xs], -1).reshape(-1, 3).astype(np.float32)
    q = []
    for j in range(4):
        for i in range(6):
            v00 = j * 7 + i
            q.append([v00, v00 + 1, v00 + 8, v00 + 7])
    return pv, np.array(q, np.uint32)


def _scene_posed_quads(oracle, capi, tr, meshes):
    """ground + ben posed + a quad mesh (a 6 x 4 plate of quads, tilted, posed)"""
    A_ben = oracle.affine_from_components(np.float32([1.5, -2.0, 0.3]), np.float32([0.2, -0.1, 1.1]))
    pv, pq = _plate()
    A_plate = oracle.affine_from_components(np.float32([4.0, 3.0, 1.5]), np.float32([0.3, 0.0, -0.4]))
    ml = [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], A_ben), (2, pv, pq, A_plate)]
    _add(tr, "ground", *meshes["ground"])
    _add(tr, "face", *meshes["ben"])
    _add(tr, "plate", pv, pq, capi.LS_GEOMETRY_TYPE_QUAD)
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
    tr.updateGeometry("face", A_ben, *meshes["ben"])
    tr.updateGeometry("plate", A_plate, pv, pq)
    assert tr.commitScene() == 0
    return ml


def _u32(rec):
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 12)


def _hits_u32(hits):
    return np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 4)


def _define(capi, scene, hits, rays=None, dirs=None):
    """The definition: per hit (ray, geom, prim, t bits) the named triangle of the oracle's scene -- a quad: its two triangles in
    order -- through ls_debug_hit_attributes_on_triangle from the ray's origin; valid when it passes with t bit-equal to hit.t.
    rays: float32 (n_rays, 8) caller rays, or None with dirs = the sensor's table directions (origin 0, p = t * d without a sum:
    the frame's points32).  -> uint32 (n, 12)"""
    h = _hits_u32(hits)
    out = np.zeros((h.shape[0], 12), np.uint32)
    out[:, 11] = h[:, 0]
    slot_of = {int(g): i for i, g in enumerate(scene.geom_ids)}
    first = [int(x) for x in scene.geom_first] + [scene.tris.shape[0]]
    bound = dirs.shape[0] if rays is None else rays.shape[0]
    zero = np.zeros(3, np.float32)
    for i in range(h.shape[0]):
        ray, geom, prim, tbits = (int(x) for x in h[i])
        if ray >= bound or geom not in slot_of:
            continue
        slot = slot_of[geom]
        quad = bool(scene.geom_quad[slot])
        n_tris = first[slot + 1] - first[slot]
        if prim >= (n_tris // 2 if quad else n_tris):
            continue
        o, d = (zero, dirs[ray]) if rays is None else (rays[ray, 0:3], rays[ray, 4:7])
        for k in ((2 * prim, 2 * prim + 1) if quad else (prim,)):
            c = scene.verts[scene.tris[first[slot] + k]]
            got = capi.hit_attributes_on_triangle(o, d, c[0], c[1], c[2])
            if got is not None and int(got[0].view(np.uint32)) == tbits:
                t, r = got
                if rays is None:
                    r[6:9] = t * np.float32(d)
                out[i, 0:6] = r[0:6].view(np.uint32)
                out[i, 6], out[i, 7] = k, 1
                out[i, 8:11] = r[6:9].view(np.uint32)
                break
    return out


def _same(got, want):
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert bad.size == 0, (bad[:10], got[bad[:3]], want[bad[:3]])


def _attr(tr, hits, rays=None):
    rc, rec = tr.hitAttributes(hits, rays)
    assert rc == 0
    return _u32(rec)


def _posed_sensor(oracle, s):
    R, Rinv = oracle.pose_from_quat(0.9, 0.1, -0.2, 0.3)
    return dataclasses.replace(s, R=R, Rinv=Rinv, t=np.float32([0.3, -0.2, 0.5]))


@pytest.mark.parametrize("engine", ["bvh", "projection"])
def test_frame_hits(oracle, capi, sensors, meshes, engine):
    """the XT-32 over ground + ben (4800 rays, 1781 points: the reference's known answer, EmbreeTracer_test.cpp; 1668 is the ground
    alone), then a posed sensor, then a posed ben with a 32-byte vertex stride
    handed over in device memory: every record valid and the definition's, p the frame's points32, tri = prim"""
    import torch
    s0 = sensors["0000"]
    A = oracle.affine_from_components(np.float32([0.4, -0.3, 0.1]), np.float32([0.1, -0.2, 0.6]))
    for case in ("plain", "posed sensor", "stride 32"):
        s = _posed_sensor(oracle, s0) if case == "posed sensor" else s0
        if case == "posed sensor":
            assert not np.array_equal(s.Rinv, np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1])) and np.any(s.t != 0)
        tr = make_tracer(capi, s, engine)
        if case == "stride 32":
            ml = _ground_ben(tr, oracle, meshes)
            bv, bt = meshes["ben"]
            wide = np.full((bv.shape[0], 8), 7.5, np.float32)
            wide[:, :3] = bv
            dv = torch.from_numpy(wide).to("cuda:0")
            dt = torch.from_numpy(np.ascontiguousarray(bt, np.uint32).view(np.int32)).to("cuda:0")
            torch.cuda.synchronize()
            tr.updateGeometryDeviceShared("face", A, dv.data_ptr(), 32, dt.data_ptr())
            assert tr.commitScene() == 0
            ml[1] = (1, bv, bt, A)
        else:
            ml = _ground_ben(tr, oracle, meshes)
        rc, pts32, hits = tr.traceScene(0)
        assert rc == 0 and hits.shape[0] > 500
        if case == "plain":
            assert tr.getTotalRays() == 4800 and hits.shape[0] == 1781
        scene = oracle.assemble_scene(s, ml)
        got = _attr(tr, hits)
        _same(got, _define(capi, scene, hits, dirs=oracle.ray_dirs(s)))
        assert np.all(got[:, 7] == 1) and (case == "posed sensor" or set(hits["geom"]) == {0, 1})
        assert np.array_equal(got[:, 8:11], np.ascontiguousarray(pts32[:, :12]).view(np.uint32).reshape(-1, 3))
        assert np.array_equal(got[:, 6], hits["prim"]) and np.array_equal(got[:, 11], hits["ray"])
        n = got[:, 0:3].view(np.float32).astype(np.float64)
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
        assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
        tr.close()


def _caller_rays(rng, scene, n_any=3200, n_plate=700, n_up=200):
    """seeded rays with origins off zero: incoherent ones through the scene's box, a set aimed at the plate (geometry 2), and
    rays that leave the scene upwards (misses)"""
    lo, hi = scene.verts.min(0), scene.verts.max(0)
    o = rng.uniform(lo - 2, hi + [2, 2, 6], (n_any, 3))
    target = rng.uniform(lo, hi, (n_any, 3))
    pt = scene.tris[int(scene.geom_first[2]):]
    w = rng.dirichlet([1, 1, 1], n_plate)
    pick = pt[rng.integers(0, pt.shape[0], n_plate)]
    on_plate = (w[:, :, None] * scene.verts[pick]).sum(1)
    o2 = on_plate + rng.normal(size=(n_plate, 3)) * 3.0
    o3 = rng.uniform(lo, hi, (n_up, 3)) + [0, 0, float(hi[2] - lo[2]) + 1.0]
    d3 = rng.normal(size=(n_up, 3)) * 0.2 + [0, 0, 1.0]
    rays = np.zeros((n_any + n_plate + n_up, 8), np.float32)
    rays[:, 0:3] = np.concatenate([o, o2, o3])
    rays[:, 4:7] = np.concatenate([target - o, (on_plate - o2) * rng.uniform(0.2, 3.0, (n_plate, 1)), d3])
    rays[:, 7] = np.inf
    return rays


def test_caller_rays(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    scene = oracle.assemble_scene(s, ml)
    rays = _caller_rays(np.random.default_rng(5), scene)
    rc, hits = tr.traceRays(rays)
    assert rc == 0
    got = _attr(tr, hits, rays)
    _same(got, _define(capi, scene, hits, rays))
    miss = hits["geom"] == INV
    assert 100 < np.count_nonzero(miss) < rays.shape[0] - 1000
    assert np.all(got[miss, :11] == 0) and np.all(got[~miss, 7] == 1) and np.array_equal(got[:, 11], np.arange(rays.shape[0]))
    plate = hits["geom"] == 2
    assert np.count_nonzero(plate & (got[:, 6] % 2 == 0)) > 50 and np.count_nonzero(plate & (got[:, 6] % 2 == 1)) > 50
    assert np.array_equal(got[plate, 6] // 2, hits["prim"][plate])
    # the device entry point on a caller stream, into a filled output, a subset of the hits in another order
    order = np.random.default_rng(6).permutation(rays.shape[0])[:3000]
    sub = np.ascontiguousarray(hits[order])
    d_h = torch.from_numpy(sub.view(np.uint8).reshape(-1)).to("cuda:0")
    d_r = torch.from_numpy(rays.view(np.uint8).reshape(-1)).to("cuda:0")
    out = torch.full((3000 * 48 + 48,), 0xAB, dtype=torch.uint8, device="cuda:0")
    qs = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert tr.hitAttributesDevice(d_h.data_ptr(), 3000, out.data_ptr(), d_rays=d_r.data_ptr(), n_rays=rays.shape[0], stream=qs.cuda_stream) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    b = out.cpu().numpy()
    assert np.array_equal(b[:3000 * 48].view(np.uint32).reshape(-1, 12), got[order]) and np.all(b[3000 * 48:] == 0xAB)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_quad_diagonal_goes_to_the_even_half(capi, sensors):
    """an axis-aligned unit quad, rays through exactly representable points of the edge its two triangles share: both halves pass
    with the same t (checked with the definition), the record names the even one"""
    ident = np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1])
    tr = make_tracer(capi, dataclasses.replace(sensors["0000"], R=ident, Rinv=ident, t=np.zeros(3, np.float32)))
    qv = np.float32([[0, 0, 2], [1, 0, 2], [1, 1, 2], [0, 1, 2]])
    qi = np.array([[0, 1, 2, 3]], np.uint32)
    _add(tr, "quad", qv, qi, capi.LS_GEOMETRY_TYPE_QUAD)
    tr.updateGeometry("quad", capi.IDENTITY_AFFINE, qv, qi)
    assert tr.commitScene() == 0
    xs = np.float32([0.5, 0.25, 0.75, 0.125, 0.875, 0.375])
    rays = np.zeros((xs.shape[0], 8), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2] = xs, 1 - xs, -1.0     # below the point (x, 1 - x, 2) of the edge v1 - v3
    rays[:, 6] = 1.0
    rays[:, 7] = np.inf
    for r in rays:
        a = capi.hit_attributes_on_triangle(r[0:3], r[4:7], qv[0], qv[1], qv[3])
        b = capi.hit_attributes_on_triangle(r[0:3], r[4:7], qv[2], qv[3], qv[1])
        assert a is not None and b is not None and a[0] == b[0] == 3.0
    rc, hits = tr.traceRays(rays)
    assert rc == 0 and np.all(hits["geom"] == 0) and np.all(hits["prim"] == 0) and np.all(hits["t"] == 3.0)
    rc, rec = tr.hitAttributes(hits, rays)
    assert rc == 0 and np.all(rec["flags"] == 1) and np.all(rec["tri"] == 0)
    assert np.all(rec["n"] == np.float32([0, 0, 1])) and np.all(rec["cos_inc"] == -1.0)
    assert np.array_equal(rec["u"], xs) and np.all(rec["v"] == 1 - xs)     # (v0, v1, v3): u with v1, v with v3
    assert np.array_equal(rec["p"], np.stack([xs, 1 - xs, np.full_like(xs, 2.0)], 1))
    tr.close()


def test_invalid_and_stale_records(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    rays = _caller_rays(np.random.default_rng(15), oracle.assemble_scene(s, ml), 1200, 300, 50)
    # two more geometries, far from every ray; the first is removed again: id 3 is a hole inside the table, id 4 its last entry
    far = np.float32([[500, 500, 300], [500.01, 500, 300], [500, 500.01, 300]])
    one = np.array([[0, 1, 2]], np.uint32)
    assert _add(tr, "spare", far, one) == 3 and _add(tr, "last", far, one) == 4
    tr.updateGeometry("spare", oracle.IDENTITY_AFFINE, far, one)
    tr.updateGeometry("last", oracle.IDENTITY_AFFINE, far, one)
    assert tr.commitScene() == 0
    assert tr.removeGeometry("spare") >= 0
    ml.append((4, far, one, oracle.IDENTITY_AFFINE))
    scene = oracle.assemble_scene(s, ml)
    rc, hits = tr.traceRays(rays)
    assert rc == 0
    good = np.nonzero(hits["geom"] != INV)[0]
    assert good.size > 600 and set(hits["geom"][good]) == {0, 1, 2}
    batch = hits.copy()
    kinds = {}
    n_elems = {0: meshes["ground"][1].shape[0], 1: meshes["ben"][1].shape[0], 2: 24}
    for j, i in enumerate(good[:560]):
        kind = j % 8
        kinds.setdefault(kind, []).append(i)
        if kind == 1:
            batch["geom"][i] = 3 if j % 16 == 1 else 1000000        # a removed id (a hole of the table); beyond the table
        elif kind == 2:
            batch["prim"][i] = n_elems[int(batch["geom"][i])]       # one past the last element
        elif kind == 3:
            batch["ray"][i] = rays.shape[0]                         # one past the last ray
        elif kind == 4:
            batch["t"][i] = np.nextafter(batch["t"][i], np.float32(np.inf))
        elif kind == 5:
            batch["t"][i] = np.nextafter(batch["t"][i], np.float32(0))
        elif kind == 6:
            batch["t"][i] = np.nan
        elif kind == 7:
            batch[i] = (batch["ray"][i], INV, INV, -1.0)
    got = _attr(tr, batch, rays)
    _same(got, _define(capi, scene, batch, rays))
    for kind, idx in kinds.items():
        assert np.all(got[idx, 7] == (1 if kind == 0 else 0)), kind
        if kind:
            assert np.all(got[idx, :11] == 0) and np.array_equal(got[idx, 11], batch["ray"][idx])
    untouched = np.setdiff1d(good, good[:560])
    assert np.all(got[untouched, 7] == 1)
    # ben moves: its old hits are stale wherever the definition says so, the others stay
    A_new = oracle.affine_from_components(np.float32([1.6, -2.0, 0.3]), np.float32([0.2, -0.1, 1.3]))
    tr.updateGeometryTransform("face", A_new)
    assert tr.commitScene() == 0
    ml[1] = (1, *meshes["ben"], A_new)
    moved = oracle.assemble_scene(s, ml)
    got = _attr(tr, hits, rays)
    _same(got, _define(capi, moved, hits, rays))
    ben = hits["geom"] == 1
    assert np.count_nonzero(ben) > 50 and np.count_nonzero(got[ben, 7] == 0) > 0
    assert np.all(got[(hits["geom"] == 0) | (hits["geom"] == 2), 7] == 1)
    # ben removed: a hole in the ids
    assert tr.removeGeometry("face") >= 0
    got = _attr(tr, hits, rays)
    _same(got, _define(capi, oracle.assemble_scene(s, [ml[0], ml[2], ml[3]]), hits, rays))
    assert np.all(got[ben, 7] == 0) and np.all(got[(hits["geom"] == 0) | (hits["geom"] == 2), 7] == 1)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_eighteen_geometries_and_a_reused_id(oracle, capi, sensors):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    rng = np.random.default_rng(9)
    sq = np.float32([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]])
    st = np.array([[0, 1, 3], [2, 3, 1]], np.uint32)
    ml = []
    for k in range(18):
        A = oracle.affine_from_components(np.float32([(k % 6) * 5.0 - 12.0, (k // 6) * 5.0 - 5.0, rng.uniform(0, 2)]),
                                          np.float32(rng.uniform(-0.6, 0.6, 3)))
        assert _add(tr, f"g{k}", sq, st) == k
        tr.updateGeometry(f"g{k}", A, sq, st)
        ml.append((k, sq, st, A))
    assert tr.commitScene() == 0

    def rays_at(scene):
        """one ray per geometry, at a point inside one of its two triangles, from an origin off zero"""
        r = np.zeros((scene.geom_ids.shape[0], 8), np.float32)
        for j in range(r.shape[0]):
            c = scene.verts[scene.tris[int(scene.geom_first[j]) + j % 2]].astype(np.float64)
            target = 0.5 * c[0] + 0.3 * c[1] + 0.2 * c[2]
            nrm = np.cross(c[1] - c[0], c[2] - c[0])
            o = target + nrm / np.linalg.norm(nrm) * 0.7 + [0.05, -0.03, 0.0]
            r[j, 0:3], r[j, 4:7], r[j, 7] = o, (target - o) * 1.7, np.inf
        return r
    scene = oracle.assemble_scene(s, ml)
    rays = rays_at(scene)
    rc, hits = tr.traceRays(rays)
    assert rc == 0 and np.array_equal(hits["geom"], np.arange(18))
    got = _attr(tr, hits, rays)
    _same(got, _define(capi, scene, hits, rays))
    assert np.all(got[:, 7] == 1) and np.array_equal(got[:, 6], np.arange(18) % 2)
    # a removal in the middle: a hole; then a new geometry takes the free id
    assert tr.removeGeometry("g7") >= 0
    holed = oracle.assemble_scene(s, ml[:7] + ml[8:])
    got = _attr(tr, hits, rays)
    _same(got, _define(capi, holed, hits, rays))
    assert got[7, 7] == 0 and np.all(np.delete(got[:, 7], 7) == 1)
    A = oracle.affine_from_components(np.float32([20.0, 8.0, 1.0]), np.float32([0.2, 0.4, -0.3]))
    assert _add(tr, "late", sq, st) == 7
    tr.updateGeometry("late", A, sq, st)
    assert tr.commitScene() == 0
    ml[7] = (7, sq, st, A)
    scene = oracle.assemble_scene(s, ml)
    got = _attr(tr, hits, rays)                 # the old hits: geometry 7's is re-resolved against the new geometry of that id
    _same(got, _define(capi, scene, hits, rays))
    assert got[7, 7] == 0 and np.all(np.delete(got[:, 7], 7) == 1)
    rays = rays_at(scene)
    rc, hits = tr.traceRays(rays)
    assert rc == 0 and np.array_equal(hits["geom"], np.arange(18))
    got = _attr(tr, hits, rays)
    _same(got, _define(capi, scene, hits, rays))
    assert np.all(got[:, 7] == 1)
    tr.close()


def test_count_on_the_device(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    _ground_ben(tr, oracle, meshes)
    rc, _, hits = tr.traceScene(0)
    assert rc == 0
    want = _attr(tr, hits)
    cap = s.V * s.H
    p, h, c = (torch.zeros(32 * cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * cap, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    out = torch.full((cap * 48,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), cap)
    tr.traceSceneAsync(1)
    assert tr.hitAttributesDevice(h.data_ptr(), cap, out.data_ptr(), d_count=c.data_ptr()) == 0   # no read-back in between
    tr.synchronize()
    torch.cuda.synchronize()
    k = int(c[0].item())
    assert k == hits.shape[0] and k < cap
    b = out.cpu().numpy()
    assert np.array_equal(b[:k * 48].view(np.uint32).reshape(-1, 12), want)
    assert np.all(b[k * 48:] == 0xAB)
    tr.close()


def test_shard_hits_carry_global_ray_indices(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    full = make_tracer(capi, s)
    _ground_ben(full, oracle, meshes)
    rc, _, fh = full.traceScene(0)
    assert rc == 0
    fa = _attr(full, fh)
    full.close()
    tr = make_tracer(capi, s)
    first, n = s.H // 3 + 1, s.H // 4
    tr.setShard(first, n)
    _ground_ben(tr, oracle, meshes)
    rc, _, hits = tr.traceScene(0)
    assert rc == 0 and hits.shape[0] > 100
    col = hits["ray"] % s.H
    assert np.all((col >= first) & (col < first + n)) and hits["ray"].max() >= s.H   # global indices
    got = _attr(tr, hits)
    assert np.all(got[:, 7] == 1)
    keep = np.isin(fh["ray"], hits["ray"])
    assert np.array_equal(fh[keep], hits) and np.array_equal(got, fa[keep])
    tr.close()


def test_return_codes(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    L = tr.L
    hits = np.zeros(4, capi.HIT_DTYPE)
    d_h = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    out = torch.full((4 * 48 + 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    # before any commit: -1, the output untouched
    assert tr.hitAttributesDevice(d_h.data_ptr(), 4, out.data_ptr()) == -1
    rc, rec = tr.hitAttributes(hits)
    assert rc == -1 and np.all(rec["flags"] == 0)
    tr.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB)
    _ground_ben(tr, oracle, meshes)
    rays = np.zeros((16, 8), np.float32)
    rays[:, 4:7], rays[:, 7] = [0.3, 0.2, -1.0], np.inf
    rc, rh = tr.traceRays(rays)
    assert rc == 0
    built = tr.info(capi.LS_INFO_RAY_QUERY_BUILT)
    assert built == 2
    # n = 0: LS_OK, nothing written
    assert tr.hitAttributesDevice(0, 0, 0) == 0
    assert tr.hitAttributesDevice(d_h.data_ptr(), 0, out.data_ptr()) == 0
    assert tr.hitAttributes(np.zeros(0, capi.HIT_DTYPE))[0] == 0
    for args in ((None, 0, None, None, 4, out.data_ptr()), (None, 0, d_h.data_ptr(), None, 4, None),
                 (None, 0, d_h.data_ptr() + 8, None, 4, out.data_ptr()), (None, 0, d_h.data_ptr(), None, 4, out.data_ptr() + 8),
                 (d_h.data_ptr() + 4, 1, d_h.data_ptr(), None, 4, out.data_ptr())):
        assert L.ls_hit_attributes(tr.h, None, *args) == INVALID_ARGUMENT, args
    assert L.ls_hit_attributes_host(tr.h, None, 0, None, 4, rec.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_hit_attributes_host(tr.h, None, 0, hits.ctypes.data, 4, None) == INVALID_ARGUMENT
    tr.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB)
    assert L.ls_hit_attributes(tr.h, None, None, 0, d_h.data_ptr(), None, 4, out.data_ptr() + 16) == 0   # 16 is enough
    rc, rec = tr.hitAttributes(rh, rays)
    assert rc == 0 and np.all(rec["flags"] == 1)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == built       # left alone
    tr.synchronize()
    b = out.cpu().numpy()
    assert np.all(b[:16] == 0xAB) and np.all(b[16:16 + 4 * 48].view(np.uint32).reshape(4, 12) == 0)   # (ray 0, geom 0, prim 0, t 0: invalid)
    tr.close()
