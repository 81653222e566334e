"""ls_closest_points / ls_closest_points_host on the MI355X: the nearest surface point to caller points, against a brute
force over the oracle's scene that runs the library's own point-triangle arithmetic on the host
(ls_debug_closest_on_triangle) over every triangle that can matter -- all 32 bytes of every record must be equal."""
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import make_tracer

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
INVALID_ARGUMENT = -2
MISS = np.array([0, 0, 0, np.float32(-1.0).view(np.uint32), INV, INV, 0, 0], np.uint32)


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


def _records(out):
    return out.view(np.uint32).reshape(-1, 8)


def _query(tr, pts):
    rc, out = tr.closestPoints(np.ascontiguousarray(pts, np.float32))
    assert rc == 0
    return _records(out)


def _query_device(tr, pts, stream=None):
    import torch
    n = pts.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(pts, np.float32).view(np.uint8).reshape(-1)).to("cuda:0")
    out = torch.full((n * 32,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert tr.closestPointsDevice(d.data_ptr(), n, out.data_ptr(), stream) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(n, 8)


def _dist64(p, a, b, c):
    """float64 distance of the point p to each triangle (a[i], b[i], c[i]): plane projection where inside, else the segments"""
    with np.errstate(all="ignore"):
        n = np.cross(b - a, c - a)
        nn = np.einsum("ij,ij->i", n, n)
        h = np.einsum("ij,ij->i", p - a, n) / nn
        proj = p - n * h[:, None]
        inside = ((np.einsum("ij,ij->i", np.cross(b - a, proj - a), n) >= 0) & (np.einsum("ij,ij->i", np.cross(c - b, proj - b), n) >= 0)
                  & (np.einsum("ij,ij->i", np.cross(a - c, proj - c), n) >= 0))
        d = np.where(inside, np.abs(h) * np.sqrt(nn), np.inf)
        for (u, v) in ((a, b), (a, c), (b, c)):
            e = v - u
            t = np.clip(np.einsum("ij,ij->i", p - u, e) / np.einsum("ij,ij->i", e, e), 0.0, 1.0)
            t = np.where(np.isfinite(t), t, 0.0)
            d = np.minimum(d, np.linalg.norm(p - (u + t[:, None] * e), axis=1))
    return d


class _Brute:
    """The definition: every triangle through ls_debug_closest_on_triangle in ascending global id, a triangle counts when its
    d2 is finite and <= radius * radius (float32), the strictly smaller d2 is kept.  To get there in reasonable time a triangle
    is only evaluated when its float64 distance is within 1e-3 relative + 1e-5 * S of the float64 minimum over the triangles
    that have an area in float32 (a superset of the issue's 1e-3 + 1e-6 * S; S = the largest |coordinate| of the point and the
    scene), found in two steps: a box distance (a lower bound) against the nearest first corner (an upper bound), then the
    exact float64 distance of the survivors.  If every evaluated triangle turns out not finite the next ring is taken."""

    def __init__(self, capi, scene):
        self.capi, self.scene = capi, scene
        V, T = scene.verts, scene.tris.astype(np.int64)
        self.a32, self.b32, self.c32 = (np.ascontiguousarray(V[T[:, k]], np.float32) for k in range(3))
        with np.errstate(all="ignore"):
            ab, ac = self.b32 - self.a32, self.c32 - self.a32   # float32, the operation order of ls_closest.h
            nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
            ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
            nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
            nn = (nx * nx + ny * ny) + nz * nz
            self.valid = (nn > 0) & (nn < np.inf)
        self.a, self.b, self.c = (x.astype(np.float64) for x in (self.a32, self.b32, self.c32))
        with np.errstate(all="ignore"):
            self.lo = np.minimum(np.minimum(self.a, self.b), self.c)
            self.hi = np.maximum(np.maximum(self.a, self.b), self.c)
        fin = V[np.isfinite(V)]
        self.vmax = float(np.abs(fin).max()) if fin.size else 0.0
        self.idx_valid = np.nonzero(self.valid)[0]

    def record(self, k, q, d2, index):
        sc = self.scene
        slot = int(np.searchsorted(sc.geom_first.astype(np.int64), k, side="right") - 1)
        local = k - int(sc.geom_first[slot])
        quad = bool(sc.geom_quad[slot]) if sc.geom_quad is not None else False
        out = np.zeros(8, np.uint32)
        out[0:3] = np.asarray(q, np.float32).view(np.uint32)
        out[3] = np.sqrt(np.float32(d2)).astype(np.float32).view(np.uint32)
        out[4], out[5], out[6] = int(sc.geom_ids[slot]), (local >> 1 if quad else local), index
        return out

    def one(self, p4, index):
        out = MISS.copy()
        out[6] = index
        p = np.float32(p4[:3])
        radius = np.float32(p4[3])
        if not (np.all(np.isfinite(p)) and radius >= 0) or self.idx_valid.size == 0:
            return out
        with np.errstate(over="ignore"):
            r2 = np.float32(radius * radius)
        p64 = p.astype(np.float64)
        S = max(self.vmax, float(np.abs(p64).max()))
        iv = self.idx_valid
        with np.errstate(all="ignore"):
            gap = np.maximum(np.maximum(self.lo[iv] - p64, p64 - self.hi[iv]), 0.0)
            lower = np.sqrt(np.einsum("ij,ij->i", gap, gap))
            upper = np.min(np.linalg.norm(self.a[iv] - p64, axis=1))
        remaining = iv[~(lower > upper * (1 + 2e-3) + 2e-5 * S)]
        d = _dist64(p64, self.a[remaining], self.b[remaining], self.c[remaining])
        while remaining.size:
            dmin = np.nanmin(d) if np.any(np.isfinite(d)) else np.inf
            take = ~(d > dmin * (1 + 1e-3) + 1e-5 * S)
            best, bid, bq, any_finite = np.float32(np.inf), -1, None, False
            for k in remaining[take]:   # ascending global id
                q, d2 = self.capi.closest_on_triangle(p, self.a32[k], self.b32[k], self.c32[k])
                if not np.isfinite(d2):
                    continue
                any_finite = True
                if d2 <= r2 and (bid < 0 or d2 < best):
                    best, bid, bq = d2, int(k), q
            if bid >= 0:
                return self.record(bid, bq, best, index)
            if any_finite:
                return out   # the smallest d2 is outside the radius
            remaining, d = remaining[~take], d[~take]
        return out

    def __call__(self, pts):
        pts = np.ascontiguousarray(pts, np.float32)
        return np.stack([self.one(pts[i], i) for i in range(pts.shape[0])]) if pts.shape[0] else np.zeros((0, 8), np.uint32)


def _with_radius(p, radius=np.inf):
    out = np.zeros((p.shape[0], 4), np.float32)
    out[:, :3] = p
    out[:, 3] = radius
    return out


def _cloud(pts32):
    return np.ascontiguousarray(pts32[:, :12]).view(np.float32).reshape(-1, 3)


def _mixed_points(rng, scene, cloud, n_box=500, n_far=24):
    """the frame's cloud as is and jittered, points in and around the box, far points, points on vertices and edge midpoints"""
    V = scene.verts
    lo, hi = V.min(0), V.max(0)
    pick = cloud[rng.choice(cloud.shape[0], min(400, cloud.shape[0]), replace=False)]
    jit = pick + rng.normal(scale=0.03, size=pick.shape).astype(np.float32)
    box = rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), (n_box, 3))
    far = rng.normal(size=(n_far, 3))
    far *= (10 ** rng.uniform(1, 3, n_far) / np.linalg.norm(far, axis=1))[:, None]
    tv = scene.tris[rng.choice(scene.tris.shape[0], 150, replace=False)]
    on_vertex = V[tv[:, 0]]
    mid = ((V[tv[:, 1]].astype(np.float64) + V[tv[:, 2]].astype(np.float64)) / 2).astype(np.float32)
    return _with_radius(np.concatenate([pick, jit, box, far, on_vertex, mid]).astype(np.float32))


@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_ground_and_ben_equal_the_brute_force(oracle, capi, sensors, meshes, engine):
    s = sensors["0000"]
    A = oracle.affine_from_components(np.float32([0.4, -0.3, 0.1]), np.float32([0.0, 0.0, 0.6]))
    tr = make_tracer(capi, s, engine)
    ml = _ground_ben(tr, oracle, meshes, A)
    rc, pts32, _ = tr.traceScene(0)
    assert rc == 0
    scene = oracle.assemble_scene(s, ml)
    pts = _mixed_points(np.random.default_rng(21), scene, _cloud(pts32))
    got = _query(tr, pts)
    want = _Brute(capi, scene)(pts)
    assert np.all(want[:, 4] != INV) and set(want[:, 4]) == {0, 1}
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert bad.size == 0, (bad[:10], got[bad[:3]], want[bad[:3]])
    # on a vertex: distance 0 exactly, and the lowest triangle that holds it
    on_vertex = slice(pts.shape[0] - 300, pts.shape[0] - 150)
    assert np.all(got[on_vertex, 3] == 0)
    assert np.array_equal(got, _query_device(tr, pts))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_traced_points_lie_on_the_surface(oracle, capi, sensors, meshes):
    """the frame's hit points t * dir: dist <= 2e-6 * S (the arithmetic's tolerance) + 4e-6 * t (the point is a rounded t * dir),
    and the triangle found is the one hit or one at equal d2"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _ground_ben(tr, oracle, meshes)
    rc, pts32, hits = tr.traceScene(0)
    assert rc == 0 and hits.shape[0] > 1000
    scene = oracle.assemble_scene(s, ml)
    cloud = _cloud(pts32)
    got = _query(tr, _with_radius(cloud))
    dist = got[:, 3].view(np.float32)
    S = max(float(np.abs(scene.verts).max()), float(np.abs(cloud).max()))
    t = hits["t"]
    print("largest dist", dist.max(), "largest dist / (2e-6 S + 4e-6 t)", (dist / (2e-6 * S + 4e-6 * t)).max())
    assert np.all(got[:, 4] != INV)
    assert np.all(dist <= 2e-6 * S + 4e-6 * t)
    other = np.nonzero((got[:, 4] != hits["geom"]) | (got[:, 5] != hits["prim"]))[0]
    print("found another triangle than the one hit:", other.size, "of", cloud.shape[0])
    first = {int(g): int(f) for g, f in zip(scene.geom_ids, scene.geom_first)}
    for i in other:
        d2 = []
        for (g, p) in ((got[i, 4], got[i, 5]), (hits["geom"][i], hits["prim"][i])):
            k = first[int(g)] + int(p)
            d2.append(capi.closest_on_triangle(cloud[i], *(scene.verts[scene.tris[k, j]] for j in range(3)))[1])
        assert d2[0] == d2[1], (i, d2, got[i], hits[i])
    tr.close()


def test_radius(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _ground_ben(tr, oracle, meshes)
    scene = oracle.assemble_scene(s, ml)
    brute = _Brute(capi, scene)
    rng = np.random.default_rng(8)
    lo, hi = scene.verts.min(0), scene.verts.max(0)
    p = rng.uniform(lo, hi + [0, 0, 2.0], (600, 3)).astype(np.float32)
    free = _query(tr, _with_radius(p))
    dist = free[:, 3].view(np.float32)
    assert np.all(free[:, 4] != INV) and np.all(dist > 0)
    # radius = dist: a hit whenever dist * dist reaches d2 again (d2 comes from the arithmetic itself)
    exact = _with_radius(p, dist)
    got = _query(tr, exact)
    want = brute(exact)
    assert np.array_equal(got, want)
    # radius just below: where radius^2 < d2 in float32, a miss
    below = _with_radius(p, np.nextafter(dist, np.float32(0)))
    d2 = np.array([capi.closest_on_triangle(p[i], *(scene.verts[scene.tris[int({0: 0, 1: scene.geom_first[1]}[int(free[i, 4])]) + int(free[i, 5]), j]]
                                                    for j in range(3)))[1] for i in range(p.shape[0])], np.float32)
    assert np.array_equal(np.sqrt(d2), dist)
    sure = below[:, 3] * below[:, 3] < d2
    hit_again = dist * dist >= d2
    assert np.count_nonzero(sure) > 300 and np.count_nonzero(hit_again) > 100
    assert np.array_equal(got[hit_again], free[hit_again])
    got = _query(tr, below)
    assert np.array_equal(got, brute(below))
    assert np.all(got[sure, 4] == INV) and np.all(got[sure, 3].view(np.float32) == -1.0) and np.all(got[sure, 0:3] == 0)
    # radius 0 on a vertex: a hit at distance 0; +inf: no bound; NaN, negative, a point that is not finite: the miss record
    v = scene.verts[scene.tris[::37, 1]]
    got = _query(tr, _with_radius(v, 0.0))
    assert np.all(got[:, 4] != INV) and np.all(got[:, 3] == 0) and np.array_equal(got[:, 0:3], v.view(np.uint32).reshape(-1, 3))
    assert np.array_equal(got, brute(_with_radius(v, 0.0)))
    good = np.float32([0.5, 0.2, -1.0, np.inf])
    bad = []
    for k in range(3):
        for x in (np.nan, np.inf, -np.inf):
            r = good.copy()
            r[k] = x
            bad.append(r)
    for x in (np.nan, -1.0, -np.inf, -1e-30):
        r = good.copy()
        r[3] = x
        bad.append(r)
    q = np.stack([good] + bad + [good])
    got = _query(tr, q)
    assert got[0, 4] != INV and np.array_equal(got[0, :6], got[-1, :6])
    want = np.tile(MISS, (len(bad), 1))
    want[:, 6] = np.arange(1, len(bad) + 1)
    assert np.array_equal(got[1:-1], want)
    assert np.array_equal(got[:, 6], np.arange(q.shape[0]))
    far = _query(tr, np.float32([[1e3, -2e3, 500.0, np.inf], [1e3, -2e3, 500.0, 10.0]]))
    assert far[0, 4] != INV and far[1, 4] == INV
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_ties_and_ids(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    A = oracle.affine_from_components(np.float32([1.0, 0.5, 0.2]), np.float32([0.1, 0.0, 0.3]))
    pv, pq = _plate()
    A_plate = oracle.affine_from_components(np.float32([4.0, 3.0, 1.5]), np.float32([0.3, 0.0, -0.4]))
    _add(tr, "a", *meshes["ben"])
    _add(tr, "b", *meshes["ben"])
    _add(tr, "plate", pv, pq, capi.LS_GEOMETRY_TYPE_QUAD)
    tr.updateGeometry("a", A, *meshes["ben"])
    tr.updateGeometry("b", A, *meshes["ben"])
    tr.updateGeometry("plate", A_plate, pv, pq)
    assert tr.commitScene() == 0
    ml = [(0, *meshes["ben"], A), (1, *meshes["ben"], A), (2, pv, pq, A_plate)]
    scene = oracle.assemble_scene(s, ml)
    rng = np.random.default_rng(31)
    lo, hi = scene.verts.min(0), scene.verts.max(0)
    pts = _with_radius(rng.uniform(lo - 1, hi + 1, (500, 3)).astype(np.float32))
    got = _query(tr, pts)
    assert np.array_equal(got, _Brute(capi, scene)(pts))
    assert not np.any(got[:, 4] == 1) and np.count_nonzero(got[:, 4] == 0) > 50   # the same mesh twice: geometry 0 wins everywhere
    on_plate = got[got[:, 4] == 2]
    assert on_plate.shape[0] > 50 and on_plate[:, 5].max() < pq.shape[0] and on_plate[:, 5].max() > pq.shape[0] // 2   # the quad index
    # a removal and a new geometry: it gets the lowest free id
    assert tr.removeGeometry("a") == 0
    assert _add(tr, "ground", *meshes["ground"]) == 0
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, *meshes["ground"])
    assert tr.commitScene() == 0
    ml[0] = (0, *meshes["ground"], oracle.IDENTITY_AFFINE)
    scene = oracle.assemble_scene(s, ml)
    got = _query(tr, pts)
    assert np.array_equal(got, _Brute(capi, scene)(pts))
    assert set(got[:, 4]) == {0, 1, 2}
    tr.close()


def test_poses(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    zero = np.zeros(12, np.float32)
    zero[3], zero[7], zero[11] = 2.0, 2.0, 0.5     # a mesh scaled to nothing next to the others: the sensor-frame slot path
    _add(tr, "hidden", *meshes["ben"])
    tr.updateGeometry("hidden", zero, *meshes["ben"])
    assert tr.commitScene() == 0
    ml.append((3, *meshes["ben"], zero))
    rng = np.random.default_rng(12)
    scene = oracle.assemble_scene(s, ml)
    lo, hi = scene.verts.min(0), scene.verts.max(0)
    pts = _with_radius(rng.uniform(lo - 0.5, hi + 0.5, (400, 3)).astype(np.float32))
    pts[:8, :3] = scene.verts[scene.tris[scene.geom_first[3], 0]]   # right where the hidden mesh collapsed to
    pts[:8, :3] += rng.normal(scale=0.01, size=(8, 3)).astype(np.float32)
    # the pose the face gets below -- rotated, scales 2, 0.5 and 1 -- and points around where it will be
    rot = oracle.affine_from_components(np.float32([-1.0, 2.5, 0.2]), np.float32([0.4, 0.3, -0.7])).reshape(3, 4)
    A_new = rot.copy()
    A_new[:, :3] = rot[:, :3] @ np.diag(np.float32([2.0, 0.5, 1.0]))
    A_new = np.ascontiguousarray(A_new, np.float32).reshape(12)
    there = oracle.assemble_scene(s, [(1, *meshes["ben"], A_new)]).verts
    pts[300:, :3] = there[rng.choice(there.shape[0], 100)] + rng.normal(scale=0.1, size=(100, 3)).astype(np.float32)
    got = _query(tr, pts)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 4
    assert np.array_equal(got, _Brute(capi, scene)(pts))
    assert not np.any(got[:, 4] == 3) and np.all(got[:, 4] != INV)
    # a pose change and a commit: nothing built, the answers follow the new pose
    tr.updateGeometryTransform("face", A_new)
    assert tr.commitScene() == 0
    got = _query(tr, pts)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0
    ml[1] = (1, *meshes["ben"], A_new)
    assert np.array_equal(got, _Brute(capi, oracle.assemble_scene(s, ml))(pts))
    assert np.count_nonzero(got[:, 4] == 1) > 20
    # new vertices: that geometry is refitted; new indices: rebuilt
    v2 = meshes["ben"][0] * np.float32(1.3)
    tr.updateGeometry("face", A_new, v2, None)
    assert tr.commitScene() == 0
    got = _query(tr, pts)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 1
    ml[1] = (1, v2, meshes["ben"][1], A_new)
    assert np.array_equal(got, _Brute(capi, oracle.assemble_scene(s, ml))(pts))
    tris = meshes["ben"][1][::-1].copy()
    tr.updateGeometry("face", A_new, v2, tris)
    assert tr.commitScene() == 0
    got = _query(tr, pts)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 1
    ml[1] = (1, v2, tris, A_new)
    assert np.array_equal(got, _Brute(capi, oracle.assemble_scene(s, ml))(pts))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_forty_geometries_three_launches(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    rng = np.random.default_rng(4)
    pv, pq = _plate()
    ptris = oracle.quads_to_triangles(pq)
    ml = []
    centers = []
    for k in range(40):
        c = np.float32([(k % 8) * 9.0 - 30.0, (k // 8) * 9.0 - 20.0, rng.uniform(0, 2)])
        A = oracle.affine_from_components(c, np.float32(rng.uniform(-1, 1, 3)))
        if k == 17:
            A = ml[3][3]   # the same pose as geometry 3 (another launch): equal d2, the lower id wins
        _add(tr, f"g{k}", pv, ptris)
        tr.updateGeometry(f"g{k}", A, pv, ptris)
        ml.append((k, pv, ptris, A))
        centers.append(c)
    assert tr.commitScene() == 0
    scene = oracle.assemble_scene(s, ml)
    lo, hi = scene.verts.min(0), scene.verts.max(0)
    pts = _with_radius(rng.uniform(lo - 2, hi + 2, (500, 3)).astype(np.float32))
    # next to the first geometry and next to the last one (in the sensor frame: their own first corners)
    pts[0, :3] = scene.verts[scene.tris[scene.geom_first[0], 0]] + np.float32([0.01, 0.02, 0.03])
    pts[1, :3] = scene.verts[scene.tris[scene.geom_first[39], 0]] + np.float32([0.01, 0.02, 0.03])
    pts[2:200, 3] = rng.uniform(0.2, 6.0, 198)
    got = _query(tr, pts)
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 40
    want = _Brute(capi, scene)(pts)
    assert want[0, 4] == 0 and want[1, 4] == 39
    assert len(set(want[:, 4]) - {INV}) >= 30 and 17 not in set(want[:, 4]) and np.count_nonzero(want[:, 4] == INV) > 5
    assert np.array_equal(got, want)
    assert np.all(got[:, 7] == 0)
    assert np.array_equal(got, _query_device(tr, pts))
    tr.close()


def test_large_mesh(oracle, capi, sensors):
    from lidarshooter_amd import synth
    s = sensors["0000"]
    grid = synth.grid_mesh(250, 200)   # 100 000 triangles
    A = oracle.affine_from_components(np.float32([2.0, -1.0, -1.5]), np.float32([0.05, -0.03, 0.8]))
    tr = make_tracer(capi, s)
    _add(tr, "grid", *grid)
    tr.updateGeometry("grid", A, *grid)
    assert tr.commitScene() == 0
    scene = oracle.assemble_scene(s, [(0, *grid, A)])
    rng = np.random.default_rng(77)
    lo, hi = scene.verts.min(0), scene.verts.max(0)
    near = scene.verts[rng.choice(scene.verts.shape[0], 1200)] + rng.normal(scale=0.05, size=(1200, 3)).astype(np.float32)
    spread = rng.uniform(lo - 5, hi + 5, (780, 3))
    far = rng.normal(size=(20, 3)) * 300.0
    pts = _with_radius(np.concatenate([near, spread, far]).astype(np.float32))
    got = _query(tr, pts)
    want = _Brute(capi, scene)(pts)
    assert np.all(want[:, 4] == 0)
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert bad.size == 0, (bad[:10], got[bad[:3]], want[bad[:3]])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def test_entry_points(oracle, capi, sensors, meshes):
    """host == device; a caller stream; refused arguments; n = 0; a removed geometry (ls_remove_geometry commits the remaining
    scene itself, so the query follows it: LS_ERR_NOT_COMMITTED is not reachable through the public entry points, as for the
    ray queries, whose host helper this query goes through); no commit and an empty scene: -1, out untouched"""
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    scene = oracle.assemble_scene(s, ml)
    rng = np.random.default_rng(19)
    lo, hi = scene.verts.min(0), scene.verts.max(0)
    pts = _with_radius(rng.uniform(lo - 1, hi + 1, (5000, 3)).astype(np.float32))
    pts[::3, 3] = rng.uniform(0.05, 3.0, pts[::3].shape[0])
    host = _query(tr, pts)
    assert np.array_equal(host, _query_device(tr, pts))
    qs = torch.cuda.Stream()
    assert np.array_equal(host, _query_device(tr, pts, qs.cuda_stream))
    assert np.array_equal(host[:300], _Brute(capi, scene)(pts[:300]))
    assert np.array_equal(host[:, 6], np.arange(pts.shape[0])) and np.all(host[:, 7] == 0)
    # the dtype form
    rec = np.zeros(50, capi.POINT_QUERY_DTYPE)
    rec["point"], rec["radius"] = pts[:50, :3], pts[:50, 3]
    rc, out = tr.closestPoints(rec)
    assert rc == 0 and out.dtype == capi.CLOSEST_DTYPE and np.array_equal(_records(out), host[:50])
    d = torch.from_numpy(pts.view(np.uint8).reshape(-1)).to("cuda:0")
    buf = torch.full((64 * 32 + 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert tr.closestPointsDevice(0, 0, 0) == 0
    assert tr.closestPoints(np.zeros((0, 4), np.float32))[0] == 0
    with pytest.raises(capi.LidarShooterHipError):
        tr.closestPointsDevice(0, 4, 0)
    with pytest.raises(capi.LidarShooterHipError):
        tr.closestPointsDevice(d.data_ptr(), 4, 0)
    with pytest.raises(capi.LidarShooterHipError):
        tr.closestPointsDevice(d.data_ptr() + 8, 4, buf.data_ptr())    # points must be 16-byte aligned
    with pytest.raises(capi.LidarShooterHipError):
        tr.closestPointsDevice(d.data_ptr(), 4, buf.data_ptr() + 8)    # and so must the records
    assert tr.closestPointsDevice(d.data_ptr(), 4, buf.data_ptr() + 16) == 0   # 16 is enough
    tr.synchronize()
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.all(b[:16] == 0xAB) and np.all(b[16 + 4 * 32:] == 0xAB) and np.array_equal(b[16:16 + 128].view(np.uint32).reshape(4, 8), host[:4])
    assert tr.removeGeometry("face") >= 0
    after = _query(tr, pts[:300])
    assert np.array_equal(after, _Brute(capi, oracle.assemble_scene(s, [ml[0], ml[2]]))(pts[:300]))
    assert not np.any(after[:, 4] == 1)
    # every geometry removed: an empty scene
    assert tr.removeGeometry("ground") >= 0 and tr.removeGeometry("plate") >= 0
    buf.fill_(0xAB)
    torch.cuda.synchronize()
    assert tr.closestPointsDevice(d.data_ptr(), 4, buf.data_ptr()) == -1
    rc, out = tr.closestPoints(pts[:5])
    assert rc == -1 and np.all(out["geom"] == INV) and np.all(out["dist"] == -1.0)
    tr.synchronize()
    assert np.all(buf.cpu().numpy() == 0xAB)
    tr.close()
    # no commit
    t2 = make_tracer(capi, s)
    assert t2.closestPointsDevice(d.data_ptr(), 4, buf.data_ptr()) == -1
    rc, out = t2.closestPoints(pts[:5])
    assert rc == -1 and np.all(out["geom"] == INV) and np.array_equal(out["index"], np.arange(5))
    t2.synchronize()
    assert np.all(buf.cpu().numpy() == 0xAB)
    t2.close()


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
    pts = torch.from_numpy(_with_radius(np.random.default_rng(6).uniform(-3, 3, (64, 3)).astype(np.float32)).reshape(-1)).to("cuda:0")
    out = torch.full((64 * 32,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != 0   # not LS_FRAME_EAGER: the frame is being captured, the graph is open
    assert L.ls_closest_points(tr.h, None, pts.data_ptr(), 64, out.data_ptr()) == INVALID_ARGUMENT
    assert L.ls_closest_points_host(tr.h, None, 0, None) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB)
    assert int(c[0].item()) > 0
    assert tr.closestPointsDevice(pts.data_ptr(), 64, out.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy().view(np.uint32).reshape(64, 8)[:, 4] != INV)
    tr.close()


def test_shared_query_set(oracle, capi, sensors, meshes):
    """one set for the three queries: what ls_trace_rays built serves ls_closest_points and the other way round"""
    s = sensors["0000"]
    rays = np.zeros((16, 8), np.float32)
    rays[:, 4:7] = [0.3, 0.2, -1.0]
    rays[:, 7] = np.inf
    pts = _with_radius(np.random.default_rng(2).uniform(-3, 3, (64, 3)).astype(np.float32))
    for first in ("rays", "points"):
        tr = make_tracer(capi, s)
        ml = _scene_posed_quads(oracle, capi, tr, meshes)
        if first == "rays":
            assert tr.traceRays(rays)[0] == 0
        else:
            _query(tr, pts)
        assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 3
        if first == "rays":
            got = _query(tr, pts)
            assert np.array_equal(got, _Brute(capi, oracle.assemble_scene(s, ml))(pts))
        else:
            assert tr.traceRays(rays)[0] == 0
        assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0
        assert tr.occludedRays(rays)[0] == 0
        assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == 0
        tr.close()


@pytest.mark.parametrize("pipeline", [0, 2])
def test_frames_are_unaffected_by_queries(oracle, capi, sensors, meshes, pipeline):
    """frames issued before, between and after nearest-point queries (on another stream in the three-stream mode): the same
    clouds as without queries, and the oracle's"""
    import torch
    s = sensors["0001"]
    A = oracle.affine_from_components(np.float32([0.3, 0.2, 0.0]), np.float32([0.0, 0.0, 0.4]))
    ml = [(0, *meshes["ground"], oracle.IDENTITY_AFFINE), (1, *meshes["ben"], A)]
    ref = oracle.trace_frame(s, ml)
    cap = s.V * s.H
    cloud = _cloud(ref["points"])
    qp = _with_radius(cloud + np.float32(0.02))
    want = None

    def run(with_queries):
        nonlocal want
        tr = make_tracer(capi, s, "projection")
        tr.setOption(capi.LS_OPT_PIPELINE, pipeline)
        if pipeline == 2:
            tr.setOption(capi.LS_OPT_FRAME_GRAPH, 1)
        _ground_ben(tr, oracle, meshes, A)
        n = qp.shape[0]
        d_pts = torch.from_numpy(qp.view(np.uint8).reshape(-1)).to("cuda:0")
        qs = torch.cuda.Stream()
        outs = [torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0") for _ in range(5)]
        bufs = [(torch.zeros(32 * cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * cap, dtype=torch.uint8, device="cuda:0"),
                 torch.zeros(4, dtype=torch.int32, device="cuda:0")) for _ in range(9)]
        torch.cuda.synchronize()
        for i in range(9):
            p, h, c = bufs[i]
            tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), cap)
            tr.traceSceneAsync(i)
            if with_queries and i % 2 == 0:
                assert tr.closestPointsDevice(d_pts.data_ptr(), n, outs[i // 2].data_ptr(), qs.cuda_stream if pipeline == 2 else None) == 0
        tr.flush()
        tr.synchronize()
        torch.cuda.synchronize()
        digests = []
        for p, h, c in bufs:
            k = int(c[0].item())
            pts = p.cpu().numpy()[:32 * k]
            assert np.array_equal(pts.reshape(k, 32), ref["points"])
            digests.append(hashlib.sha256(pts.tobytes()).hexdigest())
        if with_queries:
            res = [o.cpu().numpy().view(np.uint32).reshape(n, 8) for o in outs]
            for r in res[1:]:
                assert np.array_equal(r, res[0])
            sub = np.arange(0, n, max(1, n // 200))
            brute = _Brute(capi, oracle.assemble_scene(s, ml))(qp[sub])
            brute[:, 6] = sub
            assert np.array_equal(res[0][sub], brute)
        tr.close()
        return digests

    assert run(True) == run(False)
