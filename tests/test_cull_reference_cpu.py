"""tests/cull_reference.py pinned on the CPU: must_survive against the oracle's frames, bound_f64 against sampled tangents,
box_contains and chan_query_ref against cases with known answers."""
import numpy as np
import pytest

import cull_reference as cr

I3 = np.eye(3, dtype=np.float32).reshape(9)


def _sensor(oracle, vertical, H, t=(0.0, 0.0, 0.0)):
    return oracle.Sensor(uid="cull", vertical=np.asarray(vertical, np.float32), h_begin=np.float32(0.0), h_end=np.float32(360.0), h_count=H,
                         R=I3, Rinv=I3, t=np.asarray(t, np.float32))


def _groups_of_hits(ref, perm):
    inv = np.empty(perm.shape[0], np.int64)
    inv[perm] = np.arange(perm.shape[0])
    hit = ref["gid"][ref["gid"] != 0xFFFFFFFF]
    out = np.zeros(cr.n_groups(perm.shape[0]), bool)
    out[inv[hit] // cr.GROUP] = True
    return out


def test_must_survive_is_the_hit_set_of_a_star_shaped_scene(oracle):
    """one layer seen from inside: no triangle hides another, so the groups that must survive are the groups the frame's hits name"""
    s = _sensor(oracle, np.linspace(-15.0, 15.0, 16), 64)
    v, t = cr.radial_shell(90, 40, 20.0, seed=3)
    perm = cr.morton_perm(v, t)
    ms = cr.must_survive(oracle, s, v, t, oracle.IDENTITY_AFFINE, perm)
    ref = oracle.trace_frame(s, [(0, v, t, oracle.IDENTITY_AFFINE)])
    assert np.array_equal(ms, _groups_of_hits(ref, perm))
    assert 0.1 * ms.shape[0] < ms.sum() < 0.9 * ms.shape[0]
    # a shard's columns: the hits of those columns alone
    sh = cr.must_survive(oracle, s, v, t, oracle.IDENTITY_AFFINE, perm, shard=(10, 7))
    gid = ref["gid"].reshape(s.V, s.H)[:, 10:17]
    assert np.array_equal(sh, _groups_of_hits(dict(gid=gid.reshape(-1)), perm))
    assert 0 < sh.sum() < ms.sum() and not (sh & ~ms).any()


def test_must_survive_contains_occluded_groups(oracle):
    """two layers: the outer shell is hidden, its groups must survive all the same (their triangles take part in the depth compare)"""
    s = _sensor(oracle, np.linspace(-15.0, 15.0, 16), 64)
    v0, t0 = cr.radial_shell(60, 30, 10.0, seed=1)
    v1, t1 = cr.radial_shell(60, 30, 25.0, seed=2)
    v, t = np.concatenate([v0, v1]), np.concatenate([t0, t1 + np.uint32(v0.shape[0])])
    perm = cr.morton_perm(v, t)
    ms = cr.must_survive(oracle, s, v, t, oracle.IDENTITY_AFFINE, perm)
    seen = _groups_of_hits(oracle.trace_frame(s, [(0, v, t, oracle.IDENTITY_AFFINE)]), perm)
    assert not (seen & ~ms).any()
    outer = np.array([(cr.group_triangles(perm, g) >= t0.shape[0]).all() for g in range(ms.shape[0])])
    assert (ms & outer & ~seen).sum() > 20


def _random_map(rng, k):
    lin = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    if k % 2:   # non-rigid: stretched, sheared, possibly mirrored
        lin = lin @ np.diag(rng.uniform(0.3, 3.0, 3)) @ (np.eye(3) + 0.3 * rng.standard_normal((3, 3)))
    return np.concatenate([lin, rng.uniform(-5.0, 5.0, (3, 1))], axis=1).reshape(12).astype(np.float32)


def test_bound_f64_contains_sampled_tangents(oracle):
    """2 000 random patches of four triangles under rigid and non-rigid maps: along every edge (64 points each) the true tangent of
    the elevation stays within w + rem of its value at the box centre, wherever the remainder bound applies (eps < 1/4)"""
    rng = np.random.default_rng(11)
    s = _sensor(oracle, [0.0], 8, t=(0.5, -0.25, 1.0))
    worst, used = 0.0, 0
    lam = np.linspace(0.0, 1.0, 64)[:, None]
    for k in range(2000):
        A = _random_map(rng, k)
        L, o = cr.linear_map_f64(s, A)
        centre_sensor = rng.uniform(-1.0, 1.0, 3) * np.array([40.0, 40.0, 6.0])
        centre = np.linalg.solve(L, centre_sensor - o)
        size = np.exp(rng.uniform(np.log(0.05), np.log(3.0)))
        pts = centre + rng.standard_normal((12, 3)) * size * np.array([1.0, 1.0, rng.uniform(0.02, 1.0)])
        box = cr.sheared_box_f64(pts)
        box[3:6] += 1e-12 * (np.abs(box[0:3]).max() + 1.0)   # (float64 rounding of the box's own arithmetic)
        assert cr._inside(box, pts)
        q = cr.bound_f64(s, A, box[None, :])   # (float64 boxes: nothing is rounded on the way in)
        if not q["eps"][0] < 0.25:
            continue
        used += 1
        tri = pts.reshape(4, 3, 3)
        edges = np.concatenate([tri[:, [0, 1, 2]], tri[:, [1, 2, 0]]], axis=-1).reshape(-1, 6)
        p = (edges[:, None, 0:3] * (1.0 - lam) + edges[:, None, 3:6] * lam).reshape(-1, 3) @ L.T + o
        f = p[:, 2] / np.hypot(p[:, 0], p[:, 1])
        dev, bound = np.abs(f - q["fc"][0]).max(), q["w"][0] + q["rem"][0]
        assert dev <= bound * (1.0 + 1e-9) + 1e-12, (k, dev, bound)
        worst = max(worst, dev / bound)
    assert used > 1200 and 0.9 < worst <= 1.0 + 1e-9


def test_bound_f64_reads_float32_boxes(oracle):
    s = _sensor(oracle, [0.0], 8)
    box = np.array([[10, 0, -2, 0.5, 0.5, 0.01, 0.1, 0.0], [0, 0, 0, np.inf, np.inf, np.inf, 0, 0]], np.float32)
    q = cr.bound_f64(s, oracle.IDENTITY_AFFINE, box)
    assert list(q["unbounded"]) == [False, True]
    assert q["fc"][0] == pytest.approx(-0.2) and q["rho"][0] == pytest.approx(10.0)
    # f = z / rho: df/dx = -f x / rho^2 = 0.02, df/dz = 0.1 -> w = 0.5 |0.02 + 0.1 * 0.1| + 0.5 * 0 + 0.01 * 0.1
    assert q["w"][0] == pytest.approx(0.5 * 0.03 + 0.001, rel=1e-6)


def test_clearly_between_rings_and_chan_query_ref(oracle):
    up = np.tan(np.radians(np.array([-10.0, 0.0, 0.0, 10.0]) + 0.01)).astype(np.float32)
    dn = np.tan(np.radians(np.array([-10.0, 0.0, 0.0, 10.0]) - 0.01)).astype(np.float32)
    s = _sensor(oracle, [-10.0, 0.0, 0.0, 10.0], 8)
    boxes = np.array([[10, 0, 10 * np.tan(np.radians(5.0)), 0.05, 0.05, 0.001, 0, 0],      # between the rings at 0 and 10 degrees
                      [10, 0, 0.0, 0.05, 0.05, 0.001, 0, 0],                              # on the ring at 0
                      [10, 0, 10 * np.tan(np.radians(9.9)), 0.05, 0.05, 0.05, 0, 0],      # reaches the ring at 10
                      [0.1, 0, 5.0, 0.05, 0.05, 0.001, 0, 0],                             # next to the axis
                      [0, 0, 0, np.inf, np.inf, np.inf, 0, 0]], np.float32)
    assert list(cr.clearly_between_rings(s, oracle.IDENTITY_AFFINE, boxes, up, dn)) == [True, False, False, False, False]
    lo = np.array([-np.inf, -1.0, dn[1], up[1], np.nextafter(up[2], np.float32(np.inf)), up[3], np.nextafter(up[3], np.float32(np.inf)), np.nan, 0.05], np.float32)
    hi = np.array([np.inf, -0.5, dn[1], np.inf, 0.1, up[3], np.inf, 0.0, np.nan], np.float32)
    want = [1, 0, 1, 1, 0, 1, 0, 1, 0]
    assert list(cr.chan_query_ref(up, dn, lo, hi)) == want
    ok = ~np.isnan(lo)
    assert np.array_equal(cr.chan_query_exists(up, dn, lo[ok], hi[ok]), np.array(want, np.uint8)[ok])
    rng = np.random.default_rng(2)
    lo = rng.uniform(-0.3, 0.3, 4000).astype(np.float32)
    hi = (lo + rng.uniform(-0.01, 0.2, 4000)).astype(np.float32)
    assert np.array_equal(cr.chan_query_ref(up, dn, lo, hi), cr.chan_query_exists(up, dn, lo, hi))


def test_box_contains_sees_what_is_wrong(oracle):
    v, t = cr.relief_grid(6, 5, 4.0, seed=4)
    perm = cr.morton_perm(v, t)
    ng = cr.n_groups(t.shape[0])
    gb = np.array([cr.sheared_box_f64(v[t[cr.group_triangles(perm, g)].reshape(-1)].astype(np.float64)) for g in range(ng)])
    gb[:, 3:6] = gb[:, 3:6] * (1 + 1e-5) + 1e-6
    gb = gb.astype(np.float32)
    bb = cr.sheared_box_f64(v.astype(np.float64))[None, :]
    bb[:, 3:6] = bb[:, 3:6] * (1 + 1e-5) + 1e-6
    bb = bb.astype(np.float32)
    assert cr.box_contains(v, t, perm, gb, bb) == []
    tight = gb.copy()
    tight[3, 3] *= 0.9
    assert any("group 3" in m for m in cr.box_contains(v, t, perm, tight, bb))
    thin = bb.copy()
    thin[0, 5] *= 0.5
    assert any("block 0" in m for m in cr.box_contains(v, t, perm, gb, thin))
    vn = v.copy()
    vn[int(t[perm[0], 0]), 1] = np.nan
    assert any("non-finite" in m for m in cr.box_contains(vn, t, perm, gb, bb))
    marked = gb.copy()
    touched = [g for g in range(ng) if (t[cr.group_triangles(perm, g)] == t[perm[0], 0]).any()]
    marked[touched] = [0, 0, 0, np.inf, np.inf, np.inf, 0, 0]
    assert cr.box_contains(vn, t, perm, marked, np.array([[0, 0, 0, np.inf, np.inf, np.inf, 0, 0]], np.float32)) == []
    assert cr.box_contains(v, t, perm[::-1][:-1], gb, bb) != []
