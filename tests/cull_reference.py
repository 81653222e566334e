"""What group culling (k_group_bounds, k_cull, k_project<CULLED>: csrc/ls_project.hip) may and may not do, restated with numpy and the
CPU oracle only -- nothing here shares code with the library:

  box_contains           the downloaded sheared boxes hold their vertices (float64)
  must_survive           the groups some ray of the raster (or of the shard's columns) hits: the exact necessary condition
  bound_f64              DESIGN 3.1's bound of tan(elevation) over a sheared box, in float64 without slack factors
  clearly_between_rings  the groups whose bound, doubled, meets no channel: the pass must reject them
  chan_query_ref         the channel query: lower bound of tan_up, then the tan_dn compare
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

GROUP = 4           # sorted triangles per group
BLOCK_GROUPS = 64   # groups per block


def n_groups(n_tris):
    return (n_tris + GROUP - 1) // GROUP


def as_triangles(elements):
    """uint32[n, 3] triangles, or uint32[n, 4] quads as Embree's pair (v0, v1, v3), (v2, v3, v1)"""
    e = np.asarray(elements, np.uint32)
    if e.ndim == 2 and e.shape[1] == 4:
        t = np.empty((2 * e.shape[0], 3), np.uint32)
        t[0::2] = e[:, [0, 1, 3]]
        t[1::2] = e[:, [2, 3, 1]]
        return t
    return e.reshape(-1, 3)


def group_triangles(perm, g):
    """the caller's triangles of group g (perm: sorted position -> caller's triangle)"""
    return np.asarray(perm[GROUP * g:GROUP * (g + 1)], np.int64)


def is_unbounded(boxes):
    """the marker of a box k_cull never rejects: hx = hy = hz = +inf"""
    b = np.asarray(boxes).reshape(-1, 8)
    return np.isposinf(b[:, 3]) & np.isposinf(b[:, 4]) & np.isposinf(b[:, 5])


def _inside(box, pts):
    """|a|, |b|, |g| <= 1 for every point, in the sheared-box coordinates of `box` (cx cy cz hx hy hz sx sy), float64; written
    without the divisions so that a zero half extent asks for an exact coordinate"""
    b = np.asarray(box, np.float64)
    d = np.asarray(pts, np.float64) - b[0:3]
    r = d[:, 2] - (b[6] * d[:, 0] + b[7] * d[:, 1])
    return bool(np.all(np.abs(d[:, 0]) <= b[3]) and np.all(np.abs(d[:, 1]) <= b[4]) and np.all(np.abs(r) <= b[5]))


def box_contains(verts, tris, perm, group_boxes, block_boxes):
    """-> list of human-readable violations (empty: all is well).  Every vertex of a group's triangles lies in the group's box and
    in its block's box; a group with a non-finite vertex carries the unbounded marker, and so does its block; a box that does not
    carry the marker is finite."""
    v = np.asarray(verts, np.float32)[:, :3].astype(np.float64)
    t = as_triangles(tris).astype(np.int64)
    gb, bb = np.asarray(group_boxes, np.float32).reshape(-1, 8), np.asarray(block_boxes, np.float32).reshape(-1, 8)
    ng = n_groups(t.shape[0])
    bad = []
    if sorted(np.asarray(perm).tolist()) != list(range(t.shape[0])):
        return ["perm is not a permutation of the triangles"]
    if gb.shape[0] != ng or bb.shape[0] != (ng + BLOCK_GROUPS - 1) // BLOCK_GROUPS:
        return [f"{gb.shape[0]} group boxes / {bb.shape[0]} block boxes for {ng} groups"]
    g_unb, b_unb = is_unbounded(gb), is_unbounded(bb)
    for g in range(ng):
        pts = v[t[group_triangles(perm, g)].reshape(-1)]
        finite = bool(np.isfinite(pts).all())
        blk = g // BLOCK_GROUPS
        if not finite and not g_unb[g]:
            bad.append(f"group {g} has a non-finite vertex and a bounded box")
        if not finite and not b_unb[blk]:
            bad.append(f"group {g} has a non-finite vertex and block {blk} is bounded")
        if not g_unb[g]:
            if not np.isfinite(gb[g]).all():
                bad.append(f"group {g}: box neither finite nor the unbounded marker: {gb[g]}")
            elif finite and not _inside(gb[g], pts):
                bad.append(f"group {g}: a vertex outside its box {gb[g]}")
        if not b_unb[blk]:
            if not np.isfinite(bb[blk]).all():
                bad.append(f"block {blk}: box neither finite nor the unbounded marker: {bb[blk]}")
            elif finite and not _inside(bb[blk], pts):
                bad.append(f"group {g}: a vertex outside block {blk}'s box {bb[blk]}")
    return bad


def shard_columns(H, shard):
    if shard is None:
        return np.arange(H)
    first, n = shard
    assert 0 <= first and first + n <= H
    return np.arange(first, first + n)


def must_survive(oracle, sensor, verts, tris, affine, perm, shard=None):
    """-> bool[n_groups]: group g is hit by some ray of the raster (of the shard's columns (first, n)) when it stands ALONE in the
    scene -- oracle.trace_bruteforce over sensor-frame vertices from oracle.transform_vertices, the float32 arithmetic the frame's
    exact test runs.  Whatever else is in the scene, a frame that is bit for bit the oracle's needs every such group's triangles
    tested (an occluded triangle still has to lose the depth compare), and needs no other."""
    t = as_triangles(tris)
    tv = oracle.transform_vertices(np.ascontiguousarray(np.asarray(verts, np.float32)[:, :3]), affine, sensor)
    cols = shard_columns(sensor.H, shard)
    dirs = oracle.ray_dirs(sensor).reshape(sensor.V, sensor.H, 3)[:, cols, :].reshape(-1, 3).copy()
    ng = n_groups(t.shape[0])
    out = np.zeros(ng, bool)
    empty = np.zeros(0, np.uint32)

    def some(first):   # (one call of the oracle per group; the calls release the interpreter lock)
        for g in range(first, min(first + 64, ng)):
            scene = oracle.Scene(tv, np.ascontiguousarray(t[group_triangles(perm, g)]), empty, empty)
            _, gid = oracle.trace_bruteforce(dirs, scene, nthreads=1)
            out[g] = bool((gid != oracle.INVALID).any())
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(some, range(0, ng, 64)))
    return out


def linear_map_f64(sensor, affine):
    """p' = L p + o, the vertex transform p' = Rinv ((A v) - t) in float64"""
    A = np.asarray(affine, np.float64).reshape(3, 4)
    Rinv = np.asarray(sensor.Rinv, np.float64).reshape(3, 3)
    return Rinv @ A[:, :3], Rinv @ (A[:, 3] - np.asarray(sensor.t, np.float64))


def bound_f64(sensor, affine, boxes):
    """DESIGN 3.1's bound of f = tan(elevation) = z' / rho' over the sheared boxes, float64, no slack factors -> dict of arrays:
    fc (f at the centre), w (first-order half width: the gradient carried to mesh space against the box's three edges), ez (vertical
    half extent in the sensor frame), rad (the box's radius there), eps = sqrt 2 rad / rho, rem (bound of the second-order
    remainder, valid for eps < 1/4), rho, unbounded.  nrm = sqrt of the largest absolute row sum of L^T L, an upper bound of L's
    largest singular value (1 for a rigid pose)."""
    b = np.asarray(boxes, np.float64).reshape(-1, 8)   # (float32 boxes as downloaded, or float64 ones)
    unb = is_unbounded(b)
    b = np.where(unb[:, None], 0.0, b)
    L, o = linear_map_f64(sensor, affine)
    c, hx, hy, hz, sx, sy = b[:, 0:3], b[:, 3], b[:, 4], b[:, 5], b[:, 6], b[:, 7]
    cs = c @ L.T + o
    rho = np.hypot(cs[:, 0], cs[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        fc = cs[:, 2] / rho
        grad = np.stack([-fc * cs[:, 0] / rho ** 2, -fc * cs[:, 1] / rho ** 2, 1.0 / rho], axis=1)
        g = grad @ L                                   # L^T grad f
        w = hx * np.abs(g[:, 0] + sx * g[:, 2]) + hy * np.abs(g[:, 1] + sy * g[:, 2]) + hz * np.abs(g[:, 2])
        ez = hx * np.abs(L[2, 0] + sx * L[2, 2]) + hy * np.abs(L[2, 1] + sy * L[2, 2]) + hz * np.abs(L[2, 2])
        nrm = np.sqrt(np.abs(L.T @ L).sum(axis=1).max())
        rad = nrm * (hx * (1.0 + np.abs(sx)) + hy * (1.0 + np.abs(sy)) + hz)
        eps = np.sqrt(2.0) * rad / rho
        rem = (ez * eps + (np.abs(cs[:, 2]) + ez) * 2.0 * eps * eps) / rho
    return dict(fc=fc, w=w, ez=ez, rad=rad, eps=eps, rem=rem, rho=rho, centre=cs, unbounded=unb)


def clearly_between_rings(sensor, affine, boxes, tan_up, tan_dn):
    """-> bool[n]: the boxes that are not near the vertical axis and whose interval fc +- 2 (w + rem) meets no channel's
    [tan_dn, tan_up].  The factor 2 dwarfs the kernel's own slack (1.0001 on w + rem, 3e-6 |fc|, the boxes' 1e-6 / 1e-7 pads, float32
    rounding of two dozen products) at coordinates below 1e3 m: use it only there.  'Not near the axis' leaves a tenth of room
    under the kernel's eps < 1/4 for the same roundings."""
    q = bound_f64(sensor, affine, boxes)
    half = 2.0 * (q["w"] + q["rem"])
    with np.errstate(invalid="ignore"):
        ok = ~q["unbounded"] & (q["rho"] > 1e-3) & (q["eps"] < 0.225) & np.isfinite(q["fc"]) & np.isfinite(half)
    lo, hi = q["fc"] - half, q["fc"] + half
    up, dn = np.asarray(tan_up, np.float64), np.asarray(tan_dn, np.float64)
    meets = ((up[None, :] >= lo[:, None]) & (dn[None, :] <= hi[:, None])).any(axis=1)
    return ok & ~meets


def chan_query_ref(tan_up, tan_dn, tan_lo, tan_hi):
    """is there a channel i with tan_up[i] >= tan_lo and tan_dn[i] <= tan_hi (both tables ascending)?  As the kernel asks it: i =
    the lower bound of tan_lo in tan_up (the number of entries below it: 0 for NaN), then i < V and tan_dn[i] <= tan_hi -> uint8[n]"""
    up, dn = np.asarray(tan_up, np.float32), np.asarray(tan_dn, np.float32)
    lo, hi = np.asarray(tan_lo, np.float32).reshape(-1), np.asarray(tan_hi, np.float32).reshape(-1)
    i = (up[None, :] < lo[:, None]).sum(axis=1)
    ok = i < up.shape[0]
    return (ok & (dn[np.minimum(i, up.shape[0] - 1)] <= hi)).astype(np.uint8)


def chan_query_exists(tan_up, tan_dn, tan_lo, tan_hi):
    """the same question asked of every channel (no NaN queries) -> uint8[n]"""
    up, dn = np.asarray(tan_up, np.float32), np.asarray(tan_dn, np.float32)
    lo, hi = np.asarray(tan_lo, np.float32).reshape(-1), np.asarray(tan_hi, np.float32).reshape(-1)
    return ((up[None, :] >= lo[:, None]) & (dn[None, :] <= hi[:, None])).any(axis=1).astype(np.uint8)


def sheared_box_f64(pts):
    """a sheared box around points (float64; for the CPU tests of bound_f64): the axis-aligned footprint, tilted along the least-
    squares plane through the points (slopes beyond 8: a wall, no tilt), as thick as the residuals -> cx cy cz hx hy hz sx sy"""
    p = np.asarray(pts, np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    c = 0.5 * (lo + hi)
    d = p - c
    M = np.array([[d[:, 0] @ d[:, 0], d[:, 0] @ d[:, 1]], [d[:, 0] @ d[:, 1], d[:, 1] @ d[:, 1]]])
    sx = sy = 0.0
    if np.linalg.det(M) > 1e-6 * np.trace(M) ** 2:
        sx, sy = np.linalg.solve(M, np.array([d[:, 0] @ d[:, 2], d[:, 1] @ d[:, 2]]))
        if abs(sx) > 8.0 or abs(sy) > 8.0:
            sx = sy = 0.0
    r = d[:, 2] - (sx * d[:, 0] + sy * d[:, 1])
    return np.array([c[0], c[1], c[2] + 0.5 * (r.min() + r.max()), 0.5 * (hi[0] - lo[0]), 0.5 * (hi[1] - lo[1]), 0.5 * (r.max() - r.min()), sx, sy])


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def relief_grid(nx, ny, extent, z0=-2.0, amp=0.3, seed=0, centre=(0.0, 0.0)):
    """a relief z = z0 + amp * (two sines + noise) over [-extent, extent]^2 about `centre`: (nx - 1) (ny - 1) 2 triangles"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(-extent, extent, nx) + centre[0], np.linspace(-extent, extent, ny) + centre[1], indexing="ij")
    z = z0 + amp * (np.sin(0.37 * x + 0.5) * np.cos(0.29 * y) + 0.2 * rng.standard_normal(x.shape))
    v = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).reshape(-1)
    t = np.stack([np.stack([a, a + ny, a + 1], axis=1), np.stack([a + ny, a + ny + 1, a + 1], axis=1)], axis=1).reshape(-1, 3)
    return v, t.astype(np.uint32)


def radial_shell(n_az, n_el, radius, el_range=(-25.0, 25.0), wobble=0.1, seed=0, az0=0.7131):
    """a star-shaped surface about the origin: vertices radius * (1 + wobble * noise) along a grid of directions over the whole turn
    (from az0 degrees: no mesh edge in the plane of a column of a raster that starts at a round azimuth)"""
    rng = np.random.default_rng(seed)
    az = np.radians(az0 + np.linspace(0.0, 360.0, n_az, endpoint=False))
    el = np.radians(np.linspace(el_range[0], el_range[1], n_el))
    A, E = np.meshgrid(az, el, indexing="ij")
    r = radius * (1.0 + wobble * rng.uniform(-1.0, 1.0, A.shape))
    v = np.stack([r * np.cos(E) * np.cos(A), r * np.cos(E) * np.sin(A), r * np.sin(E)], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n_az), np.arange(n_el - 1), indexing="ij")
    a, b = (i * n_el + j).reshape(-1), (((i + 1) % n_az) * n_el + j).reshape(-1)
    t = np.stack([np.stack([a, b, a + 1], axis=1), np.stack([b, b + 1, a + 1], axis=1)], axis=1).reshape(-1, 3)
    return v, t.astype(np.uint32)


def annulus(n_r, n_az, r0, r1, z0=-2.0, amp=0.05, seed=0):
    """a ring of ground between the radii r0 and r1 around the origin, (n_r - 1) n_az 2 triangles"""
    rng = np.random.default_rng(seed)
    az = np.radians(0.7131 + np.linspace(0.0, 360.0, n_az, endpoint=False))
    A, R = np.meshgrid(az, np.linspace(r0, r1, n_r), indexing="ij")
    z = z0 + amp * (np.sin(3.0 * A) + 0.3 * rng.standard_normal(A.shape))
    v = np.stack([R * np.cos(A), R * np.sin(A), z], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n_az), np.arange(n_r - 1), indexing="ij")
    a, b = (i * n_r + j).reshape(-1), (((i + 1) % n_az) * n_r + j).reshape(-1)
    t = np.stack([np.stack([a, b, a + 1], axis=1), np.stack([b, b + 1, a + 1], axis=1)], axis=1).reshape(-1, 3)
    return v, t.astype(np.uint32)


def soup(n, scale, seed=0, size=(0.02, 1.0)):
    """n unconnected triangles, centres normal(0, scale), sizes log-uniform in `size`: (3 n vertices, n triangles)"""
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, scale, size=(n, 1, 3))
    s = np.exp(rng.uniform(np.log(size[0]), np.log(size[1]), size=(n, 1, 1)))
    v = (c + rng.normal(0.0, 1.0, size=(n, 3, 3)) * s).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def wall_ring(n_az, n_z, radius, z_range=(-3.0, 3.0), taper=0.0):
    """a wall ring about the origin, n_az x (n_z - 1) x 2 triangles, its radius growing by `taper` per metre of height"""
    az = np.radians(np.linspace(0.0, 360.0, n_az, endpoint=False))
    z = np.linspace(z_range[0], z_range[1], n_z)
    A, Z = np.meshgrid(az, z, indexing="ij")
    r = radius + taper * Z
    v = np.stack([r * np.cos(A), r * np.sin(A), Z], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n_az), np.arange(n_z - 1), indexing="ij")
    a, b = (i * n_z + j).reshape(-1), (((i + 1) % n_az) * n_z + j).reshape(-1)
    t = np.stack([np.stack([a, b, a + 1], axis=1), np.stack([b, b + 1, a + 1], axis=1)], axis=1).reshape(-1, 3)
    return v, t.astype(np.uint32)


def morton_perm(verts, tris):
    """a Morton order of the triangles' centroids (for the CPU tests, which have no device order to download): 10 bits per axis"""
    v, t = np.asarray(verts, np.float64), as_triangles(tris).astype(np.int64)
    c = v[t].mean(axis=1)
    lo, ext = c.min(axis=0), max(float((c.max(axis=0) - c.min(axis=0)).max()), 1e-30)
    q = np.clip(((c - lo) / ext * 1024.0).astype(np.int64), 0, 1023)
    key = np.zeros(t.shape[0], np.int64)
    for bit in range(10):
        for ax in range(3):
            key |= ((q[:, ax] >> bit) & 1) << (3 * bit + ax)
    return np.argsort(key, kind="stable").astype(np.uint32)
