"""Lattice scenes: terraced height fields whose vertices are small dyadic numbers, rays parallel to an axis or a 45-degree diagonal
through lattice points, and the EXACT closest hit of such a ray by integer arithmetic.  Plain numpy, no GPU, no library:
tests/test_lattice_cpu.py checks the oracle against this file, tests/test_gpu_lattice.py the device against both.

On random soup two events have probability zero, and both are the common case here: a ray with exact zeros in its direction that
runs in the face plane of a hierarchy box (only the widening of the slab test keeps that box), and one t on several triangles that
sit in different leaves and subtrees (only `<=` in the pruning, `t == best && id < bid` and the far clamp keep the lowest id).

Why the reference is exact: with coordinates on a lattice of 1 / scale and integer direction components, every operation of the
float32 triangle test (oracle/ls_oracle.c: tri_test) before its final divide has an integer result once scaled, and while those
integers stay below 2^24 float32 computes them without rounding; t is then the float32 nearest to the quotient of two integers.

The rule restated (lso_rays_bruteforce): den != 0; U >= 0, V >= 0, U + V <= |den|; T > 0; tmin <= t <= tmax on the rounded t;
the closest t, then the lowest triangle id; a ray with tmin > tmax or a zero direction misses."""
import numpy as np

INV = 0xFFFFFFFF
SPACING, HEIGHT_STEP = 0.5, 0.25
BLOCK = 8                                   # a plateau block: 8 x 8 vertices, 7 x 7 flat cells
DIRECTIONS = ((0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0),
              (1, 1, 0), (-1, -1, 0), (1, 0, -1), (-1, 0, 1), (0, 1, 1), (0, -1, -1))
THROUGH, SURFACE, RANGE = 0, 1, 2           # ray kinds


# ---- the scene ------------------------------------------------------------------------------------------------------------------
def heights(n, seed):
    """int (n + 1, n + 1) in units of 0.25, within [-4, 4]: blocks of 8 x 8 vertices at one height each (plateaus of 7 x 7 cells, one
    cell of slope between neighbours), every fourth block rough (a random height per vertex) so that not every hit is a tie"""
    assert n % BLOCK == 0 and n >= 2 * BLOCK
    rng = np.random.default_rng(seed)
    nb = n // BLOCK
    level = rng.integers(-4, 5, (nb, nb))
    rough = np.zeros(nb * nb, bool)
    rough[rng.permutation(nb * nb)[:max(1, nb * nb // 4)]] = True
    rough = rough.reshape(nb, nb)
    bi = np.minimum(np.arange(n + 1) // BLOCK, nb - 1)
    h = level[np.ix_(bi, bi)].copy()
    noise = rng.integers(-4, 5, (n + 1, n + 1))
    is_rough = rough[np.ix_(bi, bi)]
    h[is_rough] = noise[is_rough]
    return h


def _wall(x0, y0, along, length, top, bottom=-4):
    """an axis-aligned vertical wall on a lattice line from the lattice point (x0, y0) (units of 0.5), `length` cells along axis
    `along`, from height `bottom` to `top` (units of 0.25) in panels of 0.5 x 0.5 with two triangles each -> (verts int, tris)"""
    zs = np.arange(bottom, top + 1, 2)
    assert zs[-1] == top
    vid = {}
    verts, tris = [], []
    for k in range(length + 1):
        for z in zs:
            vid[(k, int(z))] = len(verts)
            verts.append((x0 + (k if along == 0 else 0), y0 + (k if along == 1 else 0), int(z)))
    for k in range(length):
        for z in zs[:-1]:
            a, b, c, d = vid[(k, int(z))], vid[(k + 1, int(z))], vid[(k + 1, int(z) + 2)], vid[(k, int(z) + 2)]
            tris += [(a, b, c), (a, c, d)]
    return np.array(verts, np.int64), np.array(tris, np.int64)


def terraces(n, seed):
    """A height field of n x n cells, spacing 0.5, centred on the origin -- the scene's mid-planes, and so the top Morton splits,
    pass through vertex rows --, heights multiples of 0.25 in [-1, 1], two triangles per cell (the diagonal alternates: vertices of
    degree 4 and 8), four vertical walls on lattice lines with lattice-height tops, the triangles in a seeded permutation
    (neighbours across an edge are far apart in id).  -> (verts float32 (nv, 3), tris uint32 (nt, 3))"""
    h = heights(n, seed)
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    iv = np.stack([(i - n // 2), (j - n // 2), h], -1).reshape(-1, 3).astype(np.int64)     # units: 0.5, 0.5, 0.25
    vid = lambda a, b: a * (n + 1) + b                                                       # noqa: E731
    tris = []
    for a in range(n):
        for b in range(n):
            v00, v10, v11, v01 = vid(a, b), vid(a + 1, b), vid(a + 1, b + 1), vid(a, b + 1)
            tris += [(v00, v10, v11), (v00, v11, v01)] if (a + b) % 2 == 0 else [(v00, v10, v01), (v10, v11, v01)]
    verts, tris = [iv], [np.array(tris, np.int64)]
    q = n // 4
    for x0, y0, along, length, top in ((-q + 1, -q - 2, 1, 5, 4), (q - 3, 1, 1, 6, 2), (-q - 1, q - 2, 0, 6, 4), (2, -q + 3, 0, 4, 0)):
        wv, wt = _wall(x0, y0, along, length, top)
        tris.append(wt + sum(v.shape[0] for v in verts))
        verts.append(wv)
    iv, tris = np.concatenate(verts), np.concatenate(tris)
    tris = tris[np.random.default_rng(seed + 1).permutation(tris.shape[0])]
    v = iv.astype(np.float64) * (SPACING, SPACING, HEIGHT_STEP)
    return v.astype(np.float32), tris.astype(np.uint32)


# ---- exact poses ----------------------------------------------------------------------------------------------------------------
def affine(lin=np.eye(3), trans=(0.0, 0.0, 0.0)):
    """row-major 3 x 4 float32[12]"""
    return np.concatenate([np.asarray(lin, np.float64), np.asarray(trans, np.float64).reshape(3, 1)], axis=1).astype(np.float32).reshape(12)


RZ90 = ((0, -1, 0), (1, 0, 0), (0, 0, 1))
RX90 = ((1, 0, 0), (0, 0, -1), (0, 1, 0))
POSES = {"identity": affine(), "far": affine(trans=(1024.5, -2048.25, 512.0)), "rz90": affine(RZ90, (1.5, -0.25, 0.5)),
         "rx90": affine(RX90, (-2.0, 0.75, 0.25)), "scale2": affine(2.0 * np.eye(3), (0.5, 0.5, -0.25)),
         "half": affine(0.5 * np.eye(3), (-0.5, 1.0, 0.25))}


def pose_points(p, A, t):
    """A p - t in float64: exact for the poses above (dyadic numbers, a signed permutation times a power of two)"""
    A = np.asarray(A, np.float64).reshape(3, 4)
    return np.asarray(p, np.float64) @ A[:, :3].T + A[:, 3] - np.asarray(t, np.float64)


def pose_rays(rays, A, t):
    """the rays that meet the posed scene as `rays` meet the scene: origins carried along, directions turned but not scaled (the
    ranges follow the pose's scale: every pose above scales all axes alike) -> float32 (n, 8)"""
    A = np.asarray(A, np.float64).reshape(3, 4)
    s = np.abs(A[:, :3]).sum(1)
    assert np.all(s == s[0])
    out = np.array(rays, np.float32)
    o, d = pose_points(rays[:, 0:3], A, t), np.asarray(rays[:, 4:7], np.float64) @ (A[:, :3] / s[0]).T
    assert np.array_equal(o.astype(np.float32), o) and np.array_equal(d.astype(np.float32), d)
    out[:, 0:3], out[:, 4:7] = o, d
    out[:, 3], out[:, 7] = rays[:, 3] * np.float32(s[0]), rays[:, 7] * np.float32(s[0])
    return out


# ---- the exact rule -------------------------------------------------------------------------------------------------------------
def _scale_of(*arrays):
    """the smallest power of two s <= 64 for which every value times s is an integer"""
    for s in (1, 2, 4, 8, 16, 32, 64):
        if all(np.array_equal(np.rint(a * s), a * s) for a in arrays):
            return s
    raise ValueError("not on a lattice of 1/64")


class _Exact:
    """tracks whether every float32 intermediate is an integer below 2^24 once scaled: `fits` (n rays,), over all triangles"""

    def __init__(self, n):
        self.fits = np.ones(n, bool)

    def __call__(self, x):
        self.fits &= np.abs(x).reshape(x.shape[0], -1).max(1) < (1 << 24)
        return x

    def cross(self, a, b):
        """(fma(a.y, b.z, -(a.z * b.y)), ...): the product rounds, then the fused result"""
        ax, ay, az = a
        bx, by, bz = b
        return (self(ay * bz - self(az * by)), self(az * bx - self(ax * bz)), self(ax * by - self(ay * bx)))

    def dot(self, a, b):
        """fma(a.x, b.x, fma(a.y, b.y, a.z * b.z)): three roundings"""
        return self(a[0] * b[0] + self(a[1] * b[1] + self(a[2] * b[2])))


def exact_closest(rays, verts, tris, chunk=128):
    """The closest hit of every ray by the rule in this file's head, in int64 with the coordinates scaled to integers (by 4 for the
    scene as built; by what a pose needs otherwise).  rays float32 (n, 8): origin, tmin, direction, tmax; the direction components
    are integers.  -> dict: gid uint32[n] (INV: a miss), t float32[n] (-1: a miss; the float32 nearest to num / den), num, den int64[n]
    (the exact t in lowest terms; 0 / 1 for a miss), ties int[n] (triangles that hit at the winner's t, the winner included), mask
    bool[n]: every intermediate of the float32 sequence (e1, e2, Ng, C, R, den, U, V, U + V, T, with the partial sums of the fused
    products) is an integer below 2^24, for every triangle, and no two different exact t round to the winner's float32 -- only
    there is the exact answer THE answer of the float32 test."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    v64 = np.asarray(verts, np.float64)
    s = _scale_of(v64, rays[:, 0:3].astype(np.float64))
    d64 = rays[:, 4:7].astype(np.float64)
    assert np.array_equal(np.rint(d64), d64), "integer directions only"
    iv = np.rint(v64 * s).astype(np.int64)
    p = iv[np.asarray(tris).astype(np.int64)]                                            # (nt, 3 corners, 3 axes)
    v0, v1, v2 = (tuple(p[None, :, c, a] for a in range(3)) for c in range(3))           # (1, nt) each
    n, nt = rays.shape[0], p.shape[0]
    tri_ok = _Exact(1)
    e1 = tuple(tri_ok(v0[a] - v1[a]) for a in range(3))
    e2 = tuple(tri_ok(v2[a] - v0[a]) for a in range(3))
    Ng = tri_ok.cross(e2, e1)
    out = dict(gid=np.full(n, INV, np.uint32), t=np.full(n, -1.0, np.float32), num=np.zeros(n, np.int64), den=np.ones(n, np.int64),
               ties=np.zeros(n, np.int64), mask=np.zeros(n, bool))
    for lo in range(0, n, chunk):
        r = rays[lo:lo + chunk]
        m = r.shape[0]
        org = tuple(np.rint(r[:, a].astype(np.float64) * s).astype(np.int64)[:, None] for a in range(3))
        d = tuple(np.rint(r[:, 4 + a].astype(np.float64)).astype(np.int64)[:, None] for a in range(3))
        ex = _Exact(m)
        C = tuple(ex(v0[a] - org[a]) for a in range(3))
        R = ex.cross(C, d)
        den = ex.dot(Ng, d) + np.zeros((m, 1), np.int64)
        sg = np.sign(den)
        U, V, T = ex.dot(R, e2) * sg, ex.dot(R, e1) * sg, ex.dot(Ng, C) * sg
        aden = np.abs(den)
        hit = (den != 0) & (U >= 0) & (V >= 0) & (ex(U + V) <= aden) & (T > 0)
        # t = (T / s^3) / (|den| / s^2); numerator and denominator are exact in float64, the double's quotient is correctly rounded
        # and rounding that to float32 is innocuous (53 >= 2 * 24 + 2): the float32 nearest to the exact quotient
        D = aden * s
        with np.errstate(divide="ignore", invalid="ignore"):
            t32 = (T.astype(np.float64) / D.astype(np.float64)).astype(np.float32)
        ok = (r[:, 3] <= r[:, 7]) & np.any(r[:, 4:7] != 0, axis=1)
        hit &= ok[:, None] & (r[:, 3:4] <= t32) & (t32 <= r[:, 7:8])
        tt = np.where(hit, t32, np.float32(np.inf))
        best = tt.min(1)
        found = np.isfinite(best)
        at_best = hit & (tt == best[:, None])
        gid = np.argmax(at_best, axis=1)                                                 # the first: the lowest id
        rows = np.arange(m)
        num, dn = T[rows, gid], D[rows, gid]
        same = at_best & (T * dn[:, None] == num[:, None] * D)                           # the same exact quotient as the winner's
        g = np.gcd(num, dn)
        g[g == 0] = 1
        sl = slice(lo, lo + m)
        out["gid"][sl] = np.where(found, gid, INV)
        out["t"][sl] = np.where(found, best, np.float32(-1.0))
        out["num"][sl], out["den"][sl] = np.where(found, num // g, 0), np.where(found, dn // g, 1)
        out["ties"][sl] = np.where(found, at_best.sum(1), 0)
        out["mask"][sl] = ex.fits & tri_ok.fits[0] & (same.sum(1) == at_best.sum(1))
    return out


def exact_any(rays, verts, tris):
    """occlusion: does the rule find any triangle in [tmin, tmax]?  -> (bool[n], mask)"""
    e = exact_closest(rays, verts, tris)
    return e["gid"] != INV, e["mask"]


# ---- the rays -------------------------------------------------------------------------------------------------------------------
def _rays(o, d, tmin=0.0, tmax=np.inf):
    o = np.asarray(o, np.float64).reshape(-1, 3)
    r = np.zeros((o.shape[0], 8), np.float32)
    r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7] = o, d, tmin, tmax
    assert np.array_equal(r[:, 0:3], o)
    return r


def _pick(rng, a, cap):
    return a if cap is None or a.shape[0] <= cap else a[np.sort(rng.choice(a.shape[0], cap, replace=False))]


def lattice_rays(n, seed, verts, tris, cap=None):
    """The ray families over terraces(n, seed) = (verts, tris), at most `cap` rays (a seeded choice) of each direction and kind:
      THROUGH  +-z through every vertex, edge midpoint and cell centre (one ring of lattice points outside the field too: misses);
               +-x and +-y at every lattice height on every lattice line: they lie in plateau planes (a coplanar triangle has
               den = 0 and is no hit) and meet slopes along shared edges and walls head-on;
               the diagonals (1, 1, 0), (1, 0, -1), (0, 1, 1) and their negatives through the mesh's vertices and lattice points
               above and below them;
      SURFACE  origins ON the surface (vertices, plateau points), every direction: t = 0 is no hit;
      RANGE    for rays of the above whose exact t is a float32: tmax = t and nextafter(t, 0), tmin = t and nextafter(t, inf).
    -> (rays float32 (m, 8), family int[m] index into DIRECTIONS, kind int[m])"""
    rng = np.random.default_rng(seed + 2)
    half = n // 2
    g = np.arange(-2 * (half + 1), 2 * (half + 1) + 1) * (SPACING / 2)           # every half step: vertices, midpoints, centres
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    line = np.arange(-half - 1, half + 2) * SPACING
    level = np.arange(-4, 5) * HEIGHT_STEP
    far = half * SPACING + 2.0
    v = np.asarray(verts, np.float64)
    targets = np.concatenate([v, v + (0, 0, HEIGHT_STEP), v - (0, 0, 2 * HEIGHT_STEP)])
    p = v[np.asarray(tris).astype(np.int64)]
    level_edge = p[:, 0, 2] == p[:, 1, 2]
    start = np.concatenate([v, 0.5 * (p[level_edge, 0] + p[level_edge, 1])])      # vertices and midpoints of level edges
    out, fam, kind = [], [], []

    def add(r, f, k):
        out.append(r), fam.append(np.full(r.shape[0], f)), kind.append(np.full(r.shape[0], k))

    for f, d in enumerate(DIRECTIONS):
        dv = np.array(d, np.float64)
        if d[0] == 0 and d[1] == 0:
            o = np.c_[xy, np.full(xy.shape[0], -4.0 * d[2])]
        elif d[2] == 0 and d[1] == 0:
            a, b = np.meshgrid(line, level, indexing="ij")
            o = np.c_[np.full(a.size, -far * d[0]), a.ravel(), b.ravel()]
        elif d[2] == 0 and d[0] == 0:
            a, b = np.meshgrid(line, level, indexing="ij")
            o = np.c_[a.ravel(), np.full(a.size, -far * d[1]), b.ravel()]
        else:
            o = targets - (2 * far) * dv
        add(_rays(_pick(rng, o, cap), dv), f, THROUGH)
        add(_rays(_pick(rng, start, None if cap is None else max(1, cap // 4)), dv), f, SURFACE)
    rays, fam, kind = np.concatenate(out), np.concatenate(fam), np.concatenate(kind)
    e = exact_closest(rays, verts, tris)
    dyadic = np.nonzero((e["gid"] != INV) & e["mask"] & (e["den"] & (e["den"] - 1) == 0) & (e["num"] < (1 << 24)))[0]
    dyadic = _pick(rng, dyadic, None if cap is None else 2 * cap)
    t = e["t"][dyadic]
    assert np.array_equal(t.astype(np.float64) * e["den"][dyadic], e["num"][dyadic])
    edge = []
    for col, val in ((7, t), (7, np.nextafter(t, np.float32(0))), (3, t), (3, np.nextafter(t, np.float32(np.inf)))):
        r = rays[dyadic].copy()
        r[:, col] = val
        edge.append(r)
    rays = np.concatenate([rays] + edge)
    fam = np.concatenate([fam] + [fam[dyadic]] * 4)
    kind = np.concatenate([kind] + [np.full(dyadic.shape[0], RANGE)] * 4)
    return rays, fam, kind


def split_scene(verts, tris, parts, seed):
    """the scene's triangles dealt into `parts` geometries by a seeded choice (every geometry keeps all vertices; a triangle's
    neighbours land in other geometries) -> [(verts, tris of part k)], and the global order: part by part"""
    which = np.random.default_rng(seed + 3).integers(0, parts, tris.shape[0])
    return [(verts, np.ascontiguousarray(tris[which == k])) for k in range(parts)]


# ---- the frame: a raster that holds exact axes ----------------------------------------------------------------------------------
ELEVATIONS = (-90.0, -45.0, 0.0, 45.0, 90.0)
H_COLUMNS = 360
DIAG = np.float32(0.70710677)


def frame_tables():
    """factor tables of a sensor of 5 channels at -90, -45, 0, 45, 90 degrees of elevation and 360 columns at 1 degree: sine and
    cosine in float32, the channels and the columns at 0, 45, ..., 315 degrees overwritten with exact 0, +-1 and +-0.70710677 (the
    float32 nearest to sqrt(1/2): within 1e-6 degrees of the angle) -> (sin_theta, cos_theta, elevation_deg, sin_phi, cos_phi)"""
    z, o, g = np.float32(0), np.float32(1), DIAG
    st, ct = np.float32([z, g, o, g, z]), np.float32([-o, -g, z, g, o])
    phi = (np.arange(H_COLUMNS, dtype=np.float64) * np.pi / 180.0).astype(np.float32)
    sp, cp = np.sin(phi).astype(np.float32), np.cos(phi).astype(np.float32)
    sp[::45] = (z, g, o, g, z, -g, -o, -g)
    cp[::45] = (o, g, z, -g, -o, -g, z, g)
    return st, ct, np.float32(ELEVATIONS), sp, cp


def frame_dirs(tabs):
    """(st cp, st sp, ct) in float32, channel-major: as the oracle and the kernels form a ray's direction"""
    st, ct, _, sp, cp = tabs
    d = np.zeros((st.shape[0], sp.shape[0], 3), np.float32)
    d[:, :, 0], d[:, :, 1], d[:, :, 2] = st[:, None] * cp[None, :], st[:, None] * sp[None, :], ct[:, None]
    return d.reshape(-1, 3)


def sensor_position(n, seed):
    """a lattice point above the centre vertex of the lowest plateau, at the height of the highest plateau: the 0-degree ring runs in
    that plateau's plane and in the faces of the boxes around it, the +-90-degree channels go straight through a vertex"""
    h = heights(n, seed)
    flat = [(int(h[i, j]), i, j) for i in range(0, n, BLOCK) for j in range(0, n, BLOCK) if np.ptp(h[i:i + BLOCK, j:j + BLOCK]) == 0]
    low, i, j = min(flat)
    top = max(level for level, _, _ in flat if level < h.max())          # something stands above it: the ring meets slopes and walls
    assert top > low
    return np.array([(i + BLOCK // 2 - n // 2) * SPACING, (j + BLOCK // 2 - n // 2) * SPACING, top * HEIGHT_STEP])
