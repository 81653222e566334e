"""tests/lattice_reference.py against itself and the oracle against it, without a device: the exact integer rule pinned by an O(n^2)
restatement in Python Fractions, oracle.rays_bruteforce and oracle.trace_bruteforce equal to the exact rule in id and in the bits
of t wherever every float32 intermediate is exact, the posed scenes' vertices equal to the integer transform, and the conditions
that keep the device tests from passing vacuously: most hits are ties between triangles that a seeded permutation scattered over
the ids, in every direction family."""
from fractions import Fraction

import numpy as np
import pytest

import lattice_reference as LR

N, SEED = 32, 7
SENSOR_T = np.float32([2.5, -1.25, 0.75])          # the caller-ray handle: identity R, a dyadic t
CAPS = {"identity": 300}                           # rays per direction and kind; the posed scenes take a third of that
_cache = {}


def lattice_sensor(oracle, t=SENSOR_T, uid="lattice"):
    """a descriptor sensor with identity R (its raster does not matter to caller rays): column 0 is the ordinary zero of sinf"""
    eye = np.eye(3, dtype=np.float32).reshape(9)
    return oracle.Sensor(uid=uid, vertical=np.float32([-45.0, -20.0, 0.0, 20.0, 45.0]), h_begin=np.float32(0.0), h_end=np.float32(360.0),
                         h_count=361, R=eye, Rinv=eye.copy(), t=np.asarray(t, np.float32))


def terrace_scene():
    if "scene" not in _cache:
        v, t = LR.terraces(N, SEED)
        v.setflags(write=False)
        t.setflags(write=False)
        _cache["scene"] = (v, t)
    return _cache["scene"]


def single(oracle, verts, tris):
    return oracle.Scene(np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.uint32), np.zeros(1, np.uint32),
                        np.zeros(1, np.uint32), np.zeros(1, bool))


def lattice_case(oracle, pose):
    """the terraces posed by LR.POSES[pose] in the frame of lattice_sensor, the ray families carried along, the exact answers and the
    oracle's -- computed once, shared by the CPU and the device tests, never changed -> dict"""
    if pose not in _cache:
        v, t = terrace_scene()
        s, A = lattice_sensor(oracle), LR.POSES[pose]
        base, fam, kind = LR.lattice_rays(N, SEED, v, t, CAPS.get(pose, 100))
        rays = LR.pose_rays(base, A, SENSOR_T)
        scene = oracle.assemble_scene(s, [(0, v, t, A)])
        exact_verts = LR.pose_points(v, A, SENSOR_T)
        exact = LR.exact_closest(rays, exact_verts, t)
        ot, og = oracle.rays_bruteforce(rays, scene)
        c = dict(sensor=s, A=A, verts=v, tris=t, rays=rays, family=fam, kind=kind, scene=scene, exact_verts=exact_verts, exact=exact,
                 oracle_t=ot, oracle_gid=og)
        for a in (rays, fam, kind, ot, og, *exact.values()):
            a.setflags(write=False)
        _cache[pose] = c
    return _cache[pose]


def frame_case(oracle):
    """the tables sensor of LR.frame_tables at LR.sensor_position over the terraces at the identity pose: the directions as the
    kernels form them, the oracle's dense answer -> dict"""
    if "frame" not in _cache:
        v, t = terrace_scene()
        tabs = LR.frame_tables()
        pos = LR.sensor_position(N, SEED)
        s = lattice_sensor(oracle, pos, "lattice-frame")
        dirs = LR.frame_dirs(tabs)
        scene = oracle.assemble_scene(s, [(0, v, t, LR.POSES["identity"])])
        ot, og = oracle.trace_bruteforce(dirs, scene)
        c = dict(sensor=s, tabs=tabs, pos=pos, dirs=dirs, scene=scene, oracle_t=ot, oracle_gid=og, verts=v, tris=t)
        for a in (dirs, ot, og):
            a.setflags(write=False)
        _cache["frame"] = c
    return _cache["frame"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the scene and the rays are what they say -------------------------------------------------------------------------------------

def test_terraces_are_a_lattice_scene():
    v, t = terrace_scene()
    assert t.shape[0] > 2 * N * N and t.shape[0] - 2 * N * N >= 100                      # the field and the walls
    q = v.astype(np.float64) / (LR.SPACING, LR.SPACING, LR.HEIGHT_STEP)
    assert np.array_equal(q, np.rint(q)) and np.abs(v[:, 2]).max() <= 1.0
    assert v[:, 0].min() == -v[:, 0].max() == -N * LR.SPACING / 2                        # centred: the mid-planes are vertex rows
    h = LR.heights(N, SEED)
    flat = 0                                                                             # plateaus of at least 4 x 4 cells
    for i in range(0, N, LR.BLOCK):
        for j in range(0, N, LR.BLOCK):
            flat += np.ptp(h[i:i + 5, j:j + 5]) == 0
    assert flat >= 4
    # neighbours across an edge are far apart in id: the median distance is of the order of the triangle count
    edges = {}
    for k, tri in enumerate(t.tolist()):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            edges.setdefault(frozenset((tri[a], tri[b])), []).append(k)
    gaps = [abs(e[0] - e[1]) for e in edges.values() if len(e) == 2]
    assert np.median(gaps) > t.shape[0] / 8
    v2, t2 = LR.terraces(N, SEED)
    assert np.array_equal(v, v2) and np.array_equal(t, t2)


def _fraction_closest(ray, verts, tris):
    """the rule, one ray, every triangle, in Fractions: -> (id or INV, t or None, ties)"""
    F = Fraction
    o, tmin, d, tmax = [F(float(x)) for x in ray[0:3]], float(ray[3]), [F(float(x)) for x in ray[4:7]], float(ray[7])
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]      # noqa: E731
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]                                                  # noqa: E731
    best, bid, ties = None, LR.INV, 0
    for k, tri in enumerate(tris):
        v0, v1, v2 = ([F(float(x)) for x in verts[i]] for i in tri)
        e1, e2 = [a - b for a, b in zip(v0, v1)], [a - b for a, b in zip(v2, v0)]
        Ng, C = cross(e2, e1), [a - b for a, b in zip(v0, o)]
        R, den = cross(C, d), dot(cross(e2, e1), d)
        if den == 0:
            continue
        sg = 1 if den > 0 else -1
        U, V, T = sg * dot(R, e2), sg * dot(R, e1), sg * dot(Ng, C)
        if U < 0 or V < 0 or U + V > abs(den) or T <= 0:
            continue
        t = T / abs(den)
        t32 = np.float32(float(t))                                    # (two roundings of a quotient of small integers: innocuous)
        if not (tmin <= t32 <= tmax):
            continue
        if best is None or t < best:
            best, bid, ties = t, k, 1
        elif t == best:
            ties += 1
    return bid, best, ties


def test_the_integer_rule_equals_its_restatement_in_fractions():
    v, t = LR.terraces(16, SEED)
    rays, fam, kind = LR.lattice_rays(16, SEED, v, t, 40)
    e = LR.exact_closest(rays, v, t)
    assert e["mask"].all()
    rng = np.random.default_rng(1)
    pick = np.concatenate([rng.choice(np.nonzero(kind == k)[0], 8, replace=False) for k in (LR.THROUGH, LR.SURFACE, LR.RANGE)]
                          + [np.nonzero(e["ties"] >= 4)[0][:8]])
    for r in pick:
        bid, best, ties = _fraction_closest(rays[r], v, t.tolist())
        assert bid == e["gid"][r] and ties == e["ties"][r], r
        if bid != LR.INV:
            assert best == Fraction(int(e["num"][r]), int(e["den"][r])), r
            assert np.float32(float(best)) == e["t"][r]
    assert np.count_nonzero(e["gid"][pick] != LR.INV) >= 12 and np.count_nonzero(e["gid"][pick] == LR.INV) >= 3


def test_the_mask_is_a_check_not_a_constant():
    """a far origin off the lattice of small numbers: intermediates pass 2^24, the mask says so"""
    v, t = LR.terraces(16, SEED)
    rays = np.float32([[1048576.25, 524288.5, 2097152.75, 0, -1, 0, -1, np.inf], [0.25, 0.5, 4.0, 0, 0, 0, -1, np.inf]])
    e = LR.exact_closest(rays, v, t)
    assert not e["mask"][0] and e["mask"][1] and e["gid"][1] != LR.INV


# ---- the conditions on the inputs -------------------------------------------------------------------------------------------------

def tie_shares(c):
    """-> (share of hits that tie between >= 2 triangles, between >= 4, the smallest share of >= 2 over the direction families)"""
    e = c["exact"]
    hit = e["gid"] != LR.INV
    per_family = [float((e["ties"][hit & (c["family"] == f)] >= 2).mean()) for f in range(len(LR.DIRECTIONS))]
    return float((e["ties"][hit] >= 2).mean()), float((e["ties"][hit] >= 4).mean()), min(per_family)


@pytest.mark.parametrize("pose", list(LR.POSES))
def test_the_rays_tie_and_hit_and_miss(oracle, pose):
    c = lattice_case(oracle, pose)
    e = c["exact"]
    hit = e["gid"] != LR.INV
    two, four, weakest = tie_shares(c)
    print(f"{pose}: {c['rays'].shape[0]} rays, {hit.mean():.3f} hit, ties >= 2 {two:.3f}, >= 4 {four:.3f}, weakest family {weakest:.3f}, "
          f"mask {e['mask'].mean():.4f}")
    assert two >= 0.50 and four >= 0.10 and weakest >= 0.25
    for f in range(len(LR.DIRECTIONS)):
        s = c["family"] == f
        assert np.any(hit & s) and np.any(~hit & s), LR.DIRECTIONS[f]
    for k in (LR.THROUGH, LR.SURFACE, LR.RANGE):
        s = c["kind"] == k
        assert np.any(hit & s) and np.any(~hit & s), k
    # a tie is between triangles far apart in id: the winner is not simply a neighbour in memory
    assert e["mask"].mean() >= 0.95


# ---- the oracle against the exact rule --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pose", list(LR.POSES))
def test_posed_vertices_equal_the_integer_transform(oracle, pose):
    c = lattice_case(oracle, pose)
    assert np.array_equal(c["scene"].verts.astype(np.float64), c["exact_verts"])
    assert np.array_equal(c["scene"].tris, c["tris"])


@pytest.mark.parametrize("pose", list(LR.POSES))
def test_rays_bruteforce_equals_the_exact_rule(oracle, pose):
    c = lattice_case(oracle, pose)
    e, m = c["exact"], c["exact"]["mask"]
    assert np.array_equal(c["oracle_gid"][m], e["gid"][m])
    assert np.array_equal(_bits(c["oracle_t"][m]), _bits(e["t"][m]))


def frame_exact(c):
    """the exact rule for the frame's rays whose direction has integer components (the axes: the 0-degree ring at 0, 90, 180 and 270
    degrees, every column of the +-90-degree channels) -> (ray indices, exact dict)"""
    d = c["dirs"]
    axis = np.nonzero(np.all(d == np.rint(d), axis=1))[0]
    rays = np.zeros((axis.shape[0], 8), np.float32)
    rays[:, 4:7], rays[:, 7] = d[axis] + np.float32(0), np.inf                            # (-0 + 0 = +0: the same ray)
    return axis, LR.exact_closest(rays, LR.pose_points(c["verts"], LR.POSES["identity"], c["pos"]), c["tris"])


def test_trace_bruteforce_equals_the_exact_rule_on_the_frames_axes(oracle):
    c = frame_case(oracle)
    st, ct, elev, sp, cp = c["tabs"]
    assert np.allclose(np.degrees(np.arctan2(ct.astype(np.float64), st)), elev, atol=1e-5)
    assert np.abs(np.degrees(np.arctan2(sp.astype(np.float64), cp)) % 360 - np.arange(360)).max() < 0.002      # check_tables' bound
    axis, e = frame_exact(c)
    assert axis.shape[0] == 2 * LR.H_COLUMNS + 4 and e["mask"].all()
    assert np.array_equal(c["oracle_gid"][axis], e["gid"]) and np.array_equal(_bits(c["oracle_t"][axis]), _bits(e["t"]))
    hit = c["oracle_gid"] != LR.INV
    per_channel = hit.reshape(len(LR.ELEVATIONS), LR.H_COLUMNS).sum(1)
    print("frame hits per channel", per_channel.tolist(), "ties on the axes", e["ties"].tolist()[:8])
    assert per_channel[0] == LR.H_COLUMNS and per_channel[-1] == 0                        # straight down: a vertex; straight up: nothing
    assert 0 < per_channel[2] < LR.H_COLUMNS and np.all(e["ties"][e["gid"] != LR.INV] >= 2)
    assert np.all(e["ties"][:LR.H_COLUMNS] >= 4)                                          # the vertex below the sensor


# ---- a wrong walk would be caught ---------------------------------------------------------------------------------------------------

def replay_walk(oracle, wide, rec, g, ray, rule="lowest"):
    """k_trace_rays' walk of one ray over bvh_reference's four-wide nodes, restated on the host: the slab test in float64 on boxes
    widened by the query's margin, the nearest entered slot walked on and the others pushed as they stand, a leaf's triangles through
    the oracle's test with tmin <= t <= far, far = min(best, tmax) -- and the tie rule as a parameter: "lowest" is the kernel's
    `t < best || (t == best && id < bid)`, "highest" turns its `<` round, "first" drops the clause.  (The equality in
    `tn <= tf * 1.0000003f` cannot be told from `<` this way: the boxes' padding and the margin keep tn below the t of a triangle
    inside the box.)  -> (id or INV, t)"""
    import ctypes
    f32p = ctypes.POINTER(ctypes.c_float)
    L = oracle.lib()
    o, d, tmin, tmax = ray[0:3].astype(np.float64), ray[4:7].astype(np.float64), np.float32(ray[3]), np.float32(ray[7])
    inv = np.where(d != 0, 1.0 / np.where(d != 0, d, 1.0), 1e30)
    eps = 4e-6 * 3.0 * float(np.abs(wide["hi"][:, :, :3][np.isfinite(wide["hi"][:, :, :3])]).max()) + 8e-6 * float(np.abs(o).max())
    refs = wide["lo"].view(np.uint32)[:, :, 3]
    lo, hi = wide["lo"][:, :, :3].astype(np.float64), wide["hi"][:, :, :3].astype(np.float64)
    nt = rec["gid"].shape[0]
    best, bid, far = np.float32(np.inf), LR.INV, tmax
    o32, d32, tt = np.ascontiguousarray(ray[0:3], np.float32), np.ascontiguousarray(ray[4:7], np.float32), np.zeros(1, np.float32)
    cur, stack = 0, []
    while True:
        if not cur & 0x80000000:
            with np.errstate(invalid="ignore", over="ignore"):
                x1, x2 = (lo[cur] - (o + eps)) * inv, (hi[cur] - (o - eps)) * inv                  # (4 slots, 3 axes)
                tn = np.maximum(np.minimum(x1, x2).max(1), 0.0)
                tf = np.minimum(np.maximum(x1, x2).min(1), float(far))
            ok = (tn <= tf * 1.0000003) & (refs[cur] != LR.INV)
            hit = [c for c in range(4) if ok[c]]
            if hit:
                near = min(hit, key=lambda c: (tn[c], c))
                stack.extend(int(refs[cur, c]) for c in reversed(hit) if c != near)
                cur = int(refs[cur, near])
                continue
        else:
            first = (cur & 0x7FFFFFFF) * g
            for s in range(first, min(first + g, nt)):
                v0, v1, v2 = (np.ascontiguousarray(rec[k][s], np.float32) for k in ("v0", "v1", "v2"))
                if L.lso_tri_intersect(o32.ctypes.data_as(f32p), d32.ctypes.data_as(f32p), v0.ctypes.data_as(f32p), v1.ctypes.data_as(f32p),
                                       v2.ctypes.data_as(f32p), tt.ctypes.data_as(f32p)) and tmin <= tt[0] <= far:
                    t, k = np.float32(tt[0]), int(rec["gid"][s])
                    tie = t == best and {"lowest": k < bid, "highest": k > bid, "first": False}[rule]
                    if t < best or tie:
                        best, bid, far = t, k, min(far, t)
        if not stack:
            return bid, best
        cur = stack.pop()


@pytest.mark.parametrize("g", [1, 4])
def test_a_walk_with_a_wrong_tie_rule_is_caught(oracle, g):
    """The device tests compare with the exact rule; would they notice?  The kernel's walk restated over the reference hierarchy
    (bvh_reference.build is the device's build bit for bit, test_gpu_bvh_exact) gives the exact answer on every sampled ray -- and
    with `id < bid` turned round, or the clause dropped, it names another triangle on a large share of them: the ties sit in
    different leaves and subtrees, and the traversal order does not happen to meet the lowest id first."""
    import bvh_reference as B
    c = lattice_case(oracle, "identity")
    e = c["exact"]
    mesh_rays = c["rays"].copy()
    mesh_rays[:, 0:3] += SENSOR_T                                                 # the identity pose: mesh space = sensor frame + t
    nodes, rec, _, _ = B.build(c["verts"], c["tris"], g)
    wide = B.wide_reference(nodes)
    rng = np.random.default_rng(3)
    tied = np.nonzero((e["gid"] != LR.INV) & (e["ties"] >= 2) & e["mask"])[0]
    pick = np.concatenate([rng.choice(tied, 60, replace=False), rng.choice(c["rays"].shape[0], 40, replace=False)])
    wrong = {"highest": 0, "first": 0}
    for r in pick:
        bid, t = replay_walk(oracle, wide, rec, g, mesh_rays[r])
        assert bid == e["gid"][r] and (bid == LR.INV or t == e["t"][r]), r
        for rule in wrong:
            wrong[rule] += replay_walk(oracle, wide, rec, g, mesh_rays[r], rule)[0] != e["gid"][r]
    print(f"leaf size {g}: of {pick.size} rays (60 tied) a reversed tie rule misnames {wrong['highest']}, no tie rule {wrong['first']}")
    assert wrong["highest"] >= 50 and wrong["first"] >= 15
