"""A plain restatement of the BVH build (csrc/ls_kernels.hip: k_morton, the stable sort, k_leaves_tree, k_hierarchy, k_refit_nodes,
k_widen) in numpy, from the DEFINITION of the radix tree rather than from Karras' searches, and the crafted scenes that reach what
ben.stl does not: tied Morton keys (the tie-break by index), runs of ties across the 512-key LDS window and the 256-node workgroup
edges, nodes whose range leaves the window (the cooperative far path), the tail of the store through LDS, walks deeper than the
32-entry LDS stack.  No GPU, no library: tests/test_bvh_reference_cpu.py checks this file against itself, tests/test_gpu_bvh_exact.py
and tests/test_gpu_stack_spill.py check the device against it.

Everything is float32 where the kernels are, and every comparison made with it is bit for bit.

The scenes: the Morton key of a triangle is the cell of its bounding box's centre on a grid of 512 / maxabs cells per unit.  Every
scene but `tiny` holds the ANCHOR triangle with a corner at (-512, -512, -512) and no coordinate beyond 512 in magnitude, so the cell
size is 1 and a triangle whose box is centred on (qx + .5, qy + .5, qz + .5) has the key that interleaves qx, qy, qz.  No coordinate
is +-0 (min and max are unambiguous in bits)."""
import numpy as np

LEAF_BIT = 0x80000000
INVALID = 0xFFFFFFFF
# include/lidarshooter_hip_debug.h: the node's two spare words are its leaf range
NODE_DTYPE = np.dtype([("llo", "<f4", 3), ("left", "<u4"), ("lhi", "<f4", 3), ("right", "<u4"),
                       ("rlo", "<f4", 3), ("l", "<u4"), ("rhi", "<f4", 3), ("r", "<u4")])
WIDE_DTYPE = np.dtype([("lo", "<f4", (4, 4)), ("hi", "<f4", (4, 4))])
SIGN_X, SIGN_Y, SIGN_Z = 1 << 29, 1 << 28, 1 << 27
ANCHOR = np.array([(-512.0, -512.0, -512.0), (-511.5, -512.0, -512.0), (-512.0, -511.5, -512.0)], np.float32)
ANCHOR_KEY = SIGN_X | SIGN_Y | SIGN_Z | ((1 << 27) - 1)
f32 = np.float32


# ---- keys -----------------------------------------------------------------------------------------------------------------------
def interleave(qx, qy, qz):
    """magnitude bits: x at 3i + 2, y at 3i + 1, z at 3i"""
    k = 0
    for i in range(9):
        k |= ((int(qx) >> i) & 1) << (3 * i + 2) | ((int(qy) >> i) & 1) << (3 * i + 1) | ((int(qz) >> i) & 1) << (3 * i)
    return k


def deinterleave(K):
    qx = qy = qz = 0
    for i in range(9):
        qx |= ((K >> (3 * i + 2)) & 1) << i
        qy |= ((K >> (3 * i + 1)) & 1) << i
        qz |= ((K >> (3 * i)) & 1) << i
    return qx, qy, qz


def morton_keys(verts, tris):
    """k_morton: per axis c = 0.5f * (min + max), q = min(511, uint32(|c| * scale)), scale = 512.0f / maxabs (0 for maxabs 0)"""
    v = np.ascontiguousarray(verts, np.float32)
    p = v[np.ascontiguousarray(tris).astype(np.int64)]                  # (n, 3 corners, 3 axes)
    maxabs = np.abs(v).max() if v.size else f32(0)
    scale = f32(512.0) / f32(maxabs) if maxabs > 0 else f32(0)
    c = f32(0.5) * (p.min(1) + p.max(1))
    assert c.dtype == np.float32
    q = np.minimum(511, (np.abs(c) * scale).astype(np.float32).astype(np.uint32)).astype(np.uint32)
    keys = np.zeros(p.shape[0], np.uint32)
    for a in range(3):
        e = np.zeros(p.shape[0], np.uint32)
        for i in range(9):
            e |= ((q[:, a] >> np.uint32(i)) & np.uint32(1)) << np.uint32(3 * i)
        keys |= e << np.uint32(2 - a)
        keys |= (c[:, a] < 0).astype(np.uint32) << np.uint32(29 - a)
    return keys


# ---- the build ------------------------------------------------------------------------------------------------------------------
def topology(leaf_keys):
    """The radix tree over the leaf keys, each extended by its index ((key << 32) | j): node [l, r] splits at the highest bit in which
    the extended keys of l and r differ, gamma = the last leaf of [l, r] with that bit clear; the root is node 0 over [0, L - 1], the
    left child is leaf gamma when l == gamma, else node gamma, the right child leaf gamma + 1 when r == gamma + 1, else node gamma + 1.
    -> (left, right, l, r) uint32[L - 1]"""
    L = len(leaf_keys)
    aug = (np.asarray(leaf_keys, np.uint64) << np.uint64(32)) | np.arange(L, dtype=np.uint64)
    assert np.all(aug[1:] > aug[:-1]), "leaf keys must ascend"
    n = max(L - 1, 0)
    left, right, lo, hi = (np.zeros(n, np.uint32) for _ in range(4))
    seen = np.zeros(n, bool)
    stack = [(0, 0, L - 1)] if L > 1 else []
    while stack:
        i, l, r = stack.pop()
        assert not seen[i]
        seen[i] = True
        bit = (int(aug[l]) ^ int(aug[r])).bit_length() - 1
        first_set = (int(aug[r]) >> bit) << bit                         # the common prefix, that bit set, zeros below
        gamma = int(np.searchsorted(aug, np.uint64(first_set), "left")) - 1
        assert l <= gamma < r
        lo[i], hi[i] = l, r
        left[i] = (LEAF_BIT | gamma) if l == gamma else gamma
        right[i] = (LEAF_BIT | (gamma + 1)) if r == gamma + 1 else gamma + 1
        if l != gamma:
            stack.append((gamma, l, gamma))
        if r != gamma + 1:
            stack.append((gamma + 1, gamma + 1, r))
    assert seen.all()
    return left, right, lo, hi


def triangle_boxes(p):
    """(n, 3, 3) corners -> lo, hi float32 (n, 3): min and max per axis widened by pad = m * 2^-16, m the largest |coordinate|"""
    p = np.ascontiguousarray(p, np.float32)
    pad = (np.abs(p).reshape(p.shape[0], 9).max(1) * f32(2.0 ** -16)).astype(np.float32)[:, None]
    lo, hi = p.min(1) - pad, p.max(1) + pad
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    return lo, hi


def boxes_over(order, verts, tris, g, left, right, lo, hi):
    """nodes (NODE_DTYPE) of a given topology over the triangles in `order`: leaf k = sorted positions [k g, min(k g + g, ntris))"""
    p = np.ascontiguousarray(verts, np.float32)[np.ascontiguousarray(tris).astype(np.int64)[order]]
    tlo, thi = triangle_boxes(p)
    nt = len(order)
    L = (nt + g - 1) // g
    starts = np.arange(L) * g
    llo, lhi = np.minimum.reduceat(tlo, starts, axis=0), np.maximum.reduceat(thi, starts, axis=0)
    nodes = np.zeros(max(L - 1, 0), NODE_DTYPE)
    nodes["left"], nodes["right"], nodes["l"], nodes["r"] = left, right, lo, hi
    for i in range(nodes.shape[0]):
        l, r = int(lo[i]), int(hi[i])
        gamma = int(left[i]) & ~LEAF_BIT
        nodes["llo"][i], nodes["lhi"][i] = llo[l:gamma + 1].min(0), lhi[l:gamma + 1].max(0)
        nodes["rlo"][i], nodes["rhi"][i] = llo[gamma + 1:r + 1].min(0), lhi[gamma + 1:r + 1].max(0)
    return nodes


def records_over(order, verts, tris):
    """-> dict gid uint32[n], v0, v1, v2, e1 = v0 - v1, e2 = v2 - v0 float32 (n, 3), in sorted order"""
    p = np.ascontiguousarray(verts, np.float32)[np.ascontiguousarray(tris).astype(np.int64)[order]]
    v0, v1, v2 = p[:, 0], p[:, 1], p[:, 2]
    return dict(gid=np.asarray(order, np.uint32), v0=v0, v1=v1, v2=v2, e1=v0 - v1, e2=v2 - v0)


def build(verts, tris, g):
    """-> (nodes NODE_DTYPE[L - 1], records dict, order, leaf keys)"""
    keys = morton_keys(verts, tris)
    order = np.argsort(keys, kind="stable")
    leaf_keys = keys[order][::g]
    topo = topology(leaf_keys)
    return boxes_over(order, verts, tris, g, *topo), records_over(order, verts, tris), order, leaf_keys


def refit(nodes, order, verts, tris, g):
    """k_refit_nodes: the old topology and order, boxes and records from the new vertices"""
    return boxes_over(order, verts, tris, g, nodes["left"], nodes["right"], nodes["l"], nodes["r"]), records_over(order, verts, tris)


def wide_reference(nodes):
    """k_widen: for every binary node i its 128-byte twin.  Slots 0, 1 = the left child's two children (the child itself with its box
    in slot 0 when it is a leaf), slots 2, 3 the same for the right child; slot c: lo.w = reference, hi.w = 0; an empty slot is
    (+inf, +inf, +inf, 0xFFFFFFFF) / (-inf, -inf, -inf, 0)"""
    n = nodes.shape[0]
    out = np.zeros(n, WIDE_DTYPE)
    lo, hi = out["lo"].view(np.uint32), out["hi"].view(np.uint32)       # (n, 4 slots, 4 words)
    inf, ninf = np.array([np.inf], np.float32).view(np.uint32)[0], np.array([-np.inf], np.float32).view(np.uint32)[0]
    lo[:, :, :3], lo[:, :, 3], hi[:, :, :3], hi[:, :, 3] = inf, INVALID, ninf, 0
    u = lambda a: np.ascontiguousarray(a).view(np.uint32)              # noqa: E731
    for i in range(n):
        nd = nodes[i]
        for side, (ref, blo, bhi) in enumerate(((int(nd["left"]), nd["llo"], nd["lhi"]), (int(nd["right"]), nd["rlo"], nd["rhi"]))):
            s = 2 * side
            if ref & LEAF_BIT:
                lo[i, s, :3], lo[i, s, 3], hi[i, s, :3] = u(blo), ref, u(bhi)
            else:
                c = nodes[ref]
                lo[i, s, :3], lo[i, s, 3], hi[i, s, :3] = u(c["llo"]), c["left"], u(c["lhi"])
                lo[i, s + 1, :3], lo[i, s + 1, 3], hi[i, s + 1, :3] = u(c["rlo"]), c["right"], u(c["rhi"])
    return out


def depth(nodes):
    """references on the longest path from the root to a leaf, both counted (a one-leaf scene: 1)"""
    if nodes.shape[0] == 0:
        return 1
    best, stack = 0, [(0, 1)]
    while stack:
        ref, d = stack.pop()
        if ref & LEAF_BIT:
            best = max(best, d)
            continue
        stack.append((int(nodes["left"][ref]), d + 1))
        stack.append((int(nodes["right"][ref]), d + 1))
    return best


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
def tri_for_key(K, z=None):
    """An isosceles triangle in a plane z = const whose bounding box is centred on the cell of key K (30 bits: three sign bits, 27
    interleaved magnitude bits): centre (cx, cy) = +-(qx + .5, qy + .5), half-width w = 2 |cx| + |cy| + 64 -- for the small keys of
    the walks' scenes every ray within 2 degrees of +z then meets the triangle at least 24 units inside its edges --, corners
    (cx - w, cy - w), (cx + w, cy - w), (cx, cy + w); z = +-(qz + .5) unless given.  Where that half-width would carry a corner past
    512 (keys of the upper cells) it is cut to 511.75 - max(|cx|, |cy|): the box keeps its centre, the scene its extent of 512."""
    qx, qy, qz = deinterleave(K & ((1 << 27) - 1))
    cx, cy, cz = qx + 0.5, qy + 0.5, qz + 0.5
    w = min(2 * cx + cy + 64, 511.75 - max(cx, cy))
    if K & SIGN_X: cx = -cx
    if K & SIGN_Y: cy = -cy
    if K & SIGN_Z: cz = -cz
    if z is None:
        z = cz
    return np.array([(cx - w, cy - w, z), (cx + w, cy - w, z), (cx, cy + w, z)], np.float32)


def _scene(tri_list, keys):
    """-> (verts float32 (3n, 3), tris uint32 (n, 3), intended keys uint32 (n,)): a triangle soup"""
    v = np.ascontiguousarray(np.concatenate(tri_list), np.float32)
    assert not np.any(v == 0) and np.abs(v).max() <= 512
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3), np.asarray(keys, np.uint32)


ONE_KEY_SIZES = (1, 2, 3, 255, 256, 257, 1279, 1280, 1281, 2049, 5000)
ONE_KEY = interleave(3, 5, 6)


def one_key(n):
    """n triangles in one cell, then the anchor"""
    return _scene([tri_for_key(ONE_KEY)] * n + [ANCHOR], [ONE_KEY] * n + [ANCHOR_KEY])


RUN_LENGTHS = (1, 2, 3, 7, 64, 255, 256, 257, 511, 512, 513, 768, 1024, 1300)


def runs():
    """5 998 triangles in runs of equal keys (every length of RUN_LENGTHS, the short ones again), the runs in a shuffled order of
    ascending keys -- they cross the 256-node workgroup edges and the +-512 window at many offsets --, the input order shuffled, the
    anchor last: 5 999 triangles"""
    rng = np.random.default_rng(20240607)
    lengths = np.array(RUN_LENGTHS + (1, 2, 3, 7, 64, 255, 64, 64, 64, 1))
    rng.shuffle(lengths)
    keys = np.sort(rng.choice(1 << 27, size=len(lengths), replace=False)) | (rng.integers(0, 8, len(lengths)) << 27)
    per_tri = np.repeat(keys, lengths)
    rng.shuffle(per_tri)
    return _scene([tri_for_key(int(k)) for k in per_tri] + [ANCHOR], list(per_tri) + [ANCHOR_KEY])


def two_halves():
    """1500 triangles of key A, then 1500 of A ^ 1, then the anchor"""
    A = interleave(200, 77, 310)
    assert not A & 1
    return _scene([tri_for_key(A)] * 1500 + [tri_for_key(A ^ 1)] * 1500 + [ANCHOR], [A] * 1500 + [A ^ 1] * 1500 + [ANCHOR_KEY])


def random_keys(n=3000, seed=11):
    """n random 27-bit keys with random sign bits (all eight octants), then the anchor"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 1 << 27, n) | (rng.integers(0, 8, n) << 27)
    assert len(set((keys >> 27).tolist())) == 8
    return _scene([tri_for_key(int(k)) for k in keys] + [ANCHOR], list(keys) + [ANCHOR_KEY])


def tiny(n):
    """1, 2 or 3 triangles without the anchor (one leaf: no node at all): each has a corner at x = -512, its box centred on
    (-511.5, qy + .5, qz + .5); the second repeats the first one's cell"""
    cells = [(7, 3), (7, 3), (2, 9)][:n]
    t = [np.array([(-512.0, qy, qz + 0.5), (-511.0, qy, qz + 0.5), (-512.0, qy + 1.0, qz + 0.5)], np.float32) for qy, qz in cells]
    return _scene(t, [SIGN_X | interleave(511, qy, qz) for qy, qz in cells])


DECK, STAIRS = 4096, 24


def staircase_deck():
    """A deck of 4096 triangles of key 0 at z = 0.25 + (k // 2) 2^-15 (pairs share their plane, so a ray meets both at the same t and
    the lower id must win), one triangle per key 1 << j, j = 0 .. 23, at z = 0.6 + 0.01 j (its own cell's z where bit j is a z bit),
    the anchor: 4121 triangles.  The radix tree peels the anchor and the 24 stairs off one level at a time before it reaches the
    deck's 12 levels of ties: depth 38, and a ray up the z axis enters every box on the way down."""
    t = [tri_for_key(0, z=0.25 + (k // 2) * 2.0 ** -15) for k in range(DECK)]
    t += [tri_for_key(1 << j, z=None if j % 3 == 0 else 0.6 + 0.01 * j) for j in range(STAIRS)]
    return _scene(t + [ANCHOR], [0] * DECK + [1 << j for j in range(STAIRS)] + [ANCHOR_KEY])


def build_scenes():
    """name -> (verts, tris, intended keys) of every scene the build is pinned on"""
    s = {f"one_key_{n}": one_key(n) for n in ONE_KEY_SIZES}
    s.update(runs=runs(), two_halves=two_halves(), random=random_keys(), staircase_deck=staircase_deck())
    s.update({f"tiny_{n}": tiny(n) for n in (1, 2, 3)})
    return s


# ---- rays against the reference tree --------------------------------------------------------------------------------------------
def path_to_first_leaf(nodes):
    """the left spine: [(node, side)] from the root down to leaf 0, and the right siblings along it"""
    path, ref = [], 0
    while not ref & LEAF_BIT:
        path.append(ref)
        ref = int(nodes["left"][ref])
    return path


def wide_walk_holds(nodes, origins, dirs):
    """The four-wide walks (k_trace_inst, k_trace_rays, k_occluded_rays, k_trace_rays_moving) restated in float64 down to the first
    leaf a ray reaches: at a node every live slot whose box the ray enters is hit, the nearest hit is walked on, the others are
    pushed.  -> the number of references each ray holds when it stands at its first leaf, int[n]"""
    wide = wide_reference(nodes)
    lo, hi = wide["lo"][:, :, :3].astype(np.float64), wide["hi"][:, :, :3].astype(np.float64)
    refs = wide["lo"].view(np.uint32)[:, :, 3]
    o, d = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    o = np.broadcast_to(o, (max(o.shape[0], d.shape[0]), 3))
    d = np.broadcast_to(d, o.shape)
    out = np.zeros(o.shape[0], np.int64)
    for k in range(o.shape[0]):
        with np.errstate(divide="ignore"):
            inv = 1.0 / d[k]
        cur, stack = (0 if nodes.shape[0] else LEAF_BIT), []
        while not cur & LEAF_BIT:
            t1, t2 = (lo[cur] - o[k]) * inv, (hi[cur] - o[k]) * inv       # (4 slots, 3 axes)
            tn, tf = np.maximum(np.minimum(t1, t2).max(1), 0.0), np.maximum(t1, t2).min(1)
            hit = [c for c in range(4) if refs[cur, c] != INVALID and tn[c] <= tf[c]]
            if not hit:
                if not stack:
                    break
                cur = stack.pop()
                continue
            near = min(hit, key=lambda c: tn[c])
            stack.extend(int(refs[cur, c]) for c in hit if c != near)
            cur = int(refs[cur, near])
        out[k] = len(stack)
    return out


def rays_enter_every_box_on_the_spine(nodes, origins, dirs, skip_root_right=True):
    """float64 slab test: does every ray enter BOTH child boxes of every node on the way from the root to leaf 0 (but for the root's
    right child, the anchor's corner of the scene)? -> (bool, the number of right siblings entered = references a binary walk holds
    when it stands at leaf 0)"""
    o, d = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore"):
        inv = 1.0 / d
    ok, held = True, 0
    for k, i in enumerate(path_to_first_leaf(nodes)):
        for side in ("l", "r"):
            if k == 0 and side == "r" and skip_root_right:
                continue
            lo, hi = nodes[side + "lo"][i].astype(np.float64), nodes[side + "hi"][i].astype(np.float64)
            t1, t2 = (lo - o) * inv, (hi - o) * inv
            tn, tf = np.minimum(t1, t2).max(1), np.maximum(t1, t2).min(1)
            ok = ok and bool(np.all(np.maximum(tn, 0.0) < tf))
            held += side == "r"
    return ok, held
