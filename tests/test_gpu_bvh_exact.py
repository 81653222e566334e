"""The BVH build on the MI355X, bit for bit against tests/bvh_reference.py: k_morton + the stable sort (the record order), k_leaves_tree
(records, leaf boxes, the aligned-range tree), k_hierarchy (the tie-break by index of equal keys, the 512-key LDS window, the far
nodes' cooperative searches and range boxes, the tail guard of the store through LDS), k_refit_nodes (the old topology, every box
recomputed, its own far path from 1280 leaves on) and k_widen (all 128 bytes of every four-wide twin) -- on scenes whose Morton
keys are crafted (tied keys in runs of every length around the window and the workgroup edges) rather than ben.stl's, at every
leaf size.  No tolerance anywhere: references, leaf ranges and boxes are compared as bytes."""
import numpy as np
import pytest

import bvh_reference as B
from conftest import make_tracer

pytestmark = pytest.mark.gpu

LEAF_SIZES = (1, 2, 4, 8)
SCENES = [f"one_key_{n}" for n in B.ONE_KEY_SIZES] + ["runs", "two_halves", "random", "tiny_1", "tiny_2", "tiny_3", "staircase_deck"]
_scenes = {}


def _scene(name):
    """the crafted scenes: made once, never changed"""
    if not _scenes:
        _scenes.update(B.build_scenes())
        for v, t, k in _scenes.values():
            for a in (v, t, k):
                a.setflags(write=False)
    return _scenes[name]


def _words(nodes):
    return np.ascontiguousarray(nodes).view(np.uint32).reshape(nodes.shape[0], nodes.dtype.itemsize // 4)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_nodes(got, want, what):
    assert got.shape[0] == want.shape[0], what
    bad = np.nonzero(np.any(_words(got) != _words(want), axis=1))[0]
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:2]], want[bad[:2]])


def _assert_classic_records(tri, rec, what):
    assert np.array_equal(tri["gid"], rec["gid"]), what
    for f in ("v0", "e1", "e2"):
        assert np.array_equal(_bits(tri[f]), _bits(rec[f])), (what, f)


def _assert_mesh_records(got, rec, what):
    assert np.array_equal(got["gid"], rec["gid"]), what
    for f in ("v0", "v1", "v2"):
        assert np.array_equal(_bits(got[f]), _bits(rec[f])), (what, f)
    assert not got["pad0"].any() and not got["pad1"].any(), what


def _classic(capi, sensors, g):
    tr = make_tracer(capi, sensors["0000"], "bvh")
    tr.setOption(capi.LS_OPT_BVH_INSTANCED, 0)
    tr.setOption(capi.LS_OPT_LEAF_SIZE, g)
    return tr


def _assert_trace_is_the_brute_force(tr, frame=0):
    rc, _, _ = tr.traceScene(frame)
    assert rc == 0
    t, gid = tr.denseHits()
    bt, bg = tr.bruteForce()
    assert np.array_equal(gid, bg) and np.array_equal(_bits(t), _bits(bt))
    return gid


def test_the_scenes_cover_ragged_leaves_and_both_sides_of_the_store_tiles():
    """the premises of the cases below, from the scenes alone: at every leaf size above 1 a one_key scene and `runs` end in a ragged
    leaf, and the node count L - 1 falls on both sides of multiples of 64 (a wave's store through LDS) and 256 (a workgroup)"""
    counts = {n: _scene(n)[1].shape[0] for n in SCENES}
    for g in LEAF_SIZES[1:]:
        assert counts["runs"] % g != 0 and any(counts[f"one_key_{n}"] % g != 0 for n in B.ONE_KEY_SIZES)
    nodes = {(-(-c // g)) - 1 for c in counts.values() for g in LEAF_SIZES}
    for tile in (64, 256):
        assert {tile - 1, 0, 1} <= {n % tile for n in nodes if n >= tile - 1}, tile


@pytest.mark.parametrize("name", SCENES)
def test_classic_build_equals_the_reference(capi, sensors, name):
    verts, tris, _ = _scene(name)
    for g in LEAF_SIZES:
        tr = _classic(capi, sensors, g)
        assert tr.addGeometry("m", verts.shape[0], tris.shape[0]) == 0
        tr.updateGeometry("m", capi.IDENTITY_AFFINE, verts, tris)
        assert tr.commitScene() == 0 and tr.info(capi.LS_INFO_BVH_INSTANCED) == 0
        sv, st = tr.downloadScene()
        assert np.array_equal(st, tris)
        nodes, tri, leaf = tr.downloadBvh()
        assert leaf == g
        want, rec, _, _ = B.build(sv, st, g)
        _assert_classic_records(tri, rec, (name, g))
        _assert_nodes(nodes, want, (name, g))
        _assert_trace_is_the_brute_force(tr)
        assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
        tr.close()


def _moved(verts, seed):
    """every triangle of the soup at the place of a randomly chosen OTHER one: its old key is wrong"""
    n = verts.shape[0] // 3
    src = (np.arange(n) + np.random.default_rng(seed).integers(1, n, n)) % n
    return np.ascontiguousarray(verts.reshape(n, 3, 3)[src].reshape(-1, 3))


@pytest.mark.parametrize("g", [1, 4])
@pytest.mark.parametrize("name", ["one_key_1281", "runs", "random"])
def test_classic_refit_keeps_the_topology_and_recomputes_every_box(capi, sensors, name, g):
    verts, tris, _ = _scene(name)
    tr = _classic(capi, sensors, g)
    assert tr.addGeometry("m", verts.shape[0], tris.shape[0]) == 0
    tr.updateGeometry("m", capi.IDENTITY_AFFINE, verts, tris)
    assert tr.commitScene() == 0 and tr.info(capi.LS_INFO_LAST_COMMIT_REFIT) == 0
    sv, st = tr.downloadScene()
    built, _, order, _ = B.build(sv, st, g)
    _assert_nodes(tr.downloadBvh()[0], built, (name, g, "build"))
    if g == 1 or name == "runs":                                             # k_refit_nodes' far path has a node to work on
        assert int((built["r"] - built["l"]).max()) >= 1280
    # new vertices, the same indices: a refit
    moved = _moved(verts, 5)
    tr.updateGeometry("m", capi.IDENTITY_AFFINE, moved, None)
    assert tr.commitScene() == 0 and tr.info(capi.LS_INFO_LAST_COMMIT_REFIT) == 1
    sv2, st2 = tr.downloadScene()
    assert np.array_equal(st2, tris) and not np.array_equal(sv2, sv)
    if name != "one_key_1281":                                               # (there the moved keys are still all but one the same)
        assert not np.array_equal(np.argsort(B.morton_keys(sv2, st2), kind="stable"), order)  # a build would have come out otherwise
    want, rec = B.refit(built, order, sv2, st2, g)
    nodes, tri, _ = tr.downloadBvh()
    _assert_classic_records(tri, rec, (name, g, "refit"))
    _assert_nodes(nodes, want, (name, g, "refit"))
    _assert_trace_is_the_brute_force(tr, 1)
    # new indices: a build
    flipped = np.ascontiguousarray(tris[::-1])
    tr.updateGeometry("m", capi.IDENTITY_AFFINE, moved, flipped)
    assert tr.commitScene() == 0 and tr.info(capi.LS_INFO_LAST_COMMIT_REFIT) == 0
    sv3, st3 = tr.downloadScene()
    assert np.array_equal(st3, flipped)
    want, rec, _, _ = B.build(sv3, st3, g)
    nodes, tri, _ = tr.downloadBvh()
    _assert_classic_records(tri, rec, (name, g, "rebuild"))
    _assert_nodes(nodes, want, (name, g, "rebuild"))
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


def _pose(oracle):
    """a 30 degree turn about z and a translation of (1, -2, 0)"""
    return oracle.affine_from_components(np.float32([1.0, -2.0, 0.0]), np.float32([0.0, 0.0, np.pi / 6]))


def _assert_instanced(tr, name, verts, tris, g, want, rec, what):
    nodes, wide, got, leaf = tr.downloadHierarchy(name)
    assert leaf == g
    _assert_mesh_records(got, rec, what)
    _assert_nodes(nodes, want, what)
    twins = B.wide_reference(nodes.view(B.NODE_DTYPE))
    assert wide.shape[0] == nodes.shape[0]
    bad = np.nonzero(np.any(_words(wide) != _words(twins), axis=1))[0]
    assert bad.size == 0, (what, "wide", bad.size, bad[:8])


@pytest.mark.parametrize("name", SCENES)
def test_instanced_hierarchy_and_its_four_wide_twins_equal_the_reference(oracle, capi, sensors, name):
    """the default engine's per-geometry hierarchy (mesh space: the reference runs over the vertices as uploaded, whatever the pose)
    through ls_debug_download_hierarchy, and k_widen's output against wide_reference of the downloaded binary nodes; then a
    vertex-only update: the old topology, new boxes, new twins"""
    verts, tris, keys = _scene(name)
    for g in (1, 4):
        tr = make_tracer(capi, sensors["0000"], "bvh")
        tr.setOption(capi.LS_OPT_LEAF_SIZE, g)
        assert tr.addGeometry("m", verts.shape[0], tris.shape[0]) == 0
        tr.updateGeometry("m", _pose(oracle), verts, tris)
        assert tr.commitScene() == 0 and tr.info(capi.LS_INFO_BVH_INSTANCED) == 2      # instanced, and this commit built
        with pytest.raises(capi.LidarShooterHipError):
            tr.downloadBvh()                                                  # the classic view has nothing to show
        assert np.array_equal(B.morton_keys(verts, tris), keys)              # mesh space: the keys the scene was made for
        built, rec, order, _ = B.build(verts, tris, g)
        _assert_instanced(tr, "m", verts, tris, g, built, rec, (name, g, "build"))
        _assert_trace_is_the_brute_force(tr)
        if tris.shape[0] > 1:
            moved = _moved(verts, 9)
            tr.updateGeometry("m", _pose(oracle), moved, None)
            assert tr.commitScene() == 0 and tr.info(capi.LS_INFO_BVH_INSTANCED) == 2
            want, rec2 = B.refit(built, order, moved, tris, g)
            _assert_instanced(tr, "m", moved, tris, g, want, rec2, (name, g, "vertex update"))
            _assert_trace_is_the_brute_force(tr, 1)
        assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
        tr.close()


def test_download_hierarchy_refusals(oracle, capi, sensors):
    import ctypes as C
    verts, tris, _ = _scene("one_key_3")
    tr = _classic(capi, sensors, 1)
    assert tr.addGeometry("m", verts.shape[0], tris.shape[0]) == 0
    tr.updateGeometry("m", capi.IDENTITY_AFFINE, verts, tris)
    assert tr.commitScene() == 0
    L, g = C.c_uint32(), C.c_uint32()
    NOT_COMMITTED, UNKNOWN_GEOMETRY = -8, -3
    assert tr.L.ls_debug_download_hierarchy(tr.h, 0, C.byref(L), C.byref(g), None, None, None) == NOT_COMMITTED     # a classic commit
    tr.setOption(capi.LS_OPT_BVH_INSTANCED, 1)
    tr.setOption(capi.LS_OPT_BVH_WIDE, 0)
    tr.updateGeometry("m", capi.IDENTITY_AFFINE, verts, tris)
    assert tr.commitScene() == 0
    assert tr.L.ls_debug_download_hierarchy(tr.h, 0, C.byref(L), C.byref(g), None, None, None) == 0 and (L.value, g.value) == (4, 1)
    assert tr.L.ls_debug_download_hierarchy(tr.h, 5, C.byref(L), C.byref(g), None, None, None) == UNKNOWN_GEOMETRY
    wide = np.zeros(3, capi.WIDE_DTYPE)
    assert tr.L.ls_debug_download_hierarchy(tr.h, 0, None, None, None, wide.ctypes.data, None) == NOT_COMMITTED     # no twins were made
    nodes, none, rec, leaf = tr.downloadHierarchy("m", wide=False)
    assert none is None and nodes.shape[0] == 3 and rec.shape[0] == 4 and leaf == 1
    tr.close()
