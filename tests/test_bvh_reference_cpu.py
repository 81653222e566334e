"""tests/bvh_reference.py checked against itself (no GPU, no library): the crafted scenes have the Morton keys they were made for,
the reference topology is Karras' numbering of a partition (against an O(n^2) recursive restatement of the definition), the walks'
scene is as deep as its premise says, a four-wide node has two to four live slots."""
import numpy as np
import pytest

import bvh_reference as B

_scenes = {}


def _all_scenes():
    if not _scenes:
        _scenes.update(B.build_scenes())
        for v, t, k in _scenes.values():
            for a in (v, t, k):
                a.setflags(write=False)
    return _scenes


def test_dtypes_are_the_library_views(capi):
    assert B.NODE_DTYPE.itemsize == capi.NODE_DTYPE.itemsize == 64 and B.WIDE_DTYPE.itemsize == capi.WIDE_DTYPE.itemsize == 128
    assert [B.NODE_DTYPE.fields[n][1] for n in B.NODE_DTYPE.names] == [capi.NODE_DTYPE.fields[n][1] for n in capi.NODE_DTYPE.names]
    assert B.LEAF_BIT == capi.LEAF_BIT and capi.MESH_TRI_DTYPE.itemsize == capi.TRI_DTYPE.itemsize == 48


def test_every_scene_has_the_keys_it_was_made_for():
    for name, (v, t, want) in _all_scenes().items():
        assert np.abs(v).max() == 512 and not np.any(v == 0), name
        assert np.array_equal(B.morton_keys(v, t), want), name
    assert B.interleave(*B.deinterleave(0x5A5A5A5)) == 0x5A5A5A5 and B.interleave(1, 0, 0) == 4 and B.interleave(0, 0, 1) == 1
    v, t, k = _all_scenes()["runs"]
    assert 5900 <= t.shape[0] <= 6100 and not np.all(np.diff(k.astype(np.int64)) >= 0)      # the sort matters
    assert sorted(set(np.bincount(np.unique(k[:-1], return_inverse=True)[1]).tolist())) == sorted(B.RUN_LENGTHS)


def _definition(aug, i, l, r, out):
    """the radix tree straight from its definition, a linear scan per node and recursive on the children: node i over [l, r]"""
    bit = max(b for b in range(64) if (aug[l] >> b) != (aug[r] >> b))
    clear = [j for j in range(l, r + 1) if not (aug[j] >> bit) & 1]
    gamma = clear[-1]
    assert clear == list(range(l, gamma + 1)) and gamma < r             # sorted: the clear ones come first
    assert i not in out
    out[i] = (l, r, gamma)
    if l != gamma:
        _definition(aug, gamma, l, gamma, out)
    if r != gamma + 1:
        _definition(aug, gamma + 1, gamma + 1, r, out)


def _check_against_definition(leaf_keys):
    L = len(leaf_keys)
    left, right, lo, hi = B.topology(leaf_keys)
    assert left.shape[0] == max(L - 1, 0)
    if L < 2:
        return
    want = {}
    _definition([(int(k) << 32) | j for j, k in enumerate(leaf_keys)], 0, 0, L - 1, want)
    assert sorted(want) == list(range(L - 1))                           # Karras' numbering uses every index once
    for i, (l, r, gamma) in want.items():
        assert i in (l, r) and (int(lo[i]), int(hi[i])) == (l, r)
        assert int(left[i]) == ((B.LEAF_BIT | gamma) if l == gamma else gamma)
        assert int(right[i]) == ((B.LEAF_BIT | (gamma + 1)) if r == gamma + 1 else gamma + 1)


@pytest.mark.parametrize("name", ["tiny_1", "tiny_2", "tiny_3", "one_key_257", "random_300"])
def test_reference_topology_is_the_definition(name):
    if name == "random_300":
        v, t, _ = B.random_keys(300, seed=5)
    else:
        v, t, _ = _all_scenes()[name]
    for g in (1, 2, 4, 8):
        keys = np.sort(B.morton_keys(v, t), kind="stable")[::g]
        _check_against_definition(keys)
    _check_against_definition(np.array([5, 5, 5, 6, 6, 9, 9, 9, 9, 1 << 29], np.uint32))


def test_reference_tree_is_a_partition_with_exact_boxes():
    v, t, _ = _all_scenes()["runs"]
    for g in (1, 4):
        nodes, rec, order, _ = B.build(v, t, g)
        nt = t.shape[0]
        L = (nt + g - 1) // g
        assert nodes.shape[0] == L - 1 and sorted(rec["gid"].tolist()) == list(range(nt))
        seen, stack = [], [0]
        while stack:
            ref = stack.pop()
            if ref & B.LEAF_BIT:
                seen.append(ref & ~B.LEAF_BIT)
                continue
            nd = nodes[ref]
            for side, child in (("l", int(nd["left"])), ("r", int(nd["right"]))):
                if not child & B.LEAF_BIT:       # a child box is the union of the grandchildren's, bit for bit
                    c = nodes[child]
                    assert np.array_equal(np.minimum(c["llo"], c["rlo"]), nd[side + "lo"]) and np.array_equal(np.maximum(c["lhi"], c["rhi"]), nd[side + "hi"])
            stack.append(int(nd["right"]))
            stack.append(int(nd["left"]))
        assert seen == list(range(L))


def test_staircase_deck_is_38_deep():
    v, t, _ = _all_scenes()["staircase_deck"]
    nodes, _, _, _ = B.build(v, t, 1)
    assert t.shape[0] == 4121 and nodes.shape[0] == 4120 and B.depth(nodes) == 38
    assert len(B.path_to_first_leaf(nodes)) == 37
    # leaf size 2: two stairs share a leaf and the deck has 2048 leaves -- 1 + 12 + 11 levels of nodes: the same scene BELOW the
    # 32-entry boundary
    assert B.depth(B.build(v, t, 2)[0]) == 25


def test_wide_reference_has_two_to_four_live_slots():
    for name in ("runs", "staircase_deck", "tiny_3", "one_key_2"):
        v, t, _ = _all_scenes()[name]
        nodes = B.build(v, t, 2 if name == "runs" else 1)[0]
        wide = B.wide_reference(nodes)
        refs = wide["lo"].view(np.uint32)[:, :, 3]
        live = (refs != B.INVALID).sum(1)
        assert wide.shape[0] == nodes.shape[0] and np.all(live >= 2) and np.all(live <= 4)
        assert set(live.tolist()) <= {2, 3, 4} and np.all(wide["hi"].view(np.uint32)[:, :, 3] == 0)
        # slots 1 and 3 are live exactly where the child is a node
        assert np.array_equal(refs[:, 1] != B.INVALID, (nodes["left"] & B.LEAF_BIT) == 0)
        assert np.array_equal(refs[:, 3] != B.INVALID, (nodes["right"] & B.LEAF_BIT) == 0)
        dead = refs == B.INVALID
        assert np.all(np.isposinf(wide["lo"][:, :, :3][dead])) and np.all(np.isneginf(wide["hi"][:, :, :3][dead]))
