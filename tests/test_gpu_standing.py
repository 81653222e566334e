"""Standing lists (csrc/ls_standing.h, k_standing_build / k_project_standing; the policy in ls_commit.cpp, the routing in
ls_trace.cpp): a geometry that has not changed for a few commits is traced from a kept list of its triangles with a footprint.
A frame traced from a list must be the frame traced from the mesh, byte for byte: points, hit records and count are compared
with the CPU oracle's frame (and so with each other) before a list exists, once it is in use and with LS_OPT_STANDING = 0.
The raster is small (16 channels x 256 columns at the XT-32's pose), so the oracle takes milliseconds; the shapes are the
smallest at which the kernels can go wrong: list lengths around the records a wave takes (32), several workgroups with a
partial last wave, every kind of footprint, a full queue, more lists than a launch takes, a shard."""
import hashlib

import numpy as np
import pytest

import cull_reference as cr
from conftest import make_tracer
from lidarshooter_amd import synth

pytestmark = pytest.mark.gpu

PER_WAVE = 32          # ls_standing.h: kStandingPerWave
SETTLE = 8             # commits within which an unchanged geometry must be standing: 2 to wait, 1 to build, 1 to see it done
BREAK_EVEN = 72        # ls_internal.h: kStandingBreakEven
GRAPH_WAIT = 64        # ls_internal.h: kStandingGraphWait


def _sensor(oracle, sensors, V=16, H=256, t=None):
    b = sensors["0000"]
    return oracle.Sensor(uid="standing", vertical=synth.syn_vertical(V), h_begin=np.float32(0.0), h_end=np.float32(360.0), h_count=H,
                         R=b.R, Rinv=b.Rinv, t=b.t if t is None else np.asarray(t, np.float32))


def _to_world(s, tri_sensor):
    R = s.R.reshape(3, 3).astype(np.float64)
    return (np.asarray(tri_sensor, np.float64).reshape(-1, 3) @ R.T + s.t.astype(np.float64)).astype(np.float32)


def _elev_dir(chi_deg, phi_deg):
    th, ph = np.radians(90.0 - chi_deg), np.radians(phi_deg)
    return np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])


def _small_tri(d, r, w):
    """a triangle of size w around the point r * d, across the direction d"""
    side = np.cross(d, [0.0, 0.0, 1.0]); side /= np.linalg.norm(side)
    up = np.cross(side, d)
    c = r * d
    return [c + w * up, c - 0.5 * w * up + 0.87 * w * side, c - 0.5 * w * up - 0.87 * w * side]


def _on_rays(oracle, s, n_hit, n_miss, seed=1):
    """n_hit triangles a sixth of a degree across, each around its own ray of the raster (one cell each: rings are 2.7 degrees
    apart, columns 1.4), and n_miss of the same size half way between two rings or above the top one: no footprint at all
    -> (verts, tris), the hit ones first"""
    rng = np.random.default_rng(seed)
    dirs = oracle.ray_dirs(s).astype(np.float64)
    cells = np.array([(v, h) for v in range(s.V) for h in range(1, s.H - 1)])
    pick = cells[rng.permutation(len(cells))[:n_hit] if n_hit <= len(cells) else rng.integers(0, len(cells), n_hit)]
    tri = []
    for v, h in pick:
        r = float(rng.uniform(5.0, 40.0))
        tri += _small_tri(dirs[v * s.H + h], r, 0.003 * r)
    chi = np.sort(s.vertical.astype(np.float64))
    for k in range(n_miss):
        e = chi[-1] + 1.3 if k % 5 == 0 else 0.5 * (chi[k % (s.V - 1)] + chi[k % (s.V - 1) + 1])
        r = float(rng.uniform(5.0, 40.0))
        tri += _small_tri(_elev_dir(e, float(rng.uniform(0.0, 360.0))), r, 0.003 * r)
    v = _to_world(s, tri)
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)


class Scene:
    """a tracer on the projection engine and what the oracle needs to trace the same scene"""

    def __init__(self, oracle, capi, s, geoms, cull=False, pipeline=0, graph=False, shard=None):
        self.o, self.capi, self.s, self.shard = oracle, capi, s, shard
        self.geoms = {}
        self.tr = make_tracer(capi, s, "projection")
        if cull:
            self.tr.setOption(capi.LS_OPT_BLOCK_CULL, 1)
            self.tr.forceGroupCull(True)
        if pipeline:
            self.tr.setOption(capi.LS_OPT_PIPELINE, pipeline)
        if graph:
            self.tr.setOption(capi.LS_OPT_FRAME_GRAPH, 1)
        for name, v, e, A in geoms:
            self.add(name, v, e, A)
        if shard is not None:
            self.tr.setShard(*shard)
        self.k = 0

    def add(self, name, v, e, A):
        e = np.asarray(e, np.uint32)
        self.tr.addGeometry(name, v.shape[0], e.shape[0], self.capi.LS_GEOMETRY_TYPE_QUAD if e.shape[1] == 4 else self.capi.LS_GEOMETRY_TYPE_TRIANGLE)
        self.tr.updateGeometry(name, A, v, e)
        self.geoms[name] = [v, e, np.asarray(A, np.float32)]

    def info(self, what):
        return self.tr.info(getattr(self.capi, "LS_INFO_STANDING_" + what))

    def ref(self):
        return self.o.trace_frame(self.s, [(self.tr.getGeometryId(n), v, e, A) for n, (v, e, A) in self.geoms.items()])

    def frame(self, ref, commit=True):
        """one commit and one frame, which must be the oracle's `ref`; -> its bytes"""
        if commit:
            assert self.tr.commitScene() == 0
        rc, pts, hits = self.tr.traceScene(self.k)
        self.k += 1
        assert rc == 0
        if self.shard is None:
            got = np.stack([hits["ray"], hits["geom"], hits["prim"], hits["t"].view(np.uint32)], axis=1)
            assert len(pts) == len(ref["points"]) and np.array_equal(got, ref["hits"]) and np.array_equal(pts, ref["points"])
        else:   # a shard's rays: the dense view against the oracle's columns
            cols = cr.shard_columns(self.s.H, self.shard)
            tt, gid = self.tr.denseHits()
            want = ref["gid"].reshape(self.s.V, self.s.H)[:, cols].reshape(-1)
            if any(e.shape[1] == 4 for _, e, _ in self.geoms.values()):
                want = np.where(want == self.o.INVALID, want, want & ~np.uint32(1))
            assert np.array_equal(gid, want)
            assert np.array_equal(tt.view(np.uint32), ref["t"].reshape(self.s.V, self.s.H)[:, cols].reshape(-1).view(np.uint32))
            assert len(pts) == int((want != self.o.INVALID).sum())
        return pts.tobytes(), hits.tobytes()

    def settle(self, ref, want, commits=SETTLE):
        """unchanged commits and frames until `want` geometries are traced from their lists -> the frames' bytes"""
        out = []
        for _ in range(commits):
            out.append(self.frame(ref))
            if self.info("GEOMETRIES") == want:
                return out
        raise AssertionError(f"{self.info('GEOMETRIES')} geometries standing after {commits} commits, expected {want}")

    def serve(self, ref, n=BREAK_EVEN):
        """n more frames from the lists: a drop after them puts the policy's wait back to its first value"""
        for _ in range(n):
            self.frame(ref)

    def close(self):
        self.tr.close()


def _before_after_off(sc, ref, want=1, records=None):
    """the three kinds of frame every case compares: before a list is usable, from the list, LS_OPT_STANDING = 0"""
    frames = sc.settle(ref, want)
    assert len(frames) >= 3                                   # (the first frames were traced from the mesh)
    if records is not None:
        assert sc.info("RECORDS") == records
    frames.append(sc.frame(ref))
    assert sc.info("GEOMETRIES") == want
    sc.tr.setOption(sc.capi.LS_OPT_STANDING, 0)
    frames.append(sc.frame(ref))
    assert sc.info("GEOMETRIES") == 0 and sc.info("RECORDS") == 0
    sc.tr.setOption(sc.capi.LS_OPT_STANDING, 1)
    frames.append(sc.frame(ref))
    assert sc.info("GEOMETRIES") == want                     # (the list was still good)
    assert all(f == frames[0] for f in frames)


# ---- 1. list lengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, PER_WAVE - 1, PER_WAVE, PER_WAVE + 1, 3001])
def test_list_lengths(oracle, capi, sensors, n):
    """n records exactly: n one-cell triangles on rays among 40 (n = 0: 400) that fall between two rings or above the top one.
    3001: 24 workgroups, the last one with two waves, the last wave with 25 records"""
    s = _sensor(oracle, sensors)
    v, e = _on_rays(oracle, s, n, 400 if n == 0 else 40, seed=n)
    sc = Scene(oracle, capi, s, [("m", v, e, oracle.IDENTITY_AFFINE)])
    ref = sc.ref()
    assert int((ref["gid"] != oracle.INVALID).sum()) >= n    # (every triangle on a ray is hit; column 0 and H - 1 coincide)
    _before_after_off(sc, ref, 1, records=n)
    assert sc.info("BUILDS") == 1
    sc.close()


# ---- 2. footprint kinds ------------------------------------------------------------------------------------------------------
def _kinds(oracle, s):
    """in the sensor frame: a triangle across the raster's seam (azimuth 0 = 360: two column intervals), one the vertical axis
    pierces (full circle, 256 columns: above big_cells, queued), a wall over ten rings (nch > 1, queued), tall narrow ones (nch >
    1, expanded in the wave), and small ones on rays"""
    tri = [[[20.0, -1.5, -3.0], [20.0, 1.5, -3.0], [20.0, 0.0, 2.0]],
           [[9.0, 0.5, -2.2], [-5.0, 8.0, -2.2], [-4.0, -8.5, -2.2]],
           [[-12.0, -9.0, -5.0], [-12.0, 9.0, -5.0], [-12.0, 0.0, 3.0]]]
    for k in range(12):
        d = _elev_dir(-5.0, 30.0 * k + 11.0)
        side = np.cross(d, [0.0, 0.0, 1.0])
        tri.append([10.0 * d + [0, 0, 1.2], 10.0 * d - [0, 0, 1.2] + 0.1 * side, 10.0 * d - [0, 0, 1.2] - 0.1 * side])
    v = _to_world(s, tri)
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("cull", [False, True])
def test_footprint_kinds_in_one_scene(oracle, capi, sensors, cull):
    """every kind of footprint, a quad geometry and (cull) every geometry with culling data -- its list is built from the Morton-
    ordered mesh and names the caller's triangles through perm -- but routed standing: no k_cull work for it"""
    s = _sensor(oracle, sensors)
    kv, ke = _kinds(oracle, s)
    gv, gt = synth.grid_mesh(12, 6, half=14.0, seed=5)
    gv = gv + np.asarray([0.0, 0.0, -1.5], np.float32) + s.t
    nx = 13
    quads = np.array([[j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i] for j in range(6) for i in range(12)], np.uint32)
    rv, re_ = _on_rays(oracle, s, 70, 30, seed=9)
    A = np.asarray(oracle.IDENTITY_AFFINE, np.float32).copy()
    A[3] = 0.25                                               # (a full transform: xform 1)
    sc = Scene(oracle, capi, s, [("kinds", kv, ke, oracle.IDENTITY_AFFINE), ("quads", gv, quads, A), ("rays", rv, re_, oracle.IDENTITY_AFFINE)],
               cull=cull)
    ref = sc.ref()
    if cull:   # the lists are built from geometries that carry culling data: perm names the caller's triangle of every sorted one
        assert sc.tr.commitScene() == 0
        for name, (v, e, A) in sc.geoms.items():
            perm = sc.tr.downloadCull(name)[0]
            n_tris = e.shape[0] * (2 if e.shape[1] == 4 else 1)
            assert perm.shape[0] == n_tris and np.array_equal(np.sort(perm), np.arange(n_tris))
    assert int((ref["gid"] != oracle.INVALID).sum()) > 400
    won = np.unique(ref["hits"][:, 1])
    assert set(won.tolist()) == {0, 1, 2}                     # every geometry is seen
    _before_after_off(sc, ref, 3)
    assert sc.info("BUILDS") == 3
    sc.close()


def test_a_scene_that_overfills_the_queue(oracle, capi, sensors):
    """3 600 triangles of hundreds of cells each: the list's frame queues 2 048 of them and expands the rest in its waves, as the
    mesh's frame does (shown by that frame's counted tests)"""
    s = _sensor(oracle, sensors)
    rng = np.random.default_rng(3600)
    n = 3600
    c = rng.normal(0.0, 1.0, size=(n, 1, 3))
    c[:, :, 2] *= 0.2
    dist = rng.uniform(8.0, 30.0, size=(n, 1, 1))
    c = c / np.linalg.norm(c, axis=2, keepdims=True) * dist
    v = _to_world(s, c + rng.normal(0.0, 1.0, size=(n, 3, 3)) * (0.4 * dist))   # ~45 degrees across: most of the 16 rings x 30 columns
    e = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    sc = Scene(oracle, capi, s, [("m", v, e, oracle.IDENTITY_AFFINE)])
    ref = sc.ref()
    _before_after_off(sc, ref, 1)
    assert sc.info("RECORDS") > 2048 + 256
    sc.tr.setOption(capi.LS_OPT_COUNT_VISITS, 1)              # (a counted frame is traced from the mesh)
    sc.frame(ref)
    assert sc.info("GEOMETRIES") == 0
    assert sc.tr.visitStats()[1] > 128 * 2048                 # the queue was full: every entry has more than 128 cells
    sc.close()


# ---- 3. invalidation ---------------------------------------------------------------------------------------------------------
def _pose(dx, dy=0.0, yaw=0.0):
    c, s_ = np.cos(yaw), np.sin(yaw)
    return np.array([c, -s_, 0, dx, s_, c, 0, dy, 0, 0, 1, 0], np.float32)


def test_invalidation(oracle, capi, sensors, meshes):
    """every change of what a record depends on makes the very NEXT frame the oracle's for the new state, and the geometries it
    concerns leave their lists; restating a pose changes nothing"""
    import torch
    s = _sensor(oracle, sensors)
    gv, ge = meshes["ground"]
    bv, be = meshes["ben"]
    sc = Scene(oracle, capi, s, [])
    sc.tr.addGeometry("front", 3 * 40, 40)                    # an id in front of the others, no data yet: not in the scene
    sc.add("ground", gv, ge, oracle.IDENTITY_AFFINE)
    sc.add("ben", bv, be, oracle.IDENTITY_AFFINE)
    hv, he = _on_rays(oracle, s, 50, 10, seed=3)
    d_v, d_e = torch.from_numpy(hv).cuda(), torch.from_numpy(he.astype(np.int32)).cuda()
    sc.tr.addGeometry("handed", hv.shape[0], he.shape[0])
    sc.tr.updateGeometryDeviceShared("handed", oracle.IDENTITY_AFFINE, d_v.data_ptr(), 12, d_e.data_ptr())
    sc.geoms["handed"] = [hv, he, np.asarray(oracle.IDENTITY_AFFINE, np.float32)]
    torch.cuda.synchronize()

    def standing_again(n):
        ref = sc.ref()
        sc.settle(ref, n)
        sc.serve(ref)
        return ref

    ref = standing_again(3)
    # the same pose restated: nothing is invalidated
    sc.tr.updateGeometryTransform("ben", oracle.IDENTITY_AFFINE)
    sc.frame(ref)
    assert sc.info("GEOMETRIES") == 3 and sc.info("BUILDS") == 3
    # a new pose
    sc.geoms["ben"][2] = _pose(0.4, -0.3, 0.2)
    sc.tr.updateGeometryTransform("ben", sc.geoms["ben"][2])
    sc.frame(sc.ref())
    assert sc.info("GEOMETRIES") == 2
    standing_again(3)
    # a vertex upload
    sc.geoms["ground"][0] = gv + np.asarray([0.0, 0.0, 0.07], np.float32)
    sc.tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, sc.geoms["ground"][0], None)
    sc.frame(sc.ref())
    assert sc.info("GEOMETRIES") == 2
    standing_again(3)
    # the same pointers handed over again with other contents
    hv2 = hv.copy()
    hv2[: 3 * 25] += np.asarray([0.0, 0.0, 0.5], np.float32)  # (half of its triangles leave their rays)
    d_v.copy_(torch.from_numpy(hv2))
    torch.cuda.synchronize()
    sc.geoms["handed"][0] = hv2
    sc.tr.updateGeometryDeviceShared("handed", oracle.IDENTITY_AFFINE, d_v.data_ptr(), 12, d_e.data_ptr())
    sc.frame(sc.ref())
    assert sc.info("GEOMETRIES") == 2
    standing_again(3)
    # an index upload (the triangles in another order: other primitive ids)
    sc.geoms["ground"][1] = np.ascontiguousarray(ge[::-1])
    sc.tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, sc.geoms["ground"][0], sc.geoms["ground"][1])
    sc.frame(sc.ref())
    assert sc.info("GEOMETRIES") == 2
    standing_again(3)
    # the sensor at a new pose
    s2 = _sensor(oracle, sensors, t=s.t + np.asarray([0.3, -0.2, 0.1], np.float32))
    sc.tr.setSensor(s2.vertical, s2.h_begin, s2.h_end, s2.h_count, s2.Rinv, s2.t)
    sc.s = s2
    sc.frame(sc.ref())
    assert sc.info("GEOMETRIES") == 0
    standing_again(3)
    # a shard, and the full turn again
    sc.tr.setShard(16, 96)
    sc.shard = (16, 96)
    sc.frame(sc.ref())
    assert sc.info("GEOMETRIES") == 0
    standing_again(3)
    sc.tr.setShard(0, s.H)
    sc.shard = None
    sc.frame(sc.ref())
    assert sc.info("GEOMETRIES") == 0
    standing_again(3)
    # a geometry enters the scene in front of the others: their global triangle ids move
    fv, fe = _on_rays(oracle, s2, 30, 10, seed=4)
    sc.tr.updateGeometry("front", oracle.IDENTITY_AFFINE, fv, fe)
    sc.geoms = {"front": [fv, fe, np.asarray(oracle.IDENTITY_AFFINE, np.float32)], **sc.geoms}
    sc.frame(sc.ref())
    assert sc.info("GEOMETRIES") == 0
    standing_again(4)
    # ... and is removed (the removal commits)
    assert sc.tr.removeGeometry("front") == 0
    del sc.geoms["front"]
    sc.frame(sc.ref(), commit=False)
    assert sc.info("GEOMETRIES") == 0
    standing_again(3)
    sc.close()


# ---- 4. mixed scenes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline,graph", [(0, False), (2, False), (2, True)])
def test_ground_standing_while_ben_moves(oracle, capi, sensors, meshes, pipeline, graph):
    s = _sensor(oracle, sensors)
    sc = Scene(oracle, capi, s, [("ground", *meshes["ground"], oracle.IDENTITY_AFFINE), ("ben", *meshes["ben"], oracle.IDENTITY_AFFINE)],
               pipeline=pipeline, graph=graph)
    poses = [_pose(0.0), _pose(0.5, 0.2, 0.3), _pose(-0.4, 0.6, -0.5)]
    refs = []
    for A in poses:
        sc.geoms["ben"][2] = A
        refs.append(sc.ref())
    # under frame graphs a list joins the captured launch sequence only once its geometry has stood for GRAPH_WAIT commits (the
    # three graphs are captured anew for it); the graphs are captured at the first three frames, before any list exists
    bound = SETTLE + (GRAPH_WAIT if graph else 0)
    seen = []
    for k in range(bound + 6):
        sc.geoms["ben"][2] = poses[k % 3]
        sc.tr.updateGeometryTransform("ben", poses[k % 3])
        sc.frame(refs[k % 3])
        seen.append(sc.info("GEOMETRIES"))
    assert seen[0] == 0 and seen[-1] == 1 and 1 in seen[:bound] and seen == sorted(seen)
    assert sc.info("BUILDS") == 1                             # the ground's: ben never stands for two commits
    if graph:
        assert 1 not in seen[:GRAPH_WAIT]
        assert sc.tr.info(capi.LS_INFO_FRAME_GRAPH_STATE) == 1 and sc.tr.info(capi.LS_INFO_FRAME_GRAPH_CAPTURES) == 6
    sc.close()


def test_seventeen_geometries_take_two_launches(oracle, capi, sensors):
    s = _sensor(oracle, sensors)
    geoms = [(f"g{k:02d}", *_on_rays(oracle, s, 20 + 3 * k, 5, seed=100 + k), oracle.IDENTITY_AFFINE) for k in range(17)]
    sc = Scene(oracle, capi, s, geoms)
    _before_after_off(sc, sc.ref(), 17, records=sum(20 + 3 * k for k in range(17)))
    sc.close()


def test_a_shard_narrower_than_half_a_turn(oracle, capi, sensors, meshes):
    s = _sensor(oracle, sensors)
    sc = Scene(oracle, capi, s, [("ground", *meshes["ground"], oracle.IDENTITY_AFFINE), ("ben", *meshes["ben"], _pose(0.3, 0.1, 0.4))],
               shard=(40, 72))
    _before_after_off(sc, sc.ref(), 2)
    full = Scene(oracle, capi, s, [("ground", *meshes["ground"], oracle.IDENTITY_AFFINE), ("ben", *meshes["ben"], _pose(0.3, 0.1, 0.4))])
    full.settle(full.ref(), 2)
    assert sc.info("RECORDS") < full.info("RECORDS")          # the sector test left triangles out of the shard's lists
    full.close()
    sc.close()


# ---- 5. back-off -------------------------------------------------------------------------------------------------------------
def test_a_geometry_that_moves_every_third_commit(oracle, capi, sensors, meshes):
    """two unchanged commits get the first build (wait = 2); it is dropped at the next commit having served nothing, which doubles
    the wait to 4 -- more unchanged commits in a row than this geometry ever has: one build in 60 commits"""
    s = _sensor(oracle, sensors)
    sc = Scene(oracle, capi, s, [("ben", *meshes["ben"], oracle.IDENTITY_AFFINE)])
    poses = [_pose(0.0), _pose(0.3, 0.3, 0.1)]
    refs = []
    for A in poses:
        sc.geoms["ben"][2] = A
        refs.append(sc.ref())
    for k in range(60):
        p = (k // 3) % 2
        sc.tr.updateGeometryTransform("ben", poses[p])
        sc.frame(refs[p])
    assert sc.info("BUILDS") <= 1
    sc.close()


def test_a_mesh_above_the_capacity(oracle, capi, sensors):
    """5 000 triangles, every one with a footprint: more than the 4 096 records the list has room for.  The one build that finds
    that out is the only one; no frame is ever traced from the list"""
    s = _sensor(oracle, sensors)
    v, e = _on_rays(oracle, s, 5000, 0, seed=7)
    sc = Scene(oracle, capi, s, [("m", v, e, oracle.IDENTITY_AFFINE)])
    ref = sc.ref()
    for _ in range(12):
        sc.frame(ref)
        assert sc.info("GEOMETRIES") == 0
    assert sc.info("BUILDS") == 1
    sc.close()


# ---- 6. the headline ---------------------------------------------------------------------------------------------------------
def test_headline_cloud_from_the_list(oracle, capi, sensors):
    """SYN-128 x SYN-1M, one frame traced from the ground's list: the cloud every round has produced"""
    s = _sensor(oracle, sensors, V=128, H=4096)
    v, t = synth.syn_1m()
    tr = make_tracer(capi, s)
    tr.addGeometry("ground", v.shape[0], t.shape[0])
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, v, t)
    for k in range(SETTLE):
        assert tr.commitScene() == 0
        rc, pts, hits = tr.traceScene(k)
        if tr.info(capi.LS_INFO_STANDING_GEOMETRIES) == 1:
            break
    assert tr.info(capi.LS_INFO_STANDING_GEOMETRIES) == 1 and 100000 < tr.info(capi.LS_INFO_STANDING_RECORDS) <= 250000
    assert len(pts) == 256482
    assert hashlib.sha256(np.ascontiguousarray(pts).tobytes()).hexdigest().startswith("5eeb1f64")
    tr.close()
