"""The standing base (ls_internal.h: StandingBase; ls_trace.cpp: base_for_frame, base_build, arm_keys; the `arm_to` argument of
k_pack / k_pack_wide, FinishPackArgs::base): while the set of geometries traced from their standing lists stays the same, the per-
ray minimum those lists give is kept, frames start from it and launch no k_project_standing.  Every frame here is compared byte
for byte -- points, hit records, count -- with the CPU oracle's frame for the scene as it stands: before a base exists, at the
frame that builds it, with every slot's keys armed by a copy and then by a pack, and after every change that must drop it.
The raster is 16 x 256 (16 ray blocks: k_pack with one frame in flight, k_finish_pack with three) except where the wide packs
are meant; an oracle frame is computed once per scene state and shared by the cases."""
import hashlib

import numpy as np
import pytest

import cull_reference as cr
from conftest import make_tracer
from lidarshooter_amd import synth

pytestmark = pytest.mark.gpu

SETTLE = 8               # commits within which an unchanged geometry is traced from its list (test_gpu_standing.py)
BASE_WAIT = 2            # ls_internal.h: kStandingFirstWait, the base's first wait: built at the second frame in a row with one set
BASE_BREAK_EVEN = 8      # ls_internal.h: kBaseBreakEven
LIST_BREAK_EVEN = 72     # ls_internal.h: kStandingBreakEven: a list dropped after serving this many frames is built again after 2 commits
# frames within which a base is in use once the scene stops changing: the lists within SETTLE; on the way a base may be built for a
# smaller set and dropped before it broke even, once, which doubles the wait to 4; then 4 frames with the final set
BASE_SETTLE = SETTLE + BASE_WAIT + 2 * BASE_WAIT

_REFS = {}


def _sensor(oracle, sensors, V=16, H=256, t=None):
    b = sensors["0000"]
    return oracle.Sensor(uid="standing", vertical=synth.syn_vertical(V), h_begin=np.float32(0.0), h_end=np.float32(360.0), h_count=H,
                         R=b.R, Rinv=b.Rinv, t=b.t if t is None else np.asarray(t, np.float32))


def _pose(dx, dy=0.0, yaw=0.0, dz=0.0):
    c, s_ = np.cos(yaw), np.sin(yaw)
    return np.array([c, -s_, 0, dx, s_, c, 0, dy, 0, 0, 1, dz], np.float32)


# ben.stl stands around the world's origin, 14 m from the sensor at (6.5, -12.6, 5.0); POSE_B puts it as far on the other side
POSE_A, POSE_B = _pose(0.0), _pose(13.0, -27.8)


class Scene:
    """a tracer on the projection engine and what the oracle needs to trace the same scene (the pattern of test_gpu_standing.py)"""

    def __init__(self, oracle, capi, s, geoms, pipeline=0, graph=False, shard=None):
        self.o, self.capi, self.s, self.shard = oracle, capi, s, shard
        self.geoms = {}
        self.tr = make_tracer(capi, s, "projection")
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
        self.tr.addGeometry(name, v.shape[0], e.shape[0])
        self.tr.updateGeometry(name, A, v, e)
        self.geoms[name] = [v, e, np.asarray(A, np.float32)]

    def move(self, name, A):
        self.geoms[name][2] = np.asarray(A, np.float32)
        self.tr.updateGeometryTransform(name, self.geoms[name][2])

    def info(self, what):
        return self.tr.info(getattr(self.capi, "LS_INFO_STANDING_" + what))

    def ref(self):
        """the oracle's frame of the scene as it stands (full turn), computed once per state and never changed"""
        key = (self.s.V, self.s.H, self.s.t.tobytes(),
               tuple((self.tr.getGeometryId(n), n, v.shape[0], A.tobytes()) for n, (v, e, A) in self.geoms.items()))
        if key not in _REFS:
            _REFS[key] = self.o.trace_frame(self.s, [(self.tr.getGeometryId(n), v, e, A) for n, (v, e, A) in self.geoms.items()])
        return _REFS[key]

    def frame(self, ref=None, commit=True):
        """one commit and one frame, which must be the oracle's"""
        ref = self.ref() if ref is None else ref
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
            assert np.array_equal(gid, want)
            assert np.array_equal(tt.view(np.uint32), ref["t"].reshape(self.s.V, self.s.H)[:, cols].reshape(-1).view(np.uint32))
            assert len(pts) == int((want != self.o.INVALID).sum())

    def until_base(self, bound=BASE_SETTLE, step=None):
        """frames (each the oracle's) until one starts from a base -> how many it took; step(k): the change before frame k"""
        for k in range(bound):
            if step:
                step(k)
            self.frame()
            if self.info("BASE") == 1:
                return k + 1
        raise AssertionError(f"no frame started from a base within {bound} frames")

    def serve(self, n=BASE_BREAK_EVEN):
        """n more frames from the base: a drop after them puts the base's wait back to its first value"""
        for _ in range(n):
            self.frame()
            assert self.info("BASE") == 1

    def close(self):
        self.tr.close()


def _ground_ben(oracle, capi, sensors, meshes, **kw):
    s = _sensor(oracle, sensors, **{k: kw.pop(k) for k in ("V", "H") if k in kw})
    return Scene(oracle, capi, s, [("ground", *meshes["ground"], oracle.IDENTITY_AFFINE), ("ben", *meshes["ben"], POSE_A)], **kw)


def _alternate(sc):
    """ben at POSE_A before even frames, POSE_B before odd ones"""
    return lambda k: sc.move("ben", POSE_B if (sc.k & 1) else POSE_A)


def _check_disjoint(sc):
    """the two poses' footprints share no ray, and rays ben has left show the ground (geomID 0) again"""
    sc.move("ben", POSE_A)
    a = sc.ref()["hits"]
    sc.move("ben", POSE_B)
    b = sc.ref()["hits"]
    ben = sc.tr.getGeometryId("ben")
    ra, rb = set(a[a[:, 1] == ben][:, 0].tolist()), set(b[b[:, 1] == ben][:, 0].tolist())
    assert len(ra) > 20 and len(rb) > 20 and not (ra & rb)
    assert len(ra & set(b[b[:, 1] != ben][:, 0].tolist())) > 10


# ---- 1. everything stands ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [0, 2])
def test_both_geometries_in_the_base(oracle, capi, sensors, meshes, pipeline):
    """frames before the base, the one that builds it and nine after it: with three slots (two in mode 0) each slot is armed by
    the copy once and by its own pack at least twice"""
    sc = _ground_ben(oracle, capi, sensors, meshes, pipeline=pipeline)
    n = sc.until_base(SETTLE + BASE_WAIT)                      # (both lists come into use at the same commit: no smaller set on the way)
    assert n >= 4                                             # (frames traced from the meshes and from the lists came first)
    assert sc.info("BASE_BUILDS") == 1 and sc.info("GEOMETRIES") == 2 and sc.info("RECORDS") > 100
    sc.serve(9)
    assert sc.info("BASE_BUILDS") == 1 and sc.info("GEOMETRIES") == 2
    # the same pose restated drops nothing
    sc.move("ben", POSE_A)
    sc.frame()
    assert sc.info("BASE") == 1 and sc.info("BASE_BUILDS") == 1
    sc.close()


# ---- 2. the ground stands, ben moves every frame ------------------------------------------------------------------------------
def _ground_stands_ben_alternates(sc, after=8):
    _check_disjoint(sc)
    sc.until_base(step=_alternate(sc))
    for _ in range(after):
        _alternate(sc)(0)
        sc.frame()
        assert sc.info("BASE") == 1
    assert sc.info("GEOMETRIES") == 1 and sc.info("BUILDS") == 1 and sc.info("BASE_BUILDS") == 1   # ben never got a list


@pytest.mark.parametrize("pipeline", [0, 2])
def test_ground_in_the_base_while_ben_alternates(oracle, capi, sensors, meshes, pipeline):
    sc = _ground_ben(oracle, capi, sensors, meshes, pipeline=pipeline)
    _ground_stands_ben_alternates(sc)
    sc.close()


# ---- 3. the base's geometry moves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [0, 2])
def test_the_ground_moves_under_a_base(oracle, capi, sensors, meshes, pipeline):
    """The ground stands and ben alternates, as in case 2, when the ground takes another pose.  The next four frames have no base
    to start from, whatever the waits are: the ground's list is gone for at least three commits (one to see the new key, one
    unchanged, one for the build to be seen), and a base is built at the second frame with its set at the earliest.  Every slot
    still holds the old generation and is armed to all ones again.  Then the second list, the second base."""
    sc = _ground_ben(oracle, capi, sensors, meshes, pipeline=pipeline)
    sc.until_base(step=_alternate(sc))
    for _ in range(3):
        _alternate(sc)(0)
        sc.frame()
        assert sc.info("BASE") == 1
    sc.move("ground", _pose(0.0, 0.0, 0.0, dz=-0.3))
    for _ in range(4):
        _alternate(sc)(0)
        sc.frame()
        assert sc.info("BASE") == 0
    sc.until_base(step=_alternate(sc))
    assert sc.info("BASE_BUILDS") == 2 and sc.info("GEOMETRIES") == 1 and sc.info("BUILDS") == 2
    for _ in range(4):
        _alternate(sc)(0)
        sc.frame()
        assert sc.info("BASE") == 1
    sc.close()


# ---- 4. every other change ------------------------------------------------------------------------------------------------------
def _sky(oracle, s, n=40):
    """n small triangles between 5 and 20 degrees above the top ring, all around: no footprint on the raster at all"""
    rng = np.random.default_rng(11)
    top = float(np.max(s.vertical))
    tri = []
    for _ in range(n):
        th, ph = np.radians(90.0 - (top + rng.uniform(5.0, 20.0))), np.radians(rng.uniform(0.0, 360.0))
        d = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
        side = np.cross(d, [0.0, 0.0, 1.0]); side /= np.linalg.norm(side)
        up = np.cross(side, d)
        c, w = 20.0 * d, 0.1
        tri += [c + w * up, c - 0.5 * w * up + 0.87 * w * side, c - 0.5 * w * up - 0.87 * w * side]
    R = s.R.reshape(3, 3).astype(np.float64)
    v = (np.asarray(tri, np.float64) @ R.T + s.t.astype(np.float64)).astype(np.float32)
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("pipeline", [0, 2])
def test_changes_under_a_base(oracle, capi, sensors, meshes, pipeline):
    """a geometry added, removed, the sensor moved, the shard narrowed: the very next frames are the oracle's for the new state
    (a frame that started from the old base would show the old scene), and a base comes into use again every time.  Between
    the changes lists and base serve their break-even numbers of frames, so that every change meets the first waits."""
    sc = _ground_ben(oracle, capi, sensors, meshes, pipeline=pipeline)

    def based_again(builds_more):
        before = sc.info("BASE_BUILDS")
        for _ in range(4):
            sc.frame()
        sc.until_base()
        sc.serve(LIST_BREAK_EVEN)
        assert 1 <= sc.info("BASE_BUILDS") - before <= builds_more

    sc.until_base(SETTLE + BASE_WAIT)
    sc.serve(LIST_BREAK_EVEN)
    # a third geometry (a copy of ben at the far pose): the two lists stay, the set's bits change; a base without it, then with it
    sc.add("ben2", *meshes["ben"], POSE_B)
    based_again(2)
    assert sc.info("GEOMETRIES") == 3
    assert sc.tr.removeGeometry("ben2") == 2                  # (its id; the removal commits)
    del sc.geoms["ben2"]
    sc.frame(commit=False)
    based_again(1)
    assert sc.info("GEOMETRIES") == 2
    s2 = _sensor(oracle, sensors, t=sc.s.t + np.asarray([0.3, -0.2, 0.1], np.float32))
    sc.tr.setSensor(s2.vertical, s2.h_begin, s2.h_end, s2.h_count, s2.Rinv, s2.t)
    sc.s = s2
    based_again(1)
    sc.tr.setShard(140, 96)                                   # 96 of 256 columns, ben's among them
    sc.shard = (140, 96)
    based_again(1)
    assert sc.info("GEOMETRIES") == 2
    sc.close()


# ---- 5. frames that cannot use the base -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [0, 2])
def test_frames_that_leave_the_base_alone(oracle, capi, sensors, meshes, pipeline):
    """a counted frame, a frame on the BVH engine and one with LS_OPT_STANDING = 0 start from all ones (their slot is armed
    again); the base is known by its set and serves the first default frame after them"""
    sc = _ground_ben(oracle, capi, sensors, meshes, pipeline=pipeline)
    sc.until_base(SETTLE + BASE_WAIT)
    sc.serve(4)
    sc.tr.setOption(capi.LS_OPT_COUNT_VISITS, 1)
    sc.frame()
    assert sc.info("BASE") == 0 and sc.info("GEOMETRIES") == 0
    sc.tr.setOption(capi.LS_OPT_COUNT_VISITS, 0)
    sc.tr.setOption(capi.LS_OPT_ENGINE, 1)
    sc.frame()
    assert sc.info("BASE") == 0 and sc.info("GEOMETRIES") == 0
    sc.tr.setOption(capi.LS_OPT_ENGINE, 2)
    sc.tr.setOption(capi.LS_OPT_STANDING, 0)
    sc.frame()
    assert sc.info("BASE") == 0 and sc.info("GEOMETRIES") == 0
    sc.tr.setOption(capi.LS_OPT_STANDING, 1)
    sc.until_base()
    sc.serve(6)
    assert sc.info("BASE_BUILDS") <= 2 and sc.info("GEOMETRIES") == 2
    sc.close()


# ---- 6. back-off ----------------------------------------------------------------------------------------------------------------
def test_a_geometry_that_moves_every_third_commit(oracle, capi, sensors, meshes):
    """ben moves every third commit: it never gets a usable list (test_gpu_standing.py: one build, dropped unserved, then a wait
    of 4), so the routed set is the ground alone from its list's first frame on and never changes: the rule allows ONE build"""
    sc = _ground_ben(oracle, capi, sensors, meshes)
    poses = [POSE_A, _pose(0.3, 0.3, 0.1)]
    for k in range(60):
        sc.move("ben", poses[(k // 3) % 2])
        sc.frame()
    assert sc.info("BASE") == 1 and sc.info("GEOMETRIES") == 1
    assert sc.info("BASE_BUILDS") <= 1
    sc.close()


def test_a_geometry_that_moves_every_sixth_commit(oracle, capi, sensors, meshes):
    """ben stands long enough for its list to come into use and go again, so the routed set does change: every base here is
    dropped within six frames of its build, before the 8 it takes to break even, and each such drop doubles the wait: 2, 4, 8,
    16, 32 frames with one set before the builds -- 62 frames in all, more than the 60 there are: at most 5 builds (ben's own
    list backs off too, and the ground's base then stays: three are expected)"""
    sc = _ground_ben(oracle, capi, sensors, meshes)
    poses = [POSE_A, _pose(0.3, 0.3, 0.1)]
    for k in range(60):
        sc.move("ben", poses[(k // 6) % 2])
        sc.frame()
    assert 1 <= sc.info("BASE_BUILDS") <= 5
    sc.close()


# ---- 7. the wide packs ------------------------------------------------------------------------------------------------------------
def test_wide_pack_2_full_sequence(oracle, capi, sensors, meshes):
    """128 x 1032: 516 ray blocks, k_project_finish_wide<2> + k_pack_wide<2> with three frames in flight"""
    sc = _ground_ben(oracle, capi, sensors, meshes, V=128, H=1032, pipeline=2)
    _ground_stands_ben_alternates(sc)
    assert sc.info("BASE_NO_FINISH") == 0                     # ben was projected in every frame
    sc.close()


@pytest.mark.parametrize("H", [2056, 4096])
def test_wide_pack_4_and_8(oracle, capi, sensors, meshes, H):
    """k_pack_wide<4> (1 028 blocks) and <8> (2 048): frames A, B, A, B after the base is in use"""
    sc = _ground_ben(oracle, capi, sensors, meshes, V=128, H=H, pipeline=2)
    _ground_stands_ben_alternates(sc, after=4)
    sc.close()


# ---- 8. a base of all ones ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [0, 2])
def test_a_base_of_empty_lists(oracle, capi, sensors, meshes, pipeline):
    """the only standing geometry lies wholly above the top ring: its list is empty, the base all ones"""
    s = _sensor(oracle, sensors)
    sc = Scene(oracle, capi, s, [("sky", *_sky(oracle, s), oracle.IDENTITY_AFFINE), ("ben", *meshes["ben"], POSE_A)], pipeline=pipeline)
    sc.until_base(step=_alternate(sc))
    for _ in range(6):
        _alternate(sc)(0)
        sc.frame()
        assert sc.info("BASE") == 1 and sc.info("GEOMETRIES") == 1 and sc.info("RECORDS") == 0
    assert len(sc.ref()["points"]) > 50
    sc.close()


# ---- 9. no finish launch when nothing was projected ------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline,H,V", [(0, 256, 16), (2, 1032, 128)])
def test_frames_without_a_finish_launch(oracle, capi, sensors, meshes, pipeline, H, V):
    """the two-launch path (one frame in flight; three with more than 512 ray blocks).  The ground alone, standing: once the base
    is in use nothing is left to project and the pack takes the base's own block counts.  With ben in the scene and moving, every
    frame projects it and launches the finish pass; with ben gone again, none."""
    s = _sensor(oracle, sensors, V=V, H=H)
    sc = Scene(oracle, capi, s, [("ground", *meshes["ground"], oracle.IDENTITY_AFFINE)], pipeline=pipeline)
    sc.until_base(SETTLE + BASE_WAIT)
    assert sc.info("BASE_NO_FINISH") == 1
    sc.serve(5)
    assert sc.info("BASE_NO_FINISH") == 6
    sc.add("ben", *meshes["ben"], POSE_A)
    sc.until_base(step=_alternate(sc))
    for _ in range(4):
        _alternate(sc)(0)
        sc.frame()
        assert sc.info("BASE") == 1
    assert sc.info("BASE_NO_FINISH") == 6
    assert sc.tr.removeGeometry("ben") == 1                   # (its id; the removal commits)
    del sc.geoms["ben"]
    sc.frame(commit=False)
    sc.until_base()
    skipped = sc.info("BASE_NO_FINISH")
    assert skipped >= 7
    sc.serve(4)
    assert sc.info("BASE_NO_FINISH") == skipped + 4
    sc.close()


# ---- 10. frame graphs ---------------------------------------------------------------------------------------------------------------
def test_no_base_under_frame_graphs(oracle, capi, sensors, meshes):
    sc = _ground_ben(oracle, capi, sensors, meshes, pipeline=2, graph=True)
    for _ in range(SETTLE + 2 * BASE_WAIT + 2):
        sc.frame()
        assert sc.info("BASE") == 0
    assert sc.info("BASE_BUILDS") == 0 and sc.tr.info(capi.LS_INFO_FRAME_GRAPH_STATE) == 1
    sc.close()


# ---- the headline ---------------------------------------------------------------------------------------------------------------------
def test_headline_cloud_from_the_base(oracle, capi, sensors):
    """SYN-128 x SYN-1M, a frame that started from the base (and launched nothing but its pack): the cloud every round has produced"""
    s = _sensor(oracle, sensors, V=128, H=4096)
    v, t = synth.syn_1m()
    tr = make_tracer(capi, s)
    tr.addGeometry("ground", v.shape[0], t.shape[0])
    tr.updateGeometry("ground", oracle.IDENTITY_AFFINE, v, t)
    based = 0
    for k in range(SETTLE + BASE_WAIT + 1):
        assert tr.commitScene() == 0
        rc, pts, hits = tr.traceScene(k)
        based += tr.info(capi.LS_INFO_STANDING_BASE)
        if based == 2:   # (the frame after the one that built it: its keys were armed by a pack)
            break
    assert based == 2 and tr.info(capi.LS_INFO_STANDING_BASE_BUILDS) == 1 and tr.info(capi.LS_INFO_STANDING_GEOMETRIES) == 1
    assert len(pts) == 256482
    assert hashlib.sha256(np.ascontiguousarray(pts).tobytes()).hexdigest().startswith("5eeb1f64")
    tr.close()
