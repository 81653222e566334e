"""Standing lists and the standing base with frames in flight (ls_commit.cpp: standing_commit, standing_build; ls_trace.cpp:
base_for_frame, base_build, arm_keys, the skipped finish launch).  The two other standing files flush every frame before the next
is issued; here frames go out with ls_trace_scene_async in TURNS of R frames with no host wait inside a turn, into a ring of R
caller-owned buffer sets, and every frame of every turn is compared byte for byte -- count, points, hit records -- with the CPU
oracle's frame for the scene as it stood when the frame was issued.  A wrong ordering does not crash: it shows last frame's pose,
the old ground, or a hole, in some frames.

A HELD turn makes "in flight" a checked fact: before its first commit a bounded delay kernel (torch.cuda._sleep, some
milliseconds) is launched on a side stream, an event is recorded behind it and handed to ls_tracer_wait_event, which holds the
handle's stream and, through main_epoch, every slot stream.  After the turn's last ls_trace_scene_async the event must still be
pending: the whole turn -- commits, list and base rebuilds, arm_keys copies -- was enqueued before any of it ran.  The delay is
ten times the host's enqueue time of the most recent turn that had no host wait in it, from a calibration of _sleep taken once.

Calls that wait for the device BY CONTRACT end a hold: a commit that lays the geometries out anew (a geometry added),
ls_remove_geometry, ls_tracer_set_sensor ("frames in flight complete first") and the first three-stream frame after
ls_tracer_set_shard (launch_project_init completes before the other streams' frames).  A turn with such a change asserts the
event pending immediately BEFORE the change (the frames before it were all enqueued and none had run), and holds again, with a
new delay and event, right after the frame that carries the change; that second event is the one that must be pending at the end.

A list becomes usable only at a commit that finds its build's event complete (hipEventQuery, never a wait): inside a held turn
never, at the first commit of the next turn always (a turn ends with flush + synchronize).  The first turn of a scene is
FIRST_WAIT + 1 frames long and not held: its last commit is the one that launches the first builds (see turns_until_base), so
every first list comes into use at the same commit, the first of the second turn, whatever the device's pace.

The scene, the poses, the sky mesh and the per-state oracle cache are those of test_gpu_standing_base.py."""
import ctypes as C
import time

import numpy as np
import pytest

import cull_reference as cr
import test_gpu_standing_base as sb
from test_gpu_standing_base import POSE_A, POSE_B, _pose, _sensor, _sky

pytestmark = pytest.mark.gpu

FIRST_WAIT = 2            # ls_internal.h: kStandingFirstWait -- the first wait of a list (commits) and of the base (frames)
LIST_BREAK_EVEN = 72      # ls_internal.h: kStandingBreakEven
BASE_BREAK_EVEN = 8       # ls_internal.h: kBaseBreakEven
FUSE_BLOCKS = 512         # ls_trace.cpp: three-stream frames of at most this many ray blocks take ONE finish + pack launch
LEAD = FIRST_WAIT + 1     # frames of a scene's first turn: commits 0, 1, 2 -- the third finds the key equal twice in a row and builds
MARGIN = 10               # the delay of a held turn over the host's enqueue time of a turn
GROUND_DOWN = _pose(0.0, 0.0, 0.0, dz=-0.3)

_CAL = {}
_STATS = {}
_HIP = []


def turns_until_base(j, R, list_wait=FIRST_WAIT, base_wait=FIRST_WAIT, first=None):
    """Turns, the one that holds the change counted as the first, within which a frame starts from the base of the final set,
    for a change before frame j of a turn of `first` frames (R by default) followed by turns of R frames.  From ls_commit.cpp and
    ls_trace.cpp alone:
      * the commit of frame j sees another key (same = 0); `same` reaches `list_wait` at the commit of frame j + list_wait, which
        launches the build (list_wait: kStandingFirstWait = 2, or 4 where the dropped list had served fewer than
        kStandingBreakEven = 72 frames -- the doubling rule; None: no list has to be built, the set is final at frame j);
      * the build's event is complete when that turn has ended (flush + synchronize), not necessarily before: the list is usable
        at the FIRST commit of the next turn at the latest, and from that frame on the routed set is the final one;
      * the base is built by the base_wait-th frame in a row with that set (kStandingFirstWait = 2; 4 where a base was dropped
        before it had served kBaseBreakEven = 8 frames, which happens at most once on the way: a base built for the set without the
        new list, inside the turn of the change, and dropped when the list joins), and that frame starts from it."""
    first = R if first is None else first
    turn_of = lambda g: 0 if g < first else 1 + (g - first) // R
    start_of = lambda t: 0 if t == 0 else first + (t - 1) * R
    g_final = j if list_wait is None else start_of(turn_of(j + list_wait) + 1)
    return turn_of(g_final + base_wait - 1) + 1


def _calibration(torch):
    """cycles of torch.cuda._sleep per millisecond, timed once with torch events"""
    if not _CAL:
        torch.cuda._sleep(1000)                                 # (the kernel's code is on the device)
        torch.cuda.synchronize()
        n = 10_000_000
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.0
        _CAL["cycles_per_ms"] = n / ms
        print(f"\n[standing-async] calibration: _sleep({n}) took {ms:.3f} ms -> {_CAL['cycles_per_ms']:.0f} cycles per ms")
    return _CAL["cycles_per_ms"]


def _device_bytes(ptr, n):
    """n bytes at a raw device address (the library's own output buffers) -> numpy uint8"""
    if not _HIP:
        # the HIP runtime this process has loaded already (torch's), by the path the loader mapped it from: whatever its version
        with open("/proc/self/maps") as maps:
            paths = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
        assert len(paths) == 1, paths
        hip = C.CDLL(paths[0])
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemcpy.restype = C.c_int
        _HIP.append(hip)
    out = np.empty(n, np.uint8)
    if n:
        assert _HIP[0].hipMemcpy(out.ctypes.data, ptr, n, 2) == 0   # hipMemcpyDeviceToHost
    return out


class Change:
    """what is done before a frame of a turn.  waits: the call, or the commit or frame behind it, waits for the device by contract
    and so ends a hold (module docstring); commit: whether ls_commit_scene is called for the frame"""

    def __init__(self, fn, waits=False, commit=True):
        self.fn, self.waits, self.commit = fn, waits, commit


class AsyncScene(sb.Scene):
    """Scene's add / move / ref bookkeeping, frames issued in turns (module docstring)"""
    INFOS = ("BASE", "GEOMETRIES", "BASE_BUILDS", "BUILDS", "BASE_NO_FINISH", "RECORDS")

    def __init__(self, oracle, capi, s, geoms, label, pipeline=2, R=8, own_stream=False, own_outputs=False):
        import torch
        self.torch = torch
        super().__init__(oracle, capi, s, [], pipeline=pipeline)
        if pipeline == 2:
            assert self.tr.info(capi.LS_INFO_PIPELINE_MODE) == 2, "fewer than three concurrent streams on this device"
        self.stream = torch.cuda.Stream() if own_stream else None
        if self.stream is not None:
            self.tr.setStream(self.stream.cuda_stream)          # before anything is uploaded: lists and base are built on it
        self.ids = {}
        for name, v, e, A in geoms:
            self.add(name, v, e, A)
        self.label, self.R, self.own_outputs = label, R, own_outputs
        self.cap = s.V * s.H
        self.side, self.side2 = torch.cuda.Stream(), torch.cuda.Stream()
        self.cycles_per_ms = _calibration(torch)
        dev = torch.device("cuda", 0)
        self.ring = [] if own_outputs else [(torch.empty(32 * self.cap, dtype=torch.uint8, device=dev),
                                             torch.empty(16 * self.cap, dtype=torch.uint8, device=dev),
                                             torch.empty(4, dtype=torch.int32, device=dev)) for _ in range(R)]
        if own_outputs:
            self.tr.setOutputBuffers(None, None, None, 0)
        self._poison(range(len(self.ring)))
        self.step = None                                        # what happens before EVERY frame (ben alternating)
        self.frame_ms = None                                    # the host's enqueue time per frame, of the last turn without a wait
        self.hold_ev = self.park_ev = None
        self.park = ()
        self.stats = _STATS.setdefault(label, dict(frames=0, based=0, held=0, held_turns=0, delay_cycles=0, enqueue_ms=0.0))

    def add(self, name, v, e, A):
        super().add(name, v, e, A)
        self.ids[name] = self.tr.getGeometryId(name)

    def remove(self, name):
        rc = self.tr.removeGeometry(name)
        del self.geoms[name]
        return rc

    # ---- the ring
    def _poison(self, sets):
        for i in sets:
            p, h, c = self.ring[i]
            p.fill_(0xA5)
            h.fill_(0xA5)
            c.fill_(0x5A5A5A5A)
        self.torch.cuda.synchronize()                           # the fill has ended before the next turn starts

    # ---- holding
    def _hold(self, n_frames):
        torch = self.torch
        assert self.frame_ms is not None, "a held turn needs an earlier turn's enqueue time"
        delay_ms = MARGIN * self.frame_ms * n_frames
        assert delay_ms < 1000.0, f"a turn took the host {self.frame_ms * n_frames:.1f} ms to enqueue: no bounded delay covers that ten times"
        cycles = int(delay_ms * self.cycles_per_ms) + 1
        ev = self._delay(self.side, cycles)
        self.tr.waitEvent(ev.cuda_event)
        self.stats["delay_cycles"] = max(self.stats["delay_cycles"], cycles)
        self.hold_cycles = cycles
        return ev

    def _delay(self, stream, cycles):
        """a delay kernel of `cycles` on a side stream -> the event behind it"""
        torch = self.torch
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
            ev = torch.cuda.Event()
            ev.record(stream)
        return ev

    # ---- one frame
    def _snapshot(self):
        """what the oracle needs for the scene as it stands, and the key of test_gpu_standing_base.py's cache (nothing is traced here:
        an oracle frame inside a turn would be the host wait the turn must not have)"""
        g = [(self.ids[n], n, v, e, A) for n, (v, e, A) in self.geoms.items()]
        key = (self.s.V, self.s.H, self.s.t.tobytes(), tuple((i, n, v.shape[0], A.tobytes()) for i, n, v, e, A in g))
        return key, self.s, [(i, v, e, A) for i, n, v, e, A in g], self.shard

    def _issue(self, i, change):
        if self.step:
            self.step(self.k)
        if change is not None:
            if change.waits and self.hold_ev is not None:
                assert self.hold_ev.query() is False, f"{self.label}: frames before the change at frame {i} of a held turn had started"
            change.fn()
        if change is None or change.commit:
            assert self.tr.commitScene() == 0
        if not self.own_outputs:
            p, h, c = self.ring[i]
            self.tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), self.cap)
        if i in self.park:
            self.tr.nextFrameWaits(self.park_ev.cuda_event)    # this frame's slot stream stays parked after the hold has ended
        fr = self.tr.traceSceneAsync(self.k)
        rec = {w: self.info(w) for w in self.INFOS}             # host state, final when the call has returned
        rec.update(i=i, k=self.k, fr=fr, snap=self._snapshot(), held=self.hold_ev is not None and self.hold_ev.query() is False)
        self.k += 1
        if change is not None and change.waits and self.hold_ev is not None:
            self.hold_ev = self._hold(self.n_turn)              # held again, for the frames that follow (a whole turn's delay)
        return rec

    def _expected(self, snap):
        key, s, ml, shard = snap
        if key not in sb._REFS:
            sb._REFS[key] = self.o.trace_frame(s, ml)
        ref = sb._REFS[key]
        if shard is None:
            return ref["points"], ref["hits"]
        cols = ref["hits"][:, 0] % s.H                          # global ray numbers are kept (test_gpu_parity.py: test_pipelined_frames)
        keep = (cols >= shard[0]) & (cols < shard[0] + shard[1])
        assert keep.sum() == int((ref["gid"].reshape(s.V, s.H)[:, cr.shard_columns(s.H, shard)] != self.o.INVALID).sum())
        return ref["points"][keep], ref["hits"][keep]

    def _compare(self, rec):
        want_p, want_h = self._expected(rec["snap"])
        where = f"{self.label}: frame {rec['k']} (frame {rec['i']} of its turn)"
        if self.own_outputs:
            fr = rec["fr"]
            n = int(_device_bytes(fr.d_n_points, 4).view(np.uint32)[0])
            assert n == len(want_p), (where, n, len(want_p))
            got_p, got_h = _device_bytes(fr.d_points32, 32 * n), _device_bytes(fr.d_hits, 16 * n)
        else:
            p, h, c = self.ring[rec["i"]]
            n = int(c[0].item())
            assert n == len(want_p), (where, n, len(want_p))   # (a frame that wrote nothing: the poison)
            got_p, got_h = p[:32 * n].cpu().numpy(), h[:16 * n].cpu().numpy()
        assert np.array_equal(got_h.view(np.uint32).reshape(n, 4), want_h), where
        assert np.array_equal(got_p.reshape(n, 32), want_p), where
        rec["n"] = n

    # ---- one turn
    def turn(self, held=False, changes=None, n=None, park=()):
        """n frames (R by default) with no host wait between them but those of `changes` {frame of the turn: Change}; then flush,
        synchronize, every frame against its oracle frame, poison.  -> the frames' records
        park: frames of a held three-stream turn that wait for a SECOND event (ls_tracer_next_frame_waits, on the frame's own slot
        stream), behind a delay twice the hold's.  When the hold ends, whatever the turn enqueued on the handle's stream -- a list's
        or a base's rebuild -- could run at once while these frames, enqueued before it, have still not started: the rebuild's
        order_after_projects is then the only thing that keeps it from overwriting what they read, whatever the streams' pace."""
        changes = changes or {}
        self.n_turn = n = self.R if n is None else n
        assert n <= self.R
        clean = not any(c.waits for c in changes.values())
        t0 = time.perf_counter()
        self.hold_ev = self._hold(n) if held else None
        self.park = tuple(park)
        if self.park:
            assert held and clean and self.tr.info(self.capi.LS_INFO_PIPELINE_MODE) == 2
            self.park_ev = self._delay(self.side2, 2 * self.hold_cycles)
        recs = [self._issue(i, changes.get(i)) for i in range(n)]
        t1 = time.perf_counter()
        if held:
            assert self.hold_ev.query() is False, f"{self.label}: the held turn had started to run before its last frame was issued"
            assert not self.park or self.park_ev.query() is False
            self.stats["held_turns"] += 1
        self.hold_ev = self.park_ev = None
        self.park = ()
        if clean:
            self.frame_ms = (t1 - t0) * 1e3 / n
            self.stats["enqueue_ms"] = max(self.stats["enqueue_ms"], (t1 - t0) * 1e3)
        self.tr.flush()
        self.tr.synchronize()
        if self.stream is not None:
            self.stream.synchronize()
        self.torch.cuda.synchronize()
        for rec in recs:
            self._compare(rec)
        if not self.own_outputs:
            self._poison(range(n))
        self.stats["frames"] += n
        self.stats["based"] += sum(r["BASE"] for r in recs)
        self.stats["held"] += sum(1 for r in recs if r["held"])
        self.last = recs
        return recs

    def until_base(self, turns, geometries, held=False, first=None):
        """turns (every frame compared) until the last frame of one starts from a base of `geometries` lists; at most `turns`"""
        for t in range(turns):
            recs = self.turn(held=held, n=first if t == 0 else None)
            if recs[-1]["BASE"] == 1 and recs[-1]["GEOMETRIES"] == geometries:
                return recs
        raise AssertionError(f"{self.label}: no frame started from a base of {geometries} lists within {turns} turns")

    def begin(self, geometries, base_wait=FIRST_WAIT):
        """the first turns of a scene: LEAD frames, then turns of R until the base is in use"""
        return self.until_base(turns_until_base(0, self.R, FIRST_WAIT, base_wait, first=LEAD), geometries, first=LEAD)

    def close(self):
        st = self.stats
        print(f"\n[standing-async] {self.label}: {st['frames']} frames compared, {st['based']} started from a base, {st['held']} issued "
              f"under a hold ({st['held_turns']} held turns); longest delay {st['delay_cycles']} cycles "
              f"({st['delay_cycles'] / self.cycles_per_ms:.2f} ms), longest turn enqueued in {st['enqueue_ms']:.3f} ms")
        super().close()


def _alternating(sc):
    """ben at POSE_A before even frames, POSE_B before odd ones"""
    sc.step = lambda k: sc.move("ben", POSE_B if (k & 1) else POSE_A)


def _ground_ben(oracle, capi, sensors, meshes, label, alternating=False, **kw):
    s = _sensor(oracle, sensors)
    sc = AsyncScene(oracle, capi, s, [("ground", *meshes["ground"], oracle.IDENTITY_AFFINE), ("ben", *meshes["ben"], POSE_A)], label, **kw)
    if alternating:
        sb._check_disjoint(sc)                                  # (on the oracle: also computes the two states' frames before any turn)
        sc.move("ben", POSE_A)
        _alternating(sc)
    return sc


def _all(recs, **want):
    for r in recs:
        for w, v in want.items():
            assert r[w] == v, (w, v, [(q["i"], q[w]) for q in recs])


# ---- 1. everything stands -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [2, 0])
def test_everything_stands(oracle, capi, sensors, meshes, pipeline):
    """Both lists are built by the last commit of the first turn and come into use together at the first commit of the second, so
    no base of a smaller set is built on the way: the base is built by the second frame of the second turn, once.  Then two held
    turns of 8: with three slots (two without the rotation) each slot's keys are armed by the copy once, in the second turn, and by
    its own packs from then on -- 16 frames whose every pack re-arms keys that the frame three later starts from.  (No info key
    counts arm_keys' copies: that each slot came through the copy once is inferred from BASE_BUILDS == 1 -- one generation, so
    keys_arm[slot] differs from it once per slot -- and from the clouds of the frames; it is not asserted.)"""
    sc = _ground_ben(oracle, capi, sensors, meshes, f"1 everything stands, pipeline {pipeline}", pipeline=pipeline)
    recs = sc.begin(2)
    assert [r["BASE"] for r in recs] == [0] + [1] * (sc.R - 1) and recs[-1]["BASE_BUILDS"] == 1 and recs[-1]["RECORDS"] > 100
    for _ in range(2):
        _all(sc.turn(held=True), BASE=1, BASE_BUILDS=1, GEOMETRIES=2, BUILDS=2)
    sc.close()


# ---- 2. the ground in the base, ben alternating ---------------------------------------------------------------------------------
def _alternating_scene(sc, turns=3, held=True):
    sc.begin(1)
    for _ in range(turns):
        _all(sc.turn(held=held), BASE=1, GEOMETRIES=1, BUILDS=1, BASE_BUILDS=1)   # ben never got a list
    sc.close()


@pytest.mark.parametrize("pipeline", [2, 0])
def test_ground_in_the_base_ben_alternating(oracle, capi, sensors, meshes, pipeline):
    """three held turns: a frame that started from another slot's keys, or whose pack re-armed to anything but the base, shows ben at
    the other pose or a hole where ben left (the footprints are disjoint, and rays ben has left see the ground again)"""
    _alternating_scene(_ground_ben(oracle, capi, sensors, meshes, f"2 ben alternating, pipeline {pipeline}", alternating=True, pipeline=pipeline))


# ---- 3. the ground moves inside a held turn -------------------------------------------------------------------------------------
@pytest.mark.parametrize("served", ["list served 72 frames", "list served fewer", "list served one frame"])
def test_the_ground_moves_in_a_held_turn(oracle, capi, sensors, meshes, served):
    """The ground takes another pose before frame 1 of a held turn.  Frame 0 was enqueued with the old list and base and has not run;
    frames 1 .. 7 trace the ground from the mesh (its list is gone until a build's event has been SEEN complete, which a held turn
    rules out).  The rebuild goes into the same record buffer, inside the turn, behind readers that have not run: at the commit
    of frame 1 + wait, wait = 2 after the list had served kStandingBreakEven = 72 frames, 4 (doubled) before.  Then the second
    list (first commit of the next turn), the second base (within turns_until_base), in held turns as well.
    A frame that starts from the base launches no k_project_standing and so does not read the list at all.  The third case moves
    the ground in the very turn in which its list comes into use: frame 0 of that turn has no base yet (the set is one frame old)
    and reads the list's records, frame 5 of the same held turn launches the rebuild into that buffer (wait 4: the list had served
    one frame) -- the reader that order_after_projects in standing_build is there for.  That frame 0 is PARKED (AsyncScene.turn):
    it starts after the hold has ended and the handle's stream could have run the rebuild, so a build that is not ordered behind
    it hands it the lowered ground's records.  There is one base in that case, not two."""
    sc = _ground_ben(oracle, capi, sensors, meshes, f"3 the ground moves, {served}", alternating=True)
    early = served.endswith("one frame")
    if early:
        _all(sc.turn(n=LEAD), BASE=0, GEOMETRIES=0)
    else:
        sc.begin(1)
        # the list serves every frame from the first of the second turn on: 7 + 1 based frames so far, 8 per turn
        for _ in range(LIST_BREAK_EVEN // sc.R if served.endswith("72 frames") else 1):
            _all(sc.turn(held=True), BASE=1)
    wait = FIRST_WAIT if served.endswith("72 frames") else 2 * FIRST_WAIT
    recs = sc.turn(held=True, changes={1: Change(lambda: sc.move("ground", GROUND_DOWN))}, park=(0,) if early else ())
    assert [r["BASE"] for r in recs] == [0 if early else 1] + [0] * (sc.R - 1)
    assert [r["GEOMETRIES"] for r in recs] == [1] + [0] * (sc.R - 1)
    assert [r["BUILDS"] for r in recs] == [1] * (1 + wait) + [2] * (sc.R - 1 - wait)
    more = turns_until_base(1, sc.R, wait, 2 * FIRST_WAIT) - 1
    recs = sc.until_base(more, 1, held=True)
    assert recs[0]["GEOMETRIES"] == 1 and recs[0]["BASE"] == 0   # the list at the first commit, no base yet
    assert recs[-1]["BUILDS"] >= 2 and recs[-1]["BASE_BUILDS"] >= (1 if early else 2) and recs[-1]["GEOMETRIES"] == 1
    _all(sc.turn(held=True), BASE=1, GEOMETRIES=1)
    sc.close()


# ---- 4. a geometry added and removed inside held turns ----------------------------------------------------------------------------
def test_a_geometry_added_and_removed_in_held_turns(oracle, capi, sensors, meshes):
    """ben2, a copy of ben at POSE_B, is added before frame 2 of a held turn.  The two lists stay, the routed set's bits change: the
    base is dropped at frame 2 and built again into the same buffer inside the turn.  Frames 0 and 1 were enqueued and had not run
    when the change was made, but the commit that lays the scene out anew waits for them: nothing reads the old base when it is
    rebuilt here (test_a_standing_geometry_moves_once_in_a_held_turn is the case with such readers).  ben2's list joins at the first commit of the next turn, another
    set: the third base.  Later ben2 is removed before frame 2 of a held turn; that frame is issued without a commit of its own
    (the removal commits), as in test_changes_under_a_base."""
    sc = _ground_ben(oracle, capi, sensors, meshes, "4 a geometry added and removed")
    sc.begin(2)
    _all(sc.turn(held=True), BASE=1)                            # (the base has served kBaseBreakEven frames: its wait is 2 again)
    recs = sc.turn(held=True, changes={2: Change(lambda: sc.add("ben2", *meshes["ben"], POSE_B), waits=True)})
    # (the base had served kBaseBreakEven frames, its wait is kStandingFirstWait: dropped at frame 2, built by the second frame with the new set)
    assert [r["BASE"] for r in recs] == [1, 1, 0] + [1] * (sc.R - 3) and [r["GEOMETRIES"] for r in recs] == [2] * sc.R
    assert [r["BASE_BUILDS"] - recs[0]["BASE_BUILDS"] for r in recs] == [0, 0, 0] + [1] * (sc.R - 3)
    assert sc.ids["ben2"] == 2
    more = turns_until_base(2, sc.R, FIRST_WAIT, 2 * FIRST_WAIT) - 1
    recs = sc.until_base(more, 3, held=True)
    assert recs[-1]["BASE_BUILDS"] >= 2 and recs[-1]["BUILDS"] == 3
    _all(sc.turn(held=True), BASE=1, GEOMETRIES=3)

    def remove():
        assert sc.remove("ben2") == 2                           # (its id; the removal commits)

    recs = sc.turn(held=True, changes={2: Change(remove, waits=True, commit=False)})
    # no list has to be built: the set is final at frame 2, and the base, which had served kBaseBreakEven frames (wait
    # kStandingFirstWait), is built by the second frame with it -- frame 3 of this turn
    assert [r["BASE"] for r in recs] == [1, 1, 0] + [1] * (sc.R - 3) and [r["GEOMETRIES"] for r in recs] == [3, 3] + [2] * (sc.R - 2)
    assert [r["BASE_BUILDS"] - recs[0]["BASE_BUILDS"] for r in recs] == [0, 0, 0] + [1] * (sc.R - 3)
    _all(sc.turn(held=True), BASE=1, GEOMETRIES=2)
    sc.close()


# ---- 4b. a standing geometry moves once: the base rebuilt behind frames that still read it ----------------------------------------
@pytest.mark.parametrize("V,H,R", [(16, 256, 8), (128, 1032, 6)])
def test_a_standing_geometry_moves_once_in_a_held_turn(oracle, capi, sensors, meshes, V, H, R):
    """Two geometries in the base, which has served kBaseBreakEven frames; one of them takes another pose before frame 2 of a held
    turn and stays there.  No call waits: the hold is never broken.  Its list is dropped, the routed set is the other geometry
    alone: the base is dropped at frame 2 and built again at frame 3 (wait kStandingFirstWait) into the SAME keys and counts
    buffers, behind frames 0 and 1, which are parked and so have not run when the handle's stream could run the rebuild.
    At 16 x 256 ben moves over the ground; at 128 x 1032 ben has more footprints than a list may hold and never stands, so there
    the ground moves under the sky mesh (an empty list: the second base is all ones and counts nothing).
    What frames 0 and 1 still read of the old base:
      * 128 x 1032 (516 ray blocks, the two-launch path): nothing was projected, their finish launch was skipped, and their packs
        take base.counts as block counts -- the new base's counts, all zero, would leave them without a single point.  This is
        the reader order_after_projects in base_build is there for;
      * 16 x 256 (the fused launch): only the values their packs re-arm the slot's keys to.  keys_arm[slot] then names the old
        generation, the next frame on the slot wants another (or all ones) and overwrites the keys: a rebuild that overtook
        these packs would change no cloud, so this size pins the clouds and the counters, not that ordering."""
    s = _sensor(oracle, sensors, V=V, H=H)
    two_launches = (V * H + 255) // 256 > FUSE_BLOCKS
    other = ("sky", *_sky(oracle, s), oracle.IDENTITY_AFFINE) if two_launches else ("ben", *meshes["ben"], POSE_A)
    moved = ("ground", GROUND_DOWN) if two_launches else ("ben", POSE_B)
    sc = AsyncScene(oracle, capi, s, [("ground", *meshes["ground"], oracle.IDENTITY_AFFINE), other], f"4b a standing geometry moves once, {V} x {H}", R=R)
    sc.begin(2)
    served = R - 1
    while served < BASE_BREAK_EVEN:
        _all(sc.turn(held=True), BASE=1, GEOMETRIES=2)
        served += R
    recs = sc.turn(held=True, changes={2: Change(lambda: sc.move(*moved))}, park=(0, 1))
    assert [r["BASE"] for r in recs] == [1, 1, 0] + [1] * (R - 3) and [r["GEOMETRIES"] for r in recs] == [2, 2] + [1] * (R - 2)
    assert [r["BASE_BUILDS"] - recs[0]["BASE_BUILDS"] for r in recs] == [0, 0, 0] + [1] * (R - 3)
    if two_launches:   # frames 0 and 1 skipped their finish launch; from frame 2 on the ground is projected from its mesh
        assert [r["BASE_NO_FINISH"] - recs[0]["BASE_NO_FINISH"] for r in recs] == [0, 1] + [1] * (R - 2)
    assert not np.array_equal(sc._expected(recs[1]["snap"])[0], sc._expected(recs[2]["snap"])[0])
    sc.turn(held=True)                                          # (the moved geometry's list is built again in here; every frame the oracle's)
    sc.close()


# ---- 5. the sensor moves, the shard narrows ---------------------------------------------------------------------------------------
def test_sensor_and_shard_change_in_held_turns(oracle, capi, sensors, meshes):
    """ls_tracer_set_sensor to a shifted origin before frame 3 of a held turn, ls_tracer_set_shard(140, 96) before frame 3 of a
    later one.  Frames 0 .. 2 are the oracle's for the old state -- they had not run when the change was made --, frames 3 .. 7
    for the new one (for the shard: the oracle's records whose column lies in it, global ray numbers kept).  Every key changes, so
    both lists go and are built again after their wait (4 commits, then 8: dropped twice before they had served 72 frames), the second
    time inside a later held turn; a base is in use again within turns_until_base."""
    sc = _ground_ben(oracle, capi, sensors, meshes, "5 sensor and shard")
    sc.begin(2)
    _all(sc.turn(held=True), BASE=1)
    s2 = _sensor(oracle, sensors, t=sc.s.t + np.asarray([0.3, -0.2, 0.1], np.float32))

    def set_sensor():
        sc.tr.setOutputBuffers(None, None, None, 0)             # (the call refuses while a caller's buffers are installed)
        sc.tr.setSensor(s2.vertical, s2.h_begin, s2.h_end, s2.h_count, s2.Rinv, s2.t)
        sc.s = s2

    def set_shard():
        sc.tr.setShard(140, 96)                                 # 96 of 256 columns, ben's among them
        sc.shard = (140, 96)

    # (the lists serve about 20 frames between their builds: dropped before kStandingBreakEven twice in a row, their wait is 4, then 8)
    for change, list_wait in ((set_sensor, 2 * FIRST_WAIT), (set_shard, 4 * FIRST_WAIT)):
        recs = sc.turn(held=True, changes={3: Change(change, waits=True)})
        assert [r["BASE"] for r in recs[:4]] == [1, 1, 1, 0] and recs[3]["GEOMETRIES"] == 0
        assert not np.array_equal(sc._expected(recs[2]["snap"])[0], sc._expected(recs[3]["snap"])[0])   # (the two states' clouds differ)
        more = turns_until_base(3, sc.R, list_wait, 2 * FIRST_WAIT) - 1
        recs = sc.until_base(more, 2, held=True)
        _all(sc.turn(held=True), BASE=1, GEOMETRIES=2)
    sc.close()


# ---- 6. no finish launch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline,V,H,R", [(2, 16, 256, 8), (0, 16, 256, 8), (2, 128, 1032, 6)])
def test_no_finish_launch_in_held_turns(oracle, capi, sensors, meshes, pipeline, V, H, R):
    """The ground alone.  The second turn is held already: its first frame traces from the list, its second builds the base -- on
    the handle's stream, not run -- and is itself the first frame whose pack takes base.counts, from a build that has not run when
    the frame is enqueued; nothing is left to project, so from that frame on LS_INFO_STANDING_BASE_NO_FINISH grows by exactly one
    per frame on the two-launch path: one frame in flight, or three with more than 512 ray blocks (128 x 1032 is 516: the wide
    packs).  Three frames in flight at 16 x 256 (16 blocks) take the fused finish + pack launch, which has no finish launch to
    skip: the counter stays where it is, the clouds are compared all the same."""
    s = _sensor(oracle, sensors, V=V, H=H)
    sc = AsyncScene(oracle, capi, s, [("ground", *meshes["ground"], oracle.IDENTITY_AFFINE)], f"6 no finish launch, pipeline {pipeline}, {V} x {H}",
                    pipeline=pipeline, R=R)
    two_launches = pipeline == 0 or (V * H + 255) // 256 > FUSE_BLOCKS
    recs = sc.turn(n=LEAD)
    _all(recs, BASE=0, BASE_NO_FINISH=0)
    assert turns_until_base(0, R, first=LEAD) == 2
    skipped = 0
    for t in range(1 if R == 6 else 2):
        recs = sc.turn(held=True)
        assert [r["BASE"] for r in recs] == ([0] + [1] * (R - 1) if t == 0 else [1] * R)
        for r in recs:
            skipped += r["BASE"] if two_launches else 0
            assert r["BASE_NO_FINISH"] == skipped, [(q["i"], q["BASE"], q["BASE_NO_FINISH"]) for q in recs]
        _all(recs, GEOMETRIES=1)
        assert recs[-1]["BASE_BUILDS"] == 1
    sc.close()


# ---- 7. a base of all ones --------------------------------------------------------------------------------------------------------
def test_a_base_of_all_ones(oracle, capi, sensors, meshes):
    """the only standing geometry lies above the top ring: an empty list, a base of all ones, ben alternating on top of it"""
    s = _sensor(oracle, sensors)
    sc = AsyncScene(oracle, capi, s, [("sky", *_sky(oracle, s), oracle.IDENTITY_AFFINE), ("ben", *meshes["ben"], POSE_A)], "7 a base of all ones")
    _alternating(sc)
    sc.begin(1)
    for _ in range(2):
        recs = sc.turn(held=True)
        _all(recs, BASE=1, GEOMETRIES=1, RECORDS=0)
        assert min(r["n"] for r in recs) > 50
    sc.close()


# ---- 8. the caller's stream -------------------------------------------------------------------------------------------------------
def test_on_the_callers_stream(oracle, capi, sensors, meshes):
    """ls_tracer_set_stream(a torch stream) before the first upload: every frame takes the `dep` branch, lists and base are built on
    a stream the library does not own, and the hold is a wait on that stream"""
    _alternating_scene(_ground_ben(oracle, capi, sensors, meshes, "8 the caller's stream", alternating=True, own_stream=True))


# ---- 9. library-owned outputs -------------------------------------------------------------------------------------------------------
def test_library_owned_outputs(oracle, capi, sensors, meshes):
    """no caller's buffers: turns of three frames, not held, each frame read from its ls_frame's d_points32 / d_hits / d_n_points
    after the flush -- the per-slot twin buffers under frames that start from the base.  Nothing poisons these buffers, but a slot
    that its frame did not write holds the frame three earlier: ben at the OTHER pose (3 is odd), which the comparison refuses."""
    sc = _ground_ben(oracle, capi, sensors, meshes, "9 library-owned outputs", alternating=True, R=3, own_outputs=True)
    assert sc.R == LEAD
    _alternating_scene(sc, turns=6, held=False)


# ---- frames that step around a live base (the synchronous API) -------------------------------------------------------------------
def _based_scene(oracle, capi, sensors, meshes, pipeline):
    sc = sb._ground_ben(oracle, capi, sensors, meshes, pipeline=pipeline)
    sc.until_base(sb.SETTLE + sb.BASE_WAIT)
    sc.serve(4)
    return sc


@pytest.mark.parametrize("pipeline", [0, 2])
def test_frames_that_step_around_a_live_base(oracle, capi, sensors, meshes, pipeline):
    """a two-step frame (progress_req), two timing frames, three rider frames (which advance pipe_seq: the next mode-0 frame may
    take the other slot): each is the oracle's and leaves the base alone; the base is known by its set and serves the first default
    frame afterwards"""
    sc = _based_scene(oracle, capi, sensors, meshes, pipeline)
    builds = sc.info("BASE_BUILDS")
    ref = sc.ref()
    assert sc.tr.commitScene() == 0
    rc, pts = sc.tr.traceSceneTwoStep(sc.k)
    sc.k += 1
    assert rc == 0 and len(pts) == len(ref["points"]) and np.array_equal(pts, ref["points"])
    assert sc.info("BASE") == 0
    sc.tr.setOption(capi.LS_OPT_TIMING, 1)
    for _ in range(2):
        sc.frame()
        assert sc.info("BASE") == 0 and sc.info("GEOMETRIES") == 0
    sc.tr.setOption(capi.LS_OPT_TIMING, 0)
    sc.tr.setOption(capi.LS_OPT_PIPELINE, 1)
    for _ in range(3):
        sc.frame()
        assert sc.info("BASE") == 0 and sc.info("GEOMETRIES") == 0
    sc.tr.setOption(capi.LS_OPT_PIPELINE, pipeline)
    sc.frame()
    assert sc.info("BASE") == 1 and sc.info("GEOMETRIES") == 2
    sc.serve(3)                                                 # (every slot of the rotation once more)
    assert sc.info("BASE_BUILDS") - builds <= 1
    sc.close()


def test_pipeline_modes_switched_under_a_live_base(oracle, capi, sensors, meshes):
    """LS_OPT_PIPELINE 0 -> 2 -> 0 -> 2, three frames in each mode: the slots' arming words outlive the switches"""
    sc = _based_scene(oracle, capi, sensors, meshes, 0)
    builds = sc.info("BASE_BUILDS")
    for mode in (0, 2, 0, 2):
        sc.tr.setOption(capi.LS_OPT_PIPELINE, mode)
        for _ in range(3):
            sc.frame()
    assert sc.info("BASE_BUILDS") - builds <= 1
    sc.close()


@pytest.mark.parametrize("pipeline", [0, 2])
def test_output_forms_under_a_live_base(oracle, capi, sensors, meshes, pipeline):
    """the pack's other output forms re-arm to the base as well: compact 1 (LS_OPT_HOST_OUTPUT = 2: 16-byte points, expanded on the
    host), records that stay on the device (LS_OPT_READBACK_HITS = 0: read through ls_debug_dense_hits) and compact 3
    (LS_OPT_EMIT_POINTS = 0: hit records only, asynchronous frames into a caller's buffers, whose point buffer stays untouched)"""
    import torch
    sc = _based_scene(oracle, capi, sensors, meshes, pipeline)
    ref = sc.ref()
    sc.tr.setOption(capi.LS_OPT_HOST_OUTPUT, 2)
    for _ in range(3):
        sc.frame()
        assert sc.info("BASE") == 1 and sc.tr.last_frame.compact16
    sc.tr.setOption(capi.LS_OPT_HOST_OUTPUT, 1)
    sc.tr.setOption(capi.LS_OPT_READBACK_HITS, 0)
    for _ in range(3):
        assert sc.tr.commitScene() == 0
        rc, pts, hits = sc.tr.traceScene(sc.k)
        sc.k += 1
        assert rc == 0 and len(hits) == 0 and sc.info("BASE") == 1
        assert len(pts) == len(ref["points"]) and np.array_equal(pts, ref["points"])
        tt, gid = sc.tr.denseHits()
        assert np.array_equal(gid, ref["gid"]) and np.array_equal(tt.view(np.uint32), ref["t"].view(np.uint32))
    sc.tr.setOption(capi.LS_OPT_READBACK_HITS, 1)
    cap = sc.s.V * sc.s.H
    dev = torch.device("cuda", 0)
    p, h, c = torch.empty(32 * cap, dtype=torch.uint8, device=dev), torch.empty(16 * cap, dtype=torch.uint8, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
    sc.tr.setOption(capi.LS_OPT_EMIT_POINTS, 0)
    sc.tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), cap)
    for _ in range(3):
        p.fill_(0xA5)
        h.fill_(0xA5)
        c.fill_(0x5A5A5A5A)
        torch.cuda.synchronize()
        assert sc.tr.commitScene() == 0
        sc.tr.traceSceneAsync(sc.k)
        sc.k += 1
        assert sc.info("BASE") == 1
        sc.tr.synchronize()
        torch.cuda.synchronize()
        n = int(c[0].item())
        assert n == len(ref["hits"])
        assert np.array_equal(h[:16 * n].cpu().numpy().view(np.uint32).reshape(n, 4), ref["hits"])
        assert bool((p == 0xA5).all())
    sc.tr.setOutputBuffers(None, None, None, 0)
    sc.tr.setOption(capi.LS_OPT_EMIT_POINTS, 1)
    sc.serve(3)
    sc.close()


def test_dense_hits_after_a_skipped_finish(oracle, capi, sensors, meshes):
    """the ground alone, unsharded, one frame in flight: a frame that launched no finish pass left nothing but its records, and
    ls_debug_dense_hits rebuilds the oracle's dense t / gid from them"""
    s = _sensor(oracle, sensors)
    sc = sb.Scene(oracle, capi, s, [("ground", *meshes["ground"], oracle.IDENTITY_AFFINE)])
    sc.until_base(sb.SETTLE + sb.BASE_WAIT)
    before = sc.info("BASE_NO_FINISH")
    sc.frame()
    assert sc.info("BASE") == 1 and sc.info("BASE_NO_FINISH") == before + 1
    ref = sc.ref()
    tt, gid = sc.tr.denseHits()
    assert np.array_equal(gid, ref["gid"]) and np.array_equal(tt.view(np.uint32), ref["t"].view(np.uint32))
    sc.close()
