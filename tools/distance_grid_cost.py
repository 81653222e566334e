"""tools/distance_grid_cost.py [out.json] -- cost of ls_scene_distance_grid and of its two tunables (EXPERIMENTS.md E24): bench.py's
SYN-1M scene under the SYN-128 sensor's pose, a 512 x 512 x 64 grid of 0.2 m cells centred on the sensor, trunc at 0.6 m (3 cells) and
at 1.6 m (8 cells).  Next to the call stand (a) ls_closest_points over the same 16.7 M cell centres with radius trunc -- what a user
had for this grid before, the yardstick -- and (b) ls_scene_grid on the same grid: the same traversal without the band, a floor.  The
forms -- the small / big threshold at 0 (every triangle queued), 1024, 5247 and at a value so large that nothing is queued, the pre-read
of the cell's word off and on -- run in one process, alternating call by call, after a warm-up of all of them; each figure is the median (min - max) of
per-call device-event times on the call's stream.  The grids of all forms are compared byte for byte.

The (triangle, cell) pairs tested are counted from a float64 estimate of the widened ranges; the atomics a call without the pre-read
issues (the counting pairs) are estimated by the numpy reference over every 512th triangle, times 512.

The forms are selected by LS_DIST_GRID_SMALL, LS_DIST_GRID_PREREAD and LS_DIST_GRID_CLEAR_ONLY, which only a library built with
EXPERIMENTAL=1 reads (csrc/ls_tuning.h):
    make -C lidarshooter_amd/csrc EXPERIMENTAL=1      (into a copy of the sources; the shipped library ignores the variables)
    LS_LIB_PATH=<that build>/liblidarshooter_hip.so python tools/distance_grid_cost.py out.json
With the shipped library every column times the shipped form; the tool says so.  DIST_GRID_COST_TRUNC=0.6 runs one band only."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import distance_grid_reference as ref  # noqa: E402
from lidarshooter_amd import capi, hostapi, synth  # noqa: E402

WARM = 2
NONE_QUEUED = 1 << 27                      # no range holds more cells than a grid may have
SAMPLE = 512
DATA = os.path.join(ROOT, "tests", "golden", "data")
d = hostapi.LidarDevice(os.path.join(DATA, "config", "hesai-pandar-XT-32-lidar_0000.json")).desc()
dev = "cuda:0"
# (threshold, pre-read)
FORMS = {"small=5247 pre-read": (5247, 1), "small=5247": (5247, 0), "small=1024 pre-read": (1024, 1), "everything queued pre-read": (0, 1),
         "nothing queued pre-read": (NONE_QUEUED, 1), "nothing queued": (NONE_QUEUED, 0)}
SHIPPED = "small=5247 pre-read"


def sensor_frame(verts):
    R, t = np.float64(d["Rinv"]).reshape(3, 3), np.float64(d["t"])
    return (np.float64(verts) - t) @ R.T


def ranges(v, tris, origin, cell, dims, trunc):
    """the cells of every triangle's widened, clamped range, estimated in float64 (the library's own arithmetic is float32: a triangle
    on a boundary may count one layer more or less; the queue's length is read from the device) -> int64[n]"""
    q = (v - np.float64(origin))[np.asarray(tris, np.int64)]
    lo, hi = np.floor((q.min(axis=1) - trunc) / cell), np.floor((q.max(axis=1) + trunc) / cell)
    n = np.float64(dims)
    inside = np.all((hi >= 0) & (lo < n), axis=1)
    w = np.clip(hi, 0, n - 1) - np.clip(lo, 0, n - 1) + 1
    return np.where(inside, w.prod(axis=1), 0).astype(np.int64)


def measure(name, verts, tris, dims, cell, trunc, calls):
    tr = capi.Tracer(synth.syn_vertical(128), np.float32(0.0), np.float32(360.0), 4096, d["Rinv"], d["t"])
    assert tr.addGeometry("ground", verts.shape[0], tris.shape[0]) == 0
    tr.updateGeometry("ground", capi.IDENTITY_AFFINE, verts, tris)
    assert tr.commitScene() == 0
    origin = [-0.5 * dims[0] * cell, -0.5 * dims[1] * cell, -0.5 * dims[2] * cell]
    desc = capi.DistanceGridDesc.make(origin, cell, dims, 0, trunc)
    sdesc = capi.SceneGridDesc.make(origin, cell, dims)
    cells = dims[0] * dims[1] * dims[2]
    d_cells = torch.zeros(cells, dtype=torch.int64, device=dev)
    d_counts = torch.zeros(cells, dtype=torch.int32, device=dev)
    d_geom = torch.zeros(cells, dtype=torch.int32, device=dev)
    d_none = torch.zeros(16, dtype=torch.uint8, device=dev)
    # (a): every cell centre as a point record with radius trunc, and its 32-byte answers
    ax = [(torch.arange(n, dtype=torch.float32, device=dev) + 0.5) * np.float32(cell) + np.float32(o) for n, o in zip(dims, origin)]
    pts = torch.empty((dims[2], dims[1], dims[0], 4), dtype=torch.float32, device=dev)
    pts[..., 0], pts[..., 1], pts[..., 2], pts[..., 3] = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None], float(trunc)
    d_near = torch.zeros(cells * 8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    sp = st.cuda_stream

    def call(form):
        os.environ["LS_DIST_GRID_CLEAR_ONLY"] = "1" if form == "clear" else "0"
        if form == "closest":
            assert tr.closestPointsDevice(pts.data_ptr(), cells, d_near.data_ptr(), stream=sp) == 0
        elif form == "scene":
            assert tr.sceneGridDevice(sdesc, d_counts.data_ptr(), d_geom.data_ptr(), stream=sp) == 0
        elif form in ("clear", "none"):    # the clear alone: the floor; nothing selected: the clear and two launches that find no work
            assert tr.sceneDistanceGridDevice(desc, d_cells.data_ptr(), d_none.data_ptr(), 1, stream=sp) == 0
        else:
            os.environ["LS_DIST_GRID_SMALL"], os.environ["LS_DIST_GRID_PREREAD"] = str(form[0]), str(form[1])
            assert tr.sceneDistanceGridDevice(desc, d_cells.data_ptr(), stream=sp) == 0

    forms = dict(FORMS, **{"nothing selected": "none", "clear alone": "clear", "(b) ls_scene_grid": "scene", "(a) ls_closest_points": "closest"})
    grids, queued = {}, {}
    for key, form in forms.items():
        for _ in range(WARM):
            call(form)
        st.synchronize()
        if form not in ("closest", "scene"):
            grids[key] = d_cells.cpu().numpy().copy().view(np.uint64)
            n_q = ctypes.c_uint32(0)
            assert tr.L.ls_debug_distance_grid_queued(tr.h, ctypes.byref(n_q)) == 0
            queued[key] = int(n_q.value)   # the device's own count word
    for key in FORMS:
        assert grids[key].tobytes() == grids[SHIPPED].tobytes(), key
    assert np.all(grids["nothing selected"] == ref.REST) and np.all(grids["clear alone"] == ref.REST)
    # the yardstick answers the same question (its points are origin + centre, rounded once more than the grid's: no bits compared)
    near = d_near.cpu().numpy().view(np.uint32).reshape(cells, 8)
    dist = (grids[SHIPPED] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    found, reached = near[:, 4] != 0xFFFFFFFF, grids[SHIPPED] != ref.REST
    both = found & reached
    same = {"cells_found_by_one_only": int(np.count_nonzero(found != reached)),
            "largest_difference_m": float(np.abs(near[both, 3].view(np.float32) - dist[both]).max()) if both.any() else 0.0}
    v = sensor_frame(verts)
    cnt = ranges(v, tris, origin, cell, dims, trunc)
    some = np.arange(0, tris.shape[0], SAMPLE)
    g = ref.grid(origin, cell, dims, trunc)
    sent = ref.counted(g, np.float32(v)[np.asarray(tris, np.int64)[some]])[0].shape[0]
    stats = {"triangles": int(tris.shape[0]), "triangles_in_reach_of_the_grid": int(np.count_nonzero(cnt)), "triangle_cell_pairs_tested": int(cnt.sum()),
             "counting_pairs_estimate": int(sent) * SAMPLE, "cells_within_trunc": int(np.count_nonzero(grids[SHIPPED] != ref.REST)), "cells": cells,
             "closest_points_agrees": same, "queued": {k: queued[k] for k in FORMS}}
    print(name, stats, flush=True)
    ev = {key: [] for key in forms}
    for _ in range(calls):
        for key, form in forms.items():    # alternating, call by call
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            call(form)
            b.record(st)
            ev[key].append((a, b))
        st.synchronize()
    us = {key: np.array([a.elapsed_time(b) * 1e3 for a, b in pairs]) for key, pairs in ev.items()}
    res = {key: {"median_us": float(np.median(x)), "min_us": float(x.min()), "max_us": float(x.max())} for key, x in us.items()}
    for key, r in res.items():
        print(name, key, "median %.1f us (%.1f - %.1f)" % (r["median_us"], r["min_us"], r["max_us"]), flush=True)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
    return {"grid": list(dims), "cell": cell, "trunc": trunc, "calls": calls, "stats": stats, "forms": res,
            "ratio_to_closest_points": res["(a) ls_closest_points"]["median_us"] / res[SHIPPED]["median_us"],
            "ratio_to_scene_grid": res[SHIPPED]["median_us"] / res["(b) ls_scene_grid"]["median_us"]}


out = {"library": os.environ.get("LS_LIB_PATH") or "shipped (the knobs are not read: every column is the shipped form)"}
bands = [float(x) for x in os.environ.get("DIST_GRID_COST_TRUNC", "0.6,1.6").split(",")]
mesh = synth.syn_1m()
for trunc in bands:
    out["trunc_%g" % trunc] = measure("SYN-1M trunc %g" % trunc, *mesh, (512, 512, 64), 0.2, trunc, 8)
if len(sys.argv) > 1:   # the figures as JSON, where the caller wants them
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out), flush=True)
if not os.environ.get("LS_LIB_PATH"):
    print("note: LS_LIB_PATH is not set -- the shipped library ignores the knobs, every column times the shipped form", flush=True)
