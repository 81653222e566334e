"""tools/scene_grid_cost.py [out.json] -- cost of ls_scene_grid and of its two tunables (EXPERIMENTS.md E22): bench.py's SYN-1M scene under
the SYN-128 sensor's pose, a 512 x 512 x 64 grid of 0.2 m cells centred on the sensor, counts and geom.  The forms -- the small / big
threshold at 8, 64, 512 and at a value so large that nothing is queued (one lane per triangle whatever its range: the baseline), and
the small path's atomics plain or aggregated per run of lanes -- run in one process, alternating call by call, after a warm-up of
all of them; each figure is the median (min - max) of per-call device-event times on the call's stream.  The clear alone
(LS_SCENE_GRID_CLEAR_ONLY) is the floor, and a call with nothing selected (the clear and two launches that find no work) stands next to it.  The grids of all forms are compared byte for byte.

A second scene shows what the queue is for: the same relief as 162 triangles of 11 m (synth.grid_mesh(9, 9)) under a 2048 x 2048 x 16
grid of 0.05 m cells around the ground's height, where every triangle's range holds tens of thousands of cells.

The forms are selected by LS_SCENE_GRID_SMALL, LS_SCENE_GRID_AGGREGATE and LS_SCENE_GRID_CLEAR_ONLY, which only a library built with EXPERIMENTAL=1 reads
(csrc/ls_tuning.h):
    make -C lidarshooter_amd/csrc EXPERIMENTAL=1      (into a copy of the sources; the shipped library ignores the variables)
    LS_LIB_PATH=<that build>/liblidarshooter_hip.so python tools/scene_grid_cost.py out.json
With the shipped library every column times the shipped form; the tool says so."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from lidarshooter_amd import capi, hostapi, synth  # noqa: E402

CALLS, WARM = 24, 3
NONE_QUEUED = 1 << 27                      # no range holds more cells than a grid may have
DATA = os.path.join(ROOT, "tests", "golden", "data")
d = hostapi.LidarDevice(os.path.join(DATA, "config", "hesai-pandar-XT-32-lidar_0000.json")).desc()
dev = "cuda:0"
# (threshold, aggregate): the threshold's candidates with plain atomics, then the aggregated atomics at the shipped threshold
FORMS = {"small=8": (8, 0), "small=64": (64, 0), "small=512": (512, 0), "nothing queued": (NONE_QUEUED, 0), "small=64 aggregated": (64, 1)}


def ranges(verts, tris, origin, cell, dims):
    """the cells of every triangle's clamped range, estimated in float64 for the number of (triangle, cell) tests (the library's own
    arithmetic is float32: a triangle on a boundary may count one layer more or less; the queue's length is read from the device)
    -> int64[n]"""
    R, t = np.float64(d["Rinv"]).reshape(3, 3), np.float64(d["t"])
    v = (np.float64(verts) - t) @ R.T - np.float64(origin)
    q = v[np.asarray(tris, np.int64)] / cell
    lo, hi = np.floor(q.min(axis=1)), np.floor(q.max(axis=1))
    n = np.float64(dims)
    inside = np.all((hi >= 0) & (lo < n), axis=1)
    w = np.clip(hi, 0, n - 1) - np.clip(lo, 0, n - 1) + 1
    return np.where(inside, w.prod(axis=1), 0).astype(np.int64)


def measure(name, verts, tris, dims, cell, calls, centre_z=0.0):
    tr = capi.Tracer(synth.syn_vertical(128), np.float32(0.0), np.float32(360.0), 4096, d["Rinv"], d["t"])
    assert tr.addGeometry("ground", verts.shape[0], tris.shape[0]) == 0
    tr.updateGeometry("ground", capi.IDENTITY_AFFINE, verts, tris)
    assert tr.commitScene() == 0
    origin = [-0.5 * dims[0] * cell, -0.5 * dims[1] * cell, centre_z - 0.5 * dims[2] * cell]
    desc = capi.SceneGridDesc.make(origin, cell, dims)
    cells = dims[0] * dims[1] * dims[2]
    d_counts = torch.zeros(cells, dtype=torch.int32, device=dev)
    d_geom = torch.zeros(cells, dtype=torch.int32, device=dev)
    d_none = torch.zeros(16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    sp = st.cuda_stream

    def call(form):
        os.environ["LS_SCENE_GRID_CLEAR_ONLY"] = "1" if form == "clear" else "0"
        if form in ("clear", "none"):      # the clear alone: the floor; nothing selected: the clear and two launches that find no work
            assert tr.sceneGridDevice(desc, d_counts.data_ptr(), d_geom.data_ptr(), d_none.data_ptr(), 1, stream=sp) == 0
            return
        os.environ["LS_SCENE_GRID_SMALL"], os.environ["LS_SCENE_GRID_AGGREGATE"] = str(form[0]), str(form[1])
        assert tr.sceneGridDevice(desc, d_counts.data_ptr(), d_geom.data_ptr(), stream=sp) == 0

    forms = dict(FORMS, **{"nothing selected": "none", "clear alone": "clear"})
    grids, queued = {}, {}
    for key, form in forms.items():
        for _ in range(WARM):
            call(form)
        st.synchronize()
        grids[key] = (d_counts.cpu().numpy().copy(), d_geom.cpu().numpy().copy())
        n_q = ctypes.c_uint32(0)
        assert tr.L.ls_debug_scene_grid_queued(tr.h, ctypes.byref(n_q)) == 0
        queued[key] = int(n_q.value)       # the device's own count word
    for key in FORMS:
        assert grids[key][0].tobytes() == grids["small=64"][0].tobytes() and grids[key][1].tobytes() == grids["small=64"][1].tobytes(), key
    assert not grids["nothing selected"][0].any() and not grids["clear alone"][0].any()
    c = grids["small=64"][0].view(np.uint32)
    cnt = ranges(verts, tris, origin, cell, dims)
    stats = {"triangles": int(tris.shape[0]), "triangles_in_the_grid": int(np.count_nonzero(cnt)), "triangle_cell_tests": int(cnt.sum()),
             "marks": int(c.sum(dtype=np.int64)), "marked_cells": int(np.count_nonzero(c)), "busiest_cell": int(c.max()),
             "queued": {k: queued[k] for k in FORMS}}
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
    return {"grid": list(dims), "cell": cell, "calls": calls, "stats": stats, "forms": res}


out = {"library": os.environ.get("LS_LIB_PATH") or "shipped (the knobs are not read: every column is the shipped form)"}
out["syn_1m"] = measure("SYN-1M", *synth.syn_1m(), (512, 512, 64), 0.2, CALLS)
out["coarse"] = measure("coarse", *synth.grid_mesh(9, 9), (2048, 2048, 16), 0.05, 8, centre_z=-float(d["t"][2]))


def decide(forms, a, b):
    """whether form a is below form b by more than the larger of the two spreads"""
    spread = max(forms[a]["max_us"] - forms[a]["min_us"], forms[b]["max_us"] - forms[b]["min_us"])
    return {"gain_us": forms[b]["median_us"] - forms[a]["median_us"], "larger_spread_us": spread,
            "wins": bool(forms[b]["median_us"] - forms[a]["median_us"] > spread)}


for scene in ("syn_1m", "coarse"):
    f = out[scene]["forms"]
    out[scene]["aggregated_against_plain"] = decide(f, "small=64 aggregated", "small=64")
    out[scene]["queue_against_none"] = {k: decide(f, k, "nothing queued") for k in ("small=8", "small=64", "small=512")}
if len(sys.argv) > 1:   # the figures as JSON, where the caller wants them
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out), flush=True)
if not os.environ.get("LS_LIB_PATH"):
    print("note: LS_LIB_PATH is not set -- the shipped library ignores the knobs, every column times the shipped form", flush=True)
