"""tools/occupancy_cost.py [out.json] -- cost of ls_occupancy_grid and of its carve's two forms (EXPERIMENTS.md E21): bench.py's SYN-128 x
4096 raster over SYN-1M, a 512 x 512 x 64 grid of 0.2 m cells centred on the sensor, max_range 60 m, LS_OCC_CARVE_MISSES; the handle's
own rays and the frame's hit records where they lie.  The wave-aggregated form and the plain one-atomic-per-lane form run in one
process, alternating call by call, after a warm-up of both; each figure is the median (min - max) of per-call device-event times on
the call's stream.

The forms are selected by LS_VOXEL_AGGREGATE, which only a library built with EXPERIMENTAL=1 reads (csrc/ls_tuning.h):
    make -C lidarshooter_amd/csrc EXPERIMENTAL=1      (into a copy of the sources; the shipped library ignores the variable)
    LS_LIB_PATH=<that build>/liblidarshooter_hip.so python tools/occupancy_cost.py out.json
With the shipped library both columns time the shipped form; the tool says so."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from lidarshooter_amd import capi, hostapi, synth  # noqa: E402

CALLS, WARM = 24, 4
DATA = os.path.join(ROOT, "tests", "golden", "data")
d = hostapi.LidarDevice(os.path.join(DATA, "config", "hesai-pandar-XT-32-lidar_0000.json")).desc()
tr = capi.Tracer(synth.syn_vertical(128), np.float32(0.0), np.float32(360.0), 4096, d["Rinv"], d["t"])
v, t = synth.syn_1m()
assert tr.addGeometry("ground", v.shape[0], t.shape[0]) == 0
tr.updateGeometry("ground", capi.IDENTITY_AFFINE, v, t)
assert tr.commitScene() == 0
rc, pts, hits = tr.traceScene(0)
assert rc == 0
n, n_rays = hits.shape[0], tr.getTotalRays()
print("records", n, "rays", n_rays, flush=True)

dims = (512, 512, 64)
cell = 0.2
desc = capi.OccupancyGridDesc.make([-0.5 * dims[0] * cell, -0.5 * dims[1] * cell, -0.5 * dims[2] * cell], cell, dims, capi.LS_OCC_CARVE_MISSES, 0.0, 60.0)
cells = dims[0] * dims[1] * dims[2]
dev = "cuda:0"
d_hits = torch.from_numpy(hits.view(np.uint8).reshape(-1).copy()).to(dev)
d_counts = torch.zeros(cells * 2, dtype=torch.int32, device=dev)
d_geom = torch.zeros(cells, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
st = torch.cuda.Stream()
sp = st.cuda_stream


def call(form):
    os.environ["LS_VOXEL_AGGREGATE"] = form
    assert tr.occupancyGridDevice(desc, d_counts.data_ptr(), d_geom.data_ptr(), d_hits.data_ptr(), n, stream=sp) == 0


FORMS = {"aggregated": "1", "plain": "0"}
grids = {}
for name, form in FORMS.items():
    for _ in range(WARM):
        call(form)
    st.synchronize()
    grids[name] = (d_counts.cpu().numpy().copy(), d_geom.cpu().numpy().copy())
assert grids["aggregated"][0].tobytes() == grids["plain"][0].tobytes() and grids["aggregated"][1].tobytes() == grids["plain"][1].tobytes()
c = grids["plain"][0].view(np.uint32).reshape(-1, 2)
print("cells visited", int(np.count_nonzero(c[:, 0])), "cell visits", int(c[:, 0].sum(dtype=np.int64)), "occupied", int(np.count_nonzero(c[:, 1])),
      "returns in the grid", int(c[:, 1].sum(dtype=np.int64)), "busiest cell", int(c[:, 0].max()), flush=True)
ev = {name: [] for name in FORMS}
for _ in range(CALLS):
    for name, form in FORMS.items():       # alternating, call by call
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        call(form)
        b.record(st)
        ev[name].append((a, b))
st.synchronize()
us = {name: np.array([a.elapsed_time(b) * 1e3 for a, b in pairs]) for name, pairs in ev.items()}
res = {name: {"median_us": float(np.median(x)), "min_us": float(x.min()), "max_us": float(x.max())} for name, x in us.items()}
for name, r in res.items():
    print(name, "median %.1f us (%.1f - %.1f)" % (r["median_us"], r["min_us"], r["max_us"]), flush=True)
spread = max(r["max_us"] - r["min_us"] for r in res.values())
gain = res["plain"]["median_us"] - res["aggregated"]["median_us"]
experimental = os.environ.get("LS_LIB_PATH") is not None
out = {"records": int(n), "rays": int(n_rays), "grid": list(dims), "cell": cell, "calls": CALLS, "forms": res, "larger_spread_us": float(spread),
       "plain_minus_aggregated_us": float(gain), "aggregated_wins": bool(gain > spread), "cell_visits": int(c[:, 0].sum(dtype=np.int64)),
       "busiest_cell": int(c[:, 0].max()), "library": os.environ.get("LS_LIB_PATH") or "shipped (LS_VOXEL_AGGREGATE is not read: both columns are the shipped form)"}
if len(sys.argv) > 1:   # the figures as JSON, where the caller wants them
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out), flush=True)
if not experimental:
    print("note: LS_LIB_PATH is not set -- the shipped library ignores LS_VOXEL_AGGREGATE, both columns time the shipped form", flush=True)
assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
tr.close()
