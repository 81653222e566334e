"""tools/label_cost.py [out.json] -- cost of ls_object_labels (EXPERIMENTS.md E20): SYN-128 x 4096 rays over the 100 000-triangle grid plus 16 posed copies of ben.
without the flag against ls_hit_attributes on the same records; with the flag against ls_trace_rays on the same rays.
Each figure: median of per-call device-event times over CALLS enqueued calls after WARM warm-up calls."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from lidarshooter_amd import capi, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

CALLS, WARM = 60, 10
DATA = os.path.join(ROOT, "tests", "golden", "data")
s0 = O.load_sensor(os.path.join(DATA, "config", "hesai-pandar-XT-32-lidar_0000.json"))
ben = O.load_stl(os.path.join(DATA, "mesh", "ben.stl"))
vertical = synth.syn_vertical(128)
tr = capi.Tracer(vertical, np.float32(0.0), np.float32(360.0), 4096, s0.Rinv, s0.t)
grid = synth.grid_mesh(250, 200)
assert tr.addGeometry("grid", grid[0].shape[0], grid[1].shape[0]) == 0
tr.updateGeometry("grid", capi.IDENTITY_AFFINE, *grid)
rng = np.random.default_rng(3)
for k in range(1, 17):
    A = O.affine_from_components(np.float32(rng.uniform(-15, 15, 3) * [1, 1, 0]), np.float32(rng.uniform(-1, 1, 3)))
    assert tr.addGeometry(f"ben{k}", ben[0].shape[0], ben[1].shape[0]) == k
    tr.updateGeometry(f"ben{k}", A, *ben)
assert tr.commitScene() == 0
rc, pts, hits = tr.traceScene(0)
assert rc == 0
n = hits.shape[0]
n_rays = tr.getTotalRays()
n_labels = 17
print("records", n, "rays", n_rays, "per geometry", np.bincount(hits["geom"], minlength=n_labels), flush=True)

dev = "cuda:0"
d_hits = torch.from_numpy(hits.view(np.uint8).reshape(-1).copy()).to(dev)
d_rays = torch.zeros(n_rays * 32, dtype=torch.uint8, device=dev)
d_attr = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
d_trace = torch.zeros(n_rays * 16, dtype=torch.uint8, device=dev)
d_lab = torch.zeros(n_labels * 64, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
tr.generateRaysAos(d_rays.data_ptr(), None)
tr.synchronize()
st = torch.cuda.Stream()
sp = st.cuda_stream


def timed(fn):
    for _ in range(WARM):
        fn()
    st.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
    for a, b in ev:
        a.record(st)
        fn()
        b.record(st)
    st.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return float(np.median(us)), float(us.min()), float(us.max())


calls = {
    "ls_hit_attributes": lambda: tr.hitAttributesDevice(d_hits.data_ptr(), n, d_attr.data_ptr(), stream=sp),
    "ls_object_labels, no flag": lambda: tr.objectLabelsDevice(d_lab.data_ptr(), n_labels, d_hits.data_ptr(), n, footprint=False, stream=sp),
    "ls_trace_rays": lambda: tr.traceRaysDevice(d_rays.data_ptr(), n_rays, d_trace.data_ptr(), stream=sp),
    "ls_object_labels, footprint, own rays": lambda: tr.objectLabelsDevice(d_lab.data_ptr(), n_labels, d_hits.data_ptr(), n, stream=sp),
    "ls_object_labels, footprint, caller rays": lambda: tr.objectLabelsDevice(d_lab.data_ptr(), n_labels, 0, 0, d_rays.data_ptr(), n_rays, stream=sp),
    "ls_occluded_rays": lambda: tr.occludedRaysDevice(d_rays.data_ptr(), n_rays, d_trace.data_ptr(), stream=sp),
}
res = {}
for rnd in range(2):   # every call twice, alternating: the second round shows the spread
    for name, fn in calls.items():
        assert fn() == 0
        res.setdefault(name, []).append(timed(fn))
        print(rnd, name, "median %.1f us (min %.1f, max %.1f)" % res[name][-1], flush=True)
lab = d_lab.cpu().numpy().view(capi.OBJECT_LABEL_DTYPE)
tr.objectLabelsDevice(d_lab.data_ptr(), n_labels, d_hits.data_ptr(), n, stream=sp)
st.synchronize()
lab = d_lab.cpu().numpy().view(capi.OBJECT_LABEL_DTYPE)
print("n_hits", lab["n_hits"], "n_alone", lab["n_alone"], flush=True)
assert int(lab["n_hits"].sum()) == n and np.all(lab["n_hits"] <= lab["n_alone"])
med = {k: float(np.median([x[0] for x in v])) for k, v in res.items()}
out = {"records": int(n), "rays": int(n_rays), "calls": CALLS, "rounds": res, "median_us": med,
       "ratio_no_flag_vs_hit_attributes": med["ls_object_labels, no flag"] / med["ls_hit_attributes"],
       "ratio_footprint_vs_trace_rays": med["ls_object_labels, footprint, own rays"] / med["ls_trace_rays"]}
if len(sys.argv) > 1:   # the figures as JSON, where the caller wants them
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out["median_us"]), out["ratio_no_flag_vs_hit_attributes"], out["ratio_footprint_vs_trace_rays"], flush=True)
assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
tr.close()
