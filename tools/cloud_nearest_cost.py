"""tools/cloud_nearest_cost.py [out.json] -- cost of ls_cloud_nearest (EXPERIMENTS.md E26): bench.py's SYN-1M scene under the pose of
lidar_0000, the cloud the frame leaves (at most 524 288 32-byte points) against 2^20 records of ls_sample_surface on the same scene
(48 bytes each), radius 0.05, 0.2 and 1.0 m.  Per radius: the whole call; the index build alone (keys, sort, arrange); the query launch
as the difference of the two medians; next to them (a) a device copy of n_queries x 16 bytes plus a read of the queries on the same
stream -- the floor of the call's own traffic -- and (b) ls_closest_points over the same 2^20 points on the same handle: the nearest
existing query.  Each figure is the median (min - max) of 8 per-call device-event times on one caller stream after a warm-up, the forms
alternating call by call.  The first records are held to the numpy reference.

The build-alone form and the count of candidates examined per query are selected by LS_CLOUD_BUILD_ONLY and LS_CLOUD_COUNT, which only
a library built with EXPERIMENTAL=1 reads (csrc/ls_tuning.h):
    make -C lidarshooter_amd/csrc EXPERIMENTAL=1      (into a copy of the sources; the shipped library ignores the variables)
    LS_LIB_PATH=<that build>/liblidarshooter_hip.so python tools/cloud_nearest_cost.py out.json
With the shipped library the build-alone column times the whole call and no candidates are counted; the tool says so."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import cloud_nearest_reference as ref  # noqa: E402
from lidarshooter_amd import capi, hostapi, synth  # noqa: E402

WARM = 2
CALLS = 8
N_QUERIES = 1 << 20
CHECKED = 4096                             # records held to the reference
RADII = (0.05, 0.2, 1.0)
DATA = os.path.join(ROOT, "tests", "golden", "data")
d = hostapi.LidarDevice(os.path.join(DATA, "config", "hesai-pandar-XT-32-lidar_0000.json")).desc()
dev = "cuda:0"
experimental = bool(os.environ.get("LS_LIB_PATH"))


def med(x):
    return {"median_us": float(np.median(x)), "min_us": float(x.min()), "max_us": float(x.max())}


def measure(tr, d_cloud, n_cloud, d_q, d_pts16, radius):
    desc = capi.CloudNearestDesc.make(radius, 32, 48)
    d_out = torch.zeros(N_QUERIES * 16, dtype=torch.uint8, device=dev)
    d_copy = torch.zeros(N_QUERIES * 16, dtype=torch.uint8, device=dev)
    d_near = torch.zeros(N_QUERIES * 32, dtype=torch.uint8, device=dev)
    d_info = torch.zeros(16, dtype=torch.uint8, device=dev)
    q_words = d_q.view(torch.int32)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    sp = st.cuda_stream

    def call(form):
        os.environ["LS_CLOUD_BUILD_ONLY"] = "1" if form == "build" else "0"
        os.environ["LS_CLOUD_COUNT"] = "1" if form == "count" else "0"
        if form == "copy":
            with torch.cuda.stream(st):
                d_copy.copy_(d_out, non_blocking=True)
                q_words.sum()
        elif form == "closest":
            assert tr.closestPointsDevice(d_pts16.data_ptr(), N_QUERIES, d_near.data_ptr(), stream=sp) == 0
        else:
            assert tr.cloudNearestDevice(desc, d_cloud.data_ptr(), n_cloud, d_q.data_ptr(), N_QUERIES, d_out.data_ptr(), d_info.data_ptr(), stream=sp) == 0

    forms = {"whole call": "whole", "index build alone": "build", "(a) copy of n x 16 bytes + a read of the queries": "copy",
             "(b) ls_closest_points": "closest"}
    for form in forms.values():
        for _ in range(WARM):
            call(form)
    call("count")
    st.synchronize()
    examined = int(d_info.cpu().numpy().view(np.uint32)[3])
    call("whole")
    st.synchronize()
    info = d_info.cpu().numpy().view(ref.INFO_DTYPE)[0]
    rec = d_out.cpu().numpy().view(ref.DTYPE)
    ev = {key: [] for key in forms}
    for _ in range(CALLS):
        for key, form in forms.items():    # alternating, call by call
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            call(form)
            b.record(st)
            ev[key].append((a, b))
        st.synchronize()
    res = {key: med(np.array([a.elapsed_time(b) * 1e3 for a, b in pairs])) for key, pairs in ev.items()}
    res["query launch (whole - build)"] = {"median_us": res["whole call"]["median_us"] - res["index build alone"]["median_us"]} if experimental else None
    stats = {"radius": radius, "n_cloud": n_cloud, "n_queries": N_QUERIES, "n_found": int(info["n_found"]), "n_query_outside": int(info["n_query_outside"]),
             "n_cloud_indexed": int(info["n_cloud_indexed"]), "candidates_per_query": examined / N_QUERIES if experimental else None}
    print("radius", radius, stats, flush=True)
    for key, r in res.items():
        if r:
            print("radius", radius, key, "median %.1f us" % r["median_us"], ("(%.1f - %.1f)" % (r["min_us"], r["max_us"])) if "min_us" in r else "", flush=True)
    return {"calls": CALLS, "stats": stats, "forms": res}, rec[:CHECKED].copy()


out = {"library": os.environ.get("LS_LIB_PATH") or "shipped (the knobs are not read: the build-alone column is the whole call, no candidates counted)"}
verts, tris = synth.syn_1m()
tr = capi.Tracer(synth.syn_vertical(128), np.float32(0.0), np.float32(360.0), 4096, d["Rinv"], d["t"])
assert tr.addGeometry("ground", verts.shape[0], tris.shape[0]) == 0
tr.updateGeometry("ground", capi.IDENTITY_AFFINE, verts, tris)
assert tr.commitScene() == 0
rc, pts, hits = tr.traceScene(0)
assert rc == 0 and 0 < pts.shape[0] <= 524288
d_cloud = torch.from_numpy(np.ascontiguousarray(pts).reshape(-1)).to(dev)
d_q = torch.zeros(N_QUERIES * 48, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
assert tr.sampleSurfaceDevice(capi.SurfaceSampleDesc.make(N_QUERIES, seed=7), d_q.data_ptr()) == 0
tr.synchronize()
samples = d_q.cpu().numpy().view(capi.SURFACE_SAMPLE_DTYPE)
pts16 = np.concatenate([samples["p"], np.full((N_QUERIES, 1), np.inf, np.float32)], axis=1)
d_pts16 = torch.from_numpy(pts16.view(np.uint8).reshape(-1)).to(dev)
torch.cuda.synchronize()
cloud_xyz = np.ascontiguousarray(pts).reshape(-1, 32)[:, :12].copy().view(np.float32).reshape(-1, 3)
for radius in RADII:
    r, first = measure(tr, d_cloud, int(pts.shape[0]), d_q, d_pts16, radius)
    want, _ = ref.grid(cloud_xyz, samples["p"][:CHECKED], radius)
    assert first.tobytes() == want.tobytes(), "the records differ from the reference"
    r["records_equal_reference"] = CHECKED
    out["radius_%g" % radius] = r
assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
tr.close()
if len(sys.argv) > 1:   # the figures as JSON, where the caller wants them
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out), flush=True)
if not experimental:
    print("note: LS_LIB_PATH is not set -- the shipped library ignores the knobs: no build-alone split, no candidate count", flush=True)
