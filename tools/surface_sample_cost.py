"""tools/surface_sample_cost.py [out.json] -- cost of ls_sample_surface and of the two forms of its bisection (EXPERIMENTS.md E25):
bench.py's SYN-1M scene under the pose of lidar_0000, 1 M and 16 M samples.  The forms -- the plain bisection over P in global memory,
and the one whose first ten levels run over 1025 entries of P staged in LDS -- run in one process, alternating call by call, after a
warm-up of both; next to them stand the set-up launches alone (the areas and the prefix: what every call pays before it draws), (a) a
device-to-device copy of n x 48 bytes on the same stream -- the floor of the output -- and (b) ls_scene_grid on the same scene over a
512 x 512 x 64 grid of 0.2 m cells: a pass over the same triangles.  Each figure is the median (min - max) of per-call device-event
times on one caller stream; a form's sample launch is its call minus the median of the set-up alone, and stands as a multiple of (a).
The records of the two forms are compared byte for byte, and a slice of them against the numpy reference.

The forms are selected by LS_SURFACE_LDS_TOP and LS_SURFACE_SETUP_ONLY, which only a library built with EXPERIMENTAL=1 reads
(csrc/ls_tuning.h):
    make -C lidarshooter_amd/csrc EXPERIMENTAL=1      (into a copy of the sources; the shipped library ignores the variables)
    LS_LIB_PATH=<that build>/liblidarshooter_hip.so python tools/surface_sample_cost.py out.json
With the shipped library every column times the shipped form; the tool says so."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import surface_sample_reference as ref  # noqa: E402
from lidarshooter_amd import capi, hostapi, synth  # noqa: E402

WARM = 2
CALLS = 8
SEED = 7
CHECKED = 4096                             # records held to the reference
DATA = os.path.join(ROOT, "tests", "golden", "data")
d = hostapi.LidarDevice(os.path.join(DATA, "config", "hesai-pandar-XT-32-lidar_0000.json")).desc()
dev = "cuda:0"
FORMS = {"plain": 0, "lds top": 1}


def sensor_frame64(verts):
    """the vertices in the sensor frame, in float64: for the area the info is held against"""
    R, t = np.float64(d["Rinv"]).reshape(3, 3), np.float64(d["t"])
    return (np.float64(verts) - t) @ R.T


def measure(name, tr, verts, tris, n):
    desc = capi.SurfaceSampleDesc.make(n, seed=SEED)
    sdesc = capi.SceneGridDesc.make([-51.2, -51.2, -6.4], 0.2, (512, 512, 64))
    d_out = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    d_copy = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    d_info = torch.zeros(16, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(512 * 512 * 64, dtype=torch.int32, device=dev)
    d_geom = torch.zeros(512 * 512 * 64, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    sp = st.cuda_stream

    def call(form):
        os.environ["LS_SURFACE_SETUP_ONLY"] = "1" if form == "setup" else "0"
        if form == "copy":
            with torch.cuda.stream(st):
                d_copy.copy_(d_out, non_blocking=True)
        elif form == "scene":
            assert tr.sceneGridDevice(sdesc, d_counts.data_ptr(), d_geom.data_ptr(), stream=sp) == 0
        else:
            os.environ["LS_SURFACE_LDS_TOP"] = str(0 if form == "setup" else form)
            assert tr.sampleSurfaceDevice(desc, d_out.data_ptr(), d_info.data_ptr(), stream=sp) == 0

    forms = dict(FORMS, **{"set-up alone": "setup", "(a) copy of n x 48 bytes": "copy", "(b) ls_scene_grid": "scene"})
    records = {}
    for key, form in forms.items():
        for _ in range(WARM):
            call(form)
        st.synchronize()
        if key in FORMS:
            records[key] = d_out.cpu().numpy().copy()
            d_out.zero_()
            torch.cuda.synchronize()
    for key in FORMS:
        assert records[key].tobytes() == records["plain"].tobytes(), key
    info = d_info.cpu().numpy().view(ref.INFO_DTYPE)[0]
    rec = records["plain"].view(ref.DTYPE)
    assert np.all(rec["flags"] == 1)
    stats = {"triangles": int(tris.shape[0]), "samples": n, "weight_total": int(info["weight_total"]), "exponent": int(info["exponent"]),
             "n_weighted": int(info["n_weighted"]), "area_m2": float(int(info["weight_total"])) * 2.0 ** int(info["exponent"]),
             "triangles_drawn": int(np.unique(rec["tri"]).shape[0])}
    print(name, stats, flush=True)
    ev = {key: [] for key in forms}
    for _ in range(CALLS):
        for key, form in forms.items():    # alternating, call by call
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            call(form)
            b.record(st)
            ev[key].append((a, b))
        st.synchronize()
    us = {key: np.array([a.elapsed_time(b) * 1e3 for a, b in pairs]) for key, pairs in ev.items()}
    res = {key: {"median_us": float(np.median(x)), "min_us": float(x.min()), "max_us": float(x.max())} for key, x in us.items()}
    setup, copy = res["set-up alone"]["median_us"], res["(a) copy of n x 48 bytes"]["median_us"]
    for key in FORMS:
        res[key]["sample_launch_us"] = res[key]["median_us"] - setup
        res[key]["sample_launch_in_copies"] = (res[key]["median_us"] - setup) / copy
    for key, r in res.items():
        print(name, key, "median %.1f us (%.1f - %.1f)" % (r["median_us"], r["min_us"], r["max_us"]),
              ("sample launch %.1f us = %.2f copies" % (r["sample_launch_us"], r["sample_launch_in_copies"])) if key in FORMS else "", flush=True)
    return {"calls": CALLS, "stats": stats, "forms": res, "records": rec[:CHECKED].copy()}


out = {"library": os.environ.get("LS_LIB_PATH") or "shipped (the knobs are not read: every column is the shipped form)"}
verts, tris = synth.syn_1m()
tr = capi.Tracer(synth.syn_vertical(128), np.float32(0.0), np.float32(360.0), 4096, d["Rinv"], d["t"])
assert tr.addGeometry("ground", verts.shape[0], tris.shape[0]) == 0
tr.updateGeometry("ground", capi.IDENTITY_AFFINE, verts, tris)
assert tr.commitScene() == 0
for n in (1 << 20, 1 << 24):
    r = measure("SYN-1M n = %d" % n, tr, verts, tris, n)
    first = r.pop("records")
    out["n_%d" % n] = r
assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
tr.close()
# the last call's first records against the reference (the oracle's transform is the device's, bit for bit), and the area in float64
from oracle import oracle as O  # noqa: E402
sensor = O.load_sensor(os.path.join(DATA, "config", "hesai-pandar-XT-32-lidar_0000.json"))
want, winfo = ref.scene_samples(O, [(0, verts, tris, O.IDENTITY_AFFINE)], sensor, None, None, capi.SurfaceSampleDesc.make(CHECKED, seed=SEED))
assert first.tobytes() == want.tobytes(), "the records differ from the reference"
q = sensor_frame64(verts)[np.asarray(tris, np.int64)]
area64 = float(0.5 * np.linalg.norm(np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), axis=1).sum())
out["area_float64_m2"] = area64
out["records_equal_reference"] = CHECKED
if len(sys.argv) > 1:   # the figures as JSON, where the caller wants them
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out), flush=True)
if not os.environ.get("LS_LIB_PATH"):
    print("note: LS_LIB_PATH is not set -- the shipped library ignores the knobs, every column times the shipped form", flush=True)
