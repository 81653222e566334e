"""ls_trace_scene_sweep_moving at SYN-1M: the SYN-128 x 4096 raster under a constant twist over the SYN-1M grid plus one small mesh
(a box of 12 triangles above the grid) that crosses the field of view during the turn, against ls_trace_scene_sweep on the same
committed scene with the box frozen at its pose -- what the walk of ls_moving.hip (a record re-read and a 12-float table entry per
change of geometry) costs over the walk of ls_rays.hip.  Both are timed with device events on a stream of their own, in
alternating rounds of the same length in one run, after a warm-up that also builds the query hierarchies.  Prints both medians per
call and their ratio.  For kernel times run it under the profiler in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/moving_cost.py
usage: python tools/moving_cost.py [--rounds N] [--calls M] [--deskew]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def box(half):
    v = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], np.float32)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([tri for a, b, c, d in q for tri in ((a, b, c), (a, c, d))], np.uint32)


def main():
    import torch

    from lidarshooter_amd import capi, synth
    from oracle import oracle as O

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=10, help="calls per round (rounds x calls >= 50 timed calls of each)")
    ap.add_argument("--deskew", action="store_true")
    a = ap.parse_args()
    assert a.rounds * a.calls >= 50
    base = O.load_sensor(os.path.join(ROOT, "tests", "golden", "data", "config", "hesai-pandar-XT-32-lidar_0000.json"))
    V, H = 128, 4096
    verts, tris = synth.syn_1m()
    tr = capi.Tracer(synth.syn_vertical(V), 0.0, 360.0, H, base.Rinv, base.t, device=0)
    assert tr.addGeometry("grid", verts.shape[0], tris.shape[0]) == 0
    tr.updateGeometry("grid", capi.IDENTITY_AFFINE, verts, tris)
    bv, bt = box(1.5)
    car = tr.addGeometry("car", bv.shape[0], bt.shape[0])
    assert car == 1
    # 12 m from the sensor, level with it
    A = np.float32([1, 0, 0, base.t[0] + 12.0, 0, 1, 0, base.t[1], 0, 0, 1, base.t[2] - 1.0])
    tr.updateGeometry("car", A, bv, bt)
    assert tr.commitScene() == 0
    n = tr.getTotalRays()
    assert n == V * H
    pose = capi.sweep_poses_constant_twist((8.0, -5.0, 0.5), (0.1, -0.15, 1.0), 0.0, 0.1 / H, H)
    pivot = O.transform_vertices(bv, A, base).astype(np.float64).mean(0)
    motion = capi.motion_constant_twist((3.0, 15.0, 0.0), (0.0, 0.0, 0.5), pivot, 0.0, 0.1 / H, H)
    d_pose = torch.from_numpy(pose).to("cuda:0")
    d_motion = torch.from_numpy(motion).to("cuda:0")
    d_points = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    d_n = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    flags = capi.LS_SWEEP_DESKEW if a.deskew else 0
    s = torch.cuda.Stream()   # (a stream of its own: None would mean the handle's stream)

    def moving():
        assert tr.traceSweepMovingDevice(d_pose.data_ptr(), H, {car: d_motion.data_ptr()}, d_n.data_ptr(), n, d_points.data_ptr(), d_hits.data_ptr(),
                                         flags=flags, stream=s.cuda_stream) == 0

    def sweep():
        assert tr.traceSweepDevice(d_pose.data_ptr(), H, d_n.data_ptr(), n, d_points.data_ptr(), d_hits.data_ptr(), 0, flags=flags,
                                   stream=s.cuda_stream) == 0

    torch.cuda.synchronize()   # (the buffers' fills run on torch's stream: done before the handle's work starts)
    counts = {}
    for name, fn in (("sweep", sweep), ("moving", moving)):   # the first call builds the hierarchies
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        h = d_hits.cpu().numpy().view(np.uint32).reshape(n, 4)[:int(d_n[0].item())]
        counts[name] = (len(h), int(np.count_nonzero(h[:, 1] == car)))
    assert counts["moving"][1] > 0 and counts["sweep"][1] > 0, counts
    t_moving, t_sweep = [], []
    for _ in range(a.rounds):
        for fn, acc in ((moving, t_moving), (sweep, t_sweep)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.calls):
                fn()
            e1.record(s)
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1) / a.calls * 1e3)
    mv, sw = float(np.median(t_moving)), float(np.median(t_sweep))
    print(f"SYN-128 x 4096 over SYN-1M + a box of 12 triangles: {n} rays, {a.rounds} rounds x {a.calls} calls each, deskew {int(a.deskew)}")
    print(f"hits (all, on the box): moving {counts['moving']}, frozen {counts['sweep']}")
    print(f"ls_trace_scene_sweep_moving: median {mv:.1f} us per call (rounds {min(t_moving):.1f} .. {max(t_moving):.1f})")
    print(f"ls_trace_scene_sweep:        median {sw:.1f} us per call (rounds {min(t_sweep):.1f} .. {max(t_sweep):.1f})")
    print(f"ratio {mv / sw:.3f}: the moving box adds {mv - sw:.1f} us")
    print(json.dumps({"tool": "moving_cost", "rays": n, "hits_moving": counts["moving"][0], "hits_sweep": counts["sweep"][0], "deskew": int(a.deskew),
                      "moving_us": round(mv, 2), "sweep_us": round(sw, 2), "ratio": round(mv / sw, 4),
                      "moving_rounds_us": [round(x, 2) for x in t_moving], "sweep_rounds_us": [round(x, 2) for x in t_sweep]}))
    tr.close()


if __name__ == "__main__":
    main()
