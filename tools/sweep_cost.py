"""ls_trace_scene_sweep at SYN-1M: the sweep call (k_sweep_rays, the ray queries' walk, k_sweep_count + k_sweep_pack) on the
SYN-128 x 4096 raster under a constant twist, against ls_trace_rays alone on the same 524 288 ray records (the sweep's own
d_rays_out) -- what the ray generation and the ordered pack add to the walk.  Both are timed with device events on a stream of
their own, in alternating rounds of the same length in one run, after a warm-up that also builds the query hierarchy.  Prints
both times per call and their ratio.  For kernel times run it under the profiler in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/sweep_cost.py
usage: python tools/sweep_cost.py [--rounds N] [--calls M] [--deskew]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    assert tr.commitScene() == 0
    n = tr.getTotalRays()
    assert n == V * H
    pose = capi.sweep_poses_constant_twist((8.0, -5.0, 0.5), (0.1, -0.15, 1.0), 0.0, 0.1 / H, H)
    d_pose = torch.from_numpy(pose).to("cuda:0")
    d_points = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    d_n = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_dense = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    flags = capi.LS_SWEEP_DESKEW if a.deskew else 0
    s = torch.cuda.Stream()   # (a stream of its own: None would mean the handle's stream)

    def sweep(rays_out=0):
        assert tr.traceSweepDevice(d_pose.data_ptr(), H, d_n.data_ptr(), n, d_points.data_ptr(), d_hits.data_ptr(), rays_out, flags=flags,
                                   stream=s.cuda_stream) == 0

    def rays_alone():
        assert tr.traceRaysDevice(d_rays.data_ptr(), n, d_dense.data_ptr(), s.cuda_stream) == 0

    torch.cuda.synchronize()   # (the buffers' fills run on torch's stream: done before the handle's work starts)
    sweep(d_rays.data_ptr())   # the first call builds the hierarchy and leaves the ray records ls_trace_rays is timed on
    torch.cuda.synchronize()
    for _ in range(5):
        sweep()
        rays_alone()
    torch.cuda.synchronize()
    k = int(d_n[0].item())
    dense_hits = int(np.count_nonzero(d_dense.cpu().numpy().view(np.uint32).reshape(n, 4)[:, 1] != 0xFFFFFFFF))
    assert k == dense_hits, (k, dense_hits)
    t_sweep, t_rays = [], []
    for _ in range(a.rounds):
        for fn, acc in ((sweep, t_sweep), (rays_alone, t_rays)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.calls):
                fn()
            e1.record(s)
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1) / a.calls * 1e3)
    sw, ra = float(np.median(t_sweep)), float(np.median(t_rays))
    print(f"SYN-128 x 4096 over SYN-1M: {n} rays, {k} hits, {a.rounds} rounds x {a.calls} calls each, deskew {int(a.deskew)}")
    print(f"ls_trace_scene_sweep: median {sw:.1f} us per call (rounds {min(t_sweep):.1f} .. {max(t_sweep):.1f})")
    print(f"ls_trace_rays alone:  median {ra:.1f} us per call (rounds {min(t_rays):.1f} .. {max(t_rays):.1f})")
    print(f"ratio {sw / ra:.3f}: ray generation + count + pack add {sw - ra:.1f} us to the walk")
    print(json.dumps({"tool": "sweep_cost", "rays": n, "hits": k, "deskew": int(a.deskew), "sweep_us": round(sw, 2), "trace_rays_us": round(ra, 2),
                      "ratio": round(sw / ra, 4), "sweep_rounds_us": [round(x, 2) for x in t_sweep], "rays_rounds_us": [round(x, 2) for x in t_rays]}))
    tr.close()


if __name__ == "__main__":
    main()
