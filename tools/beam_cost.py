"""ls_trace_scene_beams at SYN-1M: the beam call (k_beam_rays, the ray queries' walk, k_beam_reduce, k_beam_count + k_beam_pack) on
the SYN-128 x 4096 raster with S = 8 samples per beam, against ls_trace_rays alone on the same S x 524 288 sub-ray records
(restated on the host from the factor tables, the arithmetic of csrc/ls_beam.h in numpy float32) -- what the ray generation, the
echo reduction and the ordered pack add to the walk.  Both are timed with device events on a stream of their own, in alternating
rounds of the same length in one run, after a warm-up that also builds the query hierarchy.  Prints both times per call and
their ratio.  ls_trace_scene_beams_sweep (k_beam_sweep_rays, the walk, k_beam_reduce_weighted, k_beam_count + k_beam_sweep_pack)
runs in the same rounds, on the same model, in three legs: at rest with unit weights (what the weighted reduce and pack cost against
ls_trace_scene_beams), with a constant-twist pose table (unit weights), and with Gaussian weights (at rest).  For kernel times run
it under the profiler in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/beam_cost.py
usage: python tools/beam_cost.py [--rounds N] [--calls M] [--samples S]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sub_rays(st, ct, sp, cp, pat):
    """the 32-byte records of every sample of every ray, index (v * H + h) * S + s: float32 (V * H * S, 8)"""
    V, H, S = st.shape[0], sp.shape[0], pat.shape[0]
    stv, ctv = st[:, None, None], ct[:, None, None]
    cph, sph = cp[None, :, None], sp[None, :, None]
    a, b = pat[None, None, :, 0], pat[None, None, :, 1]
    r = np.zeros((V, H, S, 8), np.float32)
    r[..., 4] = (stv * cph + a * -sph) + b * -(ctv * cph)
    r[..., 5] = (stv * sph + a * cph) + b * -(ctv * sph)
    r[..., 6] = (ctv + a * np.float32(0.0)) + b * stv
    r[..., 4:7] = np.where(r[..., 4:7] == 0, np.float32(0.0), r[..., 4:7])
    r[..., 7] = np.float32(1e16)
    return r.reshape(-1, 8)


def main():
    import torch

    from lidarshooter_amd import capi, synth
    from oracle import oracle as O

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=10, help="calls per round (rounds x calls >= 50 timed calls of each)")
    ap.add_argument("--samples", type=int, default=8, help="S: the centre sample and one ring of S - 1")
    a = ap.parse_args()
    assert a.rounds * a.calls >= 50 and 2 <= a.samples <= 64
    base = O.load_sensor(os.path.join(ROOT, "tests", "golden", "data", "config", "hesai-pandar-XT-32-lidar_0000.json"))
    V, H, S = 128, 4096, a.samples
    verts, tris = synth.syn_1m()
    sensor = O.Sensor(uid="syn", vertical=synth.syn_vertical(V), h_begin=np.float32(0.0), h_end=np.float32(360.0), h_count=H, R=base.R,
                      Rinv=base.Rinv, t=base.t)
    tr = capi.Tracer(sensor.vertical, 0.0, 360.0, H, base.Rinv, base.t, device=0)
    assert tr.addGeometry("grid", verts.shape[0], tris.shape[0]) == 0
    tr.updateGeometry("grid", capi.IDENTITY_AFFINE, verts, tris)
    assert tr.commitScene() == 0
    n = tr.getTotalRays()
    assert n == V * H
    pat = capi.beam_pattern_rings(0.0015, 0.0015, 1, S - 1)      # 1.5 mrad half-angle
    model = capi.BeamModel(pat, capi.LS_BEAM_FIRST | capi.LS_BEAM_LAST | capi.LS_BEAM_STRONGEST, 2, 0.25)
    cap = 3 * n
    st, ct, sp, cp = O.ray_tables(sensor)
    d_rays = torch.from_numpy(sub_rays(st, ct, sp, cp, pat).view(np.uint8).reshape(-1)).to("cuda:0")
    d_dense = torch.zeros(n * S * 16, dtype=torch.uint8, device="cuda:0")
    d_points = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda:0")
    d_hits = torch.zeros(cap * 16, dtype=torch.uint8, device="cuda:0")
    d_echo = torch.zeros(cap * 4, dtype=torch.uint8, device="cuda:0")
    d_n = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()   # (a stream of its own: None would mean the handle's stream)

    def beams():
        assert tr.traceBeamsDevice(model, d_n.data_ptr(), cap, d_points.data_ptr(), d_hits.data_ptr(), d_echo.data_ptr(), stream=s.cuda_stream) == 0

    def rays_alone():
        assert tr.traceRaysDevice(d_rays.data_ptr(), n * S, d_dense.data_ptr(), s.cuda_stream) == 0

    # the legs of ls_trace_scene_beams_sweep: a carrier at about 10 m/s turning at about 1 rad/s, one turn in 0.1 s; sigma = the half-angle
    d_pose = torch.from_numpy(capi.sweep_poses_constant_twist((8.0, -5.0, 0.5), (0.1, -0.15, 1.0), 0.0, 0.1 / H, H)).to("cuda:0")
    gauss = capi.beam_weights_gaussian(pat, 0.0015, 0.0015)

    def sweep_leg(weights=None, pose=0):
        def run():
            assert tr.traceBeamsSweepDevice(model, d_n.data_ptr(), cap, d_points.data_ptr(), d_hits.data_ptr(), d_echo.data_ptr(), weights=weights,
                                            d_col_pose=pose, n_cols=H if pose else 0, stream=s.cuda_stream) == 0
        return run

    legs = [("ls_trace_scene_beams", beams), ("ls_trace_rays alone", rays_alone), ("beams_sweep at rest, unit weights", sweep_leg()),
            ("beams_sweep under a twist table", sweep_leg(pose=d_pose.data_ptr())), ("beams_sweep with Gaussian weights", sweep_leg(weights=gauss))]

    torch.cuda.synchronize()   # (the buffers' fills run on torch's stream: done before the handle's work starts)
    for _ in range(6):         # the first call builds the hierarchy; every leg is warmed up
        for _, fn in legs[2:] + legs[:2]:
            fn()
    torch.cuda.synchronize()
    k = int(d_n[0].item())   # (of the last warm-up call: ls_trace_scene_beams)
    dense = d_dense.cpu().numpy().view(np.uint32).reshape(n, S, 4)
    sub_hits = int(np.count_nonzero(dense[:, :, 1] != 0xFFFFFFFF))
    # the same sub-rays: every FIRST record is the nearest detectable echo of a beam with at least two sub-hits
    firsts = int(np.count_nonzero(d_echo.cpu().numpy().view(np.uint32)[:k] & 1))
    assert 0 < firsts <= int(np.count_nonzero((dense[:, :, 1] != 0xFFFFFFFF).sum(1) >= 2)), (firsts, k)
    times = [[] for _ in legs]
    t_beams, t_rays = times[0], times[1]
    for _ in range(a.rounds):
        for (_, fn), acc in zip(legs, times):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.calls):
                fn()
            e1.record(s)
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1) / a.calls * 1e3)
    be, ra = float(np.median(t_beams)), float(np.median(t_rays))
    print(f"SYN-128 x 4096 over SYN-1M, S = {S}: {n} beams, {n * S} sub-rays, {sub_hits} sub-hits, {k} returns, {a.rounds} rounds x {a.calls} calls each")
    print(f"ls_trace_scene_beams: median {be:.1f} us per call (rounds {min(t_beams):.1f} .. {max(t_beams):.1f})")
    print(f"ls_trace_rays alone:  median {ra:.1f} us per call (rounds {min(t_rays):.1f} .. {max(t_rays):.1f})")
    print(f"ratio {be / ra:.3f}: ray generation + reduction + count + pack add {be - ra:.1f} us to the walk")
    sweep = {}
    for (name, _), acc, key in zip(legs[2:], times[2:], ("sweep_rest", "sweep_twist", "sweep_gauss")):
        med = float(np.median(acc))
        print(f"{name}: median {med:.1f} us per call (rounds {min(acc):.1f} .. {max(acc):.1f}), {med / be:.3f} x ls_trace_scene_beams")
        sweep[key + "_us"], sweep[key + "_rounds_us"] = round(med, 2), [round(x, 2) for x in acc]
    print(json.dumps({"tool": "beam_cost", "beams": n, "samples": S, "sub_hits": sub_hits, "returns": k, "beams_us": round(be, 2),
                      "trace_rays_us": round(ra, 2), "ratio": round(be / ra, 4), "beams_rounds_us": [round(x, 2) for x in t_beams],
                      "rays_rounds_us": [round(x, 2) for x in t_rays], **sweep}))
    tr.close()


if __name__ == "__main__":
    main()
