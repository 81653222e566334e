"""ls_trace_rays at SYN-1M: the sensor's own 524 288 rays (SYN-128 raster) against the BVH frame's k_trace_inst on the same
scene in the same run, 1 M incoherent rays, and the first query's lazy build; then ls_occluded_rays against ls_trace_rays on
three ray sets -- the sensor's own rays, the 1 M incoherent rays, 1 M segments (origins 0.2-5 m above the ground, targets at
random scene points, tmax = 1 - 1e-4) -- whose occluded counts must equal the hit counts; then ls_closest_points on three point sets -- the frame's own cloud with
every point jittered by a few centimetres (cloud to mesh), 1 M points uniform in the scene's box, the same with a 0.5 m
radius -- next to ls_trace_rays on the incoherent rays; then ls_hit_attributes on the frame's own hit records (sensor-ray mode) and
on the hits of the 1 M incoherent rays, next to ls_trace_rays on those rays; then ls_apply_return_model on the same two record
sets.  Prints host-side event timings;
for kernel times (k_trace_rays, k_occluded_rays, k_closest_points, k_hit_attributes, k_returns_eval + k_returns_pack: their
launches come in the order of the sets, 1 + reps each) run it under the profiler in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ray_query_bench.py
usage: python tools/ray_query_bench.py [--reps N]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from lidarshooter_amd import capi, synth
    from oracle import oracle as O

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    base = O.load_sensor(os.path.join(ROOT, "tests", "golden", "data", "config", "hesai-pandar-XT-32-lidar_0000.json"))
    vert = synth.syn_vertical(128)
    verts, tris = synth.syn_1m()
    tr = capi.Tracer(vert, 0.0, 360.0, 4096, base.Rinv, base.t, device=0)
    tr.setOption(capi.LS_OPT_ENGINE, capi.ENGINE_BVH)
    assert tr.addGeometry("grid", verts.shape[0], tris.shape[0]) == 0
    tr.updateGeometry("grid", capi.IDENTITY_AFFINE, verts, tris)
    assert tr.commitScene() == 0
    for i in range(a.reps):   # BVH frames: k_trace_inst (the four-wide twins are made after the first frames)
        assert tr.traceScene(i)[0] == 0
    n = tr.getTotalRays()
    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    tr.generateRaysAos(d_rays.data_ptr(), None)
    out = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    tr.synchronize()
    t0 = time.perf_counter()
    assert tr.traceRaysDevice(d_rays.data_ptr(), n, out.data_ptr()) == 0
    tr.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    built = tr.info(capi.LS_INFO_RAY_QUERY_BUILT)

    def timed(rays, m, reps, query=tr.traceRaysDevice, out_bytes=16):
        o = torch.zeros(m * out_bytes, dtype=torch.uint8, device="cuda:0")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s = torch.cuda.Stream()   # (a stream of its own: 0 would mean the handle's stream)
        query(rays.data_ptr(), m, o.data_ptr(), s.cuda_stream)
        e0.record(s)
        for _ in range(reps):
            query(rays.data_ptr(), m, o.data_ptr(), s.cuda_stream)
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, o

    own_ms, o = timed(d_rays, n, a.reps)
    hits = int(np.count_nonzero(o.cpu().numpy().view(np.uint32).reshape(n, 4)[:, 1] != 0xFFFFFFFF))
    # 1 M incoherent rays: origins anywhere in the scene's box (sensor frame), directions uniform on the sphere
    rng = np.random.default_rng(1)
    m = 1 << 20
    r = np.zeros((m, 8), np.float32)
    R = np.asarray(base.Rinv, np.float64).reshape(3, 3)
    ow = np.c_[rng.uniform(-50, 50, (m, 2)), rng.uniform(0.2, 5.0, m)]
    r[:, 0:3] = (R @ (ow - np.asarray(base.t, np.float64)).T).T
    dw = rng.normal(size=(m, 3))
    r[:, 4:7] = (R @ (dw / np.linalg.norm(dw, axis=1)[:, None]).T).T
    r[:, 7] = np.inf
    d_inc = torch.from_numpy(r.view(np.uint8).reshape(-1)).to("cuda:0")
    inc_ms, o = timed(d_inc, m, a.reps)
    inc_hits = int(np.count_nonzero(o.cpu().numpy().view(np.uint32).reshape(m, 4)[:, 1] != 0xFFFFFFFF))
    print(f"first query (lazy build of {built} hierarchy + trace): {first_ms:.2f} ms host")
    print(f"sensor's own rays: {n} rays, {hits} hits, {own_ms * 1e3:.1f} us per query")
    print(f"incoherent rays: {m} rays, {inc_hits} hits, {inc_ms * 1e3:.1f} us per query = {m / inc_ms / 1e3:.0f} Mrays/s")
    # segments: from 0.2-5 m above the ground to random scene points (world frame, then the sensor frame as above)
    sr = np.zeros((m, 8), np.float32)
    ow = np.c_[rng.uniform(-50, 50, (m, 2)), rng.uniform(0.2, 5.0, m)]
    tw = verts[rng.integers(0, verts.shape[0], m)].astype(np.float64)
    sr[:, 0:3] = (R @ (ow - np.asarray(base.t, np.float64)).T).T
    sr[:, 4:7] = (R @ (tw - ow).T).T
    sr[:, 7] = 1.0 - 1e-4
    d_seg = torch.from_numpy(sr.view(np.uint8).reshape(-1)).to("cuda:0")
    # ls_occluded_rays against ls_trace_rays on the three sets, the same rays, the same run
    for name, rays, k in (("sensor's own rays", d_rays, n), ("incoherent rays", d_inc, m), ("segments", d_seg, m)):
        t_ms, o = timed(rays, k, a.reps)
        hit = int(np.count_nonzero(o.cpu().numpy().view(np.uint32).reshape(k, 4)[:, 1] != 0xFFFFFFFF))
        a_ms, o = timed(rays, k, a.reps, tr.occludedRaysDevice, 1)
        occ = int(np.count_nonzero(o.cpu().numpy()))
        assert occ == hit, (name, occ, hit)
        print(f"occlusion, {name}: {k} rays, {occ} occluded = {hit} hits; ls_trace_rays {t_ms * 1e3:.1f} us, "
              f"ls_occluded_rays {a_ms * 1e3:.1f} us per query ({a_ms / t_ms:.2f}x)")
    # ls_closest_points: the frame's own cloud jittered, points uniform in the scene's box, the same within 0.5 m
    rc, pts32, _ = tr.traceScene(0)
    assert rc == 0
    cloud = np.ascontiguousarray(pts32[:, :12]).view(np.float32).reshape(-1, 3)
    jit = np.zeros((cloud.shape[0], 4), np.float32)
    jit[:, :3] = cloud + rng.normal(scale=0.03, size=cloud.shape).astype(np.float32)
    jit[:, 3] = np.inf
    uni = np.zeros((m, 4), np.float32)
    pw = np.c_[rng.uniform(-50, 50, (m, 2)), rng.uniform(-0.5, 5.0, m)]
    uni[:, :3] = (R @ (pw - np.asarray(base.t, np.float64)).T).T
    uni[:, 3] = np.inf
    ball = uni.copy()
    ball[:, 3] = 0.5
    inc_ms, _ = timed(d_inc, m, a.reps)
    print(f"incoherent rays again: {inc_ms * 1e3:.1f} us per query")
    for name, pts in (("jittered cloud", jit), ("uniform in the box", uni), ("uniform, radius 0.5 m", ball)):
        k = pts.shape[0]
        d_pts = torch.from_numpy(pts.view(np.uint8).reshape(-1)).to("cuda:0")
        p_ms, o = timed(d_pts, k, a.reps, tr.closestPointsDevice, 32)
        rec = o.cpu().numpy().view(np.uint32).reshape(k, 8)
        found = rec[:, 4] != 0xFFFFFFFF
        dist = rec[found, 3].view(np.float32)
        print(f"closest points, {name}: {k} points, {int(np.count_nonzero(found))} found, mean dist {float(dist.mean()) if dist.size else 0:.4f} m; "
              f"ls_closest_points {p_ms * 1e3:.1f} us per query ({p_ms / inc_ms:.2f}x ls_trace_rays on {m} incoherent rays)")
    # ls_hit_attributes: the frame's hit records against the sensor's own rays, the incoherent rays' hits against those rays
    rc, _, fh = tr.traceScene(0)
    assert rc == 0
    d_fh = torch.from_numpy(np.ascontiguousarray(fh).view(np.uint8).reshape(-1)).to("cuda:0")
    inc_ms, o = timed(d_inc, m, a.reps)
    d_ih = o   # the incoherent rays' ls_hit records, misses included
    for name, d_h, k, rays, n_rays in (("frame hits, sensor rays", d_fh, fh.shape[0], 0, 0), ("incoherent rays' hits", d_ih, m, d_inc.data_ptr(), m)):
        q = lambda h, cnt, out_ptr, stream: tr.hitAttributesDevice(h, cnt, out_ptr, d_rays=rays, n_rays=n_rays, stream=stream)   # noqa: E731
        a_ms, o = timed(d_h, k, a.reps, q, 48)
        rec = o.cpu().numpy().view(capi.HIT_ATTR_DTYPE)
        valid = rec["flags"] == 1
        print(f"hit attributes, {name}: {k} records, {int(np.count_nonzero(valid))} valid, mean cos_inc {float(rec['cos_inc'][valid].mean()):.3f}; "
              f"ls_hit_attributes {a_ms * 1e3:.1f} us per query ({a_ms / inc_ms:.3f}x ls_trace_rays on {m} incoherent rays, {inc_ms * 1e3:.1f} us)")
    # ls_apply_return_model on the same two record sets: the gather again, the return model, the ordered compaction (k_returns_eval
    # + k_returns_pack, 1 + reps launches of each per set) -- to be read next to k_hit_attributes on those records, above
    model = capi.ReturnModel(flags=capi.LS_RETURN_LAMBERT, ref_range=10.0, intensity_floor=0.5, range_max=150.0, noise_sigma0=0.01,
                             noise_sigma1=0.001, dropout=0.05, seed=1)
    for name, d_h, k, rays, n_rays in (("frame hits, sensor rays", d_fh, fh.shape[0], 0, 0), ("incoherent rays' hits", d_ih, m, d_inc.data_ptr(), m)):
        d_ho = torch.zeros(k * 16, dtype=torch.uint8, device="cuda:0")
        d_no = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        q = lambda h, cnt, out_ptr, stream: tr.applyReturnModelDevice(model, h, cnt, d_no.data_ptr(), d_points32=out_ptr, d_hits_out=d_ho.data_ptr(),   # noqa: E731
                                                                      d_rays=rays, n_rays=n_rays, stream=stream)
        r_ms, o = timed(d_h, k, a.reps, q, 32)
        kept = int(d_no[0].item())
        inten = o.cpu().numpy().view(np.float32).reshape(-1, 8)[:kept, 4]
        print(f"return model, {name}: {k} records, {kept} kept, mean intensity {float(inten.mean()) if kept else 0:.2f}; "
              f"ls_apply_return_model {r_ms * 1e3:.1f} us per query ({r_ms / inc_ms:.3f}x ls_trace_rays on {m} incoherent rays, {inc_ms * 1e3:.1f} us)")
    tr.close()


if __name__ == "__main__":
    main()
