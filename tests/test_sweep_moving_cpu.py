"""ls_trace_scene_sweep_moving / ls_trace_scene_sweep_moving_host / ls_motion_constant_twist without a device: the symbols, the
refusal of a NULL handle, the ray a moving geometry sees (ls_debug_motion_ray, the host compilation of what k_trace_rays_moving
runs) against a restatement written here -- np.float32 operations in the stated order, bit for bit --, the constant-twist motion
table against Rodrigues' formula in numpy float64, and the pre-check of the GPU file's approximate test: the definition (the ray
through the inverse motion against the committed geometry) against a geometry re-posed per column, both through the oracle's
brute force alone."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_sweep_cpu import IDENTITY_POSE, restate_rays, rodrigues_poses

INVALID_ARGUMENT = -2
INV = 0xFFFFFFFF
F = np.float32


def _header(name="lidarshooter_hip.h"):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", name)).read())


# ---- the restatement and the reference by definition (shared with test_gpu_sweep_moving.py) ------------------------------------

def restate_motion_rays(rays, motion):
    """the ray records, float32 (n, 8), that a geometry under the motion records (n, 12) = [Q | c] row-major sees of the ray records
    rays (n, 8): e = o - c, o_g,i = (Q[0][i] e_0 + Q[1][i] e_1) + Q[2][i] e_2, d_g likewise -- every difference, product and sum
    rounded to float32 --, tmin 0, tmax 1e16"""
    r, p = np.asarray(rays, np.float32), np.asarray(motion, np.float32)
    out = np.zeros((r.shape[0], 8), np.float32)
    with np.errstate(all="ignore"):
        e = [r[:, i] - p[:, 4 * i + 3] for i in range(3)]
        for i in range(3):
            out[:, i] = (p[:, i] * e[0] + p[:, 4 + i] * e[1]) + p[:, 8 + i] * e[2]
            out[:, 4 + i] = (p[:, i] * r[:, 4] + p[:, 4 + i] * r[:, 5]) + p[:, 8 + i] * r[:, 6]
    out[:, 7] = F(1e16)
    return out


def contributions(oracle, brute, s, ml, rays, motions):
    """the definition, geometry by geometry: for every (geomID, verts, elems, affine) of ml, `brute` (test_gpu_rays._brute) over a
    scene that holds that geometry alone at its committed pose, with the ray records it sees -- rays (V * H, 8) at the global index,
    through the record of the ray's column where motions {geomID: (H, 12)} names the geometry -> {geomID: dense ls_hit records}"""
    cols = np.arange(rays.shape[0]) % s.H
    out = {}
    for gid, v, e, A in ml:
        seen = restate_motion_rays(rays, motions[gid][cols]) if gid in motions else rays
        out[gid] = brute(oracle, oracle.assemble_scene(s, [(gid, v, e, A)]), seen)
    return out


def merge(contrib, hidden=None):
    """the contribution with the smallest t per ray, the lowest (geomID, primID) among equals; hidden {geomID: bool per ray}: that
    geometry left out for those rays -> dense ls_hit records (ray, geom, prim, t bits)"""
    best = None
    for gid in sorted(contrib):
        rec = contrib[gid].copy()
        if hidden is not None and gid in hidden:
            rec[hidden[gid], 1:] = (INV, INV, F(-1.0).view(np.uint32))
        if best is None:
            best = rec
            continue
        hit, had = rec[:, 1] != INV, best[:, 1] != INV
        take = hit & (~had | (rec[:, 3].view(np.float32) < best[:, 3].view(np.float32)))
        best[take] = rec[take]
    return best


def small_sensor(oracle, V=8, H=16, begin=0.0, end=40.0, elev=21.0):
    """V x H rays around the +x axis of a handle whose sensor frame is the world frame (Rinv = I, t = 0)"""
    eye = np.eye(3, dtype=np.float32).reshape(9)
    return oracle.Sensor(uid="small", vertical=np.linspace(elev, -elev, V).astype(np.float32), h_begin=F(begin), h_end=F(end), h_count=H,
                         R=eye, Rinv=eye.copy(), t=np.zeros(3, np.float32))


def compose(motion12, affine12):
    """the pose [Q A | Q a + c] of a geometry committed at [A | a] and displaced by [Q | c]: float64, rounded once -> float32[12]"""
    D, A = np.asarray(motion12, np.float64).reshape(3, 4), np.asarray(affine12, np.float64).reshape(3, 4)
    out = np.zeros((3, 4))
    out[:, :3] = D[:, :3] @ A[:, :3]
    out[:, 3] = D[:, :3] @ A[:, 3] + D[:, 3]
    return out.reshape(12).astype(np.float32)


def yaw_case(oracle, capi, meshes):
    """GPU test 4 and its pre-check: ben 7 m in front of the small sensor, a plate behind it; ben yaws by 0.4 rad about its own
    centroid over the turn and drives on -> (sensor, meshes at their committed poses, ben's motion table, the nominal ray records)"""
    s = small_sensor(oracle)
    az = np.deg2rad(20.0)
    A_ben = np.float32([1, 0, 0, 7 * np.cos(az), 0, 1, 0, 7 * np.sin(az) - 1, 0, 0, 1, -2])
    plate = (np.float32([[30, -30, -30], [30, 40, -30], [30, 40, 30], [30, -30, 30]]), np.uint32([[0, 1, 2], [0, 2, 3]]))
    ml = [(0, *meshes["ben"], A_ben), (1, *plate, oracle.IDENTITY_AFFINE)]
    pivot = oracle.transform_vertices(meshes["ben"][0], A_ben, s).astype(np.float64).mean(0)
    turn = 0.1
    motion = capi.motion_constant_twist([3.0, -4.0, 1.0], [0.0, 0.0, 0.4 / turn], pivot, 0.0, turn / s.H, s.H)
    rays = restate_rays(oracle.ray_dirs(s), np.tile(IDENTITY_POSE, (s.V * s.H, 1)))
    return s, ml, motion, rays


def parity_misses(got, ref):
    """rays of two dense record sets that do not agree in (geom, prim) or whose t differs by more than 1e-4 t_ref"""
    t, tr = got[:, 3].view(np.float32).astype(np.float64), ref[:, 3].view(np.float32).astype(np.float64)
    same = (got[:, 1] == ref[:, 1]) & (got[:, 2] == ref[:, 2])
    hit = ref[:, 1] != INV
    return ~same | (hit & (np.abs(t - tr) > 1e-4 * tr))


# ---- exports and refusals ---------------------------------------------------------------------------------------------

def test_moving_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert capi.load().ls_abi_version() == 4      # the new entry points do not step the ABI version
    for s in ("ls_trace_scene_sweep_moving", "ls_trace_scene_sweep_moving_host", "ls_motion_constant_twist"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s
    assert "ls_debug_motion_ray" in capi.DEBUG_SYMBOLS and hasattr(lib, "ls_debug_motion_ray")
    hdr = _header()
    assert "#define LS_ABI_VERSION 4" in hdr
    assert re.search(r"typedef struct ls_geometry_motion \{ uint32_t geom; (/\*.*?\*/ )?uint32_t reserved; (/\*.*?\*/ )?const float \*col_motion; "
                     r"(/\*.*?\*/ )?\} ls_geometry_motion;", hdr)
    assert re.search(r"int ls_trace_scene_sweep_moving\(ls_tracer \*tr, void \*hip_stream, const float \*d_col_pose, uint32_t n_cols, "
                     r"const ls_geometry_motion \*motions, uint32_t n_motions, uint32_t flags, "
                     r"void \*d_points32, void \*d_hits, uint32_t \*d_n_points, uint32_t capacity\);", hdr)
    assert re.search(r"int ls_trace_scene_sweep_moving_host\(ls_tracer \*tr, const float \*col_pose, uint32_t n_cols, "
                     r"const ls_geometry_motion \*motions, uint32_t n_motions, uint32_t flags, "
                     r"void \*points32, void \*hits, uint32_t \*n_points, uint32_t capacity\);", hdr)
    assert re.search(r"int ls_motion_constant_twist\(const float lin_vel\[3\], const float ang_vel\[3\], const float pivot\[3\], double t0, double dt, "
                     r"uint32_t n_cols, float \*col_motion\);", hdr)
    assert re.search(r"int ls_debug_motion_ray\(const float ray8_in\[8\], const float motion12\[12\], float ray8_out\[8\]\);",
                     _header("lidarshooter_hip_debug.h"))
    assert ctypes.sizeof(capi.GeometryMotion) == 16 and capi.GeometryMotion.col_motion.offset == 8
    # what the header of the beams under a sweep called missing is offered now
    assert "geometries that move during the turn (without beams: ls_trace_scene_sweep_moving below)" in hdr


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    pose = np.tile(IDENTITY_POSE, (4, 1))
    m = (capi.GeometryMotion * 1)()
    m[0].geom, m[0].col_motion = 0, pose.ctypes.data
    n = ctypes.c_uint32(77)
    buf = np.zeros(64, np.uint8)
    assert L.ls_trace_scene_sweep_moving(None, None, pose.ctypes.data, 4, m, 1, 0, None, None, buf.ctypes.data, 4) == INVALID_ARGUMENT
    assert L.ls_trace_scene_sweep_moving_host(None, pose.ctypes.data, 4, m, 1, 0, None, None, ctypes.byref(n), 4) == INVALID_ARGUMENT
    assert L.ls_trace_scene_sweep_moving_host(None, None, 0, None, 0, 0, None, None, ctypes.byref(n), 4) == INVALID_ARGUMENT
    assert n.value == 77 and not buf.any()
    assert L.ls_debug_motion_ray(None, None, None) == INVALID_ARGUMENT


# ---- the ray a moving geometry sees ------------------------------------------------------------------------------------

def _random_records(rng, n):
    """rotations from random twists with offsets of some metres, some sheared or scaled records among them"""
    p = np.zeros((n, 12), np.float32)
    for k in range(n):
        p[k] = rodrigues_poses(rng.uniform(-20, 20, 3), rng.uniform(-3, 3, 3), rng.uniform(0, 0.1), 0.0, 1)[0]
    p[::11] += rng.normal(size=(len(p[::11]), 12)).astype(np.float32)
    return p


def test_motion_ray_equals_the_restatement(capi):
    rng = np.random.default_rng(20251)
    n = 10000
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = rng.normal(size=(n, 3)) * 10
    rays[:, 4:7] = rng.normal(size=(n, 3))
    rays[::7, 4:7] *= F(1e-3)
    rays[::5, 0:3] = 0          # the sensor at rest
    rays[:, 3], rays[:, 7] = rng.uniform(0, 1, n), F(1e16)      # (tmin in is ignored: the record out has tmin 0)
    motion = _random_records(rng, n)
    want = restate_motion_rays(rays, motion)
    got = np.stack([capi.motion_ray(rays[k], motion[k]) for k in range(n)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(got[:, 3] == 0) and np.all(got[:, 7] == F(1e16))
    # forward against inverse: the ray seen through [Q | c], carried forward again, is the ray (rotations only, to rounding)
    rot = np.ones(n, bool)
    rot[::11] = False
    Q, c = motion[rot].reshape(-1, 3, 4)[:, :, :3].astype(np.float64), motion[rot].reshape(-1, 3, 4)[:, :, 3].astype(np.float64)
    back_o = np.einsum("nij,nj->ni", Q, got[rot, 0:3].astype(np.float64)) + c
    back_d = np.einsum("nij,nj->ni", Q, got[rot, 4:7].astype(np.float64))
    assert np.max(np.abs(back_o - rays[rot, 0:3])) < 1e-4 and np.max(np.abs(back_d - rays[rot, 4:7])) < 1e-5


def test_identity_record_returns_the_ray_and_a_nan_propagates(capi):
    rng = np.random.default_rng(4)
    for k in range(200):
        r = np.zeros(8, np.float32)
        r[0:3], r[4:7], r[7] = rng.normal(size=3) * 5, rng.normal(size=3), F(1e16)
        g = capi.motion_ray(r, IDENTITY_POSE)
        assert np.array_equal(g, r)
    # a non-finite entry leaves a non-finite origin or direction: the geometry is invisible to that ray
    r = F([0.5, -1.5, 2.0, 0.0, 0.3, -0.2, 0.9, 1e16])
    for k in range(12):
        for bad in (np.nan, np.inf, -np.inf):
            p = IDENTITY_POSE.copy()
            p[k] = bad
            g = capi.motion_ray(r, p)
            assert not np.all(np.isfinite(g[[0, 1, 2, 4, 5, 6]]))
            assert np.array_equal(g.view(np.uint32), restate_motion_rays(r[None], p[None])[0].view(np.uint32))
    # a NaN in the ray propagates as well
    for k in (0, 1, 2, 4, 5, 6):
        bad = r.copy()
        bad[k] = np.nan
        assert np.isnan(capi.motion_ray(bad, IDENTITY_POSE)[k])


# ---- the constant-twist motion table -----------------------------------------------------------------------------------

def _rodrigues_motion(lin, ang, pivot, t0, dt, n):
    """rodrigues_poses with c_h = pivot - Q_h pivot + lin * tau_h: float64 (n, 12)"""
    ref = rodrigues_poses(lin, ang, t0, dt, n)
    piv = np.asarray(pivot, np.float32).astype(np.float64)
    P = ref.reshape(n, 3, 4)
    P[:, :, 3] += piv - P[:, :, :3] @ piv
    return ref


@pytest.mark.parametrize("lin,ang,pivot,t0,dt,n", [
    ((10.0, -4.0, 0.5), (0.1, -0.2, 1.0), (3.0, -7.0, 1.5), 0.0, 0.1 / 150, 150),
    ((-7.5, 12.0, 0.0), (0.9, 0.4, -0.6), (-20.0, 4.0, 0.25), 0.02, 0.1 / 96, 96),
    ((1.0, 2.0, 3.0), (2.5, -1.5, 3.0), (0.5, 0.5, -0.5), -0.05, 1e-3, 257),
])
def test_motion_twist_equals_rodrigues(capi, lin, ang, pivot, t0, dt, n):
    """the comparison of test_sweep_cpu for the sensor's table: every entry within 1 float32 ulp of the float64 evaluation (one
    rounding of a double result whose libm sin / cos may differ from numpy's in the last double bit -- the offsets' double error,
    some 1e-16 of the pivot, is far below a float32 ulp of the offsets here); the rotations orthonormal to 1e-6"""
    got = capi.motion_constant_twist(lin, ang, pivot, t0, dt, n)
    ref = _rodrigues_motion(lin, ang, pivot, t0, dt, n)
    ref32 = ref.astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(ref32), np.abs(got)))
    assert np.all(np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= ulp)
    R = got.reshape(n, 3, 4)[:, :, :3].astype(np.float64)
    assert np.max(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3))) <= 1e-6
    assert np.all(np.abs(np.linalg.det(R) - 1.0) <= 1e-6)
    # the pivot stays where the drive alone takes it: Q pivot + c = pivot + lin * tau
    tau = t0 + dt * np.arange(n)
    moved = R @ np.asarray(pivot, np.float64) + got.reshape(n, 3, 4)[:, :, 3]
    assert np.max(np.abs(moved - (np.asarray(pivot, np.float64) + np.outer(tau, np.asarray(lin, np.float64))))) < 1e-5


def test_zero_pivot_is_the_sensor_table_and_tau_zero_the_identity(capi):
    for lin, ang, t0, dt, n in (((10.0, -4.0, 0.5), (0.1, -0.2, 1.0), 0.0, 0.1 / 150, 150), ((-7.5, 12.0, -0.0), (0.9, 0.4, -0.6), 0.02, 1e-3, 96),
                                ((-3.0, 2.0, -1.0), (0.0, 0.0, 0.0), 0.0, 0.25, 8)):
        a = capi.motion_constant_twist(lin, ang, (0, 0, 0), t0, dt, n)
        b = capi.sweep_poses_constant_twist(lin, ang, t0, dt, n)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # tau = 0: exactly the identity, whatever the pivot
    p = capi.motion_constant_twist([3, -2, 1], [0.4, 0.1, -1.0], [5.0, -6.0, 7.0], 0.0, 1e-3, 8)
    assert np.array_equal(p[0], IDENTITY_POSE) and not np.array_equal(p[1], IDENTITY_POSE)
    p = capi.motion_constant_twist([0, 0, 0], [0, 0, 0], [5.0, -6.0, 7.0], 0.3, 1e-3, 150)
    assert np.array_equal(p.view(np.uint32), np.tile(IDENTITY_POSE, (150, 1)).view(np.uint32))


def test_motion_twist_refuses_bad_input(capi):
    L = capi.load()
    f32p = ctypes.POINTER(ctypes.c_float)
    out = np.full((4, 12), 7.0, np.float32)
    ok = np.float32([1, 2, 3])

    def call(lin, ang, piv, t0, dt, dst=out):
        return L.ls_motion_constant_twist(*(None if a is None else a.ctypes.data_as(f32p) for a in (lin, ang, piv)), t0, dt, 4,
                                          None if dst is None else dst.ctypes.data_as(f32p))

    assert call(ok, ok, ok, 0.0, 0.1) == 0
    out[:] = 7.0
    for k in range(3):
        for bad in (np.nan, np.inf):
            v = ok.copy()
            v[k] = bad
            assert call(v, ok, ok, 0.0, 0.1) == INVALID_ARGUMENT and call(ok, v, ok, 0.0, 0.1) == INVALID_ARGUMENT
            assert call(ok, ok, v, 0.0, 0.1) == INVALID_ARGUMENT
    assert call(ok, ok, ok, float("nan"), 0.1) == INVALID_ARGUMENT and call(ok, ok, ok, 0.0, float("inf")) == INVALID_ARGUMENT
    assert call(None, ok, ok, 0.0, 0.1) == INVALID_ARGUMENT and call(ok, None, ok, 0.0, 0.1) == INVALID_ARGUMENT
    assert call(ok, ok, None, 0.0, 0.1) == INVALID_ARGUMENT and call(ok, ok, ok, 0.0, 0.1, None) == INVALID_ARGUMENT
    assert np.all(out == 7.0)      # a refusal writes nothing
    with pytest.raises(capi.LidarShooterHipError):
        capi.motion_constant_twist([np.nan, 0, 0], [0, 0, 0], [0, 0, 0], 0.0, 0.1, 4)


# ---- the pre-check of the approximate GPU test ---------------------------------------------------------------------------

def test_definition_against_reposed_geometry_in_the_oracle_alone(oracle, capi, meshes):
    """test_gpu_sweep_moving.test_general_rotation_equals_reposing compares the call with a geometry re-posed per column and allows
    1 % of the rays to differ.  Both sides through the oracle's brute force on the CPU: the reference alone must stay inside that --
    measured: 0 of 128 rays differ, the largest |t - t_ref| / t_ref is 9.8e-7.  A transposed Q misses by a wide margin."""
    from test_gpu_rays import _brute
    s, ml, motion, rays = yaw_case(oracle, capi, meshes)
    n, cols = s.V * s.H, np.arange(s.V * s.H) % s.H
    by_definition = merge(contributions(oracle, _brute, s, ml, rays, {0: motion}))
    reposed = np.zeros((n, 4), np.uint32)
    for h in range(s.H):
        scene = oracle.assemble_scene(s, [(0, *ml[0][1:3], compose(motion[h], ml[0][3])), ml[1]])
        mine = np.nonzero(cols == h)[0]
        reposed[mine] = _brute(oracle, scene, rays[mine])
        reposed[mine, 0] = mine
    on_ben = np.count_nonzero(reposed[:, 1] == 0)
    assert on_ben >= n // 2 and np.count_nonzero(reposed[:, 1] == 1) >= 8      # ben and the plate behind it are both seen
    miss = parity_misses(by_definition, reposed)
    t, tr = by_definition[~miss, 3].view(np.float32).astype(np.float64), reposed[~miss, 3].view(np.float32).astype(np.float64)
    print("rays that differ:", np.count_nonzero(miss), "of", n, " largest relative t difference:", np.max(np.abs(t - tr) / tr))
    assert np.count_nonzero(miss) <= n // 100
    # the motion matters, and its direction: the static scene and a transposed Q are far outside the bound
    static = merge(contributions(oracle, _brute, s, ml, rays, {}))
    assert np.count_nonzero(parity_misses(static, reposed)) > n // 4
    wrong = motion.copy().reshape(-1, 3, 4)
    wrong[:, :, :3] = wrong[:, :, :3].transpose(0, 2, 1)
    transposed = merge(contributions(oracle, _brute, s, ml, rays, {0: wrong.reshape(-1, 12)}))
    assert np.count_nonzero(parity_misses(transposed, reposed)) > n // 4
