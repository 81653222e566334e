"""ls_trace_scene_sweep / ls_trace_scene_sweep_host / ls_sweep_poses_constant_twist without a device: the symbols, the refusal of a
NULL handle, the ray of a column (ls_debug_sweep_ray, the host compilation of what k_sweep_rays runs) against a restatement
written here -- np.float32 operations in the stated order, bit for bit --, and the constant-twist pose table against Rodrigues'
formula in numpy float64."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

INVALID_ARGUMENT = -2
F = np.float32
IDENTITY_POSE = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])


def _header(name="lidarshooter_hip.h"):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", name)).read())


# ---- the restatements (shared with test_gpu_sweep.py) -------------------------------------------------------------------

def restate_rays(d, pose):
    """the sweep's ray records, float32 (n, 8), of nominal directions d (n, 3) under pose records (n, 12) = [R | o] row-major:
    origin o, tmin 0, d'_i = (R[i][0] dx + R[i][1] dy) + R[i][2] dz -- every product and sum rounded to float32 --, tmax 1e16"""
    d, p = np.asarray(d, np.float32), np.asarray(pose, np.float32)
    r = np.zeros((d.shape[0], 8), np.float32)
    with np.errstate(all="ignore"):
        for i in range(3):
            r[:, i] = p[:, 4 * i + 3]
            r[:, 4 + i] = (p[:, 4 * i] * d[:, 0] + p[:, 4 * i + 1] * d[:, 1]) + p[:, 4 * i + 2] * d[:, 2]
    r[:, 7] = F(1e16)
    return r


def rodrigues_poses(lin_vel, ang_vel, t0, dt, n):
    """tau_h = t0 + h dt; R_h = I + sin(a) K + (1 - cos(a)) K^2 for the rotation ang_vel * tau_h, o_h = lin_vel * tau_h: float64 (n, 12)"""
    lin, w = np.asarray(lin_vel, np.float32).astype(np.float64), np.asarray(ang_vel, np.float32).astype(np.float64)
    out = np.zeros((n, 12))
    wn = np.linalg.norm(w)
    for h in range(n):
        tau = t0 + h * dt
        a = wn * tau
        R = np.eye(3)
        if a != 0.0:
            k = w / wn
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            R = np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)
        P = out[h].reshape(3, 4)
        P[:, :3] = R
        P[:, 3] = lin * tau
    return out


# ---- exports and refusals ---------------------------------------------------------------------------------------------

def test_sweep_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert capi.load().ls_abi_version() == 4      # the new entry points do not step the ABI version
    for s in ("ls_trace_scene_sweep", "ls_trace_scene_sweep_host", "ls_sweep_poses_constant_twist"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s
    assert "ls_debug_sweep_ray" in capi.DEBUG_SYMBOLS and hasattr(lib, "ls_debug_sweep_ray")
    hdr = _header()
    assert "#define LS_ABI_VERSION 4" in hdr and "#define LS_SWEEP_DESKEW 1u" in hdr and capi.LS_SWEEP_DESKEW == 1
    assert re.search(r"int ls_trace_scene_sweep\(ls_tracer \*tr, void \*hip_stream, const float \*d_col_pose, uint32_t n_cols, uint32_t flags, "
                     r"void \*d_points32, void \*d_hits, uint32_t \*d_n_points, uint32_t capacity, void \*d_rays_out\);", hdr)
    assert re.search(r"int ls_trace_scene_sweep_host\(ls_tracer \*tr, const float \*col_pose, uint32_t n_cols, uint32_t flags, "
                     r"void \*points32, void \*hits, uint32_t \*n_points, uint32_t capacity, void \*rays_out\);", hdr)
    assert re.search(r"int ls_sweep_poses_constant_twist\(const float lin_vel\[3\], const float ang_vel\[3\], double t0, double dt, "
                     r"uint32_t n_cols, float \*col_pose\);", hdr)
    assert re.search(r"int ls_debug_sweep_ray\(const float d\[3\], const float pose12\[12\], float ray8\[8\]\);", _header("lidarshooter_hip_debug.h"))


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    pose = np.tile(IDENTITY_POSE, (4, 1))
    n = ctypes.c_uint32(77)
    buf = np.zeros(64, np.uint8)
    assert L.ls_trace_scene_sweep(None, None, pose.ctypes.data, 4, 0, None, None, buf.ctypes.data, 4, None) == INVALID_ARGUMENT
    assert L.ls_trace_scene_sweep_host(None, pose.ctypes.data, 4, 0, None, None, ctypes.byref(n), 4, None) == INVALID_ARGUMENT
    assert n.value == 77 and not buf.any()
    assert L.ls_debug_sweep_ray(None, None, None) == INVALID_ARGUMENT


# ---- the ray of a column ----------------------------------------------------------------------------------------------

def test_sweep_ray_equals_the_restatement(capi):
    rng = np.random.default_rng(20250)
    n = 10000
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[::7] *= F(1e-3)
    pose = np.zeros((n, 12), np.float32)
    # rotations (from random twists), some sheared or scaled records among them: the arithmetic does not care
    for k in range(n):
        pose[k] = rodrigues_poses(rng.uniform(-20, 20, 3), rng.uniform(-3, 3, 3), rng.uniform(0, 0.1), 0.0, 1)[0]
    pose[::11] += rng.normal(size=(len(pose[::11]), 12)).astype(np.float32)
    want = restate_rays(d, pose)
    got = np.stack([capi.sweep_ray(d[k], pose[k]) for k in range(n)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(got[:, 3] == 0) and np.all(got[:, 7] == F(1e16))


def test_identity_pose_returns_the_direction(capi):
    rng = np.random.default_rng(3)
    for d in rng.normal(size=(200, 3)).astype(np.float32):
        r = capi.sweep_ray(d, IDENTITY_POSE)
        assert np.array_equal(r[4:7], d) and np.array_equal(r[0:4], np.zeros(4, np.float32))
    # a non-finite entry leaves a non-finite origin or direction: ls_trace_rays calls such a ray a miss
    for k in range(12):
        for bad in (np.nan, np.inf, -np.inf):
            p = IDENTITY_POSE.copy()
            p[k] = bad
            r = capi.sweep_ray(F([0.3, -0.2, 0.9]), p)
            assert not np.all(np.isfinite(r[[0, 1, 2, 4, 5, 6]]))


# ---- the constant-twist pose table ------------------------------------------------------------------------------------

def test_zero_twist_gives_exact_identities(capi):
    p = capi.sweep_poses_constant_twist([0, 0, 0], [0, 0, 0], 0.3, 1e-3, 150)
    assert p.shape == (150, 12) and np.array_equal(p.view(np.uint32), np.tile(IDENTITY_POSE, (150, 1)).view(np.uint32))
    # a rotation rate at tau = 0: the identity too, whatever dt does afterwards; a velocity alone: identity rotations
    p = capi.sweep_poses_constant_twist([3, -2, 1], [0.4, 0.1, -1.0], 0.0, 1e-3, 8)
    assert np.array_equal(p[0], IDENTITY_POSE) and not np.array_equal(p[1], IDENTITY_POSE)
    p = capi.sweep_poses_constant_twist([3, -2, 1], [0, 0, 0], 0.5, 0.25, 8)
    assert np.array_equal(p[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], np.tile(IDENTITY_POSE[[0, 1, 2, 4, 5, 6, 8, 9, 10]], (8, 1)))
    assert np.array_equal(p[:, 3], (3.0 * (0.5 + 0.25 * np.arange(8))).astype(np.float32))


@pytest.mark.parametrize("lin,ang,t0,dt,n", [
    ((10.0, -4.0, 0.5), (0.1, -0.2, 1.0), 0.0, 0.1 / 150, 150),
    ((-7.5, 12.0, 0.0), (0.9, 0.4, -0.6), 0.02, 0.1 / 96, 96),
    ((1.0, 2.0, 3.0), (2.5, -1.5, 3.0), -0.05, 1e-3, 257),
])
def test_constant_twist_equals_rodrigues(capi, lin, ang, t0, dt, n):
    """every entry within 1 float32 ulp of the float64 evaluation: one rounding of a double result whose libm sin / cos may differ
    from numpy's in the last double bit; the rotations orthonormal to 1e-6"""
    got = capi.sweep_poses_constant_twist(lin, ang, t0, dt, n)
    ref = rodrigues_poses(lin, ang, t0, dt, n)
    ref32 = ref.astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(ref32), np.abs(got)))
    assert np.all(np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= ulp)
    R = got.reshape(n, 3, 4)[:, :, :3].astype(np.float64)
    assert np.max(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3))) <= 1e-6
    assert np.all(np.abs(np.linalg.det(R) - 1.0) <= 1e-6)


def test_constant_twist_refuses_bad_input(capi):
    L = capi.load()
    f32p = ctypes.POINTER(ctypes.c_float)
    out = np.full((4, 12), 7.0, np.float32)
    ok = np.float32([1, 2, 3])

    def call(lin, ang, t0, dt, dst=out):
        return L.ls_sweep_poses_constant_twist(None if lin is None else lin.ctypes.data_as(f32p), None if ang is None else ang.ctypes.data_as(f32p),
                                               t0, dt, 4, None if dst is None else dst.ctypes.data_as(f32p))

    assert call(ok, ok, 0.0, 0.1) == 0
    out[:] = 7.0
    for k in range(3):
        for bad in (np.nan, np.inf):
            v = ok.copy()
            v[k] = bad
            assert call(v, ok, 0.0, 0.1) == INVALID_ARGUMENT and call(ok, v, 0.0, 0.1) == INVALID_ARGUMENT
    assert call(ok, ok, float("nan"), 0.1) == INVALID_ARGUMENT and call(ok, ok, 0.0, float("inf")) == INVALID_ARGUMENT
    assert call(None, ok, 0.0, 0.1) == INVALID_ARGUMENT and call(ok, None, 0.0, 0.1) == INVALID_ARGUMENT
    assert call(ok, ok, 0.0, 0.1, None) == INVALID_ARGUMENT
    assert np.all(out == 7.0)      # a refusal writes nothing
    with pytest.raises(capi.LidarShooterHipError):
        capi.sweep_poses_constant_twist([np.nan, 0, 0], [0, 0, 0], 0.0, 0.1, 4)
