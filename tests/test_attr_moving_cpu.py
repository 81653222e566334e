"""ls_hit_attributes_moving / ls_apply_return_model_moving (and their _host variants) without a device: the symbols and their
signatures, the refusal of a NULL handle, the one new operation sequence -- the normal of a moving geometry carried back into the
sensor frame (ls_debug_motion_normal, the host compilation of what k_hit_attributes_moving runs) -- against a restatement written
here in np.float32 operations, bit for bit, and against float64 within a derived bound; and the pre-check of the GPU file's exact
test: for a translation and a half turn the definition (the committed triangle with the ray through the inverse motion) and the
reference (the re-posed triangle with the column's ray) agree bit for bit in t, cos_inc, u and v."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT
from test_sweep_cpu import IDENTITY_POSE, restate_rays
from test_sweep_moving_cpu import compose, restate_motion_rays, small_sensor

INVALID_ARGUMENT = -2
F = np.float32
EPS = 2.0 ** -24


def _header(name="lidarshooter_hip.h"):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", name)).read())


# ---- the restatement (shared with test_gpu_attr_moving.py) ------------------------------------------------------------------

def restate_motion_normal(n, motion):
    """normals (k, 3) found on geometries where they were committed, carried forward by the motion records (k, 12) = [Q | c]
    row-major: out_i = (Q[i][0] n_0 + Q[i][1] n_1) + Q[i][2] n_2 -- every product and sum rounded to float32"""
    n, p = np.asarray(n, np.float32), np.asarray(motion, np.float32)
    out = np.zeros((n.shape[0], 3), np.float32)
    with np.errstate(all="ignore"):
        for i in range(3):
            out[:, i] = (p[:, 4 * i] * n[:, 0] + p[:, 4 * i + 1] * n[:, 1]) + p[:, 4 * i + 2] * n[:, 2]
    return out


def box():
    """the closed box of test_gpu_sweep_moving: half size 1 about the origin, corners at +-1, 12 triangles"""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([tri for a, b, c, d in q for tri in ((a, b, c), (a, c, d))], np.uint32)


def box_case(oracle, half_turn):
    """the case of test_gpu_sweep_moving.test_a_record_means_the_geometry_reposed_exactly: V = 8, H = 16, the sensor frame the
    world frame, the sensor at rest; c_h = (h / 16, -h / 32, 0), Q the identity or a half turn about z -> (sensor, the box's
    committed pose, its motion table, the nominal ray records)"""
    s = small_sensor(oracle, begin=4.0, end=36.0)
    Q = np.diag([-1.0, -1.0, 1.0]) if half_turn else np.eye(3)
    a = np.float32([-6, -2, 0]) if half_turn else np.float32([6, 2, 0])      # Q a = (6, 2, 0): in front of the sensor either way
    A0 = np.float32([1, 0, 0, a[0], 0, 1, 0, a[1], 0, 0, 1, a[2]])
    motion = np.zeros((s.H, 3, 4), np.float32)
    motion[:, :, :3] = Q
    motion[:, 0, 3], motion[:, 1, 3] = np.arange(s.H) / 16.0, -np.arange(s.H) / 32.0
    rays = restate_rays(oracle.ray_dirs(s), np.tile(IDENTITY_POSE, (s.V * s.H, 1)))
    return s, A0, motion.reshape(s.H, 12), rays


# ---- exports and refusals ---------------------------------------------------------------------------------------------

def test_moving_attribute_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert capi.load().ls_abi_version() == 4      # the new entry points do not step the ABI version
    for s in ("ls_hit_attributes_moving", "ls_hit_attributes_moving_host", "ls_apply_return_model_moving", "ls_apply_return_model_moving_host"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s
    assert "ls_debug_motion_normal" in capi.DEBUG_SYMBOLS and hasattr(lib, "ls_debug_motion_normal")
    for name in ("hitAttributesMoving", "hitAttributesMovingDevice", "applyReturnModelMoving", "applyReturnModelMovingDevice"):
        assert callable(getattr(capi.Tracer, name))
    hdr = _header()
    assert "#define LS_ABI_VERSION 4" in hdr
    tables = r"const float \*{p}col_pose, uint32_t n_cols, const ls_geometry_motion \*motions, uint32_t n_motions, uint32_t flags, "
    assert re.search(r"int ls_hit_attributes_moving\(ls_tracer \*tr, void \*hip_stream, " + tables.format(p="d_") +
                     r"const void \*d_hits, const uint32_t \*d_count, uint32_t n, void \*d_out\);", hdr)
    assert re.search(r"int ls_hit_attributes_moving_host\(ls_tracer \*tr, " + tables.format(p="") +
                     r"const void \*hits, uint32_t n, void \*out\);", hdr)
    assert re.search(r"int ls_apply_return_model_moving\(ls_tracer \*tr, void \*hip_stream, const ls_return_model \*model, uint32_t frame_index, " +
                     tables.format(p="d_") + r"const void \*d_hits, const uint32_t \*d_count, uint32_t n, "
                     r"const float \*d_reflectivity, uint32_t n_reflectivity, void \*d_points32, void \*d_hits_out, uint32_t \*d_n_out\);", hdr)
    assert re.search(r"int ls_apply_return_model_moving_host\(ls_tracer \*tr, const ls_return_model \*model, uint32_t frame_index, " +
                     tables.format(p="") + r"const void \*hits, uint32_t n, const float \*reflectivity, uint32_t n_reflectivity, "
                     r"void \*points32, void \*hits_out, uint32_t \*n_out\);", hdr)
    assert re.search(r"int ls_debug_motion_normal\(const float n3\[3\], const float motion12\[12\], float out3\[3\]\);",
                     _header("lidarshooter_hip_debug.h"))
    # what the header of the moving sweep called missing is offered now
    assert "exact test would need" not in hdr and "ls_hit_attributes_moving / ls_apply_return_model_moving below" in hdr


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    pose = np.tile(IDENTITY_POSE, (4, 1))
    mo = (capi.GeometryMotion * 1)()
    mo[0].geom, mo[0].col_motion = 0, pose.ctypes.data
    m = capi.ReturnModel()
    hits = np.zeros(4, capi.HIT_DTYPE)
    n = ctypes.c_uint32(77)
    buf = np.zeros(4 * 48, np.uint8)
    B, Hh, P = buf.ctypes.data, hits.ctypes.data, pose.ctypes.data
    assert L.ls_hit_attributes_moving(None, None, P, 4, mo, 1, 0, Hh, None, 4, B) == INVALID_ARGUMENT
    assert L.ls_hit_attributes_moving_host(None, P, 4, mo, 1, 0, Hh, 4, B) == INVALID_ARGUMENT
    assert L.ls_hit_attributes_moving_host(None, None, 0, None, 0, 0, Hh, 4, B) == INVALID_ARGUMENT
    assert L.ls_apply_return_model_moving(None, None, ctypes.byref(m), 0, P, 4, mo, 1, 0, Hh, None, 4, None, 0, B, None, B) == INVALID_ARGUMENT
    assert L.ls_apply_return_model_moving_host(None, ctypes.byref(m), 0, P, 4, mo, 1, 0, Hh, 4, None, 0, B, None, ctypes.byref(n)) == INVALID_ARGUMENT
    assert L.ls_apply_return_model_moving_host(None, ctypes.byref(m), 0, None, 0, None, 0, 0, Hh, 4, None, 0, None, None, ctypes.byref(n)) == INVALID_ARGUMENT
    assert n.value == 77 and not buf.any()
    out = np.full(3, 7.0, np.float32)
    f32p = ctypes.POINTER(ctypes.c_float)
    assert L.ls_debug_motion_normal(None, None, None) == INVALID_ARGUMENT
    assert L.ls_debug_motion_normal(None, pose.ctypes.data_as(f32p), out.ctypes.data_as(f32p)) == INVALID_ARGUMENT
    assert L.ls_debug_motion_normal(out.ctypes.data_as(f32p), None, out.ctypes.data_as(f32p)) == INVALID_ARGUMENT
    assert np.all(out == 7.0)


# ---- the normal carried back into the sensor frame ------------------------------------------------------------------------

def _rotations(rng, n):
    """proper rotations, float64 (n, 3, 3): the QR factor of a Gaussian matrix with the signs fixed"""
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def _records(Q):
    p = np.zeros((Q.shape[0], 3, 4), np.float32)
    p[:, :, :3] = Q
    return p.reshape(-1, 12)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def test_motion_normal_equals_the_restatement(capi):
    rng = np.random.default_rng(20261)
    n = 10000
    motion = _records(_rotations(rng, n))
    motion[:, [3, 7, 11]] = rng.normal(size=(n, 3)) * 10            # the offsets are not read
    motion[::11] += rng.normal(size=(len(motion[::11]), 12)).astype(np.float32)      # sheared and scaled records among them
    nrm = _unit(rng, n)
    nrm[::13] *= F(1e-3)
    for k in range(0, n, 97):                                        # non-finite entries in the record and in the normal
        motion[k, (0, 1, 2, 4, 5, 6, 8, 9, 10)[rng.integers(0, 9)]] = (np.nan, np.inf, -np.inf)[k % 3]
    nrm[5::101, 1] = np.nan
    want = restate_motion_normal(nrm, motion)
    got = np.stack([capi.motion_normal(nrm[k], motion[k]) for k in range(n)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.count_nonzero(~np.isfinite(got).all(axis=1)) >= n // 97
    # an offset does not move a direction
    moved = motion.copy()
    moved[:, [3, 7, 11]] = 0
    assert np.array_equal(restate_motion_normal(nrm, moved).view(np.uint32), want.view(np.uint32))


def test_identity_record_returns_the_normal(capi):
    rng = np.random.default_rng(5)
    for nrm in _unit(rng, 200):
        assert np.array_equal(capi.motion_normal(nrm, IDENTITY_POSE), nrm)
    for nrm in (F([0, 0, 1]), F([-0.0, 1, 0]), F([0.6, -0.0, -0.8]), F([-1, -0.0, -0.0])):      # a -0 may come back as +0: equal numerically
        got = capi.motion_normal(nrm, IDENTITY_POSE)
        assert np.array_equal(got, nrm)
    # out3 may be n3
    L = capi.load()
    f32p = ctypes.POINTER(ctypes.c_float)
    half = F([-1, 0, 0, 5, 0, -1, 0, 6, 0, 0, 1, 7])
    v = F([0.6, -0.48, 0.64])
    assert L.ls_debug_motion_normal(v.ctypes.data_as(f32p), half.ctypes.data_as(f32p), v.ctypes.data_as(f32p)) == 0
    assert np.array_equal(v, F([-0.6, 0.48, 0.64]))


def test_motion_normal_against_float64(capi):
    """random proper rotations rounded to float32, random unit normals rounded to float32, both taken as doubles: every component
    within 4 * 2^-24 of Q n.  Three products and two sums, each rounded once: the products' errors are at most 2^-24 |Q_ij n_j| each,
    the first sum's 2^-24 |a + b|, the second's 2^-24 |result|, and with sum_j |Q_ij n_j| <= |Q_i| |n| <= 1 + 2^-22 the total stays
    below (1 + 1 + 1) * 2^-24 * (1 + small) < 4 * 2^-24.  Measured over 2e6 samples in numpy: at most 1.77 * 2^-24.  The same data
    through the transposed Q -- the inverse rotation -- exceeds the bound for more than half of the samples."""
    rng = np.random.default_rng(77)
    n = 20000
    Q = _rotations(rng, n).astype(np.float32)
    nrm = _unit(rng, n)
    motion = _records(Q)
    got = np.stack([capi.motion_normal(nrm[k], motion[k]) for k in range(n)]).astype(np.float64)
    ref = np.einsum("kij,kj->ki", Q.astype(np.float64), nrm.astype(np.float64))
    err = np.abs(got - ref)
    print("largest error: %.3f * 2^-24" % (err.max() / EPS))
    assert np.all(err <= 4 * EPS)
    assert np.all(np.abs(np.linalg.norm(got, axis=1) - 1.0) < 1e-6)
    transposed = _records(Q.transpose(0, 2, 1))
    bad = np.stack([capi.motion_normal(nrm[k], transposed[k]) for k in range(0, n, 10)]).astype(np.float64)
    off = (np.abs(bad - ref[::10]) > 4 * EPS).any(axis=1)
    assert np.count_nonzero(off) > len(off) // 2


# ---- the pre-check of the exact GPU test ------------------------------------------------------------------------------------

def test_translation_and_half_turn_are_exact_on_the_host(oracle, capi):
    """test_gpu_attr_moving.test_attributes_mean_the_geometry_reposed_exactly compares ls_hit_attributes_moving with
    ls_hit_attributes on the box re-posed per column and asks for equal bits.  Both sides on the host, through
    ls_debug_hit_attributes_on_triangle: the re-posed float32 corners with the column's ray against the committed corners with
    ls_debug_motion_ray's ray -- t, cos_inc, u and v bit for bit, the normal carried forward equal numerically.  (Corner sums are
    exact and a half turn only negates components; a quarter turn would permute the axes that attr_dot fuses in a fixed order, and
    is not expected to be exact.)"""
    for half_turn in (False, True):
        s, A0, motion, rays = box_case(oracle, half_turn)
        v, tris = box()
        committed = oracle.transform_vertices(v, A0, s)
        hits = 0
        for h in range(s.H):
            reposed = oracle.transform_vertices(v, compose(motion[h], A0), s)
            for r in rays[h::s.H]:
                seen = capi.motion_ray(r, motion[h])
                assert np.array_equal(seen.view(np.uint32), restate_motion_rays(r[None], motion[h][None])[0].view(np.uint32))
                for tri in tris:
                    a = capi.hit_attributes_on_triangle(r[0:3], r[4:7], *reposed[tri])
                    b = capi.hit_attributes_on_triangle(seen[0:3], seen[4:7], *committed[tri])
                    assert (a is None) == (b is None)
                    if a is None:
                        continue
                    hits += 1
                    (ta, ra), (tb, rb) = a, b
                    assert ta.view(np.uint32) == tb.view(np.uint32)
                    assert np.array_equal(ra[3:6].view(np.uint32), rb[3:6].view(np.uint32))       # cos_inc, u, v
                    fwd = capi.motion_normal(rb[0:3], motion[h])
                    assert np.array_equal(fwd, ra[0:3])                                          # Q n_g, numerically
                    Qn = motion[h].reshape(3, 4)[:, :3].astype(np.float64) @ rb[0:3].astype(np.float64)
                    assert np.array_equal(fwd.astype(np.float64), Qn)
        assert hits >= 16      # the box is seen in many columns, each with its own offset
