"""ls_sample_surface / ls_sample_surface_host on the MI355X: points drawn from the surface of the committed scene in proportion to area,
against the numpy restatement of tests/surface_sample_reference.py, byte for byte -- the golden scene on both engines' handles, meshes
built for the edges of the prefix scan and of the weights, posed geometries and quads under transforms, pose updates and removals, the
selection, slices of one sequence, the samples against ls_closest_points and ls_scene_grid, and the entry points' plumbing.  Nothing
here is compared against the ls_debug_surface_* hooks.

Not reached here: a triangle that names a vertex its geometry does not have.  The commit refuses such a mesh, no test of the grids
gets one past it either, and the host hooks take coordinates, not indices: the kernels' index check is covered by reading only."""
import ctypes

import numpy as np
import pytest

import surface_sample_reference as ref
from conftest import make_tracer
from test_gpu_labels import _to_device
from test_gpu_rays import INV, _add, _ground_ben, _scene_posed_quads
from test_gpu_scene_grid import _dilate, _unposed
from test_occupancy_cpu import rigid_transform, rotation

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = -2                      # LS_ERR_INVALID_ARGUMENT
FRAME_EAGER = 0                            # LS_FRAME_EAGER
GUARD = 256
B = 256                                    # the workgroup of k_surface_block_sums / k_surface_prefix
F = np.float32

# torch fills a new tensor on its own stream, the library works on the handle's: every buffer is filled (a device-wide
# synchronize) before the library gets it


def _same(got, want):
    """records, byte for byte"""
    assert got.dtype == ref.DTYPE and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        for f in ref.DTYPE.names:
            a, b = got[f].reshape(got.shape[0], -1), want[f].reshape(want.shape[0], -1)
            bad = np.nonzero(np.any(a.view(np.uint32) != b.view(np.uint32), axis=1))[0]
            assert bad.size == 0, (f, bad.size, bad[:5], got[bad[:3]], want[bad[:3]])
    assert got.tobytes() == want.tobytes()


def _same_info(got, want):
    assert got.tobytes() == want.tobytes(), (got, want)


def _sample_device(tr, capi, desc, select=None, n_select=None, xf=None, stream=None, with_info=True):
    """ls_sample_surface on device buffers, 0xAB behind both outputs -> (records, info or None)"""
    import torch
    n = int(desc.n_samples)
    d_select = None if select is None else _to_device(np.ascontiguousarray(select, np.uint8))
    d_out = torch.full((n * 48 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_info = torch.full((16 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = tr.sampleSurfaceDevice(desc, d_out.data_ptr(), d_info.data_ptr() if with_info else 0, 0 if select is None else d_select.data_ptr(),
                                0 if select is None else (len(select) if n_select is None else n_select), xf, stream)
    assert rc == 0
    tr.synchronize()
    torch.cuda.synchronize()
    o, i = d_out.cpu().numpy(), d_info.cpu().numpy()
    assert np.all(o[n * 48:] == 0xAB) and np.all(i[16:] == 0xAB)
    if not with_info:
        assert np.all(i == 0xAB)
    return o[:n * 48].copy().view(ref.DTYPE), i[:16].copy().view(ref.INFO_DTYPE)[0] if with_info else None


def _desc(capi, n, seed=1, first=0):
    return capi.SurfaceSampleDesc.make(n, seed=seed, first_sample=first)


def _want(oracle, ml, s, d, xf=None, select=None):
    return ref.scene_samples(oracle, ml, s, xf, select, d)


# ---- 1. the golden scene on both engines' handles --------------------------------------------------------------------------------

GOLDEN_N = (1, 63, 64, 65, 257, 4096)
GOLDEN_SEED = 11
_golden = {}   # computed once, whichever test asks first


def _golden_reference(oracle, ml, s):
    if not _golden:
        T, G, Pr, Tr = ref.scene_triangles(oracle, ml, s)
        _golden["tris"] = (T, G)
        for n in GOLDEN_N:
            _golden[n] = ref.samples(T, G, Pr, Tr, GOLDEN_SEED, 0, n)
    return _golden


@pytest.mark.parametrize("engine", ["projection", "bvh"])
def test_ground_and_ben_on_both_engines_handles(oracle, capi, sensors, meshes, engine):
    """sensor 0000 over ground + ben in the sensor frame: the device call with and without d_info and the host variant at every count;
    the info's area against a float64 area of the same triangles"""
    s = sensors["0000"]
    tr = make_tracer(capi, s, engine)
    ml = _ground_ben(tr, oracle, meshes)
    built = tr.info(capi.LS_INFO_RAY_QUERY_BUILT)
    golden = _golden_reference(oracle, ml, s)
    for n in GOLDEN_N:
        want, winfo = golden[n]
        d = _desc(capi, n, GOLDEN_SEED)
        got, info = _sample_device(tr, capi, d)
        _same(got, want)
        _same_info(info, winfo)
        got, none = _sample_device(tr, capi, d, with_info=False)
        assert none is None
        _same(got, want)
        rc, rec, hinfo = tr.sampleSurface(d)
        assert rc == 0
        _same(rec, want)
        _same_info(hinfo, winfo)
        assert np.all(want["flags"] == 1)
    assert set(np.unique(golden[4096][0]["geom"])) == {0, 1}                 # both geometries are drawn
    q = golden["tris"][0].astype(np.float64)
    area64 = 0.5 * np.linalg.norm(np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), axis=1).sum()
    area = float(int(info["weight_total"])) * 2.0 ** int(info["exponent"])
    print("area", area, "float64", area64, "relative", area / area64 - 1)
    assert abs(area / area64 - 1) <= 1e-5 and info["n_weighted"] > 5000
    assert tr.info(capi.LS_INFO_RAY_QUERY_BUILT) == built                     # no hierarchy is touched
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 2. the scan's edges ---------------------------------------------------------------------------------------------------------

def _tiny_mesh(n):
    """n right triangles on a lattice of 5 cm, legs of 1 to 2 cm that vary with the index; one in eleven a point"""
    i = np.arange(n)
    base = np.stack([(i % 256) * 0.05, (i // 256) * 0.05, np.zeros(n)], axis=1)
    leg = 0.01 * (1.0 + ((i * 37) % 97) / 97.0)
    leg[i % 11 == 3] = 0.0
    v = np.repeat(base[:, None, :], 3, axis=1)
    v[:, 1, 0] += leg
    v[:, 2, 1] += leg
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("n_tris", [1, B - 1, B, B + 1, B * B + 1])
def test_prefix_scan_edges(oracle, capi, sensors, n_tris):
    """one geometry of n tiny triangles under the unposed sensor, n on both sides of a workgroup of the scan and, at B^2 + 1 = 65 537,
    with more workgroup sums than one workgroup adds up in one trip: the prefix read through its effect, every record"""
    s = _unposed(sensors["0000"])
    verts, idx = _tiny_mesh(n_tris)
    tr = make_tracer(capi, s)
    _add(tr, "m", verts, idx)
    tr.updateGeometry("m", oracle.IDENTITY_AFFINE, verts, idx)
    assert tr.commitScene() == 0
    ml = [(0, verts, idx, oracle.IDENTITY_AFFINE)]
    d = _desc(capi, 8192, seed=n_tris)
    want, winfo = _want(oracle, ml, s, d)
    assert winfo["n_weighted"] == n_tris - np.count_nonzero(np.arange(n_tris) % 11 == 3)
    if n_tris > 1:
        assert len(np.unique(want["tri"])) > min(n_tris, 8192) // 3          # the draws spread over the whole index
    got, info = _sample_device(tr, capi, d)
    _same(got, want)
    _same_info(info, winfo)
    rc, rec, hinfo = tr.sampleSurface(d)
    assert rc == 0
    _same(rec, want)
    _same_info(hinfo, winfo)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 3. the weights --------------------------------------------------------------------------------------------------------------

def _leg(x, y, a):
    return [[x, y, 0.0], [x + a, y, 0.0], [x, y + a, 0.0]]


def test_weights_zero_runs_and_nothing_to_draw(oracle, capi, sensors):
    """one mesh whose areas span 2^42 -- the small ones weigh nothing and never appear --, with a segment and a point, and runs of
    zero-weight triangles at the start, in the middle and at the end; a second geometry without any area: selected alone, W = 0 and
    every record is invalid; a third whose areas are all subnormal"""
    s = _unposed(sensors["0000"])
    seg = [[1.0, 1.0, 0.0], [2.0, 3.0, 0.0], [2.0, 3.0, 0.0]]
    pt = [[5.0, 5.0, 1.0]] * 3
    small = lambda k: _leg(10.0 + k, 0.0, 2.0 ** -10)                         # 2^-21
    tris = [seg, pt, small(0)]                                                # a run at the start
    tris += [_leg(0.0, 0.0, 2048.0), _leg(-8.0, -8.0, 300.0), _leg(-9.0, 3.0, 0.25)]  # 2^21, 45 000, 2^-5 (a weight of 16 in 2^31: hardly ever drawn)
    tris += [small(1), pt, seg, small(2), small(3)]                           # ... in the middle
    tris += [_leg(20.0, -30.0, 700.0), _leg(-40.0, 7.0, 0.0625), _leg(3.0, 3.0, 1500.0)]   # (2^-9: the least area with a weight, 1)
    tris += [small(4), seg, pt]                                               # ... and at the end
    verts = np.array(tris, np.float32).reshape(-1, 3)
    idx = np.arange(verts.shape[0], dtype=np.uint32).reshape(-1, 3)
    flat = np.array([seg, pt, seg, seg, pt], np.float32).reshape(-1, 3)
    fidx = np.arange(flat.shape[0], dtype=np.uint32).reshape(-1, 3)
    rng = np.random.default_rng(4)
    sub = (rng.uniform(-1, 1, (300, 3, 3)) * 1e-20).astype(np.float32).reshape(-1, 3)
    sidx = np.arange(sub.shape[0], dtype=np.uint32).reshape(-1, 3)
    tr = make_tracer(capi, s)
    for name, v, i in (("m", verts, idx), ("flat", flat, fidx), ("sub", sub, sidx)):
        _add(tr, name, v, i)
        tr.updateGeometry(name, oracle.IDENTITY_AFFINE, v, i)
    assert tr.commitScene() == 0
    ml = [(0, verts, idx, oracle.IDENTITY_AFFINE), (1, flat, fidx, oracle.IDENTITY_AFFINE), (2, sub, sidx, oracle.IDENTITY_AFFINE)]
    d = _desc(capi, 20000, seed=5)
    want, winfo = _want(oracle, ml, s, d)
    assert winfo["n_weighted"] == 6 and winfo["exponent"] == 21 - 30
    drawn = {int(t) for t in np.unique(want["tri"])}
    assert {3, 4, 11, 13} <= drawn <= {3, 4, 5, 11, 12, 13} and np.all(want["geom"] == 0) and np.all(want["flags"] == 1)
    got, info = _sample_device(tr, capi, d)
    _same(got, want)
    _same_info(info, winfo)
    # nothing with an area: rc 0, W = 0, every record invalid
    want0, winfo0 = _want(oracle, ml, s, d, select=[0, 1, 0])
    assert winfo0["weight_total"] == 0 and winfo0["n_weighted"] == 0 and winfo0["exponent"] == 0
    assert np.all(want0["geom"] == INV) and not want0["flags"].any() and not want0["p"].any()
    for sel in ([0, 1, 0], [0, 0, 0]):
        got, info = _sample_device(tr, capi, d, select=sel)
        _same(got, want0)
        _same_info(info, winfo0)
    rc, rec, hinfo = tr.sampleSurface(d, select=[0, 1, 0])
    assert rc == 0
    _same(rec, want0)
    _same_info(hinfo, winfo0)
    # subnormal areas alone: the exponent comes from a subnormal maximum
    wants, winfos = _want(oracle, ml, s, d, select=[0, 0, 1])
    assert winfos["exponent"] < -126 - 30 and winfos["n_weighted"] > 200 and np.all(wants["geom"] == 2)
    got, info = _sample_device(tr, capi, d, select=[0, 0, 1])
    _same(got, wants)
    _same_info(info, winfos)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 4. posed geometries, quads, the selection, transforms, pose updates, removals --------------------------------------------

def test_posed_quads_select_transforms_updates_and_removals(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    d = _desc(capi, 4096, seed=21)
    plain, pinfo = _want(oracle, ml, s, d)
    got, info = _sample_device(tr, capi, d)
    _same(got, plain)
    _same_info(info, pinfo)
    # the plate's 24 quads are 48 triangles: tri runs over them, prim is the quad
    only, oinfo = _want(oracle, ml, s, d, select=[0, 0, 1])
    assert oinfo["n_weighted"] == 48 and np.all(only["geom"] == 2) and len(np.unique(only["tri"])) == 48
    assert np.array_equal(only["prim"], only["tri"] >> 1) and only["tri"].max() == 47 and set(only["tri"] & 1) == {0, 1}
    got, info = _sample_device(tr, capi, d, select=[0, 0, 1])
    _same(got, only)
    _same_info(info, oinfo)
    # every geometry alone, n_select below and above the table, nothing selected
    for sel, as_if in (([1, 0, 0], None), ([0, 1, 0], None), ([0, 1], [0, 1, 1]), ([0], [0, 1, 1]), ([1, 0, 0, 0, 1, 1], [1, 0, 0])):
        want, winfo = _want(oracle, ml, s, d, select=as_if or sel)
        got, info = _sample_device(tr, capi, d, select=sel)
        _same(got, want)
        _same_info(info, winfo)
        assert np.all(want["flags"] == 1)
    got, info = _sample_device(tr, capi, d, select=[0, 0, 0])
    assert np.all(got["geom"] == INV) and not got["flags"].any() and info["weight_total"] == 0
    rc, rec, hinfo = tr.sampleSurface(d, select=[0, 1, 0])
    assert rc == 0
    _same(rec, _want(oracle, ml, s, d, select=[0, 1, 0])[0])
    for xf in (rigid_transform(), rotation(np.random.default_rng(23))):
        want, winfo = _want(oracle, ml, s, d, xf=xf)
        assert want.tobytes() != plain.tobytes()
        got, info = _sample_device(tr, capi, d, xf=xf)
        _same(got, want)
        _same_info(info, winfo)
        rc, rec, hinfo = tr.sampleSurface(d, sensor_to_out=xf)
        assert rc == 0
        _same(rec, want)
        _same_info(hinfo, winfo)
    # a new pose and a commit: the samples follow
    A = oracle.affine_from_components(np.float32([-2.0, 1.0, 0.75]), np.float32([0.1, 0.3, -0.7]))
    tr.updateGeometryTransform("face", A)
    assert tr.commitScene() == 0
    ml[1] = (1, ml[1][1], ml[1][2], A)
    moved, minfo = _want(oracle, ml, s, d)
    assert moved.tobytes() != plain.tobytes()
    got, info = _sample_device(tr, capi, d)
    _same(got, moved)
    _same_info(info, minfo)
    # a removal: the geomIDs are sparse, the free id's table entry is empty
    assert tr.removeGeometry("face") >= 0
    assert tr.commitScene() == 0
    sparse, sinfo = _want(oracle, [ml[0], ml[2]], s, d)
    assert set(np.unique(sparse["geom"])) == {0, 2}
    got, info = _sample_device(tr, capi, d)
    _same(got, sparse)
    _same_info(info, sinfo)
    rc, rec, hinfo = tr.sampleSurface(d, select=[1, 1, 0])
    assert rc == 0
    _same(rec, _want(oracle, [ml[0]], s, d)[0])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 5. slices -------------------------------------------------------------------------------------------------------------------

def test_slices_of_one_sequence(oracle, capi, sensors, meshes):
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _ground_ben(tr, oracle, meshes)
    whole, _ = _sample_device(tr, capi, _desc(capi, 3000, seed=9, first=100))
    _same(whole, _want(oracle, ml, s, _desc(capi, 3000, seed=9, first=100))[0])
    for first, n in ((100, 1), (163, 65), (1000, 2100), (3099, 1)):
        part, _ = _sample_device(tr, capi, _desc(capi, n, seed=9, first=first))
        _same(part, whole[first - 100:first - 100 + n])
    # the counter's high word, and j wrapping at 2^64
    for first in ((1 << 32) - 3, (1 << 64) - 5):
        d = _desc(capi, 8, seed=9, first=first)
        got, _ = _sample_device(tr, capi, d)
        want = _want(oracle, ml, s, d)[0]
        _same(got, want)
        assert len({r.tobytes() for r in got}) == 8
        rc, rec, _ = tr.sampleSurface(d)
        assert rc == 0
        _same(rec, want)
    # the same call twice: the same bytes; another seed: other bytes
    again, _ = _sample_device(tr, capi, _desc(capi, 3000, seed=9, first=100))
    assert again.tobytes() == whole.tobytes()
    other, _ = _sample_device(tr, capi, _desc(capi, 3000, seed=10, first=100))
    assert np.count_nonzero(np.any(other["p"] != whole["p"], axis=1)) > 2990
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 6. against the rest of the library ------------------------------------------------------------------------------------------

def test_samples_lie_on_the_surface_the_other_queries_see(oracle, capi, sensors, meshes):
    """ls_closest_points from every sample finds a surface point within test_gpu_closest's bound (2e-6 * S); the cell of every sample
    has ls_scene_grid count > 0 in its 3 x 3 x 3 neighbourhood"""
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _ground_ben(tr, oracle, meshes)
    golden = _golden_reference(oracle, ml, s)
    rec, _ = _sample_device(tr, capi, _desc(capi, 4096, GOLDEN_SEED))
    _same(rec, golden[4096][0])
    assert np.all(rec["flags"] == 1)
    pts = np.concatenate([rec["p"], np.full((4096, 1), np.inf, np.float32)], axis=1)
    rc, near = tr.closestPoints(pts)
    assert rc == 0
    S = max(float(np.abs(golden["tris"][0]).max()), float(np.abs(rec["p"]).max()))
    print("largest dist", near["dist"].max(), "in units of 2e-6 S", near["dist"].max() / (2e-6 * S))
    assert np.all(near["geom"] != INV) and np.all(near["dist"] <= 2e-6 * S)
    origin, cell, dims = (-60.0, -60.0, -12.0), 1.0, (120, 120, 24)
    rc, counts, _ = tr.sceneGrid(capi.SceneGridDesc.make(origin, cell, dims))
    assert rc == 0
    c = np.floor((rec["p"].astype(np.float64) - np.float64(origin)) / cell).astype(np.int64)
    inside = np.all((c >= 0) & (c < np.int64(dims)), axis=1)
    assert inside.sum() > 3000
    near_surface = _dilate(counts > 0)
    assert np.all(near_surface[c[inside, 2], c[inside, 1], c[inside, 0]])
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()


# ---- 7. plumbing -----------------------------------------------------------------------------------------------------------------

def test_entry_points(oracle, capi, sensors, meshes):
    """a caller stream; the host variant on unaligned pageable memory with guards; n_samples = 0 with and without buffers; the refusals
    of the device entry point in their order, nothing written; no commit: -1 and nothing written"""
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    ml = _scene_posed_quads(oracle, capi, tr, meshes)
    n = 1000
    d = _desc(capi, n, seed=3)
    want, winfo = _want(oracle, ml, s, d)
    st = torch.cuda.Stream()
    got, info = _sample_device(tr, capi, d, stream=st.cuda_stream)
    _same(got, want)
    _same_info(info, winfo)
    # the host variant on unaligned pageable memory, a guard around both outputs and the selection
    L, h = tr.L, tr.h

    def unaligned(nbytes, shift, fill=None):
        buf = np.full(nbytes + 64, 0xAB, np.uint8)
        off = (-buf.ctypes.data) % 16 + shift
        if fill is not None:
            buf[off:off + nbytes] = fill
        return buf, off
    ho, o_o = unaligned(n * 48, 5)
    hi, o_i = unaligned(16, 3)
    hs, o_s = unaligned(3, 7, np.array([1, 0, 1], np.uint8))
    part, pinfo = _want(oracle, ml, s, d, select=[1, 0, 1])
    assert L.ls_sample_surface_host(h, ctypes.byref(d), None, hs.ctypes.data + o_s, 3, ho.ctypes.data + o_o, hi.ctypes.data + o_i) == 0
    assert ho[o_o:o_o + n * 48].tobytes() == part.tobytes() and hi[o_i:o_i + 16].tobytes() == pinfo.tobytes()
    assert np.all(ho[:o_o] == 0xAB) and np.all(ho[o_o + n * 48:] == 0xAB) and np.all(hi[:o_i] == 0xAB) and np.all(hi[o_i + 16:] == 0xAB)
    ho[:] = 0xAB
    assert L.ls_sample_surface_host(h, ctypes.byref(d), None, None, 0, ho.ctypes.data + o_o, None) == 0          # no info
    assert ho[o_o:o_o + n * 48].tobytes() == want.tobytes() and np.all(ho[:o_o] == 0xAB) and np.all(ho[o_o + n * 48:] == 0xAB)
    # n_samples = 0: the way to ask for a selection's area; without any buffer it is a call that does nothing
    d0 = _desc(capi, 0)
    got, info = _sample_device(tr, capi, d0)
    assert got.shape == (0,)
    _same_info(info, winfo)
    assert tr.sampleSurfaceDevice(d0, 0, 0) == 0
    rc, rec, hinfo = tr.sampleSurface(d0, select=[1, 0, 1])
    assert rc == 0 and rec.shape == (0,)
    _same_info(hinfo, pinfo)
    hi[:] = 0xAB
    assert L.ls_sample_surface_host(h, ctypes.byref(d0), None, None, 0, None, hi.ctypes.data + o_i) == 0
    assert hi[o_i:o_i + 16].tobytes() == winfo.tobytes() and np.all(hi[:o_i] == 0xAB) and np.all(hi[o_i + 16:] == 0xAB)
    # refusals, nothing written
    out = torch.full((n * 48 + 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    iout = torch.full((32,), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_sel = _to_device(np.array([1, 1, 1], np.uint8))
    torch.cuda.synchronize()
    xf = rigid_transform()

    def call(handle=h, desc=d, **kw):
        a = dict(xf=None, select=d_sel.data_ptr(), n_select=3, samples=out.data_ptr(), info=iout.data_ptr())
        a.update(kw)
        return L.ls_sample_surface(handle, None, None if desc is None else ctypes.byref(desc), a["xf"], a["select"], a["n_select"], a["samples"], a["info"])

    def desc(**kw):
        dd = _desc(capi, n, seed=3)
        for k, v in kw.items():
            if k == "reserved":
                dd.reserved[v] = 1
            else:
                setattr(dd, k, v)
        return dd
    bad_xf = xf.copy()
    bad_xf[7] = np.inf
    nan_xf = xf.copy()
    nan_xf[0] = np.nan
    assert call(desc=None) == INVALID_ARGUMENT
    assert call(samples=None) == INVALID_ARGUMENT
    assert call(select=None) == INVALID_ARGUMENT
    assert call(desc=desc(flags=1)) == INVALID_ARGUMENT and call(desc=desc(flags=0x80000000)) == INVALID_ARGUMENT
    assert call(desc=desc(reserved=0)) == INVALID_ARGUMENT and call(desc=desc(reserved=2)) == INVALID_ARGUMENT
    assert call(xf=bad_xf.ctypes.data) == INVALID_ARGUMENT and call(xf=nan_xf.ctypes.data) == INVALID_ARGUMENT
    assert call(samples=out.data_ptr() + 8) == INVALID_ARGUMENT
    assert call(info=iout.data_ptr() + 4) == INVALID_ARGUMENT
    assert L.ls_sample_surface_host(h, ctypes.byref(desc(flags=8)), None, None, 0, ho.ctypes.data, hi.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_sample_surface_host(h, ctypes.byref(d), None, None, 2, ho.ctypes.data, hi.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_sample_surface_host(h, ctypes.byref(d), None, None, 0, None, hi.ctypes.data) == INVALID_ARGUMENT
    assert L.ls_sample_surface_host(h, ctypes.byref(d), bad_xf.ctypes.data, None, 0, ho.ctypes.data, hi.ctypes.data) == INVALID_ARGUMENT
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(iout.cpu().numpy() == 0xAB)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
    # no commit: the other refusals still come first; then -1, nothing written
    t2 = make_tracer(capi, s)
    assert call(handle=t2.h, desc=desc(flags=2)) == INVALID_ARGUMENT and call(handle=t2.h, samples=out.data_ptr() + 4) == INVALID_ARGUMENT
    assert t2.sampleSurfaceDevice(d, out.data_ptr(), iout.data_ptr()) == -1
    keep = ho.copy()
    assert t2.L.ls_sample_surface_host(t2.h, ctypes.byref(d), None, None, 0, ho.ctypes.data + o_o, hi.ctypes.data + o_i) == -1
    assert np.array_equal(ho, keep)
    rc, rec, hinfo = t2.sampleSurface(d)
    assert rc == -1 and rec.shape == (n,) and np.all(rec["geom"] == INV) and not rec["flags"].any() and hinfo["weight_total"] == 0
    t2.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(iout.cpu().numpy() == 0xAB)
    assert t2.info(capi.LS_INFO_DEVICE_STATUS) == 0
    t2.close()


def test_open_frame_graph_is_refused(oracle, capi, sensors, meshes):
    import torch
    s = sensors["0001"]
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    tr.setOption(capi.LS_OPT_FRAME_GRAPH, 1)
    ml = _ground_ben(tr, oracle, meshes)
    cap = s.V * s.H
    p, h, c = (torch.zeros(32 * cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * cap, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0"))
    tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), cap)
    n = 500
    d = _desc(capi, n, seed=4)
    out = torch.full((n * 48,), 0xAB, dtype=torch.uint8, device="cuda:0")
    iout = torch.full((16,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = tr.L
    assert L.ls_frame_graph_begin(tr.h, 7) == 0
    tr.traceSceneAsync(0)
    mode = ctypes.c_int(-1)
    assert L.ls_frame_graph_stream(tr.h, None, None, ctypes.byref(mode)) == 0
    assert mode.value != FRAME_EAGER   # the frame is being captured: the graph is open
    assert L.ls_sample_surface(tr.h, None, ctypes.byref(d), None, None, 0, out.data_ptr(), iout.data_ptr()) == INVALID_ARGUMENT
    assert L.ls_sample_surface_host(tr.h, None, None, None, 0, None, None) == INVALID_ARGUMENT
    assert L.ls_frame_graph_end(tr.h) == 0
    assert L.ls_frame_graph_reset(tr.h) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0xAB) and np.all(iout.cpu().numpy() == 0xAB)
    # the graph is closed: the call works
    assert tr.sampleSurfaceDevice(d, out.data_ptr(), iout.data_ptr()) == 0
    tr.synchronize()
    torch.cuda.synchronize()
    want, winfo = _want(oracle, ml, s, d)
    _same(out.cpu().numpy().view(ref.DTYPE), want)
    _same_info(iout.cpu().numpy().view(ref.INFO_DTYPE)[0], winfo)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
