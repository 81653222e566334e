"""ls_trace_rays / ls_trace_rays_host without a device: the symbols, the record layouts, the argument checks that come
before any device call (there is no GPU where `-m "not gpu"` runs)."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "lidarshooter_hip.h")).read()


def test_ray_query_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in ("ls_trace_rays", "ls_trace_rays_host"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s
    hdr = _header()
    assert re.search(r"int ls_trace_rays\(ls_tracer \*tr, void \*hip_stream, const void \*d_rays, uint32_t n, void \*d_out\);", hdr)
    assert re.search(r"int ls_trace_rays_host\(ls_tracer \*tr, const void \*rays, uint32_t n, void \*out\);", hdr)
    m = re.search(r"#define LS_INFO_RAY_QUERY_BUILT (\d+)", hdr)
    assert m and int(m.group(1)) == capi.LS_INFO_RAY_QUERY_BUILT == 17
    # a new info key, not one of the existing ones
    others = [int(v) for k, v in re.findall(r"#define (LS_INFO_\w+) (\d+)", hdr) if k != "LS_INFO_RAY_QUERY_BUILT"]
    assert 17 not in others


def test_ray_record_layout_is_the_one_ls_generate_rays_aos_writes(capi, oracle):
    # 32 bytes: origin xyz f32@0, tmin f32@12, direction xyz f32@16, tmax f32@28 (Ray.hpp:16-35), as the header documents
    hdr = _header()
    assert "origin xyz f32@0, tmin f32@12, direction xyz f32@16," in hdr
    for dt in (capi.RAY_DTYPE, oracle.RAY_DTYPE):
        assert dt.itemsize == 32
        assert [dt.fields[k][1] for k in ("origin", "tmin", "direction", "tmax")] == [0, 12, 16, 28]
    # the (n, 8) float32 form traceRays takes is the same bytes
    r = np.zeros(3, capi.RAY_DTYPE)
    r["origin"] = [[1, 2, 3]] * 3
    r["tmin"] = 0.5
    r["direction"] = [[4, 5, 6]] * 3
    r["tmax"] = 7
    assert np.array_equal(r.view(np.float32).reshape(3, 8), np.tile(np.float32([1, 2, 3, 0.5, 4, 5, 6, 7]), (3, 1)))
    # the output record is ls_hit
    assert capi.HIT_DTYPE.itemsize == 16
    assert [capi.HIT_DTYPE.fields[k][1] for k in ("ray", "geom", "prim", "t")] == [0, 4, 8, 12]


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    buf = (ctypes.c_uint8 * 64)()
    INVALID_ARGUMENT = -2
    assert L.ls_trace_rays(None, None, buf, 1, buf) == INVALID_ARGUMENT
    assert L.ls_trace_rays(None, None, None, 0, None) == INVALID_ARGUMENT
    assert L.ls_trace_rays_host(None, buf, 1, buf) == INVALID_ARGUMENT
    assert L.ls_trace_rays_host(None, None, 0, None) == INVALID_ARGUMENT


def test_abi_version_unchanged(capi):
    assert capi.load().ls_abi_version() == 4
