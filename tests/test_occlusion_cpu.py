"""ls_occluded_rays / ls_occluded_rays_host without a device: the symbols, the header signatures, the refusals that come
before any device call (there is no GPU where `-m "not gpu"` runs)."""
import ctypes
import os
import re

from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "lidarshooter_hip.h")).read()


def test_occlusion_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in ("ls_occluded_rays", "ls_occluded_rays_host"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s


def test_occlusion_header_signatures():
    hdr = _header()
    assert re.search(r"int ls_occluded_rays\(ls_tracer \*tr, void \*hip_stream, const void \*d_rays, uint32_t n, void \*d_out\);", hdr)
    assert re.search(r"int ls_occluded_rays_host\(ls_tracer \*tr, const void \*rays, uint32_t n, void \*out\);", hdr)


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    buf = (ctypes.c_uint8 * 64)()
    INVALID_ARGUMENT = -2
    for n in (0, 1):
        p = buf if n else None
        assert L.ls_occluded_rays(None, None, p, n, p) == INVALID_ARGUMENT
        assert L.ls_occluded_rays_host(None, p, n, p) == INVALID_ARGUMENT
    assert list(buf) == [0] * 64


def test_abi_version_is_still_4(capi):
    assert capi.load().ls_abi_version() == 4
