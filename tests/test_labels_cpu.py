"""ls_object_labels / ls_object_labels_host without a device: the symbols, the header signatures, the record's size, the refusals
that come before any device call (there is no GPU where `-m "not gpu"` runs), and the numpy reference's own reduction."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "lidarshooter_hip.h")).read()


def test_label_symbols_are_exported(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in ("ls_object_labels", "ls_object_labels_host"):
        assert s in capi.SYMBOLS
        assert hasattr(lib, s), s


def test_label_header_signatures():
    hdr = re.sub(r"\s+", " ", _header())
    assert ("int ls_object_labels(ls_tracer *tr, void *hip_stream, uint32_t flags, const void *d_rays, uint32_t n_rays, "
            "const void *d_hits, const uint32_t *d_count, uint32_t n, void *d_labels, uint32_t n_labels);") in hdr
    assert ("int ls_object_labels_host(ls_tracer *tr, uint32_t flags, const void *rays, uint32_t n_rays, "
            "const void *hits, uint32_t n, void *labels, uint32_t n_labels);") in hdr
    assert "#define LS_LABEL_FOOTPRINT 1u" in hdr


def test_label_record_is_64_bytes_with_the_header_layout(capi):
    from labels_reference import LABEL_DTYPE
    d = capi.OBJECT_LABEL_DTYPE
    assert d.itemsize == 64 and d == LABEL_DTYPE
    assert [(n, d.fields[n][1]) for n in d.names] == [("n_hits", 0), ("n_alone", 4), ("t_min", 8), ("ray_min", 12), ("t_max", 16),
                                                       ("ray_max", 20), ("lo", 24), ("hi", 36), ("flags", 48), ("reserved", 52)]
    body = re.search(r"typedef struct ls_object_label \{(.*?)\} ls_object_label;", _header(), re.S).group(1)
    fields = re.findall(r"^\s*(?:uint32_t|float)\s+(\w+)", body, re.M)
    assert fields == list(d.names)
    assert capi.LS_LABEL_FOOTPRINT == 1
    e = capi.Tracer.emptyObjectLabels(2)
    assert np.all(e["t_min"] == np.inf) and np.all(e["hi"] == -np.inf) and np.all(e["ray_max"] == 0xFFFFFFFF) and np.all(e["flags"] == 0)


def test_null_handle_is_refused_without_a_device(capi):
    L = capi.load()
    buf = (ctypes.c_uint8 * 128)()
    INVALID_ARGUMENT = -2
    for n in (0, 1):
        p = buf if n else None
        for flags in (0, 1):
            assert L.ls_object_labels(None, None, flags, p, n, p, None, n, p, n) == INVALID_ARGUMENT
            assert L.ls_object_labels_host(None, flags, p, n, p, n, p, n) == INVALID_ARGUMENT
    assert list(buf) == [0] * 128


def test_abi_version_is_still_4(capi):
    assert capi.load().ls_abi_version() == 4


def test_reference_reduction_applies_the_counting_rule():
    """the reference on a hand-made case: ties go to the lowest ray, negative coordinates and -0 order as floats, and a record out
    of any bound counts nowhere"""
    import labels_reference as ref
    f = lambda x: np.float32(x).view(np.uint32)
    rays = np.zeros((4, 8), np.float32)
    rays[:, 4:7] = [[1, 0, 0], [0, -1, 0], [0, 0, 2], [np.nan, 0, 1]]
    rays[:, 0:3] = [[0, 0, 0], [1, 1, 1], [-3, 0, 0], [0, 0, 0]]
    rays[:, 7] = np.inf
    rec = np.array([[2, 1, 0, f(2.0)], [0, 1, 1, f(2.0)], [1, 1, 0, f(0.5)], [1, 0, 0, f(0.5)],
                    [0, 1, 2, f(1.0)],          # prim out of range
                    [4, 1, 0, f(1.0)],          # ray out of range
                    [3, 1, 0, f(1.0)],          # a ray that is not walked
                    [0, 2, 0, f(1.0)],          # a free id
                    [0, 5, 0, f(1.0)],          # beyond n_labels
                    [0, 1, 0, f(np.nan)], [0, 1, 0, f(-1.0)], [0, 1, 0, f(np.inf)]], np.uint32)
    pts = ref.record_points(rec, rays)
    assert np.array_equal(pts[0], np.float32([-3, 0, 4])) and np.array_equal(pts[2], np.float32([1, 0.5, 1]))
    out = ref.reduce_records(rec, pts, {0: 1, 1: 2}, 4, 4, rays)
    assert list(out["n_hits"]) == [1, 3, 0, 0] and list(out["flags"]) == [1, 1, 0, 0] and np.all(out["n_alone"] == 0)
    assert out["t_min"][1] == 0.5 and out["ray_min"][1] == 1 and out["t_max"][1] == 2.0 and out["ray_max"][1] == 0
    assert np.array_equal(out["lo"][1], np.float32([-3, 0, 0])) and np.array_equal(out["hi"][1], np.float32([2, 0.5, 4]))
    assert np.array_equal(out[2:].tobytes(), ref.empty_labels(2).tobytes())
    # shuffled records: the same bytes
    perm = np.random.default_rng(1).permutation(rec.shape[0])
    assert ref.reduce_records(rec[perm], pts[perm], {0: 1, 1: 2}, 4, 4, rays).tobytes() == out.tobytes()
    # -0 orders below +0
    k = ref._key(np.float32([-0.0, 0.0, -1.0, 1.0, -np.inf, np.inf]))
    assert list(np.argsort(k, kind="stable")) == [4, 2, 0, 1, 3, 5]
    assert np.array_equal(ref._unkey(k).view(np.uint32), np.float32([-0.0, 0.0, -1.0, 1.0, -np.inf, np.inf]).view(np.uint32))
