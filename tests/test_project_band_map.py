"""k_project's start of a footprint's channel band by guess and verify (csrc/ls_band_map.h) without a device: the map the
library fits to a table of tan(elevation + margin), and the kernel's own start arithmetic (ls_debug_band_guess, the host
compilation of band_guess), against the true lower bound -- for every table value, its neighbours one ulp away, the midpoints,
both infinities and values beyond both ends.  The kernel checks its start against the table and bisects when the check fails,
so none of this decides what a frame returns; it decides whether the walk is as short as the handle was told."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

f32p = ctypes.POINTER(ctypes.c_float)
u32p = ctypes.POINTER(ctypes.c_uint32)
ELEV_MARGIN_DEG = 0.001


def tan_up_table(vertical_deg):
    """the ascending table as fill_tables builds it: channels by ascending elevation, tan(chi + margin) in double, rounded to float,
    one ulp up"""
    chi = np.sort(np.asarray(vertical_deg, np.float32).astype(np.float64), kind="stable")
    t = np.tan(np.radians(chi + ELEV_MARGIN_DEG)).astype(np.float32)
    return np.nextafter(t, np.float32(np.inf))


def fit(L, up):
    m = np.zeros(8, np.float32)
    assert L.ls_debug_band_map_fit(up.ctypes.data_as(f32p), len(up), m.ctypes.data_as(f32p)) == 0
    back, walk = (int(x) for x in m[6:].view(np.int32))
    return m, back, walk


def probes(up):
    p = [np.float32(-np.inf), np.float32(np.inf), np.float32(0.0), up[0] - np.float32(1.0), up[-1] + np.float32(1.0),
         np.float32(-3e38), np.float32(3e38), up[0] * np.float32(2) - np.float32(1), up[-1] * np.float32(2) + np.float32(1)]
    p += list(up) + list(np.nextafter(up, np.float32(-np.inf))) + list(np.nextafter(up, np.float32(np.inf)))
    p += list(((up[:-1].astype(np.float64) + up[1:].astype(np.float64)) * 0.5).astype(np.float32))
    return np.asarray(p, np.float32)


def bisection_rounds(V):
    return int(V).bit_length()


def check_table(L, up):
    """-> (back, walk); asserts the map's promises over the probes when the handle would use it"""
    m, back, walk = fit(L, up)
    V = len(up)
    if walk < 0:
        return back, walk
    assert back >= 0 and 1 + walk < bisection_rounds(V), (back, walk, V)
    D = max(back, walk - back)   # the largest distance between the raw guess and the lower bound
    start = ctypes.c_uint32()
    for t in probes(up):
        assert L.ls_debug_band_guess(m.ctypes.data_as(f32p), V, ctypes.c_float(t), ctypes.byref(start)) == 0
        lb = int(np.searchsorted(up, t, side="left"))
        s = start.value
        assert s <= lb, (t, s, lb)                  # the guess, stepped back, is not above the true lower bound
        assert lb - s <= walk <= 2 * D, (t, s, lb, walk, D)   # ... which the walk reaches within 2 D steps (2 D + 1 reads)
    return back, walk


def clusters16():
    return list(np.linspace(-20.0, -12.0, 8)) + list(np.linspace(8.0, 15.0, 8))     # one gap of 20 degrees


def repeated16():
    return [-15, -13, -11, -9, -7, -5, -3, -1, -1, 1, 3, 5, 7, 9, 11, 13]


def nonuniform33():
    return list(np.sign(np.linspace(-1, 1, 33)) * np.abs(np.linspace(-1, 1, 33)) ** 5 * 60.0)


SEVEN = {
    "v1": [3.0],
    "v2": [-1.0, 2.0],
    "uniform16": list(np.linspace(-15.0, 15.0, 16)),
    "clusters16": clusters16(),
    "repeated16": repeated16(),
    "nonuniform33": nonuniform33(),
    "descending16": list(np.linspace(15.0, -15.0, 16)),
}


def test_band_map_symbols(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in ("ls_debug_band_map_fit", "ls_debug_band_guess", "ls_debug_tracer_band_map"):
        assert s in capi.DEBUG_SYMBOLS and hasattr(lib, s), s
    dbg = open(os.path.join(ROOT, "include", "lidarshooter_hip_debug.h")).read()
    assert re.search(r"int ls_debug_band_map_fit\(const float \*tan_up, uint32_t V, float map8\[8\]\);", dbg)
    assert re.search(r"int ls_debug_band_guess\(const float map8\[8\], uint32_t V, float t, uint32_t \*start\);", dbg)
    L = capi.load()
    m = np.zeros(8, np.float32)
    up = np.float32([0.0, 1.0])
    assert L.ls_debug_band_map_fit(None, 2, m.ctypes.data_as(f32p)) == -2
    assert L.ls_debug_band_map_fit(up.ctypes.data_as(f32p), 0, m.ctypes.data_as(f32p)) == -2
    assert L.ls_debug_band_map_fit(up[::-1].copy().ctypes.data_as(f32p), 2, m.ctypes.data_as(f32p)) == -2   # not ascending
    assert L.ls_debug_tracer_band_map(None, m.ctypes.data_as(f32p)) == -2


@pytest.mark.parametrize("name", list(SEVEN))
def test_the_seven_tables(capi, name):
    L = capi.load()
    back, walk = check_table(L, tan_up_table(SEVEN[name]))
    if name in ("v1", "nonuniform33"):
        assert walk < 0   # nothing to fit / the walk would not beat the bisection: the handle bisects
    if name in ("uniform16", "descending16"):
        assert back == 0 and walk == 1


def test_the_shipped_sensors_are_one_step_from_the_guess(capi):
    """SYN-128 and the XT-32 are uniform in angle: the raw guess is never more than one position from the lower bound"""
    from lidarshooter_amd import synth
    L = capi.load()
    for vert in (synth.syn_vertical(), np.linspace(-16.0, 15.0, 32)):
        back, walk = check_table(L, tan_up_table(vert))
        assert walk >= 0 and max(back, walk - back) <= 1, (back, walk)


def test_random_monotone_tables(capi):
    L = capi.load()
    rng = np.random.default_rng(20240607)
    used = 0
    for k in range(200):
        V = int(rng.integers(1, 301))
        kind = k % 4
        if kind == 0:      # uniform in angle, random range
            lo = rng.uniform(-60, 20)
            chi = np.linspace(lo, lo + rng.uniform(1, 60), V)
        elif kind == 1:    # random, sorted
            chi = rng.uniform(-85, 85, V)
        elif kind == 2:    # dense centre, sparse edges
            chi = np.tanh(rng.normal(0, 1, V)) * rng.uniform(5, 80)
        else:              # uniform with jitter and a few repeats
            chi = np.linspace(-25, 15, V) + rng.normal(0, 0.05, V)
            chi[rng.integers(0, V, V // 10)] = chi[0]
        back, walk = check_table(L, tan_up_table(chi))
        used += walk >= 0
    assert used >= 50   # the uniform quarter at the least takes the map


def test_infinite_entries_are_left_out_of_the_fit(capi):
    L = capi.load()
    up = np.concatenate([[np.float32(-np.inf)], tan_up_table(np.linspace(-15, 15, 16)), [np.float32(np.inf)]]).astype(np.float32)
    back, walk = check_table(L, up)
    assert walk >= 0
