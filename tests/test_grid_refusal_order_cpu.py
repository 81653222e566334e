"""The descriptor checks of ls_occupancy_grid, ls_scene_grid, ls_scene_distance_grid and ls_sample_surface share the box's rules
(csrc/ls_grid_box.h) and keep their own around them.  Each descriptor here breaks two rules at once; the code that comes back says
which of the two the check reached first.  The expected codes are literals, recorded from the library as it was before the rules
were shared."""
import ctypes

import numpy as np
import pytest

INVALID_ARGUMENT, OUT_OF_RANGE = -2, -9
NAN, INF = float("nan"), float("inf")


def _occupancy(capi, origin=(0.0, 0.0, 0.0), cell=1.0, dims=(4, 4, 4), flags=0, min_range=0.0, max_range=10.0, reserved=(0, 0)):
    d = capi.OccupancyGridDesc.make(origin, cell, dims, flags, min_range, max_range)
    d.reserved[0], d.reserved[1] = reserved
    return capi.load().ls_occupancy_grid_check(ctypes.byref(d))


def _scene(capi, origin=(0.0, 0.0, 0.0), cell=1.0, dims=(4, 4, 4), flags=0):
    return capi.load().ls_scene_grid_check(ctypes.byref(capi.SceneGridDesc.make(origin, cell, dims, flags)))


def _distance(capi, origin=(0.0, 0.0, 0.0), cell=1.0, dims=(4, 4, 4), flags=0, trunc=1.0, reserved=(0, 0, 0)):
    d = capi.DistanceGridDesc.make(origin, cell, dims, flags, trunc)
    for k in range(3):
        d.reserved[k] = reserved[k]
    return capi.load().ls_scene_distance_grid_check(ctypes.byref(d))


def _surface(capi, flags=0, reserved=(0, 0, 0)):
    d = capi.SurfaceSampleDesc.make(16, flags=flags)
    for k in range(3):
        d.reserved[k] = reserved[k]
    return capi.load().ls_surface_sample_check(ctypes.byref(d))


CASES = [
    # ls_occupancy_grid_check: flags and reserved words, the box (origin, cell), the ranges; then the dimensions and the upper corner
    (_occupancy, dict(flags=4, origin=(NAN, 0.0, 0.0)), -2),
    (_occupancy, dict(flags=4, dims=(0, 4, 4)), -2),
    (_occupancy, dict(reserved=(0, 1), dims=(2049, 1, 1)), -2),
    (_occupancy, dict(origin=(0.0, INF, 0.0), dims=(4, 0, 4)), -2),
    (_occupancy, dict(cell=0.0, dims=(2048, 2048, 33)), -2),
    (_occupancy, dict(cell=NAN, min_range=-1.0), -2),
    (_occupancy, dict(min_range=-1.0, dims=(0, 4, 4)), -2),
    (_occupancy, dict(min_range=5.0, max_range=1.0, dims=(4, 4, 2049)), -2),
    (_occupancy, dict(max_range=INF, origin=(3e38, 0.0, 0.0), cell=1e35, dims=(2048, 1, 1)), -2),
    (_occupancy, dict(dims=(0, 2049, 4), origin=(3e38, 0.0, 0.0), cell=1e35), -9),
    (_occupancy, dict(dims=(2048, 2048, 33), origin=(0.0, 0.0, 3e38), cell=1e37), -9),
    # ls_scene_grid_check: flags, the box; then the dimensions and the upper corner
    (_scene, dict(flags=2, origin=(0.0, 0.0, -INF)), -2),
    (_scene, dict(flags=2, dims=(0, 4, 4)), -2),
    (_scene, dict(origin=(NAN, 0.0, 0.0), cell=-1.0), -2),
    (_scene, dict(origin=(0.0, NAN, 0.0), dims=(2049, 1, 1)), -2),
    (_scene, dict(cell=INF, dims=(2048, 2048, 33)), -2),
    (_scene, dict(dims=(4, 4, 0), origin=(3e38, 0.0, 0.0), cell=1e35), -9),
    # ls_scene_distance_grid_check: flags and reserved words, the box, trunc; then the dimensions, the upper corner, trunc in cells
    (_distance, dict(flags=2, origin=(NAN, 0.0, 0.0)), -2),
    (_distance, dict(reserved=(0, 0, 1), trunc=100.0), -2),
    (_distance, dict(origin=(0.0, 0.0, INF), trunc=-1.0), -2),
    (_distance, dict(cell=0.0, trunc=NAN), -2),
    (_distance, dict(cell=-1.0, dims=(0, 4, 4), trunc=100.0), -2),
    (_distance, dict(trunc=NAN, dims=(0, 4, 4)), -2),
    (_distance, dict(trunc=-1.0, dims=(2048, 2048, 33)), -2),
    (_distance, dict(dims=(0, 4, 4), trunc=100.0), -9),
    (_distance, dict(dims=(2048, 2048, 33), trunc=33.0), -9),
    (_distance, dict(origin=(3e38, 0.0, 0.0), cell=1e35, dims=(2048, 1, 1), trunc=1e37), -9),
    # ls_surface_sample_check: flags, then the reserved words
    (_surface, dict(flags=1, reserved=(0, 0, 1)), -2),
    (_surface, dict(flags=0x80000000, reserved=(1, 0, 0)), -2),
    (_surface, dict(reserved=(1, 1, 0)), -2),
]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_two_broken_rules_answer_as_before(capi, k):
    check, broken, code = CASES[k]
    assert code in (INVALID_ARGUMENT, OUT_OF_RANGE)
    got = check(capi, **broken)
    assert got == code, (check.__name__, broken, got)


def test_the_sound_descriptors_pass(capi):
    assert _occupancy(capi) == 0 and _scene(capi) == 0 and _distance(capi) == 0 and _surface(capi) == 0
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.float32(3e38) + np.float32(2048) * np.float32(1e35))   # the corner the cases above rely on
