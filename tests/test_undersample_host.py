"""Undersampled camera frames (rt_render_camera_undersampled*, csrc/rt_undersample.hpp) without a GPU: the ABI, the argument checks made
before any device is touched, the residency of the k_trace_undersampled flavours read back from the code object, and the host-side
definition of a step-s frame (expand_undersampled, undersample_cells) against brute force."""
import ctypes
import os
import re

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.test_camera_host import IDENTITY, _cam, _stand_in, bad_cameras
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB

ENTRIES = ("rt_render_camera_undersampled", "rt_render_camera_undersampled_device")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_libraries_export_the_undersampled_entries_at_abi_5():
    assert capi.ABI_VERSION == 5 and capi.RT_UNDERSAMPLE_MAX_STEP == 64 and rta.RT_UNDERSAMPLE_MAX_STEP == 64
    assert set(ENTRIES) <= set(capi.SYMBOLS)
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert lib.rt_abi_version() == 5
        for name in ENTRIES:
            assert getattr(lib, name) is not None
    header = open(ROOT + "/include/rtrace_hip.h").read()
    assert re.search(r"#define\s+RT_UNDERSAMPLE_MAX_STEP\s+64\b", header)
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRIES) <= declared and declared == set(capi.SYMBOLS), declared ^ set(capi.SYMBOLS)
    assert "rt_*" in open(ROOT + "/rust-tracer_amd/csrc/exports.map").read()


def _call(entry, scene, cam, regions, n, step, prev, out, opts=(64, 48, 1)):
    o = capi.Options(*opts)
    f = getattr(capi.lib, entry)
    if entry == "rt_render_camera_undersampled":
        return f(scene, ctypes.byref(o), cam, regions, n, step, prev, out, None)
    return f(scene, ctypes.byref(o), cam, regions, n, step, prev, out, None, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_step_errors_are_reported_before_any_device_is_touched(entry):
    _keep, handle = _stand_in()
    regions = (capi.Region * 1)(capi.Region(0, 48, 64, 0))
    out = ctypes.create_string_buffer(64 * 48 * 4)
    cam = _cam(IDENTITY)
    for step in (0, 65, 1000, 0xFFFFFFFF):
        assert _call(entry, handle, cam, regions, 1, step, 0, out) == capi.RT_ERR_INVALID_ARGUMENT, step
        assert b"step" in capi.lib.rt_last_error_message() and b"prev_step" not in capi.lib.rt_last_error_message()
    for step in (1, 2, 5, 8, 64):
        for prev in (step, 3 * step, 2 * step + 1, 2 * step - 1, 4 * step):
            assert _call(entry, handle, cam, regions, 1, step, prev, out) == capi.RT_ERR_INVALID_ARGUMENT, (step, prev)
            assert b"prev_step" in capi.lib.rt_last_error_message(), (step, prev)
    # the step is checked before the scene is looked at: a NULL scene with a bad step names the step
    assert _call(entry, None, cam, regions, 1, 0, 0, out) == capi.RT_ERR_INVALID_ARGUMENT
    assert b"step" in capi.lib.rt_last_error_message()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("step,prev", [(1, 0), (4, 0), (4, 8), (64, 0), (3, 6)])
def test_camera_argument_errors_are_reported_before_any_device_is_touched(entry, step, prev):
    _keep, handle = _stand_in()
    regions = (capi.Region * 1)(capi.Region(0, 48, 64, 0))
    out = ctypes.create_string_buffer(64 * 48 * 4)
    cam = _cam(IDENTITY)
    call = lambda *a, **k: _call(entry, a[0], a[1], a[2], a[3], step, prev, a[4], **k)
    assert call(None, cam, regions, 1, out) == capi.RT_ERR_INVALID_ARGUMENT          # NULL scene
    assert call(handle, None, regions, 1, out) == capi.RT_ERR_INVALID_ARGUMENT       # NULL camera
    assert b"camera" in capi.lib.rt_last_error_message()
    assert call(handle, cam, None, 1, out) == capi.RT_ERR_INVALID_ARGUMENT           # NULL regions
    assert call(handle, cam, regions, 1, None) == capi.RT_ERR_INVALID_ARGUMENT       # NULL buffer
    assert call(handle, cam, regions, 0, out) == capi.RT_ERR_INVALID_ARGUMENT        # n_tiles == 0
    assert call(handle, cam, regions, 1, out, opts=(0, 48, 1)) == capi.RT_ERR_INVALID_ARGUMENT      # width 0
    for name, c in bad_cameras():
        assert call(handle, _cam(c), regions, 1, out) == capi.RT_ERR_INVALID_ARGUMENT, name
        assert b"camera" in capi.lib.rt_last_error_message(), name
    for reg in ((0, 49, 64, 0), (0, 48, 65, 0), (10, 48, 10, 0), (0, 20, 64, 20)):
        bad = (capi.Region * 1)(capi.Region(*reg))
        assert call(handle, cam, bad, 1, out) == capi.RT_ERR_INVALID_REGION, reg


def test_the_undersampled_kernels_keep_eight_waves_per_simd(tmp_path):
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_trace_undersampled<")]
        assert sorted(flavours) == sorted("rt::k_trace_undersampled<%s, %s>" % (t, c) for t in ("float", "double") for c in ("true", "false")), flavours
        for n in flavours:
            assert k[n]["scratch"] == 0, (n, k[n])
            if ", false>" in n:
                assert k[n]["sgpr"] <= 80 and k[n]["vgpr"] <= 64, (n, k[n])


# ---- the definition, on the host ----

def brute_expand(image, regions, step):
    return np.array([image[y - y % step, x - x % step] for l, t, r, b in regions for y in range(b, t) for x in range(l, r)],
                    dtype=np.uint8).reshape(-1)


def brute_cells(regions, step, prev_step):
    """(traced, reused) by enumeration: the cells of each region are the distinct anchors of its pixels."""
    traced = reused = 0
    for l, t, r, b in regions:
        anchors = {(x - x % step, y - y % step) for y in range(b, t) for x in range(l, r)}
        kept = {a for a in anchors if prev_step and a[0] % prev_step == 0 and a[1] % prev_step == 0}
        traced += len(anchors) - len(kept)
        reused += len(kept)
    return traced, reused


def region_lists(w, h, rng):
    """Tile lists over a w x h image: the whole image, a bucket grid off the lattice, odd rectangles that overlap and do not cover it."""
    whole = [(0, h, w, 0)]
    grid = [(x, min(y + 24, h), min(x + 24, w), y) for y in range(0, h, 24) for x in range(0, w, 24)]
    odd = []
    for _ in range(5):
        l, b = int(rng.integers(0, w - 1)), int(rng.integers(0, h - 1))
        odd.append((l, int(rng.integers(b + 1, h + 1)), int(rng.integers(l + 1, w + 1)), b))
    return whole, grid, odd + [(w - 1, h, w, h - 1), (0, 1, 1, 0)]


@pytest.mark.parametrize("step", [1, 2, 3, 5, 8, 64])
def test_expand_undersampled_is_the_definition(step):
    rng = np.random.default_rng(100 + step)
    for w, h in ((37, 29), (64, 48), (130, 71)):
        image = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        for regions in region_lists(w, h, rng):
            got = rta.expand_undersampled(image, regions, step)
            assert got.dtype == np.uint8 and got.shape == (4 * sum((r - l) * (t - b) for l, t, r, b in regions),)
            np.testing.assert_array_equal(got, brute_expand(image, regions, step))
    if step == 1:
        np.testing.assert_array_equal(rta.expand_undersampled(image, [(0, h, w, 0)], 1), image.reshape(-1))


def test_expand_undersampled_rejects_what_it_cannot_expand():
    image = np.zeros((8, 8, 4), dtype=np.uint8)
    with pytest.raises(ValueError):
        rta.expand_undersampled(image, [(0, 8, 8, 0)], 0)
    with pytest.raises(ValueError):
        rta.expand_undersampled(image, [(0, 9, 8, 0)], 2)
    with pytest.raises(ValueError):
        rta.expand_undersampled(image[:, :, :3], [(0, 8, 8, 0)], 2)


@pytest.mark.parametrize("step", [1, 2, 3, 4, 5, 8, 16, 32, 64])
def test_the_cell_counts_are_those_of_brute_force(step):
    rng = np.random.default_rng(200 + step)
    for w, h in ((37, 29), (130, 71), (200, 150)):
        for regions in region_lists(w, h, rng):
            for prev in (0, 2 * step):
                assert rta.undersample_cells(regions, step, prev) == brute_cells(regions, step, prev), (w, h, regions, prev)
    # tiles on the coarsest lattice: the chain traces every pixel exactly once
    grid = [(x, min(y + 64, 150), min(x + 64, 200), y) for y in range(0, 150, 64) for x in range(0, 200, 64)]
    for regions in ([(0, 150, 200, 0)], grid):
        for first in (8, 64):
            steps = rta.progressive_steps(first)
            total = sum(rta.undersample_cells(regions, s, 0 if s == first else 2 * s)[0] for s in steps)
            assert total == 200 * 150
    with pytest.raises(ValueError):
        rta.undersample_cells([(0, 8, 8, 0)], 2, 3)


def test_render_camera_progressive_rejects_a_first_step_that_is_no_power_of_two_up_to_64():
    assert rta.progressive_steps(8) == [8, 4, 2, 1] and rta.progressive_steps(1) == [1]
    assert rta.progressive_steps(64) == [64, 32, 16, 8, 4, 2, 1]
    for bad in (0, 3, 128, -8, 6, 2.0, True):
        with pytest.raises(ValueError):
            rta.progressive_steps(bad)
        # the method raises when it is called, before it looks at the scene, not at the first next()
        with pytest.raises(ValueError):
            rta.DeviceScene.render_camera_progressive(None, (64, 48, 1), None, [(0, 48, 64, 0)], first_step=bad)
