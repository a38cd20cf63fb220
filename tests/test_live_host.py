"""Live and dead slots (rt_scene_update_live* / rt_scene_rebuild_n* / rt_scene_live, csrc/rt_dynamic.hpp) without a GPU: the
ABI, the refit rule over live items in its numpy restatement, the argument checks made before any device is touched, and the residency of
the new kernels read back from the code object.  One test needs a real dynamic scene and carries the gpu mark."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = {rta.RT_F32: np.float32, rta.RT_F64: np.float64}
ENTRIES = ("rt_scene_update_live", "rt_scene_update_live_device", "rt_scene_rebuild_n", "rt_scene_rebuild_n_device", "rt_scene_live")
PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])


def as_bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


# ---- the ABI ----

def test_the_new_symbols_are_declared_bound_and_exported_by_both_libraries():
    assert capi.ABI_VERSION == 5 and set(ENTRIES) <= set(capi.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "rtrace_hip.h")).read()
    assert "#define RTRACE_HIP_ABI_VERSION 5" in header
    declared = set(re.findall(r"\b(rt_[a-z_]+)\s*\(", header))
    assert declared == set(capi.SYMBOLS), declared ^ set(capi.SYMBOLS)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert hasattr(capi.lib, name) and getattr(capi.lib, name).argtypes, name
        assert re.search(r"\bfn %s\(" % name, integration), name
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        exported = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines() if l.strip()}
        assert set(ENTRIES) <= exported, path
        assert ctypes.CDLL(path).rt_abi_version() == 5
    product = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", capi.PRODUCT_LIB_PATH], capture_output=True, text=True, check=True).stdout.splitlines() if l.strip()}
    assert {s for s in product if s.startswith("rt_")} == declared
    # the Python surface: defaults that keep every existing call's meaning
    import inspect
    assert inspect.signature(rta.DeviceScene.update).parameters["live"].default is None
    assert inspect.signature(rta.DeviceScene.rebuild).parameters["n"].default is None
    assert inspect.signature(rta.refit_bounds).parameters["live"].default is None and callable(rta.DeviceScene.live)


# ---- the refit rule over live items ----

def scene_of(precision, n=600, seed=5):
    rng = np.random.default_rng(seed)
    items = np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(0.02, 0.12, (n, 1))], axis=1).astype(REAL[precision])
    return items, rta.balanced_ranges(n, 4)


@PRECISIONS
def test_all_ones_is_the_rule_without_liveness(precision):
    items, rg = scene_of(precision)
    want = rta.refit_bounds(items, rg, precision)
    for ones in (np.ones(600, dtype=np.uint8), np.ones(600, dtype=bool), np.full(600, 7, dtype=np.uint8)):       # nonzero = live
        np.testing.assert_array_equal(as_bits(rta.refit_bounds(items, rg, precision, live=ones)), as_bits(want))
    with pytest.raises(ValueError):
        rta.refit_bounds(items, rg, precision, live=np.ones(599, dtype=np.uint8))


@PRECISIONS
def test_a_group_takes_the_rule_over_its_live_items_and_a_dead_group_is_zero(precision):
    R = REAL[precision]
    items, rg = scene_of(precision)
    live = np.zeros(600, dtype=np.uint8)
    live[[3, 256, 257, 420]] = 1
    got = rta.refit_bounds(items, rg, precision, live=live)
    grow = R(1.0) + R(8.0) * np.finfo(R).eps
    seen_one = seen_two = seen_dead = 0
    for g, (first, count) in enumerate(rg):
        idx = first + np.flatnonzero(live[first:first + count])
        if len(idx) == 0:                                            # a dead group
            assert not as_bits(got[g]).any(), g
            seen_dead += 1
        elif len(idx) == 1:                                          # one live item: the box is its own, the centre its centre, reach = 0 + r
            it = items[idx[0]]
            lo, hi = it[:3] - it[3], it[:3] + it[3]
            c = (lo + hi) * R(0.5)
            d = it[:3] - c
            s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            tiny = np.ldexp(R(1.0), -80 if R == np.float32 else -918)
            dist = np.sqrt(s) if s >= tiny else (abs(d[0]) + abs(d[1])) + abs(d[2])
            np.testing.assert_array_equal(as_bits(got[g]), as_bits(np.array([c[0], c[1], c[2], (dist + it[3]) * grow], dtype=R)), err_msg=str(g))
            seen_one += 1
        else:                                                        # several: the rule over exactly those items, as one group of a compact array
            sub = np.ascontiguousarray(items[idx])
            np.testing.assert_array_equal(as_bits(got[g]), as_bits(rta.refit_bounds(sub, [[0, len(idx)]], precision)[0]), err_msg=str(g))
            seen_two += 1
    assert seen_one >= 4 and seen_two >= 2 and seen_dead >= 100
    assert (got[:, 3] >= 0).all() and ((got[:, 3] == 0) == ~np.array([live[f:f + c].any() for f, c in rg])).all()


@PRECISIONS
def test_the_values_in_dead_slots_take_no_part(precision):
    R = REAL[precision]
    items, rg = scene_of(precision)
    live = (np.random.default_rng(8).random(600) < 0.5).astype(np.uint8)
    want = rta.refit_bounds(items, rg, precision, live=live)
    for fill in (np.nan, np.inf, -np.inf, 0.0, 1e30, -3.0):
        other = items.copy()
        other[live == 0] = R(fill)
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(as_bits(rta.refit_bounds(other, rg, precision, live=live)), as_bits(want), err_msg=str(fill))
    # ... nor does the order of the live items inside a group, or how many dead ones lie between them
    root = rta.refit_bounds(items, [[0, 600]], precision, live=live)[0]
    compact = np.ascontiguousarray(items[live != 0][::-1])
    np.testing.assert_array_equal(as_bits(rta.refit_bounds(compact, [[0, len(compact)]], precision)[0]), as_bits(root))


# ---- argument errors of the host entries ----

def test_argument_errors_are_reported_before_any_device_is_touched():
    spheres = np.array([[0, 0, 0, 1], [2, 0, 0, 1], [0, 3, 0, 0.5]], dtype=np.float32)
    order = np.full(3, 77, dtype=np.uint32)
    live = np.ones(3, dtype=np.uint8)
    # a zeroed block stands in for a scene: precision 0 is RT_F32, its capacity is 0 items, and no call below gets past its argument checks
    block = ctypes.create_string_buffer(1 << 20)
    stand_in = ctypes.cast(block, ctypes.c_void_p)
    last = lambda: capi.lib.rt_last_error_message()
    for call, tail in ((capi.lib.rt_scene_rebuild_n, ()), (capi.lib.rt_scene_rebuild_n_device, (None,))):
        assert call(None, spheres.ctypes.data, 3, order.ctypes.data, *tail) == capi.RT_ERR_INVALID_ARGUMENT
        assert call(stand_in, None, 3, order.ctypes.data, *tail) == capi.RT_ERR_INVALID_ARGUMENT and b"NULL spheres" in last()      # NULL spheres with n > 0
        assert call(stand_in, spheres.ctypes.data, 3, order.ctypes.data, *tail) == capi.RT_ERR_INVALID_ARGUMENT and b"capacity" in last()      # n > n_items
        assert call(stand_in, spheres.ctypes.data, 1, None, *tail) == capi.RT_ERR_INVALID_ARGUMENT and b"capacity" in last()
        # n == 0 with NULL spheres is no argument error: the stand-in is refused for what it is, a scene that is not dynamic
        assert call(stand_in, None, 0, None, *tail) == capi.RT_ERR_UNSUPPORTED
    assert (order == 77).all()
    ul, uld = capi.lib.rt_scene_update_live, capi.lib.rt_scene_update_live_device
    assert ul(None, spheres.ctypes.data, None, live.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    assert ul(stand_in, None, None, live.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    assert ul(None, spheres.ctypes.data, None, None) == capi.RT_ERR_INVALID_ARGUMENT          # live == NULL: rt_scene_update's own checks
    assert uld(None, spheres.ctypes.data, None, live.ctypes.data, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert uld(stand_in, None, None, live.ctypes.data, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert ul(stand_in, spheres.ctypes.data, None, live.ctypes.data) == capi.RT_ERR_UNSUPPORTED        # not a dynamic scene
    assert uld(stand_in, spheres.ctypes.data, None, live.ctypes.data, None) == capi.RT_ERR_UNSUPPORTED
    assert capi.lib.rt_scene_live(None, live.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_live(stand_in, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_live(stand_in, live.ctypes.data) == capi.RT_OK and (live == 1).all()      # a static scene of no items: nothing written


@pytest.mark.gpu
@PRECISIONS
def test_only_live_items_are_validated(precision):
    # The values are checked against the scene's own capacity, so this needs a dynamic scene, and a dynamic scene needs a device: hence the
    # mark.  The refusals come before the device is touched: the scene's bounds are what they were.
    R = REAL[precision]
    items, rg = scene_of(precision, n=40)
    light, eye = rta.normalized((-1.0, -3.0, 2.0), precision), np.array([0, 0, -4], dtype=R)
    h = ctypes.c_void_p()
    st = capi.lib.rt_scene_create_dynamic(0, precision, items.ctypes.data, 40, light.ctypes.data, eye.ctypes.data, None, rg.ctypes.data, len(rg), ctypes.byref(h))
    assert st == capi.RT_OK, (st, capi.lib.rt_last_error_message())
    try:
        before = np.zeros((len(rg), 4), dtype=R)
        assert capi.lib.rt_scene_bounds(h, before.ctypes.data) == capi.RT_OK
        live = np.ones(40, dtype=np.uint8)
        for col, v in ((3, 0.0), (3, -1.0), (0, np.nan), (1, np.inf), (2, 2e15), (3, np.nan)):
            broken = items.copy()
            broken[17, col] = v
            live[17] = 1                                             # a live item with these bits is refused ...
            assert capi.lib.rt_scene_update_live(h, broken.ctypes.data, None, live.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT, (col, v)
            assert b"rt_scene_update_live" in capi.lib.rt_last_error_message()
            after = np.zeros_like(before)
            assert capi.lib.rt_scene_bounds(h, after.ctypes.data) == capi.RT_OK
            np.testing.assert_array_equal(as_bits(after), as_bits(before))
            live[17] = 0                                             # ... and the same bits in a dead slot are accepted
            assert capi.lib.rt_scene_update_live(h, broken.ctypes.data, None, live.ctypes.data) == capi.RT_OK, (col, v, capi.lib.rt_last_error_message())
            assert capi.lib.rt_scene_bounds(h, after.ctypes.data) == capi.RT_OK
            np.testing.assert_array_equal(as_bits(after), as_bits(rta.refit_bounds(items, rg, precision, live=live)))
            assert capi.lib.rt_scene_update(h, items.ctypes.data, None) == capi.RT_OK
        bad = items.copy()
        bad[5, 3] = 0.0
        assert capi.lib.rt_scene_rebuild_n(h, bad.ctypes.data, 6, None) == capi.RT_ERR_INVALID_ARGUMENT       # among the n: refused
        assert capi.lib.rt_scene_rebuild_n(h, bad.ctypes.data, 5, None) == capi.RT_OK                         # behind them: never read
        assert capi.lib.rt_scene_rebuild_n(h, items.ctypes.data, 41, None) == capi.RT_ERR_INVALID_ARGUMENT
    finally:
        capi.lib.rt_scene_destroy(h)


# ---- the kernels ----

def test_the_live_kernels_keep_eight_waves_per_simd_and_use_no_scratch(tmp_path):
    from tests.test_kernel_resources import _kernels, LIB, TEST_LIB
    names = ("refit_box_live", "refit_reach_live", "dynamic_rewrite_live")
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        mine = sorted(n for n in k if re.match(r"rt::k_(%s)<" % "|".join(names), n))
        assert mine == sorted("rt::k_%s<%s, %s>" % (name, t, p) for name in names for t in ("float", "double") for p in ("false", "true")), mine
        for n in mine:
            assert k[n]["sgpr"] <= 80 and k[n]["vgpr"] <= 64 and k[n]["scratch"] == 0, (n, k[n])
