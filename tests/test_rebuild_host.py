"""Rebuilds (rt_sphere_order* / rt_balanced_ranges / rt_scene_rebuild*, csrc/rt_rebuild.hpp) without a GPU: the ABI, the topology rule
against its restatement and property by property, the sphere key on inputs whose keys can be written down, and the argument checks made
before any device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_sphere_order", "rt_sphere_order_device", "rt_balanced_ranges", "rt_scene_rebuild", "rt_scene_rebuild_device")
SIZES, LEAVES = (1, 2, 4, 5, 9, 257, 1000), (1, 4, 7)


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


# ---- the topology ----

@pytest.mark.parametrize("leaf_size", LEAVES)
@pytest.mark.parametrize("n", SIZES)
def test_balanced_ranges_are_the_stated_halving(n, leaf_size):
    rg = rta.balanced_ranges(n, leaf_size)
    assert rg.dtype == np.int32 and rg.ndim == 2 and rg.shape[1] == 2
    np.testing.assert_array_equal(rg, rta.balanced_ranges_reference(n, leaf_size))
    first, end = rg[:, 0].astype(np.int64), rg[:, 0].astype(np.int64) + rg[:, 1]
    assert tuple(rg[0]) == (0, n) and len(rg) <= 2 * n - 1 and (rg[:, 1] >= 1).all()
    # pre-order and laminar: walking the list with a stack of open groups, every group lies inside the group open above it and starts
    # where that group's earlier children ended
    open_groups, is_leaf = [], np.ones(len(rg), dtype=bool)
    for g in range(len(rg)):
        while open_groups and first[g] >= end[open_groups[-1]]:
            open_groups.pop()
        if open_groups:
            p = open_groups[-1]
            assert first[p] <= first[g] and end[g] <= end[p] and (first[g], end[g]) != (first[p], end[p]), (g, p)
            is_leaf[p] = False
        else:
            assert g == 0
        open_groups.append(g)
    # every leaf holds at most leaf_size items, and the leaves tile 0 .. n in order
    leaves = rg[is_leaf]
    assert (leaves[:, 1] <= leaf_size).all()
    assert leaves[0, 0] == 0 and (leaves[1:, 0] == leaves[:-1, 0] + leaves[:-1, 1]).all() and leaves[-1, 0] + leaves[-1, 1] == n
    # a group that is no leaf has exactly two children: the halves of the rule
    for g in np.flatnonzero(~is_leaf):
        assert rg[g, 1] > leaf_size
        left = (int(rg[g, 1]) + 1) // 2
        assert tuple(rg[g + 1]) == (rg[g, 0], left)
        right = np.flatnonzero((first == first[g] + left) & (end == end[g]))
        assert len(right) >= 1 and right[0] > g + 1


def test_balanced_ranges_argument_errors():
    rg, ng = np.zeros((8, 2), dtype=np.int32), ctypes.c_uint32(0)
    call = capi.lib.rt_balanced_ranges
    assert call(0, 4, rg.ctypes.data, ctypes.byref(ng)) == capi.RT_ERR_INVALID_ARGUMENT
    assert call(4, 0, rg.ctypes.data, ctypes.byref(ng)) == capi.RT_ERR_INVALID_ARGUMENT
    assert call(4, 4, None, ctypes.byref(ng)) == capi.RT_ERR_INVALID_ARGUMENT
    assert call(4, 4, rg.ctypes.data, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert b"rt_balanced_ranges" in capi.lib.rt_last_error_message()
    assert not rg.any() and ng.value == 0
    with pytest.raises(rta.RtError):
        rta.balanced_ranges(0)
    with pytest.raises(rta.RtError):
        rta.balanced_ranges(5, 0)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_refit_bounds_over_balanced_ranges_pass_the_checks_of_scene_creation(precision):
    # as far as creation runs without a device: everything that is RT_ERR_INVALID_ARGUMENT is decided before a device is looked for
    R = np.float32 if precision == rta.RT_F32 else np.float64
    rng = np.random.default_rng(12)
    light, eye = rta.normalized((-1.0, -3.0, 2.0), precision), np.array([0, 0, -4], dtype=R)
    for n, leaf_size in [(n, 4) for n in SIZES] + [(1000, 1), (1000, 7)]:
        items = np.concatenate([rng.uniform(-2, 2, (n, 3)), rng.uniform(0.05, 0.3, (n, 1))], axis=1).astype(R)
        rg = rta.balanced_ranges(n, leaf_size)
        bd = rta.refit_bounds(items, rg, precision)
        assert np.isfinite(bd).all() and (bd[:, 3] > 0).all()
        for bounds in (bd, None):
            h = ctypes.c_void_p()
            st = capi.lib.rt_scene_create_dynamic(0, precision, items.ctypes.data, n, light.ctypes.data, eye.ctypes.data,
                                                  None if bounds is None else bounds.ctypes.data, rg.ctypes.data, len(rg), ctypes.byref(h))
            assert st in (capi.RT_OK, capi.RT_ERR_NO_DEVICE), (n, leaf_size, st, capi.lib.rt_last_error_message())
            if st == capi.RT_OK:
                capi.lib.rt_scene_destroy(h)


# ---- the key ----

def order_of(spheres):
    return np.argsort(rta.sphere_keys(spheres), kind="stable")


def test_sphere_keys_of_one_sphere_and_of_coincident_centres_are_zero():
    assert list(rta.sphere_keys(np.array([[0.3, -0.7, 2.5, 0.125]]))) == [0]
    same = np.tile(np.array([[1.5, -2.25, 3.0, 1.0]], dtype=np.float32), (9, 1))
    same[:, 3] = np.arange(1, 10)
    assert not rta.sphere_keys(same).any()
    np.testing.assert_array_equal(order_of(same), np.arange(9))


def test_duplicated_centres_keep_the_callers_order():
    rng = np.random.default_rng(3)
    s = np.concatenate([rng.uniform(-1, 1, (40, 3)), rng.uniform(0.1, 0.2, (40, 1))], axis=1)
    s[20:] = s[:20]
    s[20:, 3] += 1.0
    s = s[rng.permutation(40)]
    keys, order = rta.sphere_keys(s), order_of(s)
    assert sorted(order) == list(range(40)) and (np.diff(keys[order].astype(np.int64)) >= 0).all()
    ties = np.flatnonzero(np.diff(keys[order].astype(np.int64)) == 0)
    assert len(ties) >= 20 and (order[ties] < order[ties + 1]).all()


def test_the_keys_of_a_lattice_are_its_morton_codes():
    # centres on {0, 1, 2, 3}^3: ext = 3 < 2^2, scale = 2^8, q = 256 * coordinate -- the coordinate's two bits are bits 8 and 9 of q,
    # which go to bits 24 + a and 27 + a of the key.  The z = 0 plane, x fastest, and what each z adds:
    plane = [0, 1, 8, 9, 2, 3, 10, 11, 16, 17, 24, 25, 18, 19, 26, 27]
    z_adds = [0, 4, 32, 36]
    x, y, z = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    s = np.stack([x.ravel(), y.ravel(), z.ravel(), np.full(64, 0.25)], axis=1).astype(np.float64)
    want = np.array([(plane[4 * int(b) + int(a)] + z_adds[int(c)]) << 24 for a, b, c in s[:, :3]], dtype=np.uint32)
    keys = rta.sphere_keys(s)
    assert keys.dtype == np.uint32
    np.testing.assert_array_equal(keys, want)
    at = lambda a, b, c: int(keys[16 * a + 4 * b + c])
    assert (at(0, 0, 0), at(1, 0, 0), at(0, 1, 0), at(0, 0, 1)) == (0, 0x01000000, 0x02000000, 0x04000000)
    assert (at(2, 0, 0), at(0, 0, 2), at(3, 3, 3), at(1, 2, 3)) == (0x08000000, 0x20000000, 0x3F000000, 0x35000000)
    assert len(set(keys.tolist())) == 64 and int(keys.max()) < 1 << 30
    # moved and scaled by powers of two the lattice has the same cells
    np.testing.assert_array_equal(rta.sphere_keys(s * [0.125, 0.125, 0.125, 1] + [-7.0, 3.0, 0.5, 0]), want)


def test_the_keys_ignore_the_radii_and_the_dtype():
    rng = np.random.default_rng(9)
    s32 = np.concatenate([rng.uniform(-3, 5, (500, 3)), rng.uniform(0.01, 0.5, (500, 1))], axis=1).astype(np.float32)
    keys = rta.sphere_keys(s32)
    assert len(set(keys.tolist())) > 400 and int(keys.max()) < 1 << 30
    other = s32.copy()
    other[:, 3] = rng.uniform(0.5, 50.0, 500).astype(np.float32)
    np.testing.assert_array_equal(rta.sphere_keys(other), keys)
    np.testing.assert_array_equal(rta.sphere_keys(s32.astype(np.float64)), keys)       # the same values in the other type
    for bad in (s32[:, :3], s32.astype(np.float16), s32[:0], [[0, 0, 0, 1]]):
        with pytest.raises(ValueError):
            rta.sphere_keys(bad)


# ---- argument errors of the host entries ----

def test_argument_errors_are_reported_before_any_device_is_touched():
    spheres = np.array([[0, 0, 0, 1], [2, 0, 0, 1], [0, 3, 0, 0.5]], dtype=np.float32)
    order = np.full(3, 77, dtype=np.uint32)
    # a zeroed block stands in for a scene: precision 0 is RT_F32, and no call below gets past its argument checks
    block = ctypes.create_string_buffer(1 << 20)
    stand_in = ctypes.cast(block, ctypes.c_void_p)
    so = capi.lib.rt_sphere_order
    assert so(None, spheres.ctypes.data, 3, order.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    assert so(stand_in, None, 3, order.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    assert so(stand_in, spheres.ctypes.data, 3, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert so(stand_in, spheres.ctypes.data, 0, order.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    for row, col, v in ((1, 0, np.nan), (2, 2, np.inf), (0, 1, -np.inf), (0, 1, 2e15), (1, 3, 0.0), (2, 3, -1.0), (0, 3, np.nan)):
        broken = spheres.copy()
        broken[row, col] = v
        assert so(stand_in, broken.ctypes.data, 3, order.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT, (row, col, v)
        assert b"rt_sphere_order" in capi.lib.rt_last_error_message()
    sod = capi.lib.rt_sphere_order_device
    assert sod(None, spheres.ctypes.data, 3, order.ctypes.data, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert sod(stand_in, None, 3, order.ctypes.data, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert sod(stand_in, spheres.ctypes.data, 3, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert sod(stand_in, spheres.ctypes.data, 0, order.ctypes.data, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert sod(stand_in, ctypes.c_void_p(spheres.ctypes.data + 4), 2, order.ctypes.data, None) == capi.RT_ERR_INVALID_ARGUMENT      # not a whole record's alignment
    assert capi.lib.rt_scene_rebuild(None, spheres.ctypes.data, order.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_rebuild(stand_in, None, order.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_rebuild_device(None, spheres.ctypes.data, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_rebuild_device(stand_in, None, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert (order == 77).all()


# ---- the kernels ----

def test_the_rebuild_kernels_keep_eight_waves_per_simd_and_use_no_scratch(tmp_path):
    from tests.test_kernel_resources import _kernels, LIB, TEST_LIB
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        mine = sorted(n for n in k if re.match(r"rt::k_(sphere_box|sphere_keys|gather_items)<", n))
        assert mine == sorted("rt::k_%s<%s>" % (name, t) for name in ("sphere_box", "sphere_keys", "gather_items") for t in ("float", "double")), mine
        for n in mine:
            assert k[n]["sgpr"] <= 80 and k[n]["vgpr"] <= 64 and k[n]["scratch"] == 0, (n, k[n])
