"""Dynamic scenes (rt_scene_create_dynamic / rt_scene_update* / rt_scene_bounds, csrc/rt_dynamic.hpp) without a GPU: the refit rule's
restatement encloses every item in exact arithmetic and does not depend on the items' order, the ABI, the argument checks made before any
device is touched, and the residency of the new kernels read back from the code object."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.scenes import random_nested_scene
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = {rta.RT_F32: np.float32, rta.RT_F64: np.float64}
ENTRIES = ("rt_scene_create_dynamic", "rt_scene_update", "rt_scene_update_device", "rt_scene_bounds")
PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])


# ---- exact arithmetic: every float is an integer over a power of two; with one shift for all of them the integers compare exactly ----

def exact_ints(*arrays):
    """The arrays' values as Python integers over ONE common power of two (object arrays of the same shapes)."""
    fr = [[Fraction(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()] for a in arrays]
    den = max(f.denominator for row in fr for f in row)              # every denominator is a power of two: the largest is a common one
    return [np.array([f.numerator * (den // f.denominator) for f in row], dtype=object).reshape(np.shape(a)) for row, a in zip(fr, arrays)]


def assert_encloses(items, ranges, bounds, what):
    """|c_i - centre| + r_i <= radius for every item of every group, exactly: radius - r_i >= 0 and |c_i - centre|^2 <= (radius - r_i)^2."""
    it, bd = exact_ints(items, bounds)
    checked = 0
    for g, (first, count) in enumerate(np.asarray(ranges).reshape(-1, 2)):
        if count == 0:
            continue
        sl = slice(int(first), int(first + count))
        d = it[sl, :3] - bd[g, :3]
        room = bd[g, 3] - it[sl, 3]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        bad = [int(first) + k for k in range(int(count)) if room[k] < 0 or d2[k] > room[k] * room[k]]
        assert not bad, "%s: group %d does not enclose its items %r" % (what, g, bad[:5])
        checked += int(count)
    return checked


def with_loose_items(items, ranges, front, back, rng):
    """The scene with `front` items in front of and `back` items behind every group: items no bound covers."""
    lo, hi = items[:, :3].min(axis=0), items[:, :3].max(axis=0)
    extra = lambda n: np.concatenate([rng.uniform(lo, hi, (n, 3)), rng.uniform(0.05, 0.3, (n, 1))], axis=1)
    rg = np.array(ranges, dtype=np.int32).reshape(-1, 2).copy()
    rg[:, 0] += front
    return np.concatenate([extra(front), items, extra(back)]), rg


def scaled_spheres(rng, n, scale):
    """n spheres whose centres and radii are of the order of `scale` (radius below it: 1e15 is the largest value a scene takes)."""
    return np.concatenate([rng.uniform(-scale, scale, (n, 3)), rng.uniform(0.01 * scale, 0.9 * scale, (n, 1))], axis=1)


def refit_inputs(precision):
    """(name, items, ranges): what the refit must enclose."""
    R = REAL[precision]
    rng = np.random.default_rng(77 + precision)
    out = []
    it, _, rg = rta.pyramid(8, (0.0, -1.0, 0.0), 1.0, precision)
    out.append(("pyramid", it, rg))
    it, _, rg = random_nested_scene(11, depth=3, fan=3, leaf_items=3)
    it, rg = with_loose_items(it, rg, 3, 2, rng)
    assert rg[0, 0] == 3 and rg[0, 0] + rg[0, 1] == len(it) - 2 and (rg[1:, 1] < rg[0, 1]).all()      # loose items at both ends, nested groups
    out.append(("nested", it, rg))
    nest = np.array([[0, 40], [0, 13], [3, 5], [13, 27], [20, 1], [39, 1]], dtype=np.int32)
    for name, scale in (("1e15", 1e15), ("1e-30", 1e-30), ("1e-42", 1e-42)):
        if scale < 1e-37 and precision == rta.RT_F64:
            scale = 1e-300
        out.append((name, scaled_spheres(rng, 40, scale), nest))
    mixed = np.concatenate([scaled_spheres(rng, 20, 1e15), scaled_spheres(rng, 20, 1e-30)])
    out.append(("1e15 with 1e-30", mixed[rng.permutation(40)], nest))
    out.append(("one sphere", np.array([[0.3, -0.7, 2.5, 0.125]]), np.array([[0, 1]], dtype=np.int32)))
    same = np.tile(np.array([[1.5, -2.25, 3.0, 0.0]]), (9, 1))
    same[:, 3] = rng.uniform(0.1, 2.0, 9)
    out.append(("coincident centres", same, np.array([[0, 9], [2, 4]], dtype=np.int32)))
    # every radius > 0 and every value finite in REAL, as a scene takes them
    for name, it, rg in out:
        itr = np.asarray(it, dtype=R)
        assert np.isfinite(itr).all() and (itr[:, 3] > 0).all() and (np.abs(itr) <= 1e15).all(), name
    return [(name, np.asarray(it, dtype=R), rg) for name, it, rg in out]


@PRECISIONS
def test_refit_bounds_enclose_every_item_of_every_group_exactly(precision):
    R = REAL[precision]
    for name, it, rg in refit_inputs(precision):
        bd = rta.refit_bounds(it, rg, precision)
        assert bd.dtype == R and bd.shape == (len(rg), 4) and np.isfinite(bd).all() and (bd[:, 3] > 0).all(), name
        assert assert_encloses(it, rg, bd, name) == int(np.asarray(rg)[:, 1].sum())
        # ... and tightly: the radius is no more than 1 + 16 EPSILON times the largest reach, formed in twice the precision or exactly
        if name in ("pyramid", "nested"):
            wide = np.float64 if precision == rta.RT_F32 else np.longdouble
            for g, (first, count) in enumerate(rg):
                c, r = it[first:first + count, :3].astype(wide), it[first:first + count, 3].astype(wide)
                reach = (np.sqrt(((c - bd[g, :3].astype(wide)) ** 2).sum(axis=1)) + r).max()
                assert bd[g, 3] <= reach * (1 + 16 * np.finfo(R).eps), (name, g)


@PRECISIONS
def test_refit_bounds_do_not_depend_on_the_order_of_a_groups_items(precision):
    R = REAL[precision]
    rng = np.random.default_rng(5)
    as_bits = lambda a: np.ascontiguousarray(a).view(np.uint32 if R == np.float32 else np.uint64)
    for name, it, rg in refit_inputs(precision):
        if name == "pyramid":
            it, _, rg = rta.pyramid(5, (0.0, -1.0, 0.0), 1.0, precision)
        # the leaves of the laminar family: ranges that hold no other range; permuting inside one keeps every group's item SET
        rg = np.asarray(rg).reshape(-1, 2)
        shuffled = it.copy()
        for first, count in rg:
            inner = [(f, c) for f, c in rg if (f, c) != (first, count) and f >= first and f + c <= first + count]
            if not inner and count > 1:
                shuffled[first:first + count] = it[first:first + count][rng.permutation(count)]
        if len(rg) == 1:
            shuffled = it[::-1].copy()
        np.testing.assert_array_equal(as_bits(rta.refit_bounds(shuffled, rg, precision)), as_bits(rta.refit_bounds(it, rg, precision)), err_msg=name)


def test_a_group_without_items_keeps_the_bound_it_was_given():
    it = np.array([[0, 0, 0, 1], [3, 0, 0, 1]], dtype=np.float32)
    rg = np.array([[0, 2], [1, 0]], dtype=np.int32)
    given = np.array([[9, 9, 9, 9], [1, 2, 3, 4]], dtype=np.float32)
    bd = rta.refit_bounds(it, rg, rta.RT_F32, bounds=given)
    assert list(bd[1]) == [1, 2, 3, 4] and list(bd[0, :3]) == [1.5, 0, 0] and bd[0, 3] == np.float32(2.5) * (np.float32(1) + np.float32(8) * np.finfo(np.float32).eps)
    assert list(rta.refit_bounds(it, rg)[1]) == [0, 0, 0, 0]


# ---- the ABI ----

def test_the_new_symbols_are_declared_bound_and_exported_by_both_libraries():
    assert capi.ABI_VERSION == 5 and set(ENTRIES) <= set(capi.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "rtrace_hip.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z_]+)\s*\(", header))
    assert set(ENTRIES) <= declared
    assert "RT_SCENE_DYNAMIC = 4u" in header and capi.RT_SCENE_DYNAMIC == 4
    assert "rt_*" in open(os.path.join(ROOT, "rust-tracer_amd", "csrc", "exports.map")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert re.search(r"\bfn %s\(" % name, integration), name
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        exported = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines() if l.strip()}
        assert set(ENTRIES) <= exported, path
        assert ctypes.CDLL(path).rt_abi_version() == 5


def test_argument_errors_are_reported_before_any_device_is_touched():
    f = np.float32
    items = np.array([[0, 0, 0, 1], [2, 0, 0, 1]], dtype=f)
    light, eye = rta.normalized((-1.0, -3.0, 2.0)), np.array([0, 0, -4], dtype=f)
    ranges = np.array([[0, 2], [1, 0]], dtype=np.int32)
    bounds = np.array([[1, 0, 0, 2], [2, 0, 0, 1]], dtype=f)
    h = ctypes.c_void_p()

    def create(it, bd, rg, nb):
        return capi.lib.rt_scene_create_dynamic(0, rta.RT_F32, it.ctypes.data, len(it), light.ctypes.data, eye.ctypes.data, None if bd is None else bd.ctypes.data,
                                                None if rg is None else rg.ctypes.data, nb, ctypes.byref(h))
    # the refit form has nothing to refit an empty group's bound from
    assert create(items, None, ranges, 2) == capi.RT_ERR_INVALID_ARGUMENT and b"range 1" in capi.lib.rt_last_error_message()
    assert create(items, bounds, None, 2) == capi.RT_ERR_INVALID_ARGUMENT
    assert create(items, bounds, np.array([[0, 3]], dtype=np.int32), 1) == capi.RT_ERR_INVALID_ARGUMENT
    for bad in (np.nan, 0.0, -1.0):
        broken = items.copy()
        broken[1, 3] = bad
        assert create(broken, bounds, ranges, 2) == capi.RT_ERR_INVALID_ARGUMENT
    far = items.copy()
    far[0, 1] = 2e15
    assert create(far, None, ranges[:1], 1) == capi.RT_ERR_INVALID_ARGUMENT
    assert h.value is None
    # NULL scene / items / output: the handle is never read
    stand_in = ctypes.cast(ctypes.create_string_buffer(8192), ctypes.c_void_p)
    assert capi.lib.rt_scene_update(None, items.ctypes.data, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_update(stand_in, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_update_device(None, items.ctypes.data, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_update_device(stand_in, None, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_bounds(None, bounds.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT


# ---- the kernels ----

def test_the_update_kernels_keep_eight_waves_per_simd_and_use_no_scratch(tmp_path):
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        mine = sorted(n for n in k if re.match(r"rt::k_(refit_box|refit_reach|dynamic_rewrite|dynamic_topology)<", n))
        assert mine == sorted("rt::k_%s<%s>" % (name, t) for name in ("refit_box", "refit_reach", "dynamic_rewrite", "dynamic_topology")
                              for t in ("float", "double")), mine
        for n in mine:
            assert k[n]["sgpr"] <= 80 and k[n]["vgpr"] <= 64 and k[n]["scratch"] == 0, (n, k[n])
