"""Proximity queries (rt_near_spheres / rt_near_spheres_device, csrc/rt_near.hpp) without a GPU: the ABI, the argument checks made before
any device is touched, the residency of the kernel's flavours read back from the code object, the checks DeviceScene.near makes before it
calls the library, and rta.sphere_gaps -- the metric's definition in numpy -- against hand-computed cases."""
import ctypes
import os
import re

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from rust_tracer_amd.scene import DeviceScene
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_near_spheres", "rt_near_spheres_device")
BUCKETS = (1, 4, 8, 16)


def test_both_libraries_export_the_near_entries_at_abi_5():
    assert capi.ABI_VERSION == 5
    assert set(ENTRIES) <= set(capi.SYMBOLS)
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert lib.rt_abi_version() == 5
        for name in ENTRIES:
            assert getattr(lib, name) is not None
    assert (rta.RT_NEAR_CLOSEST, rta.RT_NEAR_ALL, rta.RT_NEAR_MAX_K) == (0, 1, 16)
    assert (capi.RT_NEAR_CLOSEST, capi.RT_NEAR_ALL, capi.RT_NEAR_MAX_K) == (0, 1, 16)
    header = open(os.path.join(ROOT, "include", "rtrace_hip.h")).read()
    assert "#define RTRACE_HIP_ABI_VERSION 5" in header
    assert re.search(r"RT_NEAR_CLOSEST = 0, RT_NEAR_ALL = 1", header) and re.search(r"#define\s+RT_NEAR_MAX_K\s+16\b", header)
    declared = set(re.findall(r"\b(rt_[a-z_]+)\s*\(", header))
    assert set(ENTRIES) <= declared and declared == set(capi.SYMBOLS), declared ^ set(capi.SYMBOLS)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert getattr(capi.lib, name).argtypes, name
        assert re.search(r"\bfn %s\(" % name, integration), name


def _call(entry, scene, mode, k, points, n, gap, item=None, found=None, exclude=None, order=None):
    f = getattr(capi.lib, entry)
    if entry == "rt_near_spheres":
        return f(scene, mode, k, points, None, n, exclude, order, gap, item, found, None)
    return f(scene, mode, k, points, None, n, exclude, order, gap, item, found, None, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check pointers, n, k, the mode and alignment before they use the scene: a stand-in handle will do
    stand_in = ctypes.create_string_buffer(4096)
    points = (ctypes.c_float * 3)(0, 0, 0)
    gap = (ctypes.c_float * 16)()
    words = (ctypes.c_uint32 * 20)()
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    closest = capi.RT_NEAR_CLOSEST
    bad = capi.RT_ERR_INVALID_ARGUMENT
    assert _call(entry, None, closest, 4, points, 1, gap) == bad                 # NULL scene
    assert _call(entry, handle, closest, 4, None, 1, gap) == bad                 # NULL points
    assert _call(entry, handle, closest, 4, points, 1, None) == bad              # NULL gap_out
    assert _call(entry, handle, closest, 4, points, 0, gap) == bad               # n == 0
    for k in (0, 17, 1 << 20):
        assert _call(entry, handle, closest, k, points, 1, gap) == bad           # k outside 1 .. RT_NEAR_MAX_K
        assert b"k must be" in capi.lib.rt_last_error_message()
    for mode in (2, -1, 7):
        assert _call(entry, handle, mode, 4, points, 1, gap) == bad              # unknown mode
        assert b"mode" in capi.lib.rt_last_error_message()
    misaligned = ctypes.c_void_p(ctypes.addressof(words) + 1)
    for arg, name in (("item", b"item_out"), ("found", b"found_out"), ("exclude", b"exclude"), ("order", b"order")):
        assert _call(entry, handle, closest, 4, points, 1, gap, **{arg: misaligned}) == bad
        assert name in capi.lib.rt_last_error_message(), name


def test_the_near_flavours_and_their_residency(tmp_path):
    # every flavour exists in both libraries without scratch; capacities up to 4 keep eight waves per SIMD, larger ones four or more
    want = sorted("rt::k_near_spheres<%s, %s, %s, %s, %d>" % (t, c, a, o, b) for t in ("float", "double") for c in ("true", "false")
                  for a in ("true", "false") for o in ("true", "false") for b in BUCKETS)
    assert len(want) == 64
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_near_spheres<")]
        assert sorted(flavours) == want, flavours
        for n in flavours:
            b = int(n.rstrip(">").split(",")[-1])
            r = k[n]
            assert r["scratch"] == 0, (n, r)
            if b <= 4:
                assert r["sgpr"] <= 80 and r["vgpr"] <= 64, (n, r)
            else:
                assert r["vgpr"] <= 128, (n, r)


class _Stand:
    """Enough of a Scene for DeviceScene's checks, which come before any call into the library."""
    def __init__(self, precision):
        self.precision = precision


def _device_scene(precision):
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h = _Stand(precision), 0, None
    return d


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_near_checks_shapes_and_dtypes_before_the_library(precision):
    R = np.float32 if precision == rta.RT_F32 else np.float64
    other = np.float64 if R == np.float32 else np.float32
    d = _device_scene(precision)
    good = np.array([[0, 0, -4]] * 3, dtype=R)
    for k in (0, 17, -1):
        with pytest.raises(ValueError, match="k must be"):
            d.near(good, k)
    for points in (good.astype(other), good[:, :2], good[:0], good.reshape(-1), good.tolist(), np.zeros((3, 6), R)):
        with pytest.raises(ValueError, match="points"):
            d.near(points, 4)
    for radius in (np.ones(3, dtype=other), np.ones(2, dtype=R), np.ones((3, 2), dtype=R)):
        with pytest.raises(ValueError, match="radius"):
            d.near(good, 4, radius=radius)
    for exclude in (np.zeros(3, np.int64), np.zeros(3, np.uint32), np.zeros(2, np.int32), np.zeros((3, 1), np.int32), [0, 1, 2]):
        with pytest.raises(ValueError, match="exclude"):
            d.near(good, 4, exclude=exclude)
    for order in (np.zeros(2, np.uint32), np.zeros(3, R), np.array([0, 1, -1])):
        with pytest.raises(ValueError, match="order"):
            d.near(good, 4, order=order)
    n, k = 3, 4
    ok = (np.empty((n, k), R), np.empty((n, k), np.int32), np.empty(n, np.uint32))
    wrong = [
        ok[:2],                                                                        # found missing
        (np.empty((n, k + 1), R),) + ok[1:],                                           # gap for another k
        (np.empty((n, k), other),) + ok[1:],                                           # gap of the other REAL
        (ok[0], np.empty((n, k), np.int64), ok[2]),                                    # item not int32
        ok[:2] + (np.empty(n, np.int32),),                                             # found not uint32
        (np.empty((k, n), R).T,) + ok[1:],                                             # not contiguous
    ]
    for out in wrong:
        with pytest.raises(ValueError, match="out"):
            d.near(good, k, out=out)


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_sphere_gaps_is_the_definition(R):
    inf = R(np.inf)
    # a point at a centre: vv = 0, gap = -sqrt(rr); with r = 2 the square and its root are exact
    g = rta.sphere_gaps(np.array([[1, 2, 3]], R), np.array([[1, 2, 3, 2]], R))
    assert g.dtype == R and g.shape == (1, 1) and g[0, 0] == R(-2.0)
    # a point on a surface, everything exact: centre (0, 0, 0), r = 5, p = (3, 4, 0) -> sqrt(25) - sqrt(25) = 0; and one unit further out
    g = rta.sphere_gaps(np.array([[3, 4, 0], [0, -6, 0]], R), np.array([[0, 0, 0, 5]], R))
    assert g[0, 0] == 0 and not np.signbit(g[0, 0]) and g[1, 0] == R(1.0)
    # the dot order: (v.x*v.x + v.y*v.y) + v.z*v.z with v = c - p, each step rounded once
    p, s = np.array([[0.1, -0.7, 0.3]], R), np.array([[1.3, 0.2, -2.9, 0.6]], R)
    v = s[0, :3] - p[0]
    vv = R(R(R(v[0] * v[0]) + R(v[1] * v[1])) + R(v[2] * v[2]))
    assert rta.sphere_gaps(p, s)[0, 0] == R(np.sqrt(vv) - np.sqrt(R(s[0, 3] * s[0, 3])))
    # the guard: rr <= 0 (radius 0: a dead slot, a dead group's bound {0, 0, 0, 0}) is at +inf from every point, its own centre included
    g = rta.sphere_gaps(np.array([[0, 0, 0], [1, 1, 1]], R), np.array([[0, 0, 0, 0], [0, 0, 0, 1]], R))
    assert g[0, 0] == inf and g[1, 0] == inf and g[0, 1] == R(-1.0)
    with pytest.raises(ValueError):
        rta.sphere_gaps(np.zeros((1, 3), np.float32), np.zeros((1, 4), np.float64))
    with pytest.raises(ValueError):
        rta.sphere_gaps(np.zeros((1, 4), R), np.zeros((1, 4), R))


def test_sphere_gaps_takes_the_root_of_the_rounded_square():
    # The stream holds rr = RN(r * r) and the gap subtracts sqrt_rn(rr).  In binary floating point that root is r again unless the square
    # leaves the normal range; it does for a tiny f32 radius: 3e-23 squared is 9e-46, between the denormals 0 and 2^-149 ~ 1.4e-45.
    R = np.float32
    r = R(3e-23)
    rr = R(r * r)
    assert rr == np.ldexp(R(1.0), -149)
    root = np.sqrt(rr)
    assert root != r and root == np.ldexp(R(1.0), -75) * np.sqrt(R(2.0))
    # at the centre the gap is -sqrt_rn(RN(r*r)), not -r
    g = rta.sphere_gaps(np.zeros((1, 3), R), np.array([[0, 0, 0, r]], R))
    assert g[0, 0] == -root and g[0, 0] != -r
    # on the surface along an axis vv rounds as rr does: the gap is exactly 0, though neither root is r
    g = rta.sphere_gaps(np.array([[r, 0, 0]], R), np.array([[0, 0, 0, r]], R))
    assert g[0, 0] == 0
    # a radius whose square rounds to 0 has no positive rr: the guard, +inf
    g = rta.sphere_gaps(np.zeros((1, 3), R), np.array([[0, 0, 0, 1e-23]], R))
    assert R(R(1e-23) * R(1e-23)) == 0 and g[0, 0] == np.inf
    # ... and for an ordinary radius the root of the rounded square is the radius (0.1f, 0.3f, ...): gap at the centre = -r
    for r in (R(0.1), R(0.3), R(1.7)):
        assert np.sqrt(R(r * r)) == r and rta.sphere_gaps(np.zeros((1, 3), R), np.array([[0, 0, 0, r]], R))[0, 0] == -r
