"""Sphere casts (rt_sweep_spheres / rt_sweep_spheres_device, csrc/rt_sweep.hpp) without a GPU: the ABI, the argument checks made before any
device is touched, the residency of the kernel's flavours read back from the code object, the checks DeviceScene.sweep makes before it
calls the library, and rta.sweep_distances -- the metric's definition in numpy -- against hand-computed cases and, with radius 0, against
the reference's ray-sphere distance."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from rust_tracer_amd.scene import DeviceScene
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_sweep_spheres", "rt_sweep_spheres_device")


def test_both_libraries_export_the_sweep_entries_at_abi_5():
    assert capi.ABI_VERSION == 5
    assert set(ENTRIES) <= set(capi.SYMBOLS)
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert lib.rt_abi_version() == 5
        for name in ENTRIES:
            assert getattr(lib, name) is not None
    assert (rta.RT_SWEEP_NEAREST, rta.RT_SWEEP_ANY) == (0, 1)
    assert (capi.RT_SWEEP_NEAREST, capi.RT_SWEEP_ANY) == (0, 1)
    header = open(os.path.join(ROOT, "include", "rtrace_hip.h")).read()
    assert "#define RTRACE_HIP_ABI_VERSION 5" in header
    assert re.search(r"RT_SWEEP_NEAREST = 0, RT_SWEEP_ANY = 1", header)
    declared = set(re.findall(r"\b(rt_[a-z_]+)\s*\(", header))
    assert set(ENTRIES) <= declared and declared == set(capi.SYMBOLS), declared ^ set(capi.SYMBOLS)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert getattr(capi.lib, name).argtypes, name
        assert re.search(r"\bfn %s\(" % name, integration), name


def _call(entry, scene, mode, rays, n, dist, radius=None, tmax=None, normal=None, item=None, exclude=None, order=None):
    f = getattr(capi.lib, entry)
    if entry == "rt_sweep_spheres":
        return f(scene, mode, rays, radius, tmax, n, exclude, order, dist, normal, item, None)
    return f(scene, mode, rays, radius, tmax, n, exclude, order, dist, normal, item, None, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check pointers, n, the mode and alignment before they use the scene's device: a stand-in handle will do (all zero bytes:
    # precision 0 is RT_F32)
    stand_in = ctypes.create_string_buffer(4096)
    rays = (ctypes.c_float * 6)(0, 0, 0, 0, 0, 1)
    dist = (ctypes.c_float * 4)()
    words = (ctypes.c_uint32 * 20)()
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    nearest = capi.RT_SWEEP_NEAREST
    bad = capi.RT_ERR_INVALID_ARGUMENT
    message = capi.lib.rt_last_error_message
    assert _call(entry, None, nearest, rays, 1, dist) == bad                     # NULL scene
    assert b"scene" in message()
    assert _call(entry, handle, nearest, None, 1, dist) == bad                   # NULL rays
    assert b"rays" in message()
    assert _call(entry, handle, nearest, rays, 1, None) == bad                   # NULL distance_out
    assert b"distance_out" in message()
    assert _call(entry, handle, nearest, rays, 0, dist) == bad                   # n == 0
    assert b"n == 0" in message()
    for mode in (2, -1, 7):
        assert _call(entry, handle, mode, rays, 1, dist) == bad                  # unknown mode
        assert b"mode" in message()
    misaligned = ctypes.c_void_p(ctypes.addressof(words) + 1)
    for arg, name in (("item", b"item_out"), ("exclude", b"exclude"), ("order", b"order"), ("radius", b"radius"), ("tmax", b"tmax"),
                      ("normal", b"normal_out")):
        assert _call(entry, handle, nearest, rays, 1, dist, **{arg: misaligned}) == bad
        assert name in message(), name
    assert _call(entry, handle, nearest, misaligned, 1, dist) == bad
    assert b"rays" in message()
    assert _call(entry, handle, nearest, rays, 1, misaligned) == bad
    assert b"distance_out" in message()


def test_the_host_entry_checks_its_domain_before_any_device_is_touched():
    # rays, radius, tmax and the order are read on the host before the scene's device is used
    stand_in = ctypes.create_string_buffer(4096)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    bad = capi.RT_ERR_INVALID_ARGUMENT
    message = capi.lib.rt_last_error_message
    F = ctypes.c_float
    good = (F * 12)(0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0)
    dist = (F * 2)()
    call = lambda rays, **kw: _call("rt_sweep_spheres", handle, capi.RT_SWEEP_NEAREST, rays, 2, dist, **kw)
    for q in (-1.0, float("nan"), float("inf"), 2e15):
        assert call(good, radius=(F * 2)(0.5, q)) == bad
        assert b"radius[1]" in message(), (q, message())
    assert call(good, tmax=(F * 2)(1.0, float("nan"))) == bad
    assert b"tmax[1]" in message()
    assert call((F * 12)(0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 0, 0)) == bad                                # no unit vector
    assert b"rays" in message() and b"ray 1" in message()
    assert call((F * 12)(0, 0, 0, 0, 0, 1, 1, 3e15, 1, 1, 0, 0)) == bad                             # beyond the domain
    assert b"rays" in message() and b"ray 1" in message()
    assert call((F * 12)(0, 0, 0, 0, 0, 1, 1, float("nan"), 1, 1, 0, 0)) == bad
    assert b"rays" in message()
    for order in ((0, 0), (0, 2)):
        assert call(good, order=(ctypes.c_uint32 * 2)(*order)) == bad                               # not a permutation
        assert b"order" in message()


def test_the_sweep_flavours_and_their_residency(tmp_path):
    # every flavour exists in both libraries inside k_query_rays's budget: no scratch, eight waves per SIMD
    want = sorted("rt::k_sweep_spheres<%s, %s, %s, %s>" % (t, c, a, o) for t in ("float", "double") for c in ("true", "false")
                  for a in ("true", "false") for o in ("true", "false"))
    assert len(want) == 16
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_sweep_spheres<")]
        assert sorted(flavours) == want, flavours
        for n in flavours:
            r = k[n]
            assert r["scratch"] == 0 and r["vgpr"] <= 64 and r["sgpr"] <= 80, (n, r)


class _Stand:
    """Enough of a Scene for DeviceScene's checks, which come before any call into the library."""
    def __init__(self, precision):
        self.precision = precision


def _device_scene(precision):
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h = _Stand(precision), 0, None
    return d


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_sweep_checks_shapes_and_dtypes_before_the_library(precision):
    R = np.float32 if precision == rta.RT_F32 else np.float64
    other = np.float64 if R == np.float32 else np.float32
    d = _device_scene(precision)
    good = np.array([[0, 0, -4, 0, 0, 1]] * 3, dtype=R)
    for rays in (good.astype(other), good[:, :3], good[:0], good.reshape(-1), good.tolist(), np.zeros((3, 4), R)):
        with pytest.raises(ValueError, match="rays"):
            d.sweep(rays)
    for radius in (np.ones(3, dtype=other), np.ones(2, dtype=R), np.ones((3, 2), dtype=R)):
        with pytest.raises(ValueError, match="radius"):
            d.sweep(good, radius=radius)
    for tmax in (np.ones(3, dtype=other), np.ones(2, dtype=R), np.ones((3, 2), dtype=R)):
        with pytest.raises(ValueError, match="tmax"):
            d.sweep(good, tmax=tmax)
    for exclude in (np.zeros(3, np.int64), np.zeros(3, np.uint32), np.zeros(2, np.int32), np.zeros((3, 1), np.int32), [0, 1, 2]):
        with pytest.raises(ValueError, match="exclude"):
            d.sweep(good, exclude=exclude)
    for order in (np.zeros(2, np.uint32), np.zeros(3, R), np.array([0, 1, -1])):
        with pytest.raises(ValueError, match="order"):
            d.sweep(good, order=order)
    n = 3
    ok = (np.empty(n, R), np.empty((n, 3), R), np.empty(n, np.int32))
    wrong = [
        ok[:2],                                                                        # item missing
        (np.empty(n + 1, R),) + ok[1:],                                                # distance for another n
        (np.empty(n, other),) + ok[1:],                                                # distance of the other REAL
        (ok[0], np.empty((n, 2), R), ok[2]),                                           # normal of another shape
        ok[:2] + (np.empty(n, np.int64),),                                             # item not int32
        (ok[0], np.empty((3, n), R).T, ok[2]),                                         # not contiguous
    ]
    for out in wrong:
        with pytest.raises(ValueError, match="out"):
            d.sweep(good, out=out)


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_sweep_distances_is_the_definition(R):
    inf = R(np.inf)
    sphere = np.array([[0, 0, 5, 1]], R)
    up = np.array([[0, 0, 0, 0, 0, 1]], R)
    # a sphere of radius 0.5 moving along +z touches the unit sphere at (0, 0, 5) when its centre is at z = 3.5: everything exact
    t = rta.sweep_distances(up, np.array([0.5], R), sphere)
    assert t.dtype == R and t.shape == (1, 1) and t[0, 0] == R(3.5)
    assert rta.sweep_distances(up, 0.5, sphere)[0, 0] == R(3.5)                         # one value for every cast
    # from (0, 0, 4) the moving sphere overlaps it at its start: 0, not the exit distance
    t = rta.sweep_distances(np.array([[0, 0, 4, 0, 0, 1]], R), np.array([0.5], R), sphere)
    assert t[0, 0] == 0 and not np.signbit(t[0, 0])
    # along -z the sphere lies behind
    assert rta.sweep_distances(np.array([[0, 0, 0, 0, 0, -1]], R), np.array([0.5], R), sphere)[0, 0] == inf
    # a lateral offset of 1.5 + 2^-10 passes by; 1.5 - 2^-10 does not
    off = R(1.5) + R(2.0 ** -10)
    assert rta.sweep_distances(np.array([[off, 0, 0, 0, 0, 1]], R), np.array([0.5], R), sphere)[0, 0] == inf
    near = R(1.5) - R(2.0 ** -10)
    assert np.isfinite(rta.sweep_distances(np.array([[near, 0, 0, 0, 0, 1]], R), np.array([0.5], R), sphere)[0, 0])
    # the guard: r = 0 (a dead slot, a dead group's bound) is at +inf for every cast, however large the moving sphere
    dead = np.array([[0, 0, 5, 0]], R)
    assert rta.sweep_distances(up, np.array([0.5], R), dead)[0, 0] == inf
    assert rta.sweep_distances(np.array([[0, 0, 5, 0, 0, 1]], R), np.array([100], R), dead)[0, 0] == inf
    # the operation order, each step rounded once
    ray = np.array([[0.1, -0.7, 0.3, 0.36, 0.48, 0.8]], R)
    s = np.array([[1.3, 0.2, 2.9, 0.6]], R)
    q = R(0.3)
    rr = R(s[0, 3] * s[0, 3])
    RR = R(R(rr + R(R(q + q) * np.sqrt(rr))) + R(q * q))
    v = s[0, :3] - ray[0, :3]
    dd = ray[0, 3:]
    b = R(R(R(v[0] * dd[0]) + R(v[1] * dd[1])) + R(v[2] * dd[2]))
    vv = R(R(R(v[0] * v[0]) + R(v[1] * v[1])) + R(v[2] * v[2]))
    disc = R(R(R(b * b) - vv) + RR)
    assert disc > 0 and rta.sweep_distances(ray, np.array([q], R), s)[0, 0] == R(b - np.sqrt(disc))
    # radius None is 0
    assert rta.sweep_distances(up, None, sphere)[0, 0] == R(4.0)
    with pytest.raises(ValueError):
        rta.sweep_distances(np.zeros((1, 6), np.float32), None, np.zeros((1, 4), np.float64))
    with pytest.raises(ValueError):
        rta.sweep_distances(np.zeros((1, 3), R), None, np.zeros((1, 4), R))
    with pytest.raises(ValueError):
        rta.sweep_distances(np.zeros((2, 6), R), np.zeros(3, R), np.zeros((1, 4), R))


@pytest.mark.parametrize("precision", [oracle.F32, oracle.F64], ids=["f32", "f64"])
def test_with_radius_0_from_outside_it_is_the_reference_ray_distance(precision):
    # q = 0 makes RR == rr bit for bit, and from an origin outside the sphere the near root is the one the reference reports
    R = np.float32 if precision == oracle.F32 else np.float64
    rng = np.random.default_rng(20)
    n, m = 200, 12
    spheres = np.concatenate([rng.uniform(-3, 3, (m, 3)), rng.uniform(0.05, 1.5, (m, 1))], axis=1).astype(R)
    pos = rng.normal(size=(n, 3))
    pos = (pos / np.linalg.norm(pos, axis=1, keepdims=True) * rng.uniform(8, 12, (n, 1)))           # outside every sphere
    aim = spheres[rng.integers(0, m, n), :3] + rng.normal(scale=0.4, size=(n, 3))
    d = aim - pos
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([pos, d], axis=1).astype(R)
    for q in (None, np.zeros(n, R)):
        t = rta.sweep_distances(rays, q, spheres)
        want = np.array([[oracle.sphere_intersect(spheres[j], rays[i], np.inf, precision)[0] for j in range(m)] for i in range(n)])
        hit = np.isfinite(want)
        assert hit.any() and (~hit).any()
        assert t.dtype == R and np.array_equal(np.isfinite(t), hit)
        assert np.array_equal(t[hit].astype(np.float64), want[hit])
