"""Overlap lists (rt_overlap_spheres / rt_overlap_spheres_device, csrc/rt_overlap.hpp) without a GPU: the ABI, the argument
checks made before any device is touched, the residency of the kernel's flavours read back from the code object, rta.overlap_gaps -- the
metric's definition in numpy -- against a scalar restatement, and the checks the Python wrapper makes before it calls the library."""
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
ENTRIES = ("rt_overlap_spheres", "rt_overlap_spheres_device")
BAD = capi.RT_ERR_INVALID_ARGUMENT


def test_both_libraries_export_the_overlap_entries_at_abi_5():
    assert capi.ABI_VERSION == 5
    assert set(ENTRIES) <= set(capi.SYMBOLS)
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert lib.rt_abi_version() == 5
        for name in ENTRIES:
            assert getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "rtrace_hip.h")).read()
    assert "#define RTRACE_HIP_ABI_VERSION 5" in header
    declared = set(re.findall(r"\b(rt_[a-z_]+)\s*\(", header))
    assert set(ENTRIES) <= declared and declared == set(capi.SYMBOLS), declared ^ set(capi.SYMBOLS)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert getattr(capi.lib, name).argtypes, name
        assert re.search(r"\bfn %s\(" % name, integration), name
    assert callable(rta.overlap_gaps) and "overlap_gaps" in rta.__all__ and callable(DeviceScene.overlaps)


def _call(entry, scene, queries, n, margin, exclude, order, capacity, items, gap, offsets, total):
    f = getattr(capi.lib, entry)
    args = (scene, queries, n, margin, exclude, order, capacity, items, gap, offsets, total, None)
    return f(*args) if entry == "rt_overlap_spheres" else f(*args, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check pointers, n, the margin, the capacity and alignment before they use the scene: a stand-in handle will do
    stand_in = ctypes.create_string_buffer(8192)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    words = (ctypes.c_uint64 * 128)()
    at = lambda k: ctypes.c_void_p(ctypes.addressof(words) + k)
    queries, exclude, order, items, gap, offsets, total = at(0), at(128), at(256), at(384), at(512), at(640), at(768)
    message = capi.lib.rt_last_error_message
    good = dict(scene=handle, queries=queries, n=4, margin=0.0, exclude=exclude, order=order, capacity=4, items=items, gap=gap, offsets=offsets, total=total)
    call = lambda **kw: _call(entry, **{**good, **kw})
    assert call(scene=None) == BAD
    assert call(queries=None) == BAD
    assert b"queries" in message()
    assert call(total=None) == BAD
    assert b"total_out" in message()
    assert call(n=0) == BAD
    assert b"n == 0" in message()
    assert call(margin=float("nan")) == BAD
    assert b"NaN" in message()
    assert call(items=None) == BAD                                               # gap_out without items_out
    assert b"gap_out without items_out" in message()
    for capacity in (1 << 31, 0xFFFFFFFF):
        assert call(capacity=capacity) == BAD
        assert b"capacity" in message()
    for k in (1, 2, 3):
        for name, base in (("items", 384), ("exclude", 128), ("order", 256), ("queries", 0), ("gap", 512)):
            assert call(**{name: at(base + k)}) == BAD
            assert (name.encode() if name in ("exclude", "order", "queries") else name.encode() + b"_out") in message(), name
    for k in (1, 4, 7):
        assert call(offsets=at(640 + k)) == BAD
        assert b"offsets_out" in message()
        assert call(total=at(768 + k)) == BAD
        assert b"total_out" in message()


def test_the_host_entry_checks_its_domain_before_any_device_is_touched():
    # the queries and the order are read on the host before the scene's device is used (a stand-in handle of zero bytes: precision 0 is RT_F32)
    stand_in = ctypes.create_string_buffer(8192)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    total = ctypes.c_uint64(0)
    good = np.array([[0, 0, 0, 0.5], [1, 0, 0, 0.0], [0, 2, 0, 1.0]], np.float32)
    message = capi.lib.rt_last_error_message

    def call(q, order=None):
        o = None if order is None else np.asarray(order, np.uint32)
        return capi.lib.rt_overlap_spheres(handle, q.ctypes.data, len(q), 0.0, None, None if o is None else o.ctypes.data, 0, None, None, None,
                                           ctypes.byref(total), None)
    for row, col, value in ((0, 0, np.nan), (1, 1, np.inf), (2, 2, -np.inf), (0, 1, 2e15), (1, 2, -2e15)):
        q = good.copy()
        q[row, col] = value
        assert call(q) == BAD, (row, col, value)
        assert b"coordinate" in message() and b"query %d" % row in message()
    for value in (np.nan, -1.0, -1e-30, np.inf, 2e15):
        q = good.copy()
        q[1, 3] = value
        assert call(q) == BAD, value
        assert b"radius" in message() and b"query 1" in message()
    for order in ([0, 1, 1], [0, 1, 3], [2, 2, 2]):
        assert call(good, order) == BAD, order
        assert b"permutation" in message()


def test_the_overlap_flavours_and_their_residency(tmp_path):
    # every flavour exists in both libraries, without scratch and within k_contact_pairs's budget: eight waves per SIMD
    want = sorted("rt::k_overlap_spheres<%s, %s>" % (t, f) for t in ("float", "double") for f in ("true, false", "false, false", "false, true"))
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_overlap_spheres<")]
        assert sorted(flavours) == want, flavours
        for n in flavours:
            r = k[n]
            assert r["scratch"] == 0 and r["sgpr"] <= 80 and r["vgpr"] <= 64, (n, r)


def scalar_overlap_gap(R, q, s):
    """The definition, one operation at a time on numpy scalars of type R (each rounds once)."""
    rr = R(s[3] * s[3])
    if not rr > 0:
        return R(np.inf)
    vx, vy, vz = R(s[0] - q[0]), R(s[1] - q[1]), R(s[2] - q[2])
    vv = R(R(R(vx * vx) + R(vy * vy)) + R(vz * vz))
    return R(R(np.sqrt(vv) - np.sqrt(rr)) - q[3])


def _inputs(R):
    """pair_gaps' inputs of test_contacts_host.py, and as many query spheres."""
    rng = np.random.default_rng(7)
    s = np.concatenate([rng.uniform(-1, 1, (40, 3)), rng.uniform(0.01, 0.4, (40, 1))], axis=1).astype(R)
    s[5, 3] = 0                                                                  # a dead slot as the tests hold it: {.., 0}
    s[9] = 0
    s[11, 3] = R(1e-30) if R == np.float32 else R(1e-200)                        # rr rounds to 0: no positive rr
    q = np.concatenate([rng.uniform(-1.2, 1.2, (40, 3)), rng.uniform(0.0, 0.3, (40, 1))], axis=1).astype(R)
    q[::10, 3] = 0
    return q, s


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_overlap_gaps_is_the_definition(R):
    U = np.uint32 if R == np.float32 else np.uint64
    inf = R(np.inf)
    # everything exact: centres 5 apart (3-4-5), radii 2 and 1.5 -> (5 - 1.5) - 2 = 1.5; touching spheres -> 0; one inside the other
    s = np.array([[3, 4, 0, 1.5], [0, 0, 3, 1], [0, 0, 0.5, 0.25]], R)
    g = rta.overlap_gaps(np.array([[0, 0, 0, 2]], R), s)
    assert g.dtype == R and g.shape == (1, 3) and g[0].tolist() == [1.5, 0.0, -1.75]
    q, s = _inputs(R)
    assert R(s[11, 3] * s[11, 3]) == 0
    got = rta.overlap_gaps(q, s)
    ref = np.array([[scalar_overlap_gap(R, a, b) for b in s] for a in q], R)
    np.testing.assert_array_equal(got.view(U), ref.view(U))
    # a dead record is at +inf from every query, everything else is finite
    assert (got[:, [5, 9, 11]] == inf).all()
    assert np.isfinite(np.delete(got, [5, 9, 11], axis=1)).all()
    # against a restatement in extended precision: |gap - (|c - p| - r - q)| <= 8 u (|c - p| + r + q), DESIGN.md 4.16's bound
    L = np.longdouble
    u = L(np.finfo(R).eps) / 2
    live = np.delete(np.arange(40), [5, 9, 11])
    c, p = s[live, :3].astype(L), q[:, :3].astype(L)
    dist = np.sqrt(((c[None] - p[:, None]) ** 2).sum(axis=2))
    r, qq = s[live, 3].astype(L)[None], q[:, 3].astype(L)[:, None]
    assert (np.abs(got[:, live].astype(L) - (dist - r - qq)) <= 8 * u * (dist + r + qq)).all()
    # q = 0: the proximity queries' gap, bit for bit
    zero = q.copy()
    zero[:, 3] = 0
    np.testing.assert_array_equal(rta.overlap_gaps(zero, s).view(U), rta.sphere_gaps(np.ascontiguousarray(q[:, :3]), s).view(U))
    # a scene's own spheres as the queries, q = sqrt(r * r) in REAL: the contact pairs' gap, bit for bit, with either slot as the query
    own = s.copy()
    own[:, 3] = np.sqrt(s[:, 3] * s[:, 3])
    full = rta.overlap_gaps(own, s)
    i, j = np.triu_indices(40, 1)
    for a, b in ((i, j), (j, i)):
        solid = (s[a, 3] * s[a, 3]) > 0                                          # (pair_gaps puts a dead FIRST sphere at +inf too)
        np.testing.assert_array_equal(full[a, b][solid].view(U), rta.pair_gaps(s, a, b)[solid].view(U))
    # a tiny f32 radius in the scene: the root of the rounded square, not the radius
    if R == np.float32:
        r = R(3e-23)
        root = np.sqrt(R(r * r))
        assert root != r
        g = rta.overlap_gaps(np.array([[0, 0, 0, r]], R), np.array([[0, 0, 0, r]], R))
        assert g[0, 0] == R(R(0.0) - root) - r
    assert rta.overlap_gaps(np.zeros((0, 4), R), s).shape == (0, 40) and rta.overlap_gaps(q, np.zeros((0, 4), R)).shape == (40, 0)


def test_overlap_gaps_checks_its_arguments():
    s = np.zeros((4, 4), np.float32)
    for bad in (s.astype(np.float16), s[:, :3], s.reshape(-1), s.astype(np.int32), s.astype(np.float64)):
        with pytest.raises(ValueError, match="queries"):
            rta.overlap_gaps(bad, s)
        with pytest.raises(ValueError, match="queries"):
            rta.overlap_gaps(s, bad)


class _Stand:
    """Enough of a Scene for DeviceScene's checks, which come before any call into the library."""
    def __init__(self, precision):
        self.precision = precision
        self.items = np.zeros((3, 4), np.float32 if precision == rta.RT_F32 else np.float64)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_overlaps_checks_its_arguments_before_the_library(precision):
    R = np.float32 if precision == rta.RT_F32 else np.float64
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h = _Stand(precision), 0, None
    q = np.zeros((5, 4), R)
    with pytest.raises(ValueError, match="margin"):
        d.overlaps(q, float("nan"))
    with pytest.raises((TypeError, ValueError)):
        d.overlaps(q, "near")
    for capacity in (-1, 1 << 31, 1 << 40):
        with pytest.raises(ValueError, match="capacity"):
            d.overlaps(q, 0.0, capacity=capacity)
    with pytest.raises((TypeError, ValueError)):
        d.overlaps(q, 0.0, capacity="all")
    other = np.float64 if R == np.float32 else np.float32
    for bad in (q.astype(other), q[:, :3], q.reshape(-1), q[:0], q.tolist(), None):
        with pytest.raises(ValueError, match="queries"):
            d.overlaps(bad)
    for bad in (np.zeros(5, np.int64), np.zeros(4, np.int32), np.zeros((5, 1), np.int32)):
        with pytest.raises(ValueError, match="exclude"):
            d.overlaps(q, exclude=bad)
    for bad in (np.zeros(5, R), np.zeros(4, np.uint32), np.array([0, 1, 2, 3, -1])):
        with pytest.raises(ValueError, match="order"):
            d.overlaps(q, order=bad)
