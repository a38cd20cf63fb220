"""Contact pairs (rt_scene_contacts / rt_scene_contacts_device, csrc/rt_contacts.hpp) without a GPU: the ABI, the argument
checks made before any device is touched, the residency of the kernel's flavours read back from the code object, rta.pair_gaps -- the
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
ENTRIES = ("rt_scene_contacts", "rt_scene_contacts_device")


def test_both_libraries_export_the_contacts_entries_at_abi_5():
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
    assert callable(rta.pair_gaps) and "pair_gaps" in rta.__all__ and callable(DeviceScene.contacts)


def _call(entry, scene, margin, capacity, pairs, gap, offsets, total):
    f = getattr(capi.lib, entry)
    if entry == "rt_scene_contacts":
        return f(scene, margin, capacity, pairs, gap, offsets, total, None)
    return f(scene, margin, capacity, pairs, gap, offsets, total, None, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check pointers, the margin, the capacity and alignment before they use the scene: a stand-in handle will do
    stand_in = ctypes.create_string_buffer(8192)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    words = (ctypes.c_uint64 * 64)()
    at = lambda k: ctypes.c_void_p(ctypes.addressof(words) + k)
    pairs, gap, offsets, total = at(0), at(128), at(256), at(384)
    bad = capi.RT_ERR_INVALID_ARGUMENT
    message = capi.lib.rt_last_error_message
    assert _call(entry, None, 0.0, 4, pairs, gap, offsets, total) == bad         # NULL scene
    assert _call(entry, handle, 0.0, 4, pairs, gap, offsets, None) == bad        # NULL total_out
    assert b"total_out" in message()
    assert _call(entry, handle, float("nan"), 4, pairs, gap, offsets, total) == bad
    assert b"NaN" in message()
    assert _call(entry, handle, 0.0, 4, None, gap, offsets, total) == bad        # gap_out without pairs_out
    assert b"gap_out without pairs_out" in message()
    for capacity in (1 << 31, 0xFFFFFFFF):
        assert _call(entry, handle, 0.0, capacity, pairs, gap, offsets, total) == bad
        assert b"capacity" in message()
    for k in (1, 2, 3):
        assert _call(entry, handle, 0.0, 4, at(k), gap, offsets, total) == bad
        assert b"pairs_out" in message()
        assert _call(entry, handle, 0.0, 4, pairs, at(128 + k), offsets, total) == bad
        assert b"gap_out" in message()
    for k in (1, 4, 7):
        assert _call(entry, handle, 0.0, 4, pairs, gap, at(256 + k), total) == bad
        assert b"offsets_out" in message()
        assert _call(entry, handle, 0.0, 4, pairs, gap, offsets, at(384 + k)) == bad
        assert b"total_out" in message()


def test_the_contact_flavours_and_their_residency(tmp_path):
    # every flavour exists in both libraries, without scratch and within k_query_rays's budget: eight waves per SIMD
    want = sorted("rt::k_contact_pairs<%s, %s>" % (t, f) for t in ("float", "double") for f in ("true, false", "false, false", "false, true"))
    scan = {"rt::k_contact_scan_sums", "rt::k_contact_scan_spine", "rt::k_contact_scan_offsets", "rt::k_contact_item_nodes<float>",
            "rt::k_contact_item_nodes<double>"}
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_contact_pairs<")]
        assert sorted(flavours) == want, flavours
        for n in flavours:
            r = k[n]
            assert r["scratch"] == 0 and r["sgpr"] <= 80 and r["vgpr"] <= 64, (n, r)
        assert scan <= set(k), scan - set(k)
        for n in scan:
            assert k[n]["scratch"] == 0, (n, k[n])


def scalar_pair_gap(R, si, sj):
    """The definition, one operation at a time on numpy scalars of type R (each rounds once)."""
    rri, rrj = R(si[3] * si[3]), R(sj[3] * sj[3])
    if not (rri > 0 and rrj > 0):
        return R(np.inf)
    vx, vy, vz = R(sj[0] - si[0]), R(sj[1] - si[1]), R(sj[2] - si[2])
    vv = R(R(R(vx * vx) + R(vy * vy)) + R(vz * vz))
    return R(R(np.sqrt(vv) - np.sqrt(rrj)) - np.sqrt(rri))


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_pair_gaps_is_the_definition(R):
    inf = R(np.inf)
    # everything exact: centres 5 apart (3-4-5), radii 2 and 1.5 -> (5 - 1.5) - 2 = 1.5; touching spheres -> 0; one inside the other
    s = np.array([[0, 0, 0, 2], [3, 4, 0, 1.5], [0, 0, 3, 1], [0, 0, 0.5, 0.25]], R)
    g = rta.pair_gaps(s, [0, 0, 0], [1, 2, 3])
    assert g.dtype == R and g.shape == (3,) and g.tolist() == [1.5, 0.0, -1.75]
    # random spheres against the scalar restatement, in both orders of a pair (the two may differ by an ulp: the library always takes i < j)
    rng = np.random.default_rng(7)
    s = np.concatenate([rng.uniform(-1, 1, (40, 3)), rng.uniform(0.01, 0.4, (40, 1))], axis=1).astype(R)
    s[5, 3] = 0                                                                  # a dead slot as the tests hold it: {.., 0}
    s[9] = 0
    s[11, 3] = R(1e-30) if R == np.float32 else R(1e-200)                        # rr rounds to 0: no positive rr
    assert R(s[11, 3] * s[11, 3]) == 0
    i, j = np.triu_indices(40, 1)
    for a, b in ((i, j), (j, i)):
        got = rta.pair_gaps(s, a, b)
        ref = np.array([scalar_pair_gap(R, s[x], s[y]) for x, y in zip(a, b)], R)
        np.testing.assert_array_equal(got.view(np.uint32 if R == np.float32 else np.uint64), ref.view(np.uint32 if R == np.float32 else np.uint64))
    got = rta.pair_gaps(s, i, j)
    for dead in (5, 9, 11):
        assert (got[(i == dead) | (j == dead)] == inf).all()
    assert np.isfinite(got[~np.isin(i, (5, 9, 11)) & ~np.isin(j, (5, 9, 11))]).all()
    # the identity: the proximity queries' gap of sphere j from the centre of sphere i, minus the radius of sphere i
    near = rta.sphere_gaps(np.ascontiguousarray(s[:, :3]), s)
    rri = s[:, 3] * s[:, 3]
    with np.errstate(invalid="ignore"):
        ident = np.where(rri[i] > 0, near[i, j] - np.sqrt(rri[i]), inf).astype(R)
    np.testing.assert_array_equal(got, ident)
    # a tiny f32 radius: the root of the rounded square, not the radius (test_near_host.py works the value out)
    if R == np.float32:
        r = R(3e-23)
        root = np.sqrt(R(r * r))
        assert root != r
        g = rta.pair_gaps(np.array([[0, 0, 0, r], [0, 0, 0, r]], R), [0], [1])
        assert g[0] == R(R(0.0) - root) - root
    assert rta.pair_gaps(s, np.zeros(0, np.int64), np.zeros(0, np.int64)).shape == (0,)


def test_pair_gaps_checks_its_arguments():
    s = np.zeros((4, 4), np.float32)
    for spheres in (s.astype(np.float16), s[:, :3], s.reshape(-1), s.astype(np.int32)):
        with pytest.raises(ValueError, match="spheres"):
            rta.pair_gaps(spheres, [0], [1])
    for i, j in (([0.0], [1.0]), ([0, 1], [1]), ([[0]], [[1]]), ([0], [4]), ([-1], [0])):
        with pytest.raises(ValueError, match="i and j"):
            rta.pair_gaps(s, i, j)


class _Stand:
    """Enough of a Scene for DeviceScene's checks, which come before any call into the library."""
    def __init__(self, precision):
        self.precision = precision
        self.items = np.zeros((3, 4), np.float32 if precision == rta.RT_F32 else np.float64)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_contacts_checks_its_arguments_before_the_library(precision):
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h = _Stand(precision), 0, None
    with pytest.raises(ValueError, match="margin"):
        d.contacts(float("nan"))
    with pytest.raises((TypeError, ValueError)):
        d.contacts("near")
    with pytest.raises((TypeError, ValueError)):
        d.contacts(np.zeros(3))
    for capacity in (-1, 1 << 31, 1 << 40):
        with pytest.raises(ValueError, match="capacity"):
            d.contacts(0.0, capacity)
    with pytest.raises((TypeError, ValueError)):
        d.contacts(0.0, capacity="all")
