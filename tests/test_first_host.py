"""First contacts (rt_first_contacts / rt_first_contacts_device, csrc/rt_first.hpp) without a GPU: the ABI, the argument
checks made before any device is touched, the residency of the kernel's flavours read back from the code object, and FirstWalker -- the
restatement the GPU is held to bit for bit -- against the swept walker's lists on the inputs the GPU suite uses: the result is the
row's smallest time at its lowest slot, for every query, with no allowance."""
import ctypes
import os
import re

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from rust_tracer_amd.scene import DeviceScene
from tests.test_gpu_first import SCENES, FirstWalker
from tests.test_gpu_impacts import scenes
from tests.test_gpu_near import LIGHT, EYE
from tests.test_gpu_swept import MOTIONS, N_QUERIES, Walker, queries_of, scene_disp
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB
from tests.test_wrapper_calls_host import lib  # noqa: F401  (the fixture that stands in for capi.lib)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_first_contacts", "rt_first_contacts_device")
BITS = {np.float32: np.uint32, np.float64: np.uint64}


def test_both_libraries_export_the_first_contact_entries_at_abi_5():
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
    assert len(capi.lib.rt_first_contacts_device.argtypes) == len(capi.lib.rt_first_contacts.argtypes) + 1 == 13
    assert callable(DeviceScene.first_contacts)


def _call(entry, scene, mode, queries, qdisp, n, disp, exclude, order, time, item, normal):
    f = getattr(capi.lib, entry)
    args = (scene, mode, queries, qdisp, n, disp, exclude, order, time, item, normal, None)
    return f(*args) if entry == "rt_first_contacts" else f(*args, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check pointers, n, the mode and alignment -- the host entry the values too -- before they use the scene: a stand-in handle
    # will do (its precision reads RT_F32)
    stand_in = ctypes.create_string_buffer(8192)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    words = (ctypes.c_uint64 * 256)()
    at = lambda k: ctypes.c_void_p(ctypes.addressof(words) + k)
    queries, qdisp, disp, exclude, order, time, item, normal = (at(128 * k) for k in range(8))
    bad = capi.RT_ERR_INVALID_ARGUMENT
    message = capi.lib.rt_last_error_message
    good = dict(scene=handle, mode=capi.RT_SWEEP_NEAREST, queries=queries, qdisp=qdisp, n=4, disp=disp, exclude=exclude, order=order, time=time, item=item,
                normal=normal)

    def refused(word, **change):
        assert _call(entry, **dict(good, **change)) == bad, (word, change)
        assert word in message(), (word, message())
    refused(b"scene", scene=None)
    refused(b"queries", queries=None)
    refused(b"qdisp", qdisp=None)
    refused(b"time_out", time=None)
    refused(b"time_out", time=None, item=None, normal=None)
    refused(b"n == 0", n=0)
    for mode in (2, -1, 7):
        refused(b"mode", mode=mode)
    for k in (1, 2, 3):
        for name, word, base in (("item", b"item_out", 6), ("exclude", b"exclude", 3), ("order", b"order", 4), ("queries", b"queries", 0), ("qdisp", b"qdisp", 1),
                                 ("disp", b" disp", 2), ("time", b"time_out", 5), ("normal", b"normal_out", 7)):
            refused(word, **{name: at(128 * base + k)})
    if entry != "rt_first_contacts":
        return
    # the host entry's domain, as far as it needs no scene: the queries, their displacements and the order
    f32 = lambda values: np.array(values, np.float32)
    q = f32([[0, 0, 0, 1], [1, 2, 3, 0], [4, 5, 6, 0.5], [7, 8, 9, 2]])
    dq = np.zeros((4, 3), np.float32)
    perm = np.array([2, 0, 3, 1], np.uint32)
    host = lambda **change: dict(dict(queries=q.ctypes.data, qdisp=dq.ctypes.data, disp=None, exclude=None, order=perm.ctypes.data), **change)
    for mode in (capi.RT_SWEEP_NEAREST, capi.RT_SWEEP_ANY):
        for value in (np.nan, np.inf, -np.inf, 2e15, -2e15):
            for col in range(3):
                x = q.copy()
                x[2, col] = value
                refused(b"query 2", mode=mode, **host(queries=x.ctypes.data))
                x = dq.copy()
                x[3, col] = value
                refused(b"qdisp of query 3", mode=mode, **host(qdisp=x.ctypes.data))
    for value in (np.nan, -1.0, -1e-30, np.inf, -np.inf, 2e15):
        x = q.copy()
        x[1, 3] = value
        refused(b"radius", **host(queries=x.ctypes.data))
    for values in ([0, 1, 2, 2], [0, 1, 2, 4], [1, 1, 1, 1], [0, 1, 2, 0xFFFFFFFF]):
        o = np.array(values, np.uint32)
        refused(b"order", **host(order=o.ctypes.data))


def test_the_first_contact_flavours_and_their_residency(tmp_path):
    # every flavour exists in both libraries, without scratch; f32 within k_query_rays's budget (eight waves per SIMD), f64 within 128
    # vector registers -- DESIGN.md 4.20's table has the counts: they are at most 64 too, so amdgpu_waves_per_eu(8) stays on all eight
    want = sorted("rt::k_first_contacts<%s, %s, %s>" % (t, c, a) for t in ("float", "double") for c in ("false", "true") for a in ("false", "true"))
    shared = {"rt::k_swept_query_magnitude<float>", "rt::k_swept_query_magnitude<double>", "rt::k_impact_motion_items<float>", "rt::k_impact_motion_items<double>",
              "rt::k_impact_motion_bounds<float>", "rt::k_impact_motion_bounds<double>", "rt::k_impact_bound_radii<float>", "rt::k_impact_bound_radii<double>"}
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if "first" in n]
        assert sorted(flavours) == want, flavours                                # ... and no kernel of its own besides them
        for n in flavours:
            r = k[n]
            print(n, r)
            assert r["scratch"] == 0, (n, r)
            if "<float" in n:
                assert r["sgpr"] <= 80 and r["vgpr"] <= 64, (n, r)
            else:
                assert r["vgpr"] <= 128, (n, r)
                assert r["vgpr"] <= 64, (n, r)                                   # the attribute is kept on f64: it rests on this
        # the magnitude and the motion table's kernels are the swept entry's and the impact pairs' own, once each
        assert shared <= set(k), shared - set(k)
        assert len([n for n in k if "magnitude" in n or "k_impact_motion" in n or "k_impact_bound_radii" in n]) == len(shared)
        # the existing walks keep their flavours: nothing was added to them
        assert len([n for n in k if n.startswith("rt::k_swept_overlaps<")]) == 6 and len([n for n in k if n.startswith("rt::k_impact_pairs<")]) == 6


def flat_scene(R, items):
    return rta.Scene(np.array(items, R), rta.normalized(LIGHT, rta.RT_F32 if R == np.float32 else rta.RT_F64), EYE,
                     precision=rta.RT_F32 if R == np.float32 else rta.RT_F64)


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_hand_cases_with_exact_values(R):
    inf = R(np.inf)
    arr = lambda x: np.array(x, R)
    # {0,0,0,1} moving {2,0,0} against {4,0,0,1}: cc = 12, b = 8, disc = 16, t = 12 / 12 -- a contact at exactly 1 is found
    w = FirstWalker(flat_scene(R, [[4, 0, 0, 1]]))
    for any_hit in (False, True):
        time, item, normal, st = w.first(arr([[0, 0, 0, 1]]), arr([[2, 0, 0]]), any_hit=any_hit)
        assert time[0] == 1 and item[0] == 0 and normal[0].tolist() == [-1, 0, 0] and (st["primary"], st["hits"], st["sphere_tests"]) == (1, 1, 1)
    # two identical items: the lower slot, in both modes; and the second is still tested by NEAREST (t = 1 does not finish the walk), not by ANY
    w = FirstWalker(flat_scene(R, [[4, 0, 0, 1], [4, 0, 0, 1], [9, 9, 9, 1]]))
    time, item, _, st = w.first(arr([[0, 0, 0, 1]]), arr([[2, 0, 0]]))
    assert time[0] == 1 and item[0] == 0 and st["sphere_tests"] == 3
    time, item, _, st = w.first(arr([[0, 0, 0, 1]]), arr([[2, 0, 0]]), any_hit=True)
    assert time[0] == 1 and item[0] == 0 and st["sphere_tests"] == 1
    assert w.first(arr([[0, 0, 0, 1]]), arr([[2, 0, 0]]), exclude=np.array([0], np.int32))[1][0] == 1      # ... and the twin when the first is excluded
    # a start in contact with several items: the first slot at t = 0, and the walk stops there by the counters
    w = FirstWalker(flat_scene(R, [[9, 9, 9, 1], [0.5, 0, 0, 1], [0, 0.5, 0, 1], [0, 0, 0.5, 1]]))
    time, item, normal, st = w.first(arr([[0, 0, 0, 1]]), arr([[2, 0, 0]]))
    assert time[0] == 0 and item[0] == 1 and normal[0].tolist() == [-1, 0, 0] and st["sphere_tests"] == 2 and st["tests_executed"] == 2
    everything = Walker(flat_scene(R, [[9, 9, 9, 1], [0.5, 0, 0, 1], [0, 0.5, 0, 1], [0, 0, 0.5, 1]])).all(arr([[0, 0, 0, 1]]), arr([[2, 0, 0]]))
    assert everything[0].tolist() == [1, 2, 3] and everything[4]["sphere_tests"] == 4
    # the excluded slot is tested and counted, and never the result: the walk goes on to the next one
    time, item, _, st = w.first(arr([[0, 0, 0, 1]]), arr([[2, 0, 0]]), exclude=np.array([1], np.int32))
    assert time[0] == 0 and item[0] == 2 and st["sphere_tests"] == 3
    # a query with q = -1 or NaN: +inf, -1 and a zero normal, no test; the one beside it is not disturbed
    for q in (-1.0, np.nan):
        time, item, normal, st = w.first(arr([[0, 0, 0, q], [0, 0, 0, 1]]), arr([[2, 0, 0], [2, 0, 0]]))
        assert time[0] == inf and item[0] == -1 and normal[0].tolist() == [0, 0, 0] and time[1] == 0 and item[1] == 1
        assert (st["primary"], st["hits"], st["tests_executed"]) == (1, 1, 2)
    # a later contact that is EARLIER replaces the result; an equal one does not
    w = FirstWalker(flat_scene(R, [[6, 0, 0, 1], [4, 0, 0, 1], [4, 0, 0, 1]]))
    time, item, _, _ = w.first(arr([[0, 0, 0, 1]]), arr([[8, 0, 0]]))
    assert time[0] == R(0.25) and item[0] == 1                                   # cc = 12, b = 32, disc = 1024 - 768 = 256: 12 / 48
    assert w.first(arr([[0, 0, 0, 1]]), arr([[8, 0, 0]]), any_hit=True)[1][0] == 0


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_walker_returns_the_smallest_time_of_the_swept_row_at_its_lowest_slot(R):
    """FirstWalker against Walker.all on the inputs of tests/test_gpu_first.py, with numpy alone -- the proof that those inputs are well
    chosen: a bound's time never lies above an item's below it within rounding there, so the shrinking window loses nothing."""
    precision = rta.RT_F32 if R == np.float32 else rta.RT_F64
    U = BITS[R]
    fewer = 0
    for name in SCENES:
        s, seed = scenes(precision)[name]
        w = FirstWalker(s)
        for qfam, sfam in MOTIONS:
            what = (name, qfam, sfam)
            queries, qdisp = queries_of(s, seed, qfam)
            assert len(queries) == N_QUERIES == 80
            disp = scene_disp(s, seed, sfam)
            items, times, normals, offsets, list_st = w.all(queries, qdisp, disp)
            time, item, normal, st = w.first(queries, qdisp, disp)
            a_time, a_item, a_normal, a_st = w.first(queries, qdisp, disp, any_hit=True)
            o = offsets.astype(np.int64)
            for g in range(N_QUERIES):
                row_i, row_t, row_n = items[o[g]:o[g + 1]], times[o[g]:o[g + 1]], normals[o[g]:o[g + 1]]
                assert (item[g] >= 0) == (a_item[g] >= 0) == (len(row_i) > 0), (what, g)      # a result exists exactly where the row is not empty
                if not len(row_i):
                    assert np.isinf(time[g]) and not normal[g].any(), (what, g)
                    continue
                k = int(np.flatnonzero(row_t == row_t.min())[0])                 # the smallest time at its lowest slot
                assert item[g] == row_i[k] and time[g].view(U) == row_t[k].view(U) and (normal[g].view(U) == row_n[k].view(U)).all(), (what, g)
                assert a_item[g] == row_i[0] and a_time[g].view(U) == row_t[0].view(U) and (a_normal[g].view(U) == row_n[0].view(U)).all(), (what, g)
            assert (item >= 0).any() and (item < 0).any(), what
            assert st["hits"] == a_st["hits"] == list_st["hits"] and st["primary"] == list_st["primary"], what
            assert a_st["tests_executed"] <= st["tests_executed"] <= list_st["tests_executed"], (what, st, list_st)
            fewer += qfam == "fast" and st["tests_executed"] < list_st["tests_executed"]
    assert fewer > 0


class _Stand:
    """Enough of a Scene for DeviceScene's checks, which come before any call into the library."""
    def __init__(self, precision):
        self.precision = precision
        self.items = np.zeros((3, 4), np.float32 if precision == rta.RT_F32 else np.float64)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_first_contacts_checks_its_arguments_before_the_library(precision):
    R = np.float32 if precision == rta.RT_F32 else np.float64
    other = np.float64 if precision == rta.RT_F32 else np.float32
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h = _Stand(precision), 0, None
    q, dq, disp = np.zeros((5, 4), R), np.zeros((5, 3), R), np.zeros((3, 3), R)
    for queries in (q.astype(other), q[:, :3], q[:0], q.reshape(-1), None):
        with pytest.raises(ValueError, match="queries"):
            d.first_contacts(queries, dq)
    for qdisp in (dq.astype(other), dq[:4], np.zeros((5, 4), R), None, 0.0):
        with pytest.raises(ValueError, match="qdisp"):
            d.first_contacts(q, qdisp)
    for bad in (disp.astype(other), np.zeros((5, 3), R), np.zeros((3, 4), R), 0.0):
        with pytest.raises(ValueError, match="disp"):
            d.first_contacts(q, dq, bad)
    for exclude in (np.zeros(5, np.int64), np.zeros(4, np.int32)):
        with pytest.raises(ValueError, match="exclude"):
            d.first_contacts(q, dq, exclude=exclude)
    for order in (np.zeros(4, np.uint32), np.zeros(5, np.float32), np.full(5, -1), True):
        with pytest.raises(ValueError, match="order"):
            d.first_contacts(q, dq, order=order)
    for normals, out in ((False, (np.zeros(5, R),)), (True, (np.zeros(5, R), np.zeros(5, np.int32))), (False, (np.zeros(5, R), np.zeros(5, np.int64)))):
        with pytest.raises(ValueError, match="out"):
            d.first_contacts(q, dq, normals=normals, out=out)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_the_call_first_contacts_makes_into_the_library(lib, precision):
    # tests/test_wrapper_calls_host.py's stand-in for capi.lib: one call of the host entry, its arguments in the header's order, NULL where
    # nothing was given, the staged bytes, and the shapes and dtypes that come back; every expectation is written out here
    from tests.test_wrapper_calls_host import EXCLUDE, ITEMS, N, ORDER, ORDER_BYTES, _device_scene, _is_stats, _nulls, _real, _shapes
    R = _real(precision)
    d = _device_scene(precision)
    rng = np.random.default_rng(12)
    queries, qdisp, disp = np.abs(rng.standard_normal((N, 4))).astype(R), rng.standard_normal((N, 3)).astype(R), rng.standard_normal((ITEMS, 3)).astype(R)
    esz = np.dtype(R).itemsize
    lib.snap["rt_first_contacts"] = {2: 4 * N * esz, 3: 3 * N * esz, 5: 3 * ITEMS * esz, 6: 4 * N, 7: 4 * N}
    res = d.first_contacts(queries, qdisp)
    (name, args, seen), = lib.take()
    assert name == "rt_first_contacts" and len(args) == 12 and args[1] == capi.RT_SWEEP_NEAREST and args[4] == N
    assert _nulls(args) == [5, 6, 7, 10, 11]                                      # disp, exclude, order, normal_out, stats
    assert seen[2] == queries.tobytes() and seen[3] == qdisp.tobytes()
    assert _shapes(res) == [((N,), R), ((N,), np.int32)]
    res = d.first_contacts(queries, qdisp, disp, any_hit=True, exclude=EXCLUDE, order=ORDER, normals=True, stats=True)
    (name, args, seen), = lib.take()
    assert name == "rt_first_contacts" and len(args) == 12 and args[1] == capi.RT_SWEEP_ANY and args[4] == N and _nulls(args) == [] and _is_stats(args[11])
    assert seen[5] == disp.tobytes() and seen[6] == EXCLUDE.tobytes() and seen[7] == ORDER_BYTES
    assert _shapes(res[:3]) == [((N,), R), ((N,), np.int32), ((N, 3), R)] and isinstance(res[3], dict) and len(res) == 4
    out = (np.zeros(N, R), np.zeros(N, np.int32), np.zeros((N, 3), R))
    res = d.first_contacts(queries, qdisp, normals=True, out=out)
    (name, args, seen), = lib.take()
    assert all(a is b for a, b in zip(res, out)) and [args[8], args[9], args[10]] == [a.ctypes.data for a in out]
