"""Contact islands (rt_scene_islands / rt_scene_impact_islands and their _device entries, csrc/rt_islands.hpp) without a
GPU: the ABI, the argument checks made before any device is touched, the residency of the hook kernel's flavours read back from the code
object, rta.pair_islands -- the definition in numpy -- on known answers and against a scalar union-find, and the checks the Python
wrapper makes before it calls the library."""
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
ENTRIES = ("rt_scene_islands", "rt_scene_islands_device", "rt_scene_impact_islands", "rt_scene_impact_islands_device")


def test_both_libraries_export_the_islands_entries_at_abi_5():
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
    assert len(capi.lib.rt_scene_islands_device.argtypes) == len(capi.lib.rt_scene_islands.argtypes) + 1 == 8
    assert len(capi.lib.rt_scene_impact_islands_device.argtypes) == len(capi.lib.rt_scene_impact_islands.argtypes) + 1 == 8
    assert callable(rta.pair_islands) and "pair_islands" in rta.__all__ and callable(DeviceScene.islands) and callable(DeviceScene.impact_islands)


def _call(entry, scene, first, label, index, size, n_islands):
    """first: the margin, or disp for the impact form."""
    f = getattr(capi.lib, entry)
    if entry.endswith("_device"):
        return f(scene, first, label, index, size, n_islands, None, None)
    return f(scene, first, label, index, size, n_islands, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check pointers, the margin and alignment before they use the scene: a stand-in handle will do
    stand_in = ctypes.create_string_buffer(8192)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    words = (ctypes.c_uint64 * 96)()
    at = lambda k: ctypes.c_void_p(ctypes.addressof(words) + k)
    label, index, size, n_islands, disp = at(0), at(128), at(256), at(384), at(512)
    moving = "impact" in entry
    first = disp if moving else 0.0
    bad = capi.RT_ERR_INVALID_ARGUMENT
    message = capi.lib.rt_last_error_message
    assert _call(entry, None, first, label, index, size, n_islands) == bad        # NULL scene
    assert b"scene" in message() and entry.encode() + b":" in message()
    assert _call(entry, handle, first, None, index, size, n_islands) == bad       # NULL label_out
    assert b"label_out" in message()
    assert _call(entry, handle, first, None, None, None, None) == bad
    if moving:
        assert _call(entry, handle, None, label, index, size, n_islands) == bad   # NULL disp
        assert b"disp" in message()
        for k in (1, 2, 3):
            assert _call(entry, handle, at(512 + k), label, index, size, n_islands) == bad
            assert b"disp" in message()
    else:
        assert _call(entry, handle, float("nan"), label, index, size, n_islands) == bad
        assert b"NaN" in message()
        assert _call(entry, handle, float("nan"), label, None, None, None) == bad
    for k in (1, 2, 3):
        assert _call(entry, handle, first, at(k), index, size, n_islands) == bad
        assert b"label_out" in message()
        assert _call(entry, handle, first, label, at(128 + k), size, n_islands) == bad
        assert b"index_out" in message()
        assert _call(entry, handle, first, label, index, at(256 + k), n_islands) == bad
        assert b"size_out" in message()
    for k in (1, 4, 7):
        assert _call(entry, handle, first, label, index, size, at(384 + k)) == bad
        assert b"n_islands_out" in message()


def test_the_islands_entries_are_not_in_the_refusals_table():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_query_refusals as recorder
    assert not set(ENTRIES) & set(recorder.ENTRIES)


def test_the_hook_flavours_and_their_residency(tmp_path):
    # every flavour exists in both libraries, without scratch and within eight waves per SIMD, as the pair walks they restate; the scan is
    # the contact pairs' own, not a copy
    want = sorted("rt::k_island_hook<%s, %s, %s>" % (t, c, m) for t in ("float", "double") for c in ("true", "false") for m in ("true", "false"))
    rest = {"rt::k_island_init", "rt::k_island_labels<float>", "rt::k_island_labels<double>", "rt::k_island_finish"}
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_island_hook<")]
        assert sorted(flavours) == want, flavours
        for n in flavours:
            r = k[n]
            assert r["scratch"] == 0 and r["sgpr"] <= 80 and r["vgpr"] <= 64, (n, r)
        assert rest <= set(k), rest - set(k)
        for n in rest:
            assert k[n]["scratch"] == 0, (n, k[n])
        assert not [n for n in k if "island" in n and "scan" in n]
        # the pair kernels are untouched: their flavours are the ones their own tests pin
        assert len([n for n in k if n.startswith("rt::k_contact_pairs<")]) == 6 and len([n for n in k if n.startswith("rt::k_impact_pairs<")]) == 6


def scalar_islands(pairs, n, live):
    """The definition with a textbook union-find, one edge at a time."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for a, b in pairs:
        a, b = find(int(a)), find(int(b))
        if a != b:
            parent[max(a, b)] = min(a, b)
    label = [find(x) if live[x] else -1 for x in range(n)]
    roots = sorted(set(l for l in label if l >= 0))
    index = [roots.index(l) if l >= 0 else -1 for l in label]
    size = [label.count(l) if l >= 0 else 0 for l in label]
    return label, index, size, len(roots)


def check(got, label, index, size, n_islands):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.uint32 and isinstance(got[3], int)
    assert got[0].tolist() == list(label) and got[1].tolist() == list(index) and got[2].tolist() == list(size) and got[3] == n_islands


def test_pair_islands_known_answers():
    # no pair at all: every slot an island of one -- as a list, as an empty (0, 2) array, and for no slot at all
    for empty in ([], np.zeros((0, 2), np.int32)):
        check(rta.pair_islands(empty, 4), [0, 1, 2, 3], [0, 1, 2, 3], [1, 1, 1, 1], 4)
    check(rta.pair_islands([], 0), [], [], [], 0)
    # a chain 0 - 1 - ... - 9 with its edges scrambled, given in either direction and some of them twice
    rng = np.random.default_rng(5)
    chain = np.stack([np.arange(9), np.arange(1, 10)], axis=1)
    chain = np.concatenate([chain, chain[:3]])[rng.permutation(12)]
    chain[::2] = chain[::2, ::-1]
    check(rta.pair_islands(chain, 10), [0] * 10, [0] * 10, [10] * 10, 1)
    # two components whose minima (1 and 2) are not their first-listed members, and a slot in no pair on either side of them
    pairs = [(7, 4), (4, 1), (9, 5), (5, 2), (2, 8)]
    check(rta.pair_islands(pairs, 11), [0, 1, 2, 3, 1, 2, 6, 1, 2, 2, 10], [0, 1, 2, 3, 1, 2, 4, 1, 2, 2, 5], [1, 3, 4, 1, 3, 4, 1, 3, 4, 4, 1], 6)
    # live masks: a slot that is not live is -1 / -1 / 0 and takes no index; uint8 and bool masks alike
    live = np.ones(11, bool)
    live[[0, 3, 10]] = False
    for mask in (live, live.astype(np.uint8)):
        check(rta.pair_islands(pairs, 11, mask), [-1, 1, 2, -1, 1, 2, 6, 1, 2, 2, -1], [-1, 0, 1, -1, 0, 1, 2, 0, 1, 1, -1], [0, 3, 4, 0, 3, 4, 1, 3, 4, 4, 0], 3)
    check(rta.pair_islands([], 3, np.zeros(3, bool)), [-1] * 3, [-1] * 3, [0] * 3, 0)
    # the lowest slot dead: the island of the rest is labelled with its own minimum
    check(rta.pair_islands([(1, 2), (2, 3)], 4, np.array([0, 1, 1, 1], np.uint8)), [-1, 1, 1, 1], [-1, 0, 0, 0], [0, 3, 3, 3], 1)


def test_pair_islands_is_the_union_find_of_the_definition():
    rng = np.random.default_rng(11)
    for n, m in ((1, 0), (2, 1), (50, 20), (50, 60), (400, 150), (400, 390), (400, 3000)):
        live = rng.random(n) < 0.8
        alive = np.flatnonzero(live)
        pairs = rng.choice(alive, (m, 2)) if len(alive) and m else np.zeros((0, 2), np.int64)
        check(rta.pair_islands(pairs, n, live), *scalar_islands(pairs, n, live))
        check(rta.pair_islands(pairs.astype(np.int32), n, live.astype(np.uint8)), *scalar_islands(pairs, n, live))
    # a long path whose labels have to travel its whole length: slots in a random order along the path
    order = rng.permutation(3000)
    path = np.stack([order[:-1], order[1:]], axis=1)
    label, index, size, n_islands = rta.pair_islands(path, 3000)
    assert n_islands == 1 and not label.any() and not index.any() and (size == 3000).all()


def test_pair_islands_checks_its_arguments():
    for pairs in ([(0, 1, 2)], [0, 1], np.zeros((2, 2), np.float32), [[[0, 1]]]):
        with pytest.raises(ValueError, match="pairs"):
            rta.pair_islands(pairs, 4)
    for pairs in ([(0, 4)], [(-1, 0)]):
        with pytest.raises(ValueError, match="slots"):
            rta.pair_islands(pairs, 4)
    for live in (np.ones(3, bool), np.ones(4, np.int32), np.ones((4, 1), bool)):
        with pytest.raises(ValueError, match="live"):
            rta.pair_islands([(0, 1)], 4, live)
    with pytest.raises(ValueError, match="not live"):
        rta.pair_islands([(0, 1)], 4, np.array([1, 0, 1, 1], np.uint8))
    with pytest.raises(ValueError, match="n_items"):
        rta.pair_islands([], -1)


class _Stand:
    """Enough of a Scene for DeviceScene's checks, which come before any call into the library."""
    def __init__(self, precision):
        self.precision = precision
        self.items = np.zeros((3, 4), np.float32 if precision == rta.RT_F32 else np.float64)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_the_wrappers_check_their_arguments_before_the_library(precision):
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h = _Stand(precision), 0, None
    R = np.float32 if precision == rta.RT_F32 else np.float64
    other = np.float64 if precision == rta.RT_F32 else np.float32
    with pytest.raises(ValueError, match="margin"):
        d.islands(float("nan"))
    with pytest.raises((TypeError, ValueError)):
        d.islands("near")
    with pytest.raises((TypeError, ValueError)):
        d.islands(np.zeros(3))
    for disp in (np.zeros((3, 3), other), np.zeros((2, 3), R), np.zeros((3, 4), R), np.zeros(9, R), [[0.0] * 3] * 3, None):
        with pytest.raises(ValueError, match="disp"):
            d.impact_islands(disp)
