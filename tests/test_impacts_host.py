"""Impact pairs (rt_scene_impacts / rt_scene_impacts_device, csrc/rt_impacts.hpp) without a GPU: the ABI, the argument
checks made before any device is touched, the residency of the kernel's flavours read back from the code object, rta.pair_impacts -- the
metric's definition in numpy -- against a scalar restatement and against the geometry in higher precision, and the checks the Python
wrapper makes before it calls the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from rust_tracer_amd.scene import DeviceScene
from tests.scenes import random_nested_scene
from tests.test_gpu_impacts import FAMILIES, SEEDS, displacements
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB
from tests.test_scales_contact_host import higher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_scene_impacts", "rt_scene_impacts_device")


def test_both_libraries_export_the_impacts_entries_at_abi_5():
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
    assert len(capi.lib.rt_scene_impacts_device.argtypes) == len(capi.lib.rt_scene_impacts.argtypes) + 1 == 9
    assert callable(rta.pair_impacts) and "pair_impacts" in rta.__all__ and callable(DeviceScene.impacts)


def _call(entry, scene, disp, capacity, pairs, time, offsets, total):
    f = getattr(capi.lib, entry)
    if entry == "rt_scene_impacts":
        return f(scene, disp, capacity, pairs, time, offsets, total, None)
    return f(scene, disp, capacity, pairs, time, offsets, total, None, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check pointers, the capacity and alignment before they use the scene: a stand-in handle will do
    stand_in = ctypes.create_string_buffer(8192)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    words = (ctypes.c_uint64 * 80)()
    at = lambda k: ctypes.c_void_p(ctypes.addressof(words) + k)
    pairs, time, offsets, total, disp = at(0), at(128), at(256), at(384), at(512)
    bad = capi.RT_ERR_INVALID_ARGUMENT
    message = capi.lib.rt_last_error_message
    assert _call(entry, None, disp, 4, pairs, time, offsets, total) == bad       # NULL scene
    assert b"scene" in message()
    assert _call(entry, handle, None, 4, pairs, time, offsets, total) == bad     # NULL disp
    assert b"disp" in message()
    assert _call(entry, handle, disp, 4, pairs, time, offsets, None) == bad      # NULL total_out
    assert b"total_out" in message()
    assert _call(entry, handle, disp, 4, None, time, offsets, total) == bad      # time_out without pairs_out
    assert b"time_out without pairs_out" in message()
    for capacity in (1 << 31, 0xFFFFFFFF):
        assert _call(entry, handle, disp, capacity, pairs, time, offsets, total) == bad
        assert b"capacity" in message()
    for k in (1, 2, 3):
        assert _call(entry, handle, disp, 4, at(k), time, offsets, total) == bad
        assert b"pairs_out" in message()
        assert _call(entry, handle, disp, 4, pairs, at(128 + k), offsets, total) == bad
        assert b"time_out" in message()
        assert _call(entry, handle, at(512 + k), 4, pairs, time, offsets, total) == bad
        assert b"disp" in message()
    for k in (1, 4, 7):
        assert _call(entry, handle, disp, 4, pairs, time, at(256 + k), total) == bad
        assert b"offsets_out" in message()
        assert _call(entry, handle, disp, 4, pairs, time, offsets, at(384 + k)) == bad
        assert b"total_out" in message()


def test_the_impact_flavours_and_their_residency(tmp_path):
    # every flavour exists in both libraries, without scratch; f32 within k_query_rays's budget (eight waves per SIMD), f64 within 128
    # vector registers -- DESIGN.md 4.18's table has the counts: they are below 64 too, so amdgpu_waves_per_eu(8) holds for all six
    want = sorted("rt::k_impact_pairs<%s, %s>" % (t, f) for t in ("float", "double") for f in ("true, false", "false, false", "false, true"))
    pre = {"rt::k_impact_motion_items<float>", "rt::k_impact_motion_items<double>", "rt::k_impact_motion_bounds<float>", "rt::k_impact_motion_bounds<double>"}
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_impact_pairs<")]
        assert sorted(flavours) == want, flavours
        for n in flavours:
            r = k[n]
            assert r["scratch"] == 0, (n, r)
            if "<float" in n:
                assert r["sgpr"] <= 80 and r["vgpr"] <= 64, (n, r)
            else:
                assert r["vgpr"] <= 128, (n, r)
                assert r["vgpr"] <= 64, (n, r)                                   # the table's "8 waves per SIMD" for f64 rests on this
        assert pre <= set(k), pre - set(k)
        for n in pre:
            assert k[n]["scratch"] == 0, (n, k[n])
        # the scan is the contact pairs' own, not a copy
        assert not [n for n in k if "impact" in n and "scan" in n]


def scalar_pair_impact(R, si, sj, di, dj):
    """The definition, one operation at a time on numpy scalars of type R (each rounds once)."""
    inf = R(np.inf)
    rri, rrj = R(si[3] * si[3]), R(sj[3] * sj[3])
    if not (rri > 0 and rrj > 0):
        return inf
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        v = [R(sj[k] - si[k]) for k in range(3)]
        w = [R(di[k] - dj[k]) for k in range(3)]
        rad = R(R(np.sqrt(rrj) + R(0.0)) + np.sqrt(rri))
        RR = R(rad * rad)
        dot = lambda p, q: R(R(R(p[0] * q[0]) + R(p[1] * q[1])) + R(p[2] * q[2]))
        a, b, c = dot(w, w), dot(v, w), R(dot(v, v) - RR)
        disc = R(R(b * b) - R(a * c))
        if not c > 0:
            return R(0.0)
        if not b > 0 or disc < 0:
            return inf
        return R(c / R(b + np.sqrt(disc)))


BRANCHES = ("dead i", "dead j", "contact at the start", "receding", "w = 0", "passing by", "impact before 1", "impact after 1")


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_pair_impacts_is_the_definition(R):
    inf = R(np.inf)
    # every branch once, with exact values: (spheres, displacements, i, j) -> t
    s = np.array([[0, 0, 0, 1], [4, 0, 0, 1], [0, 0, 0, 0], [1.5, 0, 0, 1], [0, 4, 0, 1], [10, 0, 0, 1], [3, 5, 0, 1]], R)
    d = np.array([[2, 0, 0], [0, 0, 0], [9, 9, 9], [-1, 0, 0], [2, 0, 0], [-1, 0, 0], [0, 0, 0]], R)
    want = {"dead i": ((2, 3), inf), "dead j": ((0, 2), inf),
            "contact at the start": ((0, 3), R(0.0)),                            # centres 1.5 apart, radii 1 + 1: c < 0
            "receding": ((3, 1), inf),                                           # v = (2.5, 0, 0), w = (-1, 0, 0): b < 0
            "w = 0": ((0, 4), inf),                                              # both move by (2, 0, 0): a = b = 0
            "passing by": ((0, 6), inf),                                         # v = (3, 5, 0), w = (2, 0, 0): b = 6, disc = 36 - 4 * 30 < 0
            "impact before 1": ((0, 1), R(1.0)),                                 # gap 2, closing 2: c = 12, b = 8, disc = 64 - 48 = 16, 12 / 12
            "impact after 1": ((0, 5), R(96.0) / R(36.0))}                       # v = (10, 0, 0), w = (3, 0, 0): c = 96, b = 30, disc = 36
    assert tuple(want) == BRANCHES
    for name, ((i, j), t) in want.items():
        got = rta.pair_impacts(s, d, [i], [j])
        assert got.dtype == R and got.shape == (1,), name
        assert got[0] == t and got[0] == scalar_pair_impact(R, s[i], s[j], d[i], d[j]), (name, got[0], t)
    assert rta.pair_impacts(s, d, [0], [5])[0] > 1 and rta.pair_impacts(s, d, [0], [1])[0] <= 1
    # random spheres and both displacement families against the scalar restatement, in both orders of a pair
    it = random_nested_scene(1)[0].astype(R)
    it[5, 3] = 0                                                                 # a dead slot as the tests hold it: {.., 0}
    it[9] = 0
    it[11, 3] = R(1e-30) if R == np.float32 else R(1e-200)                       # rr rounds to 0: no positive rr
    assert R(it[11, 3] * it[11, 3]) == 0
    n = len(it)
    i, j = np.triu_indices(n, 1)
    U = np.uint32 if R == np.float32 else np.uint64
    for family in FAMILIES:
        disp = displacements(it, 1, family, R)
        seen = set()
        for a, b in ((i, j), (j, i)):
            got = rta.pair_impacts(it, disp, a, b)
            ref = np.array([scalar_pair_impact(R, it[x], it[y], disp[x], disp[y]) for x, y in zip(a, b)], R)
            np.testing.assert_array_equal(got.view(U), ref.view(U))
            seen |= {"inf" if t == inf else "0" if t == 0 else "<=1" if t <= 1 else ">1" for t in got.tolist()}
        assert seen == {"inf", "0", "<=1", ">1"}, (family, seen)
        got = rta.pair_impacts(it, disp, i, j)
        for dead in (5, 9, 11):
            assert (got[(i == dead) | (j == dead)] == inf).all()
    # inflate = 0 is no inflation, bit for bit; a positive E adds to the radius of sphere j
    disp = displacements(it, 1, "fast", R)
    np.testing.assert_array_equal(rta.pair_impacts(it, disp, i, j, np.zeros(n, R)).view(U), rta.pair_impacts(it, disp, i, j).view(U))
    E = np.full(n, R(0.25))
    assert (rta.pair_impacts(it, disp, i, j, E) <= rta.pair_impacts(it, disp, i, j)).all()
    assert rta.pair_impacts(it, disp, np.zeros(0, np.int64), np.zeros(0, np.int64)).shape == (0,)


def test_pair_impacts_checks_its_arguments():
    s, d = np.zeros((4, 4), np.float32), np.zeros((4, 3), np.float32)
    for spheres in (s.astype(np.float16), s[:, :3], s.reshape(-1), s.astype(np.int32)):
        with pytest.raises(ValueError, match="spheres"):
            rta.pair_impacts(spheres, d, [0], [1])
    for disp in (d.astype(np.float64), d[:3], np.zeros((4, 4), np.float32), d.reshape(-1)):
        with pytest.raises(ValueError, match="disp"):
            rta.pair_impacts(s, disp, [0], [1])
    for inflate in (np.zeros(3, np.float32), np.zeros(4, np.float64)):
        with pytest.raises(ValueError, match="inflate"):
            rta.pair_impacts(s, d, [0], [1], inflate)
    for i, j in (([0.0], [1.0]), ([0, 1], [1]), ([[0]], [[1]]), ([0], [4]), ([-1], [0])):
        with pytest.raises(ValueError, match="i and j"):
            rta.pair_impacts(s, d, i, j)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_pair_impacts_is_the_time_two_moving_spheres_first_touch(precision):
    """Every pair i < j of random_nested_scene(0 .. 3) under both displacement families against the geometry in higher precision H (float64
    for f32, np.longdouble for f64), from the REAL inputs: v = c_j - c_i, w = d_i - d_j, R = r_i + r_j, A = w.w, B = v.w, VV = v.v,
    C = VV - R^2, D = B^2 - A C, S = sqrt(D), T = C / (B + S).  With u the unit roundoff of REAL and K = VV + R^2, the roundings carried
    through c / (b + sqrt(disc)):
        c      9 u K                  (two rounded differences and a sum of three squares: 6 u VV; r*r, two roots, a sum and a square: 8 u R^2;
                                       the last subtraction)
        b      6 u |v| |w|
        disc   32 u A K               (b*b: 13 u VV A; a*c: A 9 u K + 7 u A |C|; the subtraction u |D| <= u A (2 VV + R^2))
        root   16 u A K / S + u S
        b + s  the two above + u (B + S)
        t      [9 K + T (6 |v| |w| + 16 A K / S + S + (B + S))] u / (B + S) + u T
    and tol is twice that sum.  A pair is judged only where its decision is clear (1024 u of the terms' scale):
        R^2 == 0 on either side                       +inf  (dead)
        C <= -1024 u K                                exactly 0  (in contact at the start)
        C >= 1024 u K and (A == 0 or B <= -1024 u |v| |w|)       +inf  (not approaching)
        C >= 1024 u K, B >= 1024 u |v| |w|, D <= -1024 u A K      +inf  (passing by)
        C >= 1024 u K, B >= 1024 u |v| |w|, D >= 1024 u A K       finite, within tol of T; t <= 1 as T says where |T - 1| > tol
    and at most 1 % of all pairs may be left unjudged.  The worst error seen is 0.091 of the bound (f32) and 0.066 (f64)."""
    R = np.float32 if precision == rta.RT_F32 else np.float64
    H, u = higher(precision)
    u = H(u)
    worst_all = 0.0
    for seed in SEEDS:
        items = random_nested_scene(seed)[0].astype(R)
        items[7, 3] = 0                                                          # one dead slot
        n = len(items)
        i, j = np.triu_indices(n, 1)
        for family in FAMILIES:
            what = (seed, family)
            disp = displacements(items, seed, family, R)
            t = rta.pair_impacts(items, disp, i, j).astype(H)
            it, dd = items.astype(H), disp.astype(H)
            v, w = it[j, :3] - it[i, :3], dd[i] - dd[j]
            rad = it[j, 3] + it[i, 3]
            A, B, VV = (w * w).sum(axis=1), (v * w).sum(axis=1), (v * v).sum(axis=1)
            K = VV + rad * rad
            Cc = VV - rad * rad
            D = B * B - A * Cc
            S = np.sqrt(np.abs(D))
            vw = np.sqrt(VV * A)
            with np.errstate(divide="ignore", invalid="ignore"):
                T = Cc / (B + S)
                tol = H(2.0) * u * ((H(9.0) * K + T * (H(6.0) * vw + H(16.0) * A * K / S + S + (B + S))) / (B + S) + T)
            k = H(1024.0) * u
            dead = (it[i, 3] == 0) | (it[j, 3] == 0)
            start = ~dead & (Cc <= -k * K)
            apart = ~dead & (Cc >= k * K)
            away = apart & ((A == 0) | (B <= -k * vw))
            toward = apart & (A > 0) & (B >= k * vw)
            by = toward & (D <= -k * A * K)
            front = toward & (D >= k * A * K)
            judged = dead | start | away | by | front
            assert (dead.astype(int) + start + away + by + front <= 1).all()
            worst = float(np.max(np.abs(t[front] - T[front]) / tol[front]))
            worst_all = max(worst_all, worst)
            print("%s: %d dead, %d in contact at the start, %d not approaching, %d passing by, %d in front of %d pairs, %.2f %% unjudged; "
                  "the worst error is %.3f of its bound" % (what, dead.sum(), start.sum(), away.sum(), by.sum(), front.sum(), judged.size,
                                                            100.0 * (1.0 - judged.mean()), worst))
            assert 1.0 - judged.mean() <= 0.01, what
            assert dead.any() and start.any() and away.any() and by.any() and front.any(), what
            for sel in (dead, away, by):
                assert np.isinf(t[sel]).all() and (t[sel] > 0).all(), what
            assert (t[start] == 0).all(), what
            assert np.isfinite(t[front]).all() and (t[front] > 0).all(), what
            assert (np.abs(t[front] - T[front]) <= tol[front]).all(), (what, worst)
            sure = front & (np.abs(T - 1) > tol)
            assert ((t[sure] <= 1) == (T[sure] <= 1)).all() and (t[sure] <= 1).any() and (t[sure] > 1).any(), what
    print("worst of all: %.3f of the bound" % worst_all)


class _Stand:
    """Enough of a Scene for DeviceScene's checks, which come before any call into the library."""
    def __init__(self, precision):
        self.precision = precision
        self.items = np.zeros((3, 4), np.float32 if precision == rta.RT_F32 else np.float64)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_impacts_checks_its_arguments_before_the_library(precision):
    R = np.float32 if precision == rta.RT_F32 else np.float64
    other = np.float64 if precision == rta.RT_F32 else np.float32
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h = _Stand(precision), 0, None
    good = np.zeros((3, 3), R)
    for disp in (good.astype(other), np.zeros((2, 3), R), np.zeros((3, 4), R), np.zeros(9, R), [[0.0] * 3] * 3, None, 0.0):
        with pytest.raises(ValueError, match="disp"):
            d.impacts(disp)
    for capacity in (-1, 1 << 31, 1 << 40):
        with pytest.raises(ValueError, match="capacity"):
            d.impacts(good, capacity)
    with pytest.raises((TypeError, ValueError)):
        d.impacts(good, capacity="all")
    with pytest.raises(ValueError, match="times"):
        d.impacts(good, 0, times=True)
