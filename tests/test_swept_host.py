"""Swept overlap lists (rt_swept_overlaps / rt_swept_overlaps_device, csrc/rt_swept.hpp) without a GPU: the ABI, the
argument checks made before any device is touched, the residency of the kernel's flavours read back from the code object,
rta.swept_times -- the metric's definition in numpy -- against a scalar restatement, against rta.pair_impacts, against the geometry in
higher precision and under exact scalings, the share of grazing entries the GPU suite tolerates, and the checks the Python wrapper makes
before it calls the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from rust_tracer_amd.scene import DeviceScene
from tests import scaled_scenes as ss
from tests.scenes import random_nested_scene
from tests.test_gpu_impacts import FAMILIES, SEEDS, displacements, scenes
from tests.test_gpu_overlap import queries_for
from tests.test_gpu_swept import MOTIONS, POW2, N_QUERIES, Walker, brute_cases, brute_force, placed_inputs, queries_of, scene_disp
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB
from tests.test_scales_contact_host import higher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_swept_overlaps", "rt_swept_overlaps_device")
BITS = {np.float32: np.uint32, np.float64: np.uint64}


def test_both_libraries_export_the_swept_entries_at_abi_5():
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
    assert len(capi.lib.rt_swept_overlaps_device.argtypes) == len(capi.lib.rt_swept_overlaps.argtypes) + 1 == 15
    for name in ("swept_times", "swept_normals"):
        assert callable(getattr(rta, name)) and name in rta.__all__
    assert callable(DeviceScene.swept_overlaps)


def _call(entry, scene, queries, qdisp, n, disp, exclude, order, capacity, items, time, normal, offsets, total):
    f = getattr(capi.lib, entry)
    args = (scene, queries, qdisp, n, disp, exclude, order, capacity, items, time, normal, offsets, total, None)
    return f(*args) if entry == "rt_swept_overlaps" else f(*args, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check pointers, n, the capacity and alignment -- the host entry the values too -- before they use the scene: a stand-in
    # handle will do (its precision reads RT_F32)
    stand_in = ctypes.create_string_buffer(8192)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    words = (ctypes.c_uint64 * 256)()
    at = lambda k: ctypes.c_void_p(ctypes.addressof(words) + k)
    queries, qdisp, disp, exclude, order, items, time, normal, offsets, total = (at(128 * k) for k in range(10))
    bad = capi.RT_ERR_INVALID_ARGUMENT
    message = capi.lib.rt_last_error_message
    good = dict(scene=handle, queries=queries, qdisp=qdisp, n=4, disp=disp, exclude=exclude, order=order, capacity=4, items=items, time=time, normal=normal,
                offsets=offsets, total=total)

    def refused(word, **change):
        assert _call(entry, **dict(good, **change)) == bad, (word, change)
        assert word in message(), (word, message())
    refused(b"scene", scene=None)
    refused(b"queries", queries=None)
    refused(b"qdisp", qdisp=None)
    refused(b"total_out", total=None)
    refused(b"n == 0", n=0)
    refused(b"time_out without items_out", items=None, normal=None)
    refused(b"normal_out without items_out", items=None, time=None)
    for capacity in (1 << 31, 0xFFFFFFFF):
        refused(b"capacity", capacity=capacity)
    for k in (1, 2, 3):
        for name, word, base in (("items", b"items_out", 5), ("exclude", b"exclude", 3), ("order", b"order", 4), ("queries", b"queries", 0), ("qdisp", b"qdisp", 1),
                                 ("disp", b" disp", 2), ("time", b"time_out", 6), ("normal", b"normal_out", 7)):
            refused(word, **{name: at(128 * base + k)})
    for k in (1, 4, 7):
        refused(b"offsets_out", offsets=at(128 * 8 + k))
        refused(b"total_out", total=at(128 * 9 + k))
    if entry != "rt_swept_overlaps":
        return
    # the host entry's domain, as far as it needs no scene: the queries, their displacements and the order
    f32 = lambda values: np.array(values, np.float32)
    q = f32([[0, 0, 0, 1], [1, 2, 3, 0], [4, 5, 6, 0.5], [7, 8, 9, 2]])
    dq = np.zeros((4, 3), np.float32)
    perm = np.array([2, 0, 3, 1], np.uint32)
    host = lambda **change: dict(dict(queries=q.ctypes.data, qdisp=dq.ctypes.data, disp=None, exclude=None, order=perm.ctypes.data), **change)
    for value in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        for col in range(3):
            x = q.copy()
            x[2, col] = value
            refused(b"query 2", **host(queries=x.ctypes.data))
            x = dq.copy()
            x[3, col] = value
            refused(b"qdisp of query 3", **host(qdisp=x.ctypes.data))
    for value in (np.nan, -1.0, -1e-30, np.inf, -np.inf, 2e15):
        x = q.copy()
        x[1, 3] = value
        refused(b"radius", **host(queries=x.ctypes.data))
    for values in ([0, 1, 2, 2], [0, 1, 2, 4], [1, 1, 1, 1], [0, 1, 2, 0xFFFFFFFF]):
        o = np.array(values, np.uint32)
        refused(b"order", **host(order=o.ctypes.data))


def test_the_swept_flavours_and_their_residency(tmp_path):
    # every flavour exists in both libraries, without scratch; f32 within k_query_rays's budget (eight waves per SIMD), f64 within 128
    # vector registers -- DESIGN.md 4.19's table has the counts: they are at most 64 too, so amdgpu_waves_per_eu(8) stays on all six
    want = sorted("rt::k_swept_overlaps<%s, %s>" % (t, f) for t in ("float", "double") for f in ("true, false", "false, false", "false, true"))
    pre = {"rt::k_swept_query_magnitude<float>", "rt::k_swept_query_magnitude<double>", "rt::k_impact_motion_items<float>", "rt::k_impact_motion_items<double>",
           "rt::k_impact_motion_bounds<float>", "rt::k_impact_motion_bounds<double>", "rt::k_impact_bound_radii<float>", "rt::k_impact_bound_radii<double>"}
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_swept_overlaps<")]
        assert sorted(flavours) == want, flavours
        for n in flavours:
            r = k[n]
            assert r["scratch"] == 0, (n, r)
            if "<float" in n:
                assert r["sgpr"] <= 80 and r["vgpr"] <= 64, (n, r)
            else:
                assert r["vgpr"] <= 128, (n, r)
                assert r["vgpr"] <= 64, (n, r)                                   # the attribute is kept on f64: it rests on this
        assert pre <= set(k), pre - set(k)
        for n in pre:
            assert k[n]["scratch"] == 0, (n, k[n])
        # the motion table's kernels and the scan are the impact pairs' and the contact pairs' own, not copies
        assert not [n for n in k if "swept" in n and ("scan" in n or "motion" in n or "radii" in n)]
        assert sorted(n for n in k if "scan" in n and "sort" not in n) == ["rt::k_contact_scan_offsets", "rt::k_contact_scan_spine", "rt::k_contact_scan_sums"]


def scalar_swept_time(R, query, dq, sphere, d, S, E=0.0):
    """The definition, one operation at a time on numpy scalars of type R (each rounds once) -> (t, normal or None)."""
    inf = R(np.inf)
    S, E = R(S), R(E)
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        rr = R(sphere[3] * sphere[3])
        if not rr > 0:
            return inf, None
        p = [R(query[k] * S) for k in range(3)]
        q = R(query[3] * S)
        dqs = [R(dq[k] * S) for k in range(3)]
        c = [R(sphere[k] * S) for k in range(3)]
        r = R(abs(sphere[3]) * S)
        e = [R(d[k] * S) for k in range(3)]
        v = [R(c[k] - p[k]) for k in range(3)]
        w = [R(dqs[k] - e[k]) for k in range(3)]
        rad = R(R(r + R(E * S)) + q)
        RR = R(rad * rad)
        dot = lambda a, b: R(R(R(a[0] * b[0]) + R(a[1] * b[1])) + R(a[2] * b[2]))
        qa, qb, qc = dot(w, w), dot(v, w), R(dot(v, v) - RR)
        disc = R(R(qb * qb) - R(qa * qc))
        if not qc > 0:
            t = R(0.0)
        elif not qb > 0 or disc < 0:
            return inf, None
        else:
            t = R(qc / R(qb + np.sqrt(disc)))
        u = [R(R(w[k] * t) - v[k]) for k in range(3)]
        rc = R(R(1.0) / np.sqrt(dot(u, u)))
        return t, [R(u[k] * rc) for k in range(3)]


BRANCHES = ("dead record", "q = 0", "contact at the start", "receding", "w = 0", "passing by", "impact before 1", "impact after 1")


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_swept_times_is_the_definition(R):
    inf = R(np.inf)
    U = BITS[R]
    # every branch once, with exact values: (query, its displacement, sphere, its displacement) -> t
    want = {"dead record": (([0, 0, 0, 1], [2, 0, 0], [1.5, 0, 0, 0], [9, 9, 9]), inf),
            "q = 0": (([0, 0, 0, 0], [4, 0, 0], [4, 0, 0, 1], [0, 0, 0]), R(0.75)),                      # a point: v = (4, 0, 0), w = (4, 0, 0): cc = 15, b = 16, disc = 16
            "contact at the start": (([0, 0, 0, 1], [2, 0, 0], [1.5, 0, 0, 1], [-1, 0, 0]), R(0.0)),     # centres 1.5 apart, radii 1 + 1: cc < 0
            "receding": (([1.5, 0, 0, 1], [-1, 0, 0], [4, 0, 0, 1], [0, 0, 0]), inf),                    # v = (2.5, 0, 0), w = (-1, 0, 0): b < 0
            "w = 0": (([0, 0, 0, 1], [2, 0, 0], [0, 4, 0, 1], [2, 0, 0]), inf),                          # both move by (2, 0, 0): a = b = 0
            "passing by": (([0, 0, 0, 1], [2, 0, 0], [3, 5, 0, 1], [0, 0, 0]), inf),                     # b = 6, disc = 36 - 4 * 30 < 0
            "impact before 1": (([0, 0, 0, 1], [2, 0, 0], [4, 0, 0, 1], [0, 0, 0]), R(1.0)),             # cc = 12, b = 8, disc = 64 - 48 = 16, 12 / 12
            "impact after 1": (([0, 0, 0, 1], [2, 0, 0], [10, 0, 0, 1], [-1, 0, 0]), R(96.0) / R(36.0))}  # v = (10, 0, 0), w = (3, 0, 0): cc = 96, b = 30, disc = 36
    assert tuple(want) == BRANCHES
    for name, ((query, dq, sphere, d), t) in want.items():
        qs, qd, sp, dd = (np.array([x], R) for x in (query, dq, sphere, d))
        got = rta.swept_times(qs, qd, sp, dd)
        assert got.dtype == R and got.shape == (1, 1), name
        S = rta.impact_scale(sp, dd, qs, qd)
        ref_t, ref_n = scalar_swept_time(R, qs[0], qd[0], sp[0], dd[0], S)
        assert got[0, 0] == t and got[0, 0] == ref_t, (name, got[0, 0], t)
        if name in ("q = 0", "impact before 1"):                                  # the point arrives from the left: the normal points back at it
            np.testing.assert_array_equal(rta.swept_normals(qs, qd, sp, dd)[0, 0], np.array([-1, 0, 0], R))
    standing = rta.swept_times(np.array([[0, 0, 0, 1]], R), np.array([[2, 0, 0]], R), np.array([[4, 0, 0, 1]], R))
    assert standing[0, 0] == 1 and rta.swept_times(np.array([[0, 0, 0, 1]], R), np.array([[2, 0, 0]], R), np.array([[4, 0, 0, 1]], R), None, np.array([1], R))[0, 0] == 0.5
    # S: the largest magnitude of everything given, the queries that carry one included
    assert rta.impact_scale(np.array([[1, 0, 0, 1]], R), None, np.array([[0, 0, 0, 0], [5, 0, 0, -1]], R), np.array([[0, -3, 0], [9, 9, 9]], R)) == R(0.25)
    assert rta.impact_scale(np.array([[1, 0, 0, 1]], R), None, np.array([[0, 0, 0, 0], [5, 0, 0, 0]], R), np.array([[0, -3, 0], [9, 9, 9]], R)) == R(1.0 / 16)
    # random spheres, queries and both displacement families against the scalar restatement
    it = random_nested_scene(1)[0].astype(R)
    it[5, 3] = 0                                                                 # a dead slot as the tests hold it: {.., 0}
    it[9] = 0
    it[11, 3] = R(1e-30) if R == np.float32 else R(1e-200)                       # rr rounds to 0: no positive rr
    assert R(it[11, 3] * it[11, 3]) == 0
    queries = queries_for(rta.Scene(it, rta.normalized((-1.0, -3.0, 2.0), rta.RT_F32 if R == np.float32 else rta.RT_F64), (0.0, 0.0, -4.0),
                                    precision=rta.RT_F32 if R == np.float32 else rta.RT_F64), 40)
    assert (queries[::10, 3] == 0).all()
    seen = set()
    for family in FAMILIES:
        qdisp, disp = displacements(queries, 1, family, R), displacements(it, 1, family, R)
        E = np.zeros(len(it), R)
        E[::3] = R(0.125)
        for moving, inflate in ((disp, None), (None, None), (disp, E)):
            got = rta.swept_times(queries, qdisp, it, moving, inflate)
            nrm = rta.swept_normals(queries, qdisp, it, moving, inflate)
            S = rta.impact_scale(it, moving, queries, qdisp)
            for g in range(len(queries)):
                for j in range(len(it)):
                    ref_t, ref_n = scalar_swept_time(R, queries[g], qdisp[g], it[j], (0, 0, 0) if moving is None else moving[j], S, 0.0 if inflate is None else inflate[j])
                    assert got[g, j].view(U) == ref_t.view(U), (family, g, j)
                    if ref_n is not None:
                        assert [x.view(U) for x in nrm[g, j]] == [x.view(U) for x in ref_n], (family, g, j)
                    seen.add("inf" if ref_t == inf else "0" if ref_t == 0 else "<=1" if ref_t <= 1 else ">1")
            for dead in (5, 9, 11):
                assert (got[:, dead] == inf).all()
            if inflate is not None:
                assert (got <= rta.swept_times(queries, qdisp, it, moving)).all()
    assert seen == {"inf", "0", "<=1", ">1"}, seen
    assert rta.swept_times(queries[:0], qdisp[:0], it).shape == (0, len(it)) and rta.swept_times(queries, qdisp, it[:0]).shape == (len(queries), 0)


def test_swept_times_checks_its_arguments():
    q, dq, s, d = np.zeros((3, 4), np.float32), np.zeros((3, 3), np.float32), np.zeros((5, 4), np.float32), np.zeros((5, 3), np.float32)
    for queries in (q.astype(np.float16), q[:, :3], q.reshape(-1), q.astype(np.int32)):
        with pytest.raises(ValueError, match="queries"):
            rta.swept_times(queries, dq, s, d)
    for qdisp in (dq.astype(np.float64), dq[:2], np.zeros((3, 4), np.float32)):
        with pytest.raises(ValueError, match="qdisp"):
            rta.swept_times(q, qdisp, s, d)
    for spheres in (s.astype(np.float64), s[:, :3], s.reshape(-1)):
        with pytest.raises(ValueError, match="spheres"):
            rta.swept_times(q, dq, spheres, None)
    for disp in (d.astype(np.float64), d[:4], np.zeros((5, 4), np.float32)):
        with pytest.raises(ValueError, match="disp"):
            rta.swept_times(q, dq, s, disp)
    for inflate in (np.zeros(4, np.float32), np.zeros(5, np.float64)):
        with pytest.raises(ValueError, match="inflate"):
            rta.swept_times(q, dq, s, d, inflate)
    for scale in (0.0, 3.0, -2.0, np.inf):
        with pytest.raises(ValueError, match="scale"):
            rta.swept_times(q, dq, s, d, None, scale)


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_swept_times_is_pair_impacts_with_the_query_as_the_first_sphere(R):
    U = BITS[R]
    precision = rta.RT_F32 if R == np.float32 else rta.RT_F64
    for seed in SEEDS:
        s = scenes(precision)["refit%d" % seed][0]
        items = np.ascontiguousarray(s.items.astype(R))
        m = len(items)
        for family in FAMILIES:
            queries, qdisp = queries_of(s, seed, family)
            disp = displacements(items, seed, family, R)
            n = len(queries)
            solid = queries[:, 3] > 0
            assert solid.sum() == n - n // 10
            # q > 0: pair_impacts over the concatenated records, bit for bit (one S: the same magnitudes)
            both, moves = np.concatenate([queries, items]), np.concatenate([qdisp, disp])
            assert rta.impact_scale(both[np.concatenate([solid, np.ones(m, bool)])], moves[np.concatenate([solid, np.ones(m, bool)])]) == \
                rta.impact_scale(items, disp, queries[solid], qdisp[solid])
            got = rta.swept_times(queries[solid], qdisp[solid], items, disp)
            gi, gj = np.meshgrid(np.flatnonzero(solid), n + np.arange(m), indexing="ij")
            S = rta.impact_scale(items, disp, queries[solid], qdisp[solid])
            ref = rta.pair_impacts(both, moves, gi.reshape(-1), gj.reshape(-1), scale=S).reshape(got.shape)
            np.testing.assert_array_equal(got.view(U), ref.view(U), err_msg=str((seed, family)))
            assert (got <= 1).any() and (got > 1).any()
            # a point is no sphere to pair_impacts, and a query here
            pi, pj = np.meshgrid(np.flatnonzero(~solid), n + np.arange(m), indexing="ij")
            assert np.isinf(rta.pair_impacts(both, moves, pi.reshape(-1), pj.reshape(-1))).all()
            # the scene's own spheres and displacements as the queries: a symmetric matrix, in its bits (negation is exact, the radius sum commutes)
            own = rta.swept_times(items, disp, items, disp)
            np.testing.assert_array_equal(own.view(U), own.T.copy().view(U), err_msg=str((seed, family)))
            i, j = np.triu_indices(m, 1)
            np.testing.assert_array_equal(own[i, j].view(U), rta.pair_impacts(items, disp, i, j).view(U), err_msg=str((seed, family)))


def judge(t, queries, qdisp, items, disp, H, u):
    """The decisions, the bound and the unjudged share of tests/test_impacts_host.py
    test_pair_impacts_is_the_time_two_moving_spheres_first_touch (its docstring derives them; they sit in its body and are restated here
    line for line), with the query in the place of sphere i, for the matrix t of every (query, item) -> (classes dict, T, tol, judged)."""
    qs, qd, it, dd = (x.astype(H) for x in (queries, qdisp, items, disp))
    v, w = it[None, :, :3] - qs[:, None, :3], qd[:, None, :] - dd[None, :, :]
    rad = it[None, :, 3] + qs[:, None, 3]
    A, B, VV = (w * w).sum(axis=2), (v * w).sum(axis=2), (v * v).sum(axis=2)
    K = VV + rad * rad
    Cc = VV - rad * rad
    D = B * B - A * Cc
    S = np.sqrt(np.abs(D))
    vw = np.sqrt(VV * A)
    with np.errstate(divide="ignore", invalid="ignore"):
        T = Cc / (B + S)
        tol = H(2.0) * u * ((H(9.0) * K + T * (H(6.0) * vw + H(16.0) * A * K / S + S + (B + S))) / (B + S) + T)
    k = H(1024.0) * u
    dead = np.broadcast_to(it[None, :, 3] == 0, T.shape)
    start = ~dead & (Cc <= -k * K)
    apart = ~dead & (Cc >= k * K)
    away = apart & ((A == 0) | (B <= -k * vw))
    toward = apart & (A > 0) & (B >= k * vw)
    by = toward & (D <= -k * A * K)
    front = toward & (D >= k * A * K)
    judged = dead | start | away | by | front
    assert (dead.astype(int) + start + away + by + front <= 1).all()
    return {"dead": dead, "start": start, "away": away, "by": by, "front": front}, T, tol, judged


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_swept_times_is_the_time_a_moving_query_first_touches_a_moving_sphere(precision):
    """Every (query, item) of random_nested_scene(0 .. 3) under 80 queries drawn as tests/test_gpu_overlap.py queries_for draws them, with
    both displacement families for the queries and for the scene, against the geometry in higher precision H (float64 for f32,
    np.longdouble for f64) from the REAL inputs.  The four decisions are asserted wherever they are clear, |t - T| is held within the
    bound tests/test_impacts_host.py derives, and at most 1 % of the pairs may be left unjudged."""
    R = np.float32 if precision == rta.RT_F32 else np.float64
    H, u = higher(precision)
    u = H(u)
    worst_all = 0.0
    for seed in SEEDS:
        items = random_nested_scene(seed)[0].astype(R)
        items[7, 3] = 0                                                          # one dead slot
        s = rta.Scene(items, rta.normalized((-1.0, -3.0, 2.0), precision), (0.0, 0.0, -4.0), precision=precision)
        for family in FAMILIES:
            what = (seed, family)
            queries = queries_for(s, N_QUERIES, 77 + seed)
            qdisp, disp = displacements(queries, seed, family, R), displacements(items, seed, family, R)
            t = rta.swept_times(queries, qdisp, items, disp).astype(H)
            cls, T, tol, judged = judge(t, queries, qdisp, items, disp, H, u)
            dead, start, away, by, front = (cls[k] for k in ("dead", "start", "away", "by", "front"))
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


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_the_grazing_share_of_the_gpu_comparison_stays_under_its_cap(precision):
    """check_brute of tests/test_gpu_swept.py compares the walk with brute force away from grazing entries and lets at most 5 % of the listed
    entries graze.  Here, with numpy alone, that cap holds for every scene and motion it runs on -- and the walker, which the GPU must
    restate bit for bit, already agrees with brute force there."""
    R = np.float32 if precision == rta.RT_F32 else np.float64
    U = BITS[R]
    for name, s, seed in brute_cases(precision):
        w = Walker(s)
        m = len(s.items)
        for qfam, sfam in MOTIONS:
            what = (name, qfam, sfam)
            queries, qdisp = queries_of(s, seed, qfam)
            disp = scene_disp(s, seed, sfam)
            t, grazing = brute_force(queries, qdisp, s.items, disp, R)
            listed = t <= 1
            share = (listed & grazing).sum() / max(listed.sum(), 1)
            assert listed.any() and share <= 0.05, (what, share)
            if name.startswith("refit") and seed > 1:
                continue
            items, times, normals, offsets, st = w.all(queries, qdisp, disp)
            rows = np.repeat(np.arange(len(queries)), np.diff(offsets.astype(np.int64)))
            keep = ~grazing[rows, items]
            gi, gj = np.nonzero(listed & ~grazing)
            np.testing.assert_array_equal((rows * m + items)[keep], gi * m + gj, err_msg=str(what))
            np.testing.assert_array_equal(times[keep].view(U), t[listed & ~grazing].view(U), err_msg=str(what))


def scaled(arrays, k, R):
    """(queries, qdisp, items, disp) times 2^k, and whether that is a scaling of the inputs: every product exact and a normal number, and
    every item alive that was -- r * r, which the stream holds and which decides that, may not underflow to 0."""
    out = [None if a is None else np.ascontiguousarray(np.ldexp(a, k).astype(R)) for a in arrays]
    exact = all(a is None or (np.isfinite(b).all() and (np.ldexp(b, -k) == a).all() and (np.abs(b[b != 0]) >= np.finfo(R).tiny).all()) for a, b in zip(arrays, out))
    with np.errstate(under="ignore", over="ignore"):
        alive = ((out[2][:, 3] * out[2][:, 3] > 0) == (arrays[2][:, 3] * arrays[2][:, 3] > 0)).all()
    return out, exact and bool(alive)


@pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)
def test_an_exact_scaling_keeps_every_bit_of_every_time_and_normal(param):
    """The time has no dimension and the normal is a direction: the placed scenes of tests/scaled_scenes.py with their queries and both
    displacement families, times 2^-66, 2^-40, 2^33 and 2^45, keep every bit of swept_times and swept_normals -- wherever the product is
    exact: a factor that takes an input of a placement out of the normal range of REAL is not a scaling of that placement (f32 at 1e-20
    times 2^-66 is 1e-40) and is left out, and every factor is used by some placement."""
    precision, placement = param
    R = np.float32 if precision == rta.RT_F32 else np.float64
    U = BITS[R]
    used = set()
    for c in ss.case(precision, placement)[:2]:
        items = np.ascontiguousarray(c.scene.items.astype(R))
        for family in FAMILIES:
            queries, qdisp, disp = placed_inputs(c, family)
            for moving in (disp, None):
                ref_t = rta.swept_times(queries, qdisp, items, moving)
                ref_n = rta.swept_normals(queries, qdisp, items, moving)
                assert (ref_t == 0).any() and ((ref_t > 0) & (ref_t <= 1)).any() and np.isinf(ref_t).any(), (c.name, family)
                for k in POW2:
                    (q2, qd2, it2, d2), exact = scaled((queries, qdisp, items, moving), k, R)
                    if not exact:
                        continue
                    used.add(k)
                    got_t, got_n = rta.swept_times(q2, qd2, it2, d2), rta.swept_normals(q2, qd2, it2, d2)
                    np.testing.assert_array_equal(got_t.view(U), ref_t.view(U), err_msg=str((c.name, family, k)))
                    hit = np.isfinite(ref_t)
                    np.testing.assert_array_equal(got_n[hit].view(U), ref_n[hit].view(U), err_msg=str((c.name, family, k)))
    assert used, param
    if placement in ("x1", "+3e3", "+3e9"):
        assert used == set(POW2), (param, used)


class _Stand:
    """Enough of a Scene for DeviceScene's checks, which come before any call into the library."""
    def __init__(self, precision):
        self.precision = precision
        self.items = np.zeros((3, 4), np.float32 if precision == rta.RT_F32 else np.float64)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_swept_overlaps_checks_its_arguments_before_the_library(precision):
    R = np.float32 if precision == rta.RT_F32 else np.float64
    other = np.float64 if precision == rta.RT_F32 else np.float32
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h = _Stand(precision), 0, None
    q, dq, disp = np.zeros((5, 4), R), np.zeros((5, 3), R), np.zeros((3, 3), R)
    for queries in (q.astype(other), q[:, :3], q[:0], q.reshape(-1), None):
        with pytest.raises(ValueError, match="queries"):
            d.swept_overlaps(queries, dq)
    for qdisp in (dq.astype(other), dq[:4], np.zeros((5, 4), R), None, 0.0):
        with pytest.raises(ValueError, match="qdisp"):
            d.swept_overlaps(q, qdisp)
    for bad in (disp.astype(other), np.zeros((5, 3), R), np.zeros((3, 4), R), 0.0):
        with pytest.raises(ValueError, match="disp"):
            d.swept_overlaps(q, dq, bad)
    for exclude in (np.zeros(5, np.int64), np.zeros(4, np.int32)):
        with pytest.raises(ValueError, match="exclude"):
            d.swept_overlaps(q, dq, exclude=exclude)
    for order in (np.zeros(4, np.uint32), np.zeros(5, np.float32), np.full(5, -1)):
        with pytest.raises(ValueError, match="order"):
            d.swept_overlaps(q, dq, order=order)
    for capacity in (-1, 1 << 31, 1 << 40):
        with pytest.raises(ValueError, match="capacity"):
            d.swept_overlaps(q, dq, capacity=capacity)
    for kw in (dict(times=True), dict(normals=True)):
        with pytest.raises(ValueError, match="times and normals"):
            d.swept_overlaps(q, dq, capacity=0, **kw)
