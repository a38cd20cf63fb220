"""Live and dead slots on the GPU (rt_scene_update_live* / rt_scene_rebuild_n* / rt_scene_live, csrc/rt_dynamic.hpp).

The yardstick is tests/test_gpu_dynamic.py's, extended.  A STAND-IN scene is made by rt_scene_create from all n_items slots and the same
ranges: each dead slot holds a dummy sphere {0, 1000 + slot, 0, 1e-3}, and the bounds are rt_scene_bounds' output with each {0, 0, 0, 0}
-- a dead group -- replaced by the dummy of the group's first slot.  Every ray here starts below y = 3 and points down (dir.y <= -0.2;
the camera looks down as well), so it cannot reach y ~ 1000; the shadow rays of trace and render_camera go up, along -light, and pass the
column of dummies more than 300 units away.  Every dummy and every dummy bound is therefore missed by every ray, as the dead records are:
the stand-in makes the same tests, and the dynamic scene must write its bytes and counters.  The same stand-in is also run through the CPU
oracle, ray by ray, and the test first asserts from the oracle's answers that no result lies on a dummy -- a condition on the inputs, for
every ray.  Every check is bit equality.

The scene: 600 random spheres in [-1, 1]^3 under rt_balanced_ranges(600, 4) -- the root has three 256-item work records, and its two
children (300 items each) straddle the record edge at slot 256 -- plus the level-2 pyramid (5 items, one group) under its own ranges."""
import ctypes as C

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.test_gpu_camera import camera_sample_rays
from tests.test_gpu_dynamic import COUNTERS, EYE, LIGHT, PREC, PRECISIONS, REAL, as_bits, assert_same, counters, scene_of

pytestmark = pytest.mark.gpu

N, LEAF, N_RAYS = 600, 4, 4096
OPTS, REGIONS = (96, 64, 1), [(0, 64, 56, 0), (56, 64, 96, 24), (56, 24, 96, 0)]
CAM_EYE = (0.0, 3.0, -4.0)


def spheres_of(precision):
    rng = np.random.default_rng(600)
    return np.ascontiguousarray(np.concatenate([rng.uniform(-1, 1, (N, 3)), rng.uniform(0.03, 0.12, (N, 1))], axis=1).astype(REAL[precision]))


def rays_of(precision):
    """4,096 rays from y in [1.5, 3] aimed into the lower part of the box: dir.y <= -0.2; a quarter of them with a finite tmax."""
    rng = np.random.default_rng(77)
    pos = np.stack([rng.uniform(-1, 1, N_RAYS), rng.uniform(1.5, 3.0, N_RAYS), rng.uniform(-1, 1, N_RAYS)], axis=1)
    to = np.stack([rng.uniform(-1, 1, N_RAYS), rng.uniform(-1, 0.5, N_RAYS), rng.uniform(-1, 1, N_RAYS)], axis=1)
    d = to - pos
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    rays = np.ascontiguousarray(np.concatenate([pos, d], axis=1).astype(REAL[precision]))
    tmax = np.full(N_RAYS, np.inf, dtype=REAL[precision])
    tmax[::4] = 2.75
    assert (rays[:, 1] < 3.0 + 1e-6).all() and (rays[:, 4] <= -0.2).all()
    return rays, tmax


def camera_of(precision):
    cam = rta.look_at(CAM_EYE, (0.0, 0.0, 0.0), precision=precision)
    ys, xs = np.meshgrid(np.arange(OPTS[1]), np.arange(OPTS[0]), indexing="ij")
    rays = camera_sample_rays(OPTS[0], OPTS[1], 1, xs.ravel(), ys.ravel(), 0, 0, cam, REAL[precision])
    assert (rays[:, 4] <= -0.2).all() and (rays[:, 1] == 3.0).all()             # every camera ray points down
    return cam


def dummies(n, R):
    return np.stack([np.zeros(n), 1000.0 + np.arange(n), np.zeros(n), np.full(n, 1e-3)], axis=1).astype(R)


def stand_in_arrays(items, live, ranges, reported_bounds, R, dummy=None):
    """(items, bounds) of the stand-in scene.  dummy: one sphere {cx, cy, cz, r} that stands in for every dead slot (None: the column of
    dummies(), for a scene of unit size around the origin)."""
    dm = dummies(len(items), R) if dummy is None else np.tile(np.asarray(dummy, dtype=R).reshape(1, 4), (len(items), 1))
    it = np.where((np.asarray(live) != 0)[:, None], items, dm).astype(R)
    it = np.ascontiguousarray(it)
    bd = None
    if reported_bounds is not None:
        bd = np.array(reported_bounds, dtype=R)
        dead = ~as_bits(bd).reshape(len(bd), -1).any(axis=1)
        bd[dead] = dm[np.asarray(ranges)[dead, 0]]
    return it, bd


def answers(d, rays, tmax, cam):
    """[(entry, bytes of every result, counters)] of the general-ray entries on device scene d, and every item index they wrote."""
    out, slots = [], []

    def put(name, res, item_at=None):
        *arrays, st = res
        out.append((name, [as_bits(a) for a in arrays], counters(st)))
        if item_at is not None:
            slots.append(np.asarray(arrays[item_at]).reshape(-1))

    for any_hit in (False, True):
        put("intersect any=%d" % any_hit, d.intersect(rays, tmax, any_hit=any_hit, want_stats=True), 2)
    put("intersect ordered", d.intersect(rays, tmax, want_stats=True, order=True), 2)
    for all_hits in (False, True):
        put("multi all=%d" % all_hits, d.intersect_multi(rays, 4, tmax, all_hits=all_hits, want_stats=True), 2)
    put("multi ordered", d.intersect_multi(rays, 4, tmax, want_stats=True, order=True), 2)
    put("trace", d.trace(rays, want_stats=True))
    put("trace ordered", d.trace(rays, want_stats=True, order=True))
    put("camera", d.render_camera(OPTS, cam, REGIONS, want_stats=True))
    buf, st = d.render_camera_undersampled(OPTS, cam, REGIONS, 2)
    put("undersampled step 2", (buf.copy(), st))
    buf, st = d.render_camera_undersampled(OPTS, cam, REGIONS, 1, prev_step=2, out=buf)
    put("undersampled step 1", (buf.copy(), st))
    return out, np.concatenate(slots)


_STAND_IN = {}


def stand_in_answers(items, live, ranges, reported_bounds, precision, rays, tmax, cam, key=None):
    """The stand-in's answers; with ranges, after the oracle has said that none of them lies on a dummy.  Made once per key."""
    if key is not None and (key, precision) in _STAND_IN:
        return _STAND_IN[key, precision]
    R = REAL[precision]
    it, bd = stand_in_arrays(items, live, ranges, reported_bounds, R)
    sdir = -np.asarray(rta.normalized(LIGHT, precision), dtype=np.float64)
    assert sdir[1] > 0 and (1000.0 - 3.0) * abs(sdir[0]) / sdir[1] > 300.0          # the shadow rays pass the dummies' column far away
    s = rta.DeviceScene(scene_of(it, bd, ranges, precision))
    try:
        ref, slots = answers(s, rays, tmax, cam)
        near = s.intersect(rays, tmax)
    finally:
        s.close()
    dead = np.flatnonzero(np.asarray(live) == 0)
    assert not np.isin(slots[slots >= 0], dead).any()
    if bd is not None and tuple(np.asarray(ranges)[0]) == (0, len(it)):
        o = oracle.Scene.from_ranges(it.astype(np.float64), bd.astype(np.float64), ranges, LIGHT, EYE, PREC[precision])
        for k in range(len(rays)):                                   # all of them, none left out
            dist, _ = o.intersect(rays[k].astype(np.float64), float(tmax[k]), oracle.MODE_HIERARCHY)
            assert R(dist) == near[0][k] or (np.isnan(dist) and np.isnan(near[0][k])), (k, dist, near[0][k])
            if dist < float(tmax[k]):
                assert float(rays[k, 1]) + dist * float(rays[k, 4]) < 10.0, (k, dist)       # the hit lies in the box, not at y ~ 1000
    if key is not None:
        _STAND_IN[key, precision] = ref
    return ref


def check(d, items, live, ranges, precision, rays, tmax, cam, what, callers_bounds=None, key=None):
    """Everything a liveness pattern checks of dynamic scene d, which was just given `items` with `live`."""
    live = (np.asarray(live) != 0).astype(np.uint8)
    np.testing.assert_array_equal(d.live(), live, err_msg=what)
    bd = None
    if ranges is not None:
        bd = d.bounds()
        with np.errstate(all="ignore"):
            want = callers_bounds if callers_bounds is not None else rta.refit_bounds(items, ranges, precision, live=live)
        np.testing.assert_array_equal(as_bits(bd), as_bits(want), err_msg=what)
    ref = stand_in_answers(items, live, ranges, bd, precision, rays, tmax, cam, key)
    got, slots = answers(d, rays, tmax, cam)
    assert_same(got, ref, what)
    assert not np.isin(slots[slots >= 0], np.flatnonzero(live == 0)).any(), what
    return got


def patterns(n, ranges):
    """(name, live uint8[n]) -- the liveness patterns of the 600-sphere scene, or those that exist at n = 5."""
    one = lambda v, at: np.where(np.isin(np.arange(n), at), v, 1 - v).astype(np.uint8)
    out = [("all live", np.ones(n, dtype=np.uint8)), ("all dead", np.zeros(n, dtype=np.uint8)), ("one live", one(1, [n // 2 + 1])), ("one dead", one(0, [n // 2 + 1]))]
    if n == N:
        leaf = next(g for g in range(len(ranges)) if ranges[g, 1] <= LEAF and ranges[g, 0] > 256)
        out.append(("a leaf group dead", one(0, np.arange(ranges[leaf, 0], ranges[leaf, 0] + ranges[leaf, 1]))))
        out.append(("a work record of the root dead", one(0, np.arange(256, 512))))
        out.append(("slots 255 / 256 / 257 dead", one(0, [255, 256, 257])))
        out.append(("random half", (np.random.default_rng(50).random(n) < 0.5).astype(np.uint8)))
    return out


def setup(precision):
    s, rg = spheres_of(precision), rta.balanced_ranges(N, LEAF)
    rays, tmax = rays_of(precision)
    return s, rg, rays, tmax, camera_of(precision)


# ---- 1: the liveness patterns ----

@PRECISIONS
def test_every_liveness_pattern_answers_as_its_stand_in(precision):
    s, rg, rays, tmax, cam = setup(precision)
    assert (rg[0] == (0, N)).all() and (rg[1] == (0, 300)).all() and (rg[:, 0] == 300).any()      # three work records; children across slot 256
    d = rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)
    np.testing.assert_array_equal(d.live(), np.ones(N, dtype=np.uint8))                 # as created
    np.testing.assert_array_equal(rta.DeviceScene(scene_of(s, rta.refit_bounds(s, rg, precision), rg, precision)).live(), np.ones(N, dtype=np.uint8))
    seen = {}
    for name, live in patterns(N, rg):
        d.update(s, live=live)
        got = check(d, s, live, rg, precision, rays, tmax, cam, name, key=name)
        seen[name] = got
        bd = d.bounds()
        dead_groups = ~as_bits(bd).reshape(len(bd), -1).any(axis=1)
        np.testing.assert_array_equal(dead_groups, np.array([not live[f:f + c].any() for f, c in rg]), err_msg=name)
    # all dead: every ray misses at the cost of one bound test
    for name, arrays, c in seen["all dead"]:
        c = dict(zip(COUNTERS, c))
        assert c["hits"] == 0 and c["sphere_tests"] == 0 and c["bound_tests"] == c["primary"] and c["shadow"] == 0, (name, c)
    assert any(dict(zip(COUNTERS, c))["hits"] for _, _, c in seen["random half"]) and any(dict(zip(COUNTERS, c))["occluded"] for _, _, c in seen["all live"])
    d.close()


@PRECISIONS
def test_the_level_2_pyramid_with_its_own_ranges(precision):
    it, bd0, rg = rta.pyramid(2, (0.0, -1.0, 0.0), 1.0, precision)
    rays, tmax = rays_of(precision)
    cam = camera_of(precision)
    for bounds in (None, bd0):                                       # created with refit bounds / with its own
        d = rta.DeviceScene(scene_of(it, bounds, rg, precision), dynamic=True)
        for name, live in patterns(len(it), rg):
            d.update(it, live=live)
            check(d, it, live, rg, precision, rays, tmax, cam, "pyramid: " + name, key=("pyramid", name))
        d.close()


# ---- 2: a sphere dies ----

@PRECISIONS
def test_a_killed_sphere_is_no_longer_hit(precision):
    R = REAL[precision]
    s, rg, rays, tmax, cam = setup(precision)
    d = rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)
    first = d.intersect(rays, None)[2]
    aimed = rays[first >= 0].copy()
    to = s[first[first >= 0], :3].astype(np.float64) - aimed[:, :3]
    aimed[:, 3:] = (to / np.sqrt((to * to).sum(axis=1))[:, None]).astype(R)
    down = aimed[:, 4] <= -0.2
    aimed, target = np.ascontiguousarray(aimed[down]), first[first >= 0][down]
    assert len(aimed) > 100
    seen = d.intersect(aimed, None)[2]
    k = int(np.flatnonzero(seen == target)[0])                       # a ray that is reported the sphere it is aimed at
    victim = int(seen[k])
    live = np.ones(N, dtype=np.uint8)
    live[victim] = 0
    d.update(s, live=live)
    dist, nrm, item = d.intersect(aimed, None)
    assert item[k] != victim and not (item == victim).any()
    it, bd = stand_in_arrays(s, live, rg, d.bounds(), R)
    ref = rta.DeviceScene(scene_of(it, bd, rg, precision))
    for a, b in zip((dist, nrm, item), ref.intersect(aimed, None)):
        np.testing.assert_array_equal(as_bits(a), as_bits(b))
    ref.close(); d.close()


# ---- 3: the update forms ----

@PRECISIONS
def test_the_callers_bounds_with_dead_items(precision):
    R = REAL[precision]
    s, rg, rays, tmax, cam = setup(precision)
    live = patterns(N, rg)[-1][1]
    d = rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)
    mine = rta.refit_bounds(s, rg, precision)                        # of ALL items: every one is written as given, none is {0, 0, 0, 0}
    mine[:, 3] *= R(1.125)
    d.update(s, mine, live=live)
    check(d, s, live, rg, precision, rays, tmax, cam, "caller's bounds", callers_bounds=mine)
    d.update(s, live=live)                                           # ... and a refit behind it replaces every one of them
    np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(rta.refit_bounds(s, rg, precision, live=live)))
    bad = mine.copy()
    bad[3, 0] = np.nan                                               # validated as today
    assert capi.lib.rt_scene_update_live(d._h, s.ctypes.data, bad.ctypes.data, live.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    d.close()


@PRECISIONS
def test_a_flat_dynamic_scene_takes_liveness(precision):
    s, _, rays, tmax, cam = setup(precision)
    s = np.ascontiguousarray(s[:97])
    d = rta.DeviceScene(scene_of(s, None, None, precision), dynamic=True)
    for name, live in (("random half", (np.random.default_rng(4).random(97) < 0.5).astype(np.uint8)), ("all dead", np.zeros(97, dtype=np.uint8))):
        d.update(s, live=live)
        check(d, s, live, None, precision, rays, tmax, cam, "flat: " + name)
    d.update(s)
    np.testing.assert_array_equal(d.live(), np.ones(97, dtype=np.uint8))
    d.close()


@PRECISIONS
def test_nan_in_every_dead_slot_changes_nothing_and_a_plain_update_revives_every_slot(precision):
    import torch
    R = REAL[precision]
    s, rg, rays, tmax, cam = setup(precision)
    name, live = patterns(N, rg)[-1]
    poisoned = s.copy()
    poisoned[live == 0] = R(np.nan)
    d = rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)
    d.update(poisoned, live=live)                                    # the host entry: only live items are validated
    check(d, s, live, rg, precision, rays, tmax, cam, "NaN in dead slots, host", key=name)
    d.update(s)                                                      # every slot is live again
    plain = check(d, s, np.ones(N, dtype=np.uint8), rg, precision, rays, tmax, cam, "a plain update behind a live one", key="all live")
    np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(rta.refit_bounds(s, rg, precision)))
    d.update(torch.from_numpy(poisoned).cuda(), live=torch.from_numpy(live).cuda())      # the device entry
    torch.cuda.current_stream().synchronize()
    check(d, s, live, rg, precision, rays, tmax, cam, "NaN in dead slots, device", key=name)
    d.update(torch.from_numpy(poisoned).cuda(), live=torch.from_numpy(live != 0).cuda())      # a bool tensor is the same bytes
    torch.cuda.current_stream().synchronize()
    np.testing.assert_array_equal(d.live(), live)
    d.rebuild(s)                                                     # a rebuild makes every slot live as well
    np.testing.assert_array_equal(d.live(), np.ones(N, dtype=np.uint8))
    fresh = rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)
    assert_same(plain, answers(fresh, rays, tmax, cam)[0], "against a scene that never had a dead slot")
    fresh.close(); d.close()


@PRECISIONS
def test_a_device_live_update_orders_the_queries_behind_it_on_its_stream(precision):
    import torch
    s, rg, rays, tmax, cam = setup(precision)
    nbytes = sum((r - l) * (t - b) for l, t, r, b in REGIONS) * 4
    host = rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)
    dev = rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    trays, ttmax, ts = torch.from_numpy(rays).cuda(), torch.from_numpy(tmax).cuda(), torch.from_numpy(s).cuda()
    for name, live in patterns(N, rg)[4:]:
        host.update(s, live=live)
        frame_ref, _ = host.render_camera(OPTS, cam, REGIONS, want_stats=False)
        near_ref = host.intersect(rays, tmax)
        frame = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        dev.update(ts, live=torch.from_numpy(live).cuda(), stream=side)
        dev.render_camera_device(OPTS, cam, REGIONS, frame.data_ptr(), stream=side.cuda_stream)      # no synchronisation in between
        near = dev.intersect(trays, ttmax, stream=side)
        side.synchronize()
        np.testing.assert_array_equal(frame.cpu().numpy(), frame_ref, err_msg=name)
        for a, b in zip(near_ref, near):
            np.testing.assert_array_equal(as_bits(a), as_bits(b.cpu().numpy()), err_msg=name)
        np.testing.assert_array_equal(as_bits(dev.bounds()), as_bits(host.bounds()))
        np.testing.assert_array_equal(dev.live(), live)
    # a raw pointer for the liveness bytes, NULL for "every slot": exactly rt_scene_update_device
    tl = torch.from_numpy(patterns(N, rg)[-1][1]).cuda()
    torch.cuda.current_stream().synchronize()
    dev.update(int(ts.data_ptr()), live=int(tl.data_ptr()), stream=side.cuda_stream)
    np.testing.assert_array_equal(dev.live(), tl.cpu().numpy())      # (rt_scene_live waits for the update)
    capi.check(capi.lib.rt_scene_update_live_device(dev._h, C.c_void_p(ts.data_ptr()), None, None, C.c_void_p(side.cuda_stream)), "rt_scene_update_live_device")
    np.testing.assert_array_equal(dev.live(), np.ones(N, dtype=np.uint8))
    np.testing.assert_array_equal(as_bits(dev.bounds()), as_bits(rta.refit_bounds(s, rg, precision)))
    host.close(); dev.close()


# ---- 4: rebuilds of n ----

@PRECISIONS
@pytest.mark.parametrize("n", [0, 1, 2, 299, 599, 600])
def test_a_rebuild_of_n_is_the_live_update_of_the_sorted_prefix(n, precision):
    import torch
    s, rg, rays, tmax, cam = setup(precision)
    caller = np.ascontiguousarray(s[np.random.default_rng(11).permutation(N)])          # a seeded random order
    order = np.argsort(rta.sphere_keys(caller[:n]), kind="stable").astype(np.uint32) if n else np.zeros(0, dtype=np.uint32)
    x = caller.copy()
    x[:n] = caller[:n][order]
    live = (np.arange(N) < n).astype(np.uint8)
    a = rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)
    b = rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)
    got_order = a.rebuild(caller, n=n)
    assert got_order.dtype == np.uint32 and got_order.shape == (n,)
    np.testing.assert_array_equal(got_order, order)
    b.update(x, live=live)
    np.testing.assert_array_equal(as_bits(a.bounds()), as_bits(b.bounds()))
    ref = check(b, x, live, rg, precision, rays, tmax, cam, "update of the sorted prefix, n = %d" % n)
    got, slots = answers(a, rays, tmax, cam)
    assert_same(got, ref, "rebuild_n against the live update, n = %d" % n)
    assert (slots < n).all()
    np.testing.assert_array_equal(a.live(), live)
    if n == 0:                                                       # an empty scene: every query misses, one bound test per ray
        for name, arrays, c in got:
            c = dict(zip(COUNTERS, c))
            assert c["hits"] == 0 and c["sphere_tests"] == 0 and c["bound_tests"] == c["primary"], (name, c)
        assert (a.intersect(rays, tmax)[2] == -1).all()
        capi.check(capi.lib.rt_scene_rebuild_n(a._h, None, 0, None), "rt_scene_rebuild_n")      # spheres may be NULL
    if n == N:                                                       # rt_scene_rebuild, byte for byte
        np.testing.assert_array_equal(b.rebuild(caller), order)
        np.testing.assert_array_equal(as_bits(a.bounds()), as_bits(b.bounds()))
        assert_same(got, answers(b, rays, tmax, cam)[0], "rebuild_n(600) against rebuild")
    # over the balanced ranges everything to the right of the live prefix is dead groups
    bd = a.bounds()
    dead_groups = ~as_bits(bd).reshape(len(bd), -1).any(axis=1)
    np.testing.assert_array_equal(dead_groups, rg[:, 0] >= n)
    # the device form, on a side stream, with the queries behind it
    side = torch.cuda.Stream()
    dev = rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)
    torder = dev.rebuild(torch.from_numpy(caller).cuda(), stream=side, n=n)
    near = dev.intersect(torch.from_numpy(rays).cuda(), torch.from_numpy(tmax).cuda(), stream=side)
    side.synchronize()
    np.testing.assert_array_equal(torder.cpu().numpy().view(np.uint32), order)
    for p, q in zip(a.intersect(rays, tmax), near):
        np.testing.assert_array_equal(as_bits(p), as_bits(q.cpu().numpy()))
    np.testing.assert_array_equal(as_bits(dev.bounds()), as_bits(a.bounds()))
    np.testing.assert_array_equal(dev.live(), live)
    if n == 0:                                                       # a tensor without rows still takes the device entry, on its stream
        dev.update(torch.from_numpy(s).cuda(), stream=side)
        empty = torch.empty((0, 4), dtype=torch.float32 if precision == rta.RT_F32 else torch.float64, device="cuda")
        assert dev.rebuild(empty, stream=side, n=0).is_cuda
        np.testing.assert_array_equal(dev.live(), live)
    a.close(); b.close(); dev.close()


# ---- 5: status codes ----

def test_status_codes_and_a_refused_call_leaves_the_scene_alone():
    import torch
    precision = rta.RT_F32
    s, rg, rays, tmax, cam = setup(precision)
    live = patterns(N, rg)[-1][1]
    d = rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)
    d.update(s, live=live)
    before, _ = answers(d, rays, tmax, cam)
    bounds_before = d.bounds()
    dbuf = torch.zeros(N * 16 + 64, dtype=torch.uint8, device="cuda")
    order = np.zeros(N + 1, dtype=np.uint32)
    lib = capi.lib
    # a static scene: no liveness to set, all ones to report
    static = rta.DeviceScene(scene_of(s, rta.refit_bounds(s, rg, precision), rg, precision))
    assert lib.rt_scene_update_live(static._h, s.ctypes.data, None, live.ctypes.data) == capi.RT_ERR_UNSUPPORTED
    assert lib.rt_scene_update_live_device(static._h, C.c_void_p(dbuf.data_ptr()), None, C.c_void_p(dbuf.data_ptr()), None) == capi.RT_ERR_UNSUPPORTED
    assert lib.rt_scene_rebuild_n(static._h, s.ctypes.data, 10, None) == capi.RT_ERR_UNSUPPORTED
    assert lib.rt_scene_rebuild_n_device(static._h, C.c_void_p(dbuf.data_ptr()), 10, None, None) == capi.RT_ERR_UNSUPPORTED
    np.testing.assert_array_equal(static.live(), np.ones(N, dtype=np.uint8))
    # a flat dynamic scene takes liveness but no rebuild
    flat = rta.DeviceScene(scene_of(s, None, None, precision), dynamic=True)
    assert lib.rt_scene_rebuild_n(flat._h, s.ctypes.data, 10, None) == capi.RT_ERR_UNSUPPORTED
    assert lib.rt_scene_rebuild_n_device(flat._h, C.c_void_p(dbuf.data_ptr()), 10, None, None) == capi.RT_ERR_UNSUPPORTED
    assert lib.rt_scene_update_live(flat._h, s.ctypes.data, None, live.ctypes.data) == capi.RT_OK
    # arguments
    assert lib.rt_scene_rebuild_n(d._h, s.ctypes.data, N + 1, order.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_scene_rebuild_n_device(d._h, C.c_void_p(dbuf.data_ptr()), N + 1, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_scene_rebuild_n(d._h, None, 1, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_scene_rebuild_n_device(d._h, None, 1, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_scene_rebuild_n_device(d._h, C.c_void_p(dbuf.data_ptr() + 4), 1, None, None) == capi.RT_ERR_INVALID_ARGUMENT         # misaligned
    assert lib.rt_scene_update_live_device(d._h, C.c_void_p(dbuf.data_ptr() + 4), None, C.c_void_p(dbuf.data_ptr()), None) == capi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_scene_update_live(d._h, None, None, live.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_scene_live(d._h, None) == capi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(rta.RtError):
        d.rebuild(s, n=N + 1)
    with pytest.raises(ValueError):
        d.update(s, live=np.ones(N - 1, dtype=np.uint8))
    # values: a live item outside the domain is refused, the same bits in a dead slot are not looked at
    at_live, at_dead = int(np.flatnonzero(live)[7]), int(np.flatnonzero(live == 0)[7])
    for col, v in ((3, 0.0), (3, -1.0), (0, np.nan), (1, np.inf), (2, 2e15)):
        broken = s.copy()
        broken[at_live, col] = v
        assert lib.rt_scene_update_live(d._h, broken.ctypes.data, None, live.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT, (col, v)
        assert lib.rt_scene_rebuild_n(d._h, broken.ctypes.data, at_live + 1, None) == capi.RT_ERR_INVALID_ARGUMENT, (col, v)
    assert (order == 0).all()
    np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(bounds_before))
    np.testing.assert_array_equal(d.live(), live)
    assert_same(answers(d, rays, tmax, cam)[0], before, "after the refused calls")
    broken = s.copy()
    broken[at_dead] = (np.nan, np.inf, 2e15, 0.0)
    assert lib.rt_scene_update_live(d._h, broken.ctypes.data, None, live.ctypes.data) == capi.RT_OK
    assert_same(answers(d, rays, tmax, cam)[0], before, "bits in a dead slot")
    static.close(); flat.close(); d.close()
