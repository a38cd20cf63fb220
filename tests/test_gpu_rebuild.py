"""Rebuilds on the GPU (rt_sphere_order* / rt_scene_rebuild*, csrc/rt_rebuild.hpp).  The contract is a permutation and the existing update:
rebuild(s) is update(s[order]) with order = np.argsort(sphere_keys(s), kind="stable"), so the yardstick of tests/test_gpu_dynamic.py holds
as it stands -- after a rebuild the scene answers every general-ray entry with the bytes and counters of a FRESH static scene made from
s[order], the bounds rt_scene_bounds reports and the same ranges.  One frame is held against the oracle directly, and the point of the
feature -- fewer tests per ray than the same spheres left in the caller's order -- is a condition on the counters.

Sizes: 1 (the smallest batch), 2 with one centre (every sort pass skipped), 257 (one past a 256-key sort step and a 256-item refit
record), 5,000 with 500 exact duplicates of other centres (stability, three sort slices, the root group cut into 20 refit records)."""
import ctypes as C

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.test_gpu_camera import restate_frame
from tests.test_gpu_dynamic import (EYE, LIGHT, OPTS, PREC, PRECISIONS, REAL, REGIONS, animate, answers, as_bits, assert_same, fresh_answers,
                                    scene_of, views)
from tests.test_gpu_query import ray_families

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 257, 5000)
LEAF = 4


def spheres_of(n, precision, seed=2026):
    """n spheres in a seeded random caller order, in front of the eye; n == 2: one centre twice; n == 5000: 500 of them share their centre
    with another sphere (other radii)."""
    R = REAL[precision]
    rng = np.random.default_rng(seed + n)
    s = np.concatenate([rng.uniform([-2.0, -2.0, -0.5], [2.0, 1.5, 3.5], (n, 3)), rng.uniform(*((0.02, 0.08) if n > 2 else (0.1, 0.3)), (n, 1))], axis=1)
    if n == 2:
        s[1, :3] = s[0, :3]
    if n == 5000:
        s[4500:, :3] = s[rng.choice(4500, 500, replace=False), :3]
        s = s[rng.permutation(n)]
    return np.ascontiguousarray(s.astype(R))


def expected_order(s):
    return np.argsort(rta.sphere_keys(s), kind="stable").astype(np.uint32)


_SHARED = {}


def case(n, precision):
    """(spheres in caller order, ranges, order, rays, tmax, answers of the fresh static scene of spheres[order]) -- made once."""
    if (n, precision) not in _SHARED:
        s = spheres_of(n, precision)
        rg = rta.balanced_ranges(n, LEAF)
        order = expected_order(s)
        bd = rta.refit_bounds(s[order], rg, precision)
        rays, tmax = ray_families(scene_of(s[order], bd, rg, precision), np.random.default_rng(31), 40)
        _SHARED[n, precision] = (s, rg, order, rays, tmax, fresh_answers(s[order], bd, rg, rays, tmax, precision))
    return _SHARED[n, precision]


def dynamic_scene(s, rg, precision):
    return rta.DeviceScene(scene_of(s, None, rg, precision), dynamic=True)


# ---- 1: the order ----

@PRECISIONS
def test_the_sphere_order_is_the_stable_sort_of_the_numpy_keys(precision):
    import torch
    static = rta.Scene.three_spheres(precision).device()
    dyn = rta.Scene.default(level=3, precision=precision).device(dynamic=True)
    side = torch.cuda.Stream()
    for n in SIZES:
        s = spheres_of(n, precision)
        want = expected_order(s)
        if n == 5000:
            keys = rta.sphere_keys(s)
            assert (np.diff(keys[want].astype(np.int64)) == 0).sum() >= 500          # ties for the sort to keep in order
        for d in (static, dyn):                                                      # the scene lends its device, REAL and workspace
            got = d.sphere_order(s)
            assert got.dtype == np.uint32
            np.testing.assert_array_equal(got, want, err_msg="host entry, n = %d" % n)
            t = d.sphere_order(torch.from_numpy(s).cuda(), stream=side)
            side.synchronize()
            np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), want, err_msg="device entry, n = %d" % n)


@PRECISIONS
def test_the_order_and_the_rebuild_on_a_side_stream_and_on_its_handle_are_the_default_stream_ones(precision):
    import torch
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    static = rta.Scene.three_spheres(precision).device()
    s = spheres_of(65, precision)                                                    # one wave and one lane
    ts = torch.from_numpy(s).cuda()
    ref = static.sphere_order(ts)
    torch.cuda.current_stream().synchronize()
    np.testing.assert_array_equal(ref.cpu().numpy().view(np.uint32), expected_order(s))
    for stream in (side, side.cuda_stream):
        got = static.sphere_order(ts * 1.0, stream=stream)                           # an input made on the current stream and dropped at once
        side.synchronize()
        assert got.dtype == torch.uint32 and got.device.type == "cuda"
        np.testing.assert_array_equal(as_bits(got.cpu().numpy()), as_bits(ref.cpu().numpy()))
    # a rebuild of the level-2 pyramid from its own spheres, reversed
    items = rta.pyramid(2, (0.0, -1.0, 0.0), 1.0, precision)[0]
    back = np.ascontiguousarray(items[::-1])
    tb = torch.from_numpy(back).cuda()
    d = dynamic_scene(items, rta.balanced_ranges(len(items), LEAF), precision)
    ref = d.rebuild(tb)
    ref_bounds = d.bounds()
    np.testing.assert_array_equal(ref.cpu().numpy().view(np.uint32), expected_order(back))
    for stream in (side, side.cuda_stream):
        d.update(items)                                                              # the caller's order again
        got = d.rebuild(tb * 1.0, stream=stream)
        side.synchronize()
        assert got.dtype == torch.uint32 and got.device.type == "cuda"
        np.testing.assert_array_equal(as_bits(got.cpu().numpy()), as_bits(ref.cpu().numpy()))
        np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(ref_bounds))
    d.close()


# ---- 2: a rebuild is the update with the permuted spheres ----

@PRECISIONS
@pytest.mark.parametrize("n", SIZES)
def test_a_rebuilt_scene_is_the_fresh_scene_of_the_sorted_spheres(n, precision):
    s, rg, order, rays, tmax, ref = case(n, precision)
    d = dynamic_scene(s, rg, precision)
    np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(rta.refit_bounds(s, rg, precision)))      # as created: the caller's order
    got_order = d.rebuild(s)
    assert got_order.dtype == np.uint32
    np.testing.assert_array_equal(got_order, order)
    np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(rta.refit_bounds(s[order], rg, precision)))
    got = answers(d, rays, tmax, precision)
    assert_same(got, ref, "rebuilt, n = %d" % n)
    if n >= 257:
        assert any(c[1] for _, _, c in ref) and any(c[3] for _, _, c in ref)             # hits and occluded shadow rays among them
        slots = d.intersect(rays, tmax)[2]                            # item_out names DFS slots; through the order, the caller's spheres
        hit = slots >= 0
        assert hit.any() and (slots[hit] < n).all()
    d.close()


# ---- 3: host and device entries; the device entry on a stream that is not the current one ----

@PRECISIONS
def test_a_device_rebuild_orders_the_queries_behind_it_on_its_stream(precision):
    import torch
    n = 5000
    s, rg, order, rays, tmax, _ = case(n, precision)
    cam = views(precision)[0][1]
    opts, nbytes = OPTS + (1,), sum((r - l) * (t - b) for l, t, r, b in REGIONS) * 4
    host, dev = dynamic_scene(s, rg, precision), dynamic_scene(s, rg, precision)
    np.testing.assert_array_equal(host.rebuild(s), order)
    frame_ref, _ = host.render_camera(opts, cam, REGIONS, want_stats=False)
    near_ref = host.intersect(rays, tmax)
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    trays, ttmax = torch.from_numpy(rays).cuda(), torch.from_numpy(tmax).cuda()
    frame = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torder = dev.rebuild(torch.from_numpy(s).cuda(), stream=side)
    dev.render_camera_device(opts, cam, REGIONS, frame.data_ptr(), stream=side.cuda_stream)      # no synchronisation in between
    near = dev.intersect(trays, ttmax, stream=side)
    side.synchronize()
    np.testing.assert_array_equal(torder.cpu().numpy().view(np.uint32), order)
    np.testing.assert_array_equal(frame.cpu().numpy(), frame_ref)
    for a, b in zip(near_ref, near):
        np.testing.assert_array_equal(as_bits(a), as_bits(b.cpu().numpy()))
    np.testing.assert_array_equal(as_bits(dev.bounds()), as_bits(host.bounds()))
    # a second device rebuild, from other spheres, without an order: the workspace is the scene's and is there already
    s2 = np.ascontiguousarray(animate(s, 1, REAL[precision])[::-1])
    t2 = torch.from_numpy(s2).cuda()
    torch.cuda.current_stream().synchronize()
    capi.check(capi.lib.rt_scene_rebuild_device(dev._h, C.c_void_p(t2.data_ptr()), None, C.c_void_p(side.cuda_stream)), "rt_scene_rebuild_device")
    capi.check(capi.lib.rt_scene_rebuild(host._h, s2.ctypes.data, None), "rt_scene_rebuild")
    np.testing.assert_array_equal(as_bits(dev.bounds()), as_bits(host.bounds()))          # (rt_scene_bounds waits for the rebuild)
    np.testing.assert_array_equal(as_bits(host.bounds()), as_bits(rta.refit_bounds(s2[expected_order(s2)], rg, precision)))
    host.close(); dev.close()


# ---- 4: rebuild, update, rebuild: the topology survives ----

@PRECISIONS
def test_rebuild_update_rebuild_each_match_their_fresh_scene(precision):
    R = REAL[precision]
    n = 257
    s, rg, order, rays, tmax, ref = case(n, precision)
    d = dynamic_scene(s, rg, precision)
    d.rebuild(s)
    assert_same(answers(d, rays, tmax, precision), ref, "first rebuild")
    moved = animate(s[order], 2, R)                                  # in DFS order, as an update takes them
    d.update(moved)
    bd = d.bounds()
    np.testing.assert_array_equal(as_bits(bd), as_bits(rta.refit_bounds(moved, rg, precision)))
    assert_same(answers(d, rays, tmax, precision), fresh_answers(moved, bd, rg, rays, tmax, precision), "update behind a rebuild")
    back = np.empty_like(moved)
    back[order] = moved                                              # the moved spheres in the caller's order
    order2 = d.rebuild(back)
    np.testing.assert_array_equal(order2, expected_order(back))
    bd2 = d.bounds()
    np.testing.assert_array_equal(as_bits(bd2), as_bits(rta.refit_bounds(back[order2], rg, precision)))
    assert_same(answers(d, rays, tmax, precision), fresh_answers(back[order2], bd2, rg, rays, tmax, precision), "second rebuild")
    d.close()


# ---- 5: a scene created with the caller's own bounds and other ranges ----

def test_a_scene_with_the_callers_bounds_and_ranges_is_rebuilt_too():
    precision = rta.RT_F32
    s = spheres_of(257, precision)
    rg = np.array([[0, 257], [0, 100], [10, 30], [100, 157], [256, 1]], dtype=np.int32)      # any ranges a scene takes
    wide = np.tile(np.array([[0.0, 0.0, 1.5, 9.0]], dtype=np.float32), (len(rg), 1))
    d = rta.DeviceScene(scene_of(s, wide, rg, precision), dynamic=True)
    np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(wide))
    order = d.rebuild(s)
    np.testing.assert_array_equal(order, expected_order(s))
    bd = d.bounds()
    np.testing.assert_array_equal(as_bits(bd), as_bits(rta.refit_bounds(s[order], rg, precision)))
    rays, tmax = ray_families(scene_of(s[order], bd, rg, precision), np.random.default_rng(5), 12)
    assert_same(answers(d, rays, tmax, precision), fresh_answers(s[order], bd, rg, rays, tmax, precision), "caller's ranges")
    d.close()


# ---- 6: one frame against the oracle ----

@PRECISIONS
def test_a_rebuilt_frame_against_the_oracle(precision):
    R = REAL[precision]
    s, rg, order, *_ = case(257, precision)
    d = dynamic_scene(s, rg, precision)
    d.rebuild(s)
    bd = d.bounds()
    o = oracle.Scene.from_ranges(s[order].astype(np.float64), bd.astype(np.float64), rg, LIGHT, EYE, PREC[precision])
    cam = views(precision)[0][1]
    frame, _ = d.render_camera((48, 32, 1), cam, [(0, 32, 48, 0)])
    light = rta.normalized(LIGHT, precision).astype(R)
    np.testing.assert_array_equal(frame, restate_frame(o, oracle.MODE_HIERARCHY, 48, 32, 1, cam, light, [(0, 32, 48, 0)], R))
    assert frame.reshape(-1, 4)[:, :3].any()
    d.close()


# ---- 7: the point of the feature ----

@PRECISIONS
def test_a_rebuild_costs_fewer_tests_than_the_same_spheres_in_the_callers_order(precision):
    """sphere_tests + bound_tests of one camera frame over the 5,000 spheres in a seeded random order: after update(s) -- the caller's
    order under the same ranges -- against after rebuild(s).  A condition, not a tolerance.  The CPU oracle's counters for this seed and
    frame (96 x 64, one sample, the identity camera = the oracle's own): see DESIGN.md 4.12."""
    s, rg, *_ = case(5000, precision)
    cam = views(precision)[1][1]
    d = dynamic_scene(s, rg, precision)
    tests = lambda st: int(st["sphere_tests"]) + int(st["bound_tests"])
    d.update(s)
    shuffled_frame, st_shuffled = d.render_camera(OPTS + (1,), cam, [(0, 64, 96, 0)])
    d.rebuild(s)
    rebuilt_frame, st_rebuilt = d.render_camera(OPTS + (1,), cam, [(0, 64, 96, 0)])
    print("tests per frame: caller's order %d, rebuilt %d, ratio %.2f" % (tests(st_shuffled), tests(st_rebuilt), tests(st_shuffled) / max(1, tests(st_rebuilt))))
    assert st_shuffled["primary"] == st_rebuilt["primary"] == 96 * 64
    assert tests(st_rebuilt) < tests(st_shuffled)
    np.testing.assert_array_equal(rebuilt_frame, shuffled_frame)                         # the same spheres: the same picture
    d.close()


# ---- 8: any bits through the device entry ----

def test_hostile_bits_give_a_permutation_and_a_scene_that_still_answers():
    import torch
    precision, n = rta.RT_F32, 257
    s, rg, _, rays, tmax, _ = case(n, precision)
    bad = s.copy()
    rng = np.random.default_rng(8)
    bad[rng.choice(n, 40, replace=False), rng.integers(0, 4, 40)] = np.nan
    bad[rng.choice(n, 40, replace=False), rng.integers(0, 3, 40)] = np.inf
    bad[rng.choice(n, 20, replace=False), rng.integers(0, 3, 20)] = -np.inf
    bad[rng.choice(n, 40, replace=False), 3] = -1.0
    bad[rng.choice(n, 10, replace=False), 0] = 3e38
    d = dynamic_scene(s, rg, precision)
    order = d.rebuild(torch.from_numpy(bad).cuda())
    near = d.intersect(torch.from_numpy(rays).cuda(), torch.from_numpy(tmax).cuda())
    torch.cuda.synchronize()
    assert sorted(order.cpu().numpy().view(np.uint32).tolist()) == list(range(n))
    assert near[2].shape == (len(rays),)
    order2 = d.sphere_order(torch.from_numpy(bad).cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(order2.cpu().numpy(), order.cpu().numpy())
    d.rebuild(s)                                                     # ... and good values behind them leave nothing stale
    np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(rta.refit_bounds(s[expected_order(s)], rg, precision)))
    d.close()


# ---- 9: status codes ----

def test_status_codes_and_a_refused_rebuild_leaves_the_scene_alone():
    import torch
    precision = rta.RT_F32
    s, rg, _, rays, tmax, _ = case(257, precision)
    order = np.zeros(257, dtype=np.uint32)
    dev_s = torch.from_numpy(s).cuda()
    torch.cuda.synchronize()
    bd = rta.refit_bounds(s, rg, precision)
    static = rta.DeviceScene(scene_of(s, bd, rg, precision))
    flat = rta.DeviceScene(scene_of(s, None, None, precision), dynamic=True)
    dyn = dynamic_scene(s, rg, precision)
    for d, word in ((static, b"rt_scene_create"), (flat, b"n_bounds == 0")):
        before = [as_bits(a) for a in d.intersect(rays, tmax)]
        assert capi.lib.rt_scene_rebuild(d._h, s.ctypes.data, order.ctypes.data) == capi.RT_ERR_UNSUPPORTED
        assert word in capi.lib.rt_last_error_message()
        assert capi.lib.rt_scene_rebuild_device(d._h, C.c_void_p(dev_s.data_ptr()), None, None) == capi.RT_ERR_UNSUPPORTED
        with pytest.raises(rta.RtError) as e:
            d.rebuild(s)
        assert e.value.status == capi.RT_ERR_UNSUPPORTED
        for a, b in zip(before, d.intersect(rays, tmax)):
            np.testing.assert_array_equal(a, as_bits(b))
    # values outside the domain, NULL and misaligned pointers: refused before the device is touched, the scene unchanged
    before = [as_bits(a) for a in dyn.intersect(rays, tmax)]
    for row, col, v in ((7, 0, np.nan), (0, 3, 0.0), (200, 3, -1.0), (100, 2, 2e15), (3, 1, np.inf)):
        broken = s.copy()
        broken[row, col] = v
        assert capi.lib.rt_scene_rebuild(dyn._h, broken.ctypes.data, order.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
        assert dyn.sphere_order(s).shape == (257,) and capi.lib.rt_sphere_order(dyn._h, broken.ctypes.data, 257, order.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_rebuild(dyn._h, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_rebuild_device(dyn._h, None, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_rebuild_device(dyn._h, C.c_void_p(dev_s.data_ptr() + 4), None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert not order.any()
    for a, b in zip(before, dyn.intersect(rays, tmax)):
        np.testing.assert_array_equal(a, as_bits(b))
    np.testing.assert_array_equal(as_bits(dyn.bounds()), as_bits(bd))
    for d in (static, flat, dyn):
        d.close()
