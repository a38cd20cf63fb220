"""Dynamic scenes on the GPU (rt_scene_create_dynamic / rt_scene_update* / rt_scene_bounds, csrc/rt_dynamic.hpp).  Bit equality is the
yardstick: after any update a dynamic scene answers every general-ray entry with the bytes and counters of a FRESH scene made by
rt_scene_create from the same items, the bounds rt_scene_bounds reports and the same ranges -- which the other suites hold against the
oracle; one animation frame is held against the oracle here as well."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.scenes import random_nested_scene
from tests.test_gpu_camera import identity, restate_frame
from tests.test_gpu_query import ray_families

pytestmark = pytest.mark.gpu

PREC = {rta.RT_F32: oracle.F32, rta.RT_F64: oracle.F64}
REAL = {rta.RT_F32: np.float32, rta.RT_F64: np.float64}
PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
COUNTERS = ("primary", "hits", "shadow", "occluded", "sphere_tests", "bound_tests", "tests_executed", "primary_tests")
LIGHT, EYE = (-1.0, -3.0, 2.0), (0.0, 0.0, -4.0)
OPTS, REGIONS = (96, 64), [(0, 64, 56, 0), (56, 64, 96, 24), (56, 24, 96, 0)]      # one 16x16 block is cut by every tile edge


def scene_of(items, bounds, ranges, precision):
    return rta.Scene(items, rta.normalized(LIGHT, precision), EYE, bounds, ranges, precision)


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def counters(st):
    return tuple(int(st[k]) for k in COUNTERS)


def views(precision):
    return [("look_at", rta.look_at((2.5, 1.5, -3.5), (0.0, -0.5, 0.0), precision=precision)),
            ("identity", np.concatenate([np.asarray(EYE), [1, 0, 0, 0, 1, 0, 0, 0, 1]]).astype(REAL[precision]))]


def answers(d, rays, tmax, precision, cameras=None):
    """[(entry, bytes of every result, counters)] of every general-ray entry on device scene d.  cameras: (name, camera) for the frame
    entries (None: views(precision), which look at a scene of unit size around the origin; tests/test_gpu_scales.py, whose scenes are
    elsewhere, asks for none)."""
    out = []

    def put(name, res):
        *arrays, st = res
        out.append((name, [as_bits(a) for a in arrays], counters(st)))

    for any_hit in (False, True):
        put("intersect any=%d" % any_hit, d.intersect(rays, tmax, any_hit=any_hit, want_stats=True))
        put("intersect any=%d ordered" % any_hit, d.intersect(rays, tmax, any_hit=any_hit, want_stats=True, order=True))
    for all_hits in (False, True):
        put("multi all=%d" % all_hits, d.intersect_multi(rays, 4, tmax, all_hits=all_hits, want_stats=True))
        put("multi all=%d ordered" % all_hits, d.intersect_multi(rays, 4, tmax, all_hits=all_hits, want_stats=True, order=True))
    put("trace", d.trace(rays, want_stats=True))
    put("trace ordered", d.trace(rays, want_stats=True, order=True))
    for name, cam in (views(precision) if cameras is None else cameras):
        for spp in (1, 2):
            put("camera %s spp %d" % (name, spp), d.render_camera(OPTS + (spp,), cam, REGIONS, want_stats=True))
        buf, prev = None, 0
        for step in (4, 2, 1):
            buf, st = d.render_camera_undersampled(OPTS + (1,), cam, REGIONS, step, prev_step=prev, out=buf)
            put("undersampled %s step %d" % (name, step), (buf.copy(), st))
            prev = step
    return out


def assert_same(got, ref, what):
    assert [g[0] for g in got] == [r[0] for r in ref]
    for (name, ga, gc), (_, ra, rc) in zip(got, ref):
        for k, (a, b) in enumerate(zip(ga, ra)):
            np.testing.assert_array_equal(a, b, err_msg="%s: %s, result %d" % (what, name, k))
        assert gc == rc, (what, name, gc, rc)


def fresh_answers(items, bounds, ranges, rays, tmax, precision, cameras=None):
    d = rta.DeviceScene(scene_of(items, bounds, ranges, precision))
    try:
        return answers(d, rays, tmax, precision, cameras)
    finally:
        d.close()


def animate(items, k, R):
    """Frame k of a deterministic animation: every centre displaced by up to 0.3 radii, every radius scaled by 0.75 .. 1.25."""
    it = np.asarray(items, dtype=np.float64)
    i = np.arange(len(it), dtype=np.float64)
    out = it.copy()
    out[:, :3] += it[:, 3:4] * 0.3 * np.stack([np.sin(0.37 * i + k), np.cos(0.91 * i + 2 * k), np.sin(0.13 * i - k)], axis=1)
    out[:, 3] *= 1.0 + 0.25 * np.sin(0.71 * i + 1.3 * k)
    return np.ascontiguousarray(out.astype(R))


def cases(precision):
    """(name, items, bounds, ranges) in REAL: the default pyramid and random nested scenes, one with items that no group covers."""
    R = REAL[precision]
    it, bd, rg = rta.pyramid(8, (0.0, -1.0, 0.0), 1.0, precision)
    out = [("pyramid", it, bd, rg)]
    it, bd, rg = random_nested_scene(8)
    loose = np.array([[1.4, 0.6, 0.3, 0.2], [-1.1, -0.8, 0.5, 0.25]])
    rg = rg.copy()
    rg[:, 0] += 1
    out.append(("nested", np.concatenate([loose[:1], it, loose[1:]]).astype(R), bd.astype(R), rg))
    it, bd, rg = random_nested_scene(9, depth=2)
    out.append(("rooted", it.astype(R), bd.astype(R), rg))           # its first group holds every item: a scene the oracle takes
    return out


_RAYS = {}


def rays_of(name, items, bounds, ranges, precision):
    if (name, precision) not in _RAYS:
        _RAYS[name, precision] = ray_families(scene_of(items, bounds, ranges, precision), np.random.default_rng(31), 12)
    return _RAYS[name, precision]


# ---- 1: a dynamic scene that was never updated is the static scene ----

@PRECISIONS
def test_a_dynamic_pyramid_with_its_own_bounds_is_the_default_scene(precision):
    s = rta.Scene.default(precision=precision)
    rays, tmax = rays_of("pyramid", s.items, s.bounds, s.ranges, precision)
    d = s.device(dynamic=True)
    assert d.traits() == capi.RT_SCENE_DYNAMIC | capi.RT_SCENE_HAS_BOUNDS and s.device().traits() & capi.RT_SCENE_DYNAMIC == 0
    ref = answers(s.device(), rays, tmax, precision)
    assert_same(answers(d, rays, tmax, precision), ref, "dynamic default scene")
    assert any(c[1] for _, _, c in ref) and any(c[3] for _, _, c in ref)                 # hits and occluded shadow rays among them
    np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(s.bounds))
    np.testing.assert_array_equal(as_bits(s.device().bounds()), as_bits(s.bounds))      # a static scene: the bounds it was created with


# ---- 2, 4: an animation with refit bounds; back to the start ----

@PRECISIONS
def test_an_animation_with_refit_bounds_follows_fresh_static_scenes(precision):
    R = REAL[precision]
    for name, it0, bd0, rg in cases(precision):
        rays, tmax = rays_of(name, it0, bd0, rg, precision)
        d = rta.DeviceScene(scene_of(it0, bd0, rg, precision), dynamic=True)
        start = answers(d, rays, tmax, precision)
        assert_same(start, fresh_answers(it0, bd0, rg, rays, tmax, precision), name + " as created")
        for k in (1, 2, 3):
            it = animate(it0, k, R)
            d.update(it)
            bd = d.bounds()
            np.testing.assert_array_equal(as_bits(bd), as_bits(rta.refit_bounds(it, rg, precision)), err_msg="%s frame %d" % (name, k))
            got = answers(d, rays, tmax, precision)
            assert_same(got, fresh_answers(it, bd, rg, rays, tmax, precision), "%s frame %d" % (name, k))
            assert any(not np.array_equal(a, b) for (_, ga, _), (_, sa, _) in zip(got, start) for a, b in zip(ga, sa)), "the animation changed nothing"
            if k == 2 and tuple(rg[0]) == (0, len(it)):      # ... and one frame against the oracle: render.rs over its intersect, restated in numpy
                o = oracle.Scene.from_ranges(it.astype(np.float64), bd.astype(np.float64), rg, LIGHT, EYE, PREC[precision])
                cam = views(precision)[0][1]
                frame, _ = d.render_camera((48, 32, 1), cam, [(0, 32, 48, 0)])
                light = rta.normalized(LIGHT, precision).astype(R)
                np.testing.assert_array_equal(frame, restate_frame(o, oracle.MODE_HIERARCHY, 48, 32, 1, cam, light, [(0, 32, 48, 0)], R))
        # back to the original items and bounds: the original bytes, nothing stale
        d.update(it0, bd0)
        np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(bd0))
        assert_same(answers(d, rays, tmax, precision), start, name + " restored")
        d.close()


# ---- 3: the caller's bounds ----

@PRECISIONS
def test_an_update_with_the_callers_bounds(precision):
    R = REAL[precision]
    name, it0, bd0, rg = cases(precision)[1]
    rays, tmax = rays_of(name, it0, bd0, rg, precision)
    d = rta.DeviceScene(scene_of(it0, bd0, rg, precision), dynamic=True)
    it = animate(it0, 2, R)
    bd = bd0.copy()
    bd[:, :3] += R(0.05)
    bd[:, 3] *= R(0.9)                   # (bounds that do not enclose: culling really changes the results, as in the static suites)
    d.update(it, bd)
    np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(bd))
    assert_same(answers(d, rays, tmax, precision), fresh_answers(it, bd, rg, rays, tmax, precision), "caller's bounds")
    d.update(it)                         # ... and a refit behind it replaces every one of them
    np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(rta.refit_bounds(it, rg, precision)))
    d.close()


# ---- 5: created without bounds = created with the refit ones ----

@PRECISIONS
def test_a_scene_created_without_bounds_is_the_scene_created_with_the_refit_ones(precision):
    for name, it0, bd0, rg in cases(precision):
        rays, tmax = rays_of(name, it0, bd0, rg, precision)
        refit = rta.refit_bounds(it0, rg, precision)
        a = rta.DeviceScene(scene_of(it0, None, rg, precision), dynamic=True)
        b = rta.DeviceScene(scene_of(it0, refit, rg, precision), dynamic=True)
        np.testing.assert_array_equal(as_bits(a.bounds()), as_bits(refit), err_msg=name)
        np.testing.assert_array_equal(as_bits(b.bounds()), as_bits(refit), err_msg=name)
        got = answers(a, rays, tmax, precision)
        assert_same(got, answers(b, rays, tmax, precision), name)
        assert_same(got, fresh_answers(it0, refit, rg, rays, tmax, precision), name + " against the static scene")
        a.close(); b.close()


@PRECISIONS
def test_the_device_refit_is_the_numpy_rule_at_every_scale(precision):
    # spheres at 1e15, at 1e-30 and where even the radii are subnormal, one group of one sphere, coincident centres: the reach's second
    # form (no product in it) and the exactness of subnormal sums are the device's as they are numpy's
    from tests.test_dynamic_host import refit_inputs
    for name, it, rg in refit_inputs(precision):
        if name == "pyramid":
            continue                     # (the tests above)
        d = rta.DeviceScene(scene_of(it, None, rg, precision), dynamic=True)
        np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(rta.refit_bounds(it, rg, precision)), err_msg=name)
        back = np.ascontiguousarray(it[::-1])          # other values through an update (the same spheres, the other way round)
        d.update(back)
        np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(rta.refit_bounds(back, rg, precision)), err_msg=name + " reversed")
        d.close()


# ---- 6: no ranges at all ----

@PRECISIONS
def test_a_flat_dynamic_scene_follows_its_updates(precision):
    R = REAL[precision]
    it0 = random_nested_scene(4)[0].astype(R)
    rays, tmax = ray_families(scene_of(it0, None, None, precision), np.random.default_rng(6), 12)
    d = rta.DeviceScene(scene_of(it0, None, None, precision), dynamic=True)
    assert d.traits() == capi.RT_SCENE_DYNAMIC and d.bounds().shape == (0, 4)
    for k in (1, 0, 2):                  # the first update lands before the first query
        it = animate(it0, k, R) if k else it0
        d.update(it)
        assert_same(answers(d, rays, tmax, precision), fresh_answers(it, None, None, rays, tmax, precision), "flat frame %d" % k)
    d.close()


# ---- 7: the device entry, on a stream that is not the current one ----

@PRECISIONS
def test_a_device_update_orders_the_queries_behind_it_on_its_stream(precision):
    import torch
    R = REAL[precision]
    name, it0, bd0, rg = cases(precision)[0]
    rays, tmax = rays_of(name, it0, bd0, rg, precision)
    cam = views(precision)[0][1]
    opts, nbytes = OPTS + (1,), sum((r - l) * (t - b) for l, t, r, b in REGIONS) * 4
    host = rta.DeviceScene(scene_of(it0, bd0, rg, precision), dynamic=True)
    dev = rta.DeviceScene(scene_of(it0, bd0, rg, precision), dynamic=True)
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    trays, ttmax = torch.from_numpy(rays).cuda(), torch.from_numpy(tmax).cuda()
    for k, with_bounds in ((1, False), (2, True), (3, False)):
        it = animate(it0, k, R)
        bd = rta.refit_bounds(animate(it0, k + 1, R), rg, precision) if with_bounds else None      # (some other frame's: they enclose nothing in particular)
        host.update(it, bd)
        frame_ref, _ = host.render_camera(opts, cam, REGIONS, want_stats=False)
        near_ref = host.intersect(rays, tmax)
        frame = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        dev.update(torch.from_numpy(it).cuda(), None if bd is None else torch.from_numpy(bd).cuda(), stream=side)
        dev.render_camera_device(opts, cam, REGIONS, frame.data_ptr(), stream=side.cuda_stream)      # no synchronisation in between
        near = dev.intersect(trays, ttmax, stream=side)
        side.synchronize()
        np.testing.assert_array_equal(frame.cpu().numpy(), frame_ref, err_msg="frame %d" % k)
        for a, b in zip(near_ref, near):
            np.testing.assert_array_equal(as_bits(a), as_bits(b.cpu().numpy()), err_msg="frame %d" % k)
        np.testing.assert_array_equal(as_bits(dev.bounds()), as_bits(host.bounds()))
    # a raw device pointer and a raw stream handle
    it = animate(it0, 5, R)
    t = torch.from_numpy(it).cuda()
    torch.cuda.current_stream().synchronize()
    dev.update(int(t.data_ptr()), stream=side.cuda_stream)
    host.update(it)
    np.testing.assert_array_equal(as_bits(dev.bounds()), as_bits(host.bounds()))          # (rt_scene_bounds waits for the update)
    host.close(); dev.close()


@PRECISIONS
def test_an_update_on_a_side_stream_and_on_its_handle_is_the_default_stream_update(precision):
    import torch
    R = REAL[precision]
    it0, bd0, rg = rta.pyramid(2, (0.0, -1.0, 0.0), 1.0, precision)
    rng = np.random.default_rng(65)
    rays = np.concatenate([np.tile(np.asarray(EYE), (65, 1)), rng.normal(size=(65, 3)) * (0.3, 0.3, 0.0) + (0.0, -0.15, 1.0)], axis=1)      # one wave and one lane
    rays[:, 3:] /= np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
    trays = torch.from_numpy(rays.astype(R)).cuda()
    d = rta.DeviceScene(scene_of(it0, bd0, rg, precision), dynamic=True)
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    it, other = animate(it0, 1, R), animate(it0, 2, R)
    live = np.array([1, 1, 0, 1, 1], np.uint8)
    for lv in (None, live):
        tit, tlv = torch.from_numpy(it).cuda(), None if lv is None else torch.from_numpy(lv).cuda()
        d.update(tit, live=tlv)
        ref = [as_bits(a.cpu().numpy()) for a in d.intersect(trays)]
        ref_bounds = d.bounds()
        assert (d.intersect(trays)[2] >= 0).any()
        for stream in (side, side.cuda_stream):
            d.update(other)
            d.update(tit * 1.0, live=None if lv is None else tlv.clone(), stream=stream)      # inputs made on the current stream and dropped at once
            got = d.intersect(trays, stream=stream)
            side.synchronize()
            for a, b in zip(ref, got):
                np.testing.assert_array_equal(a, as_bits(b.cpu().numpy()))
            np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(ref_bounds))
    d.close()


# ---- 8: status codes ----

def test_status_codes_and_a_refused_update_leaves_the_scene_alone():
    import torch
    s = rta.Scene.default(level=5)
    d = s.device(dynamic=True)
    rays, tmax = ray_families(s, np.random.default_rng(2), 12)
    before = [as_bits(a) for a in d.intersect(rays, tmax)]
    frame_before, _ = d.render_camera((64, 48, 1), identity(s), [(0, 48, 64, 0)], want_stats=False)
    regions, opts = [(0, 48, 64, 0)], (64, 48, 1)
    out = torch.zeros(64 * 48 * 4, dtype=torch.uint8, device="cuda")
    refused = [lambda: d.render_tiles(opts, regions, rta.RT_TRAVERSAL_SKIP), lambda: d.render_tiles(opts, regions, rta.RT_TRAVERSAL_FLAT),
               lambda: d.render_tiles(opts, regions, rta.RT_TRAVERSAL_SKIP, want_stats=False), lambda: d.render_region(opts, regions[0]),
               lambda: d.render_region(opts, regions[0], want_stats=True), lambda: d.render_tiles_stream(opts, regions, lambda *a: None),
               lambda: d.render_frame_stream(opts, regions, capi.RT_FRAME_RGBA, np.zeros(64 * 48 * 4, dtype=np.uint8)),
               lambda: d.render_tiles_device(opts, regions, out.data_ptr()), lambda: d.render_frame_device(opts, regions, out.data_ptr())]
    for call in refused:
        with pytest.raises(rta.RtError) as e:
            call()
        assert e.value.status == capi.RT_ERR_UNSUPPORTED and "rt_render_camera" in str(e.value)
    # an immutable scene takes no update
    static = s.device()
    assert capi.lib.rt_scene_update(static._h, s.items.ctypes.data, None) == capi.RT_ERR_UNSUPPORTED
    assert capi.lib.rt_scene_update_device(static._h, C.c_void_p(out.data_ptr()), None, None) == capi.RT_ERR_UNSUPPORTED
    # values outside the domain: refused before the device is touched
    def broken(row, col, v):
        it = s.items.copy()
        it[row, col] = v
        return it
    for it in (broken(7, 0, np.nan), broken(0, 3, 0.0), broken(340, 3, -1.0), broken(100, 2, 2e15), broken(3, 1, np.inf)):
        assert capi.lib.rt_scene_update(d._h, it.ctypes.data, None) == capi.RT_ERR_INVALID_ARGUMENT
    bad_bounds = s.bounds.copy()
    bad_bounds[2, 1] = np.nan
    assert capi.lib.rt_scene_update(d._h, animate(s.items, 1, np.float32).ctypes.data, bad_bounds.ctypes.data) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_update(d._h, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_update_device(d._h, None, None, None) == capi.RT_ERR_INVALID_ARGUMENT
    assert capi.lib.rt_scene_update_device(d._h, C.c_void_p(out.data_ptr() + 4), None, None) == capi.RT_ERR_INVALID_ARGUMENT      # misaligned
    for a, b in zip(before, d.intersect(rays, tmax)):
        np.testing.assert_array_equal(a, as_bits(b))
    np.testing.assert_array_equal(d.render_camera((64, 48, 1), identity(s), regions, want_stats=False)[0], frame_before)
    np.testing.assert_array_equal(as_bits(d.bounds()), as_bits(s.bounds))


# ---- 9: readers while a host update runs ----

def test_readers_during_a_host_update_see_the_old_scene_or_the_new_one():
    precision, R = rta.RT_F32, np.float32
    name, it0, bd0, rg = cases(precision)[0]
    rays, tmax = rays_of(name, it0, bd0, rg, precision)
    it1 = animate(it0, 1, R)
    d = rta.DeviceScene(scene_of(it0, bd0, rg, precision), dynamic=True)
    read = lambda: b"".join(as_bits(a).tobytes() for a in d.intersect(rays, tmax))
    old = read()
    d.update(it1)
    new = read()
    assert old != new
    d.update(it0, bd0)
    assert read() == old
    seen, errors = [[] for _ in range(4)], []
    gate = threading.Barrier(5)

    def reader(k):
        try:
            gate.wait()
            for _ in range(6):
                seen[k].append(read())
        except BaseException as e:      # noqa: BLE001
            errors.append(e)

    def writer():
        try:
            gate.wait()
            d.update(it1)
        except BaseException as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=reader, args=(k,)) for k in range(4)] + [threading.Thread(target=writer)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(4):
        states = ["old" if b == old else "new" if b == new else "mixed" for b in seen[k]]
        assert "mixed" not in states and states == sorted(states, reverse=True), states      # old ... old new ... new: never back
    assert read() == new
    d.close()
