"""Coherent ray batches on the GPU (rt_ray_order*, rt_*_ordered*; csrc/rt_order.hpp).  Everything here is exact: the device's
order is the stable argsort of the numpy key, and a walk in ANY order writes the bytes and counts the tests of the unordered call.
No test feeds a device entry an index >= n: that guard is one comparison to be read in the kernels, not something to try out."""
import ctypes as C

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.scenes import hundred_thousand_spheres, random_nested_scene
from tests.test_gpu_query import REAL, ray_families
from tests.test_order_host import camera_rays

pytestmark = pytest.mark.gpu

QUERY_COUNTERS = ("primary", "hits", "shadow", "occluded", "sphere_tests", "bound_tests", "tests_executed", "primary_tests")


def raw(a):
    """The bytes of a result as integers, so that tmax / NaN patterns count."""
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint8)


def same(ref, got, what):
    assert len(ref) == len(got), what
    for i, (a, b) in enumerate(zip(ref, got)):
        if isinstance(a, dict):
            for key in QUERY_COUNTERS:
                assert a[key] == b[key], (what, key, a[key], b[key])
        else:
            assert np.array_equal(raw(a), raw(b)), (what, i)


def random_inside_root(s, n, rng):
    """tools/query_rate.py's "random" batch: origins inside the scene's root bound, random unit directions."""
    root = s.bounds[0].astype(np.float64)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = root[:3] + rng.normal(size=(n, 3)) / np.sqrt(3) * root[3] * 0.5
    o = np.where(np.linalg.norm(o - root[:3], axis=1, keepdims=True) < root[3], o, root[:3])
    return np.concatenate([o, u], axis=1).astype(REAL[s.precision])


def check_order(d, rays, what):
    import torch
    want = np.argsort(rta.ray_keys(rays), kind="stable").astype(np.uint32)
    host = d.ray_order(rays)
    assert host.dtype == np.uint32 and np.array_equal(host, want), (what, "host", int((host != want).sum()))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev = d.ray_order(torch.from_numpy(rays).cuda(), stream=stream)
    stream.synchronize()
    assert dev.dtype == torch.uint32 and dev.device.type == "cuda"
    assert np.array_equal(dev.cpu().numpy(), want), (what, "device")


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_ray_order_on_a_side_stream_and_on_its_handle_is_the_default_stream_order(precision):
    import torch
    d = rta.Scene.three_spheres(precision).device()
    rng = np.random.default_rng(65)
    rays = np.concatenate([rng.normal(size=(65, 3)) * 0.5 + (0.0, 0.0, -4.0), rng.normal(size=(65, 3))], axis=1).astype(REAL[precision])      # one wave and one lane
    tr = torch.from_numpy(rays).cuda()
    ref = d.ray_order(tr)
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(ref.cpu().numpy(), np.argsort(rta.ray_keys(rays), kind="stable"))
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    for stream in (side, side.cuda_stream):
        got = d.ray_order(tr * 1.0, stream=stream)                             # an input made on the current stream and dropped at once
        side.synchronize()
        assert got.dtype == torch.uint32 and got.device.type == "cuda" and np.array_equal(raw(got), raw(ref)), stream


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_ray_order_is_the_stable_argsort_of_the_key(precision):
    R = REAL[precision]
    s = rta.Scene.default(precision=precision)
    d = s.device()
    rng = np.random.default_rng(40 + precision)
    w, h = 1920, 1080
    cam = camera_rays(w, h, s.eye).astype(R)                                   # one origin: no origin bits, the top pass has nothing to move
    check_order(d, cam[rng.permutation(w * h)], "shuffled camera")
    check_order(d, cam, "camera")
    rnd = random_inside_root(s, 2 << 20, rng)                                  # exactly kSortMaxBlocks slices of kSortTile
    check_order(d, rnd, "random")
    check_order(d, random_inside_root(s, 2300001, rng), "random, slices above a tile")
    # repeated identical rays: equal keys keep the caller's order
    few = rnd[:7]
    check_order(d, few[rng.integers(0, 7, 50000)], "repeated rays")
    check_order(d, np.repeat(rnd[:1], 3000, axis=0), "one ray 3000 times")
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 100003):
        check_order(d, rnd[100:100 + n], "n = %d" % n)
        check_order(d, cam[rng.integers(0, w * h, n)], "camera, n = %d" % n)
    # origins on a line, on a plane, in a box far from 0 and a box of tiny extent
    for k, batch in enumerate((rnd[:5000] * np.array([1, 0, 0, 1, 1, 1], R), rnd[:5000] * np.array([1, 1, 0, 1, 1, 1], R),
                               rnd[:5000] + np.array([1e6, -3e5, 7e3, 0, 0, 0], R), rnd[:5000] * np.array([1e-20, 1e-20, 1e-20, 1, 1, 1], R))):
        check_order(d, np.ascontiguousarray(batch.astype(R)), "degenerate box %d" % k)
    d.close()


def order_scenes(precision):
    """The query scenes of the existing GPU tests: the default scene at L8, a scene without bounds, the 100,000-sphere scene."""
    it, _, _ = random_nested_scene(3)
    return [("default_L8", rta.Scene.default(8, precision=precision), 60),
            ("no_bounds", rta.Scene(it, rta.normalized((-1.0, -3.0, 2.0), precision), (0.0, 0.0, -4.0), precision=precision), 60),
            ("100k", rta.Scene.from_spheres_auto(hundred_thousand_spheres(), precision=precision), 12)]


def orders_of(d, rays, rng):
    n = len(rays)
    return [("one call", True), ("ray_order", d.ray_order(rays)), ("random permutation", rng.permutation(n).astype(np.uint32)),
            ("identity", np.arange(n, dtype=np.uint32)), ("reversed, int64", np.arange(n)[::-1])]


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_walks_in_any_order_write_the_same_bytes_and_count_the_same_tests(precision):
    import torch
    rng = np.random.default_rng(50 + precision)
    for name, s, n_each in order_scenes(precision):
        d = s.device()
        rays, tmax = ray_families(s, rng, n_each)
        rays = np.concatenate([rays] * 3)[:len(rays) * 3 - 5]                  # several waves, the last one partly filled
        tmax = np.concatenate([tmax] * 3)[:len(rays)]
        calls = [("nearest", lambda **kw: d.intersect(rays, tmax, want_stats=True, **kw)),
                 ("any", lambda **kw: d.intersect(rays, tmax, any_hit=True, want_stats=True, **kw)),
                 ("nearest, no stats", lambda **kw: d.intersect(rays, tmax, **kw)),
                 ("nearest, tmax inf", lambda **kw: d.intersect(rays, want_stats=True, **kw)),
                 ("trace", lambda **kw: d.trace(rays, want_stats=True, **kw)),
                 ("trace, no stats", lambda **kw: d.trace(rays, **kw))]
        for k in (1, 4, 8, 16):                                                 # every list capacity, both modes, with and without counters
            for all_hits in (False, True):
                calls.append(("multi k=%d all=%d" % (k, all_hits), lambda k=k, all_hits=all_hits, **kw:
                              d.intersect_multi(rays, k, tmax, all_hits=all_hits, want_stats=True, **kw)))
                calls.append(("multi k=%d all=%d, no stats" % (k, all_hits), lambda k=k, all_hits=all_hits, **kw:
                              d.intersect_multi(rays, k, tmax, all_hits=all_hits, **kw)))
        orders = orders_of(d, rays, rng)
        for what, call in calls:
            ref = call()
            for oname, order in orders:
                same(ref, call(order=order), (name, what, oname))
        # the device entries: torch tensors on a stream of their own, with and without counters
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            tr, tt = torch.from_numpy(rays).cuda(), torch.from_numpy(tmax).cuda()
            torders = [("one call", True), ("ray_order", d.ray_order(tr, stream=stream)),
                       ("random permutation", torch.from_numpy(rng.permutation(len(rays)).astype(np.int32)).cuda()),
                       ("identity", torch.arange(len(rays), dtype=torch.int32, device="cuda"))]
            for want_stats in (False, True):
                refs = (d.intersect(rays, tmax, want_stats=want_stats), d.intersect(rays, tmax, any_hit=True, want_stats=want_stats),
                        d.intersect_multi(rays, 16, tmax, want_stats=want_stats), d.intersect_multi(rays, 4, tmax, all_hits=True, want_stats=want_stats),
                        d.trace(rays, want_stats=want_stats))
                for oname, order in torders:
                    got = (d.intersect(tr, tt, want_stats=want_stats, stream=stream, order=order),
                           d.intersect(tr, tt, any_hit=True, want_stats=want_stats, stream=stream, order=order),
                           d.intersect_multi(tr, 16, tt, want_stats=want_stats, stream=stream, order=order),
                           d.intersect_multi(tr, 4, tt, all_hits=True, want_stats=want_stats, stream=stream, order=order),
                           d.trace(tr, want_stats=want_stats, stream=stream, order=order))
                    stream.synchronize()
                    for i, (a, b) in enumerate(zip(refs, got)):
                        same(a, b, (name, "device", oname, want_stats, i))
        d.close()


def test_a_large_incoherent_batch_through_the_one_call_form():
    # 300,000 shuffled camera rays on the default scene: many sort slices, every wave full, the order computed inside the call
    s = rta.Scene.default()
    d = s.device()
    rng = np.random.default_rng(7)
    cam = camera_rays(1920, 1080, s.eye)
    rays = cam[rng.permutation(len(cam))[:300000]]
    same(d.intersect(rays, want_stats=True), d.intersect(rays, want_stats=True, order=True), "nearest")
    same(d.intersect_multi(rays, 16, want_stats=True), d.intersect_multi(rays, 16, want_stats=True, order=True), "multi")
    same(d.trace(rays, want_stats=True), d.trace(rays, want_stats=True, order=True), "trace")
    d.close()


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_optional_outputs_may_be_null(precision):
    R = REAL[precision]
    s = rta.Scene.default(5, precision=precision)
    d = s.device()
    rng = np.random.default_rng(9)
    rays, tmax = ray_families(s, rng, 30)
    n = len(rays)
    order = rng.permutation(n).astype(np.uint32)
    lib, h = capi.lib, d._h
    p = lambda a: None if a is None else a.ctypes.data
    for optional in ((True, True), (True, False), (False, True), (False, False)):
        for mode in (capi.RT_QUERY_NEAREST, capi.RT_QUERY_ANY):
            outs = []
            for ordp in (None, "sort", order):
                dist = np.empty(n, R)
                nrm = np.empty((n, 3), R) if optional[0] else None
                item = np.empty(n, np.int32) if optional[1] else None
                if ordp is None:
                    rc = lib.rt_intersect_rays(h, mode, p(rays), p(tmax), n, p(dist), p(nrm), p(item), None)
                else:
                    rc = lib.rt_intersect_rays_ordered(h, mode, p(rays), p(tmax), n, None if isinstance(ordp, str) else p(ordp), p(dist), p(nrm), p(item), None)
                capi.check(rc, "rt_intersect_rays*")
                outs.append([x for x in (dist, nrm, item) if x is not None])
            same(outs[0], outs[1], ("nearest/any", optional, mode, "one call"))
            same(outs[0], outs[2], ("nearest/any", optional, mode, "permutation"))
    k = 4
    for optional in ((True, True, True), (False, False, False), (True, False, True), (False, True, False)):
        outs = []
        for ordp in (None, "sort", order):
            dist = np.empty((n, k), R)
            nrm = np.empty((n, k, 3), R) if optional[0] else None
            item = np.empty((n, k), np.int32) if optional[1] else None
            hits = np.empty(n, np.uint32) if optional[2] else None
            if ordp is None:
                rc = lib.rt_intersect_rays_multi(h, capi.RT_MULTIHIT_CLOSEST, k, p(rays), p(tmax), n, p(dist), p(nrm), p(item), p(hits), None)
            else:
                rc = lib.rt_intersect_rays_multi_ordered(h, capi.RT_MULTIHIT_CLOSEST, k, p(rays), p(tmax), n, None if isinstance(ordp, str) else p(ordp),
                                                         p(dist), p(nrm), p(item), p(hits), None)
            capi.check(rc, "rt_intersect_rays_multi*")
            outs.append([x for x in (dist, nrm, item, hits) if x is not None])
        same(outs[0], outs[1], ("multi", optional, "one call"))
        same(outs[0], outs[2], ("multi", optional, "permutation"))
    outs = []
    for ordp in (None, "sort", order):
        color = np.empty((n, 3), R)
        if ordp is None:
            rc = lib.rt_trace_rays(h, p(rays), n, p(color), None, None)
        else:
            rc = lib.rt_trace_rays_ordered(h, p(rays), n, None if isinstance(ordp, str) else p(ordp), p(color), None, None)
        capi.check(rc, "rt_trace_rays*")
        outs.append([color])
    same(outs[0], outs[1], "trace without alpha, one call")
    same(outs[0], outs[2], "trace without alpha, permutation")
    d.close()


def test_host_entries_reject_an_order_that_is_no_permutation_and_pinned_buffers_work():
    s = rta.Scene.default(5)
    d = s.device()
    rays, tmax = ray_families(s, np.random.default_rng(2), 20)
    n = len(rays)
    for bad in (np.zeros(n, np.uint32), np.arange(1, n + 1, dtype=np.uint32), np.full(n, 0xFFFFFFFF, np.int64)):
        for call in (lambda o: d.intersect(rays, tmax, order=o), lambda o: d.intersect_multi(rays, 4, tmax, order=o), lambda o: d.trace(rays, order=o)):
            with pytest.raises(rta.RtError) as e:
                call(bad)
            assert e.value.status == capi.RT_ERR_INVALID_ARGUMENT and "permutation" in str(e.value)
    for wraps in (np.full(n, -1, np.int64), np.arange(n, dtype=np.int64) + (1 << 32)):      # would wrap into range in a cast to uint32
        with pytest.raises(ValueError, match="order"):
            d.intersect(rays, tmax, order=wraps)
    r = rays.copy()
    r[3, 1] = np.nan
    with pytest.raises(rta.RtError) as e:
        d.ray_order(r)
    assert e.value.status == capi.RT_ERR_INVALID_ARGUMENT
    # pinned rays and a pinned order: read by the kernels in place
    hb = [capi.HostBuffer(k) for k in (rays.nbytes, 4 * n)]
    pr = hb[0].array.view(np.float32).reshape(n, 6)
    pr[:] = rays
    order = hb[1].array.view(np.uint32)
    rc = capi.lib.rt_ray_order(d._h, pr.ctypes.data, n, order.ctypes.data)
    capi.check(rc, "rt_ray_order")
    assert np.array_equal(order, np.argsort(rta.ray_keys(rays), kind="stable"))
    same(d.intersect(rays, tmax), d.intersect(pr, tmax, order=order), "pinned")
    d.close()
