"""Ray queries on the GPU (rt_intersect_rays / rt_intersect_rays_device, csrc/rt_query.hpp): TypedGroup::intersect for arbitrary rays,
bit for bit against the oracle's restatement of it, and tied at frame scale to the render's counters (which are pinned to the oracle)."""
import threading

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests import util
from tests.edge_scenes import sample_rays
from tests.scenes import hundred_thousand_spheres, random_nested_scene

pytestmark = pytest.mark.gpu

PREC = {rta.RT_F32: oracle.F32, rta.RT_F64: oracle.F64}
REAL = {rta.RT_F32: np.float32, rta.RT_F64: np.float64}
SKIP = rta.RT_TRAVERSAL_SKIP


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def ray_families(scene, rng, n_each=40):
    """(rays REAL[n, 6], tmax REAL[n]): origins outside / inside the root bound, inside inner bounds, on sphere surfaces; directions random,
    aimed at items, and pointing away from everything; tmax +inf, finite, 0 and negative."""
    items = scene.items.astype(np.float64)
    if scene.bounds is not None and len(scene.bounds):
        bounds = scene.bounds.astype(np.float64)
    else:
        c = items[:, :3].mean(axis=0)
        bounds = np.array([[c[0], c[1], c[2], np.max(np.linalg.norm(items[:, :3] - c, axis=1) + items[:, 3])]])
    root_c, root_r = bounds[0, :3], bounds[0, 3]
    o, d = [], []

    def add(origins, dirs):
        o.append(np.asarray(origins, dtype=np.float64).reshape(-1, 3))
        d.append(_unit(np.asarray(dirs, dtype=np.float64).reshape(-1, 3)))

    pick = lambda k: items[rng.integers(0, len(items), k)]
    outside = root_c + _unit(rng.normal(size=(n_each, 3))) * root_r * rng.uniform(1.2, 3.0, (n_each, 1))
    add(outside, pick(n_each)[:, :3] - outside)                                                    # outside the root, aimed at items
    add(outside, rng.normal(size=(n_each, 3)))                                                     # ... random directions
    add(outside, outside - root_c)                                                                 # ... pointing away from everything
    inside = root_c + _unit(rng.normal(size=(n_each, 3))) * root_r * rng.uniform(0.0, 0.9, (n_each, 1))
    add(inside, rng.normal(size=(n_each, 3)))                                                      # inside the root bound
    add(inside, pick(n_each)[:, :3] - inside)
    inner = bounds[rng.integers(0, len(bounds), n_each)]
    ib = inner[:, :3] + _unit(rng.normal(size=(n_each, 3))) * inner[:, 3:] * rng.uniform(0.0, 0.5, (n_each, 1))
    add(ib, rng.normal(size=(n_each, 3)))                                                          # inside inner bounds
    s = pick(n_each)
    surf = s[:, :3] + _unit(rng.normal(size=(n_each, 3))) * s[:, 3:]
    add(surf, rng.normal(size=(n_each, 3)))                                                        # on sphere surfaces
    rays = np.concatenate([np.concatenate(o), np.concatenate(d)], axis=1)
    R = REAL[scene.precision]
    rays = rays.astype(R)
    n = len(rays)
    choice = rng.integers(0, 4, n)
    nearest = 0.2 if 2.5 * root_r > 0.2 else 0.08 * root_r         # (a scene far below unit size, tests/scaled_scenes.py: sized by its root as well)
    tmax = np.where(choice == 0, np.inf, np.where(choice == 1, rng.uniform(nearest, 2.5 * root_r, n), np.where(choice == 2, 0.0, -1.0))).astype(R)
    return rays, tmax


def oracle_nearest(o, rays, tmax, mode=oracle.MODE_HIERARCHY):
    out = [o.intersect(r.astype(np.float64), float(t), mode) for r, t in zip(rays, tmax)]
    return np.array([x[0] for x in out]), np.array([x[1] for x in out])


def scene_cases(precision):
    """(name, rta.Scene, oracle.Scene) for every parity scene."""
    R = REAL[precision]
    out = []
    for level in (3, 8):
        s, o = util.scene_pair_default(precision, level)
        out.append(("default_L%d" % level, s, o))
    spheres3 = [(0.0, -1.0, 0.0, 1.0), (-1.2, 0.2, 0.0, 0.5), (1.2, 0.2, 0.0, 0.5)]
    out.append(("three_spheres",) + util.scene_pair_spheres(spheres3, (0.0, -1.0, 0.0, 3.0), precision))
    for conc in (False, True):
        it, bd, rg = random_nested_scene(7 + conc, concentric=conc)
        out.append(("nested_conc%d" % conc,) + util.scene_pair_ranges(it, bd, rg, precision))
    sp = hundred_thousand_spheres()
    s = rta.Scene.from_spheres_auto(sp, precision=precision)
    o = oracle.Scene.from_ranges(s.items.astype(np.float64), s.bounds.astype(np.float64), s.ranges, prec=PREC[precision])
    out.append(("100k", s, o))
    assert all(c[1].items.dtype == R for c in out)
    return out


def bits(a, R):
    a = np.ascontiguousarray(np.asarray(a, dtype=R))
    return a.view(np.uint32 if R == np.float32 else np.uint64)


def check_nearest(s, o, rays, tmax, mode=oracle.MODE_HIERARCHY):
    R = REAL[s.precision]
    dist, nrm, item = s.device().intersect(rays, tmax)
    ref_d, ref_n = oracle_nearest(o, rays, tmax, mode)
    np.testing.assert_array_equal(bits(dist, R), bits(ref_d, R))
    np.testing.assert_array_equal(bits(nrm, R), bits(ref_n, R))
    hit = item >= 0
    np.testing.assert_array_equal(hit, dist.astype(np.float64) < tmax.astype(np.float64))
    np.testing.assert_array_equal(bits(dist[~hit], R), bits(tmax[~hit], R))
    for k in np.flatnonzero(hit):          # the reported item reproduces the hit on its own
        d1, n1 = oracle.sphere_intersect(s.items[item[k]].astype(np.float64), rays[k].astype(np.float64), float("inf"), PREC[s.precision])
        assert R(d1) == dist[k] and np.array_equal(bits(n1, R), bits(nrm[k], R)), k
    return dist, item


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_nearest_and_any_match_the_oracle_ray_for_ray(precision):
    rng = np.random.default_rng(11 + precision)
    for name, s, o in scene_cases(precision):
        rays, tmax = ray_families(s, rng, 12 if name == "100k" else 40)
        ref_d, item = check_nearest(s, o, rays, tmax)
        # ANY: "something closer than tmax" is the nearest query's own answer; the reported item is closer than tmax
        R = REAL[precision]
        ad, an, ai = s.device().intersect(rays, tmax, any_hit=True)
        found = ai >= 0
        np.testing.assert_array_equal(found, ref_d.astype(np.float64) < tmax.astype(np.float64), err_msg=name)
        np.testing.assert_array_equal(found, ad.astype(np.float64) < tmax.astype(np.float64), err_msg=name)
        np.testing.assert_array_equal(bits(ad[~found], R), bits(tmax[~found], R), err_msg=name)
        assert not an[~found].any()
        for k in np.flatnonzero(found):
            d1, _ = oracle.sphere_intersect(s.items[ai[k]].astype(np.float64), rays[k].astype(np.float64), float("inf"), PREC[precision])
            assert R(d1) == ad[k] and d1 < tmax[k], (name, k)
        s.device().close()


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_tangent_ties_and_scenes_without_bounds(precision):
    R = REAL[precision]
    # a zero discriminant: from (0, 0, -4) along +z the sphere (0.5, 0, -2) r 0.5 is grazed at t = 2 (test_gpu_parity's tangent ray)
    s, o = util.scene_pair_spheres([(0.5, 0.0, -2.0, 0.5), (-3.0, 2.0, 1.0, 0.75)], (0.0, 0.0, 0.0, 6.0), precision)
    rays = np.array([(0, 0, -4, 0, 0, 1), (0, 0, -4, 0, 0, -1), (0.5, 0.0, -2.5, 0, 0, 1)], dtype=R)
    tmax = np.array([np.inf, np.inf, 3.0], dtype=R)
    dist, _ = check_nearest(s, o, rays, tmax)
    assert dist[0] == 2.0
    # two bit-identical spheres: the lower DFS index wins (strict `<`, primitive.rs:79)
    twins = [(3.0, 0.0, 0.0, 0.5), (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 1.0)]
    s, o = util.scene_pair_spheres(twins, (0.0, 0.0, 0.0, 6.0), precision)
    rays = np.array([(0, 0, -5, 0, 0, 1), (0, 0, 5, 0, 0, -1), (0.3, 0.2, -5, 0, 0, 1)], dtype=R)
    _, item = check_nearest(s, o, rays, np.full(3, np.inf, dtype=R))
    assert list(item) == [1, 1, 1]
    # a scene created without bounds: the flat nearest hit over all items in DFS order
    it, bd, rg = random_nested_scene(3)
    flat = rta.Scene(it, rta.normalized((-1.0, -3.0, 2.0), precision), (0.0, 0.0, -4.0), precision=precision)
    o = oracle.Scene.from_ranges(it, bd, rg, prec=PREC[precision])
    rays, tmax = ray_families(flat, np.random.default_rng(5))
    dist, nrm, item = flat.device().intersect(rays, tmax)
    ref = [o.intersect(r.astype(np.float64), float(t), oracle.MODE_FLAT) for r, t in zip(rays, tmax)]
    np.testing.assert_array_equal(bits(dist, R), bits([x[0] for x in ref], R))
    np.testing.assert_array_equal(bits(nrm, R), bits([x[1] for x in ref], R))
    assert (item >= 0).any() and (item < 0).any()


def camera_rays(w, h, eye, spp=1, prec=oracle.F32):
    """The render's primary rays (render.rs:231-241), one per pixel and sample, in the order y, x, ssx, ssy (tests/edge_scenes.py
    sample_rays, the one restatement of the sample ray)."""
    y, x, sx, sy = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), np.arange(spp), indexing="ij")
    return sample_rays(w, h, spp, x, y, sx, sy, eye, prec).reshape(-1, 6)


@pytest.mark.parametrize("w,h", [(1920, 1080), (800, 600), (1024, 768)])
def test_two_queries_make_the_frames_counters(w, h):
    f = np.float32
    s = rta.Scene.default()
    d = s.device()
    _, st = d.render_tiles((w, h, 1), [(0, h, w, 0)], SKIP, want_stats=True)
    rays = camera_rays(w, h, s.eye)
    dist, nrm, item, qs = d.intersect(rays, want_stats=True)
    hit = item >= 0
    assert qs["primary"] == w * h and qs["hits"] == int(hit.sum()) == st["hits"]
    assert qs["sphere_tests"] + qs["bound_tests"] == qs["tests_executed"] == st["primary_tests"]
    # the shadow rays, render.rs:190-207: where n.light < 0, from (pos + dir*d) + n*(d*sqrt(EPSILON)) along -light
    light = s.directional_light
    g = (nrm[:, 0] * light[0] + nrm[:, 1] * light[1]) + nrm[:, 2] * light[2]
    sh = hit & (g < f(0))
    dd = dist[sh][:, None]
    p = (rays[sh, :3] + rays[sh, 3:] * dd) + nrm[sh] * (dd * np.sqrt(np.finfo(f).eps))
    srays = np.concatenate([p, np.broadcast_to(-light, p.shape)], axis=1).astype(f)
    assert len(srays) == st["shadow"]
    _, _, sitem, ss = d.intersect(srays, any_hit=True, want_stats=True)
    assert int((sitem >= 0).sum()) == ss["hits"] == st["occluded"]
    assert ss["sphere_tests"] + ss["bound_tests"] == st["sphere_tests"] + st["bound_tests"] - st["primary_tests"]


def test_entries_flavours_buffers_and_threads_agree():
    import torch
    s = rta.Scene.default()
    d = s.device()
    rays, tmax = ray_families(s, np.random.default_rng(3), 200)
    for any_hit in (False, True):
        ref = d.intersect(rays, tmax, any_hit=any_hit)
        counted = d.intersect(rays, tmax, any_hit=any_hit, want_stats=True)
        for a, b in zip(ref, counted):
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
        # the device entry, torch tensors on a stream of their own
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            tr, tt = torch.from_numpy(rays).cuda(), torch.from_numpy(tmax).cuda()
            dev = d.intersect(tr, tt, any_hit=any_hit, stream=stream)
        stream.synchronize()
        for a, b in zip(ref, dev):
            assert b.device.type == "cuda"
            np.testing.assert_array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))
        # pinned host buffers (read and written by the kernel directly) against pageable ones
        n = len(rays)
        hb = [capi.HostBuffer(k) for k in (rays.nbytes, tmax.nbytes, 4 * n, 12 * n, 4 * n)]
        pr, pt = hb[0].array.view(np.float32).reshape(n, 6), hb[1].array.view(np.float32)
        pr[:], pt[:] = rays, tmax
        out = (hb[2].array.view(np.float32), hb[3].array.view(np.float32).reshape(n, 3), hb[4].array.view(np.int32))
        pinned = d.intersect(pr, pt, any_hit=any_hit, out=out)
        for a, b in zip(ref, pinned):
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    # four threads on one scene at once
    ref = d.intersect(rays, tmax)
    results, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(5):
                results[k] = d.intersect(rays, tmax)
        except Exception as e:          # noqa: BLE001 (reported below)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for r in results:
        for a, b in zip(ref, r):
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_the_host_entry_rejects_rays_outside_the_domain(precision):
    R = REAL[precision]
    d = rta.Scene.three_spheres(precision).device()
    good = np.array([[0, 0, -4, 0, 0, 1]] * 4, dtype=R)
    d.intersect(good)
    bad_rays = []
    for k, v in ((1, np.nan), (5, np.inf), (0, 2e15)):
        r = good.copy(); r[2, k] = v; bad_rays.append(r)
    r = good.copy(); r[1, 3:] = (0, 0, 1.01); bad_rays.append(r)            # squared length 1.0201
    for r in bad_rays:
        with pytest.raises(rta.RtError) as e:
            d.intersect(r)
        assert e.value.status == capi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(rta.RtError) as e:
        d.intersect(good, np.array([1, np.nan, 1, 1], dtype=R))
    assert e.value.status == capi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        d.intersect(good.astype(np.float64 if R == np.float32 else np.float32))
    with pytest.raises(ValueError):
        d.intersect(good[:, :5])


def test_device_entry_on_a_stream_that_is_not_the_current_one():
    # the query waits for the inputs the caller made on the current stream, and the memory it uses stays its own while it runs: a scalar
    # tmax (an ambient-occlusion radius), a torch stream and a raw handle that are not the current stream, inputs dropped right away and
    # the current stream's allocations reusing what they can -- every result equals the host entry's
    import torch
    s = rta.Scene.default()
    d = s.device()
    rays, _ = ray_families(s, np.random.default_rng(9), 300)
    radius = 1.5                                              # a Python float: rounded to the scene's REAL
    ref = d.intersect(rays, np.full(len(rays), radius, dtype=np.float32))
    for a, b in zip(ref, d.intersect(rays, radius)):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    ref_any = d.intersect(rays, radius, any_hit=True)
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    results = []
    for k in range(4):
        big = torch.randn(4096, 4096, device="cuda")          # keeps the current stream busy while the inputs are made behind it
        big = big @ big
        tr = torch.from_numpy(rays).cuda() * 1.0              # made on the current stream
        stream = side if k % 2 == 0 else side.cuda_stream
        tmax = radius if k < 2 else torch.tensor(radius, dtype=torch.float64)
        results.append((d.intersect(tr, tmax, stream=stream), d.intersect(tr, tmax, any_hit=True, stream=stream)))
        del tr, big
        torch.full((len(rays), 6), float("nan"), device="cuda")    # the current stream's next allocations
    side.synchronize()
    for near, anyh in results:
        for a, b in zip(ref, near):
            np.testing.assert_array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))
        for a, b in zip(ref_any, anyh):
            np.testing.assert_array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))


def test_the_first_query_of_a_scene_without_bounds_on_a_side_stream():
    # the items-only stream is derived on the first query's stream; a host query right behind it (another stream) waits for it
    import torch
    it, _, _ = random_nested_scene(4)
    flat = rta.Scene(it, rta.normalized((-1.0, -3.0, 2.0)), (0.0, 0.0, -4.0))
    rays, tmax = ray_families(flat, np.random.default_rng(6))
    d = flat.device()
    side = torch.cuda.Stream()
    dev = d.intersect(torch.from_numpy(rays).cuda(), torch.from_numpy(tmax).cuda(), stream=side)
    host = d.intersect(rays, tmax)
    side.synchronize()
    for a, b in zip(host, dev):
        np.testing.assert_array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))
    assert (host[2] >= 0).any()
