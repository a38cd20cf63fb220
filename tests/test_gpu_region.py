"""Region overlap lists on the GPU (rt_overlap_regions / rt_overlap_regions_device, csrc/rt_region.hpp): every sphere of the
scene that reaches into each convex region of six planes, bit for bit against the walkers of tests/test_region_host.py -- the list
against the one-lane walk for every number of sections, the counters against the sectioned walk -- against the box lists where those can
answer, against the rays of a camera's own frame, and at the edges: NaN and absent planes, dead slots, an emptied scene, capacities, the
launch, scenes without bounds, threads, streams and dynamic scenes."""
import ctypes as C
import threading

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.scenes import random_nested_scene
from tests.test_gpu_box import boxes_for
from tests.test_gpu_camera import camera_sample_rays
from tests.test_gpu_near import CAPACITY, LEAF, LIGHT, EYE, cases, same_bytes, scene_of, spheres_of
from tests.test_gpu_overlap import counters, five_scenes, median_radius, queries_for, scale_of
from tests.test_gpu_query import REAL, bits
from tests.test_region_host import ABSENT, SCENES, Walker, carried_of, regions_for, unit_regions

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])


def host(x):
    """numpy from a result column, whichever side made it."""
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
        return x.view(np.uint64) if x.dtype == np.int64 else x
    return x


def assert_walk(d, w, margin, sections, what, ref=None, planes=None):
    """region_overlaps against the walkers: the list is the one-lane walk's (ref = w.all(margin), made once per margin), the counters the
    sectioned walk's at the J the library uses.  planes: what goes to the library in place of w.planes (the same values in other memory)."""
    items, gap, offsets, total, st = d.region_overlaps(w.planes if planes is None else planes, margin, sections=sections, gaps=True, offsets=True, stats=True)
    items, gap, offsets = host(items), host(gap), host(offsets)
    ref_i, ref_g, ref_o, _ = w.all(margin) if ref is None else ref
    np.testing.assert_array_equal(items, ref_i, err_msg=str(what))
    np.testing.assert_array_equal(bits(gap, w.R), bits(ref_g, w.R), err_msg=str(what))
    np.testing.assert_array_equal(offsets, ref_o, err_msg=str(what))
    assert int(total) == len(ref_i) == int(offsets[-1]), what
    J = rta.region_sections(len(w.planes), w.n_nodes, sections or 0)
    assert counters(st) == w.sectioned(margin, J)[3], (what, J)
    for g in range(len(w.planes)):                                               # ascending within a region
        assert (np.diff(items[int(offsets[g]):int(offsets[g + 1])]) > 0).all(), (what, g)
    return items, gap, offsets


# ---- 1: the walkers, bit for bit ----

@PRECISIONS
@pytest.mark.parametrize("name", SCENES)
def test_the_list_is_the_walks_and_the_counters_the_sections(precision, name):
    import torch
    s = five_scenes(precision)[name]
    d = rta.DeviceScene(s)
    w = Walker(s, regions_for(s, 24))
    assert w.carried.all()
    dp = torch.from_numpy(w.planes).cuda()
    side = torch.cuda.Stream()
    r, N = median_radius(s), w.n_nodes
    n_live = int(((s.items[:, 3] * s.items[:, 3]) > 0).sum())
    assert rta.region_sections(24, N) == max(1, N // 8)
    for margin in (0.0, r, -0.25 * r, 4.0 * r, np.inf, -np.inf):
        ref = w.all(margin)
        assert counters(d.region_overlaps(w.planes, margin, sections=1, stats=True)[2]) == ref[3]       # one section: the one-lane walk's counters
        for sections in (1, 2, 3, 64, 65, N, 0, None):
            items, gap, offsets = assert_walk(d, w, margin, sections, (name, margin, sections), ref)      # the same bytes for every J
        # the device entry: torch tensors, on a stream of its own
        assert_walk(d, w, margin, 3, (name, margin, "device"), ref, planes=dp)
        got = d.region_overlaps(dp, margin, sections=65, capacity=len(ref[0]), gaps=True, offsets=True, stream=side)
        side.synchronize()
        same_bytes(tuple(host(x) for x in got[:3]), ref[:3])
        assert int(got[3].item()) == len(ref[0])
        if margin == np.inf:
            assert (np.diff(offsets.astype(np.int64)) == n_live).all() and len(items) == 24 * n_live
        if margin == -np.inf:
            assert len(items) == 0
    d.close()


# ---- 2: the box lists ----

@PRECISIONS
def test_half_spaces_and_boxes_against_the_box_lists(precision):
    R = REAL[precision]
    inf = np.inf
    for name in ("refit", "clump", "default_L3"):
        s = five_scenes(precision)[name]
        d = rta.DeviceScene(s)
        sc, r = scale_of(s), median_radius(s)
        # a half-space as ONE plane, and as a box with five infinite sides: outside both metrics are the one excess minus the radius, inside
        # both are negative -- the same items at margins 0 and r
        planes, boxes = [], []
        for axis in range(3):
            for sign in (-1.0, 1.0):
                for a in (-0.7, -0.1, 0.0, 0.35, 0.9):
                    p = np.array([ABSENT] * 6)
                    p[0, axis], p[0, 3] = sign, -sign * a * sc                      # sign * (c - a) <= 0
                    lo, hi = np.full(3, -inf), np.full(3, inf)
                    (hi if sign > 0 else lo)[axis] = a * sc
                    planes.append(p)
                    boxes.append(np.concatenate([lo, hi]))
        planes, boxes = np.array(planes, R), np.ascontiguousarray(np.array(boxes, R))
        for margin in (0.0, r):
            got = d.region_overlaps(planes, margin, offsets=True)
            want = d.box_overlaps(boxes, margin, offsets=True)
            assert want[2] > 0
            same_bytes(got[:2], want[:2])
        # a finite box as six planes: region_gaps <= box_gaps, so its list holds the box list wherever that does not graze
        boxes = boxes_for(s, 60)
        planes = rta.box_planes(boxes[:, :3], boxes[:, 3:])
        bg = rta.box_gaps(boxes, s.items)
        n_items = len(s.items)
        for margin in (0.0, r):
            items, offsets, total = d.region_overlaps(planes, margin, offsets=True)
            b_items, b_offsets, b_total = d.box_overlaps(boxes, margin, offsets=True)
            key = lambda it, off: np.repeat(np.arange(len(boxes)), np.diff(off.astype(np.int64))) * n_items + it
            rows = np.repeat(np.arange(len(boxes)), np.diff(b_offsets.astype(np.int64)))
            clear = np.abs(bg[rows, b_items].astype(np.float64) - margin) > 1e-5 * sc
            assert clear.sum() > 0.9 * b_total > 0
            assert np.isin(key(b_items, b_offsets)[clear], key(items, offsets)).all(), (name, margin)
            assert total >= clear.sum()
        d.close()


# ---- 3: a camera's frame ----

@PRECISIONS
def test_everything_a_cameras_rays_hit_is_in_its_frustums_list(precision):
    R = REAL[precision]
    w, h = 32, 24
    s = five_scenes(precision)["default_L3"]
    d = rta.DeviceScene(s)
    n_items = len(s.items)
    views = (rta.look_at((2.0, 1.5, -4.5), (0.0, -0.5, 0.0), hfov_deg=60.0, precision=precision),        # outside the pyramid
             rta.look_at((0.05, -0.6, -0.1), (0.4, -1.0, 0.6), hfov_deg=90.0, precision=precision))       # inside it
    for v, cam in enumerate(views):
        for rect in (None, (12, 16, 20, 8)):
            l, t, r, b = (0, h, w, 0) if rect is None else rect
            ys, xs = (a.reshape(-1) for a in np.mgrid[b:t, l:r])
            seen = set()
            for spp, ssx, ssy in ((1, 0, 0), (2, 1, 1), (4, 3, 0)):
                rays = camera_sample_rays(w, h, spp, xs, ys, ssx, ssy, cam, R)
                _, _, item = d.intersect(rays)
                seen |= set(item[item >= 0].tolist())
            assert len(seen) > 0, (v, rect)
            items, total = d.region_overlaps(rta.camera_planes(cam, w, h, rect), 0.0)
            assert seen <= set(items.tolist()), (v, rect, sorted(seen - set(items.tolist())))
            if rect is not None:
                assert total < n_items or v == 1                                 # a rectangle of the outside view does not see everything
            # near and far planes in front of and behind everything seen change nothing; a far plane in front of the eye lists nothing
            wide = rta.camera_planes(cam, w, h, rect, near=1e-3, far=100.0)
            np.testing.assert_array_equal(d.region_overlaps(wide, 0.0)[0], items)
            assert d.region_overlaps(rta.camera_planes(cam, w, h, rect, far=-50.0), 0.0)[1] == 0
    d.close()


# ---- 4: regions that carry no query, absent planes, dead slots, an emptied scene ----

@PRECISIONS
def test_nan_regions_absent_planes_dead_slots_and_an_emptied_scene(precision):
    import torch
    R = REAL[precision]
    s = five_scenes(precision)["refit"]
    d = rta.DeviceScene(s)
    planes = regions_for(s, 9)
    planes[2, 3, 1] = np.nan                                                     # a NaN normal component
    planes[5, 0, 3] = np.nan                                                     # a NaN d
    planes[7] = np.nan
    planes[4] = ABSENT                                                           # six absent planes: every live sphere
    w = Walker(s, planes)
    assert w.carried.tolist() == [True, True, False, True, True, False, True, False, True]
    with pytest.raises(rta.RtError) as err:                                      # the host entry refuses a NaN, with its place
        d.region_overlaps(planes)
    assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and "region 2, plane 3" in str(err.value)
    dp = torch.from_numpy(planes).cuda()
    n_live = len(s.items)
    for margin in (0.0, median_radius(s), np.inf):
        for sections in (1, 7, 0):
            items, gap, offsets = assert_walk(d, w, margin, sections, (margin, sections), planes=dp)     # (primary = 6: the walker's)
            rows = np.diff(offsets.astype(np.int64))
            assert (rows[~w.carried] == 0).all() and rows[4] == n_live
            np.testing.assert_array_equal(items[int(offsets[4]):int(offsets[5])], np.arange(n_live))
    d.close()
    # dead slots after update(live=) are never listed, at +inf and through six absent planes too; the emptied scene makes one test per region
    ranges = rta.balanced_ranges(CAPACITY, LEAF)
    sp = spheres_of(3, R, spread=2.0)
    d = rta.DeviceScene(rta.Scene.from_spheres_balanced(sp, leaf_size=LEAF, precision=precision), 0, True)
    planes = np.ascontiguousarray(unit_regions(20, 92).astype(R))
    planes[3] = ABSENT
    live = (np.random.default_rng(4).random(CAPACITY) < 0.5).astype(np.uint8)
    live[:8] = 0
    garbage = sp.copy()
    garbage[live == 0] = np.nan                                                  # a dead slot may hold any bits
    d.update(garbage, live=live)
    fresh = scene_of(np.where(live[:, None] != 0, sp, 0).astype(R), d.bounds(), ranges, precision)
    w = Walker(fresh, planes)
    dead = np.flatnonzero(live == 0)
    for margin in (0.0, 0.1, np.inf):
        for sections in (1, 5, 0):
            items, _, offsets = assert_walk(d, w, margin, sections, ("half dead", margin, sections))
            assert not np.isin(items, dead).any()
        assert np.diff(offsets.astype(np.int64))[3] == int(live.sum())
    d.rebuild(sp, n=0)
    empty = Walker(scene_of(np.zeros((CAPACITY, 4), R), d.bounds(), ranges, precision), planes)
    for margin in (0.0, np.inf):
        items, offsets, total, st = d.region_overlaps(planes, margin, sections=1, offsets=True, stats=True)
        assert total == 0 and len(items) == 0 and not offsets.any() and len(offsets) == len(planes) + 1
        assert counters(st) == empty.all(margin)[3]
        assert st["bound_tests"] == len(planes) and st["sphere_tests"] == 0 and st["primary"] == len(planes) and st["hits"] == 0
        assert_walk(d, empty, margin, 0, ("emptied", margin))                    # (every section's descent tests the dead root: the walker says so too)
    d.close()


# ---- 5: capacities ----

def raw(d, planes, margin, sections, capacity, items, gap, offsets, entry="host", stream=None):
    """One call of the C entry with the caller's own buffers (numpy arrays for "host", torch tensors for "device"); None: NULL -> total."""
    ptr = lambda x: None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data)
    n = len(planes)
    if entry == "host":
        total = C.c_uint64(0)
        capi.check(capi.lib.rt_overlap_regions(d._h, ptr(planes), n, margin, sections, capacity, ptr(items), ptr(gap), ptr(offsets), C.byref(total), None),
                   "rt_overlap_regions")
        return int(total.value)
    import torch
    total = torch.full((), -1, dtype=torch.int64, device="cuda")
    qs = torch.cuda.current_stream() if stream is None else stream
    capi.check(capi.lib.rt_overlap_regions_device(d._h, ptr(planes), n, margin, sections, capacity, ptr(items), ptr(gap), ptr(offsets), ptr(total), None,
                                                  C.c_void_p(qs.cuda_stream)), "rt_overlap_regions_device")
    qs.synchronize()
    return int(total.item())


@PRECISIONS
def test_every_capacity_gets_the_exact_prefix(precision):
    import torch
    R = REAL[precision]
    s = cases(precision)["refit"]
    d = rta.DeviceScene(s)
    planes = regions_for(s, 30)
    n = len(planes)
    margin = median_radius(s)
    ref_i, ref_g, ref_o, total = d.region_overlaps(planes, margin, sections=1, gaps=True, offsets=True)
    assert total > 16 and len(ref_i) == total
    dp = torch.from_numpy(planes).cuda()
    GUARD = 16
    for capacity in (0, 1, total - 1, total, total + 1):
        for with_items in (True, False):
            for entry, sections in (("host", 0), ("device", 70), ("host", 3)):     # 70: two waves per region, the second partly filled
                items = np.full(capacity + GUARD, -77, np.int32)
                gap = np.full(capacity + GUARD, -77.0, R)
                offsets = np.full(n + 1 + GUARD, 77, np.uint64)
                if entry == "device":
                    items, gap, offsets = (torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (items, gap, offsets))
                got = raw(d, dp if entry == "device" else planes, margin, sections, capacity, items if with_items else None, gap if with_items else None, offsets, entry)
                items, gap, offsets = host(items), host(gap), host(offsets)
                what = (capacity, with_items, entry, sections)
                assert got == total, what
                np.testing.assert_array_equal(offsets[:n + 1], ref_o, err_msg=str(what))
                assert (offsets[n + 1:] == 77).all(), what
                m = min(capacity, total) if with_items else 0
                np.testing.assert_array_equal(items[:m], ref_i[:m], err_msg=str(what))
                np.testing.assert_array_equal(bits(gap[:m], R), bits(ref_g[:m], R), err_msg=str(what))
                assert (items[m:] == -77).all() and (gap[m:] == -77.0).all(), what      # nothing behind the list, the guard words included
    items = np.full(total, -77, np.int32)                                        # items without gaps at a short capacity
    assert raw(d, planes, margin, 5, total - 5, items, None, None) == total
    np.testing.assert_array_equal(items[:total - 5], ref_i[:total - 5])
    assert (items[total - 5:] == -77).all()
    for capacity in (0, 1, total - 1, total, total + 1):                         # through the wrapper
        items, gap, got = d.region_overlaps(planes, margin, capacity=capacity, gaps=True)
        m = min(capacity, total)
        assert got == total and len(items) == m == len(gap)
        np.testing.assert_array_equal(items, ref_i[:m])
        np.testing.assert_array_equal(bits(gap, R), bits(ref_g[:m], R))
    d.close()


# ---- 6: the launch -- n = 1, 64, 65, a J that is no multiple of 64 -- and scenes without bounds ----

@PRECISIONS
def test_the_edges_of_the_launch_and_scenes_without_bounds(precision):
    R = REAL[precision]
    s = cases(precision)["refit"]
    d = rta.DeviceScene(s)
    every = regions_for(s, 65)
    w = Walker(s, every)
    margin = median_radius(s)
    ref_i, ref_g, ref_o, _ = w.all(margin)
    for n in (1, 64, 65):
        for sections in (1, 63, 64, 65, 100, 129, w.n_nodes, w.n_nodes + 1000, 0):
            items, gap, offsets, total = d.region_overlaps(every[:n], margin, sections=sections, gaps=True, offsets=True)
            m = int(ref_o[n])
            assert total == m, (n, sections)
            np.testing.assert_array_equal(items, ref_i[:m], err_msg=str((n, sections)))
            np.testing.assert_array_equal(bits(gap, R), bits(ref_g[:m], R), err_msg=str((n, sections)))
            np.testing.assert_array_equal(offsets, ref_o[:n + 1], err_msg=str((n, sections)))
    w1 = Walker(s, every[:1])
    assert_walk(d, w1, margin, 100, "one region, 100 sections")
    d.close()
    # without bounds the stream is the items: every item is tested once whatever J is, and the list is brute force's
    light = rta.normalized(LIGHT, precision)
    it, _, _ = random_nested_scene(3)
    for items0 in (it, it[:10], it[:1]):
        s = rta.Scene(items0, light, EYE, precision=precision)
        d = s.device()
        planes = regions_for(s, 20)
        n, m = len(planes), len(s.items)
        gap = rta.region_gaps(planes, s.items)
        for margin in (0.0, median_radius(s), 1.5, -0.5, np.inf, -np.inf):
            listed = ~(gap >= R(margin))
            for sections in (1, 3, m, 0):
                got, got_gap, offsets, total, st = d.region_overlaps(planes, margin, sections=sections, gaps=True, offsets=True, stats=True)
                np.testing.assert_array_equal(got, np.nonzero(listed)[1])
                np.testing.assert_array_equal(bits(got_gap, R), bits(gap[listed], R))
                assert total == listed.sum() == offsets[-1]
                np.testing.assert_array_equal(np.diff(offsets.astype(np.int64)), listed.sum(axis=1))
                assert st["bound_tests"] == 0 and st["sphere_tests"] == n * m and st["primary"] == n and st["hits"] == int(listed.any(axis=1).sum())
        d.close()


# ---- 7: threads, streams, pinned buffers, device memory refused, dynamic scenes ----

def test_entries_buffers_streams_and_threads_agree():
    import torch
    s = cases(rta.RT_F32)["refit"]
    d = rta.DeviceScene(s)
    planes = regions_for(s, 40)
    n = len(planes)
    margin = median_radius(s)
    ref = d.region_overlaps(planes, margin, gaps=True, offsets=True, stats=True)
    total = ref[3]
    assert total > 0
    same_bytes(ref[:3], d.region_overlaps(planes, margin, gaps=True, offsets=True)[:3])              # two runs, with and without counters
    dp = torch.from_numpy(planes).cuda()
    dev = d.region_overlaps(dp, margin, gaps=True, offsets=True)
    assert all(x.device.type == "cuda" for x in dev[:3]) and dev[3] == total
    same_bytes(ref[:3], dev[:3])
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    a = d.region_overlaps(dp, margin, capacity=total, gaps=True, offsets=True, stream=side)
    b = d.region_overlaps(dp, margin, capacity=total, gaps=True, offsets=True, stats=True, stream=side.cuda_stream)
    c = d.region_overlaps(dp, 0.0, sections=9, capacity=total, stream=other)     # another margin and J on another stream, in between
    e = d.region_overlaps(dp, margin, sections=200, capacity=total, gaps=True, offsets=True)
    side.synchronize()
    other.synchronize()
    torch.cuda.synchronize()
    for got in (a, b, e):
        same_bytes(ref[:3], got[:3])
        assert int(got[3].item()) == total
    assert counters(b[4]) == counters(ref[4])
    zero = d.region_overlaps(planes, 0.0)
    assert int(c[1].item()) == zero[1] and np.array_equal(c[0].cpu().numpy()[:zero[1]], zero[0])
    # pinned host buffers (read and written by the kernels directly) against pageable ones
    hb = [capi.HostBuffer(x) for x in (96 * n, 4 * total, 4 * total, 8 * (n + 1))]
    pp, items, gap, offsets = hb[0].array.view(np.float32).reshape(n, 24), hb[1].array.view(np.int32), hb[2].array.view(np.float32), hb[3].array.view(np.uint64)
    pp[:] = planes.reshape(n, 24)
    assert raw(d, pp, margin, 0, total, items, gap, offsets) == total
    same_bytes(ref[:3], (items, gap, offsets))
    # a buffer in device memory is refused by the host entry
    t = torch.zeros(total, dtype=torch.int32, device="cuda")
    with pytest.raises(rta.RtError) as err:
        raw(d, planes, margin, 0, total, t, None, None)
    assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and "device memory" in str(err.value)
    with pytest.raises(rta.RtError) as err:                                      # n * J above 2^26, before anything is enqueued
        raw(d, np.zeros(((1 << 20) + 1, 24), np.float32), margin, 64, 0, None, None, None)            # (never read: the check comes first)
    assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and "2^26" in str(err.value)
    # two threads on one scene at once: one lists regions, the other spheres -- they share the workspace, which the regions grow
    queries = queries_for(s)
    spheres = d.overlaps(queries, 2 * margin, gaps=True, offsets=True)
    many = d.region_overlaps(planes, margin, sections=w_nodes(s), gaps=True, offsets=True)
    same_bytes(ref[:3], many[:3])
    results, errors = [None] * 2, []

    def work(k):
        try:
            for _ in range(5):
                results[k] = d.overlaps(queries, 2 * margin, gaps=True, offsets=True) if k else d.region_overlaps(planes, margin, sections=w_nodes(s), gaps=True, offsets=True)
        except Exception as ex:          # noqa: BLE001 (reported below)
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k, r in enumerate(results):
        same_bytes((spheres if k else many)[:3], r[:3])
        assert r[3] == (spheres if k else many)[3]
    d.close()


def w_nodes(s):
    from tests.test_gpu_multihit import node_stream
    return len(node_stream(s))


@PRECISIONS
def test_a_call_between_the_updates_of_a_dynamic_scene(precision):
    R = REAL[precision]
    ranges = rta.balanced_ranges(CAPACITY, LEAF)
    d = rta.DeviceScene(rta.Scene.from_spheres_balanced(spheres_of(1, R), leaf_size=LEAF, precision=precision), 0, True)
    planes = np.ascontiguousarray(unit_regions(20, 93).astype(R))
    for step, sp in enumerate((spheres_of(1, R), spheres_of(2, R), spheres_of(3, R, spread=2.0))):
        if step == 1:
            d.update(sp)
        if step == 2:
            sp = sp[d.rebuild(sp)]
        w = Walker(scene_of(sp, d.bounds(), ranges, precision), planes)
        for margin in (0.0, float(np.median(sp[:, 3]))):
            for sections in (1, 0, 33):
                assert_walk(d, w, margin, sections, (step, margin, sections))
    d.close()
