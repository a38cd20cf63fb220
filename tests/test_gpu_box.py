"""Box overlap lists on the GPU (rt_overlap_boxes / rt_overlap_boxes_device, csrc/rt_box.hpp): every sphere of the scene
within a margin of each axis-aligned query box, bit for bit against a restatement of the walk over the scene's node stream with
rta.box_gaps as its metric, against brute force wherever no gap grazes the margin, against the overlap lists where a box is a point, for
infinite, inverted and NaN boxes, and at the edges of the launch, the scan and the capacity."""
import ctypes as C
import threading

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.scenes import random_nested_scene
from tests.test_gpu_multihit import node_stream
from tests.test_gpu_near import CAPACITY, LEAF, LIGHT, EYE, cases, same_bytes, scene_of, spheres_of
from tests.test_gpu_overlap import COUNTERS, Walker as OverlapWalker, counters, five_scenes, median_radius, queries_for, scale_of
from tests.test_gpu_query import REAL, bits

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
MARGINS = (("0", lambda r: 0.0), ("r", lambda r: r), ("-r/4", lambda r: -0.25 * r), ("4r", lambda r: 4.0 * r))


def unit_boxes(n, seed):
    """float64[n, 6]: centres uniform in +-1.2, half-extents uniform in [0, 0.3] per axis; rows 0::10 are point boxes (half-extent 0), rows
    5::10 have an x half-extent of 2.5: a slab across a scene of unit size."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.2, 1.2, (n, 3))
    h = rng.uniform(0.0, 0.3, (n, 3))
    h[0::10] = 0.0
    h[5::10, 0] = 2.5
    return np.concatenate([c - h, c + h], axis=1)


def boxes_for(s, n=200, seed=78):
    """n query boxes, unit_boxes scaled to the scene's extent, in the scene's REAL."""
    return np.ascontiguousarray((unit_boxes(n, seed) * scale_of(s)).astype(REAL[s.precision]))


def carried_of(boxes):
    with np.errstate(invalid="ignore"):
        return (boxes[:, :3] <= boxes[:, 3:]).all(axis=1)                       # (NaN fails the comparison)


class Walker(OverlapWalker):
    """The definition of the box walk (include/rtrace_hip.h): tests/test_gpu_overlap.py's Walker -- one query at a time over node_stream(s)
    from node 0 -- with rta.box_gaps as the metric and lo <= hi on every axis as "carried"."""

    def __init__(self, s, boxes):
        self.R = R = REAL[s.precision]
        nodes = node_stream(s)
        self.bound = [x[1] for x in nodes]
        self.skip = [x[2] for x in nodes]
        self.item = [x[3] for x in nodes]
        self.node_of = {x[3]: k for k, x in enumerate(nodes) if not x[1]}
        self.queries = self.boxes = b = np.asarray(boxes, dtype=R)
        records = np.array([x[0] for x in nodes], dtype=np.float64).reshape(-1, 4).astype(R)         # (exact: they were REAL)
        self.gaps = [row.tolist() for row in rta.box_gaps(b, records)] if len(nodes) else [[] for _ in b]
        self.carried = carried_of(b)


def assert_walk(d, w, margin, what, exclude=None, boxes=None):
    """box_overlaps against the walker; boxes: what goes to the library in place of w.boxes (the same values in other memory)."""
    items, gap, offsets, total, st = d.box_overlaps(w.boxes if boxes is None else boxes, margin, exclude=exclude, gaps=True, offsets=True, stats=True)
    if hasattr(items, "cpu"):
        items, gap, offsets = items.cpu().numpy(), gap.cpu().numpy(), offsets.cpu().numpy().view(np.uint64)
    ref_i, ref_g, ref_o, ref_st = w.all(margin, None if exclude is None else np.asarray(exclude.cpu() if hasattr(exclude, "cpu") else exclude))
    np.testing.assert_array_equal(items, ref_i, err_msg=str(what))
    np.testing.assert_array_equal(bits(gap, w.R), bits(ref_g, w.R), err_msg=str(what))
    np.testing.assert_array_equal(offsets, ref_o, err_msg=str(what))
    assert int(total) == len(ref_i) == int(offsets[-1]), what
    assert counters(st) == ref_st, what
    for g in range(len(w.boxes)):                                                # ascending within a box
        assert (np.diff(items[int(offsets[g]):int(offsets[g + 1])]) > 0).all(), (what, g)
    return items, gap, offsets


# ---- 1 ----

@PRECISIONS
def test_the_list_restates_the_walk_bit_for_bit(precision):
    for name, s in five_scenes(precision).items():
        d = rta.DeviceScene(s)
        w = Walker(s, boxes_for(s))
        assert w.carried.all()
        r = median_radius(s)
        n_live = int(((s.items[:, 3] * s.items[:, 3]) > 0).sum())
        for margin in (0.0, r, -0.25 * r, 4.0 * r, np.inf, -np.inf):
            items, gap, offsets = assert_walk(d, w, margin, (name, margin))
            if margin == np.inf:
                assert (np.diff(offsets.astype(np.int64)) == n_live).all() and len(items) == len(w.boxes) * n_live
            if margin == -np.inf:
                assert len(items) == 0
        d.close()


# ---- 2 ----

def brute_force(s, boxes, margin):
    """(gap[n, m], listed, grazing): an entry may be left out only if its gap lies within 1e-5 max(scale, |gap|) (f64: 1e-12) of the margin."""
    R = REAL[s.precision]
    gap = rta.box_gaps(boxes, s.items)
    m = R(margin)
    listed = ~(gap >= m)
    eps = 1e-5 if R == np.float32 else 1e-12
    g = gap.astype(np.float64)
    with np.errstate(invalid="ignore"):
        grazing = np.abs(g - float(m)) <= eps * np.maximum(scale_of(s), np.abs(g))
    return gap, listed, grazing


def check_brute(d, s, boxes, margin, what):
    R = REAL[s.precision]
    gap, listed, grazing = brute_force(s, boxes, margin)
    assert (listed & grazing).sum() <= 0.05 * max(listed.sum(), 1), what         # before the device is asked
    items, got_gap, offsets, total = d.box_overlaps(boxes, margin, gaps=True, offsets=True)
    m = gap.shape[1]
    rows = np.repeat(np.arange(len(boxes)), np.diff(offsets.astype(np.int64)))
    got_key = rows * m + items
    keep = ~grazing[rows, items]
    ref = listed & ~grazing
    gi, gj = np.nonzero(ref)                                                     # row-major: sorted by (g, item slot)
    np.testing.assert_array_equal(got_key[keep], gi * m + gj, err_msg=str(what))  # as sets and in order
    np.testing.assert_array_equal(bits(got_gap[keep], R), bits(gap[ref], R), err_msg=str(what))
    assert (np.diff(got_key) > 0).all(), what
    return items, offsets, int((listed & grazing).sum())


# the 300 refit spheres and the 200 boxes of default_rng(78), worked out in numpy in both precisions: entries and the longest row
REFIT_ENTRIES = {"0": (496, 28), "r": (991, 40), "-r/4": (419, 24), "4r": (3882, 107)}


@PRECISIONS
def test_the_walk_is_brute_force_where_nothing_grazes(precision):
    scenes = five_scenes(precision)
    for name in ("default_L3", "refit", "clump"):
        s = scenes[name]
        d = rta.DeviceScene(s)
        boxes = boxes_for(s)
        r = median_radius(s)
        for label, margin in MARGINS:
            items, offsets, grazed = check_brute(d, s, boxes, margin(r), (name, label))
            assert len(items) > 0
            if name == "refit":
                longest = int(np.diff(offsets.astype(np.int64)).max())
                assert (len(items), longest) == REFIT_ENTRIES[label] and grazed == 0, (label, len(items), longest, grazed)
        d.close()


# ---- 3 ----

@PRECISIONS
def test_scenes_without_bounds_give_the_brute_force_answer(precision):
    R = REAL[precision]
    light = rta.normalized(LIGHT, precision)
    it, _, _ = random_nested_scene(3)
    for items in (it, it[:10], it[:1]):
        s = rta.Scene(items, light, EYE, precision=precision)
        d = s.device()
        boxes = boxes_for(s, 70)
        n, m = len(boxes), len(s.items)
        gap = rta.box_gaps(boxes, s.items)
        for margin in (0.0, median_radius(s), 1.5, -0.5, np.inf, -np.inf):
            listed = ~(gap >= R(margin))                                         # every item is tested: nothing is left out
            got, got_gap, offsets, total, st = d.box_overlaps(boxes, margin, gaps=True, offsets=True, stats=True)
            np.testing.assert_array_equal(got, np.nonzero(listed)[1])
            np.testing.assert_array_equal(bits(got_gap, R), bits(gap[listed], R))
            assert total == listed.sum() == offsets[-1]
            np.testing.assert_array_equal(np.diff(offsets.astype(np.int64)), listed.sum(axis=1))
            assert st["bound_tests"] == 0 and st["sphere_tests"] == n * m and st["primary"] == n
        d.close()


# ---- 4 ----

@PRECISIONS
def test_point_boxes_are_the_overlap_lists_with_q_zero(precision):
    for name, s in five_scenes(precision).items():
        d = rta.DeviceScene(s)
        queries = queries_for(s)
        queries[:, 3] = 0
        boxes = np.ascontiguousarray(np.concatenate([queries[:, :3], queries[:, :3]], axis=1))
        r = median_radius(s)
        exclude = (np.arange(len(queries)) % len(s.items)).astype(np.int32)
        for margin in (0.0, r, 4.0 * r, np.inf):
            for ex in (None, exclude):
                a = d.box_overlaps(boxes, margin, exclude=ex, gaps=True, offsets=True, stats=True)
                b = d.overlaps(queries, margin, exclude=ex, gaps=True, offsets=True, stats=True)
                what = (name, margin, ex is not None)
                same_bytes(a[:3], b[:3])
                assert a[3] == b[3] and counters(a[4]) == counters(b[4]), what
                if margin == np.inf and ex is None:
                    assert a[3] == len(queries) * int(((s.items[:, 3] * s.items[:, 3]) > 0).sum()), what
        d.close()


# ---- 5 ----

@PRECISIONS
def test_infinite_inverted_and_nan_boxes(precision):
    import torch
    R = REAL[precision]
    s = cases(precision)["refit"]
    d = rta.DeviceScene(s)
    m = len(s.items)
    inf = np.inf
    r = median_radius(s)
    # the all-infinite box lists every live sphere at -sqrt(rr), whatever the margin above that
    everything = np.array([[-inf] * 3 + [inf] * 3], R)
    items, gap, total = d.box_overlaps(everything, 0.0, gaps=True)
    rr = (s.items[:, 3] * s.items[:, 3]).astype(R)
    np.testing.assert_array_equal(items, np.arange(m))
    np.testing.assert_array_equal(bits(gap, R), bits(-np.sqrt(rr), R))
    assert total == m and np.isfinite(gap).all()
    assert_walk(d, Walker(s, everything), -0.5 * r, "everything")
    # a half-space per axis and sign, and the slabs between two of them
    half = []
    for axis in range(3):
        for cut in (-0.3, 0.0, 0.45):
            below = [-inf] * 3 + [inf] * 3
            below[3 + axis] = cut
            above = [-inf] * 3 + [inf] * 3
            above[axis] = cut
            slab = [-inf] * 3 + [inf] * 3
            slab[axis], slab[3 + axis] = cut - 0.1, cut + 0.1
            half += [below, above, slab]
    half = np.ascontiguousarray(np.array(half, R))
    w = Walker(s, half)
    for margin in (0.0, r, -0.25 * r, np.inf):
        got, _, offsets = assert_walk(d, w, margin, ("half-spaces", margin))
        items, offsets, _ = check_brute(d, s, half, margin, ("half-spaces", margin))
        assert 0 < len(items) and (margin == np.inf or len(items) < len(half) * m)
    assert np.isfinite(rta.box_gaps(half, s.items)).all()                        # no NaN, no inf from infinite sides
    # through the device entry: every third box inverted, every fifth with a NaN -- empty rows, no test, and the rest as without them
    boxes = boxes_for(s)
    odd = boxes.copy()
    odd[::3, [1, 4]] = odd[::3, [4, 1]] + np.array([1.0, -1.0], R) * R(scale_of(s))       # lo.y > hi.y, also where the box was a point
    odd[::5, 2] = np.nan
    odd[25, 3] = np.nan
    w = Walker(s, odd)
    carried = w.carried
    gone = np.zeros(len(odd), bool)
    gone[::3] = gone[::5] = True
    assert not carried[gone].any() and carried[~gone].all()
    margin = 2.0 * r
    ref = d.box_overlaps(np.ascontiguousarray(boxes[carried]), margin, gaps=True, offsets=True, stats=True)
    got = d.box_overlaps(torch.from_numpy(odd).cuda(), margin, gaps=True, offsets=True, stats=True)
    same_bytes(ref[:2], got[:2])                                                 # empty rows add nothing to the list
    rows = np.diff(got[2].cpu().numpy().view(np.uint64).astype(np.int64))
    np.testing.assert_array_equal(rows[carried], np.diff(ref[2].astype(np.int64)))
    assert (rows[~carried] == 0).all() and got[3] == ref[3] > 0
    assert counters(got[4]) == counters(ref[4]) and got[4]["primary"] == int(carried.sum())
    assert_walk(d, w, margin, "odd", boxes=torch.from_numpy(odd).cuda())
    # a batch of nothing but such boxes: no test at all
    none = odd[gone]
    items, offsets, total, st = d.box_overlaps(torch.from_numpy(np.ascontiguousarray(none)).cuda(), np.inf, offsets=True, stats=True)
    assert total == 0 and len(items) == 0 and not offsets.cpu().numpy().any()
    assert st["primary"] == 0 and st["tests_executed"] == 0
    d.close()


# ---- 6 ----

def raw(d, boxes, margin, capacity, items, gap, offsets, entry="host", exclude=None, order=None, stream=None):
    """One call of the C entry with the caller's own buffers (numpy arrays for "host", torch tensors for "device"); None: NULL -> total."""
    ptr = lambda x: None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data)
    n = len(boxes)
    if entry == "host":
        total = C.c_uint64(0)
        capi.check(capi.lib.rt_overlap_boxes(d._h, ptr(boxes), n, margin, ptr(exclude), ptr(order), capacity, ptr(items), ptr(gap), ptr(offsets),
                                             C.byref(total), None), "rt_overlap_boxes")
        return int(total.value)
    import torch
    total = torch.full((), -1, dtype=torch.int64, device="cuda")
    qs = torch.cuda.current_stream() if stream is None else stream
    capi.check(capi.lib.rt_overlap_boxes_device(d._h, ptr(boxes), n, margin, ptr(exclude), ptr(order), capacity, ptr(items), ptr(gap), ptr(offsets),
                                                ptr(total), None, C.c_void_p(qs.cuda_stream)), "rt_overlap_boxes_device")
    qs.synchronize()
    return int(total.item())


@PRECISIONS
def test_every_capacity_gets_the_exact_prefix(precision):
    import torch
    R = REAL[precision]
    s = cases(precision)["refit"]
    d = rta.DeviceScene(s)
    boxes = boxes_for(s)
    n = len(boxes)
    margin = median_radius(s)
    ref_i, ref_g, ref_o, total = d.box_overlaps(boxes, margin, gaps=True, offsets=True)
    assert total > 16 and len(ref_i) == total
    db = torch.from_numpy(boxes).cuda()
    GUARD = 16
    for capacity in (0, 1, total - 1, total, total + 1):
        for with_items in (True, False):
            for entry in ("host", "device"):
                items = np.full(capacity + GUARD, -77, np.int32)
                gap = np.full(capacity + GUARD, -77.0, R)
                offsets = np.full(n + 1 + GUARD, 77, np.uint64)
                if entry == "device":
                    items, gap, offsets = (torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (items, gap, offsets))
                got = raw(d, db if entry == "device" else boxes, margin, capacity, items if with_items else None, gap if with_items else None, offsets, entry)
                if entry == "device":
                    items, gap, offsets = items.cpu().numpy(), gap.cpu().numpy(), offsets.cpu().numpy().view(np.uint64)
                what = (capacity, with_items, entry)
                assert got == total, what
                np.testing.assert_array_equal(offsets[:n + 1], ref_o, err_msg=str(what))
                assert (offsets[n + 1:] == 77).all(), what
                m = min(capacity, total) if with_items else 0
                np.testing.assert_array_equal(items[:m], ref_i[:m], err_msg=str(what))
                np.testing.assert_array_equal(bits(gap[:m], R), bits(ref_g[:m], R), err_msg=str(what))
                assert (items[m:] == -77).all() and (gap[m:] == -77.0).all(), what      # nothing behind the list, the guard words included
    # items without gaps at a short capacity, and through the wrapper: a capacity gives the prefix, 0 the count alone
    items = np.full(total, -77, np.int32)
    assert raw(d, boxes, margin, total - 5, items, None, None) == total
    np.testing.assert_array_equal(items[:total - 5], ref_i[:total - 5])
    assert (items[total - 5:] == -77).all()
    for capacity in (0, 1, total - 1, total, total + 1):
        items, gap, got = d.box_overlaps(boxes, margin, capacity=capacity, gaps=True)
        m = min(capacity, total)
        assert got == total and len(items) == m == len(gap)
        np.testing.assert_array_equal(items, ref_i[:m])
        np.testing.assert_array_equal(bits(gap, R), bits(ref_g[:m], R))
    d.close()


# ---- 7 ----

# the launch: 64 lanes a wave, 256 threads a block; the scan: 256 counts a block, 256 block sums a turn of the spine (65,536 counts)
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 65537)


@PRECISIONS
def test_the_edges_of_the_launch_and_of_the_scan(precision):
    import torch
    R = REAL[precision]
    s = cases(precision)["default_L3"]
    d = rta.DeviceScene(s)
    base = boxes_for(s, 257)
    margin = median_radius(s)
    ref_i, ref_g, ref_o, ref_st = Walker(s, base).all(margin)                     # rows are independent: n boxes are the first n rows, repeated
    rows = [ref_i[int(ref_o[g]):int(ref_o[g + 1])] for g in range(257)]
    gaps = [ref_g[int(ref_o[g]):int(ref_o[g + 1])] for g in range(257)]
    assert sum(len(x) for x in rows) > 0 and min(len(x) for x in rows) == 0
    for n in EDGE_SIZES:
        pick = np.arange(n) % 257
        boxes = np.ascontiguousarray(base[pick])
        items, gap, offsets, total = d.box_overlaps(boxes, margin, gaps=True, offsets=True)
        counts = np.array([len(rows[g]) for g in pick], np.uint64)
        np.testing.assert_array_equal(offsets, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), err_msg=str(n))
        assert total == int(counts.sum()) == len(items), n
        np.testing.assert_array_equal(items, np.concatenate([rows[g] for g in pick]).astype(np.int32), err_msg=str(n))
        np.testing.assert_array_equal(bits(gap, R), bits(np.concatenate([gaps[g] for g in pick]).astype(R), R), err_msg=str(n))
    # the first 64 boxes carry no query: their wave returns before the loop, and the others answer as they did
    quiet = base[:200].copy()
    quiet[:64, 3] = quiet[:64, 0] - R(scale_of(s))                                # hi.x < lo.x
    w = Walker(s, quiet)
    assert not w.carried[:64].any() and w.carried[64:].all()
    items, gap, offsets = assert_walk(d, w, margin, "a quiet wave", boxes=torch.from_numpy(quiet).cuda())
    assert not offsets[:65].any() and len(items) == sum(len(rows[g]) for g in range(64, 200)) > 0
    # only the last box lists anything: in the fill pass every other lane has nothing to write and walks nothing
    far = base[:130].copy()
    far[:129] += R(64.0 * scale_of(s))
    far[129] = np.array([-np.inf] * 3 + [np.inf] * 3, R)
    items, gap, offsets = assert_walk(d, Walker(s, far), margin, "the last box alone")
    assert not offsets[:130].any() and len(items) == len(s.items)
    d.close()


# ---- 8 ----

@PRECISIONS
def test_exclude_and_any_order_give_the_same_bytes(precision):
    import torch
    R = REAL[precision]
    s = cases(precision)["refit"]
    d = rta.DeviceScene(s)
    boxes = boxes_for(s)
    n = len(boxes)
    margin = 2.0 * median_radius(s)
    exclude = np.random.default_rng(5).integers(-1, len(s.items) + 3, n).astype(np.int32)
    w = Walker(s, boxes)
    assert_walk(d, w, margin, "exclude", exclude=exclude)
    plain = d.box_overlaps(boxes, margin, gaps=True, offsets=True)
    ref = d.box_overlaps(boxes, margin, exclude=exclude, gaps=True, offsets=True, stats=True)
    assert ref[3] < plain[3]                                                      # something was excluded
    rows = np.repeat(np.arange(n), np.diff(ref[2].astype(np.int64)))
    assert (ref[0] != exclude[rows]).all()
    centres = (0.5 * (boxes[:, :3].astype(np.float64) + boxes[:, 3:])).astype(R)
    orders = {"identity": np.arange(n, dtype=np.uint32), "reversed": np.arange(n, dtype=np.uint32)[::-1].copy(),
              "random": np.random.default_rng(6).permutation(n).astype(np.uint32),
              "sphere_order": d.sphere_order(np.ascontiguousarray(np.concatenate([centres, np.ones((n, 1), R)], axis=1)))}
    for name, order in orders.items():
        assert sorted(order.tolist()) == list(range(n)), name
        got = d.box_overlaps(boxes, margin, exclude=exclude, order=order, gaps=True, offsets=True, stats=True)
        same_bytes(ref[:3], got[:3])
        assert got[3] == ref[3] and counters(got[4]) == counters(ref[4]), name
    with pytest.raises(ValueError, match="order"):
        d.box_overlaps(boxes, margin, order=True)
    # the device entry: the same in every order; an entry >= n carries no query, and a box nobody carries has count 0
    db, dex = torch.from_numpy(boxes).cuda(), torch.from_numpy(exclude).cuda()
    got = d.box_overlaps(db, margin, exclude=dex, order=torch.from_numpy(orders["random"].astype(np.int32)).cuda(), gaps=True, offsets=True, stats=True)
    same_bytes(ref[:3], got[:3])
    assert got[3] == ref[3] and counters(got[4]) == counters(ref[4])
    # one call lives on one side: numpy boxes take no device companions, device boxes no numpy ones
    with pytest.raises((TypeError, ValueError)):
        d.box_overlaps(boxes, margin, exclude=dex)
    with pytest.raises(ValueError, match="exclude"):
        d.box_overlaps(db, margin, exclude=exclude)
    with pytest.raises(ValueError, match="order"):
        d.box_overlaps(db, margin, order=orders["random"])
    with pytest.raises(ValueError, match="boxes"):
        d.box_overlaps(torch.from_numpy(boxes), margin)                           # a tensor that is not on the scene's device
    holes = orders["random"].astype(np.int64)
    dropped = holes[::7].copy()
    holes[::7] = n                                                                # nobody carries these boxes
    holes[7] = 0x7FFFFFFF
    dropped = np.append(dropped, orders["random"][7])
    kept = np.ones(n, bool)
    kept[dropped] = False
    sub = boxes.copy()
    sub[~kept, 3] = -np.inf                                                       # the walker's way to say "no query": hi.x < lo.x
    sub[~kept, 0] = np.inf
    ref_i, ref_g, ref_o, ref_st = Walker(s, sub).all(margin, exclude)
    got = d.box_overlaps(db, margin, exclude=dex, order=torch.from_numpy(holes.astype(np.int32)).cuda(), gaps=True, offsets=True, stats=True)
    same_bytes((ref_i, ref_g, ref_o), got[:3])
    assert got[3] == len(ref_i) and counters(got[4]) == ref_st
    d.close()


# ---- 9 ----

def check_dynamic(d, items, live, ranges, precision, what, boxes=None):
    """box_overlaps() on dynamic scene d, which holds `items` with `live`, against the Walker over a fresh static scene (host side only) made
    from the live items -- a dead slot is {0, 0, 0, 0}, which box_gaps puts at +inf as the walk does the dead record -- and bounds().
    boxes: REAL[n, 6], or None: 120 boxes around a scene of unit size at the origin."""
    R = REAL[precision]
    live = np.asarray(live) != 0
    it = np.where(live[:, None], items, 0).astype(R)
    fresh = scene_of(it, d.bounds() if ranges is not None else None, ranges, precision)
    if boxes is None:
        boxes = np.ascontiguousarray(unit_boxes(120, 79).astype(R))
    w = Walker(fresh, boxes)
    dead = np.flatnonzero(~live)
    r = float(np.median(it[live, 3])) if live.any() else 0.1
    for margin in (0.0, r, np.inf):
        got, _, offsets = assert_walk(d, w, margin, (what, margin))
        assert not np.isin(got, dead).any(), (what, margin)
        if margin == np.inf:
            assert (np.diff(offsets.astype(np.int64)) == int(live.sum())).all()
    if live.all():                                                               # ... and a fresh device scene says the same (it takes no dead slot)
        f = rta.DeviceScene(fresh)
        same_bytes(d.box_overlaps(boxes, r, gaps=True, offsets=True)[:3], f.box_overlaps(boxes, r, gaps=True, offsets=True)[:3])
        f.close()
    return boxes


@PRECISIONS
def test_dynamic_and_live_scenes_answer_as_a_fresh_scene(precision):
    R = REAL[precision]
    ranges = rta.balanced_ranges(CAPACITY, LEAF)
    d = rta.DeviceScene(rta.Scene.from_spheres_balanced(spheres_of(1, R), leaf_size=LEAF, precision=precision), 0, True)
    everyone = np.ones(CAPACITY, np.uint8)
    check_dynamic(d, spheres_of(1, R), everyone, ranges, precision, "as created")
    moved = spheres_of(2, R)
    d.update(moved)
    check_dynamic(d, moved, everyone, ranges, precision, "update")
    sp = spheres_of(3, R, spread=2.0)
    order = d.rebuild(sp)
    check_dynamic(d, sp[order], everyone, ranges, precision, "rebuild")
    live = (np.random.default_rng(4).random(CAPACITY) < 0.5).astype(np.uint8)
    live[:8] = 0                                                                 # two whole leaves: dead groups
    garbage = sp[order].copy()
    garbage[live == 0] = np.nan                                                  # a dead slot may hold any bits
    d.update(garbage, live=live)
    check_dynamic(d, sp[order], live, ranges, precision, "50 % dead")
    half = CAPACITY // 2
    order = d.rebuild(sp, n=half)
    it = np.zeros((CAPACITY, 4), R)
    it[:half] = sp[:half][order]
    boxes = check_dynamic(d, it, np.arange(CAPACITY) < half, ranges, precision, "rebuild of half")
    # n = 0: every box still walks, and the dead root culls at its one test -- the walker says so too
    d.rebuild(sp, n=0)
    empty = Walker(scene_of(np.zeros((CAPACITY, 4), R), d.bounds(), ranges, precision), boxes).all(np.inf)
    assert len(empty[0]) == 0 and empty[3]["sphere_tests"] == 0 and empty[3]["primary"] == len(boxes) and empty[3]["hits"] == 0
    assert empty[3]["bound_tests"] == len(boxes)                                 # one test per carried box
    for margin in (0.0, np.inf):
        items, offsets, total, st = d.box_overlaps(boxes, margin, offsets=True, stats=True)
        assert total == 0 and len(items) == 0 and not offsets.any() and len(offsets) == len(boxes) + 1
        assert counters(st) == empty[3]
    d.close()
    # a flat dynamic scene takes liveness too
    flat = rta.DeviceScene(rta.Scene(spheres_of(5, R, 40), rta.normalized(LIGHT, precision), EYE, precision=precision), 0, True)
    live = (np.arange(40) % 3 != 0).astype(np.uint8)
    items = spheres_of(6, R, 40, spread=0.4)
    flat.update(items, live=live)
    check_dynamic(flat, items, live, None, precision, "flat, a third dead")
    flat.close()


# ---- 10 ----

def test_entries_buffers_streams_and_threads_agree():
    import torch
    s = cases(rta.RT_F32)["refit"]
    d = rta.DeviceScene(s)
    boxes = boxes_for(s)
    n = len(boxes)
    margin = median_radius(s)
    ref = d.box_overlaps(boxes, margin, gaps=True, offsets=True, stats=True)
    total = ref[3]
    assert total > 0
    same_bytes(ref[:3], d.box_overlaps(boxes, margin, gaps=True, offsets=True)[:3])                  # two runs, with and without counters
    # the device entry: counted first (an int), with a capacity (nothing waited for), with counters
    db = torch.from_numpy(boxes).cuda()
    dev = d.box_overlaps(db, margin, gaps=True, offsets=True)
    assert all(x.device.type == "cuda" for x in dev[:3]) and dev[3] == total
    same_bytes(ref[:3], dev[:3])
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    a = d.box_overlaps(db, margin, capacity=total, gaps=True, offsets=True, stream=side)
    b = d.box_overlaps(db, margin, capacity=total, gaps=True, offsets=True, stats=True, stream=side.cuda_stream)
    other = torch.cuda.Stream()
    c = d.box_overlaps(db, 0.0, capacity=total, stream=other)                    # another margin on another stream, in between
    e = d.box_overlaps(db, margin, capacity=total, gaps=True, offsets=True)
    side.synchronize()
    other.synchronize()
    torch.cuda.synchronize()
    for got in (a, b, e):
        same_bytes(ref[:3], got[:3])
        assert int(got[3].item()) == total
    assert counters(b[4]) == counters(ref[4])
    zero = d.box_overlaps(boxes, 0.0)
    assert int(c[1].item()) == zero[1] and np.array_equal(c[0].cpu().numpy()[:zero[1]], zero[0])
    # pinned host buffers (read and written by the kernels directly) against pageable ones
    hb = [capi.HostBuffer(x) for x in (24 * n, 4 * total, 4 * total, 8 * (n + 1))]
    pb, items, gap, offsets = hb[0].array.view(np.float32).reshape(n, 6), hb[1].array.view(np.int32), hb[2].array.view(np.float32), hb[3].array.view(np.uint64)
    pb[:] = boxes
    assert raw(d, pb, margin, total, items, gap, offsets) == total
    same_bytes(ref[:3], (items, gap, offsets))
    # a buffer in device memory is refused by the host entry
    t = torch.zeros(total, dtype=torch.int32, device="cuda")
    with pytest.raises(rta.RtError) as err:
        raw(d, boxes, margin, total, t, None, None)
    assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and "device memory" in str(err.value)
    # a call that grows the workspace, then a smaller one: the same bytes as fresh calls
    grown = np.ascontiguousarray(np.concatenate([boxes] * 5)[:937])
    many = d.box_overlaps(grown, margin, gaps=True, offsets=True)
    same_bytes(ref[:3], d.box_overlaps(boxes, margin, gaps=True, offsets=True)[:3])
    same_bytes(ref[:3], d.box_overlaps(db, margin, gaps=True, offsets=True)[:3])
    fresh = rta.DeviceScene(s)
    same_bytes(many[:3], fresh.box_overlaps(grown, margin, gaps=True, offsets=True)[:3])
    fresh.close()
    assert many[3] == int(np.diff(ref[2].astype(np.int64))[np.arange(937) % n].sum())
    # two threads on one scene at once: one lists boxes, the other spheres -- they share the workspace
    queries = queries_for(s)
    spheres = d.overlaps(queries, 2 * margin, gaps=True, offsets=True)
    results, errors = [None] * 2, []

    def work(k):
        try:
            for _ in range(5):
                results[k] = d.overlaps(queries, 2 * margin, gaps=True, offsets=True) if k else d.box_overlaps(grown, margin, gaps=True, offsets=True)
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
