"""Overlap lists on the GPU (rt_overlap_spheres / rt_overlap_spheres_device, csrc/rt_overlap.hpp): every sphere of the
scene within a margin of each query sphere, bit for bit against a restatement of the walk over the scene's node stream with
rta.overlap_gaps as its metric, against brute force wherever no gap grazes the margin, against the proximity queries and the contact pairs
where those can answer, and at the edges of the launch, the scan and the capacity."""
import ctypes as C
import threading

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.scenes import random_nested_scene
from tests.test_gpu_contacts import clump
from tests.test_gpu_multihit import node_stream
from tests.test_gpu_near import CAPACITY, LEAF, LIGHT, EYE, cases, same_bytes, scene_of, spheres_of
from tests.test_gpu_query import REAL, bits

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
COUNTERS = ("primary", "hits", "shadow", "occluded", "sphere_tests", "bound_tests", "tests_executed", "primary_tests")
counters = lambda st: {c: st[c] for c in COUNTERS}


class Walker:
    """The definition of the overlap walk (include/rtrace_hip.h), one query at a time, over node_stream(s) from node 0; every gap is
    rta.overlap_gaps' in the scene's precision (made once for all queries and nodes: the walks for every margin share them)."""

    def __init__(self, s, queries):
        self.R = R = REAL[s.precision]
        nodes = node_stream(s)
        self.bound = [x[1] for x in nodes]
        self.skip = [x[2] for x in nodes]
        self.item = [x[3] for x in nodes]
        self.node_of = {x[3]: k for k, x in enumerate(nodes) if not x[1]}
        self.queries = q = np.asarray(queries, dtype=R)
        records = np.array([x[0] for x in nodes], dtype=np.float64).reshape(-1, 4).astype(R)         # (exact: they were REAL)
        self.gaps = [row.tolist() for row in rta.overlap_gaps(q, records)] if len(nodes) else [[] for _ in q]
        self.carried = q[:, 3] >= 0                                              # (NaN fails the comparison)

    def all(self, margin, exclude=None, home=None):
        """(items int32[m], gaps REAL[m], offsets uint64[n + 1], counters).  home (item slot per query, or None): asserts that no bound
        above that item's node culled, so that the walk behind the node is the contact pairs' walk."""
        m = float(self.R(margin))
        n = len(self.queries)
        items, gaps, counts = [], [], np.zeros(n, np.uint64)
        tests_items = tests_bounds = 0
        for g in range(n):
            if not self.carried[g]:
                continue
            gap = self.gaps[g]
            ex = -1 if exclude is None else int(exclude[g])
            at = None if home is None else self.node_of[int(home[g])]
            i, n_nodes = 0, len(gap)
            while i < n_nodes:
                d = gap[i]
                if self.bound[i]:
                    tests_bounds += 1
                    if d >= m:
                        assert at is None or not i < at < self.skip[i], (g, i, "a bound above the query's own item culled")
                        i = self.skip[i]
                    else:
                        i += 1
                    continue
                tests_items += 1
                if self.item[i] != ex and not d >= m:
                    items.append(self.item[i])
                    gaps.append(d)
                    counts[g] += 1
                i += 1
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        st = {c: 0 for c in COUNTERS}
        st.update(primary=int(self.carried.sum()), hits=int((counts > 0).sum()), sphere_tests=tests_items, bound_tests=tests_bounds,
                  tests_executed=tests_items + tests_bounds)
        return np.array(items, np.int32), np.array(gaps, self.R), offsets, st


def assert_walk(d, w, margin, what, exclude=None, home=None):
    items, gap, offsets, total, st = d.overlaps(w.queries, margin, exclude=exclude, gaps=True, offsets=True, stats=True)
    ref_i, ref_g, ref_o, ref_st = w.all(margin, exclude, home)
    np.testing.assert_array_equal(items, ref_i, err_msg=str(what))
    np.testing.assert_array_equal(bits(gap, w.R), bits(ref_g, w.R), err_msg=str(what))
    np.testing.assert_array_equal(offsets, ref_o, err_msg=str(what))
    assert total == len(ref_i) == int(offsets[-1]), what
    assert counters(st) == ref_st, what
    for g in range(len(w.queries)):                                              # ascending within a query
        assert (np.diff(items[int(offsets[g]):int(offsets[g + 1])]) > 0).all(), (what, g)
    return items, gap, offsets


def median_radius(s):
    return float(np.median(s.items[:, 3]))


def scale_of(s):
    """The scene's extent as a power of two (the scaling is exact): 1 for spheres in +-1."""
    live = s.items[s.items[:, 3] > 0]
    return float(2.0 ** np.round(np.log2(np.abs(live[:, :3].astype(np.float64)).max())))


def queries_for(s, n=200, seed=77):
    """n query spheres: centres uniform in +-1.2 and q uniform in [0, 0.3], scaled to the scene's extent, every tenth q = 0."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.2, 1.2, (n, 3))
    q = rng.uniform(0.0, 0.3, n)
    q[::10] = 0.0
    return np.ascontiguousarray((np.concatenate([c, q[:, None]], axis=1) * scale_of(s)).astype(REAL[s.precision]))


def five_scenes(precision):
    it, bd, rg = random_nested_scene(3)
    scenes = {name: cases(precision)[name] for name in ("default_L3", "nested", "refit")}
    scenes["nested3"] = scene_of(it, bd, rg, precision)
    scenes["clump"] = clump(precision)[0]
    return scenes


@PRECISIONS
def test_the_list_restates_the_walk_bit_for_bit(precision):
    for name, s in five_scenes(precision).items():
        d = rta.DeviceScene(s)
        queries = queries_for(s)
        w = Walker(s, queries)
        r = median_radius(s)
        n_live = int(((s.items[:, 3] * s.items[:, 3]) > 0).sum())
        for margin in (0.0, r, -0.25 * r, 4.0 * r, np.inf, -np.inf):
            items, gap, offsets = assert_walk(d, w, margin, (name, margin))
            if margin == np.inf:
                assert (np.diff(offsets.astype(np.int64)) == n_live).all() and len(items) == len(queries) * n_live
            if margin == -np.inf:
                assert len(items) == 0
        d.close()


def brute_force(s, queries, margin):
    """(gap[n, m], listed, grazing): an entry may be left out only if its gap lies within 1e-5 max(1, |gap|) (f64: 1e-12) of the margin."""
    R = REAL[s.precision]
    gap = rta.overlap_gaps(queries, s.items)
    m = R(margin)
    listed = ~(gap >= m)
    eps = 1e-5 if R == np.float32 else 1e-12
    g = gap.astype(np.float64)
    with np.errstate(invalid="ignore"):
        grazing = np.abs(g - float(m)) <= eps * np.maximum(1.0, np.abs(g))
    return gap, listed, grazing


def check_brute(d, s, queries, margin, what):
    R = REAL[s.precision]
    gap, listed, grazing = brute_force(s, queries, margin)
    assert (listed & grazing).sum() <= 0.05 * max(listed.sum(), 1), what
    items, got_gap, offsets, total = d.overlaps(queries, margin, gaps=True, offsets=True)
    m = gap.shape[1]
    rows = np.repeat(np.arange(len(queries)), np.diff(offsets.astype(np.int64)))
    got_key = rows * m + items
    keep = ~grazing[rows, items]
    ref = listed & ~grazing
    gi, gj = np.nonzero(ref)                                                     # row-major: sorted by (g, item slot)
    np.testing.assert_array_equal(got_key[keep], gi * m + gj, err_msg=str(what))  # as sets and in order
    np.testing.assert_array_equal(bits(got_gap[keep], R), bits(gap[ref], R), err_msg=str(what))
    assert (np.diff(got_key) > 0).all(), what
    return items, offsets, int((listed & grazing).sum())


# the 300 refit spheres and the 200 queries of default_rng(77), worked out in numpy in both precisions: entries and the longest row
REFIT_ENTRIES = {"0": (289, 10), "r": (590, 17), "-r/4": (239, 9), "4r": (2620, 63)}


@PRECISIONS
def test_the_walk_is_brute_force_where_nothing_grazes(precision):
    scenes = five_scenes(precision)
    for name in ("default_L3", "refit", "clump"):
        s = scenes[name]
        d = rta.DeviceScene(s)
        queries = queries_for(s)
        r = median_radius(s)
        for label, margin in (("0", 0.0), ("r", r), ("-r/4", -0.25 * r), ("4r", 4.0 * r)):
            items, offsets, grazed = check_brute(d, s, queries, margin, (name, margin))
            assert len(items) > 0
            if name == "refit":
                longest = int(np.diff(offsets.astype(np.int64)).max())
                assert (len(items), longest) == REFIT_ENTRIES[label] and grazed == 0, (label, len(items), longest, grazed)
        d.close()
    assert REFIT_ENTRIES["r"][1] > rta.RT_NEAR_MAX_K and REFIT_ENTRIES["4r"][1] > rta.RT_NEAR_MAX_K      # rows no proximity query can list


@PRECISIONS
def test_scenes_without_bounds_give_the_brute_force_answer(precision):
    R = REAL[precision]
    light = rta.normalized(LIGHT, precision)
    it, _, _ = random_nested_scene(3)
    for items in (it, it[:10], it[:1]):
        s = rta.Scene(items, light, EYE, precision=precision)
        d = s.device()
        queries = queries_for(s, 70)
        n, m = len(queries), len(s.items)
        gap = rta.overlap_gaps(queries, s.items)
        for margin in (0.0, median_radius(s), 1.5, -0.5, np.inf, -np.inf):
            listed = ~(gap >= R(margin))                                         # every item is tested: nothing is left out
            got, got_gap, offsets, total, st = d.overlaps(queries, margin, gaps=True, offsets=True, stats=True)
            np.testing.assert_array_equal(got, np.nonzero(listed)[1])
            np.testing.assert_array_equal(bits(got_gap, R), bits(gap[listed], R))
            assert total == listed.sum() == offsets[-1]
            np.testing.assert_array_equal(np.diff(offsets.astype(np.int64)), listed.sum(axis=1))
            assert st["bound_tests"] == 0 and st["sphere_tests"] == n * m and st["primary"] == n
        d.close()


@PRECISIONS
def test_it_is_near_where_near_can_answer(precision):
    R = REAL[precision]
    K = rta.RT_NEAR_MAX_K
    scenes = five_scenes(precision)
    for name in ("refit", "clump", "nested"):
        s = scenes[name]
        d = rta.DeviceScene(s)
        queries = queries_for(s)
        queries[:, 3] = 0
        points = np.ascontiguousarray(queries[:, :3])
        r = median_radius(s)
        exclude = (np.arange(len(queries)) % len(s.items)).astype(np.int32)
        for rho in (r, 4.0 * r, 0.0, np.inf):
            for ex in (None, exclude):
                items, gap, offsets, total, st = d.overlaps(queries, rho, exclude=ex, gaps=True, offsets=True, stats=True)
                ngap, nitem, found, nst = d.near(points, K, np.full(len(queries), rho, R), all_within=True, exclude=ex, want_stats=True)
                what = (name, rho, ex is not None)
                assert counters(st) == counters(nst), what
                lengths = np.diff(offsets.astype(np.int64))
                np.testing.assert_array_equal(found, lengths, err_msg=str(what))
                for g in range(len(queries)):
                    a, b = int(offsets[g]), int(offsets[g + 1])
                    first = np.argsort(gap[a:b], kind="stable")[:K]              # equal gaps keep the order of the slots
                    k = len(first)
                    np.testing.assert_array_equal(nitem[g, :k], items[a:b][first], err_msg=str((what, g)))
                    np.testing.assert_array_equal(bits(ngap[g, :k], R), bits(gap[a:b][first], R), err_msg=str((what, g)))
                    assert (nitem[g, k:] == -1).all(), (what, g)
                if rho == np.inf:
                    assert lengths.min() > K                                     # ... and there near stops
        d.close()


@PRECISIONS
def test_it_is_contacts_where_contacts_can_answer(precision):
    R = REAL[precision]
    scenes = five_scenes(precision)
    big = clump(precision)[1]
    for name in ("refit", "clump", "default_L3"):
        s = scenes[name]
        d = rta.DeviceScene(s)
        n = len(s.items)
        own = np.ascontiguousarray(s.items.astype(R))
        own[:, 3] = np.sqrt(s.items[:, 3] * s.items[:, 3])                       # the root of the stream's rr, in REAL
        me = np.arange(n, dtype=np.int32)
        w = Walker(s, own)
        r = median_radius(s)
        for margin in (0.0, r, -0.25 * r):
            items, gap, offsets = assert_walk(d, w, margin, (name, margin), exclude=me, home=me)
            pairs, pgap, total = d.contacts(margin, gaps=True)
            rows = np.repeat(np.arange(n), np.diff(offsets.astype(np.int64)))
            assert (items != rows).all()
            upper = items > rows
            np.testing.assert_array_equal(np.stack([rows[upper], items[upper]], axis=1), pairs, err_msg=str((name, margin)))
            np.testing.assert_array_equal(bits(gap[upper], R), bits(pgap, R), err_msg=str((name, margin)))
            if name == "clump" and margin == 0.0:
                row = items[int(offsets[big]):int(offsets[big + 1])]
                assert len(row) == 40 > rta.RT_NEAR_MAX_K and len(set(row.tolist())) == 40
        d.close()


def raw(d, queries, margin, capacity, items, gap, offsets, entry="host", exclude=None, order=None, stream=None):
    """One call of the C entry with the caller's own buffers (numpy arrays for "host", torch tensors for "device"); None: NULL -> total."""
    ptr = lambda x: None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data)
    n = len(queries)
    if entry == "host":
        total = C.c_uint64(0)
        capi.check(capi.lib.rt_overlap_spheres(d._h, ptr(queries), n, margin, ptr(exclude), ptr(order), capacity, ptr(items), ptr(gap), ptr(offsets),
                                               C.byref(total), None), "rt_overlap_spheres")
        return int(total.value)
    import torch
    total = torch.full((), -1, dtype=torch.int64, device="cuda")
    qs = torch.cuda.current_stream() if stream is None else stream
    capi.check(capi.lib.rt_overlap_spheres_device(d._h, ptr(queries), n, margin, ptr(exclude), ptr(order), capacity, ptr(items), ptr(gap), ptr(offsets),
                                                  ptr(total), None, C.c_void_p(qs.cuda_stream)), "rt_overlap_spheres_device")
    qs.synchronize()
    return int(total.item())


@PRECISIONS
def test_every_capacity_gets_the_exact_prefix(precision):
    import torch
    R = REAL[precision]
    s = cases(precision)["refit"]
    d = rta.DeviceScene(s)
    queries = queries_for(s)
    n = len(queries)
    margin = median_radius(s)
    ref_i, ref_g, ref_o, total = d.overlaps(queries, margin, gaps=True, offsets=True)
    assert total > 16 and len(ref_i) == total
    dq = torch.from_numpy(queries).cuda()
    GUARD = 16
    for capacity in (0, 1, total - 1, total, total + 7):
        for with_items in (True, False):
            for entry in ("host", "device"):
                items = np.full(capacity + GUARD, -77, np.int32)
                gap = np.full(capacity + GUARD, -77.0, R)
                offsets = np.full(n + 1 + GUARD, 77, np.uint64)
                if entry == "device":
                    items, gap, offsets = (torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (items, gap, offsets))
                got = raw(d, dq if entry == "device" else queries, margin, capacity, items if with_items else None, gap if with_items else None, offsets, entry)
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
    # through the wrapper: a capacity gives the prefix, 0 the count alone
    for capacity in (0, 1, total - 1, total, total + 7):
        items, gap, got = d.overlaps(queries, margin, capacity=capacity, gaps=True)
        m = min(capacity, total)
        assert got == total and len(items) == m == len(gap)
        np.testing.assert_array_equal(items, ref_i[:m])
        np.testing.assert_array_equal(bits(gap, R), bits(ref_g[:m], R))
    d.close()


# the launch: 64 lanes a wave, 256 threads a block; the scan: 256 counts a block, 256 block sums a turn of the spine (65,536 counts)
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 65537)


@PRECISIONS
def test_the_edges_of_the_launch_and_of_the_scan(precision):
    R = REAL[precision]
    s = cases(precision)["default_L3"]
    d = rta.DeviceScene(s)
    base = queries_for(s, 257)
    margin = median_radius(s)
    ref_i, ref_g, ref_o, ref_st = Walker(s, base).all(margin)                     # rows are independent: n queries are the first n rows, repeated
    rows = [ref_i[int(ref_o[g]):int(ref_o[g + 1])] for g in range(257)]
    gaps = [ref_g[int(ref_o[g]):int(ref_o[g + 1])] for g in range(257)]
    assert sum(len(x) for x in rows) > 0 and min(len(x) for x in rows) == 0
    for n in EDGE_SIZES:
        pick = np.arange(n) % 257
        queries = np.ascontiguousarray(base[pick])
        items, gap, offsets, total = d.overlaps(queries, margin, gaps=True, offsets=True)
        counts = np.array([len(rows[g]) for g in pick], np.uint64)
        np.testing.assert_array_equal(offsets, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), err_msg=str(n))
        assert total == int(counts.sum()) == len(items), n
        np.testing.assert_array_equal(items, np.concatenate([rows[g] for g in pick]).astype(np.int32), err_msg=str(n))
        np.testing.assert_array_equal(bits(gap, R), bits(np.concatenate([gaps[g] for g in pick]).astype(R), R), err_msg=str(n))
    d.close()


@PRECISIONS
def test_exclude_and_any_order_give_the_same_bytes(precision):
    import torch
    R = REAL[precision]
    s = cases(precision)["refit"]
    d = rta.DeviceScene(s)
    queries = queries_for(s)
    n = len(queries)
    margin = 2.0 * median_radius(s)
    exclude = np.random.default_rng(5).integers(-1, len(s.items) + 3, n).astype(np.int32)
    w = Walker(s, queries)
    assert_walk(d, w, margin, "exclude", exclude=exclude)
    plain = d.overlaps(queries, margin, gaps=True, offsets=True)
    ref = d.overlaps(queries, margin, exclude=exclude, gaps=True, offsets=True, stats=True)
    assert ref[3] < plain[3]                                                      # something was excluded
    rows = np.repeat(np.arange(n), np.diff(ref[2].astype(np.int64)))
    assert (ref[0] != exclude[rows]).all()
    orders = {"identity": np.arange(n, dtype=np.uint32), "reversed": np.arange(n, dtype=np.uint32)[::-1].copy(),
              "random": np.random.default_rng(6).permutation(n).astype(np.uint32), "sphere_order": d.sphere_order(np.concatenate([queries[:, :3], np.ones((n, 1), R)], axis=1))}
    for name, order in orders.items():
        assert sorted(order.tolist()) == list(range(n)), name
        got = d.overlaps(queries, margin, exclude=exclude, order=order, gaps=True, offsets=True, stats=True)
        same_bytes(ref[:3], got[:3])
        assert got[3] == ref[3] and counters(got[4]) == counters(ref[4]), name
    got = d.overlaps(queries, margin, exclude=exclude, order=True, gaps=True, offsets=True, stats=True)
    same_bytes(ref[:3], got[:3])
    assert counters(got[4]) == counters(ref[4])
    # the device entry: the same in every order; an entry >= n carries no query, and a query nobody carries has count 0
    dq, dex = torch.from_numpy(queries).cuda(), torch.from_numpy(exclude).cuda()
    got = d.overlaps(dq, margin, exclude=dex, order=torch.from_numpy(orders["random"].astype(np.int32)).cuda(), gaps=True, offsets=True, stats=True)
    same_bytes(ref[:3], got[:3])
    assert got[3] == ref[3] and counters(got[4]) == counters(ref[4])
    got = d.overlaps(dq, margin, exclude=dex, order=True, gaps=True, offsets=True)
    same_bytes(ref[:3], got[:3])
    holes = orders["random"].astype(np.int64)
    dropped = holes[::7].copy()
    holes[::7] = n                                                                # nobody carries these queries
    holes[7] = 0x7FFFFFFF
    kept = np.ones(n, bool)
    kept[dropped] = False
    sub = queries.copy()
    sub[~kept, 3] = -1                                                            # the walker's way to say "no query"
    ref_i, ref_g, ref_o, ref_st = Walker(s, sub).all(margin, exclude)
    got = d.overlaps(dq, margin, exclude=dex, order=torch.from_numpy(holes.astype(np.int32)).cuda(), gaps=True, offsets=True, stats=True)
    same_bytes((ref_i, ref_g, ref_o), got[:3])
    assert got[3] == len(ref_i) and counters(got[4]) == ref_st
    # a query with q = -1 or NaN on the device entry: an empty row and no test
    for value in (-1.0, np.nan, -np.inf):
        odd = queries.copy()
        odd[3::5, 3] = value
        wo = Walker(s, odd)
        assert not wo.carried[3::5].any() and wo.carried.sum() == n - len(odd[3::5])
        ref_i, ref_g, ref_o, ref_st = wo.all(margin, exclude)
        got = d.overlaps(torch.from_numpy(odd).cuda(), margin, exclude=dex, gaps=True, offsets=True, stats=True)
        same_bytes((ref_i, ref_g, ref_o), got[:3])
        assert counters(got[4]) == ref_st and (np.diff(ref_o.astype(np.int64))[3::5] == 0).all()
    d.close()


def check_dynamic(d, items, live, ranges, precision, what, queries=None):
    """overlaps() on dynamic scene d, which holds `items` with `live`, against the Walker over a fresh static scene (host side only) made
    from the live items -- a dead slot is {0, 0, 0, 0}, which overlap_gaps puts at +inf as the walk does the dead record -- and bounds().
    queries: REAL[n, 4], or None: 120 query spheres around a scene of unit size at the origin."""
    R = REAL[precision]
    live = np.asarray(live) != 0
    it = np.where(live[:, None], items, 0).astype(R)
    fresh = scene_of(it, d.bounds() if ranges is not None else None, ranges, precision)
    if queries is None:
        rng = np.random.default_rng(78)
        queries = np.concatenate([rng.uniform(-1.2, 1.2, (120, 3)), rng.uniform(0.0, 0.3, (120, 1))], axis=1).astype(R)
        queries[::10, 3] = 0
    w = Walker(fresh, queries)
    dead = np.flatnonzero(~live)
    r = float(np.median(it[live, 3])) if live.any() else 0.1
    for margin in (0.0, r, np.inf):
        got, _, offsets = assert_walk(d, w, margin, (what, margin))
        assert not np.isin(got, dead).any(), (what, margin)
        if margin == np.inf:
            assert (np.diff(offsets.astype(np.int64)) == int(live.sum())).all()
    if live.all():                                                               # ... and a fresh device scene says the same (it takes no dead slot)
        f = rta.DeviceScene(fresh)
        same_bytes(d.overlaps(queries, r, gaps=True, offsets=True)[:3], f.overlaps(queries, r, gaps=True, offsets=True)[:3])
        f.close()
    return queries


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
    queries = check_dynamic(d, it, np.arange(CAPACITY) < half, ranges, precision, "rebuild of half")
    # n = 0: every query still walks, and the dead root culls at its one test -- the walker says so too
    d.rebuild(sp, n=0)
    empty = Walker(scene_of(np.zeros((CAPACITY, 4), R), d.bounds(), ranges, precision), queries).all(np.inf)
    assert len(empty[0]) == 0 and empty[3]["sphere_tests"] == 0 and empty[3]["primary"] == len(queries) and empty[3]["hits"] == 0
    for margin in (0.0, np.inf):
        items, offsets, total, st = d.overlaps(queries, margin, offsets=True, stats=True)
        assert total == 0 and len(items) == 0 and not offsets.any() and len(offsets) == len(queries) + 1
        assert counters(st) == empty[3]
    d.close()
    # a flat dynamic scene takes liveness too
    flat = rta.DeviceScene(rta.Scene(spheres_of(5, R, 40), rta.normalized(LIGHT, precision), EYE, precision=precision), 0, True)
    live = (np.arange(40) % 3 != 0).astype(np.uint8)
    items = spheres_of(6, R, 40, spread=0.4)
    flat.update(items, live=live)
    check_dynamic(flat, items, live, None, precision, "flat, a third dead")
    flat.close()


def test_entries_buffers_streams_and_threads_agree():
    import torch
    s = cases(rta.RT_F32)["refit"]
    d = rta.DeviceScene(s)
    queries = queries_for(s)
    n = len(queries)
    margin = median_radius(s)
    ref = d.overlaps(queries, margin, gaps=True, offsets=True, stats=True)
    total = ref[3]
    assert total > 0
    same_bytes(ref[:3], d.overlaps(queries, margin, gaps=True, offsets=True)[:3])                    # two runs, with and without counters
    # the device entry: counted first (an int), with a capacity (nothing waited for), with counters
    dq = torch.from_numpy(queries).cuda()
    dev = d.overlaps(dq, margin, gaps=True, offsets=True)
    assert all(x.device.type == "cuda" for x in dev[:3]) and dev[3] == total
    same_bytes(ref[:3], dev[:3])
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    a = d.overlaps(dq, margin, capacity=total, gaps=True, offsets=True, stream=side)
    b = d.overlaps(dq, margin, capacity=total, gaps=True, offsets=True, stats=True, stream=side.cuda_stream)
    other = torch.cuda.Stream()
    c = d.overlaps(dq, 0.0, capacity=total, stream=other)                        # another margin on another stream, in between
    e = d.overlaps(dq, margin, capacity=total, gaps=True, offsets=True)
    side.synchronize()
    other.synchronize()
    torch.cuda.synchronize()
    for got in (a, b, e):
        same_bytes(ref[:3], got[:3])
        assert int(got[3].item()) == total
    assert counters(b[4]) == counters(ref[4])
    zero = d.overlaps(queries, 0.0)
    assert int(c[1].item()) == zero[1] and np.array_equal(c[0].cpu().numpy()[:zero[1]], zero[0])
    # pinned host buffers (read and written by the kernels directly) against pageable ones
    hb = [capi.HostBuffer(x) for x in (16 * n, 4 * total, 4 * total, 8 * (n + 1))]
    pq, items, gap, offsets = hb[0].array.view(np.float32).reshape(n, 4), hb[1].array.view(np.int32), hb[2].array.view(np.float32), hb[3].array.view(np.uint64)
    pq[:] = queries
    assert raw(d, pq, margin, total, items, gap, offsets) == total
    same_bytes(ref[:3], (items, gap, offsets))
    # a buffer in device memory is refused by the host entry
    t = torch.zeros(total, dtype=torch.int32, device="cuda")
    with pytest.raises(rta.RtError) as err:
        raw(d, queries, margin, total, t, None, None)
    assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT
    # a call that grows the workspace, then a smaller one: the same bytes as fresh calls
    grown = np.ascontiguousarray(np.concatenate([queries] * 5)[:937])
    many = d.overlaps(grown, margin, gaps=True, offsets=True)
    same_bytes(ref[:3], d.overlaps(queries, margin, gaps=True, offsets=True)[:3])
    same_bytes(ref[:3], d.overlaps(dq, margin, gaps=True, offsets=True)[:3])
    fresh = rta.DeviceScene(s)
    same_bytes(many[:3], fresh.overlaps(grown, margin, gaps=True, offsets=True)[:3])
    fresh.close()
    assert many[3] == int(np.diff(ref[2].astype(np.int64))[np.arange(937) % n].sum())
    # four threads on one scene at once, two margins, two sizes
    wide = d.overlaps(grown, 2 * margin, gaps=True, offsets=True)
    results, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(5):
                results[k] = d.overlaps(grown, 2 * margin, gaps=True, offsets=True) if k % 2 else d.overlaps(queries, margin, gaps=True, offsets=True)
        except Exception as ex:          # noqa: BLE001 (reported below)
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k, r in enumerate(results):
        same_bytes((wide if k % 2 else ref)[:3], r[:3])
        assert r[3] == (wide if k % 2 else ref)[3]
    d.close()
