"""Contact pairs on the GPU (rt_scene_contacts / rt_scene_contacts_device, csrc/rt_contacts.hpp): every pair of spheres of
the scene closer than a margin, bit for bit against a restatement of the walk over the scene's node stream with rta.pair_gaps as its
metric, against brute force over all i < j wherever no gap grazes the margin, and at the edges of the launch, the scan and the capacity."""
import ctypes as C
import threading

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.scenes import random_nested_scene
from tests.test_gpu_multihit import node_stream
from tests.test_gpu_near import CAPACITY, LEAF, LIGHT, EYE, cases, same_bytes, scene_of, spheres_of
from tests.test_gpu_query import REAL, bits

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
COUNTERS = ("primary", "hits", "shadow", "occluded", "sphere_tests", "bound_tests", "tests_executed", "primary_tests")


class Walker:
    """The definition of the contacts walk (include/rtrace_hip.h), one item at a time, over node_stream(s): item t starts behind its own
    node; every gap is rta.pair_gaps' in the scene's precision, with the item as the pair's first sphere."""

    def __init__(self, s):
        self.R = R = REAL[s.precision]
        nodes = node_stream(s)
        self.n_items = n = len(s.items)
        self.bound = [x[1] for x in nodes]
        self.skip = [x[2] for x in nodes]
        self.item = [x[3] for x in nodes]
        self.node_of = {x[3]: k for k, x in enumerate(nodes) if not x[1]}
        assert sorted(self.node_of) == list(range(n)) and all(self.node_of[t] < self.node_of[t + 1] for t in range(n - 1))
        records = np.array([x[0] for x in nodes], dtype=np.float64).reshape(-1, 4).astype(R)         # (exact: they were REAL)
        self.spheres = np.concatenate([np.asarray(s.items, dtype=R), records])
        self.live = (self.spheres[:n, 3] * self.spheres[:n, 3]) > 0

    def all(self, margin):
        """(pairs int32[m, 2], gaps REAL[m], offsets uint64[n + 1], counters) of the whole scene."""
        m = float(self.R(margin))
        n, n_nodes = self.n_items, len(self.bound)
        pairs, gaps, counts = [], [], np.zeros(n, np.uint64)
        tests_items = tests_bounds = 0
        for t in range(n):
            if not self.live[t]:
                continue
            first = self.node_of[t] + 1
            later = np.arange(first, n_nodes)
            gap = rta.pair_gaps(self.spheres, np.full(len(later), t), n + later).tolist()
            i = first
            while i < n_nodes:
                g = gap[i - first]
                if self.bound[i]:
                    tests_bounds += 1
                    i = self.skip[i] if g >= m else i + 1
                    continue
                tests_items += 1
                if not g >= m:
                    pairs.append((t, self.item[i]))
                    gaps.append(g)
                    counts[t] += 1
                i += 1
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        st = {c: 0 for c in COUNTERS}
        st.update(primary=int(self.live.sum()), hits=int((counts > 0).sum()), sphere_tests=tests_items, bound_tests=tests_bounds,
                  tests_executed=tests_items + tests_bounds)
        return np.array(pairs, np.int32).reshape(-1, 2), np.array(gaps, self.R), offsets, st


def assert_walk(d, w, margin, what):
    pairs, gap, offsets, total, st = d.contacts(margin, gaps=True, offsets=True, stats=True)
    ref_p, ref_g, ref_o, ref_st = w.all(margin)
    np.testing.assert_array_equal(pairs, ref_p, err_msg=str(what))
    np.testing.assert_array_equal(bits(gap, w.R), bits(ref_g, w.R), err_msg=str(what))
    np.testing.assert_array_equal(offsets, ref_o, err_msg=str(what))
    assert total == len(ref_p) == int(offsets[-1]), what
    assert {c: st[c] for c in COUNTERS} == ref_st, what
    assert (pairs[:, 0] < pairs[:, 1]).all(), what
    return pairs, gap


def clump(precision):
    """One large sphere that 40 small ones on a shell around it overlap, and 60 small ones further out: Morton order, balanced ranges,
    refit bounds (which enclose).  -> (Scene, the large sphere's slot)"""
    R = REAL[precision]
    rng = np.random.default_rng(40)
    u = rng.normal(size=(100, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = np.concatenate([np.full(40, 1.03), rng.uniform(1.6, 2.5, 60)])
    sp = np.concatenate([[[0.0, 0.0, 0.0, 1.0]], np.concatenate([u * dist[:, None], np.full((100, 1), 0.1)], axis=1)]).astype(R)
    order = np.argsort(rta.sphere_keys(sp), kind="stable")
    sp = sp[order]
    rg = rta.balanced_ranges(len(sp), 4)
    return scene_of(sp, rta.refit_bounds(sp, rg, precision), rg, precision), int(np.flatnonzero(order == 0)[0])


def median_radius(s):
    return float(np.median(s.items[:, 3]))


@PRECISIONS
def test_the_list_restates_the_walk_bit_for_bit(precision):
    it, bd, rg = random_nested_scene(3)
    scenes = {name: cases(precision)[name] for name in ("default_L3", "nested", "refit")}
    scenes["nested3"] = scene_of(it, bd, rg, precision)
    scenes["clump"], big = clump(precision)
    for name, s in scenes.items():
        d = rta.DeviceScene(s)
        w = Walker(s)
        r = median_radius(s)
        for margin in (0.0, r, -0.25 * r, 4.0 * r, np.inf, -np.inf):
            pairs, gap = assert_walk(d, w, margin, (name, margin))
            if margin == np.inf:
                n = len(s.items)
                assert len(pairs) == n * (n - 1) // 2
            if margin == -np.inf:
                assert len(pairs) == 0
            if name == "clump" and margin == 0.0:
                # the large sphere touches 40 others: all of them are listed, which no k <= RT_NEAR_MAX_K of rt_near_spheres can do
                partners = np.concatenate([pairs[pairs[:, 0] == big, 1], pairs[pairs[:, 1] == big, 0]])
                assert len(partners) == 40 > rta.RT_NEAR_MAX_K and len(set(partners.tolist())) == 40
                found = d.near(np.ascontiguousarray(s.items[big:big + 1, :3]), 16, s.items[big, 3:4].copy(), all_within=True,
                               exclude=np.array([big], np.int32))[2]
                assert found[0] == 40
        d.close()


def brute_force(s, margin):
    """(i, j, gap, contact, grazing) over all i < j: rule 2 of the issue -- a pair may be left out only if its gap lies within
    1e-5 max(1, |gap|) (f64: 1e-12) of the margin."""
    R = REAL[s.precision]
    n = len(s.items)
    i, j = np.triu_indices(n, 1)
    gap = rta.pair_gaps(s.items, i, j)
    m = R(margin)
    contact = ~(gap >= m)
    eps = 1e-5 if R == np.float32 else 1e-12
    g = gap.astype(np.float64)
    with np.errstate(invalid="ignore"):
        grazing = np.abs(g - float(m)) <= eps * np.maximum(1.0, np.abs(g))
    return i, j, gap, contact, grazing


def check_brute(d, s, margin, what):
    R = REAL[s.precision]
    i, j, gap, contact, grazing = brute_force(s, margin)
    assert (contact & grazing).sum() <= 0.05 * max(contact.sum(), 1), what
    pairs, got_gap, total = d.contacts(margin, gaps=True)
    n = len(s.items)
    graze_key = set((i[grazing] * n + j[grazing]).tolist())
    got_key = pairs[:, 0].astype(np.int64) * n + pairs[:, 1]
    keep = np.array([k not in graze_key for k in got_key.tolist()], bool)
    ref = contact & ~grazing
    np.testing.assert_array_equal(got_key[keep], (i[ref] * n + j[ref]), err_msg=str(what))           # as sets and in order: both are sorted
    np.testing.assert_array_equal(bits(got_gap[keep], R), bits(gap[ref], R), err_msg=str(what))
    assert (np.diff(got_key) > 0).all(), what
    return pairs, grazing, (i, j)


@PRECISIONS
def test_the_walk_is_brute_force_where_nothing_grazes(precision):
    clump_scene, _ = clump(precision)
    for name, s in (("refit", cases(precision)["refit"]), ("clump", clump_scene)):
        d = rta.DeviceScene(s)
        r = median_radius(s)
        for margin in (0.0, r, -0.25 * r, 3.0 * r, np.inf):
            pairs, _, _ = check_brute(d, s, margin, (name, margin))
            assert len(pairs) > 0
        d.close()


@PRECISIONS
def test_scenes_without_bounds_give_the_brute_force_answer(precision):
    R = REAL[precision]
    light = rta.normalized(LIGHT, precision)
    it, _, _ = random_nested_scene(3)
    ties = [(0.0, 0.0, 0.0, 1.0), (3.0, 0.0, 0.0, 0.5), (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, -3.0, 0.5), (0.0, 4.0, 0.0, 0.5), (0.0, -3.0, 4.0, 0.5), (0.0, 0.0, 0.0, 1.0)]
    for items in (it, it[:10], ties, it[:1]):
        s = rta.Scene(items, light, EYE, precision=precision)
        d = s.device()
        n = len(s.items)
        i, j = np.triu_indices(n, 1)
        gap = rta.pair_gaps(s.items, i, j)
        for margin in (0.0, median_radius(s), 1.5, -0.5, np.inf, -np.inf):
            contact = ~(gap >= R(margin))                                        # every later item is tested: nothing is left out
            pairs, got, offsets, total, st = d.contacts(margin, gaps=True, offsets=True, stats=True)
            np.testing.assert_array_equal(pairs, np.stack([i[contact], j[contact]], axis=1))
            np.testing.assert_array_equal(bits(got, R), bits(gap[contact], R))
            assert total == contact.sum() == offsets[-1]
            np.testing.assert_array_equal(np.diff(offsets.astype(np.int64)), np.bincount(i[contact], minlength=n))
            assert st["bound_tests"] == 0 and st["sphere_tests"] == n * (n - 1) // 2 and st["primary"] == n
        d.close()


def line_scene(n, precision):
    R = REAL[precision]
    sp = np.zeros((n, 4), R)
    sp[:, 0] = np.arange(n)
    sp[:, 3] = 0.75
    return rta.DeviceScene(rta.Scene.from_spheres_balanced(sp, leaf_size=4, precision=precision), 0, True)


# the launch: 64 lanes a wave, 256 threads a block; the scan: 256 counts a block, 256 block sums a turn of the spine (65,536 counts)
LINE_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 65537)


@PRECISIONS
def test_the_edges_of_the_launch_and_of_the_scan(precision):
    R = REAL[precision]
    for n in LINE_SIZES:
        d = line_scene(n, precision)
        # spheres of radius 0.75 at 0, 1, 2, ...: neighbours overlap by 0.5 = (1 - 0.75) - 0.75, everything else is 0.5 or more apart, exactly
        pairs, gap, offsets, total = d.contacts(0.0, gaps=True, offsets=True)
        assert total == n - 1, n
        np.testing.assert_array_equal(pairs, np.stack([np.arange(n - 1), np.arange(1, n)], axis=1), err_msg=str(n))
        assert (gap == R(-0.5)).all(), n
        np.testing.assert_array_equal(offsets, np.minimum(np.arange(n + 1), n - 1).astype(np.uint64), err_msg=str(n))
        if n <= 65:
            pairs, total = d.contacts(np.inf)
            assert total == n * (n - 1) // 2 == len(pairs)
            i, j = np.triu_indices(n, 1)
            np.testing.assert_array_equal(pairs, np.stack([i, j], axis=1))
        d.close()


def raw(d, margin, capacity, pairs, gap, offsets, entry="host", stream=None):
    """One call of the C entry with the caller's own buffers (numpy arrays for "host", torch tensors for "device"); None: NULL -> total."""
    ptr = lambda x: None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data)
    if entry == "host":
        total = C.c_uint64(0)
        capi.check(capi.lib.rt_scene_contacts(d._h, margin, capacity, ptr(pairs), ptr(gap), ptr(offsets), C.byref(total), None), "rt_scene_contacts")
        return int(total.value)
    import torch
    total = torch.full((), -1, dtype=torch.int64, device="cuda")
    qs = torch.cuda.current_stream() if stream is None else stream
    capi.check(capi.lib.rt_scene_contacts_device(d._h, margin, capacity, ptr(pairs), ptr(gap), ptr(offsets), ptr(total), None, C.c_void_p(qs.cuda_stream)),
               "rt_scene_contacts_device")
    qs.synchronize()
    return int(total.item())


@PRECISIONS
def test_every_capacity_gets_the_exact_prefix(precision):
    import torch
    R = REAL[precision]
    s = cases(precision)["refit"]
    d = rta.DeviceScene(s)
    n = len(s.items)
    margin = median_radius(s)
    ref_p, ref_g, ref_o, total = d.contacts(margin, gaps=True, offsets=True)
    assert total > 16 and len(ref_p) == total
    GUARD = 16
    for capacity in (0, 1, total - 1, total, total + 7):
        for with_pairs in (True, False):
            for entry in ("host", "device"):
                pairs = np.full((capacity + GUARD, 2), -77, np.int32)
                gap = np.full(capacity + GUARD, -77.0, R)
                offsets = np.full(n + 1 + GUARD, 77, np.uint64)
                if entry == "device":
                    pairs, gap, offsets = (torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (pairs, gap, offsets))
                got = raw(d, margin, capacity, pairs if with_pairs else None, gap if with_pairs else None, offsets, entry)
                if entry == "device":
                    pairs, gap, offsets = pairs.cpu().numpy(), gap.cpu().numpy(), offsets.cpu().numpy().view(np.uint64)
                what = (capacity, with_pairs, entry)
                assert got == total, what
                np.testing.assert_array_equal(offsets[:n + 1], ref_o, err_msg=str(what))
                assert (offsets[n + 1:] == 77).all(), what
                m = min(capacity, total) if with_pairs else 0
                np.testing.assert_array_equal(pairs[:m], ref_p[:m], err_msg=str(what))
                np.testing.assert_array_equal(bits(gap[:m], R), bits(ref_g[:m], R), err_msg=str(what))
                assert (pairs[m:] == -77).all() and (gap[m:] == -77.0).all(), what      # nothing behind the list, the guard words included
    # through the wrapper: a capacity gives the prefix, 0 the count alone
    for capacity in (0, 1, total - 1, total, total + 7):
        pairs, gap, got = d.contacts(margin, capacity, gaps=True)
        m = min(capacity, total)
        assert got == total and len(pairs) == m == len(gap)
        np.testing.assert_array_equal(pairs, ref_p[:m])
        np.testing.assert_array_equal(bits(gap, R), bits(ref_g[:m], R))
    d.close()


def check_dynamic(d, items, live, ranges, precision, what):
    """contacts() on dynamic scene d, which holds `items` with `live`, against the Walker over a fresh static scene (host side only) made
    from the live items -- a dead slot is {0, 0, 0, 0}, which pair_gaps puts at +inf as the walk does the dead record -- and bounds()."""
    R = REAL[precision]
    live = np.asarray(live) != 0
    it = np.where(live[:, None], items, 0).astype(R)
    fresh = scene_of(it, d.bounds() if ranges is not None else None, ranges, precision)
    w = Walker(fresh)
    dead = np.flatnonzero(~live)
    r = float(np.median(it[live, 3])) if live.any() else 0.1
    for margin in (0.0, r, np.inf):
        pairs, _ = assert_walk(d, w, margin, (what, margin))
        assert not np.isin(pairs, dead).any(), (what, margin)
        if margin == np.inf:
            k = int(live.sum())
            assert len(pairs) == k * (k - 1) // 2
    if live.all():                                                               # ... and a fresh device scene says the same (it takes no dead slot)
        f = rta.DeviceScene(fresh)
        same_bytes(d.contacts(r, gaps=True, offsets=True)[:3], f.contacts(r, gaps=True, offsets=True)[:3])
        f.close()


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
    check_dynamic(d, it, np.arange(CAPACITY) < half, ranges, precision, "rebuild of half")
    # n = 0: no slot is live, so no lane carries a query and no wave makes a test -- the walker says so too
    d.rebuild(sp, n=0)
    empty = Walker(scene_of(np.zeros((CAPACITY, 4), R), d.bounds(), ranges, precision)).all(np.inf)
    assert len(empty[0]) == 0 and empty[3]["bound_tests"] == 0 and empty[3]["sphere_tests"] == 0 and empty[3]["primary"] == 0
    for margin in (0.0, np.inf):
        pairs, offsets, total, st = d.contacts(margin, offsets=True, stats=True)
        assert total == 0 and len(pairs) == 0 and not offsets.any()
        assert {c: st[c] for c in COUNTERS} == empty[3]
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
    n = len(s.items)
    margin = median_radius(s)
    counters = lambda st: {c: st[c] for c in COUNTERS}
    ref = d.contacts(margin, gaps=True, offsets=True, stats=True)
    total = ref[3]
    assert total > 0
    same_bytes(ref[:3], d.contacts(margin, gaps=True, offsets=True)[:3])                             # two runs, with and without counters
    # the device entry: counted first (an int), with a capacity (nothing waited for), with counters
    dev = d.contacts(margin, gaps=True, offsets=True, device=True)
    assert all(x.device.type == "cuda" for x in dev[:3]) and dev[3] == total
    same_bytes(ref[:3], dev[:3])
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    a = d.contacts(margin, total, gaps=True, offsets=True, device=True, stream=side)
    b = d.contacts(margin, total, gaps=True, offsets=True, stats=True, device=True, stream=side.cuda_stream)
    other = torch.cuda.Stream()
    c = d.contacts(0.0, total, device=True, stream=other)                        # another margin on another stream, in between
    e = d.contacts(margin, total, gaps=True, offsets=True, device=True)
    side.synchronize()
    other.synchronize()
    torch.cuda.synchronize()
    for got in (a, b, e):
        same_bytes(ref[:3], got[:3])
        assert int(got[3].item()) == total
    assert counters(b[4]) == counters(ref[4])
    zero = d.contacts(0.0)
    assert int(c[1].item()) == zero[1] and np.array_equal(c[0].cpu().numpy()[:zero[1]], zero[0])
    # pinned host buffers (written by the kernels directly) against pageable ones
    hb = [capi.HostBuffer(x) for x in (8 * total, 4 * total, 8 * (n + 1))]
    pairs, gap, offsets = hb[0].array.view(np.int32).reshape(total, 2), hb[1].array.view(np.float32), hb[2].array.view(np.uint64)
    assert raw(d, margin, total, pairs, gap, offsets) == total
    same_bytes(ref[:3], (pairs, gap, offsets))
    # a buffer in device memory is refused by the host entry
    t = torch.zeros((total, 2), dtype=torch.int32, device="cuda")
    with pytest.raises(rta.RtError) as err:
        raw(d, margin, total, t, None, None)
    assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT
    # four threads on one scene at once, two margins
    wide = d.contacts(2 * margin, gaps=True, offsets=True)
    results, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(5):
                results[k] = d.contacts(margin * (1 + k % 2), gaps=True, offsets=True)
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


@PRECISIONS
def test_degrees_agree_with_near_where_nothing_grazes(precision):
    R = REAL[precision]
    clump_scene, _ = clump(precision)
    for name, s in (("refit", cases(precision)["refit"]), ("clump", clump_scene)):
        d = rta.DeviceScene(s)
        n = len(s.items)
        r = median_radius(s)
        centres = np.ascontiguousarray(s.items[:, :3])
        me = np.arange(n, dtype=np.int32)
        own = np.sqrt(s.items[:, 3] * s.items[:, 3])
        for margin in (0.0, r, -0.25 * r):
            pairs, grazing, (i, j) = check_brute(d, s, margin, (name, margin))
            # a sphere takes part where none of its pairs grazes, seen from either side (near measures every pair from the sphere's own centre)
            back = rta.pair_gaps(s.items, j, i).astype(np.float64)
            eps = 1e-5 if R == np.float32 else 1e-12
            grazing = grazing | (np.abs(back - float(R(margin))) <= eps * np.maximum(1.0, np.abs(back)))
            touched = np.zeros(n, bool)
            touched[i[grazing]] = True
            touched[j[grazing]] = True
            assert touched.sum() <= 0.05 * n, (name, margin)
            degree = np.bincount(pairs.reshape(-1), minlength=n)
            found = d.near(centres, 1, (R(margin) + own).astype(R), all_within=True, exclude=me)[2]
            np.testing.assert_array_equal(degree[~touched], found[~touched], err_msg=str((name, margin)))
        d.close()
