"""Sphere casts and contact pairs away from unit scale and away from the origin (tests/scaled_scenes.py: the frame tests' scales 1e-20, 1e-10,
1e6 and 5e13, and translations under which c - o and c_j - c_i cancel), bit for bit and counter for counter against the yardsticks the
unit-scale suites already use, each of which takes a scene of any size:
  casts      the walk over the node stream with rta.sweep_distances as its metric (tests/test_gpu_sweep.py Walker, assert_walk); brute force
             over all items on the scenes without bounds, no cast left out; with radius 0 from outside the root DeviceScene.intersect, and
             through it the oracle (tests/test_gpu_query.py check_nearest): the one place the casts meet the reference's own arithmetic
  contacts   the walk over the node stream with rta.pair_gaps as its metric (tests/test_gpu_contacts.py Walker, assert_walk); brute force
             over all i < j on the scenes without bounds; the exact prefix for every capacity; the device entry
  dynamic    check_dynamic of both suites in every state of a dynamic scene: a fresh host-side scene made from the reported bounds
tests/test_scales_contact_host.py holds the inputs to their conditions on the CPU (contacts, misses, starts in contact, cutoffs that bite,
culls, margins that list some pairs and not all) and the two metrics to the geometry in higher precision, so none of this passes on a
scene that rounding has emptied or against a metric that is not the distance.  What the placements are for: at 1e-20 in f32 rr,
(q + q) * sqrt(rr) and q * q are all denormals, sqrt(rr) is not r, and the start clamp and the rr > 0 guard decide on a few ulp of the
denormal range; at 5e13 q * q reaches 2e29; under the translations the differences cancel; and a contacts wave resumes at the smallest
`resume` of its lanes, so one differently rounded cull would change the tests of every other lane.  No control of csrc/rt_debug.h is used."""
import numpy as np
import pytest

import rust_tracer_amd as rta
from tests import scaled_scenes as ss
from tests.test_gpu_contacts import Walker as PairWalker, assert_walk as assert_pair_walk, check_dynamic as check_dynamic_contacts, median_radius
from tests.test_gpu_dynamic import animate, scene_of
from tests.test_gpu_query import REAL, bits, check_nearest
from tests.test_gpu_scales import counters, release, same_bytes
from tests.test_gpu_sweep import (Walker as CastWalker, assert_reals, assert_walk as assert_cast_walk, check_dynamic as check_dynamic_casts,
                                  normals, two_smallest)

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)
LEAF = 4


# ---- casts ----

@CASES
def test_the_casts_restate_the_walk_bit_for_bit(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        s = c.scene
        d = s.device()
        rays, radius, which, tmax = ss.casts(c)
        w = CastWalker(s, rays, radius)
        for any_hit in (False, True):
            what = (ss.case_id(param), c.name, any_hit)
            res = d.sweep(rays, radius, tmax, any_hit=any_hit, want_stats=True)
            assert_cast_walk(res, w.all(tmax, any_hit), w, R, what)
            dist, nrm, item = res[:3]
            np.testing.assert_array_equal(item >= 0, dist < tmax, err_msg=str(what))
            np.testing.assert_array_equal(bits(dist[item < 0], R), bits(tmax[item < 0], R), err_msg=str(what))
            assert not nrm[item < 0].any(), what
            assert (item >= 0).any() and (item < 0).any(), what
            same_bytes(d.sweep(rays, radius, tmax, any_hit=any_hit), res[:3], what)              # the launch without counters
        release(s)


@CASES
def test_the_casts_of_a_scene_without_bounds_are_brute_force_exactly(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        s = c.scene
        if s.bounds is not None:
            continue
        what = (ss.case_id(param), c.name)
        d = s.device()
        rays, radius, which, tmax = ss.casts(c)
        n_items = len(s.items)
        first, slot, _ = two_smallest(rays, radius, s.items)                         # the row minimum and its lowest slot
        hit = first < tmax
        ref_d, ref_i = np.where(hit, first, tmax).astype(R), np.where(hit, slot, -1).astype(np.int32)
        dist, nrm, item, st = d.sweep(rays, radius, tmax, want_stats=True)           # the flat stream is never culled: no cast is left out
        np.testing.assert_array_equal(bits(dist, R), bits(ref_d, R), err_msg=str(what))
        np.testing.assert_array_equal(item, ref_i, err_msg=str(what))
        assert_reals(nrm, normals(rays, ref_d, ref_i, s.items), R, what)
        assert st["bound_tests"] == 0 and st["sphere_tests"] == len(rays) * n_items, (what, st)
        dist, nrm, item, st = d.sweep(rays, radius, tmax, any_hit=True, want_stats=True)
        np.testing.assert_array_equal(item >= 0, ref_i >= 0, err_msg=str(what))
        assert st["bound_tests"] == 0 and st["sphere_tests"] == sum(int(i) + 1 if i >= 0 else n_items for i in item), (what, st)
        release(s)


@CASES
def test_radius_0_from_outside_the_root_is_the_ray_query_and_the_oracle(param):
    precision, placement = param
    for c in ss.case(precision, placement):
        s = c.scene
        d = s.device()
        rays, zeros, tmax = ss.ray_casts(c)              # (tests/test_scales_contact_host.py: no record is entered at or below 0, every rr > 0)
        check_nearest(s, c.oracle, rays, tmax, c.mode)                              # DeviceScene.intersect against the reference
        for t in (tmax, None):
            for any_hit in (False, True):
                what = (ss.case_id(param), c.name, t is None, any_hit)
                want = d.intersect(rays, t, any_hit=any_hit, want_stats=True)
                for q in (None, zeros, 0.0):
                    got = d.sweep(rays, q, t, any_hit=any_hit, want_stats=True)
                    same_bytes(want[:3], got[:3], what)
                    assert counters(got[3]) == counters(want[3]), what
                assert (want[2] >= 0).any() and (want[2] < 0).any(), what
        release(s)


@CASES
def test_self_casts_and_exclude(param):
    """Every item cast from its own centre with its own radius.  At 1e-20 in f32 the clamp to 0 is what puts ANY's answer below the smallest
    normal number: b and the root are denormals there, and their difference is whatever the roundings leave."""
    precision, placement = param
    R = REAL[precision]
    for k, c in enumerate(ss.case(precision, placement)):
        s = c.scene
        d = s.device()
        n = len(s.items)
        rng = np.random.default_rng(500 + k)
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        rays = np.ascontiguousarray(np.concatenate([s.items[:, :3].astype(np.float64), u], axis=1).astype(R))
        radius = np.ascontiguousarray(s.items[:, 3])
        me = np.arange(n, dtype=np.int32)
        w = CastWalker(s, rays, radius)
        # without exclude a cast overlaps its own sphere at its start: 0 and an item, in NEAREST without a cutoff and in ANY below the
        # smallest normal number (only a start overlap lies below that).  The walk is the definition: where a bound of `nested` that does
        # not enclose its items is culled with the cast's own item inside, the cast finds what the walk finds -- nothing there
        for any_hit, tmax in ((False, None), (True, np.finfo(R).tiny)):
            what = (ss.case_id(param), c.name, "self", any_hit)
            res = d.sweep(rays, radius, tmax, any_hit=any_hit, want_stats=True)
            assert_cast_walk(res, w.all(np.full(n, np.inf if tmax is None else tmax, R), any_hit), w, R, what)
            dist, nrm, item = res[:3]
            assert (dist[item >= 0] == 0).all() and (item >= 0).sum() >= 0.9 * n, what
            if c.name != "nested":
                assert (item >= 0).all(), what
        t = rta.sweep_distances(rays, radius, s.items)
        t[me, me] = np.inf
        first = t.min(axis=1).astype(np.float64)
        tmax = np.where(np.arange(n) % 3 == 0, np.inf, np.where(np.isfinite(first) & (first > 0), first, 1.0) * rng.uniform(0.3, 3.0, n)).astype(R)
        for any_hit in (False, True):
            what = (ss.case_id(param), c.name, "exclude", any_hit)
            res = d.sweep(rays, radius, tmax, any_hit=any_hit, exclude=me, want_stats=True)
            assert_cast_walk(res, w.all(tmax, any_hit, me), w, R, what)
            assert not (res[2] == me).any(), what
            assert (res[2] >= 0).any(), what
        release(s)


@CASES
def test_any_order_of_the_casts_gives_the_same_bytes_and_counters(param):
    precision, placement = param
    for k, c in enumerate(ss.case(precision, placement)):
        s = c.scene
        d = s.device()
        rays, radius, which, tmax = ss.casts(c)
        n = len(rays)
        exclude = np.random.default_rng(600 + k).integers(-1, len(s.items), n).astype(np.int32)
        perm = np.random.default_rng(700 + k).permutation(n).astype(np.uint32)
        coherent = d.sphere_order(np.ascontiguousarray(np.concatenate([rays[:, :3], np.ones((n, 1), rays.dtype)], axis=1)))
        assert sorted(coherent.tolist()) == list(range(n)), (ss.case_id(param), c.name)             # a permutation at this placement
        for any_hit in (False, True):
            what = (ss.case_id(param), c.name, any_hit)
            ref = d.sweep(rays, radius, tmax, any_hit=any_hit, exclude=exclude, want_stats=True)
            for order in (np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)[::-1], perm, coherent):
                got = d.sweep(rays, radius, tmax, any_hit=any_hit, exclude=exclude, want_stats=True, order=order)
                same_bytes(ref[:3], got[:3], what)
                assert counters(got[3]) == counters(ref[3]), what
        release(s)


# ---- contacts ----

@CASES
def test_the_contact_lists_restate_the_walk_bit_for_bit(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        s = c.scene
        d = s.device()
        w = PairWalker(s)
        n = len(s.items)
        margins = ss.margins(c)
        assert margins[1] == median_radius(s)
        if s.bounds is None:
            i, j = np.triu_indices(n, 1)
            gap = rta.pair_gaps(s.items, i, j)
        for margin in margins:
            what = (ss.case_id(param), c.name, margin)
            pairs, gaps = assert_pair_walk(d, w, margin, what)
            if margin == np.inf:
                assert len(pairs) == n * (n - 1) // 2, what
            if margin == -np.inf:
                assert len(pairs) == 0, what
            if s.bounds is None:                                                     # every later item is tested: all i < j, exactly
                contact = ~(gap >= R(margin))
                np.testing.assert_array_equal(pairs, np.stack([i[contact], j[contact]], axis=1), err_msg=str(what))
                np.testing.assert_array_equal(bits(gaps, R), bits(gap[contact], R), err_msg=str(what))
        # every capacity gets the exact prefix and the full total; the device entry gives the host entry's bytes
        margin = margins[1]
        ref_p, ref_g, ref_o, total = d.contacts(margin, gaps=True, offsets=True)
        assert total > 2 and len(ref_p) == total
        for capacity in (0, 1, total - 1, total + 1):
            what = (ss.case_id(param), c.name, "capacity", capacity)
            pairs, gaps, offsets, got = d.contacts(margin, capacity, gaps=True, offsets=True)
            m = min(capacity, total)
            assert got == total and len(pairs) == m == len(gaps), what
            same_bytes((pairs, gaps, offsets), (ref_p[:m], ref_g[:m], ref_o), what)
        dev = d.contacts(margin, gaps=True, offsets=True, device=True)
        assert dev[3] == total
        same_bytes((ref_p, ref_g, ref_o), [x.cpu().numpy() for x in dev[:3]], (ss.case_id(param), c.name, "device entry"))
        release(s)


# ---- dynamic and live scenes ----

@CASES
def test_casts_and_contacts_follow_updates_rebuilds_and_kills(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        if c.scene.bounds is None:
            continue                                                 # (the same items as the bounded twin)
        what = "%s %s: " % (ss.case_id(param), c.name)
        it0 = np.ascontiguousarray(c.items.astype(R))
        n = len(it0)
        rg = rta.balanced_ranges(n, LEAF)
        everyone = np.ones(n, dtype=np.uint8)
        d = rta.DeviceScene(scene_of(it0, rta.refit_bounds(it0, rg, precision), rg, precision), dynamic=True)

        def hold(items, live, state):
            check_dynamic_casts(d, items, live, rg, precision, what + state)
            check_dynamic_contacts(d, items, live, rg, precision, what + state)

        hold(it0, everyone, "as created")
        moved = animate(it0, 2, R)
        assert not np.array_equal(moved, it0)
        d.update(moved)
        hold(moved, everyone, "updated")
        sh = ss.shuffled(it0, R)
        order = d.rebuild(sh)
        cur = np.ascontiguousarray(sh[order])
        hold(cur, everyone, "rebuilt")
        live = (np.arange(n) % 3 != 0).astype(np.uint8)
        d.update(cur, live=live)
        hold(cur, live, "every third slot dead")
        half = n // 2
        order = d.rebuild(sh, n=half)
        cur = np.zeros((n, 4), dtype=R)
        cur[:half] = sh[:half][order]
        hold(cur, (np.arange(n) < half).astype(np.uint8), "rebuild of half")
        assert (d.bounds()[:, 3] == 0).any()                         # dead groups among them
        d.close()
