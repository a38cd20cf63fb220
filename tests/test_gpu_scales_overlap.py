"""Overlap lists and impact pairs away from unit scale and away from the origin (tests/scaled_scenes.py: the frame tests' scales 1e-20, 1e-10,
1e6 and 5e13, and translations under which c - p and c_j - c_i cancel), bit for bit and counter for counter against the yardsticks the
unit-scale suites already use, each of which takes a scene of any size:
  overlaps   the walk over the node stream with rta.overlap_gaps as its metric (tests/test_gpu_overlap.py Walker, assert_walk); brute force
             over all items on the scenes without bounds and, away from grazes, on the refit twin; the proximity query where q = 0; the
             contact pairs where the scene's own spheres are the queries; the exact prefix for every capacity; the device entry; any order
  impacts    the walk over the node stream and its motion table with rta.pair_impacts as its metric (tests/test_gpu_impacts.py Walker,
             assert_walk); brute force over all i < j on the scenes without bounds and, away from grazes, on the refit twin, where some
             impact is in neither pose's contact list; standing still and moving together; capacities; the device entry; and exact
             power-of-two scalings of the unit-scale scenes, which may not change a bit of a time
  dynamic    check_dynamic of both suites in every state of a dynamic scene: a fresh host-side scene made from the reported bounds
tests/test_scales_overlap_host.py holds the inputs to their conditions on the CPU and the two metrics to the geometry in higher precision,
so none of this passes on a scene that rounding has emptied or against a metric that is not the distance or the time.  What the
placements are for: the impact metric has terms of the fourth degree in a length, which the call's power of two S keeps normal; at 1e-20
in f32 every length of the motion table comes from the L1 rule; under the translations the differences cancel; and a wave of either walk
continues at the smallest `resume` of its lanes, so one differently rounded cull would change the tests of every other lane.  No control
of csrc/rt_debug.h is used."""
import numpy as np
import pytest

import rust_tracer_amd as rta
from tests import scaled_scenes as ss
from tests.test_gpu_dynamic import animate, scene_of
from tests.test_gpu_impacts import (FAMILIES, Walker as ImpactWalker, assert_walk as assert_impact_walk, brute_force as impact_brute_force,
                                    check_dynamic as check_dynamic_impacts, contact_keys, displacements)
from tests.test_gpu_overlap import Walker as OverlapWalker, assert_walk as assert_overlap_walk, check_dynamic as check_dynamic_overlaps, counters
from tests.test_gpu_query import REAL, bits
from tests.test_gpu_scales import release, same_bytes
from tests.test_scales_overlap_host import overlap_brute_force, unit_of

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)
LEAF = 4
CAPACITIES = lambda total: (0, 1, total - 1, total + 1)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


# ---- overlaps ----

@CASES
def test_the_overlap_lists_restate_the_walk_bit_for_bit(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        s = c.scene
        d = s.device()
        queries = ss.overlap_queries(c)
        w = OverlapWalker(s, queries)
        n, m = len(queries), len(s.items)
        if s.bounds is None:
            gap = rta.overlap_gaps(queries, s.items)
        for margin in ss.margins(c):
            what = (ss.case_id(param), c.name, margin)
            items, gaps, offsets = assert_overlap_walk(d, w, margin, what)
            if margin == np.inf:
                assert len(items) == n * m, what
            if margin == -np.inf:
                assert len(items) == 0, what
            if s.bounds is None:                                                     # every item is tested: nothing is left out
                listed = ~(gap >= R(margin))
                np.testing.assert_array_equal(items, np.nonzero(listed)[1], err_msg=str(what))
                np.testing.assert_array_equal(bits(gaps, R), bits(gap[listed], R), err_msg=str(what))
                np.testing.assert_array_equal(np.diff(offsets.astype(np.int64)), listed.sum(axis=1), err_msg=str(what))
                st = d.overlaps(queries, margin, stats=True)[-1]
                assert st["bound_tests"] == 0 and st["sphere_tests"] == n * m and st["primary"] == n, (what, st)
        release(s)


def check_overlap_brute(d, s, queries, margin, unit, what):
    """check_brute of tests/test_gpu_overlap.py with the grazing band of the placement (tests/test_scales_overlap_host.py overlap_brute_force,
    which also holds the share of grazing entries under that function's 5 %)."""
    R = REAL[s.precision]
    gap, listed, grazing = overlap_brute_force(s, queries, margin, unit)
    assert (listed & grazing).sum() <= 0.05 * max(listed.sum(), 1), what
    items, got_gap, offsets, total = d.overlaps(queries, margin, gaps=True, offsets=True)
    m = gap.shape[1]
    rows = np.repeat(np.arange(len(queries)), np.diff(offsets.astype(np.int64)))
    got_key = rows * m + items
    keep = ~grazing[rows, items]
    ref = listed & ~grazing
    gi, gj = np.nonzero(ref)
    np.testing.assert_array_equal(got_key[keep], gi * m + gj, err_msg=str(what))
    np.testing.assert_array_equal(bits(got_gap[keep], R), bits(gap[ref], R), err_msg=str(what))
    assert (np.diff(got_key) > 0).all() and total == len(items) > 0, what


@CASES
def test_the_refit_twins_are_brute_force_where_nothing_grazes(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement)[:2]:
        s = ss.refit_twin(c)
        d = rta.DeviceScene(s)
        n = len(s.items)
        unit = unit_of(c)
        queries = ss.overlap_queries(c)
        for margin in ss.margins(c)[:4]:
            check_overlap_brute(d, s, queries, margin, unit, (ss.case_id(param), c.name, margin))
        # impacts: tests/test_gpu_impacts.py check_brute (its grazing band has no dimension), and the tunnelling assertion
        for family in FAMILIES:
            what = (ss.case_id(param), c.name, family)
            disp = ss.displacements(c, family)
            i, j, t, grazing = impact_brute_force(s.items, disp, R)
            impact = t <= 1
            assert (impact & grazing).sum() <= 0.05 * max(impact.sum(), 1), what
            pairs, time, total = d.impacts(disp, times=True)
            graze_key = set((i[grazing] * n + j[grazing]).tolist())
            got_key = pairs[:, 0].astype(np.int64) * n + pairs[:, 1]
            keep = np.array([k not in graze_key for k in got_key.tolist()], bool)
            ref = impact & ~grazing
            np.testing.assert_array_equal(got_key[keep], i[ref] * n + j[ref], err_msg=str(what))
            np.testing.assert_array_equal(bits(time[keep], R), bits(t[ref], R), err_msg=str(what))
            assert (np.diff(got_key) > 0).all() and total == len(pairs) > 0, what
            if family == "fast":                                                 # a fast sphere passes through another between two poses
                start = contact_keys(s.items, precision)
                moved = s.items.copy()
                moved[:, :3] = s.items[:, :3] + disp
                end = contact_keys(moved, precision)
                through = [k for k, tm in zip(got_key.tolist(), time.tolist()) if 0.0 < tm <= 1.0 and k not in start and k not in end]
                assert len(through) >= 1, what
        d.close()


@CASES
def test_with_q_0_it_is_the_proximity_query(param):
    precision, placement = param
    R = REAL[precision]
    K = rta.RT_NEAR_MAX_K
    for c in ss.case(precision, placement):
        s = c.scene
        d = s.device()
        queries = np.array(ss.overlap_queries(c))
        queries[:, 3] = 0
        points = np.ascontiguousarray(queries[:, :3])
        r = ss.margins(c)[1]
        exclude = (np.arange(len(queries)) % len(s.items)).astype(np.int32)
        for rho in (r, 4.0 * r, 0.0, np.inf):
            for ex in (None, exclude):
                what = (ss.case_id(param), c.name, rho, ex is not None)
                items, gap, offsets, total, st = d.overlaps(queries, rho, exclude=ex, gaps=True, offsets=True, stats=True)
                ngap, nitem, found, nst = d.near(points, K, np.full(len(queries), rho, R), all_within=True, exclude=ex, want_stats=True)
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
                    assert lengths.min() > K, what                               # ... and there near stops
                if rho >= 4.0 * r:
                    assert total > 0, what
        release(s)


@CASES
def test_with_the_scenes_own_spheres_it_is_the_contact_pairs(param):
    """The scene's spheres as queries, each excluding itself: the upper half of the lists is contacts(margin) byte for byte -- on the scenes
    whose bounds enclose their items (the refit twins and the scenes without bounds: a bound of `nested` that does not enclose a query's
    own item may cull it from node 0, where the contact pairs' walk starts behind the item's node)."""
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        s = ss.refit_twin(c) if c.scene.bounds is not None else c.scene
        d = rta.DeviceScene(s)
        n = len(s.items)
        own = np.ascontiguousarray(s.items.astype(R))
        with np.errstate(under="ignore"):
            own[:, 3] = np.sqrt(s.items[:, 3] * s.items[:, 3])                   # the root of the stream's rr, in REAL
        me = np.arange(n, dtype=np.int32)
        w = OverlapWalker(s, own)
        for margin in ss.margins(c)[:3]:
            what = (ss.case_id(param), c.name, margin)
            items, gap, offsets = assert_overlap_walk(d, w, margin, what, exclude=me, home=me)
            pairs, pgap, total = d.contacts(margin, gaps=True)
            rows = np.repeat(np.arange(n), np.diff(offsets.astype(np.int64)))
            assert (items != rows).all() and total > 0, what
            upper = items > rows
            np.testing.assert_array_equal(np.stack([rows[upper], items[upper]], axis=1), pairs, err_msg=str(what))
            np.testing.assert_array_equal(bits(gap[upper], R), bits(pgap, R), err_msg=str(what))
        d.close()


@CASES
def test_overlap_capacities_the_device_entry_and_any_order(param):
    import torch
    precision, placement = param
    R = REAL[precision]
    for k, c in enumerate(ss.case(precision, placement)):
        s = c.scene
        d = s.device()
        queries = np.array(ss.overlap_queries(c))
        n = len(queries)
        margin = ss.margins(c)[1]
        ref_i, ref_g, ref_o, total = d.overlaps(queries, margin, gaps=True, offsets=True)
        assert total > 2 and len(ref_i) == total
        for capacity in CAPACITIES(total):
            what = (ss.case_id(param), c.name, "capacity", capacity)
            items, gaps, offsets, got = d.overlaps(queries, margin, capacity=capacity, gaps=True, offsets=True)
            m = min(capacity, total)
            assert got == total and len(items) == m == len(gaps), what
            same_bytes((items, gaps, offsets), (ref_i[:m], ref_g[:m], ref_o), what)
        dq = torch.from_numpy(queries).cuda()
        dev = d.overlaps(dq, margin, gaps=True, offsets=True)
        assert dev[3] == total
        same_bytes((ref_i, ref_g, ref_o), [host(x) for x in dev[:3]], (ss.case_id(param), c.name, "device entry"))
        # exclude, in the four orders: the same bytes and the same counters
        exclude = np.random.default_rng(600 + k).integers(-1, len(s.items) + 3, n).astype(np.int32)
        assert_overlap_walk(d, OverlapWalker(s, queries), margin, (ss.case_id(param), c.name, "exclude"), exclude=exclude)
        ref = d.overlaps(queries, margin, exclude=exclude, gaps=True, offsets=True, stats=True)
        assert ref[3] < total                                                     # something was excluded
        coherent = d.sphere_order(np.ascontiguousarray(np.concatenate([queries[:, :3], np.ones((n, 1), R)], axis=1)))
        orders = {"identity": np.arange(n, dtype=np.uint32), "reversed": np.arange(n, dtype=np.uint32)[::-1].copy(),
                  "random": np.random.default_rng(700 + k).permutation(n).astype(np.uint32), "sphere_order": coherent}
        for name, order in orders.items():
            what = (ss.case_id(param), c.name, name)
            assert sorted(order.tolist()) == list(range(n)), what                # a permutation at this placement
            got = d.overlaps(queries, margin, exclude=exclude, order=order, gaps=True, offsets=True, stats=True)
            same_bytes(ref[:3], got[:3], what)
            assert got[3] == ref[3] and counters(got[4]) == counters(ref[4]), what
        release(s)


# ---- impacts ----

@CASES
def test_the_impact_lists_restate_the_walk_bit_for_bit(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        s = c.scene
        d = s.device()
        w = ImpactWalker(s)
        n = len(s.items)
        every = n * (n - 1) // 2
        i, j = np.triu_indices(n, 1)
        for family in FAMILIES:
            what = (ss.case_id(param), c.name, family)
            disp = ss.displacements(c, family)
            pairs, time, st = assert_impact_walk(d, w, disp, what)
            assert 0 < len(pairs) < every and (time == 0).any() and (time > 0).any(), what
            if s.bounds is None:                                                     # every later item is tested: all i < j, exactly
                t = rta.pair_impacts(s.items, disp, i, j)
                impact = t <= 1
                np.testing.assert_array_equal(pairs, np.stack([i[impact], j[impact]], axis=1), err_msg=str(what))
                np.testing.assert_array_equal(bits(time, R), bits(t[impact], R), err_msg=str(what))
                assert st["bound_tests"] == 0 and st["sphere_tests"] == every and st["primary"] == n, (what, st)
        release(s)


@CASES
def test_standing_still_and_moving_together_list_the_pairs_in_contact(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement)[:2]:
        s = ss.refit_twin(c)
        what = (ss.case_id(param), c.name)
        d = rta.DeviceScene(s)
        n = len(s.items)
        unit = unit_of(c)
        zero = np.zeros((n, 3), R)
        pairs, time, total = d.impacts(zero, times=True)
        assert total == len(pairs) > 0 and (time == 0).all(), what
        # away from a gap within 1e-5 max(unit, r_i + r_j) of 0 (f64: 1e-12) they are the pairs of contacts(0); unit: what 1 stands for here
        cp, gap, _ = d.contacts(0.0, gaps=True)
        i, j = np.triu_indices(n, 1)
        g = rta.pair_gaps(s.items, i, j).astype(np.float64)
        eps = 1e-5 if R == np.float32 else 1e-12
        near0 = set((i * n + j)[np.abs(g) <= eps * np.maximum(unit, s.items[i, 3] + s.items[j, 3])].tolist())
        key = lambda p: [k for k in (p[:, 0].astype(np.int64) * n + p[:, 1]).tolist() if k not in near0]
        assert key(pairs) == key(cp) and len(key(cp)) >= 0.75 * len(cp) > 0, what
        # one displacement for every sphere: w = 0 for every pair, the list of disp = 0
        for move in ((0.25, -0.5, 0.125), (-3.0, 0.0, 0.0)):
            together = np.ascontiguousarray(np.broadcast_to((np.array(move) * unit).astype(R), (n, 3)))
            p2, t2, total2 = d.impacts(together, times=True)
            np.testing.assert_array_equal(p2, pairs, err_msg=str((what, move)))
            assert (t2 == 0).all() and total2 == total, (what, move)
        d.close()


@CASES
def test_impact_capacities_and_the_device_entry(param):
    import torch
    precision, placement = param
    for c in ss.case(precision, placement):
        s = c.scene
        d = s.device()
        disp = np.array(ss.displacements(c, "fast"))
        ref_p, ref_t, ref_o, total = d.impacts(disp, times=True, offsets=True)
        assert total > 2 and len(ref_p) == total
        for capacity in CAPACITIES(total):
            what = (ss.case_id(param), c.name, "capacity", capacity)
            if capacity == 0:
                pairs, offsets, got = d.impacts(disp, 0, offsets=True)
                assert got == total and len(pairs) == 0, what
                same_bytes((offsets,), (ref_o,), what)
                continue
            pairs, time, offsets, got = d.impacts(disp, capacity, times=True, offsets=True)
            m = min(capacity, total)
            assert got == total and len(pairs) == m == len(time), what
            same_bytes((pairs, time, offsets), (ref_p[:m], ref_t[:m], ref_o), what)
        dev = d.impacts(torch.from_numpy(disp).cuda(), times=True, offsets=True)
        assert dev[3] == total
        same_bytes((ref_p, ref_t, ref_o), [host(x) for x in dev[:3]], (ss.case_id(param), c.name, "device entry"))
        release(s)


POW2_CASES = [(p, k) for p in (rta.RT_F32, rta.RT_F64) for k in ss.POW2]


@pytest.mark.parametrize("precision,k", POW2_CASES, ids=["%s-2^%d" % ("f32" if p == rta.RT_F32 else "f64", k) for p, k in POW2_CASES])
def test_a_power_of_two_scaling_changes_no_bit_on_the_device(precision, k):
    """The unit-scale base scenes and their displacements times 2^k: the scenes without bounds list the unit-scale pairs with the unit-scale
    time bits, and the bounded scenes (items and bounds scaled alike) restate their own walker.  At 2^-66 in f32 r * r is a denormal: the
    lists agree because the radius is the scene's r and not the root of the stream's rr."""
    R = REAL[precision]
    light = rta.normalized(ss.LIGHT, precision)
    i = j = None
    for index, (name, items0, bounds0, ranges) in enumerate(ss.base_scenes()):
        items0 = np.ascontiguousarray(np.asarray(items0, dtype=np.float64).reshape(-1, 4).astype(R))
        n = len(items0)
        for family in FAMILIES:
            what = (name, family, k)
            disp0 = displacements(items0, 900 + index, family, R)
            items, disp = ss.pow2_scaled(items0, disp0, k, R)
            if bounds0 is None:
                unit = rta.DeviceScene(rta.Scene(items0, light, ss.EYE, precision=precision))
                ref_p, ref_t, _ = unit.impacts(disp0, times=True)
                unit.close()
                d = rta.DeviceScene(rta.Scene(items, light, ss.EYE, precision=precision))
                pairs, time, total = d.impacts(disp, times=True)
                d.close()
                i, j = np.triu_indices(n, 1)
                t = rta.pair_impacts(items, disp, i, j)
                np.testing.assert_array_equal(pairs, np.stack([i[t <= 1], j[t <= 1]], axis=1), err_msg=str(what))
                np.testing.assert_array_equal(bits(time, R), bits(t[t <= 1], R), err_msg=str(what))
                assert total == len(ref_p) > 0, what
                np.testing.assert_array_equal(pairs, ref_p, err_msg=str(what))
                np.testing.assert_array_equal(bits(time, R), bits(ref_t, R), err_msg=str(what))
            else:
                bounds = np.ldexp(np.asarray(bounds0, dtype=np.float64).reshape(-1, 4).astype(R), k).astype(R)
                s = rta.Scene(items, light, ss.EYE, bounds, ranges, precision)
                d = rta.DeviceScene(s)
                pairs, time, st = assert_impact_walk(d, ImpactWalker(s), disp, what)
                d.close()
                assert len(pairs) > 0, what


# ---- dynamic and live scenes ----

@CASES
def test_overlaps_and_impacts_follow_updates_rebuilds_and_kills(param):
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
        queries = ss.overlap_queries(c)
        d = rta.DeviceScene(scene_of(it0, rta.refit_bounds(it0, rg, precision), rg, precision), dynamic=True)

        def hold(items, live, state):
            check_dynamic_overlaps(d, items, live, rg, precision, what + state, queries=queries)
            for family in FAMILIES:
                check_dynamic_impacts(d, items, live, ss.displacements(c, family), rg, precision, what + state + ", " + family)

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
