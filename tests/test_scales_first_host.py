"""First contacts (rt_first_contacts*, csrc/rt_first.hpp) away from unit scale and away from the origin, without a GPU:
the placements of tests/scaled_scenes.py (uniform scales 1e-20, 1e-10, 1e6, 5e13 and the translations where c - p cancels) with numpy,
the walkers and the host side of the package.
  - rta.swept_times, the metric of both swept entries, against the geometry in higher precision at every placement: until here it was
    held to geometry at unit scale only (tests/test_swept_host.py), so "earliest touch" had no reference there that the package did not
    write itself;
  - FirstWalker -- what the GPU is held to bit for bit -- against Walker.all at every placement, with no allowance: the place where the
    hazard DESIGN.md 4.20 documents (a bound's tm above that of an item below it by rounding) would show, if anywhere;
  - FirstWalker's result against the geometry itself, on the scenes whose bounds enclose: hold_to_geometry(), which
    tests/test_gpu_scales_first.py applies to the GPU's result too;
  - exact scalings by powers of two, which change no bit of time, item or normal."""
import numpy as np
import pytest

import rust_tracer_amd as rta
from tests import scaled_scenes as ss
from tests.test_gpu_first import FirstWalker
from tests.test_gpu_impacts import FAMILIES
from tests.test_gpu_near import scene_of
from tests.test_gpu_query import REAL
from tests.test_gpu_swept import placed_inputs
from tests.test_scales_contact_host import higher
from tests.test_swept_host import BITS, judge, scaled

CASES = pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)
UNJUDGED_CAP = 0.01                          # tests/test_swept_host.py's own: the share of (query, item) pairs no decision is clear for
DOMAIN = 1e15                                # the entries refuse a coordinate, a radius or a displacement beyond it (include/rtrace_hip.h)
UNDECIDED_CAP = 0.05                         # the share of queries with a pair that is neither surely touched nor surely missed


def enclosing_scenes(cases):
    """[(name, Case, rta.Scene)] of one placement whose bounds enclose their items, so that the walk's result is the scene's: the refit
    twins of the bounded cases, and the scenes without bounds."""
    return [(c.name + ("_refit" if c.bounds is not None else ""), c, ss.refit_twin(c) if c.bounds is not None else c.scene) for c in cases]


def all_scenes(cases):
    """enclosing_scenes() and, in front of them, the nested scenes as made (some of their bounds do not enclose: the result is the walk's)."""
    return [(c.name, c, c.scene) for c in cases if c.bounds is not None] + enclosing_scenes(cases)


def motions(c):
    """(family, moving, queries, qdisp, disp or None) of Case c: both families, the scene moving and standing."""
    for family in FAMILIES:
        queries, qdisp, disp = placed_inputs(c, family)
        for moving in (True, False):
            yield family, moving, queries, qdisp, disp if moving else None


@CASES
def test_swept_times_is_the_time_of_first_touch_at_every_placement(param):
    """tests/test_swept_host.py test_swept_times_is_the_time_a_moving_query_first_touches_a_moving_sphere at every placement: every (query,
    item) of the first two cases, one item dead, both families, the scene moving and standing, against judge() in higher precision.
    The four decisions wherever they are clear, |t - T| <= tol on `front`, the sure side of t <= 1, every class non-empty, and at most
    1 % of the pairs unjudged."""
    precision, placement = param
    R = REAL[precision]
    H, u = higher(precision)
    u = H(u)
    worst_all = unjudged_all = 0.0
    for c in ss.case(precision, placement)[:2]:
        items = np.ascontiguousarray(c.scene.items.astype(R))
        items[7, 3] = 0                                                          # one dead slot
        for family, moving, queries, qdisp, disp in motions(c):
            what = (ss.case_id(param), c.name, family, "moving" if moving else "standing")
            t = rta.swept_times(queries, qdisp, items, disp).astype(H)
            cls, T, tol, judged = judge(t, queries, qdisp, items, np.zeros((len(items), 3), R) if disp is None else disp, H, u)
            dead, start, away, by, front = (cls[k] for k in ("dead", "start", "away", "by", "front"))
            assert dead.any() and start.any() and away.any() and by.any() and front.any(), what
            worst = float(np.max(np.abs(t[front] - T[front]) / tol[front]))
            unjudged = 1.0 - judged.mean()
            worst_all, unjudged_all = max(worst_all, worst), max(unjudged_all, unjudged)
            print("%s: %d dead, %d in contact at the start, %d not approaching, %d passing by, %d in front of %d pairs, %.3f %% unjudged; "
                  "the worst error is %.3f of its bound" % (what, dead.sum(), start.sum(), away.sum(), by.sum(), front.sum(), judged.size, 100.0 * unjudged, worst))
            assert unjudged <= UNJUDGED_CAP, (what, unjudged)
            for sel in (dead, away, by):
                assert np.isinf(t[sel]).all() and (t[sel] > 0).all(), what
            assert (t[start] == 0).all(), what
            assert np.isfinite(t[front]).all() and (t[front] > 0).all(), what
            assert (np.abs(t[front] - T[front]) <= tol[front]).all(), (what, worst)
            sure = front & (np.abs(T - 1) > tol)
            assert ((t[sure] <= 1) == (T[sure] <= 1)).all() and (t[sure] <= 1).any() and (t[sure] > 1).any(), what
    print("%s: worst of all %.3f of the bound, at most %.3f %% unjudged" % (ss.case_id(param), worst_all, 100.0 * unjudged_all))


def check_rows(w, queries, qdisp, disp, what):
    """FirstWalker w against its own Walker.all on one input: a result exists exactly where the row is not empty, ANY is the row's first
    entry, NEAREST the row's smallest time at its lowest slot with that entry's time and normal bits -- for every query, no allowance --
    and NEAREST makes no more tests than the list's count walk.  -> the NEAREST items."""
    U = BITS[w.R]
    items, times, normals, offsets, list_st = w.all(queries, qdisp, disp)
    time, item, normal, st = w.first(queries, qdisp, disp)
    a_time, a_item, a_normal, a_st = w.first(queries, qdisp, disp, any_hit=True)
    o = offsets.astype(np.int64)
    for g in range(len(queries)):
        row_i, row_t, row_n = items[o[g]:o[g + 1]], times[o[g]:o[g + 1]], normals[o[g]:o[g + 1]]
        assert (item[g] >= 0) == (a_item[g] >= 0) == (len(row_i) > 0), (what, g)
        if not len(row_i):
            assert np.isinf(time[g]) and not normal[g].any() and np.isinf(a_time[g]), (what, g)
            continue
        k = int(np.flatnonzero(row_t == row_t.min())[0])                         # the smallest time at its lowest slot
        # a failure here is DESIGN.md 4.20's hazard made real: the query, the row and the two times are in the message
        assert item[g] == row_i[k] and time[g].view(U) == row_t[k].view(U), (what, g, queries[g], qdisp[g], row_i, row_t, item[g], time[g])
        assert (normal[g].view(U) == row_n[k].view(U)).all(), (what, g)
        assert a_item[g] == row_i[0] and a_time[g].view(U) == row_t[0].view(U) and (a_normal[g].view(U) == row_n[0].view(U)).all(), (what, g)
    assert st["hits"] == a_st["hits"] == list_st["hits"] and st["primary"] == list_st["primary"], what
    assert a_st["tests_executed"] <= st["tests_executed"] <= list_st["tests_executed"], (what, a_st, st, list_st)
    return item


@CASES
def test_the_walker_returns_the_rows_smallest_time_at_its_lowest_slot_at_every_placement(param):
    """tests/test_first_host.py's comparison of FirstWalker with Walker.all, at every placement: the nested scenes as made, their refit
    twins and the scenes without bounds, both families, the scene moving and standing, NEAREST and ANY."""
    precision, placement = param
    combinations = 0
    for name, c, s in all_scenes(ss.case(precision, placement)):
        w = FirstWalker(s)
        for family, moving, queries, qdisp, disp in motions(c):
            what = (ss.case_id(param), name, family, "moving" if moving else "standing")
            item = check_rows(w, queries, qdisp, disp, what)
            assert (item >= 0).any() and (item < 0).any(), what
            combinations += 2
    print("%s: %d combinations agree" % (ss.case_id(param), combinations))


def hold_to_geometry(time, item, queries, qdisp, items, disp, precision, what):
    """One first-contacts result (NEAREST) of a scene whose bounds enclose, against the geometry in higher precision.  With judge()'s classes,
    T and tol, an item is SURELY TOUCHED when it is `start`, or `front` with T + tol <= 1; SURELY MISSED when it is `dead`, `away`, `by`, or
    `front` with T - tol > 1; a query is DECIDED when every item is one or the other.  A decided query with no surely touched item has no
    result.  A decided query with one has a surely touched item k as its result, with |time - T[k]| <= tol[k] (time == 0 if k is
    `start`), and min (T - tol) <= time <= min (T + tol) over the surely touched items, `start` counting as 0: the result is the
    earliest touch within the reference's own error.  At most 5 % of the queries may be undecided; the message carries the share.
    -> the number of decided queries."""
    R = REAL[precision]
    H, u = higher(precision)
    n = len(queries)
    d = np.zeros((len(items), 3), R) if disp is None else disp
    cls, T, tol, _ = judge(None, queries, qdisp, np.ascontiguousarray(np.asarray(items).astype(R)), d, H, H(u))
    with np.errstate(invalid="ignore"):
        touched = cls["start"] | (cls["front"] & (T + tol <= 1))
        missed = cls["dead"] | cls["away"] | cls["by"] | (cls["front"] & (T - tol > 1))
    decided = (touched | missed).all(axis=1)
    share = "%s: %d of %d queries decided (%.2f %% undecided)" % (what, decided.sum(), n, 100.0 * (1.0 - decided.mean()))
    assert 1.0 - decided.mean() <= UNDECIDED_CAP, share
    lo = np.where(touched, np.where(cls["start"], H(0.0), T - tol), H(np.inf))
    hi = np.where(touched, np.where(cls["start"], H(0.0), T + tol), H(np.inf))
    for g in np.flatnonzero(decided):
        if not touched[g].any():
            assert item[g] == -1 and np.isinf(time[g]), (share, g, item[g], time[g])
            continue
        k, t = int(item[g]), H(time[g])
        assert k >= 0 and touched[g, k], (share, g, k, time[g], np.flatnonzero(touched[g]))
        if cls["start"][g, k]:
            assert t == 0, (share, g, k, time[g])
        else:
            assert abs(t - T[g, k]) <= tol[g, k], (share, g, k, time[g], T[g, k], tol[g, k])
        assert lo[g].min() <= t <= hi[g].min(), (share, g, k, time[g], lo[g].min(), hi[g].min())
    assert (item >= 0).any() and (item < 0).any(), share
    return int(decided.sum())


@CASES
def test_the_walkers_result_is_the_earliest_touch_of_the_geometry(param):
    """hold_to_geometry() on FirstWalker's NEAREST result: the refit twins and the scenes without bounds of every placement, both families,
    the scene moving and standing."""
    precision, placement = param
    higher(precision)
    decided = total = 0
    least = 1.0
    for name, c, s in enclosing_scenes(ss.case(precision, placement)):
        w = FirstWalker(s)
        for family, moving, queries, qdisp, disp in motions(c):
            what = (ss.case_id(param), name, family, "moving" if moving else "standing")
            time, item, _, _ = w.first(queries, qdisp, disp)
            k = hold_to_geometry(time, item, queries, qdisp, s.items, disp, precision, what)
            print("%s: %d of %d decided, %d with a result" % (what, k, len(queries), (item >= 0).sum()))
            decided, total, least = decided + k, total + len(queries), min(least, k / len(queries))
    print("%s: %d of %d queries decided, at least %.2f %% in every combination" % (ss.case_id(param), decided, total, 100.0 * least))


@CASES
def test_an_exact_scaling_keeps_every_bit_of_the_first_contact(param):
    """The time has no dimension, the normal is a direction and the item is a slot: FirstWalker on the placed scenes whose bounds enclose
    (the first refit twin and the first scene without bounds), both families, the scene moving and standing, NEAREST and ANY, gives the
    same bits when every length is multiplied by 2^k, k in scaled_scenes.POW2 -- wherever that product is exact and leaves every item
    alive (tests/test_swept_host.py's `scaled`: a factor that takes an input out of the normal range is no scaling of that placement
    and is left out) and inside the entry's domain of 1e15, beyond which the table's squared lengths may overflow.  The bounds are refit from the scaled items, as a caller would.  Not the counters: a displacement shorter than the
    square root of refit_tiny takes its length from the L1 rule, so a bound's D -- never an item's time -- depends on the scale."""
    precision, placement = param
    R = REAL[precision]
    U = BITS[R]
    used = set()
    cases = ss.case(precision, placement)
    for c in (cases[0], cases[2]):
        items = np.ascontiguousarray(c.scene.items.astype(R))
        ranges = c.ranges

        def scene(it):
            return scene_of(it, None if ranges is None else rta.refit_bounds(it, ranges, precision), ranges, precision)
        w = FirstWalker(scene(items))
        for family, moving, queries, qdisp, disp in motions(c):
            ref = {any_hit: w.first(queries, qdisp, disp, any_hit=any_hit) for any_hit in (False, True)}
            assert (ref[False][1] >= 0).any() and (ref[False][1] < 0).any(), (c.name, family, moving)
            for k in ss.POW2:
                (q2, qd2, it2, d2), exact = scaled((queries, qdisp, items, disp), k, R)
                if not exact or max(float(np.abs(a).max()) for a in (q2, qd2, it2)) > DOMAIN:
                    continue
                used.add(k)
                w2 = FirstWalker(scene(it2))
                for any_hit in (False, True):
                    what = (ss.case_id(param), c.name, family, moving, k, any_hit)
                    time, item, normal, _ = w2.first(q2, qd2, d2, any_hit=any_hit)
                    np.testing.assert_array_equal(time.view(U), ref[any_hit][0].view(U), err_msg=str(what))
                    np.testing.assert_array_equal(item, ref[any_hit][1], err_msg=str(what))
                    np.testing.assert_array_equal(normal.view(U), ref[any_hit][2].view(U), err_msg=str(what))
    assert used, param
    if placement in ("+3e3", "+3e9"):                                            # (their 2^45 lies beyond 1e15, and 3e9 times 2^33 too)
        assert used >= {k for k in ss.POW2 if k < 0}, (param, used)
