"""The inputs and the yardsticks of tests/test_gpu_scales_overlap.py, checked without a GPU: the query spheres and the displacements that
tests/scaled_scenes.py gives every placed scene (the frame tests' scales 1e-20, 1e-10, 1e6 and 5e13, and the translations under which
c - p and c_j - c_i cancel), for the overlap lists and the impact pairs (4.18).
  - Conditions on the inputs, with the tests' own walkers (pure numpy): every margin lists some entries and not all, some row is longer than
    a proximity query can list and some row is empty, bounded scenes cull; both displacement families give impacts at t = 0 and in (0, 1]
    and not for every pair, every bound above a mover is inflated, and the lengths of the motion table come from the rule the placement
    is there for.  These are conditions on the inputs: one that fails is answered by another seed, never by another condition.
  - rta.overlap_gaps and rta.pair_impacts are the metric of every GPU comparison, and were written together with the kernels.  Here they
    are held to the geometry itself in float64 (f32 scenes) or np.longdouble (f64 scenes) from the placed REAL inputs, within the bounds
    the unit-scale tests derive on paper, and rta.overlap_gaps bit for bit to include/rtrace_hip.h's statement written out a second time.
  - The time of impact has no dimension: scaling a scene and its displacements by an exact power of two may not change a bit of it.
  - The share of grazing entries that check_brute of both GPU suites tolerates is asserted here, so that the GPU test cannot hide behind it,
    and the walk over the refit twin is brute force away from the grazes already on the CPU."""
import numpy as np
import pytest

import rust_tracer_amd as rta
from tests import scaled_scenes as ss
from tests.test_gpu_impacts import FAMILIES, TINY, Walker as ImpactWalker, brute_force as impact_brute_force, displacements, extent, lengths
from tests.test_gpu_overlap import Walker as OverlapWalker
from tests.test_gpu_query import REAL, bits
from tests.test_scales_contact_host import DENORMAL_SQUARES, higher

CASES = pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)
# refit_tiny is 2^-80 in f32: a length below 2^-40 = 9.1e-13 comes from the L1 rule.  At 1e-20 every length does; at 1e-10 the median radius
# is 5e-12, so the "slow" lengths below 0.18 of it do, whatever the seed, and the "fast" ones (factors of the extent, 3e-10) do not
L1_LENGTHS = {(rta.RT_F32, "x1e-20", "slow"): "all", (rta.RT_F32, "x1e-20", "fast"): "all", (rta.RT_F32, "x1e-10", "slow"): "some"}


def unit_of(c):
    """The length that 1 stands for at Case c's placement: its scale (1 under a translation, to rounding)."""
    return extent(c.scene.items) / extent(np.asarray(c.items0, dtype=np.float64).reshape(-1, 4))


# ---- the statement of include/rtrace_hip.h, a second time ----

def stated_overlap_gaps(queries, spheres):
    """The gap as include/rtrace_hip.h states it, sphere by sphere, every operation rounded once in the arrays' dtype -> REAL[n, m]."""
    R = queries.dtype.type
    px, py, pz, q = (np.ascontiguousarray(queries[:, a]) for a in range(4))
    out = np.full((len(queries), len(spheres)), np.inf, R)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j, (cx, cy, cz, r) in enumerate(spheres):
            rr = r * r
            if not rr > 0:
                continue
            vx, vy, vz = cx - px, cy - py, cz - pz
            vv = (vx * vx + vy * vy) + vz * vz
            out[:, j] = (np.sqrt(vv) - np.sqrt(rr)) - q
    assert out.dtype == R
    return out


def overlap_brute_force(s, queries, margin, unit):
    """tests/test_gpu_overlap.py's brute_force with the length that 1 stands for: (gap[n, m], listed, grazing).  An entry may be left out only
    if its gap lies within 1e-5 max(unit, |gap|) (f64: 1e-12) of the margin; unit = 1 is that function exactly."""
    R = REAL[s.precision]
    gap = rta.overlap_gaps(queries, s.items)
    m = R(margin)
    listed = ~(gap >= m)
    eps = 1e-5 if R == np.float32 else 1e-12
    g = gap.astype(np.float64)
    with np.errstate(invalid="ignore"):
        grazing = np.abs(g - float(m)) <= eps * np.maximum(unit, np.abs(g))
    return gap, listed, grazing


# ---- conditions on the inputs ----

def test_every_case_has_its_queries_displacements_and_twin_once():
    for precision, placement in (ss.cases_of()[0], ss.cases_of()[-1]):
        R = REAL[precision]
        for c in ss.case(precision, placement):
            q = ss.overlap_queries(c)
            assert q is ss.overlap_queries(c) and q.shape == (80, 4) and q.dtype == R and not q.flags.writeable
            assert (q[::10, 3] == 0).all() and (q[:, 3] >= 0).all() and (np.delete(q[:, 3], np.arange(0, 80, 10)) > 0).all()
            n = len(c.scene.items)
            for family in FAMILIES:
                d = ss.displacements(c, family)
                assert d is ss.displacements(c, family) and d.shape == (n, 3) and d.dtype == R and not d.flags.writeable
                np.testing.assert_array_equal(d, displacements(c.scene.items, 900 + [b[0] for b in ss.base_scenes()].index(c.name), family, R))
            t = ss.refit_twin(c)
            assert t is ss.refit_twin(c) and t.bounds is not None and len(t.items) == n and t.precision == precision
            np.testing.assert_array_equal(bits(t.items.astype(R), R), bits(c.scene.items.astype(R), R))
    assert ss.POW2 == (-66, -40, -33, 33, 45)
    items, disp = ss.pow2_scaled(np.array([[1.5, -2, 3, 0.25]], np.float32), np.array([[0.5, 0, -1]], np.float32), -33, np.float32)
    assert items.dtype == disp.dtype == np.float32 and items[0, 3] == np.ldexp(0.25, -33) and disp[0, 2] == -np.ldexp(1.0, -33)


@CASES
def test_the_queries_of_a_placed_scene_list_some_entries_and_not_all(param):
    precision, placement = param
    K = rta.RT_NEAR_MAX_K
    for c in ss.case(precision, placement):
        what = (ss.case_id(param), c.name)
        queries = ss.overlap_queries(c)
        w = OverlapWalker(c.scene, queries)
        n, m, n_nodes = len(queries), len(c.scene.items), len(w.bound)
        counts, longest, empty = [], [], []
        for margin in ss.margins(c)[:4]:
            items, gaps, offsets, st = w.all(margin)
            rows = np.diff(offsets.astype(np.int64))
            counts.append(len(items))
            longest.append(int(rows.max()))
            empty.append(int((rows == 0).sum()))
            assert 0 < len(items) < n * m, (what, margin, len(items))
            if c.scene.bounds is not None:
                assert st["tests_executed"] < n * n_nodes and st["sphere_tests"] < n * m, (what, margin, st)       # culls happen
            else:
                assert st["tests_executed"] == st["sphere_tests"] == n * m == n * n_nodes, (what, margin, st)
        print("%s %s: %s entries of %d, longest rows %s, empty rows %s" % (what + (" / ".join(map(str, counts)), n * m, longest, empty)))
        assert max(longest) > K, (what, longest)                                    # a row no proximity query can list
        assert max(empty) > 0, (what, empty)
        assert counts[2] < counts[0] < counts[1] < counts[3], (what, counts)        # more overlap asked for: fewer entries; a wider skin: more


@CASES
def test_the_displacements_of_a_placed_scene_give_impacts_culls_and_inflated_bounds(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        w = ImpactWalker(c.scene)
        n, n_nodes = len(c.scene.items), len(w.bound)
        every = n * (n - 1) // 2
        uncut = sum(n_nodes - 1 - w.node_of[t] for t in range(n))
        for family in FAMILIES:
            what = (ss.case_id(param), c.name, family)
            disp = ss.displacements(c, family)
            pairs, times, offsets, st = w.all(disp)
            at_start, during = int((times == 0).sum()), int(((times > 0) & (times <= 1)).sum())
            assert 0 < len(pairs) < every, (what, len(pairs))
            assert at_start > 0 and during > 0 and at_start + during == len(pairs), (what, at_start, during)
            if c.scene.bounds is not None:
                assert st["tests_executed"] < uncut and st["sphere_tests"] < every, (what, st)
            else:
                assert st["tests_executed"] == st["sphere_tests"] == every == uncut, (what, st)
            # every bound above a mover is inflated
            e, E = w.motion(disp)
            m = lengths(disp, w.live, R)
            above = 0
            for k in range(n_nodes):
                if w.bound[k] and any(not w.bound[x] and m[w.item[x]] > 0 for x in range(k + 1, w.skip[k])):
                    above += 1
                    assert E[k] > 0, (what, k)
            assert above > 0 or c.scene.bounds is None, what
            # the rule the lengths come from
            d = np.asarray(disp, R)
            with np.errstate(under="ignore", over="ignore"):
                s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            moving = m > 0
            by_l1 = int((moving & ~(s >= R(TINY[R]))).sum())
            print("%s %s %s: %d impacts of %d pairs (%d at the start), %d tests of %d, %d of %d lengths by the L1 rule"
                  % (what + (len(pairs), every, at_start, st["tests_executed"], uncut, by_l1, int(moving.sum()))))
            assert moving.any() and np.isfinite(m).all(), what
            rule = L1_LENGTHS.get(param + (family,), "none")
            assert {"all": by_l1 == moving.sum(), "some": 0 < by_l1 < moving.sum(), "none": by_l1 == 0}[rule], (what, rule, by_l1)


# ---- the metrics against the geometry, in higher precision ----

@CASES
def test_overlap_gaps_is_the_surface_distance_of_query_and_sphere(param):
    """Every (query, item) of the two base scenes: |overlap_gaps - (|c - p| - r - q)| <= 8 u (|c - p| + r + q), the reference in higher
    precision from the placed REAL inputs -- tests/test_scales_contact_host.py's bound for pair_gaps with q given and exact in place of the
    second root.  f32 at 1e-20 is that test's exception: rr and vv are denormals, so no value is asserted there, only that every gap is a
    number with the sign of the reference wherever the reference is more than a quarter of |c - p| + r + q.  And bit for bit
    include/rtrace_hip.h's statement written out a second time."""
    precision, placement = param
    R = REAL[precision]
    H, u = higher(precision)
    for c in ss.case(precision, placement)[:2]:
        what = (ss.case_id(param), c.name)
        items, queries = c.scene.items, ss.overlap_queries(c)
        got = rta.overlap_gaps(queries, items)
        np.testing.assert_array_equal(bits(got, R), bits(stated_overlap_gaps(queries, items), R), err_msg=str(what))
        gap = got.astype(H)
        it, qs = items.astype(H), queries.astype(H)
        v = it[None, :, :3] - qs[:, None, :3]
        dist = np.sqrt((v * v).sum(axis=2))
        ref = dist - it[None, :, 3] - qs[:, None, 3]
        reach = dist + it[None, :, 3] + qs[:, None, 3]
        bound = H(8.0) * H(u) * reach
        assert np.isfinite(gap).all() and (ref < 0).any() and (ref > 0).any(), what
        worst = float(np.max(np.abs(gap - ref) / bound))
        print("%s %s: %d gaps, %d overlap; the worst error is %.3f of its bound" % (what + (gap.size, int((ref < 0).sum()), worst)))
        if param != DENORMAL_SQUARES:
            assert (np.abs(gap - ref) <= bound).all(), (what, worst)
        else:
            far = np.abs(ref) > 0.25 * reach
            assert far.any() and (np.sign(gap[far]) == np.sign(ref[far])).all(), what


def judge_impacts(t, items, disp, i, j, H, u):
    """The decisions, the bound and the unjudged share of tests/test_impacts_host.py
    test_pair_impacts_is_the_time_two_moving_spheres_first_touch (its docstring derives them), for the times t of the pairs (i, j) ->
    (classes dict, T, tol, judged)."""
    it, dd = items.astype(H), disp.astype(H)
    v, w = it[j, :3] - it[i, :3], dd[i] - dd[j]
    rad = it[j, 3] + it[i, 3]
    A, B, VV = (w * w).sum(axis=1), (v * w).sum(axis=1), (v * v).sum(axis=1)
    K = VV + rad * rad
    Cc = VV - rad * rad
    D = B * B - A * Cc
    S = np.sqrt(np.abs(D))
    vw = np.sqrt(VV * A)
    with np.errstate(divide="ignore", invalid="ignore"):
        T = Cc / (B + S)
        tol = H(2.0) * u * ((H(9.0) * K + T * (H(6.0) * vw + H(16.0) * A * K / S + S + (B + S))) / (B + S) + T)
    k = H(1024.0) * u
    dead = (it[i, 3] == 0) | (it[j, 3] == 0)
    start = ~dead & (Cc <= -k * K)
    apart = ~dead & (Cc >= k * K)
    away = apart & ((A == 0) | (B <= -k * vw))
    toward = apart & (A > 0) & (B >= k * vw)
    by = toward & (D <= -k * A * K)
    front = toward & (D >= k * A * K)
    judged = dead | start | away | by | front
    assert (dead.astype(int) + start + away + by + front <= 1).all()
    return {"dead": dead, "start": start, "away": away, "by": by, "front": front}, T, tol, judged


@CASES
def test_pair_impacts_is_the_time_two_placed_moving_spheres_first_touch(param):
    """Every pair i < j of the two base scenes at every placement, under both displacement families, against the geometry in higher
    precision from the placed REAL inputs: the decisions, the bound and the 1 % cap on unjudged pairs are those of
    tests/test_impacts_host.py test_pair_impacts_is_the_time_two_moving_spheres_first_touch, restated in judge_impacts line for line (that
    test keeps them inside its body, so they cannot be imported).

    f32 at 1e-20 is held like every other placement: the radius is the record's r, not the root of the stream's rr (a denormal there, whose
    root is within 1.4 % of r), and S keeps the fourth-degree terms normal.  The worst error is 0.116 of the bound in f32 (5e13) and
    0.087 in f64.  With the parent's arithmetic f32 fails at 1e-20, 1e-10 and 5e13: b*b and a*c underflow to 0 or overflow there."""
    precision, placement = param
    R = REAL[precision]
    H, u = higher(precision)
    u = H(u)
    for c in ss.case(precision, placement)[:2]:
        items = c.scene.items.astype(R)
        items[7, 3] = 0                                                          # one dead slot
        n = len(items)
        i, j = np.triu_indices(n, 1)
        for family in FAMILIES:
            what = (ss.case_id(param), c.name, family)
            disp = ss.displacements(c, family)
            t = rta.pair_impacts(items, disp, i, j).astype(H)
            cls, T, tol, judged = judge_impacts(t, items, disp, i, j, H, u)
            dead, start, away, by, front = (cls[k] for k in ("dead", "start", "away", "by", "front"))
            with np.errstate(invalid="ignore"):
                worst = float(np.max(np.abs(t[front] - T[front]) / tol[front]))
            true = ~dead & (start | (front & (T <= 1)))
            listed = t <= 1
            print("%s %s %s: %d dead, %d in contact at the start, %d not approaching, %d passing by, %d in front of %d pairs, %.2f %% unjudged; "
                  "the worst error is %.3f of its bound; %d clear impacts, %d listed, %d of the clear ones missed, %d listed against a clear decision"
                  % (what + (dead.sum(), start.sum(), away.sum(), by.sum(), front.sum(), judged.size, 100.0 * (1.0 - judged.mean()), worst,
                             true.sum(), listed.sum(), (true & ~listed).sum(), (listed & judged & ~true).sum())))
            assert 1.0 - judged.mean() <= 0.01, what
            assert dead.any() and start.any() and away.any() and by.any() and front.any(), what
            for sel in (dead, away, by):
                assert np.isinf(t[sel]).all() and (t[sel] > 0).all(), what
            assert (t[start] == 0).all(), what
            assert np.isfinite(t[front]).all() and (t[front] > 0).all(), what
            assert (np.abs(t[front] - T[front]) <= tol[front]).all(), (what, worst)
            sure = front & (np.abs(T - 1) > tol)
            assert ((t[sure] <= 1) == (T[sure] <= 1)).all() and (t[sure] <= 1).any() and (t[sure] > 1).any(), what


# ---- the time of impact has no dimension ----

POW2_CASES = [(p, k) for p in (rta.RT_F32, rta.RT_F64) for k in ss.POW2]


@pytest.mark.parametrize("precision,k", POW2_CASES, ids=["%s-2^%d" % ("f32" if p == rta.RT_F32 else "f64", k) for p, k in POW2_CASES])
def test_a_power_of_two_scaling_changes_no_bit_of_a_time_of_impact(precision, k):
    """pair_impacts(items 2^k, disp 2^k) has the bits of k = 0 for every pair i < j of the four base scenes under both families.

    With the parent's arithmetic every factor fails in f32: the bits of 72 (2^-33) to 1696 (2^-66) of nested's 3160 pairs differ, and at
    2^33 15 of its 29 fast impacts are decided differently.  2^-66 is there for the radius: r * r is a denormal, and its root is not r 2^-66."""
    R = REAL[precision]
    U = np.uint32 if R == np.float32 else np.uint64
    for index, (name, items0, _, _) in enumerate(ss.base_scenes()):
        items0 = np.ascontiguousarray(np.asarray(items0, dtype=np.float64).reshape(-1, 4).astype(R))
        i, j = np.triu_indices(len(items0), 1)
        for family in FAMILIES:
            disp0 = displacements(items0, 900 + index, family, R)
            ref = rta.pair_impacts(items0, disp0, i, j)
            assert (ref == 0).any() and ((ref > 0) & (ref <= 1)).any() and (ref > 1).any() and np.isinf(ref).any(), (name, family)
            items, disp = ss.pow2_scaled(items0, disp0, k, R)
            assert np.isfinite(items).all() and (items[:, 3] > 0).all() and (np.ldexp(items, -k) == items0).all() and (np.ldexp(disp, -k) == disp0).all()
            got = rta.pair_impacts(items, disp, i, j)
            differ = int((got.view(U) != ref.view(U)).sum())
            decided = int(((got <= 1) != (ref <= 1)).sum())
            print("%s %s 2^%d: the bits of %d of %d pairs differ, %d impacts of %d are decided differently" % (name, family, k, differ, len(i), decided, int((ref <= 1).sum())))
            np.testing.assert_array_equal(got.view(U), ref.view(U), err_msg=str((name, family, k)))


# ---- the refit twins: what check_brute of both GPU suites may leave out, and that the walk is brute force elsewhere ----

@CASES
def test_the_grazing_share_stays_under_the_cap_and_the_refit_walk_is_brute_force(param):
    """check_brute of tests/test_gpu_overlap.py and of tests/test_gpu_impacts.py compares the walk with brute force away from grazing
    entries and lets at most 5 % of the listed entries graze.  Here that cap holds for every refit twin, margin and family -- for the
    overlap lists with the grazing band 1e-5 max(unit, |gap|), unit the length that 1 stands for at the placement (the band of
    test_gpu_overlap.py is written for unit scale: at 1e-20 its 1e-5 max(1, |gap|) would call every entry grazing, at 1e6 it would be a
    fraction of one rounding) -- and the walkers, which the GPU must restate bit for bit, already agree with brute force there."""
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement)[:2]:
        s = ss.refit_twin(c)
        n = len(s.items)
        unit = unit_of(c)
        queries = ss.overlap_queries(c)
        ow = OverlapWalker(s, queries)
        for margin in ss.margins(c)[:4]:
            what = (ss.case_id(param), c.name, margin)
            gap, listed, grazing = overlap_brute_force(s, queries, margin, unit)
            share = (listed & grazing).sum() / max(listed.sum(), 1)
            assert listed.any() and share <= 0.05, (what, share)
            items, gaps, offsets, st = ow.all(margin)
            rows = np.repeat(np.arange(len(queries)), np.diff(offsets.astype(np.int64)))
            keep = ~grazing[rows, items]
            gi, gj = np.nonzero(listed & ~grazing)
            np.testing.assert_array_equal((rows * n + items)[keep], gi * n + gj, err_msg=str(what))
        iw = ImpactWalker(s)
        for family in FAMILIES:
            what = (ss.case_id(param), c.name, family)
            disp = ss.displacements(c, family)
            i, j, t, grazing = impact_brute_force(s.items, disp, R)
            impact = t <= 1
            share = (impact & grazing).sum() / max(impact.sum(), 1)
            assert impact.any() and share <= 0.05, (what, share)
            pairs, times, offsets, st = iw.all(disp)
            graze_key = set((i[grazing] * n + j[grazing]).tolist())
            got_key = pairs[:, 0].astype(np.int64) * n + pairs[:, 1]
            keep = np.array([key not in graze_key for key in got_key.tolist()], bool)
            ref = impact & ~grazing
            np.testing.assert_array_equal(got_key[keep], i[ref] * n + j[ref], err_msg=str(what))
            np.testing.assert_array_equal(bits(times[keep], R), bits(t[ref], R), err_msg=str(what))
