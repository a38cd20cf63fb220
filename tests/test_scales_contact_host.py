"""The inputs and the yardsticks of tests/test_gpu_scales_contact.py, checked without a GPU: the sphere casts and the contact margins that
tests/scaled_scenes.py gives every placed scene (the frame tests' scales 1e-20, 1e-10, 1e6 and 5e13, and the translations under which
c - o and c_j - c_i cancel).
  - Conditions on the inputs, with the tests' own walkers (pure numpy): casts still find contacts and miss, start in contact, are stopped
    by their cutoffs and are culled; every margin lists some pairs and not all.  These are conditions on the inputs: one that fails is
    answered by another seed, never by another condition.
  - rta.sweep_distances and rta.pair_gaps are the metric of every GPU comparison of the casts and the contacts, and were written together
    with the kernels.  Here they are held to the geometry itself -- the distance at which a ray meets a sphere of radius r + q, the surface
    distance of two spheres -- evaluated from the placed REAL inputs in float64 (f32 scenes) or np.longdouble (f64 scenes), within bounds
    derived on paper (below), and bit for bit to include/rtrace_hip.h's statement of the two metrics written out a second time here
    (stated_distances, stated_gaps), through the walkers of the scenes without bounds, which must be brute force exactly."""
import numpy as np
import pytest

import rust_tracer_amd as rta
from tests import scaled_scenes as ss
from tests.test_gpu_contacts import Walker as PairWalker
from tests.test_gpu_multihit import node_stream
from tests.test_gpu_query import REAL, bits
from tests.test_gpu_sweep import RADII, Walker as CastWalker

CASES = pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)
N_EACH = ss.N_EACH_CASTS
DENORMAL_SQUARES = (rta.RT_F32, "x1e-20")            # the one placement whose squares are denormals: absolute errors of 2^-149


# ---- the statement of include/rtrace_hip.h, a second time ----

def stated_distances(rays, q, spheres, rad=None):
    """The cast distance as include/rtrace_hip.h states it, sphere by sphere, every operation rounded once in the arrays' dtype -> REAL[n, m].
    rad: the value used for sqrt(rr), per sphere (None: sqrt(rr) itself)."""
    R = rays.dtype.type
    ox, oy, oz, dx, dy, dz = (np.ascontiguousarray(rays[:, a]) for a in range(6))
    out = np.full((len(rays), len(spheres)), np.inf, R)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j, (cx, cy, cz, r) in enumerate(spheres):
            rr = r * r
            if not rr > 0:
                continue
            root = np.sqrt(rr) if rad is None else rad[j]
            RR = (rr + (q + q) * root) + q * q
            vx, vy, vz = cx - ox, cy - oy, cz - oz
            b = (vx * dx + vy * dy) + vz * dz
            vv = (vx * vx + vy * vy) + vz * vz
            disc = (b * b - vv) + RR
            s = np.sqrt(np.where(disc < 0, R(0.0), disc))
            t1 = b - s
            out[:, j] = np.where((disc < 0) | (b + s < 0), R(np.inf), np.where(t1 > 0, t1, R(0.0)))
    assert out.dtype == R
    return out


def stated_gaps(spheres):
    """(i, j, gap) over all i < j as include/rtrace_hip.h states the gap of a pair, the lower slot as the query."""
    R = spheres.dtype.type
    i, j = np.triu_indices(len(spheres), 1)
    rr = spheres[:, 3] * spheres[:, 3]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        vx, vy, vz = (spheres[j, a] - spheres[i, a] for a in range(3))
        vv = (vx * vx + vy * vy) + vz * vz
        gap = (np.sqrt(vv) - np.sqrt(rr)[j]) - np.sqrt(rr)[i]
    gap = np.where((rr[i] > 0) & (rr[j] > 0), gap, R(np.inf))
    assert gap.dtype == R
    return i, j, gap


# ---- conditions on the inputs ----

def test_every_case_has_its_casts_and_margins_once():
    for precision, placement in (ss.cases_of()[0], ss.cases_of()[-1]):
        R = REAL[precision]
        for c in ss.case(precision, placement):
            rays, radius, which, tmax = ss.casts(c)
            assert all(a is b for a, b in zip(ss.casts(c), (rays, radius, which, tmax)))             # made once
            assert rays.shape == (4 * N_EACH, 6) and rays.dtype == R and radius.dtype == R and tmax.dtype == R and len(rays) == 80
            assert not rays.flags.writeable and not tmax.flags.writeable                             # ... and left unchanged
            for r in range(5):
                assert (which == r).sum() == 16
            assert (radius[which == 0] == 0).all() and (radius[which != 0] > 0).all()
            assert np.isinf(tmax).any() and np.isfinite(tmax).any() and (tmax > 0).all()
            m = ss.margins(c)
            r = float(np.median(c.scene.items[:, 3]))
            assert m == (0.0, r, -0.25 * r, 4.0 * r, np.inf, -np.inf) and r > 0 and R(m[2]) < 0


@CASES
def test_the_casts_of_a_placed_scene_touch_miss_start_in_contact_and_are_culled(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        what = (ss.case_id(param), c.name)
        rays, radius, which, tmax = ss.casts(c)
        n = len(rays)
        w = CastWalker(c.scene, rays, radius)
        n_nodes = len(w.bound)
        free = np.full(n, np.inf, R)
        for any_hit in (False, True):
            ref = w.all(tmax, any_hit)
            dist, item = np.array([x[0] for x in ref]), np.array([x[1] for x in ref])
            tests = sum(x[2] + x[3] for x in ref)
            open_item = np.array([x[1] for x in w.all(free, any_hit)])
            stopped = int(((open_item >= 0) & (item < 0)).sum())
            print("%s %s %s: %d of %d casts find a contact, %d of them at distance 0, %d are stopped by their cutoff, %d tests of %d"
                  % (what + ("ANY" if any_hit else "NEAREST", int((item >= 0).sum()), n, int(((item >= 0) & (dist == 0)).sum()), stopped, tests, n * n_nodes)))
            assert (item >= 0).any() and (item < 0).any(), what
            assert ((item >= 0) & (dist == 0)).any(), what                           # a cast that starts in contact with an item
            for r in range(5):
                assert (open_item[which == r] >= 0).any(), (what, RADII[r])         # every radius touches something
            for r in (0, 1):
                assert (open_item[which == r] < 0).any(), (what, RADII[r])          # the small ones also pass everything by
            assert stopped >= 1, what                                               # the cutoff bites
            if c.scene.bounds is not None:
                assert tests < n * n_nodes, (what, tests)                           # culls happen
            elif not any_hit:
                assert tests == n * len(c.scene.items) == n * n_nodes, (what, tests)


@CASES
def test_the_margins_of_a_placed_scene_list_some_pairs_and_not_all(param):
    precision, placement = param
    for c in ss.case(precision, placement):
        what = (ss.case_id(param), c.name)
        w = PairWalker(c.scene)
        n = len(c.scene.items)
        every = n * (n - 1) // 2
        uncut = sum(len(w.bound) - 1 - w.node_of[t] for t in range(n))             # every node behind every item: n (n - 1) / 2 plus the bounds
        assert uncut == every + sum(sum(w.bound[w.node_of[t] + 1:]) for t in range(n))
        counts = []
        for margin in ss.margins(c)[:4]:
            pairs, gaps, offsets, st = w.all(margin)
            counts.append(len(pairs))
            assert 0 < len(pairs) < every, (what, margin, len(pairs))
            if c.scene.bounds is not None:
                assert st["tests_executed"] < uncut and st["sphere_tests"] < every, (what, margin, st)
            else:
                assert st["tests_executed"] == st["sphere_tests"] == every == uncut, (what, margin, st)
        print("%s %s: %s pairs of %d" % (what + (" / ".join(str(k) for k in counts), every)))
        assert counts[2] < counts[0] < counts[1] < counts[3], (what, counts)        # more overlap asked for: fewer pairs; a wider skin: more


@CASES
def test_radius_0_from_outside_the_root_meets_the_condition_of_the_ray_query(param):
    """The condition under which a cast is the ray query (tests/test_gpu_scales_contact.py compares the two, and the ray query with the
    oracle): no record these casts test is entered at or below 0, and every record has rr > 0."""
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        rays, zeros, tmax = ss.ray_casts(c)
        assert len(rays) == 2 * N_EACH and not zeros.any()
        w = CastWalker(c.scene, rays, zeros)
        found = 0
        for any_hit in (False, True):
            found += sum(x[1] >= 0 for x in w.all(tmax, any_hit))
            found += sum(x[1] >= 0 for x in w.all(np.full(len(rays), np.inf, R), any_hit))
        assert w.lowest > 0, (ss.case_id(param), c.name, w.lowest)
        assert 0 < found < 4 * len(rays)
        rec = np.array([x[0][3] for x in node_stream(c.scene)]).astype(R)
        assert (rec * rec > 0).all(), (ss.case_id(param), c.name)


def test_at_1e_minus_20_the_f32_casts_inflate_denormals_by_denormals():
    # what the placement does to RR = (rr + (q + q) * sqrt(rr)) + q * q: all three terms are denormals, q * q keeps no bit at all for the
    # smaller radii, sqrt(rr) is not r -- so that a distance formed from r itself has other bits -- and the identity "q = 0 gives RR == rr"
    # and the start clamp act on values of a few ulp of the denormal range
    f = np.float32
    for c in ss.case(rta.RT_F32, "x1e-20"):
        rays, q, which, tmax = ss.casts(c)
        r = c.scene.items[:, 3]
        rr = r * r
        rad = np.sqrt(rr)
        RR = (rr[None, :] + (q + q)[:, None] * rad[None, :]) + (q * q)[:, None]
        assert RR.dtype == f and (RR < np.ldexp(f(1), -126)).all() and (RR > 0).all(), c.name
        # q * q of the smallest positive radius, a quarter of the median, keeps a handful of bits or none (below 2^-140: at most nine);
        # three root radii keep all of theirs, so the condition is on the casts of that radius
        qq = (q * q)[which == 1]
        assert (q[which == 1] > 0).all() and ((qq == 0).any() or (qq < np.ldexp(f(1), -140)).all()), c.name
        assert ((q * q)[which == 4] >= np.ldexp(f(1), -130)).all(), c.name     # (20 bits or more)
        assert (rad != r).mean() > 0.5, c.name
        t = rta.sweep_distances(rays, q, c.scene.items)
        with_r = stated_distances(rays, q, c.scene.items, rad=r)
        both = np.isfinite(t) & np.isfinite(with_r)
        assert both.any() and (t[both] != with_r[both]).any(), c.name
        np.testing.assert_array_equal(bits(RR[q == 0], f), bits(np.broadcast_to(rr, RR.shape)[q == 0], f))          # the identity holds there too
    for c in ss.case(rta.RT_F32, "x1e-10"):                                          # ... while at 1e-10 every RR is normal and the lean root runs
        q = ss.casts(c)[1]
        rr = c.scene.items[:, 3] * c.scene.items[:, 3]
        RR = (rr[None, :] + (q + q)[:, None] * np.sqrt(rr)[None, :]) + (q * q)[:, None]
        assert (RR >= np.ldexp(f(1), -96)).all(), c.name


# ---- the scenes without bounds: the walkers are brute force over the stated metric, exactly ----

@CASES
def test_the_flat_walks_are_brute_force_over_the_stated_metrics_bit_for_bit(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        if c.scene.bounds is not None:
            continue
        what = (ss.case_id(param), c.name)
        rays, radius, which, tmax = ss.casts(c)
        items = c.scene.items
        t = stated_distances(rays, radius, items)
        np.testing.assert_array_equal(bits(rta.sweep_distances(rays, radius, items), R), bits(t, R), err_msg=str(what))
        slot = np.argmin(t, axis=1)                                                  # the lowest slot of equal minima
        first = t[np.arange(len(t)), slot]
        hit = first < tmax
        ref = CastWalker(c.scene, rays, radius).all(tmax, False)
        np.testing.assert_array_equal(bits([x[0] for x in ref], R), bits(np.where(hit, first, tmax), R), err_msg=str(what))
        np.testing.assert_array_equal([x[1] for x in ref], np.where(hit, slot, -1), err_msg=str(what))
        assert sum(x[2] for x in ref) == len(rays) * len(items) and sum(x[3] for x in ref) == 0
        i, j, gap = stated_gaps(items)
        np.testing.assert_array_equal(bits(rta.pair_gaps(items, i, j), R), bits(gap, R), err_msg=str(what))
        w = PairWalker(c.scene)
        for margin in ss.margins(c):
            contact = ~(gap >= R(margin))
            pairs, gaps, offsets, st = w.all(margin)
            np.testing.assert_array_equal(pairs, np.stack([i[contact], j[contact]], axis=1), err_msg=str((what, margin)))
            np.testing.assert_array_equal(bits(gaps, R), bits(gap[contact], R), err_msg=str((what, margin)))
            assert int(offsets[-1]) == int(contact.sum())


# ---- the metrics against the geometry, in higher precision ----

def higher(precision):
    """(H, u): the type the reference is evaluated in, and the unit roundoff of the scene's REAL."""
    if precision == rta.RT_F32:
        return np.float64, 2.0 ** -24
    if np.finfo(np.longdouble).eps > 2e-19:
        pytest.skip("np.longdouble is no wider than float64 here (eps %g): no higher precision to hold an f64 scene to" % np.finfo(np.longdouble).eps)
    return np.longdouble, 2.0 ** -53


@CASES
def test_sweep_distances_is_the_distance_to_the_inflated_sphere(param):
    """Every (cast, item) of the two base scenes against the geometry in higher precision H, from the placed REAL inputs:
        v = c - pos, b = v.d, vv = v.v, RR = (r + q)^2, disc = b^2 - vv + RR, s = sqrt(disc), t1 = b - s, t2 = b + s
    With u the unit roundoff of REAL, tol = 16 u (|v| + (vv + RR) / s + |t1|): the rounded v and the two dot products put at most
    16 u (vv + RR) on disc, which is at most 8 u (vv + RR) / s on the root; b carries at most 4 u |v|; the last subtraction u |t1|; the
    constant is twice that sum.  A pair is judged only where the decision is clear (C = 1024 u (vv + RR)):
        disc <= -C                              +inf  (miss)
        disc >=  C, t2 < -tol                   +inf  (behind)
        disc >=  C, t1 < -tol < tol < t2        exactly 0  (start in contact)
        disc >=  C, t1 > tol                    finite, within tol of t1
    and at most 1 % of all pairs may be left unjudged.  f32 at 1e-20 is the exception: the squares are denormals, every operation on them
    has an absolute error of up to 2^-149 that no relative bound covers, so there only the four decisions are asserted, not the values."""
    precision, placement = param
    R = REAL[precision]
    H, u = higher(precision)
    u = H(u)
    for c in ss.case(precision, placement)[:2]:
        what = (ss.case_id(param), c.name)
        rays, radius, which, tmax = ss.casts(c)
        items = c.scene.items
        t = rta.sweep_distances(rays, radius, items).astype(H)
        ry, q, it = rays.astype(H), radius.astype(H), items.astype(H)
        v = it[None, :, :3] - ry[:, None, :3]
        d = ry[:, None, 3:]
        b = (v * d).sum(axis=2)
        vv = (v * v).sum(axis=2)
        reach = it[None, :, 3] + q[:, None]
        RR = reach * reach
        disc = b * b - vv + RR
        clear = H(1024.0) * u * (vv + RR)
        s = np.sqrt(np.abs(disc))
        t1, t2 = b - s, b + s
        with np.errstate(divide="ignore", invalid="ignore"):
            tol = H(16.0) * u * (np.sqrt(vv) + (vv + RR) / s + np.abs(t1))
        real = disc >= clear
        miss = disc <= -clear
        behind = real & (t2 < -tol)
        start = real & (t1 < -tol) & (tol < t2)
        front = real & (t1 > tol)
        judged = miss | behind | start | front
        assert (miss.astype(int) + behind + start + front <= 1).all()
        with np.errstate(invalid="ignore"):
            worst = float(np.max(np.abs(t[front] - t1[front]) / tol[front])) if front.any() else 0.0
        print("%s %s: %d miss, %d behind, %d start in contact, %d in front of %d pairs, %.2f %% unjudged; the worst error is %.3f of its bound"
              % (what + (int(miss.sum()), int(behind.sum()), int(start.sum()), int(front.sum()), judged.size, 100.0 * (1.0 - judged.mean()), worst)))
        assert 1.0 - judged.mean() <= 0.01, what
        assert miss.any() and behind.any() and start.any() and front.any(), what
        assert np.isinf(t[miss]).all() and (t[miss] > 0).all(), what
        assert np.isinf(t[behind]).all() and (t[behind] > 0).all(), what
        assert (t[start] == 0).all(), what
        assert np.isfinite(t[front]).all(), what
        if param != DENORMAL_SQUARES:
            assert (np.abs(t[front] - t1[front]) <= tol[front]).all(), (what, worst)


@CASES
def test_pair_gaps_is_the_surface_distance_of_two_spheres(param):
    """Every pair i < j of the two base scenes: |pair_gaps - (|c_j - c_i| - r_j - r_i)| <= 8 u (|c_j - c_i| + r_i + r_j), the reference in
    higher precision from the placed REAL inputs -- one rounded difference, a sum of three squares, three roots and two subtractions,
    doubled.  f32 at 1e-20 is the exception of the test above: rr and vv are denormals (rr holds a handful of bits), so no value is
    asserted there, only that every gap is a number with the sign of the reference wherever the reference is more than a quarter of
    |c_j - c_i| + r_i + r_j: the smallest rr there is 18 units of 2^-149, so a root of rr is within 1.4 % of r, and vv is within 1.5 units,
    so its root is within sqrt(1.5 * 2^-149) = 4.6e-23 -- a seventh of the smallest r_i + r_j -- and within 2.5 % of the sum once
    |c_j - c_i| >= 1e-22."""
    precision, placement = param
    H, u = higher(precision)
    for c in ss.case(precision, placement)[:2]:
        what = (ss.case_id(param), c.name)
        items = c.scene.items
        i, j = np.triu_indices(len(items), 1)
        gap = rta.pair_gaps(items, i, j).astype(H)
        it = items.astype(H)
        v = it[j, :3] - it[i, :3]
        dist = np.sqrt((v * v).sum(axis=1))
        ref = dist - it[j, 3] - it[i, 3]
        reach = dist + it[i, 3] + it[j, 3]
        bound = H(8.0) * H(u) * reach
        assert np.isfinite(gap).all() and (ref < 0).any() and (ref > 0).any(), what
        worst = float(np.max(np.abs(gap - ref) / bound))
        print("%s %s: %d pairs, %d overlap; the worst error is %.3f of its bound" % (what + (len(i), int((ref < 0).sum()), worst)))
        if param != DENORMAL_SQUARES:
            assert (np.abs(gap - ref) <= bound).all(), (what, worst)
        else:
            far = np.abs(ref) > 0.25 * reach
            assert far.any() and (np.sign(gap[far]) == np.sign(ref[far])).all(), what
