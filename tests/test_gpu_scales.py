"""The ray, proximity and dynamic-scene entries away from unit scale and away from the origin (tests/scaled_scenes.py: the frame tests'
scales 1e-20, 1e-10, 1e6 and 5e13, and translations under which c - o cancels), bit for bit and counter for counter against the
yardsticks the unit-scale suites already use, each of which takes a scene of any size:
  nearest / any   oracle.Scene.intersect and oracle.sphere_intersect (tests/test_gpu_query.py check_nearest); the test counters against
                  the k = 1 CLOSEST walk over the node stream, every test of which is the oracle's (tests/test_gpu_multihit.py Walker)
  multi-hit       that Walker, for k = 1, 4, 16 and both modes
  trace           render.rs restated over the oracle's intersect (tests/test_gpu_camera.py restate_rays / accumulate)
  proximity       the walk over the node stream with rta.sphere_gaps as its metric (tests/test_gpu_near.py Walker, assert_walk)
  dynamic scenes  rta.refit_bounds and rta.sphere_keys; a fresh static scene of the same values (tests/test_gpu_dynamic.py answers /
                  fresh_answers); the oracle built from the reported bounds; the stand-in of tests/test_gpu_live.py for dead slots
  the sphere sort np.argsort(rta.sphere_keys(s), kind="stable"), on 300,001 spheres: the strided iterations of k_sphere_box / k_sphere_keys
tests/test_scales_host.py holds the inputs to their conditions on the CPU (hits, misses, culls, several hits per ray, negative gaps,
empty slots), so none of this passes on a scene that rounding has emptied.  No control of csrc/rt_debug.h is used."""
import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from tests import scaled_scenes as ss
from tests.test_gpu_camera import AMBIENT, LIT, MISS, SHADOWED, accumulate, restate_rays
from tests.test_gpu_dynamic import EYE, LIGHT, animate, answers, as_bits, assert_same, fresh_answers, scene_of
from tests.test_gpu_live import stand_in_arrays
from tests.test_gpu_multihit import Walker as HitWalker, check_normals
from tests.test_gpu_near import Walker as NearWalker, assert_walk, check_dynamic
from tests.test_gpu_query import PREC, REAL, bits, check_nearest, ray_families

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)
LEAF = 4
_REFS = {}


def counters(st):
    return tuple(int(st[k]) for k in ("primary", "hits", "shadow", "occluded", "sphere_tests", "bound_tests", "tests_executed"))


def same_bytes(a, b, what):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(as_bits(x), as_bits(y), err_msg=str(what))


def release(scene):
    """Closes the device copy of a shared case's scene (check_nearest makes it as scene.device()) and forgets it: the next test uploads its own."""
    for d in scene._device.values():
        d.close()
    scene._device.clear()


def hit_walks(c):
    """(Walker, one cache of oracle tests per ray) of case c -- made once: every k and both modes share the tests."""
    key = ("hits", c.precision, c.placement, c.name)
    if key not in _REFS:
        _REFS[key] = (HitWalker(c.scene), [dict() for _ in c.rays])
    return _REFS[key]


# ---- nearest and any ----

@CASES
def test_nearest_and_any_hit_match_the_oracle_ray_for_ray(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        s, rays, tmax = c.scene, c.rays, c.tmax
        d = s.device()
        what = (ss.case_id(param), c.name)
        ref_d, item = check_nearest(s, c.oracle, rays, tmax, c.mode)                  # distance, normal and item against the oracle
        hit = item >= 0
        assert hit.any() and not hit.all(), what
        # ANY: "something closer than tmax" is the nearest query's own answer; the reported item is closer than tmax
        ad, an, ai = d.intersect(rays, tmax, any_hit=True)
        found = ai >= 0
        np.testing.assert_array_equal(found, hit, err_msg=str(what))
        np.testing.assert_array_equal(found, ad.astype(np.float64) < tmax.astype(np.float64), err_msg=str(what))
        np.testing.assert_array_equal(bits(ad[~found], R), bits(tmax[~found], R), err_msg=str(what))
        assert not an[~found].any()
        for k in np.flatnonzero(found):
            d1, n1 = oracle.sphere_intersect(s.items[ai[k]].astype(np.float64), rays[k].astype(np.float64), float("inf"), PREC[precision])
            assert R(d1) == ad[k] and d1 < tmax[k] and np.array_equal(bits(n1, R), bits(an[k], R)), (what, k)
        # the counting launch: the same bytes; the nearest walk's tests are the oracle's, node by node
        w, caches = hit_walks(c)
        walk = [w.walk(r, t, 1, False, cache) for r, t, cache in zip(rays, tmax, caches)]
        plain = d.intersect(rays, tmax)
        *counted, st = d.intersect(rays, tmax, want_stats=True)
        same_bytes(counted, plain, what)
        assert st["primary"] == len(rays) and st["hits"] == int(hit.sum()), what
        assert (st["sphere_tests"], st["bound_tests"]) == (sum(x[3] for x in walk), sum(x[4] for x in walk)), what
        assert st["tests_executed"] == st["sphere_tests"] + st["bound_tests"], what
        *any_counted, ast = d.intersect(rays, tmax, any_hit=True, want_stats=True)
        same_bytes(any_counted, (ad, an, ai), what)
        assert ast["primary"] == len(rays) and ast["hits"] == int(found.sum()), what
        # the same rays walked in the device's coherent order: the same bytes and counters
        *ordered, ost = d.intersect(rays, tmax, want_stats=True, order=True)
        same_bytes(ordered, plain, what)
        assert counters(ost) == counters(st), what
        *ordered, ost = d.intersect(rays, tmax, any_hit=True, want_stats=True, order=True)
        same_bytes(ordered, (ad, an, ai), what)
        assert counters(ost) == counters(ast), what
        release(s)


# ---- multi-hit ----

@CASES
def test_the_multi_hit_lists_restate_the_walk_bit_for_bit(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        s, rays, tmax = c.scene, c.rays, c.tmax
        d = s.device()
        w, caches = hit_walks(c)
        most = 0
        for all_hits in (False, True):
            for k in (1, 4, 16):
                dist, nrm, item, hits, st = d.intersect_multi(rays, k, tmax, all_hits=all_hits, want_stats=True)
                ref = [w.walk(r, t, k, all_hits, cache) for r, t, cache in zip(rays, tmax, caches)]
                what = str((ss.case_id(param), c.name, k, all_hits))
                np.testing.assert_array_equal(bits(dist, R), bits([x[0] for x in ref], R), err_msg=what)
                np.testing.assert_array_equal(item, [x[1] for x in ref], err_msg=what)
                np.testing.assert_array_equal(hits, [x[2] for x in ref], err_msg=what)
                assert st["sphere_tests"] == sum(x[3] for x in ref), what
                assert st["bound_tests"] == sum(x[4] for x in ref), what
                assert st["hits"] == int((hits > 0).sum()) and st["primary"] == len(rays), what
                check_normals(s, rays, dist, nrm, item)
                most = max(most, int(hits.max()))
        assert most >= 2, (ss.case_id(param), c.name)
        release(s)


# ---- trace ----

@CASES
def test_traced_rays_match_the_restated_render(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        s, rays = c.scene, c.rays
        d = s.device()
        what = str((ss.case_id(param), c.name))
        light = s.directional_light.astype(R)
        state, gdot = restate_rays(c.oracle, c.mode, rays, light, R)                 # restate_colors, and the exits for the counters
        ref_c, ref_a = np.zeros((len(rays), 3), dtype=R), np.zeros(len(rays), dtype=R)
        accumulate(ref_c, ref_a, state, gdot, R)
        color, alpha, st = d.trace(rays, want_stats=True)
        np.testing.assert_array_equal(bits(color, R), bits(ref_c, R), err_msg=what)
        np.testing.assert_array_equal(bits(alpha, R), bits(ref_a, R), err_msg=what)
        want = (len(rays), int((state != MISS).sum()), int(((state == LIT) | (state == SHADOWED)).sum()), int((state == SHADOWED).sum()))
        assert (st["primary"], st["hits"], st["shadow"], st["occluded"]) == want, (what, st, want)
        assert want[1] > 0 and want[1] < want[0] and want[2] > 0 and (state == AMBIENT).any(), (what, want)
        plain = d.trace(rays)
        same_bytes(plain, (color, alpha), what)
        oc, oa, ost = d.trace(rays, want_stats=True, order=True)
        same_bytes((oc, oa), (color, alpha), what)
        assert counters(ost) == counters(st), what
        release(s)


# ---- proximity ----

@CASES
def test_the_proximity_lists_restate_the_walk_bit_for_bit(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        s, points, radius = c.scene, c.points, c.radius
        d = s.device()
        w = NearWalker(s, points)
        for all_within in (False, True):
            for k in (1, 5, 16):
                res = d.near(points, k, radius, all_within=all_within, want_stats=True)
                assert_walk(res, w.all(radius, k, all_within), R, (ss.case_id(param), c.name, k, all_within))
                gap, item, found = res[:3]
                empty = item < 0
                np.testing.assert_array_equal(bits(gap[empty], R), bits(np.broadcast_to(radius[:, None], gap.shape)[empty], R))
                assert (gap[:, 1:] >= gap[:, :-1]).all()                             # nearest first
        # every item's centre as a query that leaves its own sphere out
        n = len(s.items)
        centres = np.ascontiguousarray(s.items[:, :3])
        me = np.arange(n, dtype=np.int32)
        rho = np.ascontiguousarray(np.resize(radius, n))
        own = NearWalker(s, centres)
        for all_within in (False, True):
            res = d.near(centres, 4, rho, all_within=all_within, exclude=me, want_stats=True)
            assert_walk(res, own.all(rho, 4, all_within, me), R, (ss.case_id(param), c.name, "exclude", all_within))
            assert not (res[1] == me[:, None]).any()
        release(s)


# ---- dynamic scenes ----

def far_dummy(root, items, light):
    """One sphere that no ray of a batch sized by `root` is meant to meet: four root radii from the root's centre towards -x.  The shadow
    rays of trace() leave hit points, which lie inside the refit root, along -light, whose x is positive: they move away from it.  The
    primary rays are checked against it one by one by the caller."""
    assert -light[0] > 0
    dummy = np.array([root[0] - 4.0 * root[3], root[1], root[2], np.min(items[:, 3])], dtype=np.float64)
    assert dummy[0] + dummy[3] < root[0] - 1.5 * root[3] and np.abs(dummy).max() <= 1e15
    return dummy


def hold(d, items, live, rg, rays, tmax, precision, what):
    """Dynamic scene d, which holds `items` with `live`, against its yardsticks: the refit rule for its bounds, a fresh static scene of the
    same values for every ray entry's bytes and counters, and the oracle for the nearest distances."""
    R = REAL[precision]
    live = np.asarray(live) != 0
    np.testing.assert_array_equal(d.live(), live.astype(np.uint8), err_msg=what)
    bd = d.bounds()
    with np.errstate(all="ignore"):
        want = rta.refit_bounds(items, rg, precision, live=None if live.all() else live)
    np.testing.assert_array_equal(as_bits(bd), as_bits(want), err_msg=what)
    it = np.ascontiguousarray(items.astype(R))
    if not live.all():
        # the stand-in of tests/test_gpu_live.py: a dummy sphere in every dead slot and for every dead group's bound, which every ray misses
        # as it misses the dead record
        light = np.asarray(rta.normalized(LIGHT, precision), dtype=np.float64)
        dummy = far_dummy(bd[0].astype(np.float64), it[live].astype(np.float64), light)
        it, bd = stand_in_arrays(it, live, rg, bd, R, dummy=dummy)
        for k, r in enumerate(rays):
            assert not oracle.sphere_distance_from_ray(it[np.flatnonzero(~live)[0]].astype(np.float64), r.astype(np.float64), PREC[precision]) < np.inf, (what, k)
    got = answers(d, rays, tmax, precision, cameras=())
    assert_same(got, fresh_answers(it, bd, rg, rays, tmax, precision, cameras=()), what)
    dead = np.flatnonzero(~live)
    dist, _, item = d.intersect(rays, tmax)
    assert not np.isin(item, dead).any(), what
    o = oracle.Scene.from_ranges(it.astype(np.float64), bd.astype(np.float64), rg, LIGHT, EYE, PREC[precision])
    ref = np.array([o.intersect(r.astype(np.float64), float(t), oracle.MODE_HIERARCHY)[0] for r, t in zip(rays, tmax)])
    np.testing.assert_array_equal(bits(dist, R), bits(ref, R), err_msg=what)
    return got


@CASES
def test_dynamic_scenes_follow_updates_rebuilds_and_kills(param):
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
        bd0 = rta.refit_bounds(it0, rg, precision)
        rays, tmax = ray_families(scene_of(it0, bd0, rg, precision), np.random.default_rng(31), ss.N_EACH_RAYS)
        d = rta.DeviceScene(scene_of(it0, bd0, rg, precision), dynamic=True)
        created = hold(d, it0, everyone, rg, rays, tmax, precision, what + "as created")
        assert any(cnt[1] for _, _, cnt in created) and any(cnt[3] for _, _, cnt in created)      # hits and occluded shadow rays among them
        moved = animate(it0, 2, R)
        assert not np.array_equal(moved, it0)
        d.update(moved)
        hold(d, moved, everyone, rg, rays, tmax, precision, what + "updated")
        sh = ss.shuffled(it0, R)
        order = d.rebuild(sh)
        np.testing.assert_array_equal(order, np.argsort(rta.sphere_keys(sh), kind="stable").astype(np.uint32), err_msg=what + "rebuild")
        assert len(np.unique(rta.sphere_keys(sh))) > n // 2                          # the keys tell the spheres apart at this placement
        cur = np.ascontiguousarray(sh[order])
        hold(d, cur, everyone, rg, rays, tmax, precision, what + "rebuilt")
        live = (np.arange(n) % 3 != 0).astype(np.uint8)
        d.update(cur, live=live)
        hold(d, cur, live, rg, rays, tmax, precision, what + "every third slot dead")
        check_dynamic(d, cur, live, rg, precision, what + "every third slot dead")
        half = n // 2
        order = d.rebuild(sh, n=half)
        np.testing.assert_array_equal(order, np.argsort(rta.sphere_keys(sh[:half]), kind="stable").astype(np.uint32), err_msg=what + "rebuild of half")
        cur = np.zeros((n, 4), dtype=R)
        cur[:half] = sh[:half][order]
        live = (np.arange(n) < half).astype(np.uint8)
        hold(d, cur, live, rg, rays, tmax, precision, what + "rebuild of half")
        assert (d.bounds()[:, 3] == 0).any()                                         # dead groups among them
        check_dynamic(d, cur, live, rg, precision, what + "rebuild of half")
        d.close()


# ---- the sphere sort beyond one pass of its grid ----

@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_the_sphere_order_of_more_spheres_than_one_grid_pass_has_threads(precision):
    import torch
    R = REAL[precision]
    d = rta.Scene.three_spheres(precision).device()                  # the scene lends its device and REAL: no scene of this size is made
    s = ss.sort_inputs(precision)
    assert len(s) == 300001 > 1024 * 256
    for name, sp in (("as is", s), ("x5e13", np.ascontiguousarray((s.astype(np.float64) * 5e13).astype(R)))):
        keys = rta.sphere_keys(sp)
        want = np.argsort(keys, kind="stable").astype(np.uint32)
        assert (np.diff(keys[want].astype(np.int64)) == 0).sum() >= 1000                          # ties for the sort to keep in order
        assert len(np.unique(keys[1024 * 256:])) > 10000                                         # the strided spheres have keys of their own
        got = d.sphere_order(sp)
        np.testing.assert_array_equal(got, want, err_msg="host entry, " + name)
        t = d.sphere_order(torch.from_numpy(sp).cuda())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), want, err_msg="device entry, " + name)
    d.close()
