"""The inputs of tests/test_gpu_scales.py, checked without a GPU: at every placement of tests/scaled_scenes.py the rays still hit and miss,
the bounds still cull, rays still collect several hits, and the proximity queries still meet negative gaps and empty slots -- with the
oracle, numpy and the tests' own restatements alone, so that no GPU comparison can pass on a scene that rounding has emptied.  These are
conditions on the inputs: one that fails is answered by other inputs (a seed, a translation's pre-scale), never by another condition."""
import numpy as np
import pytest

import rust_tracer_amd as rta
from tests import scaled_scenes as ss
from tests.test_gpu_camera import AMBIENT, LIT, MISS, SHADOWED, restate_rays
from tests.test_gpu_multihit import Walker as HitWalker
from tests.test_gpu_near import Walker as NearWalker
from tests.test_gpu_query import REAL

CASES = pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)


def test_the_placements_are_the_ones_the_frame_tests_use_and_the_translations():
    assert ss.placement_ids(rta.RT_F32) == ["x1e-20", "x1e-10", "x1e+06", "x5e+13", "+3e3"]
    assert ss.placement_ids(rta.RT_F64) == ["x1e-20", "x1e-10", "x1e+06", "x5e+13", "+3e9", "x1e3+9e14"]
    assert [b[0] for b in ss.base_scenes()] == ["nested", "concentric", "nested_flat", "concentric_flat"]
    items, bounds, eye = dict(ss.placements(rta.RT_F32))["+3e3"](np.array([[1.0, 2.0, 3.0, 0.5]]), None, (0.0, 0.0, -1.0))
    assert items.tolist() == [[3001.0, -4998.0, 7003.0, 0.5]] and bounds is None and eye == (3000.0, -5000.0, 6999.0)
    items, _, _ = dict(ss.placements(rta.RT_F64))["x1e3+9e14"](np.array([[1.0, 2.0, 3.0, 0.5]]), None, (0.0, 0.0, 0.0))
    assert items.tolist() == [[1000.0, 2000.0, 9e14 + 3000.0, 500.0]]
    # every placed value is a value of the scene's REAL
    for precision in (rta.RT_F32, rta.RT_F64):
        R = REAL[precision]
        for _, f in ss.placements(precision):
            for _, it, bd, _ in ss.base_scenes():
                a, b, e = f(it, bd, ss.EYE)
                assert np.array_equal(a, a.astype(R).astype(np.float64)) and (b is None or np.array_equal(b, b.astype(R).astype(np.float64)))
                assert np.abs(a).max() <= 1e15 and np.isfinite(a).all() and max(abs(v) for v in e) <= 1e15


@CASES
def test_a_placed_scene_keeps_its_spheres_apart_and_their_radii_positive(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        placed = c.scene.items
        assert placed.dtype == R and (placed[:, 3] > 0).all() and np.isfinite(placed).all(), c.name
        assert c.scene.bounds is None or (c.scene.bounds[:, 3] > 0).all(), c.name
        # no two distinct items have become bit-identical (the base scenes hold no duplicates: asserted, not assumed)
        assert len(np.unique(c.items0, axis=0)) == len(c.items0), c.name
        assert len(np.unique(placed, axis=0)) == len(placed), (c.name, placement)
        # ... and every radius squared, the value the streams hold, is still positive in REAL
        assert (placed[:, 3] * placed[:, 3] > 0).all(), c.name


def test_at_1e_minus_20_every_f32_square_is_a_denormal_whose_root_is_not_the_radius():
    # what the placement is for: rr, vv and the discriminants lie below 2^-126, far below the 2^-96 under which the lean f32 root takes its
    # general path; and a stream's rr = RN(r * r) keeps so few bits there that its root is no longer r -- a gap or a distance formed
    # from r itself, or from a square rounded any other way, has other bits
    f = np.float32
    for c in ss.case(rta.RT_F32, "x1e-20"):
        r = c.scene.items[:, 3]
        rr = r * r
        assert (rr > 0).all() and (rr < np.ldexp(f(1), -126)).all(), c.name
        assert (np.sqrt(rr) != r).mean() > 0.5, c.name
        v = c.scene.items[None, :, :3] - c.points[:, None, :]
        vv = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        assert (vv < np.ldexp(f(1), -126)).all() and (vv > 0).any(), c.name
        gaps = rta.sphere_gaps(c.points, c.scene.items)
        with_r = np.sqrt(vv) - r[None, :]
        assert (gaps != with_r).any(), c.name
    for c in ss.case(rta.RT_F32, "x1e-10"):                          # ... while at 1e-10 the squares are normal and the lean sequence runs
        rr = c.scene.items[:, 3] * c.scene.items[:, 3]
        assert (rr >= np.ldexp(f(1), -96)).all(), c.name


@CASES
def test_the_rays_of_a_placed_scene_hit_miss_and_are_culled(param):
    precision, placement = param
    n_each = ss.N_EACH_RAYS
    for c in ss.case(precision, placement):
        assert len(c.rays) == 7 * n_each == 84
        dist, _ = ss.oracle_nearest(c)
        hit = dist < c.tmax.astype(np.float64)
        aimed = np.concatenate([np.arange(f * n_each, (f + 1) * n_each) for f in ss.AIMED_FAMILIES])
        reach, _ = ss.oracle_nearest(c, c.rays[aimed], np.full(len(aimed), np.inf))
        share, share_tmax = float(np.isfinite(reach).mean()), float(hit[aimed].mean())
        print("%s %s %s: %.0f %% of the %d aimed rays hit (%.0f %% below their own tmax); %d of all %d rays hit"
              % (ss.case_id(param), c.name, "flat" if c.scene.bounds is None else "walk", 100 * share, len(aimed), 100 * share_tmax,
                 int(hit.sum()), len(hit)))
        assert share >= 0.25 and share_tmax >= 0.25, (c.name, share, share_tmax)
        assert hit.any() and not hit.all(), c.name
        assert (~np.isfinite(ss.oracle_nearest(c, c.rays, np.full(len(c.rays), np.inf))[0])).any(), c.name      # a ray that misses everything
        # the nearest walk restated test by test over the node stream (every test the oracle's): k = 1 CLOSEST of the multi-hit walk
        w = HitWalker(c.scene)
        caches = [dict() for _ in c.rays]
        walk = [w.walk(r, t, 1, False, cache) for r, t, cache in zip(c.rays, c.tmax, caches)]
        np.testing.assert_array_equal(np.array([x[0][0] for x in walk]), dist, err_msg=c.name)       # it is the oracle's own walk
        tests = sum(x[3] + x[4] for x in walk)
        if c.scene.bounds is not None:
            assert tests < len(c.rays) * len(w.nodes), (c.name, tests)                               # culls happen
        else:
            assert tests == len(c.rays) * len(w.nodes)
        # several hits on one ray
        many = [w.walk(r, t, 4, True, cache) for r, t, cache in zip(c.rays, c.tmax, caches)]
        assert max(x[2] for x in many) >= 2, c.name


@CASES
def test_the_queries_of_a_placed_scene_meet_negative_gaps_and_empty_slots(param):
    precision, placement = param
    for c in ss.case(precision, placement):
        assert len(c.points) == 4 * ss.N_EACH_POINTS == 80
        w = NearWalker(c.scene, c.points)
        for all_within in (False, True):
            ref = w.all(c.radius, 5, all_within)
            gaps, items = np.array([x[0] for x in ref]), np.array([x[1] for x in ref])
            assert ((items >= 0) & (gaps < 0)).any(axis=1).any(), (c.name, all_within)               # a query inside a sphere
            finite = np.isfinite(c.radius)
            assert ((items < 0).any(axis=1) & finite).any(), (c.name, all_within)                    # an empty slot under a finite radius
            assert ((items >= 0).any(axis=1) & finite).any(), (c.name, all_within)                   # ... and a filled one


@CASES
def test_the_traced_rays_of_a_placed_scene_take_every_exit(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement):
        state, gdot = restate_rays(c.oracle, c.mode, c.rays, c.scene.directional_light.astype(R), R)
        assert set(np.unique(state)) == {MISS, AMBIENT, LIT, SHADOWED}, (c.name, np.bincount(state, minlength=4))
        assert (gdot[(state == LIT) | (state == SHADOWED)] < 0).all()


@CASES
def test_the_sphere_keys_of_a_placed_scene_tell_its_spheres_apart(param):
    precision, placement = param
    R = REAL[precision]
    for c in ss.case(precision, placement)[:2]:
        sh = ss.shuffled(c.items, R)
        keys = rta.sphere_keys(sh)
        assert len(np.unique(keys)) > len(sh) // 2 and keys.max() >= 1 << 27, c.name              # ext >= 2^(e - 1): the longest axis reaches cell 512, bit 9
        order = np.argsort(keys, kind="stable")
        assert not np.array_equal(order, np.arange(len(sh)))
        # the refit bounds of the sorted spheres enclose them: the root's reach covers every sphere
        rg = rta.balanced_ranges(len(sh), 4)
        bd = rta.refit_bounds(sh[order], rg, precision).astype(np.float64)
        it = sh[order].astype(np.float64)
        assert (np.linalg.norm(it[:, :3] - bd[0, :3], axis=1) + it[:, 3] <= bd[0, 3]).all() and (bd[:, 3] > 0).all(), c.name


def test_the_sort_inputs_hold_their_duplicates_at_both_placements():
    for precision in (rta.RT_F32, rta.RT_F64):
        R = REAL[precision]
        s = ss.sort_inputs(precision)
        assert s.shape == (300001, 4) and s.dtype == R and len(s) > 1024 * 256
        for sp in (s, (s.astype(np.float64) * 5e13).astype(R)):
            assert len(sp) - len(np.unique(sp[:, :3], axis=0)) >= 1000 and np.abs(sp).max() <= 1e15 and (sp[:, 3] > 0).all()
            keys = rta.sphere_keys(sp)
            assert len(np.unique(keys[1024 * 256:])) > 10000                                      # the strided spheres have keys of their own
