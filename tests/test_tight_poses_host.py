"""The tight spheres (rust-tracer_amd/csrc/rt_tight.hpp, NOTES.md T) away from the home pose, on the host: rules (a) - (d) and the selection
rule on every f32 scene the frame tests have (tests/posed_scenes.py, tests/scaled_scenes.py, tests/edge_scenes.py), with a census that keeps
tests/test_gpu_tight_poses.py from running empty; the theorem itself -- an item's finite distance implies its bound's, and from the eye
the bound's is not larger -- asked of the reference's f32 sphere test on rays that graze the items; and rim fixtures with closed-form tight
balls, on which the same checker must find the un-inflated ball wrong.  The helpers are in tests/tight_scenes.py.  No GPU."""
import numpy as np
import pytest

import oracle
from tests import edge_scenes as es
from tests import posed_scenes as ps
from tests import tight_scenes as ts


def _rules_hold(scene, rule):
    """Rules (a) - (d) as far as the result shows them, for every bound of an rta.Scene (f32); -> (tight bounds, bounds)."""
    spheres, tight, k = ts.tight_of(scene)
    assert k["rule"] == rule, (k, int(tight.sum()), len(tight))
    for b, (first, count) in enumerate(scene.ranges):
        if not tight[b]:
            assert spheres[b].tobytes() == scene.bounds[b].tobytes(), b
            continue
        sub = scene.items[first:first + count]
        assert ts.encloses_with_inflation(spheres[b], sub, k["S"], k["eta"]), b                      # (a)
        assert ts.encloses_with_inflation(scene.bounds[b], sub, k["S"], k["eta"]), b                 # (b)
        assert ts.eye_outside(spheres[b], scene.eye) and ts.eye_outside(scene.bounds[b], scene.eye), b   # (c)
        assert spheres[b, 3] < scene.bounds[b, 3], b                                                 # (d)
    return int(tight.sum()), len(tight)


@pytest.mark.parametrize("placement", ["id", "moved", "x1e-10", "x1e+06"])
@pytest.mark.parametrize("scene", sorted(ps.SCENES))
def test_the_rules_on_every_posed_scene(scene, placement):
    mine = [k for k in ts.posed_inputs() if k[0] == scene and k[3] == placement]
    assert len(mine) >= (20 if placement in ("id", "moved") else 1)
    eyes = set()
    for key in mine:
        n_tight, n = _rules_hold(ts.posed_scene(key), ts.posed_rule(key))
        eyes.add(key[2])
        if placement == "x1e-10":
            assert n_tight == 0, key
        elif key[2] in ts.INSIDE_EYES:
            assert n_tight >= 20 and n - n_tight >= 1, (key, n_tight, n)
        else:
            assert n_tight >= 20, (key, n_tight, n)
    if placement in ("id", "moved"):
        assert eyes >= set(ps.EYES) | set(ps.SPECIAL_EYES)


@pytest.mark.parametrize("key", ts.placed_inputs(), ids="-".join)
def test_the_rules_on_every_placed_scene(key):
    n_tight, n = _rules_hold(ts.placed_case(key).scene, ts.placed_rule(key))
    assert (n_tight == 0) if key[0] in ts.PLACED_NONE else (n_tight >= 20), (key, n_tight, n)
    assert key[0] in ts.PLACED_NONE + ts.PLACED_TIGHT


@pytest.mark.parametrize("spp", es.SPPS)
@pytest.mark.parametrize("family", es.FAMILIES)
def test_the_rules_on_every_edge_scene(family, spp):
    _, s, _ = ts.edge_pair(family, spp)
    n_tight, n = _rules_hold(s, ts.EDGE_RULE.get(family, 0))
    assert (n_tight >= 1) == (family in ts.EDGE_TIGHT), (family, spp, n_tight, n)


# ---- the theorem against the reference's arithmetic -----------------------------------------------------------------------------------

THEOREM_EYES = ("home", "left", "far", "inside_root", "inside_item")
THEOREM_POSED = [(scene, "home", eye, placement) for scene in sorted(ps.SCENES) for eye in THEOREM_EYES for placement in ("id", "moved", "x1e+06")]
THEOREM_PLACED = [k for k in ts.placed_inputs() if k[0] in ("x5e+13", "+3e3")]


def _holds(tally, what):
    hit, miss = tally.shares()
    print("%s: %d rays (%d of shadow type), %.0f %% hit their item, %.0f %% miss" % (what, tally.rays, tally.unordered, 100 * hit, 100 * miss))
    assert not tally.violations, (what, len(tally.finite), len(tally.order), tally.violations[:3])
    # (conditions on the rays, not tolerances: a band in which every ray hit, or none, would ask nothing at the silhouette)
    assert tally.rays >= 1000 and tally.unordered >= 100 and hit >= 0.25 and miss >= 0.10, (what, tally.rays, tally.unordered, hit, miss)


@pytest.mark.parametrize("key", THEOREM_POSED, ids="-".join)
def test_the_theorem_holds_in_the_references_arithmetic_on_posed_scenes(key):
    _holds(ts.check_scene(ts.posed_scene(key)), "-".join(key))


@pytest.mark.parametrize("key", THEOREM_PLACED, ids="-".join)
def test_the_theorem_holds_in_the_references_arithmetic_on_placed_scenes(key):
    _holds(ts.check_scene(ts.placed_case(key).scene), "-".join(key))


def test_shadow_type_rays_start_on_other_items():
    # what shadow_rays promises, on one scene: origins on the surface of an item other than the one grazed, the scene's light as direction
    s = ts.posed_scene(("nested", "home", "home", "id"))
    items = np.asarray(s.items, dtype=np.float64)
    to_light = -np.asarray(s.directional_light, dtype=np.float64)
    n = 0
    for i in range(len(items)):
        rays = ts.shadow_rays(items, i, np.array([1.0, 0.0, 0.0]), to_light)
        for ray in rays:
            off = np.abs(np.linalg.norm(items[:, :3] - ray[:3], axis=1) - items[:, 3]) / items[:, 3]
            off[i] = np.inf
            assert off.min() < 1e-5 and np.array_equal(ray[3:], to_light)
        n += len(rays)
    assert n >= 2 * len(items)


# ---- rim fixtures ---------------------------------------------------------------------------------------------------------------------

def _rim_tallies(name):
    """(Tally of the library's and the given spheres, Tally of the un-inflated closed-form balls) over the tuned rays of one rim fixture."""
    sc, s, _ = ts.rim_pair(name)
    spheres, tight, _ = ts.tight_of(s)
    lib, plain = ts.Tally(), ts.Tally()
    for r in sc.rim:
        b, item = r["bound"], sc.items[r["item"]]
        assert tight[b], (name, b)
        ts.check_bound(lib, item, (("tight", spheres[b].astype(np.float64)), ("given", sc.bounds[b])), [r["ray"]], ordered=True)
        ts.check_bound(plain, item, (("plain", r["plain"]),), [r["ray"]], ordered=True)
    return lib, plain


@pytest.mark.parametrize("name", sorted(ts.RIM))
def test_a_rim_fixture_is_what_it_says(name):
    sc, s, _ = ts.rim_pair(name)
    n_items, ratio = ts.RIM[name]
    assert len(sc.rim) >= ts.RIM_MIN_TARGETS and len({r["case"].pixel for r in sc.rim}) == len(sc.rim)
    assert {r["case"].offset for r in sc.rim} == set(range(-es.K, es.K + 1))
    spheres, tight, k = ts.tight_of(s)
    assert int(tight.sum()) == len(sc.rim) and not tight[0]                   # every block's bound; the root holds the eye
    for r in sc.rim:
        cs, m = r["case"], r["centre"]
        its = sc.items[r["items"]]
        assert len(its) == n_items and len(set(its[:, 3])) == 1
        D = np.linalg.norm(its[:, :3] - m, axis=1)
        assert np.ptp(D) <= 4 * ts.RIM_GRID                                   # on one circle around m ...
        if n_items == 2:
            assert np.array_equal(0.5 * (its[0, :3] + its[1, :3]), m)         # ... the midpoint, exactly
        # the rim item sits within K ulps of where the reference's verdict on the target ray flips, on the side its offset says
        assert abs(es._bits(cs.value, oracle.F32) - es._bits(cs.flip, oracle.F32)) <= es.K
        assert np.isfinite(oracle.sphere_distance_from_ray(its[0], cs.ray, oracle.F32)) == cs.outcome
        # ... touched at its outermost point: the ray's nearest point to the centre lies along m -> centre
        o, d = cs.ray[:3], cs.ray[3:]
        foot = o + ((its[0, :3] - o) @ d) * d - its[0, :3]
        assert foot @ (its[0, :3] - m) >= (1.0 - 1e-6) * np.linalg.norm(foot) * D[0]
        v = np.linalg.norm(its[0, :3] - np.asarray(sc.eye))
        assert 0.8 * ratio <= v / its[0, 3] <= 1.25 * ratio
        # the closed form is a lower bound of any enclosing ball around m, and the library's ball is no smaller than the smallest one
        assert r["plain"][3] >= D.max() + its[0, 3] and spheres[r["bound"], 3] >= r["plain"][3]


@pytest.mark.parametrize("name", sorted(ts.RIM))
def test_the_theorem_holds_on_the_rim_fixtures(name):
    _, s, _ = ts.rim_pair(name)
    lib, _ = _rim_tallies(name)
    assert lib.hits >= len(ts.rim_scene(name).rim) // 4 and not lib.violations, lib.violations[:3]
    _holds(ts.check_scene(s), name)


def test_the_checker_notices_a_missing_inflation():
    # the same rays on the un-inflated ball of the same centre, radius max(D + r) rounded up: it encloses its items, and the reference's f32
    # test still misses it on rays that hit the item on its rim
    found = {name: _rim_tallies(name)[1] for name in sorted(ts.RIM)}
    for name, t in found.items():
        print("%s: %d tuned rays hit their item; the un-inflated ball: %d not finite, %d further away" % (name, t.hits, len(t.finite), len(t.order)))
    assert sum(len(t.violations) for t in found.values()) >= 1
