"""The tight spheres of the filtered f32 walks (rust-tracer_amd/csrc/rt_tight.hpp) on the host: every one encloses its subtree's items with the
stated inflation, and a bound that leaves an item outside or holds the eye keeps the sphere it was given, bit for bit.
tests/test_tight_poses_host.py holds the same, and the theorem behind the inflation, on every light, eye and placement of the frame tests.
No GPU."""
import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests import tight_scenes as ts


def _tight(scene):
    return capi.tight_bounds(scene.items, scene.directional_light, scene.eye, scene.bounds, [tuple(r) for r in scene.ranges])


@pytest.mark.parametrize("level", [2, 5])
def test_every_tight_sphere_of_the_default_scene_encloses_its_subtree(level):
    s = rta.Scene.default(level)
    spheres, tight, k = _tight(s)
    assert tight.all() and k["rule"] == 1 and k["volume_ratio"] < 0.75
    for b, (first, count) in enumerate(s.ranges):
        assert ts.encloses_with_inflation(spheres[b], s.items[first:first + count], k["S"], k["eta"]), b
        assert spheres[b, 3] < s.bounds[b, 3]
        # (the pyramid's items fit into 2.454 r, the given bound is 3 r: the inflation must not eat the difference)
        assert spheres[b, 3] < 0.85 * s.bounds[b, 3], b


@pytest.mark.parametrize("name", sorted(ts.FIXTURES))
def test_bounds_that_must_keep_their_record_keep_it(name):
    items, bounds, ranges, keeps = ts.FIXTURES[name]
    s = rta.Scene(items, rta.normalized(ts.LIGHT), ts.EYE, bounds, ranges)
    spheres, tight, k = _tight(s)
    for b, (first, count) in enumerate(ranges):
        if b in keeps:
            assert tight[b] == 0 and spheres[b].tobytes() == s.bounds[b].tobytes(), b
        else:
            assert tight[b] == 1 and spheres[b, 3] < s.bounds[b, 3], b
            assert ts.encloses_with_inflation(spheres[b], s.items[first:first + count], k["S"], k["eta"]), b
    if name == "outside":
        # the fixture is what it says: the kept bound does not even enclose its items plainly
        assert not ts.encloses_with_inflation(s.bounds[1], s.items[1:3], k["S"], k["eta"])


def test_the_rule_for_a_scene_whose_deepest_groups_do_not_qualify():
    # level 9: the 16,384 deepest groups (three quarters of all) are too small for the inflation; un-fusing the walk for the quarter that
    # qualifies pays in large one-sample passes only (rule 2), where level 8 -- every bound tight -- walks them everywhere (rule 1)
    s = rta.Scene.default(9)
    _, tight, k = _tight(s)
    assert int(tight.sum()) == 5461 and len(tight) == 21845 and k["rule"] == 2
    assert _tight(rta.Scene.default(8))[2]["rule"] == 1


def test_a_built_hierarchy_has_nothing_to_gain():
    rng = np.random.default_rng(7)
    sph = np.concatenate([rng.uniform(-2.0, 2.0, (300, 3)), rng.uniform(0.02, 0.2, (300, 1))], axis=1)
    s = rta.Scene.from_spheres_auto(sph)
    _, tight, k = _tight(s)
    assert int(tight.sum()) == 0 and not k["by_rule"], (int(tight.sum()), k)
