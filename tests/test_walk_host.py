"""The per-walk records (rust-tracer_amd/csrc/rt_tight.hpp build_walk, NOTES.md "Per-walk bounds") on the host: for every bound with a
record and every item of its subtree, whenever the REFERENCE's f32 sphere test of the item returns a finite distance, the primary filter as
the loops form it lets the ray through (b' >= T') and the shadow filter on the light disc does not say MISS (P2 <= R2o', and the
behind-the-origin test on the disc's front does not fire).  Scenes: the posed and placed `nested` and `concentric` scenes and the rim
fixtures of tests/tight_scenes.py; rim rays for either claim, on which the records of the plain geometry (no rounding term) must FAIL; the
host and device statements of the items' own bounds are one function (csrc/rt_filter_bounds.hpp).  No GPU."""
import numpy as np
import pytest

from tests import posed_scenes as ps
from tests import tight_scenes as ts
from tests import walk_scenes as ws

EYES = ("home", "left", "far")
POSED = [(scene, "home", eye, placement) for scene in sorted(ps.SCENES) for eye in EYES for placement in ("id", "moved", "x1e+06")] + \
        [(scene, light, "left", "id") for scene in sorted(ps.SCENES) for light in ("+y", "up", "-x")]
PLACED = [k for k in ts.placed_inputs() if k[0] in ("x5e+13", "+3e3")]

# The share of bounds that must carry a record, from the census of these scenes (a scratch run of capi.walk_bounds over every input below):
# posed and placed `nested` 31 of 40 and `concentric` 34 of 40 -- every bound that has a tight ball gets an eye sphere and a light disc --,
# the rim fixtures all but the root.  The conditions ask for three quarters: above one half, below what the census found.
MIN_SHARE = 0.75


def _census(scene):
    records, fr = ws.walk_of(scene)
    fl = ws.flags_of(records)
    _, tight, _ = ts.tight_of(scene)
    assert not np.any(fl[tight == 0]), "a record on a bound without a tight ball"
    return records, fr, float(np.mean(fl & ws.EYE_SPHERE != 0)), float(np.mean(fl & ws.LIGHT_DISC != 0))


def _holds(scene, what):
    records, fr, eye_share, disc_share = _census(scene)
    assert eye_share >= MIN_SHARE and disc_share >= MIN_SHARE, (what, eye_share, disc_share)
    t = ws.check_scene(scene, records=records, fr=fr)
    print("%s: eye spheres %.2f, light discs %.2f of the bounds; %d rays, %d hit their item; asked %d cones, %d discs; cone / disc radius %.3f / %.3f of the tight ball's"
          % (what, eye_share, disc_share, t.rays, t.hits, t.primary_asked, t.shadow_asked, fr["cone_ratio"], fr["disc_ratio"]))
    assert not t.violations, (what, len(t.cone), len(t.disc), t.violations[:3])
    assert t.rays >= 1000 and t.primary_asked >= 500 and t.shadow_asked >= 100, (what, t.rays, t.primary_asked, t.shadow_asked)
    # the records are narrower than the tight ball's own filter terms, or they would not be there
    assert fr["cone_ratio"] < 1.0 and fr["disc_ratio"] < 1.0


@pytest.mark.parametrize("key", POSED, ids="-".join)
def test_the_claims_hold_in_the_references_arithmetic_on_posed_scenes(key):
    _holds(ts.posed_scene(key), "-".join(key))


@pytest.mark.parametrize("key", PLACED, ids="-".join)
def test_the_claims_hold_in_the_references_arithmetic_on_placed_scenes(key):
    _holds(ts.placed_case(key).scene, "-".join(key))


@pytest.mark.parametrize("name", sorted(ts.RIM))
def test_the_claims_hold_on_the_rim_fixtures(name):
    _holds(ts.rim_pair(name)[1], name)


def _cone_rim(name, slack):
    """The tuned target rays of a rim fixture (tangent to the first item of a block where its cap touches the block's cone, within 2 ulps of
    where the reference's verdict flips) against the eye spheres' thresholds."""
    sc, s, _ = ts.rim_pair(name)
    records, fr = ws.walk_of(s, slack)
    t = ws.Tally()
    for r in sc.rim:
        assert ws.flags_of(records)[r["bound"]] & ws.EYE_SPHERE, (name, r["bound"])
        ws.ask(t, s, records, fr, r["item"], [r["ray"]], True)
    return t


def _disc_rim(name, slack):
    """Rays along the light past the item whose disc touches its block's light disc, an origin coordinate tuned to the ulp where the
    reference's verdict flips: the last origin that hits, and its neighbour that misses."""
    _, s, _ = ts.rim_pair(name)
    records, fr = ws.walk_of(s, slack)
    rays = ws.disc_rim_rays(s, *ws.walk_of(s, True))           # (the same rays for both: placed by the library's discs)
    t = ws.Tally()
    for b, i, hit, miss in rays:
        ws.ask(t, s, records, fr, i, [hit, miss], False)
    return t, len(rays)


@pytest.mark.parametrize("name", sorted(ts.RIM))
def test_the_rim_rays_pass_the_library_records(name):
    cone = _cone_rim(name, True)
    disc, n = _disc_rim(name, True)
    print("%s: cone rim %d rays, %d hit; disc rim %d tuned pairs, %d hit" % (name, cone.rays, cone.hits, n, disc.hits))
    assert cone.hits >= len(ts.rim_scene(name).rim) // 4 and not cone.violations, cone.violations[:3]
    assert n >= ts.RIM_MIN_TARGETS and disc.hits >= n and not disc.violations, disc.violations[:3]


def test_the_checker_notices_records_without_their_rounding_terms():
    # the same rays against records of the plain geometry (the items' silhouette caps and own discs, no rounding term): the reference's f32
    # test still sees items the plain cone or the plain disc rules out -- a fixture that passed here would prove nothing above
    cone = {name: _cone_rim(name, False) for name in sorted(ts.RIM)}
    disc = {name: _disc_rim(name, False)[0] for name in sorted(ts.RIM)}
    for name in sorted(ts.RIM):
        print("%s, plain geometry: cone rim %d of %d hits ruled out; disc rim %d of %d" % (name, len(cone[name].cone), cone[name].hits, len(disc[name].disc), disc[name].hits))
    assert sum(len(t.cone) for t in cone.values()) >= 1
    assert sum(len(t.disc) for t in disc.values()) >= 1


def test_one_statement_of_the_items_bounds():
    # csrc/rt_filter_bounds.hpp is what k_build_fstreams calls and what build_walk calls: rt_skip.hpp holds no copy of either formula
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rust-tracer_amd", "csrc")
    skip = open(os.path.join(root, "rt_skip.hpp")).read()
    tight = open(os.path.join(root, "rt_tight.hpp")).read()
    assert "rt_bounds::primary_threshold(vv_f, rr_f)" in skip and "rt_bounds::shadow_bounds(fc.S, fc.eta, rr_f, r2o, r2i)" in skip
    assert "rt_bounds::primary_threshold(" in tight and "rt_bounds::shadow_bounds(" in tight
    assert skip.count("102.7") == 0 and skip.count("1e-44") == 0           # (constants of the two derivations: stated once, in the shared header)
