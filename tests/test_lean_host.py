"""The lean BOUND step (rust-tracer_amd/csrc/rt_filter_bounds.hpp lean_radius, NOTES.md "Lean bound steps") on the host: a bound with an
eye sphere X is entered iff b'_X >= T'_X and b'_X - Rq_X < hit.distance, so no item I of its subtree may come nearer than b'_X - Rq_X.  The
claim is asked of the REFERENCE's f32 sphere test: for every such bound and every item of its subtree, on the grazing rays of
tests/tight_scenes.py from the eye (impact parameters (1 +- 1e-6, 1 +- 3e-6, 1 - 1e-3, 0.8) r at four azimuths), the central ray through
the item's near pole, and the ray through the point of the item nearest the eye sphere's near pole -- where the margin is smallest --:
wherever oracle.sphere_distance_from_ray in f32 is finite, b'_X - Rq_X <= d_I, with b' as the loops form it (tests/walk_scenes.py b_prime:
one rounding per fma).  Scenes: the posed and placed scenes of tests/test_walk_host.py, the rim fixtures, the default scene at levels 4
and 5.  The census gate runs tools/step_census.cpp --lean against the figures the change was derived with.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests import posed_scenes as ps
from tests import tight_scenes as ts
from tests import walk_scenes as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

EYES = ("home", "left", "far")
POSED = [(scene, "home", eye, placement) for scene in sorted(ps.SCENES) for eye in EYES for placement in ("id", "moved", "x1e+06")] + \
        [(scene, light, "left", "id") for scene in sorted(ps.SCENES) for light in ("+y", "up", "-x")]
PLACED = [k for k in ts.placed_inputs() if k[0] in ("x5e+13", "+3e3")]
MIXED = [(scene, light, "inside_root", "id") for scene in sorted(ps.SCENES) for light in ("home", "+y")]
MIN_SHARE = 0.75                  # of the bounds of a posed scene: the figure tests/test_walk_host.py holds the same scenes to


def lean_of(scene):
    """(records of capi.walk_bounds, Rq per bound: > 0 exactly where the bound has an eye sphere)."""
    records, rq = capi.lean_bounds(scene.items, scene.directional_light, scene.eye, scene.bounds, [tuple(r) for r in scene.ranges])
    fl = ws.flags_of(records)
    assert np.array_equal(rq > 0.0, fl & ws.EYE_SPHERE != 0), "Rq exactly where a bound has an eye sphere"
    assert np.all(np.isfinite(rq))
    return records, rq


def _through(eye, point):
    """The primary-type ray from the eye through `point`: the direction rounded to f32 and normalised as the reference normalises one."""
    d = (np.asarray(point, dtype=np.float64) - eye).astype(F32)
    return np.concatenate([eye, oracle.vec_normalized(d, oracle.F32)[0]])


def rays_of(eye, item, sphere):
    """The rays on `item` the claim is asked on, for the enclosing eye sphere `sphere`."""
    c, r = item[:3], float(item[3])
    x, rx = np.asarray(sphere[:3], dtype=np.float64), float(sphere[3])
    rays = list(ts.primary_rays(eye, item, c - x))
    v = c - eye
    rays.append(_through(eye, c - r * v / np.linalg.norm(v)))                 # the central ray, through the item's near pole
    u = x - eye
    pole = eye + (np.linalg.norm(u) - rx) * u / np.linalg.norm(u)             # the eye sphere's near pole ...
    w = pole - c
    if np.linalg.norm(w) > 0.0:
        rays.append(_through(eye, c + r * w / np.linalg.norm(w)))             # ... and the point of the item nearest to it
    return rays


class Tally:
    def __init__(self):
        self.rays = self.hits = self.asked = self.bare = 0
        self.margin = np.inf           # the smallest (d_I - (b' - Rq)) / Rq
        self.violations = []


def check_scene(scene, records, rq):
    fl = ws.flags_of(records)
    items = np.asarray(scene.items, dtype=np.float64)
    eye = np.asarray(scene.eye, dtype=np.float64)
    t = Tally()
    for b in np.nonzero(fl & ws.EYE_SPHERE)[0]:
        first, count = (int(v) for v in scene.ranges[b])
        bare = float(np.nextafter(records[b, 3], F32(0.0)))                   # the bare radius rounded down: what the slack is for
        for i in range(first, first + count):
            for ray in rays_of(eye, items[i], records[b, :4]):
                t.rays += 1
                d = oracle.sphere_distance_from_ray(items[i], ray, oracle.F32)
                if not np.isfinite(d):
                    continue
                t.hits += 1
                bp = float(ws.b_prime(records[b, :4], scene.eye, ray[3:]))
                t.asked += 1                                                  # (inside the cone or not: tests/test_walk_host.py holds b' >= T' for these)
                t.margin = min(t.margin, (float(d) - (bp - float(rq[b]))) / float(rq[b]))
                t.bare += not bp - bare <= float(d)
                if not bp - float(rq[b]) <= float(d):
                    t.violations.append((int(b), i, tuple(ray), bp, float(rq[b]), float(d)))
    return t


def _holds(scene, what, min_share=None, min_asked=500):
    records, rq = lean_of(scene)
    share = float(np.mean(rq > 0.0))
    if min_share is not None:
        assert share >= min_share, (what, share)
    t = check_scene(scene, records, rq)
    print("%s: lean flags on %.2f of %d bounds; %d rays, %d hit their item, %d asked; smallest margin %.3g Rq; %d rays fail with the bare radius rounded down"
          % (what, share, len(rq), t.rays, t.hits, t.asked, t.margin, t.bare))
    assert not t.violations, (what, len(t.violations), t.violations[:3])
    assert t.asked >= min_asked, (what, t.asked)
    return share


@pytest.mark.parametrize("key", POSED, ids="-".join)
def test_no_item_is_nearer_than_b_minus_rq_on_posed_scenes(key):
    _holds(ts.posed_scene(key), "-".join(key), MIN_SHARE)


@pytest.mark.parametrize("key", PLACED, ids="-".join)
def test_no_item_is_nearer_than_b_minus_rq_on_placed_scenes(key):
    _holds(ts.placed_case(key).scene, "-".join(key), MIN_SHARE)


@pytest.mark.parametrize("name", sorted(ts.RIM))
def test_no_item_is_nearer_than_b_minus_rq_on_the_rim_fixtures(name):
    _holds(ts.rim_pair(name)[1], name, MIN_SHARE)


@pytest.mark.parametrize("level", (4, 5))
def test_no_item_is_nearer_than_b_minus_rq_on_the_default_scene(level):
    _holds(rta.Scene.default(level), "default L%d" % level, MIN_SHARE)


@pytest.mark.parametrize("key", MIXED, ids="-".join)
def test_a_scene_with_flagged_and_unflagged_bounds(key):
    # the eye inside the root: 23 - 33 of the 40 bounds carry a tight ball, the others keep the reference's test -- one stream walks both paths
    scene = ts.posed_scene(key)
    share = _holds(scene, "-".join(key), None, min_asked=100)
    assert 0.0 < share < 1.0, share


def test_rq_is_one_statement_for_host_and_device():
    csrc = os.path.join(ROOT, "rust-tracer_amd", "csrc")
    bounds = open(os.path.join(csrc, "rt_filter_bounds.hpp")).read()
    assert bounds.count("float lean_radius(") == 1
    assert "rt_bounds::lean_radius(" in open(os.path.join(csrc, "rt_tight.hpp")).read()
    skip = open(os.path.join(csrc, "rt_skip.hpp")).read()
    assert "fp.a4 = o.rq; fp.tag = rt_bounds::kTagLeanBound" in skip           # the device copies the host's value: no second formula
    assert "LEAN_TAG = \"0x20000000\"" in open(os.path.join(ROOT, "tools", "gen_skip_asm.py")).read() and "kTagLeanBound = 0x20000000u" in bounds


# ---- the census gate ----------------------------------------------------------------------------------------------------------------

WALK_STEPS_1080P = 577970          # tools/step_census.cpp --walk, 1920 x 1080 level 8: the steps of the exact BOUND test
GATE = 1.025                       # the weaker cull may cost this much and no more


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("census") / "step_census")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-w", "-o", exe, os.path.join(ROOT, "tools", "step_census.cpp")], check=True)
    return exe


@pytest.mark.parametrize("w,h,hash_", [(1920, 1080, "02d8eb4bcce46798"), (800, 600, "4fca3a65f5b3b2c2")])
def test_the_census_of_the_lean_walk(census, w, h, hash_):
    import re
    out = subprocess.run([census, str(w), str(h), "8", "--lean"], capture_output=True, text=True, check=True)
    print(out.stdout)
    assert out.stderr == "", out.stderr                                        # (a lane asleep where the exact test finds a winner is reported there)
    m = re.search(r"steps: primary (\d+), shadow (\d+); hash of hit items and shadow verdicts ([0-9a-f]{16})", out.stdout)
    assert m and m.group(3) == hash_, out.stdout
    assert re.search(r"sleeping lanes the exact test makes winners 0\b", out.stdout)
    if (w, h) == (1920, 1080):
        assert int(m.group(1)) <= GATE * WALK_STEPS_1080P, m.group(1)
