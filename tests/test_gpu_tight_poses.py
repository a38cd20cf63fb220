"""The tight streams (rust-tracer_amd/csrc/rt_tight.hpp, NOTES.md T) on the GPU away from the home pose: every frame rendered over the given
streams (RT_DEBUG_TIGHT_BOUNDS 0) and over the tight ones (2), byte for byte against the oracle, through every kernel a launch can take
(tests/tight_scenes.py MODES); the launch says `tight_bounds` exactly when the knob is 2 and the scene has a tight bound; the counting
launch behind them counts no ITEM test that a tight bound would have culled.  Inputs: the posed frames of tests/posed_scenes.py (every eye --
inside the root, at an item's centre, inside an item: there rule (c) decides node by node -- and every light), the placed scenes of
tests/scaled_scenes.py, the edge scenes with bounds that qualify, and the rim fixtures of tests/tight_scenes.py, whose target pixels' rays
touch an item where it touches the smallest ball.  tests/test_tight_poses_host.py holds the same inputs on the CPU."""
import functools
import os

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests import edge_scenes as es
from tests import posed_scenes as ps
from tests import tight_scenes as ts
from tests import util

pytestmark = pytest.mark.gpu

HIER_EXIT = oracle.MODE_HIERARCHY | oracle.MODE_ANYHIT_EXIT
SKIP = rta.RT_TRAVERSAL_SKIP
THREADS = max(1, min(16, os.cpu_count() or 1))
F32 = rta.RT_F32
STAR_LIGHTS = ("home", "+y", "up")

_WALKED = {}                      # input group -> [launches that walked the tight streams, launches with the knob at 2]


def _walk(group, scene, ref, shape, regs):
    """One scene's frame through every kernel, over both pairs of streams (ts.frames); one counting launch behind them."""
    _, tight, _ = ts.tight_of(scene)              # (first: on the library that ships this needs a control, and the test skips here)
    expect = bool(tight.any())
    modes = ts.WALKS + (("one_ray",) if shape[2] > 1 else ())
    d = rta.DeviceScene(scene)
    try:
        for k, mode in enumerate(modes):
            n = ts.frames(d, ref, shape, regs, expect_tight=expect, controls=ts.MODES[mode], count=k == len(modes) - 1)
            assert n == int(expect), (mode, n)
            tally = _WALKED.setdefault(group, [0, 0])
            tally[0] += n
            tally[1] += 1
    finally:
        d.close()
    return expect


def _posed_params():
    out = []
    for scene in sorted(ps.SCENES):
        for placement in ("id", "moved"):
            poses = [(l, e) for e in tuple(ps.EYES) + ps.SPECIAL_EYES for l in STAR_LIGHTS] + [(l, "left") for l in ps.LIGHTS]
            out.extend((scene, l, e, placement, F32, ps.SHAPE) for l, e in dict.fromkeys(poses))
            out.extend((scene, l, e, placement, F32, shape) for l, e in ps.RAGGED_POSES for shape in ps.RAGGED_SHAPES)
    out.extend((scene, l, e, placement, F32, ps.SHAPE) for scene, l, e, placement in ps.SCALED_POSES)
    return out


POSED = _posed_params()


@pytest.mark.parametrize("param", POSED, ids=ps.case_id)
def test_a_posed_frame_over_the_tight_streams_is_the_oracles(param):
    c = ps.case(*param)
    expect = _walk("posed " + param[3], c.scene, ps.frame(param)[0], c.shape, ps.regions(c.shape))
    # the two poses at 1e-10 have nothing to walk (and rendered the same bytes at 0 and 2); everything else has
    assert expect == (param[3] != "x1e-10")


def test_the_posed_frames_cover_what_they_should():
    keys = {p[:4] for p in POSED}
    for scene in ps.SCENES:
        for placement in ("id", "moved"):
            assert {(l, e) for s, l, e, p in keys if s == scene and p == placement} >= (
                {(l, e) for l in STAR_LIGHTS for e in tuple(ps.EYES) + ps.SPECIAL_EYES} | {(l, "left") for l in ps.LIGHTS})
            for shape in ps.RAGGED_SHAPES:
                assert all((scene, l, e, placement, F32, shape) in POSED for l, e in ps.RAGGED_POSES)
    assert sum(p[3] == "x1e-10" for p in POSED) == 2 and sum(p[3] == "x1e+06" for p in POSED) == 2


PLACED = [k for k in ts.placed_inputs() if k[0] in ("x5e+13", "+3e3")]


@pytest.mark.parametrize("key", PLACED, ids="-".join)
def test_a_placed_frame_over_the_tight_streams_is_the_oracles(key):
    c = ts.placed_case(key)
    shape = (96, 64, 1)
    ref = c.oracle.render(96, 64, 1, THREADS, HIER_EXIT)[0]
    assert _walk("placed", c.scene, ref, shape, ps.regions(shape))


@functools.lru_cache(maxsize=None)
def _edge_ref(family, spp):
    sc, _, o = ts.edge_pair(family, spp)
    return o.render(sc.w, sc.h, spp, THREADS, HIER_EXIT)[0]


@pytest.mark.parametrize("spp", es.SPPS)
@pytest.mark.parametrize("family", ts.EDGE_TIGHT)
def test_an_edge_scene_over_the_tight_streams_is_the_oracles(family, spp):
    sc, s, _ = ts.edge_pair(family, spp)
    shape = (sc.w, sc.h, spp)
    assert _walk("edge " + family, s, _edge_ref(family, spp), shape, ps.regions(shape))


@pytest.mark.parametrize("name", sorted(ts.RIM))
def test_a_rim_fixture_over_the_tight_streams_is_the_oracles(name):
    sc, s, o = ts.rim_pair(name)
    assert len({r["case"].pixel for r in sc.rim}) >= ts.RIM_MIN_TARGETS
    shape = (sc.w, sc.h, 1)
    ref = o.render(sc.w, sc.h, 1, THREADS, HIER_EXIT)[0]
    assert _walk("rim", s, ref, shape, ps.regions(shape))


def test_the_rule_without_the_knob():
    # RT_DEBUG_TIGHT_BOUNDS at its default: the plain-stream scene (rule 1) walks its tight streams in every launch that can, the fused one
    # (rule 2) not at 128 x 96.  A scene's tight streams are made behind its first tile list's dispatch orders, so the first launch may
    # still walk the given ones: asserted from the second uncounted one-ray launch on.
    for scene, expect in (("nested", True), ("concentric", False)):
        param = (scene, "home", "home", "id", F32, ps.SHAPE)
        c = ps.case(*param)
        assert ts.tight_of(c.scene)[2]["rule"] == (1 if expect else 2)
        ref, regs = ps.frame(param)[0], ps.regions(c.shape)
        d = rta.DeviceScene(c.scene)
        try:
            with capi.debug(capi.DEBUG_SKIP_RAYS, 1):
                for k in range(3):
                    data, _ = d.render_tiles(c.shape, regs, SKIP, want_stats=False)
                    flags = capi.last_launch()
                    np.testing.assert_array_equal(util.stitch(c.shape, regs, data), ref, err_msg="%s launch %d" % (scene, k))
                    if k >= 1:
                        assert ("tight_bounds" in flags) == expect, (scene, k, flags)
                        tally = _WALKED.setdefault("no knob " + scene, [0, 0])
                        tally[0] += "tight_bounds" in flags
                        tally[1] += 1
        finally:
            d.close()


def test_the_launches_that_walked_tight_streams():
    # the census of this process's launches above (printed for the record; run alone it has nothing to say)
    for group in sorted(_WALKED):
        walked, asked = _WALKED[group]
        print("TIGHT LAUNCHES %-14s %4d of %4d launches set tight_bounds" % (group, walked, asked))
        assert 0 <= walked <= asked
        if group.startswith(("posed id", "posed moved", "posed x1e+06", "placed", "edge", "rim")) or group == "no knob nested":
            assert walked == asked, group
        else:
            assert walked == 0, group
