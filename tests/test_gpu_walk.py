"""The per-walk filter streams (rust-tracer_amd/csrc/rt_tight.hpp build_walk, NOTES.md "Per-walk bounds") on the GPU: every frame rendered
over the tight streams with the per-walk streams off (RT_DEBUG_WALK_BOUNDS 0) and on (2), byte for byte against the oracle, through the
generic filtered kernel, k_render_skip_fast and k_render_skip_fast_coop (passes of more samples: the generic kernel with one ray per lane);
the launch says `walk_bounds` for every launch that was asked to read the records and for none under 0; the counting launch behind every
frame holds each ITEM test against T' and the light discs of the enclosing bounds and counts no violation.  Inputs: posed and placed
`nested` and `concentric` scenes at 128 x 128 and a ragged 200 x 120, the three sample counts of the tight tests, the rim fixtures, and
the default scene at levels 4 and 5.  tests/test_walk_host.py holds the same records on the CPU."""
import os

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests import posed_scenes as ps
from tests import tight_scenes as ts
from tests import walk_scenes as ws

pytestmark = pytest.mark.gpu

HIER_EXIT = oracle.MODE_HIERARCHY | oracle.MODE_ANYHIT_EXIT
THREADS = max(1, min(16, os.cpu_count() or 1))
F32 = rta.RT_F32

_WALKED = {}                      # input group -> [launches that read the per-walk streams, launches with the knob at 2]


def _walk(group, scene, ref, shape, regs):
    """One scene's frame through every kernel, with and without the per-walk streams (ws.frames); a counting launch behind every frame."""
    records, _ = ws.walk_of(scene)
    expect = bool(ws.flags_of(records).any())
    modes = ws.WALKS if shape[2] == 1 else ("one_ray",)
    d = rta.DeviceScene(scene)
    try:
        for mode in modes:
            n = ws.frames(d, ref, shape, regs, expect_walk=expect, controls=ts.MODES[mode], count=True)
            assert n == int(expect), (mode, n)
            tally = _WALKED.setdefault(group, [0, 0])
            tally[0] += n
            tally[1] += 1
    finally:
        d.close()
    return expect


SQUARE, RAGGED = (128, 128, 1), (200, 120, 1)
POSED = [(scene, l, e, placement, F32, SQUARE) for scene in sorted(ps.SCENES) for placement in ("id", "moved") for l, e in (("home", "home"), ("+y", "left"))] + \
        [(scene, "up", "home", "id", F32, RAGGED) for scene in sorted(ps.SCENES)] + \
        [(scene, "+y", "left", "moved", F32, shape) for scene in sorted(ps.SCENES) for shape in ps.RAGGED_SHAPES]


@pytest.mark.parametrize("param", POSED, ids=ps.case_id)
def test_a_posed_frame_over_the_per_walk_streams_is_the_oracles(param):
    c = ps.case(*param)
    assert _walk("posed", c.scene, ps.frame(param)[0], c.shape, ps.regions(c.shape))


def test_the_posed_frames_cover_the_sizes_and_sample_counts():
    assert {p[5][2] for p in POSED} == {1, 2, 4} and SQUARE in {p[5] for p in POSED} and RAGGED in {p[5] for p in POSED}


PLACED = [k for k in ts.placed_inputs() if k[0] in ("x5e+13", "+3e3")]


@pytest.mark.parametrize("shape", (SQUARE, RAGGED), ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("key", PLACED, ids="-".join)
def test_a_placed_frame_over_the_per_walk_streams_is_the_oracles(key, shape):
    c = ts.placed_case(key)
    ref = c.oracle.render(shape[0], shape[1], 1, THREADS, HIER_EXIT)[0]
    assert _walk("placed", c.scene, ref, shape, ps.regions(shape))


@pytest.mark.parametrize("name", sorted(ts.RIM))
def test_a_rim_fixture_over_the_per_walk_streams_is_the_oracles(name):
    sc, s, o = ts.rim_pair(name)
    assert len({r["case"].pixel for r in sc.rim}) >= ts.RIM_MIN_TARGETS
    shape = (sc.w, sc.h, 1)
    ref = o.render(sc.w, sc.h, 1, THREADS, HIER_EXIT)[0]
    assert _walk("rim", s, ref, shape, ps.regions(shape))


@pytest.mark.parametrize("level", (4, 5))
def test_the_default_scene_over_the_per_walk_streams_is_the_oracles(level):
    shape = (160, 120, 1)
    ref = oracle.Scene.default(oracle.F32, level).render(160, 120, 1, THREADS, HIER_EXIT)[0]
    assert _walk("default", rta.Scene.default(level), ref, shape, ps.regions(shape))


def test_the_launches_that_read_the_per_walk_streams():
    # the census of this process's launches above (printed for the record; run alone it has nothing to say)
    for group in sorted(_WALKED):
        walked, asked = _WALKED[group]
        print("WALK LAUNCHES %-8s %4d of %4d launches set walk_bounds" % (group, walked, asked))
        assert walked == asked, group
