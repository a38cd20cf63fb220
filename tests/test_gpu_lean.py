"""The lean BOUND step (rust-tracer_amd/csrc/rt_filter_bounds.hpp lean_radius, NOTES.md "Lean bound steps") on the GPU: every frame rendered
over the per-walk streams of a scene made under RT_DEBUG_LEAN_BOUNDS 0 (the build kernel writes no flag) and 2 (every bound with an eye
sphere carries Rq and the flag), byte for byte against the oracle, through the generic filtered kernel, k_render_skip_fast and
k_render_skip_fast_coop (passes of more samples: the generic kernel with one ray per lane); the launch says `lean_bounds` for every launch
of a scene that asked and has an eye sphere, and for none under 0; the counting launch behind each scene holds every ITEM test that counts
against b' - Rq of the enclosing lean bounds and counts no violation.  Inputs: those of tests/test_gpu_walk.py, thinned -- posed and placed
`nested` and `concentric` scenes at 128 x 128 and a ragged 200 x 120, passes of 1, 4 and 16 samples, the rim fixtures, the default scene
at levels 4 and 5, and one pose with the eye inside the root, whose stream has lean and exact bounds side by side.
tests/test_lean_host.py holds the same records on the CPU."""
import os

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests import posed_scenes as ps
from tests import tight_scenes as ts
from tests import util
from tests import walk_scenes as ws

pytestmark = pytest.mark.gpu

HIER_EXIT = oracle.MODE_HIERARCHY | oracle.MODE_ANYHIT_EXIT
THREADS = max(1, min(16, os.cpu_count() or 1))
F32 = rta.RT_F32

_ASKED = {}                       # input group -> [launches that set lean_bounds, launches of scenes made with the knob at 2]


def _frame(d, shape, regs, controls):
    with capi.debug(capi.DEBUG_TIGHT_BOUNDS, 2), capi.debug(capi.DEBUG_WALK_BOUNDS, 2):
        for key, value in controls:
            capi.debug_set(key, value)
        try:
            data, _ = d.render_tiles(shape, regs, rta.RT_TRAVERSAL_SKIP, want_stats=False)
            flags = capi.last_launch()
        finally:
            for key, _ in controls:
                capi.debug_set(key, -1)
    return util.stitch(shape, regs, data), flags


def _lean(group, scene, ref, shape, regs):
    """One scene's frame through every kernel over per-walk streams made without and with the lean records; one counting launch behind each."""
    _, rq = capi.lean_bounds(scene.items, scene.directional_light, scene.eye, scene.bounds, [tuple(r) for r in scene.ranges])
    expect = bool((rq > 0.0).any())
    covered = np.zeros(ref.shape[:2], dtype=bool)
    for (l, t, r, b) in regs:
        covered[b:t, l:r] = True
    modes = ws.WALKS if shape[2] == 1 else ("one_ray",)
    for lb in (0, 2):
        # (the control is read when the scene's per-walk streams are made: by its worker, or by the first launch that wants them)
        with capi.debug(capi.DEBUG_LEAN_BOUNDS, lb):
            d = rta.DeviceScene(scene)
            try:
                for mode in modes:
                    frame, flags = _frame(d, shape, regs, ts.MODES[mode])
                    np.testing.assert_array_equal(frame[covered], ref[covered], err_msg="RT_DEBUG_LEAN_BOUNDS %d, %s" % (lb, mode))
                    assert ("lean_bounds" in flags) == (lb == 2 and expect), (lb, mode, flags)
                    assert "lean_bounds" not in flags or "walk_bounds" in flags, flags
                    if lb == 2:
                        tally = _ASKED.setdefault(group, [0, 0])
                        tally[0] += "lean_bounds" in flags
                        tally[1] += 1
                # the counting launch: the given streams, every ITEM test that counts held against the records of this scene's streams
                before = capi.debug_count(capi.DEBUG_COUNT_FILTER_VIOLATIONS)
                data, _ = d.render_tiles(shape, regs, rta.RT_TRAVERSAL_SKIP, want_stats=True)
                np.testing.assert_array_equal(util.stitch(shape, regs, data)[covered], ref[covered])
                assert capi.debug_count(capi.DEBUG_COUNT_TIGHT_VIOLATIONS) == 0
                assert capi.debug_count(capi.DEBUG_COUNT_FILTER_VIOLATIONS) == before
            finally:
                d.close()
    return expect


SQUARE, RAGGED = (128, 128, 1), (200, 120, 1)
POSED = [(scene, l, e, placement, F32, shape) for scene in sorted(ps.SCENES)
         for l, e, placement, shape in (("home", "home", "id", SQUARE), ("+y", "left", "moved", SQUARE), ("up", "home", "id", RAGGED))] + \
        [(scene, "+y", "left", "moved", F32, shape) for scene in sorted(ps.SCENES) for shape in ps.RAGGED_SHAPES]


@pytest.mark.parametrize("param", POSED, ids=ps.case_id)
def test_a_posed_frame_with_lean_bound_steps_is_the_oracles(param):
    c = ps.case(*param)
    assert _lean("posed", c.scene, ps.frame(param)[0], c.shape, ps.regions(c.shape))


def test_the_posed_frames_cover_the_sizes_and_sample_counts():
    assert {p[5][2] for p in POSED} == {1, 2, 4} and SQUARE in {p[5] for p in POSED} and RAGGED in {p[5] for p in POSED}


PLACED = [(("x5e+13", name), SQUARE) for name in ("nested", "concentric")] + [(("+3e3", name), RAGGED) for name in ("nested", "concentric")]


@pytest.mark.parametrize("key,shape", PLACED, ids=lambda v: "-".join(v) if isinstance(v[0], str) else "%dx%d" % v[:2])
def test_a_placed_frame_with_lean_bound_steps_is_the_oracles(key, shape):
    c = ts.placed_case(key)
    ref = c.oracle.render(shape[0], shape[1], 1, THREADS, HIER_EXIT)[0]
    assert _lean("placed", c.scene, ref, shape, ps.regions(shape))


@pytest.mark.parametrize("name", sorted(ts.RIM))
def test_a_rim_fixture_with_lean_bound_steps_is_the_oracles(name):
    sc, s, o = ts.rim_pair(name)
    shape = (sc.w, sc.h, 1)
    ref = o.render(sc.w, sc.h, 1, THREADS, HIER_EXIT)[0]
    assert _lean("rim", s, ref, shape, ps.regions(shape))


@pytest.mark.parametrize("level", (4, 5))
def test_the_default_scene_with_lean_bound_steps_is_the_oracles(level):
    shape = (160, 120, 1)
    ref = oracle.Scene.default(oracle.F32, level).render(160, 120, 1, THREADS, HIER_EXIT)[0]
    assert _lean("default", rta.Scene.default(level), ref, shape, ps.regions(shape))


def test_lean_and_exact_bounds_side_by_side():
    # the eye inside the root: the bounds that hold it keep the reference's test, the others are lean -- one stream, both paths
    param = ("nested", "home", "inside_root", "id", F32, SQUARE)
    c = ps.case(*param)
    _, rq = capi.lean_bounds(c.scene.items, c.scene.directional_light, c.scene.eye, c.scene.bounds, [tuple(r) for r in c.scene.ranges])
    assert 0 < int((rq > 0.0).sum()) < len(rq)
    assert _lean("mixed", c.scene, ps.frame(param)[0], c.shape, ps.regions(c.shape))


def test_the_launches_that_took_the_lean_step():
    # the census of this process's launches above (printed for the record; run alone it has nothing to say)
    for group in sorted(_ASKED):
        took, asked = _ASKED[group]
        print("LEAN LAUNCHES %-8s %4d of %4d launches set lean_bounds" % (group, took, asked))
        assert took == asked, group
