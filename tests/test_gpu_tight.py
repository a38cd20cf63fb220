"""The tight streams (rust-tracer_amd/csrc/rt_tight.hpp) on the GPU: frames walked over the tight bounds (RT_DEBUG_TIGHT_BOUNDS 2) and over the
given ones (0) against the oracle byte for byte, through the generic kernel, the lean kernel, cooperative quads and a sample-parallel pass;
and the launch flag that says which streams a launch walked.  tests/test_gpu_tight_poses.py does the same away from the home pose: every
light, eye and placement of the frame tests, the edge scenes, and rim fixtures with an item on the tight ball's rim."""
import functools
import os

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests import edge_scenes as es
from tests import tight_scenes as ts
from tests import util

pytestmark = pytest.mark.gpu

HIER_EXIT = oracle.MODE_HIERARCHY | oracle.MODE_ANYHIT_EXIT
SKIP = rta.RT_TRAVERSAL_SKIP
THREADS = max(1, min(16, os.cpu_count() or 1))


@functools.lru_cache(maxsize=None)
def _default(level):
    return util.scene_pair_default(level=level)


@functools.lru_cache(maxsize=None)
def _fixture(name):
    items, bounds, ranges, _ = ts.FIXTURES[name]
    return util.scene_pair_ranges(items, bounds, ranges, light=ts.LIGHT, eye=ts.EYE)


@functools.lru_cache(maxsize=None)
def _ref(key, w, h, spp):
    o = _default(key)[1] if isinstance(key, int) else _fixture(key)[1]
    return o.render(w, h, spp, THREADS, HIER_EXIT)[0]


def _frames(s, ref, opts, regs, expect_tight=True, controls=()):
    """Renders `regs` with the given and with the tight streams under `controls`; both must equal the oracle's frame where a tile covers it
    (tests/tight_scenes.py frames, shared with tests/test_gpu_tight_poses.py)."""
    ts.frames(s.device(), ref, opts, regs, expect_tight=expect_tight, controls=controls)


def _buckets(w, h, spp=1):
    return (w, h, spp), [tuple(r) for r in rta.buckets(rta.RenderOptions(w, h, spp))]


MODES = ts.MODES


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("size", [(96, 64), (160, 120)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("level", [4, 5])
def test_default_scene_frames_match_the_oracle(level, size, mode):
    s, _ = _default(level)
    opts, regs = _buckets(*size)
    _frames(s, _ref(level, size[0], size[1], 1), opts, regs, controls=MODES[mode])


@pytest.mark.parametrize("name", sorted(ts.FIXTURES))
def test_fixture_frames_match_the_oracle(name):
    # one bound of each keeps its record (rules (b) and (c)), another walks a tight sphere: the culling the reference shows stays in the picture
    s, _ = _fixture(name)
    opts, regs = _buckets(96, 64)
    for mode in ("generic", "lean_coop"):
        _frames(s, _ref(name, 96, 64, 1), opts, regs, controls=MODES[mode])


def test_an_edge_scene_matches_the_oracle():
    # the grazing-ray scenes (tests/edge_scenes.py): nodes within a few ulps of where the reference's verdict flips
    sc = es.scene("O", oracle.F32, 1)
    s, o = util.scene_pair_ranges(sc.items, sc.bounds, sc.ranges, rta.RT_F32, light=sc.light, eye=sc.eye)
    ref = o.render(sc.w, sc.h, 1, THREADS, HIER_EXIT)[0]
    opts, regs = _buckets(sc.w, sc.h)
    _, tight, _ = capi.tight_bounds(s.items, s.directional_light, s.eye, s.bounds, [tuple(r) for r in s.ranges])
    _frames(s, ref, opts, regs, expect_tight=bool(tight.any()), controls=MODES["generic"])
    _frames(s, ref, opts, regs, expect_tight=bool(tight.any()), controls=MODES["lean_coop"])


def test_a_ragged_tile_list_with_a_hole():
    s, _ = _default(5)
    regs = [(0, 50, 37, 19), (37, 50, 70, 0), (0, 19, 20, 0)]          # (l, t, r, b); nobody renders [20, 37) x [0, 19)
    for mode in ("generic", "lean_coop"):
        _frames(s, _ref(5, 70, 50, 1), (70, 50, 1), regs, controls=MODES[mode])


def test_four_samples_per_pixel_through_the_generic_kernel():
    s, _ = _default(4)
    opts, regs = _buckets(64, 48, 4)
    _frames(s, _ref(4, 64, 48, 4), opts, regs, controls=MODES["one_ray"])


def test_the_launch_flag_follows_the_rule():
    s, _ = _default(5)
    opts, regs = _buckets(96, 64)
    with capi.debug(capi.DEBUG_TIGHT_BOUNDS, 1), capi.debug(capi.DEBUG_SKIP_RAYS, 1):
        s.device().render_tiles(opts, regs, SKIP, want_stats=False)
        assert "tight_bounds" in capi.last_launch()
        # a hierarchy the library built is as tight as its items allow
        rng = np.random.default_rng(11)
        sph = np.concatenate([rng.uniform(-2.0, 2.0, (200, 3)), rng.uniform(0.05, 0.2, (200, 1))], axis=1)
        built = rta.Scene.from_spheres_auto(sph)
        data, _ = built.device().render_tiles(opts, regs, SKIP, want_stats=False)
        assert "tight_bounds" not in capi.last_launch()
        o = oracle.Scene.from_ranges(built.items, built.bounds, built.ranges, (-1.0, -3.0, 2.0), (0.0, 0.0, -4.0), oracle.F32)
        np.testing.assert_array_equal(util.stitch(opts, regs, data), o.render(96, 64, 1, THREADS, HIER_EXIT)[0])
    # a fused scene on which only some bounds qualified (level 9: a quarter) walks them in one-sample passes of a million pixels or more
    deep = rta.Scene.default(9)
    big = _buckets(1280, 800)
    frames = {}
    for tb in (0, 1):
        with capi.debug(capi.DEBUG_TIGHT_BOUNDS, tb), capi.debug(capi.DEBUG_SKIP_RAYS, 1):
            frames[tb], _ = deep.device().render_tiles(big[0], big[1], SKIP, want_stats=False)
            assert ("tight_bounds" in capi.last_launch()) == (tb == 1)
    np.testing.assert_array_equal(frames[0], frames[1])
    with capi.debug(capi.DEBUG_TIGHT_BOUNDS, 1), capi.debug(capi.DEBUG_SKIP_RAYS, 1):
        deep.device().render_tiles(opts, regs, SKIP, want_stats=False)
        assert "tight_bounds" not in capi.last_launch()
    # the two-ray kernel keeps the given streams
    with capi.debug(capi.DEBUG_TIGHT_BOUNDS, 2), capi.debug(capi.DEBUG_SKIP_RAYS, 2):
        s.device().render_tiles(opts, regs, SKIP, want_stats=False)
        assert "two_rays" in capi.last_launch() and "tight_bounds" not in capi.last_launch()
    # a dynamic scene has no tight streams: its frames go through rt_render_camera, which walks the one stream the scene has
    with capi.debug(capi.DEBUG_TIGHT_BOUNDS, 0):
        s.device().render_tiles(opts, regs, SKIP, want_stats=False)
        assert "tight_bounds" not in capi.last_launch()
    with capi.debug(capi.DEBUG_TIGHT_BOUNDS, 2):
        dyn = rta.Scene.default(4).device(dynamic=True)
        cam = np.concatenate([np.asarray((0.0, 0.0, -4.0)), [1, 0, 0, 0, 1, 0, 0, 0, 1]]).astype(np.float32)
        frame, _ = dyn.render_camera(opts, cam, regs, want_stats=False)
        assert "tight_bounds" not in capi.last_launch()
        np.testing.assert_array_equal(util.stitch(opts, regs, frame), _ref(4, 96, 64, 1))
