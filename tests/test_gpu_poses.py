"""Frames away from the home pose, bit for bit against the oracle (tests/posed_scenes.py; tests/test_poses_host.py shows on the CPU that
every case renders something): lights along an axis, lights that point up, lights with equal components; eyes off the axis, far away,
inside the root bound, at an item's centre and inside an item; the scene and the eye moved far from the origin, and scaled.  What derives
its bounds from the light and the eye -- the filtered assembly loops (plain-stream on the nested scene, fused on the concentric one), the
two-ray kernel, the cooperative walk, the lean kernels, the flat scan's filter -- renders every case; the counting launch evaluates the
filtered loops' bounds next to every test it makes (tests/conftest.py asserts that none ruled out a hit)."""
import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests import posed_scenes as ps
from tests import util
from tests.test_gpu_camera import COUNTERS, identity

pytestmark = pytest.mark.gpu
SKIP, FLAT = rta.RT_TRAVERSAL_SKIP, rta.RT_TRAVERSAL_FLAT
FLAVOURS = (1, 3, 7, 23)          # the reference C++ loop, the generated assembly, its fused form (dropped by the library where the scene
#                                   is not concentric), the filtered assembly loops: what a scene gets by itself

_SHARE = {}                       # param -> (tests the filtered loops' bound lets through, tests made) of the counted launch: f32, with hooks


def _counted(param, d):
    """The counted hierarchy launch of one case on device scene d (and, through tests/conftest.py, its plain, cooperative, lean and
    generic twins) -> (bytes, stats); records the filter's share of an f32 case where the library counts it."""
    c = ps.case(*param)
    count = capi.HAVE_TEST_HOOKS and c.scene.precision == rta.RT_F32
    before = capi.debug_count(capi.DEBUG_COUNT_FILTER_PASS) if count else 0
    data, st = d.render_tiles(c.shape, ps.regions(c.shape), SKIP, want_stats=True)
    if count:
        passed = capi.debug_count(capi.DEBUG_COUNT_FILTER_PASS) - before
        made = st["sphere_tests"] + st["bound_tests"]
        print("%s: the filtered loops' bound lets %d of %d tests through" % (ps.case_id(param), passed, made))
        assert 0 <= passed <= made, (passed, made)
        _SHARE[param] = (passed, made)
    return data, st


@pytest.mark.parametrize("param", ps.CASES, ids=ps.case_id)
def test_a_posed_frame_is_the_oracles(param):
    c = ps.case(*param)
    w, h, spp = c.shape
    regs = ps.regions(c.shape)
    f32, hooks = c.scene.precision == rta.RT_F32, capi.HAVE_TEST_HOOKS
    ref, rst = ps.frame(param)
    d = rta.DeviceScene(c.scene)
    try:
        data, st = _counted(param, d)
        np.testing.assert_array_equal(util.stitch((w, h), regs, data), ref)
        assert util.all_stats(st) == util.all_stats(rst)
        # every loop flavour, uncounted (the library that ships has its own choice only: flavour 23)
        for v in FLAVOURS:
            if hooks or v == 23:
                with util.loop_flavour(v):
                    plain, _ = d.render_tiles(c.shape, regs, SKIP, want_stats=False)
                assert np.array_equal(plain, data), "loop flavour %d renders different bytes" % v
        if f32:
            # two rays per lane (the sample-packed passes at spp 2 and 4) and one
            before = capi.debug_count(capi.DEBUG_COUNT_TWO_RAY_LAUNCHES) if hooks else None
            for rays in (2, 1):
                with util.control(capi.DEBUG_SKIP_RAYS, rays):
                    got, _ = d.render_tiles(c.shape, regs, SKIP, want_stats=False)
                assert np.array_equal(got, data), "%d ray(s) per lane render different bytes" % rays
            assert before is None or capi.debug_count(capi.DEBUG_COUNT_TWO_RAY_LAUNCHES) >= before + 1
        # the flat scan, whose filter's shadow half is built from the light
        fref, frst = ps.frame(param, oracle.MODE_FLAT)
        flat, fst = d.render_tiles(c.shape, regs, FLAT)
        np.testing.assert_array_equal(util.stitch((w, h), regs, flat), fref)
        assert util.ray_stats(fst) == util.ray_stats(frst)
        if f32 and hooks:
            # pair by pair (every ray x every item of this frame): no candidate rejected, primary or shadow
            k = capi.flat_filter_check(d._h, w, h, spp)
            assert k[2] == 0 and k[5] == 0, k
    finally:
        d.close()


CAMERA_CASES = [p for p in ps.CASES if p[1] in ("+y", "up") and p[2] in ("left", "low_right") and p[3] == "moved" and p[5] == ps.SHAPE]


@pytest.mark.parametrize("param", CAMERA_CASES, ids=ps.case_id)
def test_the_identity_camera_renders_a_posed_frame(param):
    # rt_render_camera from the scene's own eye along +z is the frame: bytes and counters (tests/test_gpu_camera.py holds this at the home pose)
    assert len(CAMERA_CASES) == 2 * 2 * 2 * 2
    c = ps.case(*param)
    w, h, _ = c.shape
    regs = ps.regions(c.shape)
    ref, rst = ps.frame(param)
    d = rta.DeviceScene(c.scene)
    try:
        data, st0 = d.render_tiles(c.shape, regs, SKIP, want_stats=True)
        got, st = d.render_camera(c.shape, identity(c.scene), regs, want_stats=True)
        np.testing.assert_array_equal(util.stitch((w, h), regs, got), ref)
        assert np.array_equal(got, data)
        assert tuple(st[k] for k in COUNTERS) == tuple(st0[k] for k in COUNTERS), (st, st0)
        assert util.all_stats(st) == util.all_stats(rst)
        plain, none = d.render_camera(c.shape, identity(c.scene), regs, want_stats=False)
        assert none is None and np.array_equal(plain, data)
    finally:
        d.close()


UNCOVERED_CASES = [p for p in ps.CASES if p[1] in ("+y", "xyz_tie", "-x") and p[2] == "left" and p[3] in ("id", "moved")]


@pytest.mark.parametrize("param", UNCOVERED_CASES, ids=ps.case_id)
def test_shadow_origins_the_bounds_do_not_cover_fall_back_exactly_under_any_light(param):
    # RT_DEBUG_FILTER_RO_PERCENT = 35 at scene creation: the shadow bounds cover a third of the reach around the centroid m0, most origins
    # lie outside it and get q1 = NaN -- no sure verdict, the reference's arithmetic at every node (tests/test_gpu_parity.py holds this on
    # the default scene under the home light).  The bytes are the oracle's all the same, for one and two rays per lane.
    if not capi.HAVE_TEST_HOOKS:
        pytest.skip("needs a control of csrc/rt_debug.h (RT_DEBUG_FILTER_RO_PERCENT): not in the library that ships")
    assert len(UNCOVERED_CASES) >= 3 * 2 * 2 * 2
    c = ps.case(*param)
    w, h, _ = c.shape
    regs = ps.regions(c.shape)
    ref, rst = ps.frame(param)
    with capi.debug(capi.DEBUG_FILTER_RO_PERCENT, 35):
        d = rta.DeviceScene(c.scene)
    try:
        data, st = d.render_tiles(c.shape, regs, SKIP, want_stats=True)
        np.testing.assert_array_equal(util.stitch((w, h), regs, data), ref)
        assert util.all_stats(st) == util.all_stats(rst)
        for rays in (1, 2):
            with capi.debug(capi.DEBUG_SKIP_RAYS, rays):
                got, _ = d.render_tiles(c.shape, regs, SKIP, want_stats=False)
            assert np.array_equal(got, data), rays
    finally:
        d.close()


@pytest.mark.parametrize("light", list(ps.LIGHTS))
def test_the_filtered_loops_bound_settles_tests_under_every_light(light):
    # Of the tests the reference makes for the f32 frames of one light, the filtered loops' bound lets strictly fewer through: it settles
    # something under every light, not only under the home light it was tuned at.  (A frame test above that has run has left its counts.)
    if not capi.HAVE_TEST_HOOKS:
        pytest.skip("needs a counter of csrc/rt_debug.h (RT_DEBUG_COUNT_FILTER_PASS): not in the library that ships")
    mine = [p for p in ps.CASES if p[1] == light and p[4] == rta.RT_F32]
    assert len(mine) >= 8
    for p in mine:
        if p not in _SHARE:
            d = rta.DeviceScene(ps.case(*p).scene)
            try:
                _counted(p, d)
            finally:
                d.close()
    passed, made = sum(_SHARE[p][0] for p in mine), sum(_SHARE[p][1] for p in mine)
    by_scene = {s: 100.0 * sum(_SHARE[p][0] for p in mine if p[0] == s) / sum(_SHARE[p][1] for p in mine if p[0] == s) for s in ps.SCENES}
    print("FILTER SHARE light %-14s %2d frames: %9d of %9d tests pass the bound = %5.1f %% (nested %5.1f %%, concentric %5.1f %%)"
          % (light, len(mine), passed, made, 100.0 * passed / made, by_scene["nested"], by_scene["concentric"]))
    assert 0 < passed < made, (light, passed, made)
