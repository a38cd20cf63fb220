"""Dispatch orders built from costs counted on the streams a list's frames walk (rust-tracer_amd/csrc/rt_capi_dispatch.hpp build_orders,
tight_cost_map_of; NOTES.md T): a list whose launches walk the scene's tight streams gets its cost map, its exact recount and its
orders from a counting launch over those streams, and its launches say `tight_costs` beside `tight_bounds`; every other list keeps the
given-stream costs.  Whatever the orders are made from, a frame is the oracle's byte for byte, and a counting launch returns the
given-stream counters.  With every control at its default the scene's worker swaps the tight set in under the caller's launches, its
recount counted as one that walked the tight streams.  The 256 x 256 map of either source (rt_debug_cost_map) is held against the reference's own count of tests over the
same bounds."""
import functools
import os
import threading

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests import posed_scenes as ps
from tests import tight_scenes as ts
from tests import util

pytestmark = pytest.mark.gpu

HIER_EXIT = oracle.MODE_HIERARCHY | oracle.MODE_ANYHIT_EXIT
SKIP = rta.RT_TRAVERSAL_SKIP
THREADS = max(1, min(16, os.cpu_count() or 1))
F32 = rta.RT_F32
POSES = {"home": ("nested", "home", "home", "id"), "moved": ("nested", "home", "home", "moved")}
SHAPES = ((128, 128, 1), (200, 136, 1))                   # whole blocks; a ragged frame (200 = 12.5 blocks, 136 = 8.5)
COOP_THR = 8                                              # tests per pixel: low enough for cooperative quads at these sizes
MAP_RES = 256


def _case(pose, shape=SHAPES[0]):
    return ps.case(*POSES[pose], F32, shape)


@functools.lru_cache(maxsize=None)
def _ref(pose, shape):
    img, st, _ = _case(pose, shape).oracle.render(shape[0], shape[1], shape[2], THREADS, HIER_EXIT)
    img.setflags(write=False)
    return img, dict(st)


def _controls(fast, coop):
    c = [(capi.DEBUG_FAST_KERNEL, fast)]
    return c + ([(capi.DEBUG_COOP, 1), (capi.DEBUG_COOP_THR, COOP_THR)] if coop else [(capi.DEBUG_COOP, 0)])


def _launch(d, shape, regs, controls, tb):
    """One uncounted launch, its list's orders built in the foreground, under `controls` and RT_DEBUG_TIGHT_BOUNDS tb (None: the default)
    -> (frame, flags)."""
    capi.debug_set(capi.DEBUG_ASYNC_ORDERS, 0)
    for key, value in controls:
        capi.debug_set(key, value)
    if tb is not None:
        capi.debug_set(capi.DEBUG_TIGHT_BOUNDS, tb)
    try:
        data, _ = d.render_tiles(shape, regs, SKIP, want_stats=False)
        flags = capi.last_launch()
    finally:
        for key, _ in controls:
            capi.debug_set(key, -1)
        capi.debug_set(capi.DEBUG_TIGHT_BOUNDS, -1)
    return util.stitch(shape, regs, data), flags


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("pose", sorted(POSES))
def test_frames_and_flags_whatever_the_orders_are_made_from(pose, shape):
    c = _case(pose, shape)
    _, tight, consts = ts.tight_of(c.scene)
    assert consts["rule"] == 1 and tight.any()
    ref = _ref(pose, shape)[0]
    regs = ps.regions(shape)
    d = rta.DeviceScene(c.scene)
    try:
        for fast in (0, 2):
            for coop in (False, True):
                for tb in (0, 2):
                    for k in range(2):
                        frame, flags = _launch(d, shape, regs, _controls(fast, coop), tb)
                        np.testing.assert_array_equal(frame, ref, err_msg="fast %d coop %d tight %d launch %d" % (fast, coop, tb, k))
                        assert "ordered" in flags, (fast, coop, tb, k, flags)
                        assert ("fast_kernel" in flags) == (fast == 2), (fast, coop, tb, k, flags)
                        if tb == 0:
                            assert not flags & {"tight_bounds", "tight_costs"}, (fast, coop, k, flags)
                        elif k == 1:
                            assert flags >= {"tight_bounds", "tight_costs"}, (fast, coop, flags)
                    if coop and tb == 2:
                        assert "cooperative" in flags, (fast, flags)      # (quads exist at this size: the orders really had holes)
    finally:
        d.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_a_rule_two_scene_keeps_the_given_costs_at_these_sizes(shape):
    param = ("concentric", "home", "home", "id", F32, shape)
    c = ps.case(*param)
    assert ts.tight_of(c.scene)[2]["rule"] == 2
    ref = c.oracle.render(shape[0], shape[1], 1, THREADS, HIER_EXIT)[0]
    regs = ps.regions(shape)
    d = rta.DeviceScene(c.scene)
    try:
        for fast in (0, 2):
            for k in range(2):
                frame, flags = _launch(d, shape, regs, _controls(fast, False), None)
                np.testing.assert_array_equal(frame, ref, err_msg="fast %d launch %d" % (fast, k))
                assert "ordered" in flags and not flags & {"tight_bounds", "tight_costs"}, (fast, k, flags)
    finally:
        d.close()


@pytest.mark.parametrize("pose", sorted(POSES))
def test_a_counting_launch_keeps_the_given_stream_counters(pose):
    shape = SHAPES[1]
    c = _case(pose, shape)
    ts.tight_of(c.scene)                                      # (needs a control: the library that ships skips here)
    ref, rst = _ref(pose, shape)
    regs = ps.regions(shape)
    d = rta.DeviceScene(c.scene)
    try:
        capi.debug_set(capi.DEBUG_ASYNC_ORDERS, 0)
        for when in ("before", "after"):
            data, st = d.render_tiles(shape, regs, SKIP, want_stats=True)
            np.testing.assert_array_equal(util.stitch(shape, regs, data), ref, err_msg=when)
            assert util.all_stats(st) == util.all_stats(rst), when
            assert capi.debug_count(capi.DEBUG_COUNT_TIGHT_VIOLATIONS) == 0, when
            if when == "before":                              # the tight orders arrive
                for k in range(2):
                    frame, flags = _launch(d, shape, regs, _controls(2, False), 2)
                    np.testing.assert_array_equal(frame, ref)
                assert flags >= {"tight_bounds", "tight_costs"}, flags
    finally:
        d.close()


# ---- the path the product runs: orders from the scene's worker, the tight set swapped in under launches --------------------------------

MAX_LAUNCHES = 5000                                       # (the worker needs a few milliseconds; a launch and its read-back take 0.1 - 0.2)


@pytest.mark.parametrize("pose", sorted(POSES))
def test_the_worker_swaps_the_tight_orders_in_under_launches(pose):
    shape = SHAPES[1]
    c = _case(pose, shape)
    ts.tight_of(c.scene)                                      # (needs a control: the library that ships skips here)
    ref = _ref(pose, shape)[0]
    regs = ps.regions(shape)
    d0 = rta.DeviceScene(c.scene)
    try:
        shards = capi.shard_costs(d0._h, shape, regs, 2)      # (a scene whose worker has done nothing: the call makes the tight streams itself)
    finally:
        d0.close()
    d = rta.DeviceScene(c.scene)
    recounts = capi.debug_count(capi.DEBUG_COUNT_TIGHT_RECOUNTS)
    try:
        capi.debug_set(capi.DEBUG_ASYNC_ORDERS, -1)           # every control at its default: the list goes to the scene's worker
        seen, arrived = [], None
        for k in range(MAX_LAUNCHES):
            data, _ = d.render_tiles(shape, regs, SKIP, want_stats=False)
            flags = capi.last_launch()
            np.testing.assert_array_equal(util.stitch(shape, regs, data), ref, err_msg="launch %d %r" % (k, sorted(flags)))
            if not seen or seen[-1] != flags:
                seen.append(flags)
            if arrived is None and "tight_costs" in flags:
                arrived = k
            if arrived is not None and k >= arrived + 40:     # (the second trial: seven candidates, three samples each, and past it)
                break
        print("TIGHT ORDERS %-6s arrived at launch %s; flags seen: %s" % (pose, arrived, [sorted(f) for f in seen]))
        assert arrived is not None, seen
        assert flags >= {"ordered", "tight_bounds", "tight_costs"}, flags
        # once the tight set is in, no launch goes back to the first one
        first = next(i for i, f in enumerate(seen) if "tight_costs" in f)
        assert all("tight_costs" in f for f in seen[first:]), seen
        # the list's exact recount walked the tight streams (and nothing but that second pass did)
        assert capi.debug_count(capi.DEBUG_COUNT_TIGHT_RECOUNTS) == recounts + 1
        # the shards' costs follow the source of the list they describe, whenever they are asked for
        np.testing.assert_array_equal(capi.shard_costs(d._h, shape, regs, 2), shards)
    finally:
        capi.debug_set(capi.DEBUG_ASYNC_ORDERS, 0)
        d.close()


# ---- the map of either source against the reference's arithmetic ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_map_sums(pose):
    """(given, tight): sphere_tests + bound_tests of the reference over a 256 x 256 one-sample frame, with the scene's given bounds and with
    the spheres of the tight streams put in where a bound is tight; and whether the eye is outside every one of those bounds."""
    c = _case(pose)
    spheres, tight, _ = ts.tight_of(c.scene)
    given = np.asarray(c.bounds, dtype=np.float64)
    mixed = given.copy()
    mixed[tight != 0] = spheres[tight != 0].astype(np.float64)
    light = ps.LIGHTS[POSES[pose][1]]
    sums = []
    for b in (given, mixed):
        st = oracle.Scene.from_ranges(c.items, b, c.ranges, light, c.eye, oracle.F32).render(MAP_RES, MAP_RES, 1, THREADS, HIER_EXIT)[1]
        sums.append(int(st["sphere_tests"]) + int(st["bound_tests"]))
    outside = all(ts.eye_outside(b, c.eye) for b in np.concatenate([given.astype(np.float32), mixed.astype(np.float32)]))
    return sums[0], sums[1], outside


def _map_fixtures():
    """The poses whose two reference sums differ (one whose sums were equal would tell the sources apart by nothing)."""
    return [p for p in sorted(POSES) if _oracle_map_sums(p)[0] != _oracle_map_sums(p)[1]]


def test_the_cost_maps_are_the_references_counts():
    fixtures = _map_fixtures()
    assert fixtures, "no fixture tells the two cost sources apart"
    for pose in fixtures:
        given, tight, outside = _oracle_map_sums(pose)
        assert outside, pose                                   # (the eye inside a bound: its tests are counted another way)
        assert tight < given, (pose, tight, given)
        d = rta.DeviceScene(_case(pose).scene)
        try:
            h = d._h
            got_tight = capi.cost_map(h, True)
            got_given = capi.cost_map(h, False)
            print("COST MAP %-6s given %d (reference %d)  tight %d (reference %d)" % (pose, int(got_given.sum(dtype=np.uint64)), given,
                                                                                      int(got_tight.sum(dtype=np.uint64)), tight))
            assert int(got_given.sum(dtype=np.uint64)) == given, pose
            assert int(got_tight.sum(dtype=np.uint64)) == tight, pose
        finally:
            d.close()


# ---- each map is made once, whoever asks, in whatever order ------------------------------------------------------------------------------

# (the default pyramid of 85 spheres under 21 bounds, and the one of 341 under 85: rule 1 holds for both)
@pytest.mark.parametrize("level, n_items", [(4, 85), (5, 341)])
def test_each_cost_map_is_the_same_every_time_it_is_fetched(level, n_items):
    scene = rta.Scene.default(level=level)
    assert len(scene.items) == n_items
    assert ts.tight_of(scene)[2]["rule"] == 1
    d = rta.DeviceScene(scene)
    try:
        first = {t: capi.cost_map(d._h, t) for t in (False, True)}
        assert first[True].sum(dtype=np.uint64) < first[False].sum(dtype=np.uint64)
        for t in (True, False, False, True):
            np.testing.assert_array_equal(capi.cost_map(d._h, t), first[t])
        # a list's foreground order build reads the maps too: still the same behind it
        shape = (128, 128, 1)
        _launch(d, shape, ps.regions(shape), _controls(2, False), 2)
        for t in (False, True):
            np.testing.assert_array_equal(capi.cost_map(d._h, t), first[t])
    finally:
        d.close()
    # two threads at once on a scene nobody has asked yet, one source first each
    d = rta.DeviceScene(scene)
    try:
        got, errors = {}, []
        go = threading.Barrier(2)

        def fetch(order):
            try:
                go.wait()
                for t in order:
                    got[(order[0], t)] = capi.cost_map(d._h, t)
            except Exception as e:      # noqa: BLE001  (reported below, on the test's own thread)
                errors.append(e)
        threads = [threading.Thread(target=fetch, args=(order,)) for order in ((True, False), (False, True))]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for (_, t), m in got.items():
            np.testing.assert_array_equal(m, first[t])
    finally:
        d.close()
