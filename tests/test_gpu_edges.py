"""The kernels on the edge-case scenes of tests/edge_scenes.py: nodes tuned to within a few ulps of where the reference's own verdict flips
for one target sample ray, so that every conservative bound of the walk (the primary threshold and its cut-off, the root-free BOUND decision,
the two-sided shadow bounds, the f64 walk's f32 filter, the fused streams' own-sphere bounds) is asked at its edge.  The counting launches
hold each bound's verdict against the exact test (FILTER_VIOLATIONS, asserted 0 by tests/conftest.py); the launches without counters (the
generated assembly loops) are compared with the oracle pixel for pixel."""
import functools
import os

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from tests import edge_scenes as es
from tests import util
from tests.test_gpu_query import check_nearest

pytestmark = pytest.mark.gpu

HIER_EXIT = oracle.MODE_HIERARCHY | oracle.MODE_ANYHIT_EXIT
SKIP, FLAT = rta.RT_TRAVERSAL_SKIP, rta.RT_TRAVERSAL_FLAT
RT_PREC = {oracle.F32: rta.RT_F32, oracle.F64: rta.RT_F64}
PREC_IDS = {oracle.F32: "f32", oracle.F64: "f64"}
THREADS = max(1, min(16, os.cpu_count() or 1))


@functools.lru_cache(maxsize=None)
def _pair(family, prec, spp):
    sc = es.scene(family, prec, spp)
    s, o = util.scene_pair_ranges(sc.items, sc.bounds, sc.ranges, RT_PREC[prec], light=sc.light, eye=sc.eye)
    return sc, s, o


@functools.lru_cache(maxsize=None)
def _ref(family, prec, spp, mode=HIER_EXIT):
    sc, _, o = _pair(family, prec, spp)
    ref, rst, _ = o.render(sc.w, sc.h, spp, THREADS, mode)
    return ref, rst


def _opts(sc, spp):
    return (sc.w, sc.h, spp), [tuple(r) for r in rta.buckets(rta.RenderOptions(sc.w, sc.h, spp))]


@pytest.mark.parametrize("spp", es.SPPS)
@pytest.mark.parametrize("prec", es.PRECS, ids=PREC_IDS.get)
@pytest.mark.parametrize("family", es.FAMILIES)
def test_counting_launch_matches_the_oracle(family, prec, spp):
    # bytes and every counter; the autouse fixture re-renders without counters, with every quad cooperative and with the lean / generic
    # kernels swapped, and asserts that no bound ruled out a test that returned a finite distance
    sc, s, o = _pair(family, prec, spp)
    opts, regs = _opts(sc, spp)
    data, st = s.device().render_tiles(opts, regs, SKIP, want_stats=True)
    ref, rst = _ref(family, prec, spp)
    np.testing.assert_array_equal(util.stitch(opts, regs, data), ref)
    assert util.all_stats(st) == util.all_stats(rst)
    assert rst["hits"] >= len(sc.cases) // 2
    # the O scenes are built fused (every bound followed by an item with its centre): the library must see it, or flavours 7 / 23 on them
    # would quietly walk the plain streams
    assert bool(s.device().traits() & rta.capi.RT_SCENE_CONCENTRIC) == (family == "O")


@pytest.mark.parametrize("variant", [0, 1, 3, 7, 19, 23])
@pytest.mark.parametrize("prec", es.PRECS, ids=PREC_IDS.get)
@pytest.mark.parametrize("family", es.FAMILIES)
def test_every_loop_flavour_matches_the_oracle(family, prec, variant):
    # 0 / 1: the C++ loops, 3: the generated assembly loops, 7: fused (the O scenes), 19 / 23: the filtered loops, plain and fused
    for spp in es.SPPS:
        sc, s, o = _pair(family, prec, spp)
        opts, regs = _opts(sc, spp)
        ref, rst = _ref(family, prec, spp)
        with util.loop_flavour(variant):
            plain, _ = s.device().render_tiles(opts, regs, SKIP, want_stats=False)
            counted, st = s.device().render_tiles(opts, regs, SKIP, want_stats=True)
        np.testing.assert_array_equal(util.stitch(opts, regs, plain), ref, err_msg=sc.name)
        np.testing.assert_array_equal(counted, plain)
        assert util.all_stats(st) == util.all_stats(rst), sc.name


@pytest.mark.parametrize("prec", es.PRECS, ids=PREC_IDS.get)
@pytest.mark.parametrize("family", es.FAMILIES)
def test_two_rays_per_lane_walk_matches_the_oracle(family, prec):
    # k_render_skip2 and its lean twin (one-sample, sample-split and sample-packed passes), forced where the library would not pick them
    for spp in es.SPPS:
        sc, s, o = _pair(family, prec, spp)
        opts, regs = _opts(sc, spp)
        ref, _ = _ref(family, prec, spp)
        with util.control(rta.capi.DEBUG_SKIP_RAYS, 2):
            two, _ = s.device().render_tiles(opts, regs, SKIP, want_stats=False)
        np.testing.assert_array_equal(util.stitch(opts, regs, two), ref, err_msg=sc.name)


@pytest.mark.parametrize("prec", es.PRECS, ids=PREC_IDS.get)
@pytest.mark.parametrize("family", es.FAMILIES)
def test_flat_scan_matches_the_oracle(family, prec):
    for spp in es.SPPS:
        sc, s, o = _pair(family, prec, spp)
        opts, regs = _opts(sc, spp)
        flat, fst = s.device().render_tiles(opts, regs, FLAT)
        fref, frst = _ref(family, prec, spp, oracle.MODE_FLAT)
        np.testing.assert_array_equal(util.stitch(opts, regs, flat), fref, err_msg=sc.name)
        assert util.ray_stats(fst) == util.ray_stats(frst), sc.name
        if rta.capi.HAVE_TEST_HOOKS:
            # the flat scan's conservative filter, pair by pair: no candidate that the reference hits rejected
            c = rta.capi.flat_filter_check(s.device()._h, sc.w, sc.h, spp)
            assert c[2] == 0 and c[5] == 0, (sc.name, c)


@pytest.mark.parametrize("prec", es.PRECS, ids=PREC_IDS.get)
@pytest.mark.parametrize("family", ["P1", "P1c", "S1"])
def test_queries_of_the_grazing_rays(family, prec):
    # the target rays (primary sample rays, shadow rays) as ray queries of their scene: tmax = +inf, = the oracle's distance (the strict `<`
    # keeps it out) and one ulp either side, nearest and any-hit, bit for bit with the oracle
    R = es.REAL[prec]
    for spp in es.SPPS:
        sc, s, o = _pair(family, prec, spp)
        rays = np.array([c.ray for c in sc.cases]).astype(R)
        near = np.array([o.intersect(r.astype(np.float64))[0] for r in rays]).astype(R)
        fin = np.isfinite(near)
        tm = [np.full(len(rays), np.inf, dtype=R), near[fin], np.nextafter(near[fin], R(np.inf)), np.nextafter(near[fin], R(0))]
        rr = [rays, rays[fin], rays[fin], rays[fin]]
        rays_all, tmax = np.concatenate(rr), np.concatenate(tm).astype(R)
        assert fin.sum() >= len(rays) // 4, sc.name
        ref_d, _ = check_nearest(s, o, rays_all, tmax)
        ad, an, ai = s.device().intersect(rays_all, tmax, any_hit=True)
        found = ai >= 0
        np.testing.assert_array_equal(found, ref_d.astype(np.float64) < tmax.astype(np.float64), err_msg=sc.name)
        np.testing.assert_array_equal(found, ad.astype(np.float64) < tmax.astype(np.float64), err_msg=sc.name)
