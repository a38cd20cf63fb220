"""First contacts on the GPU (rt_first_contacts / rt_first_contacts_device, csrc/rt_first.hpp) away from unit scale and
away from the origin: the placements of tests/scaled_scenes.py, 80 queries (one full wave and a partly filled one) over scenes of 80 to
120 items.  Per placement: time bits, item, normal bits and every counter against FirstWalker; the GPU's own links between
first_contacts and swept_overlaps; the GPU's NEAREST result against the geometry in higher precision
(tests/test_scales_first_host.py hold_to_geometry: the comparison with a reference that the package did not write); and exact scalings
by powers of two, which change no byte.  tests/test_scales_first_host.py makes the same statements about the walker without a GPU."""
import numpy as np
import pytest

import rust_tracer_amd as rta
from tests import scaled_scenes as ss
from tests.test_gpu_first import FirstWalker, assert_first, check_links, rows_of
from tests.test_gpu_impacts import FAMILIES
from tests.test_gpu_near import same_bytes, scene_of
from tests.test_gpu_query import REAL
from tests.test_gpu_swept import POW2_CASES, pow2_inputs
from tests.test_scales_contact_host import higher
from tests.test_scales_first_host import all_scenes, enclosing_scenes, hold_to_geometry, motions

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)


@CASES
def test_the_result_of_a_placed_scene_restates_the_walk_bit_for_bit(param):
    """assert_first (time bits, item, normal bits, all counters) against FirstWalker, NEAREST and ANY: the nested scenes as made, their
    refit twins and the scenes without bounds, both families, the scene moving and standing; the first combination of every scene goes
    through the device entry with tensors too.  Every combination has results and empty queries.  (The walker forms its tm / nm matrices
    again for the ANY walk: at 80 queries over at most 160 nodes that is numpy's work of a millisecond, next to the walk in Python.)"""
    import torch
    precision, placement = param
    for name, c, s in all_scenes(ss.case(precision, placement)):
        d = rta.DeviceScene(s)
        w = FirstWalker(s)
        for k, (family, moving, queries, qdisp, disp) in enumerate(motions(c)):
            for any_hit in (False, True):
                what = (ss.case_id(param), name, family, "moving" if moving else "standing", "any" if any_hit else "nearest")
                _, item, _, st = assert_first(d, w, queries, qdisp, disp, what, any_hit)
                assert (item >= 0).any() and (item < 0).any() and st["tests_executed"] > 0, what
                if k == 0:
                    dev = [None if x is None else torch.from_numpy(x.copy()).cuda() for x in (queries, qdisp, disp)]
                    assert_first(d, w, queries, qdisp, disp, what + ("device",), any_hit, args=(*dev, None))
        d.close()


@CASES
def test_the_result_of_a_placed_scene_is_the_smallest_time_of_its_swept_row(param):
    """The GPU's own links, with no walker: check_links of first_contacts (NEAREST and ANY) against the rows of swept_overlaps on the same
    inputs, and tests_executed ordered any <= nearest <= list, for every scene, family and motion of the placement."""
    precision, placement = param
    R = REAL[precision]
    for name, c, s in all_scenes(ss.case(precision, placement)):
        d = rta.DeviceScene(s)
        for family, moving, queries, qdisp, disp in motions(c):
            what = (ss.case_id(param), name, family, "moving" if moving else "standing")
            rows, list_st = rows_of(d, queries, qdisp, disp)
            time, item, normal, st = d.first_contacts(queries, qdisp, disp, normals=True, stats=True)
            a_time, a_item, a_st = d.first_contacts(queries, qdisp, disp, any_hit=True, stats=True)
            check_links(rows, time, item, normal, a_time, a_item, R, what)
            assert a_st["tests_executed"] <= st["tests_executed"] <= list_st["tests_executed"], (what, a_st, st, list_st)
        d.close()


@CASES
def test_the_result_of_a_placed_scene_is_the_earliest_touch_of_the_geometry(param):
    """hold_to_geometry of tests/test_scales_first_host.py on the GPU's NEAREST result: the refit twins and the scenes without bounds (their
    bounds enclose, so the result is the scene's), both families, the scene moving and standing.  The classes, the 5 % cap on undecided
    queries and the messages are that function's."""
    precision, placement = param
    higher(precision)
    for name, c, s in enclosing_scenes(ss.case(precision, placement)):
        d = rta.DeviceScene(s)
        for family, moving, queries, qdisp, disp in motions(c):
            what = (ss.case_id(param), name, family, "moving" if moving else "standing", "gpu")
            time, item = d.first_contacts(queries, qdisp, disp)
            k = hold_to_geometry(time, item, queries, qdisp, s.items, disp, precision, what)
            print("%s: %d of %d decided, %d with a result" % (what, k, len(queries), (item >= 0).sum()))
        d.close()


@pytest.mark.parametrize("precision,k", POW2_CASES, ids=["%s-2^%d" % ("f32" if p == rta.RT_F32 else "f64", k) for p, k in POW2_CASES])
def test_a_power_of_two_scaling_changes_no_byte_of_the_result(precision, k):
    R = REAL[precision]
    for index in (0, 2):                                                         # nested, and the same items without bounds
        for family in FAMILIES:
            for any_hit in (False, True):
                results = []
                for factor in (0, k):
                    items, bounds, ranges, queries, qdisp, disp = pow2_inputs(index, family, factor, R)
                    s = scene_of(items, bounds, ranges, precision)
                    d = rta.DeviceScene(s)
                    results.append(assert_first(d, FirstWalker(s), queries, qdisp, disp, (index, family, factor, any_hit), any_hit))
                    d.close()
                assert (results[0][1] >= 0).any() and (results[0][1] < 0).any()
                # time bits, item, normal bits.  (Not the counters: a displacement shorter than the square root of refit_tiny takes its length
                # from the L1 rule, so a bound's D -- never an item's time -- depends on the scale, and each walk matches its own walker.)
                same_bytes(results[0][:3], results[1][:3])
