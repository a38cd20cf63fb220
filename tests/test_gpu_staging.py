"""The host buffers of ONE call in different kinds of memory (csrc/rt_capi_query.hpp, HostStaging): memory from rt_host_alloc is read and
written by the kernels in place, pageable memory -- and a pinned range too small for its row -- goes through the call's workspace, row by
row.  Whatever the mix, rt_near_spheres and rt_overlap_spheres give the bytes of the all-pageable call and leave what lies behind every
output alone.  (Every buffer pinned, every buffer pageable and the refusal of device memory: test_gpu_near.py, test_gpu_overlap.py.)"""
import ctypes as C

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.scenes import random_nested_scene
from tests.test_gpu_near import scene_of
from tests.test_gpu_overlap import PRECISIONS, median_radius, queries_for
from tests.test_gpu_query import REAL

pytestmark = pytest.mark.gpu

N, K = 65, 4                  # one query more than a wave
GUARD, SENTINEL = 128, 0xA5   # bytes behind every output (16 elements of the widest type) and what they hold

ptr = lambda a: None if a is None else a.ctypes.data


def place(src, pinned):
    """The bytes of `src` in memory of one kind: a capi.HostBuffer's (pinned) or numpy's own (pageable)."""
    raw = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
    a = capi.HostBuffer(raw.nbytes).array if pinned else np.empty(raw.nbytes, np.uint8)
    a[:] = raw
    return a


def blank(nbytes, pinned):
    """An output of `nbytes` and its guard, all sentinel."""
    return place(np.full(nbytes + GUARD, SENTINEL, np.uint8), pinned)


def small_scene(precision):
    it, bd, rg = random_nested_scene(3)
    s = scene_of(it, bd, rg, precision)
    queries = queries_for(s, N)
    exclude = (np.arange(N) % len(s.items)).astype(np.int32)
    return s, queries, exclude


def assert_same(got, ref, written, what):
    """Every output: the bytes written are the reference's, and everything behind them -- the guard included -- is untouched."""
    for k, (g, r, w) in enumerate(zip(got, ref, written)):
        np.testing.assert_array_equal(g[:w], r[:w], err_msg=str((what, k)))
        assert (g[w:] == SENTINEL).all(), (what, k)


# (inputs pinned, outputs pinned): all in, none out; the reverse; a mix inside both groups
MIXES = (((True, True, True), (False, False, False)), ((False, False, False), (True, True, True)), ((True, False, True), (False, True, False)))


@PRECISIONS
def test_near_gives_the_same_bytes_whatever_memory_each_buffer_is(precision):
    R = REAL[precision]
    esz = np.dtype(R).itemsize
    s, queries, exclude = small_scene(precision)
    d = rta.DeviceScene(s)
    points = np.ascontiguousarray(queries[:, :3])
    radius = np.full(N, 4.0 * median_radius(s), R)
    sizes = (esz * N * K, 4 * N * K, 4 * N)                                       # gap, item, found

    def run(ins_pinned, outs_pinned):
        ins = [place(x, p) for x, p in zip((points, radius, exclude), ins_pinned)]
        outs = [blank(b, p) for b, p in zip(sizes, outs_pinned)]
        capi.check(capi.lib.rt_near_spheres(d._h, capi.RT_NEAR_ALL, K, ptr(ins[0]), ptr(ins[1]), N, ptr(ins[2]), None, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), None),
                   "rt_near_spheres")
        return outs

    ref = run((False,) * 3, (False,) * 3)
    assert_same(ref, [x.view(np.uint8).reshape(-1) for x in d.near(points, K, radius, all_within=True, exclude=exclude)], sizes, "the wrapper")
    assert ref[2][:sizes[2]].view(np.uint32).max() > 0
    for mix in MIXES:
        assert_same(run(*mix), ref, sizes, mix)
    d.close()


@PRECISIONS
def test_overlaps_give_the_same_bytes_whatever_memory_each_buffer_is(precision):
    R = REAL[precision]
    esz = np.dtype(R).itemsize
    s, queries, exclude = small_scene(precision)
    d = rta.DeviceScene(s)
    margin = 4.0 * median_radius(s)

    def run(ins_pinned, outs_pinned, capacity, room=None):
        """room: the entries each list buffer holds in front of its guard (default: capacity)."""
        room = (capacity, capacity) if room is None else room
        ins = [place(x, p) for x, p in zip((queries, exclude), ins_pinned)]
        outs = [blank(b, p) for b, p in zip((4 * room[0], esz * room[1], 8 * (N + 1)), outs_pinned)]
        total = C.c_uint64(0)
        capi.check(capi.lib.rt_overlap_spheres(d._h, ptr(ins[0]), N, margin, ptr(ins[1]), None, capacity, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), C.byref(total), None),
                   "rt_overlap_spheres")
        return outs, int(total.value)

    total = run((False,) * 2, (False,) * 3, 0)[1]
    assert total > 0                                                              # (the list rows carry something)
    sizes = (4 * total, esz * total, 8 * (N + 1))                                 # items, gap, offsets
    ref, got_total = run((False,) * 2, (False,) * 3, total)
    assert got_total == total
    items, gap, offsets, _ = d.overlaps(queries, margin, exclude=exclude, gaps=True, offsets=True)
    assert_same(ref, [x.view(np.uint8).reshape(-1) for x in (items, gap, offsets)], sizes, "the wrapper")
    for ins_pinned, outs_pinned in MIXES:
        got, got_total = run(ins_pinned[:2], outs_pinned, total)
        assert got_total == total
        assert_same(got, ref, sizes, (ins_pinned[:2], outs_pinned))
    # every buffer pinned, and one list buffer one entry short of `capacity` entries: that row alone is staged, and the `total` entries it
    # gets still fit in front of its guard.  (Only a list row can be short: any other row is written whole, past the end of such a buffer.)
    for short in (0, 1):
        unit = (4, esz)[short]
        capacity = total + GUARD // unit + 1
        room = [capacity, capacity]
        room[short] = total
        assert unit * room[short] + GUARD == unit * capacity - unit
        got, got_total = run((True, True), (True, True, True), capacity, room)
        assert got_total == total
        assert_same(got, ref, sizes, ("short", short))
    d.close()
