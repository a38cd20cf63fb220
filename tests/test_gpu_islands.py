"""Contact islands on the GPU (rt_scene_islands / rt_scene_impact_islands and their _device entries, csrc/rt_islands.hpp):
the labels, indices, sizes and the island count against rta.pair_islands -- the definition in numpy -- over the pairs of the contacts
and impacts tests' walkers, and the counters against the pair entries' counting pass.  Every comparison is exact: the labels are integers,
and the edge set is defined bit for bit by the pair walks."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.scenes import random_nested_scene
from tests.test_gpu_contacts import COUNTERS, Walker, clump, median_radius
from tests.test_gpu_impacts import Walker as ImpactWalker, displacements, scenes as impact_scenes
from tests.test_gpu_near import LIGHT, EYE, cases, same_bytes, scene_of
from tests.test_gpu_query import REAL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
WALK_SCENES = ("default_L3", "nested", "refit", "nested3", "clump")
# what the margins are multiples of: the median radius
MARGINS = (0.0, 1.0, -0.25, 2.0, 4.0, np.inf, -np.inf)
# the refit scene's component structure, (islands, largest island) per margin in median radii -- worked out on the CPU in f64 from the
# walker's pairs (f32 gives the same): singletons, many mid-sized islands, a giant component, one island
REFIT_STRUCTURE = {0.0: (218, 8), 1.0: (117, 26), 2.0: (23, 265), 4.0: (1, 300)}
counters = lambda st: {c: st[c] for c in COUNTERS}


def walk_scene(name, precision):
    if name == "nested3":
        return scene_of(*random_nested_scene(3), precision)
    if name == "clump":
        return clump(precision)[0]
    return cases(precision)[name]


@functools.lru_cache(maxsize=None)
def walk_reference(name, precision):
    """(Scene, [(margin, pair_islands of the walker's pairs, the walker's counters)]), made once."""
    s = walk_scene(name, precision)
    w = Walker(s)
    r = median_radius(s)
    out = []
    for k in MARGINS:
        margin = k * r if np.isfinite(k) else k
        pairs, _, _, st = w.all(margin)
        out.append((k, margin, rta.pair_islands(pairs, len(s.items), w.live), st))
    return s, out


def assert_islands(got, ref, what):
    """got: (label, index, size, n_islands) of the library, numpy or torch; ref: pair_islands'."""
    label, index, size = [x.cpu().numpy() if hasattr(x, "cpu") else x for x in got[:3]]
    n_islands = int(got[3])
    assert label.dtype == np.int32 and index.dtype == np.int32 and size.dtype == np.uint32, what
    np.testing.assert_array_equal(label, ref[0], err_msg=str(what))
    np.testing.assert_array_equal(index, ref[1], err_msg=str(what))
    np.testing.assert_array_equal(size, ref[2], err_msg=str(what))
    assert n_islands == ref[3] == int((label == np.arange(len(label))).sum()), what


@PRECISIONS
@pytest.mark.parametrize("name", WALK_SCENES)
def test_the_islands_are_the_components_of_the_walks_pairs(name, precision):
    s, refs = walk_reference(name, precision)
    n = len(s.items)
    d = rta.DeviceScene(s)
    for k, margin, ref, ref_st in refs:
        what = (name, k)
        got = d.islands(margin, index=True, sizes=True, stats=True)
        assert_islands(got, ref, what)
        # the counters: the walker's, and the counting pass's of contacts() for the same margin -- the same walk, test for test
        assert counters(got[4]) == ref_st, what
        assert counters(got[4]) == counters(d.contacts(margin, capacity=0, stats=True)[2]), what
        label, index, size, n_islands = got[:4]
        if k == np.inf:
            assert n_islands == 1 and not label.any() and (size == n).all(), what                # every slot is live here: slot 0 is the lowest
        if k == -np.inf:
            assert n_islands == n and (label == np.arange(n)).all() and (size == 1).all() and (index == np.arange(n)).all(), what
        if name == "refit" and k in REFIT_STRUCTURE:
            assert (n_islands, int(size.max())) == REFIT_STRUCTURE[k], what
        if name == "clump" and k == 0.0:
            assert int(size.max()) == 41 and n_islands == 61, what                                # 40 lanes hook one root
    d.close()


# ---- chains: what goes wrong when a union is lost or a find reads a stale parent ----

CHAIN = 600


def block_threads():
    text = open(os.path.join(ROOT, "rust-tracer_amd", "csrc", "rt_kernels.hpp")).read()
    return int(re.search(r"constexpr int kBlockThreads = (\d+);", text).group(1))


def chain(R, n=CHAIN, y=0.0):
    """n spheres of radius 0.5 spaced 0.9 apart on a line: neighbours overlap by 0.1, everything else is 0.8 or more apart."""
    sp = np.zeros((n, 4), R)
    sp[:, 0] = np.arange(n) * 0.9
    sp[:, 1] = y
    sp[:, 3] = 0.5
    return sp


def chain_pairs(slot_of):
    """The edges of a chain whose k-th sphere sits in slot slot_of[k], as the library lists them: (lower slot, higher slot), sorted."""
    a, b = slot_of[:-1], slot_of[1:]
    p = np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1)
    return p[np.lexsort((p[:, 1], p[:, 0]))].astype(np.int32)


def flat_scene(items, precision):
    return rta.Scene(items, rta.normalized(LIGHT, precision), EYE, precision=precision)


@PRECISIONS
def test_a_chain_scattered_over_the_workgroups_is_one_island(precision):
    R = REAL[precision]
    assert CHAIN > 2 * block_threads()                                           # several workgroups: a chain's neighbours meet across them
    # (a) a flat scene, the slots a fixed random permutation of the chain: neighbours sit in different waves and workgroups
    slot_of = np.random.default_rng(600).permutation(CHAIN)
    items = np.zeros((CHAIN, 4), R)
    items[slot_of] = chain(R)
    d = rta.DeviceScene(flat_scene(items, precision))
    edges = chain_pairs(slot_of)
    np.testing.assert_array_equal(d.contacts(0.0)[0], edges)                     # (the reference is the edge set the library itself lists)
    got = d.islands(0.0, index=True, sizes=True)
    assert_islands(got, rta.pair_islands(edges, CHAIN), "scattered")
    assert got[3] == 1 and not got[0].any() and not got[1].any() and (got[2] == CHAIN).all()
    d.close()
    # (b) Morton order under balanced ranges with refit bounds
    sp = chain(R)
    sp = sp[np.argsort(rta.sphere_keys(sp), kind="stable")]
    rg = rta.balanced_ranges(CHAIN, 4)
    d = rta.DeviceScene(scene_of(sp, rta.refit_bounds(sp, rg, precision), rg, precision))
    pairs = d.contacts(0.0)[0]
    assert len(pairs) == CHAIN - 1
    got = d.islands(0.0, index=True, sizes=True)
    assert_islands(got, rta.pair_islands(pairs, CHAIN), "morton")
    assert got[3] == 1 and not got[0].any() and (got[2] == CHAIN).all()
    d.close()


@PRECISIONS
def test_two_interleaved_chains_are_two_islands_with_their_own_minima(precision):
    R = REAL[precision]
    # (c) two chains 5 apart, interleaved by one permutation of all their spheres
    slot_of = np.random.default_rng(1200).permutation(2 * CHAIN)
    items = np.zeros((2 * CHAIN, 4), R)
    items[slot_of] = np.concatenate([chain(R), chain(R, y=5.0)])
    d = rta.DeviceScene(flat_scene(items, precision))
    edges = np.concatenate([chain_pairs(slot_of[:CHAIN]), chain_pairs(slot_of[CHAIN:])])
    edges = edges[np.lexsort((edges[:, 1], edges[:, 0]))]
    np.testing.assert_array_equal(d.contacts(0.0)[0], edges)
    label, index, size, n_islands = got = d.islands(0.0, index=True, sizes=True)
    assert_islands(got, rta.pair_islands(edges, 2 * CHAIN), "two chains")
    lows = sorted((int(slot_of[:CHAIN].min()), int(slot_of[CHAIN:].min())))
    assert n_islands == 2 and sorted(set(label.tolist())) == lows and lows[0] == 0 and (size == CHAIN).all()
    assert (label[slot_of[:CHAIN]] == slot_of[:CHAIN].min()).all() and (label[slot_of[CHAIN:]] == slot_of[CHAIN:].min()).all()
    assert set(index.tolist()) == {0, 1}
    d.close()


# ---- dead slots ----

@PRECISIONS
def test_a_dead_sphere_bridges_nothing(precision):
    R = REAL[precision]
    sp = chain(R)                                                                # (in chain order: Morton order along a line)
    d = rta.DeviceScene(rta.Scene.from_spheres_balanced(sp, leaf_size=4, precision=precision), 0, True)
    items = np.asarray(d.scene.items, R)
    np.testing.assert_array_equal(items, sp)
    assert d.islands(0.0)[1] == 1
    live = np.ones(CHAIN, np.uint8)
    dead = CHAIN // 2
    live[dead] = 0
    garbage = items.copy()
    garbage[dead] = np.nan                                                       # a dead slot may hold any bits
    d.update(garbage, live=live)
    np.testing.assert_array_equal(d.live(), live)
    label, index, size, n_islands = got = d.islands(0.0, index=True, sizes=True)
    assert_islands(got, rta.pair_islands(d.contacts(0.0)[0], CHAIN, live), "killed")
    assert n_islands == 2 and (label[dead], index[dead], size[dead]) == (-1, -1, 0)
    assert (label[:dead] == 0).all() and (label[dead + 1:] == dead + 1).all()
    assert (size[:dead] == dead).all() and (size[dead + 1:] == CHAIN - dead - 1).all()
    assert (index[:dead] == 0).all() and (index[dead + 1:] == 1).all()
    # ... and at +inf the island of the live slots leaves it out
    label, size, n_islands = d.islands(np.inf, sizes=True)
    assert n_islands == 1 and label[dead] == -1 and size[dead] == 0 and (np.delete(label, dead) == 0).all() and (np.delete(size, dead) == CHAIN - 1).all()
    # a rebuild of fewer spheres than the capacity: the slots behind them are dead
    some = 400
    scattered = sp[np.random.default_rng(9).permutation(CHAIN)]
    order = d.rebuild(scattered, n=some)
    now = scattered[:some][order]                                                # slot k holds now[k]
    place = np.rint(now[:, 0].astype(np.float64) / 0.9).astype(np.int64)         # its place in the chain
    by_place = np.full(CHAIN + 1, -1, np.int64)
    by_place[place] = np.arange(some)
    k = np.flatnonzero((by_place[:-1] >= 0) & (by_place[1:] >= 0))               # both neighbours are there
    edges = np.stack([np.minimum(by_place[k], by_place[k + 1]), np.maximum(by_place[k], by_place[k + 1])], axis=1)
    edges = edges[np.lexsort((edges[:, 1], edges[:, 0]))].astype(np.int32)
    np.testing.assert_array_equal(d.contacts(0.0)[0], edges)
    alive = np.arange(CHAIN) < some
    np.testing.assert_array_equal(d.live() != 0, alive)
    label, index, size, n_islands = got = d.islands(0.0, index=True, sizes=True)
    assert_islands(got, rta.pair_islands(edges, CHAIN, alive), "rebuild of 400")
    assert 1 < n_islands < some and (label[some:] == -1).all() and (index[some:] == -1).all() and not size[some:].any() and (label[:some] >= 0).all()
    d.close()


# ---- impacts ----

def shot(precision):
    """Two clusters at rest -- four overlapping spheres each, in a column at x = -2 and at x = 2 -- and one fast sphere that passes through
    both during the step, from x = -5 to x = 5, apart from everything at either end.  Morton order, balanced ranges, refit bounds.
    -> (Scene, disp, the mover's slot)"""
    R = REAL[precision]
    column = lambda x: [(x, y, 0.0, 0.3) for y in (-0.75, -0.25, 0.25, 0.75)]
    sp = np.array(column(-2.0) + column(2.0) + [(-5.0, 0.0, 0.0, 0.2)], R)
    order = np.argsort(rta.sphere_keys(sp), kind="stable")
    sp = sp[order]
    mover = int(np.flatnonzero(order == 8)[0])
    disp = np.zeros((9, 3), R)
    disp[mover, 0] = 10.0
    rg = rta.balanced_ranges(9, 4)
    return scene_of(sp, rta.refit_bounds(sp, rg, precision), rg, precision), disp, mover


@PRECISIONS
def test_a_fast_sphere_joins_the_clusters_it_passes_through(precision):
    s, disp, mover = shot(precision)
    d = rta.DeviceScene(s)
    w = ImpactWalker(s)
    pairs, _, _, ref_st = w.all(disp)
    np.testing.assert_array_equal(d.impacts(disp)[0], pairs)
    label, index, size, n_islands, st = got = d.impact_islands(disp, index=True, sizes=True, stats=True)
    assert_islands(got, rta.pair_islands(pairs, 9), "shot")
    assert n_islands == 1 and not label.any() and (size == 9).all()
    assert counters(st) == ref_st == counters(d.impacts(disp, capacity=0, stats=True)[2])
    # at the start pose and at the end pose the clusters are apart and the mover is alone
    apart = d.islands(0.0, sizes=True)
    assert apart[2] == 3 and sorted(apart[1].tolist()) == [1] + [4] * 8 and apart[1][mover] == 1 and apart[0][mover] == mover
    d.close()
    end = np.asarray(s.items).copy()
    end[:, :3] += disp
    rg = rta.balanced_ranges(9, 4)
    e = rta.DeviceScene(scene_of(end, rta.refit_bounds(end, rg, precision), rg, precision))
    after = e.islands(0.0, sizes=True)
    assert after[2] == 3 and after[1][mover] == 1
    np.testing.assert_array_equal(after[0], apart[0])
    e.close()


@PRECISIONS
def test_impact_islands_are_the_components_of_the_impacts_walk(precision):
    R = REAL[precision]
    for name in ("nested0", "refit1", "flat2", "clump"):
        s, seed = impact_scenes(precision)[name]
        n = len(s.items)
        d = rta.DeviceScene(s)
        w = ImpactWalker(s)
        for family in ("slow", "fast"):
            disp = displacements(s.items, seed, family, R)
            pairs, _, _, ref_st = w.all(disp)
            got = d.impact_islands(disp, index=True, sizes=True, stats=True)
            assert_islands(got, rta.pair_islands(pairs, n, w.live), (name, family))
            assert counters(got[4]) == ref_st == counters(d.impacts(disp, capacity=0, stats=True)[2]), (name, family)
            assert 1 <= got[3] < n, (name, family)
        # standing still: the islands of the pairs in contact, which impacts() lists at t = 0
        zero = np.zeros((n, 3), R)
        assert_islands(d.impact_islands(zero, index=True, sizes=True), rta.pair_islands(d.impacts(zero)[0], n, w.live), (name, "still"))
        d.close()


# ---- the entries ----

def raw(d, first, label, index, size, n_islands, entry="rt_scene_islands", stream=None):
    """One call of a C entry with the caller's own buffers (numpy arrays for a host entry, torch tensors for a _device entry); None: NULL.
    first: the margin, or disp for the impact form.  n_islands: a uint64 array / int64 tensor of one element, or None."""
    ptr = lambda x: None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data)
    head = first if isinstance(first, float) else ptr(first)
    f = getattr(capi.lib, entry)
    if not entry.endswith("_device"):
        capi.check(f(d._h, head, ptr(label), ptr(index), ptr(size), ptr(n_islands), None), entry)
        return
    import torch
    qs = torch.cuda.current_stream() if stream is None else stream
    capi.check(f(d._h, head, ptr(label), ptr(index), ptr(size), ptr(n_islands), None, C.c_void_p(qs.cuda_stream)), entry)
    qs.synchronize()


def test_entries_buffers_and_streams_agree():
    import torch
    s = cases(rta.RT_F32)["refit"]
    d = rta.DeviceScene(s)
    n = len(s.items)
    margin = median_radius(s)
    ref = d.islands(margin, index=True, sizes=True, stats=True)
    assert 1 < ref[3] < n
    same_bytes(ref[:3], d.islands(margin, index=True, sizes=True)[:3])           # two runs, with and without counters
    # the device entry on a stream that is not the default one writes the host entry's bytes; a second call writes them again
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    a = d.islands(margin, index=True, sizes=True, device=True, stream=side)
    b = d.islands(margin, index=True, sizes=True, stats=True, device=True, stream=side.cuda_stream)
    other = torch.cuda.Stream()
    c = d.islands(0.0, device=True, stream=other)                                # another margin on another stream, in between
    e = d.islands(margin, index=True, sizes=True, device=True)
    side.synchronize()
    other.synchronize()
    torch.cuda.synchronize()
    for got in (a, b, e):
        assert all(x.device.type == "cuda" for x in got[:3])
        same_bytes(ref[:3], got[:3])
        assert int(got[3].item()) == ref[3]
    assert counters(b[4]) == counters(ref[4])
    zero = d.islands(0.0)
    same_bytes(zero[:1], c[:1])
    assert int(c[1].item()) == zero[1]
    # each optional output as NULL leaves the others as they are, host and device; nothing is written behind n_items
    GUARD = 16
    for entry in ("rt_scene_islands", "rt_scene_islands_device"):
        for drop in (None, "index", "size", "n_islands", "all"):
            bufs = {"label": np.full(n + GUARD, -77, np.int32), "index": np.full(n + GUARD, -77, np.int32), "size": np.full(n + GUARD, 77, np.uint32),
                    "n_islands": np.full(1 + GUARD, 77, np.uint64)}
            if entry.endswith("_device"):
                bufs = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).cuda() for k, v in bufs.items()}
            given = {k: (None if drop in (k, "all") and k != "label" else v) for k, v in bufs.items()}
            raw(d, margin, given["label"], given["index"], given["size"], given["n_islands"], entry)
            out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in bufs.items()}
            what = (entry, drop)
            for k, r in (("label", ref[0]), ("index", ref[1]), ("size", ref[2])):
                if given[k] is None:
                    assert (out[k] == out[k][-1]).all(), what                    # not given: not written
                else:
                    np.testing.assert_array_equal(out[k][:n], r, err_msg=str(what))
                    assert (out[k][n:] == out[k][-1]).all() and abs(int(out[k][-1])) == 77, what
            count = out["n_islands"].view(np.uint64)
            assert (count[1:] == 77).all() and count[0] == (77 if given["n_islands"] is None else ref[3]), what
    # pinned host buffers (written by the kernels directly) against pageable ones
    hb = [capi.HostBuffer(4 * n) for _ in range(3)]
    label, index, size = hb[0].array.view(np.int32), hb[1].array.view(np.int32), hb[2].array.view(np.uint32)
    count = np.zeros(1, np.uint64)
    raw(d, margin, label, index, size, count)
    same_bytes(ref[:3], (label, index, size))
    assert count[0] == ref[3]
    # a buffer in device memory is refused by the host entry
    t = torch.zeros(n, dtype=torch.int32, device="cuda")
    with pytest.raises(rta.RtError) as err:
        raw(d, margin, t, None, None, None)
    assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT
    # an islands call between two contacts calls leaves the contacts results as they are: they share a workspace.  On the host ...
    before = d.contacts(margin, gaps=True, offsets=True)
    d.islands(2 * margin, index=True, sizes=True)
    same_bytes(before[:3], d.contacts(margin, gaps=True, offsets=True)[:3])
    # ... and queued on one stream and on two, nothing waited for in between
    total = before[3]
    for second in (side, other):
        x = d.contacts(margin, total, gaps=True, offsets=True, device=True, stream=side)
        y = d.islands(2 * margin, index=True, sizes=True, device=True, stream=second)
        z = d.contacts(margin, total, gaps=True, offsets=True, device=True, stream=side)
        torch.cuda.synchronize()
        same_bytes(before[:3], x[:3])
        same_bytes(before[:3], z[:3])
        same_bytes(d.islands(2 * margin, index=True, sizes=True)[:3], y[:3])
    # the impact form: a tensor goes through the device entry on the stream and gives the host entry's bytes
    disp = displacements(s.items, 3, "fast", np.float32)
    href = d.impact_islands(disp, index=True, sizes=True, stats=True)
    dev = d.impact_islands(torch.from_numpy(disp).cuda(), index=True, sizes=True, stats=True, stream=side)
    again = d.impact_islands(torch.from_numpy(disp).cuda(), index=True, sizes=True, stream=side)
    side.synchronize()
    for got in (dev, again):
        same_bytes(href[:3], got[:3])
        assert int(got[3].item()) == href[3]
    assert counters(dev[4]) == counters(href[4])
    assert_islands(href, rta.pair_islands(d.impacts(disp)[0], n), "impact form")
    count = np.zeros(1, np.uint64)
    label = np.zeros(n, np.int32)
    raw(d, disp, label, None, None, count, "rt_scene_impact_islands")
    np.testing.assert_array_equal(label, href[0])
    assert count[0] == href[3]
    with pytest.raises(rta.RtError) as err:                                      # a displacement outside the host entry's domain
        bad = disp.copy()
        bad[5, 1] = np.inf
        d.impact_islands(bad)
    assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT
    d.close()


# ---- one larger scene, for races: many workgroups unite at once ----

@PRECISIONS
def test_the_default_scene_against_the_components_of_its_contact_list(precision):
    s = rta.Scene.default(precision=precision)
    n = len(s.items)
    assert n == 21845
    d = rta.DeviceScene(s)
    for margin in (0.0, median_radius(s)):
        pairs, total = d.contacts(margin)                                        # (the list is held to the oracle by its own tests)
        assert total == len(pairs) > 0
        ref = rta.pair_islands(pairs, n)
        got = d.islands(margin, index=True, sizes=True)
        assert_islands(got, ref, margin)
        same_bytes(got[:3], d.islands(margin, index=True, sizes=True, device=True)[:3])
        print("default scene, margin %g: %d pairs, %d islands, the largest of %d" % (margin, total, got[3], int(got[2].max())))
    d.close()
