"""Impact pairs on the GPU (rt_scene_impacts / rt_scene_impacts_device, csrc/rt_impacts.hpp): every pair of spheres of the
scene that comes into contact during one step, and when -- bit for bit against a restatement of the walk over the scene's node stream
and its motion table with rta.pair_impacts as the metric, against brute force over all i < j wherever nothing grazes, against the
contact pairs of the start and the end pose (tunnelling), and at the edges of the launch, the scan and the capacity."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.scenes import random_nested_scene
from tests.test_gpu_contacts import COUNTERS, Walker as PairWalker, clump
from tests.test_gpu_near import CAPACITY, LEAF, LIGHT, EYE, same_bytes, scene_of, spheres_of
from tests.test_gpu_query import REAL, bits

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
SEEDS = (0, 1, 2, 3)
FAMILIES = ("slow", "fast")
REFIT_K = 8                                                  # csrc/rt_dynamic.hpp: kRefitK
TINY = {np.float32: np.ldexp(1.0, -80), np.float64: np.ldexp(1.0, -918)}         # csrc/rt_dynamic.hpp: refit_tiny


def extent(items):
    """The largest extent of the spheres along an axis."""
    it = np.asarray(items, np.float64)
    return float(((it[:, :3] + it[:, 3:]).max(axis=0) - (it[:, :3] - it[:, 3:]).min(axis=0)).max())


def displacements(items, seed, family, R):
    """One displacement per sphere from default_rng(100 + seed): a normal direction scaled by a uniform factor of the median radius
    ("slow") or of the largest extent of the scene ("fast"); 30 % of the rows are zero."""
    it = np.asarray(items, np.float64)
    rng = np.random.default_rng(100 + seed)
    u = rng.normal(size=(len(it), 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    scale = float(np.median(it[:, 3])) if family == "slow" else extent(it)
    d = u * rng.uniform(0.0, 1.0, (len(it), 1)) * scale
    d[rng.random(len(it)) < 0.3] = 0.0
    return np.ascontiguousarray(d.astype(R))


MOTION_CHUNK = 256                                           # csrc/rt_impacts.hpp: kMotionChunk


def whole_chunks_of(node, skip):
    """[head, tail): the nodes of the stream range (node, skip) that lie in whole chunks of MOTION_CHUNK nodes (empty: head == tail)."""
    lo = node + 1
    head = min(skip, (lo + MOTION_CHUNK - 1) // MOTION_CHUNK * MOTION_CHUNK)
    return head, max(head, skip // MOTION_CHUNK * MOTION_CHUNK)


def lengths(disp, live, R):
    """m_j of the motion table: the refit's rule for a length, 0 for a slot that is not live."""
    d = np.asarray(disp, R)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        m = np.where(s >= R(TINY[R]), np.sqrt(s), (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2]))
    return np.where(live, m, R(0.0)).astype(R)


class Walker(PairWalker):
    """The definition of the impacts walk (include/rtrace_hip.h), one item at a time, over node_stream(s): the motion table by its rule,
    then item t from behind its own node; every time is rta.pair_impacts' in the scene's precision, the item as the pair's first sphere."""

    def motion(self, disp, whole_chunks=True):
        """(e REAL[n_nodes, 3], E REAL[n_nodes]) parallel to the stream.  whole_chunks=False leaves out of every bound's maximum the
        nodes that k_impact_motion_bounds reads through the chunk maxima -- the whole chunks of MOTION_CHUNK nodes inside (node, skip):
        the table a kernel that lost that path would make."""
        R = self.R
        n_nodes = len(self.bound)
        m = lengths(disp, self.live, R)
        e, E = np.zeros((n_nodes, 3), R), np.zeros(n_nodes, R)
        grow = R(R(1.0) + R(REFIT_K) * np.finfo(R).eps)
        for k in range(n_nodes):
            if not self.bound[k]:
                e[k] = disp[self.item[k]]
                continue
            head, tail = whole_chunks_of(k, self.skip[k])
            below = [self.item[x] for x in range(k + 1, self.skip[k]) if not self.bound[x] and (whole_chunks or not head <= x < tail)]
            E[k] = R(m[below].max() if below else R(0.0)) * grow
        return e, E

    def all(self, disp, table=None):
        """(pairs int32[m, 2], times REAL[m], offsets uint64[n + 1], counters) of the whole scene; table: motion()'s, or another."""
        R = self.R
        disp = np.asarray(disp, R)
        n, n_nodes = self.n_items, len(self.bound)
        e, E = self.motion(disp) if table is None else table
        moves = np.concatenate([disp, e])
        inflate = np.concatenate([np.zeros(n, R), E])
        pairs, times, counts = [], [], np.zeros(n, np.uint64)
        tests_items = tests_bounds = 0
        for t in range(n):
            if not self.live[t]:
                continue
            first = self.node_of[t] + 1
            later = np.arange(first, n_nodes)
            tm = rta.pair_impacts(self.spheres, moves, np.full(len(later), t), n + later, inflate).tolist()
            i = first
            while i < n_nodes:
                g = tm[i - first]
                if self.bound[i]:
                    tests_bounds += 1
                    i = i + 1 if g <= 1.0 else self.skip[i]
                    continue
                tests_items += 1
                if g <= 1.0:
                    pairs.append((t, self.item[i]))
                    times.append(g)
                    counts[t] += 1
                i += 1
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        st = {c: 0 for c in COUNTERS}
        st.update(primary=int(self.live.sum()), hits=int((counts > 0).sum()), sphere_tests=tests_items, bound_tests=tests_bounds,
                  tests_executed=tests_items + tests_bounds)
        return np.array(pairs, np.int32).reshape(-1, 2), np.array(times, R), offsets, st


def assert_walk(d, w, disp, what):
    pairs, time, offsets, total, st = d.impacts(disp, times=True, offsets=True, stats=True)
    ref_p, ref_t, ref_o, ref_st = w.all(disp)
    np.testing.assert_array_equal(pairs, ref_p, err_msg=str(what))
    np.testing.assert_array_equal(bits(time, w.R), bits(ref_t, w.R), err_msg=str(what))
    np.testing.assert_array_equal(offsets, ref_o, err_msg=str(what))
    assert total == len(ref_p) == int(offsets[-1]), what
    assert {c: st[c] for c in COUNTERS} == ref_st, what
    assert (pairs[:, 0] < pairs[:, 1]).all() and (time >= 0).all() and (time <= 1).all(), what
    return pairs, time, {c: st[c] for c in COUNTERS}


@functools.lru_cache(maxsize=None)
def scenes(precision):
    """name -> (rta.Scene, seed of its displacements): random_nested_scene(0 .. 3) as made (some bounds do not enclose: the result is the
    walk's), with refit bounds (which enclose), without bounds, and the contact tests' clump."""
    R = REAL[precision]
    out = {}
    for seed in SEEDS:
        it, bd, rg = random_nested_scene(seed)
        out["nested%d" % seed] = (scene_of(it, bd, rg, precision), seed)
        out["refit%d" % seed] = (scene_of(it, rta.refit_bounds(it.astype(R), rg, precision), rg, precision), seed)
        out["flat%d" % seed] = (rta.Scene(it, rta.normalized(LIGHT, precision), EYE, precision=precision), seed)
    out["clump"] = (clump(precision)[0], 40)
    return out


@PRECISIONS
def test_the_list_restates_the_walk_bit_for_bit(precision):
    R = REAL[precision]
    for name, (s, seed) in scenes(precision).items():
        if name.startswith("refit") and seed > 1:
            continue
        d = rta.DeviceScene(s)
        w = Walker(s)
        n = len(s.items)
        every = n * (n - 1) // 2
        for family in FAMILIES:
            disp = displacements(s.items, seed, family, R)
            pairs, time, st = assert_walk(d, w, disp, (name, family))
            assert 0 < len(pairs) < every, (name, family)
        d.close()


def brute_force(items, disp, R):
    """(i, j, t, grazing) over all i < j.  grazing: the pairs the issue hands to the walk -- in float64 (f64 scenes: the same formula again)
    c > 0, b > 0 and either |t - 1| <= 1e-5 or |disc| <= 1e-5 (b*b + a |c|) (f64: 1e-12 for both)."""
    n = len(items)
    i, j = np.triu_indices(n, 1)
    t = rta.pair_impacts(items, disp, i, j)
    eps = 1e-5 if R == np.float32 else 1e-12
    it, dd = items.astype(np.float64), disp.astype(np.float64)
    v, w = it[j, :3] - it[i, :3], dd[i] - dd[j]
    rad = it[j, 3] + it[i, 3]
    a, b, c = (w * w).sum(axis=1), (v * w).sum(axis=1), (v * v).sum(axis=1) - rad * rad
    disc = b * b - a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        t64 = c / (b + np.sqrt(np.abs(disc)))
        grazing = (c > 0) & (b > 0) & ((np.abs(t64 - 1.0) <= eps) | (np.abs(disc) <= eps * (b * b + a * np.abs(c))))
    return i, j, t, grazing


def check_brute(d, s, disp, what):
    R = REAL[s.precision]
    n = len(s.items)
    i, j, t, grazing = brute_force(s.items, disp, R)
    impact = t <= 1
    assert (impact & grazing).sum() <= 0.05 * max(impact.sum(), 1), what
    pairs, time, total = d.impacts(disp, times=True)
    graze_key = set((i[grazing] * n + j[grazing]).tolist())
    got_key = pairs[:, 0].astype(np.int64) * n + pairs[:, 1]
    keep = np.array([k not in graze_key for k in got_key.tolist()], bool)
    ref = impact & ~grazing
    np.testing.assert_array_equal(got_key[keep], i[ref] * n + j[ref], err_msg=str(what))              # as sets and in order: both are sorted
    np.testing.assert_array_equal(bits(time[keep], R), bits(t[ref], R), err_msg=str(what))
    assert (np.diff(got_key) > 0).all() and total == len(pairs), what
    return pairs, time


@PRECISIONS
def test_the_walk_is_brute_force_where_nothing_grazes(precision):
    R = REAL[precision]
    for name, (s, seed) in scenes(precision).items():
        if not (name.startswith("refit") or name == "clump"):
            continue
        d = rta.DeviceScene(s)
        for family in FAMILIES:
            pairs, _ = check_brute(d, s, displacements(s.items, seed, family, R), (name, family))
            assert len(pairs) > 0
        d.close()


def two_clusters(precision, n=1200):
    """(Scene, disp, Walker): two clusters of n / 2 spheres four units apart, each in Morton order, under balanced ranges (a binary tree whose
    root's children are the clusters) with refit bounds -- about 2,000 nodes, eight chunks of the motion table.  Only spheres move whose
    node lies, for EVERY bound above them except the root, either in a whole chunk of that bound's range or in a range that holds no whole
    chunk: the largest displacement below the bounds that span chunks comes from the chunk maxima alone.  The movers of the second
    cluster cross over into the first, whose spheres stand outside the second cluster's bounds and reach them only through D."""
    R = REAL[precision]
    rng = np.random.default_rng(7)

    def cluster(cx):
        c = np.concatenate([rng.uniform(-1, 1, (n // 2, 3)) + [cx, 0, 0], rng.uniform(0.01, 0.04, (n // 2, 1))], axis=1).astype(R)
        return c[np.argsort(rta.sphere_keys(c), kind="stable")]
    sp = np.concatenate([cluster(-2.0), cluster(2.0)])
    rg = rta.balanced_ranges(n, 4)
    s = scene_of(sp, rta.refit_bounds(sp, rg, precision), rg, precision)
    w = Walker(s)
    n_nodes = len(w.bound)
    in_chunk, allowed = np.zeros(n_nodes, bool), np.ones(n_nodes, bool)
    for k in range(1, n_nodes):
        if w.bound[k]:
            head, tail = whole_chunks_of(k, w.skip[k])
            if tail > head:
                in_chunk[head:tail] = True
                allowed[k + 1:head] = False
                allowed[tail:w.skip[k]] = False
    movers = np.array([w.item[x] for x in np.flatnonzero(in_chunk & allowed) if not w.bound[x]])
    u = rng.normal(size=(len(movers), 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    d = u * rng.uniform(0.1, 0.4, (len(movers), 1))
    d[movers >= n // 2, 0] -= rng.uniform(2.0, 4.0, int((movers >= n // 2).sum()))
    disp = np.zeros((n, 3), R)
    disp[movers] = d.astype(R)
    return s, disp, w


@PRECISIONS
def test_a_bound_over_whole_chunks_takes_its_displacement_from_the_chunk_maxima(precision):
    s, disp, w = two_clusters(precision)
    n = len(s.items)
    # conditions on the inputs: a table made without the whole chunks has other values, culls where the true one enters, and loses pairs
    (_, E), (_, E_cut) = w.motion(disp), w.motion(disp, whole_chunks=False)
    spanning = [k for k in range(1, len(w.bound)) if w.bound[k] and np.diff(whole_chunks_of(k, w.skip[k]))[0] > 0]
    assert len(spanning) >= 6 and all(E[k] > 0 and E_cut[k] == 0 for k in spanning), spanning
    full, cut = w.all(disp), w.all(disp, (w.motion(disp)[0], E_cut))
    assert len(cut[0]) < len(full[0]) and cut[3]["bound_tests"] < full[3]["bound_tests"]
    lost = set(map(tuple, full[0].tolist())) - set(map(tuple, cut[0].tolist()))
    assert lost and all(i < n // 2 <= j for i, j in lost)                        # first-cluster queries, second-cluster movers
    d = rta.DeviceScene(s)
    pairs, time, st = assert_walk(d, w, disp, "two clusters")
    assert lost <= set(map(tuple, pairs.tolist()))
    check_brute(d, s, disp, "two clusters")
    d.close()


def contact_keys(items, precision):
    """The pairs of contacts(0) of a scene without bounds holding `items` (every pair is tested: brute force), as i * n + j."""
    f = rta.DeviceScene(rta.Scene(items, rta.normalized(LIGHT, precision), EYE, precision=precision))
    pairs, _ = f.contacts(0.0)
    f.close()
    return set((pairs[:, 0].astype(np.int64) * len(items) + pairs[:, 1]).tolist())


@PRECISIONS
def test_fast_spheres_that_tunnel_are_impacts_and_in_no_contact_list(precision):
    R = REAL[precision]
    for seed in SEEDS:
        s = scenes(precision)["refit%d" % seed][0]
        n = len(s.items)
        disp = displacements(s.items, seed, "fast", R)
        d = rta.DeviceScene(s)
        pairs, time, total = d.impacts(disp, times=True)
        d.close()
        start = contact_keys(s.items, precision)
        moved = s.items.copy()
        moved[:, :3] = s.items[:, :3] + disp
        end = contact_keys(moved, precision)
        keys = pairs[:, 0].astype(np.int64) * n + pairs[:, 1]
        through = [(k, t) for k, t in zip(keys.tolist(), time.tolist()) if 0.0 < t <= 1.0 and k not in start and k not in end]
        print("seed %d: %d impacts, %d of them apart at the start and at the end" % (seed, total, len(through)))
        assert len(through) >= 1, seed
        # every pair in contact at the start is an impact at t = 0, unless it grazes
        assert (time >= 0).all()


@PRECISIONS
def test_standing_still_and_moving_together_list_the_pairs_in_contact(precision):
    R = REAL[precision]
    for name in ("refit0", "refit3", "clump"):
        s = scenes(precision)[name][0]
        n = len(s.items)
        d = rta.DeviceScene(s)
        zero = np.zeros((n, 3), R)
        pairs, time, total = d.impacts(zero, times=True)
        assert total == len(pairs) > 0 and (time == 0).all(), name
        # away from a gap within 1e-5 max(1, r_i + r_j) of 0 they are the pairs of contacts(0)
        cp, gap, _ = d.contacts(0.0, gaps=True)
        i, j = np.triu_indices(n, 1)
        g = rta.pair_gaps(s.items, i, j).astype(np.float64)
        eps = 1e-5 if R == np.float32 else 1e-12
        near0 = set((i * n + j)[np.abs(g) <= eps * np.maximum(1.0, s.items[i, 3] + s.items[j, 3])].tolist())
        key = lambda p: [k for k in (p[:, 0].astype(np.int64) * n + p[:, 1]).tolist() if k not in near0]
        assert key(pairs) == key(cp), name
        # one displacement for every sphere: w = 0 for every pair, the list of disp = 0
        for move in ((0.25, -0.5, 0.125), (-3.0, 0.0, 0.0)):
            together = np.ascontiguousarray(np.broadcast_to(np.array(move, R), (n, 3)))
            p2, t2, total2 = d.impacts(together, times=True)
            np.testing.assert_array_equal(p2, pairs, err_msg=str((name, move)))
            assert (t2 == 0).all() and total2 == total
        d.close()


@PRECISIONS
def test_scenes_without_bounds_give_the_brute_force_answer(precision):
    R = REAL[precision]
    for seed in SEEDS:
        s = scenes(precision)["flat%d" % seed][0]
        n = len(s.items)
        d = rta.DeviceScene(s)
        i, j = np.triu_indices(n, 1)
        for family in FAMILIES:
            disp = displacements(s.items, seed, family, R)
            t = rta.pair_impacts(s.items, disp, i, j)
            impact = t <= 1                                                          # every later item is tested: nothing is left out
            pairs, time, offsets, total, st = d.impacts(disp, times=True, offsets=True, stats=True)
            np.testing.assert_array_equal(pairs, np.stack([i[impact], j[impact]], axis=1))
            np.testing.assert_array_equal(bits(time, R), bits(t[impact], R))
            assert total == impact.sum() == offsets[-1] and total > 0
            np.testing.assert_array_equal(np.diff(offsets.astype(np.int64)), np.bincount(i[impact], minlength=n))
            assert st["bound_tests"] == 0 and st["sphere_tests"] == n * (n - 1) // 2 and st["primary"] == n
        d.close()


def line_scene(n, precision):
    """n spheres of diameter 1 in a row at spacing 1.5; every odd one moves one spacing toward its left neighbour."""
    R = REAL[precision]
    sp = np.zeros((n, 4), R)
    sp[:, 0] = 1.5 * np.arange(n)
    sp[:, 3] = 0.5
    disp = np.zeros((n, 3), R)
    disp[1::2, 0] = -1.5
    return rta.DeviceScene(rta.Scene.from_spheres_balanced(sp, leaf_size=4, precision=precision), 0, True), disp


def check_line(n, precision):
    # odd k meets k - 1 (which stands still) after a third of the step: v = w = (1.5, 0, 0), a = b = 2.25, c = 2.25 - 1, disc = 2.25, all
    # exact, t = 1.25 / 3.75; k + 1 recedes, k - 2 moves along (w = 0), and every other sphere is more than 1.5 away
    R = REAL[precision]
    d, disp = line_scene(n, precision)
    pairs, time, offsets, total = d.impacts(disp, times=True, offsets=True)
    odd = np.arange(1, n, 2)
    assert total == n // 2 == len(odd), n
    np.testing.assert_array_equal(pairs, np.stack([odd - 1, odd], axis=1), err_msg=str(n))
    assert (bits(time, R) == bits(R(1.25) / R(3.75), R)).all(), n
    counts = np.zeros(n, np.int64)
    counts[odd - 1] = 1
    np.testing.assert_array_equal(offsets, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), err_msg=str(n))
    d.close()


# the launch: 64 lanes a wave, 256 threads a block; the scan: 256 counts a block; the motion table: 256 nodes a chunk
LINE_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)


@PRECISIONS
def test_the_edges_of_the_launch_and_of_the_scan(precision):
    for n in LINE_SIZES:
        check_line(n, precision)


def test_the_second_round_of_the_scan_and_a_large_subtree():
    check_line(65537, rta.RT_F32)                                                # 257 block sums; the root's subtree spans hundreds of chunks


def raw(d, disp, capacity, pairs, time, offsets, entry="host", stream=None):
    """One call of the C entry with the caller's own buffers (numpy arrays for "host", torch tensors for "device"); None: NULL -> total."""
    ptr = lambda x: None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data)
    if entry == "host":
        total = C.c_uint64(0)
        capi.check(capi.lib.rt_scene_impacts(d._h, ptr(disp), capacity, ptr(pairs), ptr(time), ptr(offsets), C.byref(total), None), "rt_scene_impacts")
        return int(total.value)
    import torch
    total = torch.full((), -1, dtype=torch.int64, device="cuda")
    qs = torch.cuda.current_stream() if stream is None else stream
    capi.check(capi.lib.rt_scene_impacts_device(d._h, ptr(disp), capacity, ptr(pairs), ptr(time), ptr(offsets), ptr(total), None, C.c_void_p(qs.cuda_stream)),
               "rt_scene_impacts_device")
    qs.synchronize()
    return int(total.item())


@PRECISIONS
def test_every_capacity_gets_the_exact_prefix(precision):
    import torch
    R = REAL[precision]
    s = scenes(precision)["refit2"][0]
    d = rta.DeviceScene(s)
    n = len(s.items)
    disp = displacements(s.items, 2, "fast", R)
    ref_p, ref_t, ref_o, total = d.impacts(disp, times=True, offsets=True)
    assert total > 16 and len(ref_p) == total
    GUARD = 16
    for capacity in (0, 1, total - 1, total, total + 1):
        for with_pairs in (True, False):
            for entry in ("host", "device"):
                pairs = np.full((capacity + GUARD, 2), -77, np.int32)
                time = np.full(capacity + GUARD, -77.0, R)
                offsets = np.full(n + 1 + GUARD, 77, np.uint64)
                dv = disp
                if entry == "device":
                    pairs, time, offsets = (torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (pairs, time, offsets))
                    dv = torch.from_numpy(disp).cuda()
                got = raw(d, dv, capacity, pairs if with_pairs else None, time if with_pairs else None, offsets, entry)
                if entry == "device":
                    pairs, time, offsets = pairs.cpu().numpy(), time.cpu().numpy(), offsets.cpu().numpy().view(np.uint64)
                what = (capacity, with_pairs, entry)
                assert got == total, what
                np.testing.assert_array_equal(offsets[:n + 1], ref_o, err_msg=str(what))
                assert (offsets[n + 1:] == 77).all(), what
                m = min(capacity, total) if with_pairs else 0
                np.testing.assert_array_equal(pairs[:m], ref_p[:m], err_msg=str(what))
                np.testing.assert_array_equal(bits(time[:m], R), bits(ref_t[:m], R), err_msg=str(what))
                assert (pairs[m:] == -77).all() and (time[m:] == -77.0).all(), what      # nothing behind the list, the guard words included
    # through the wrapper: a capacity gives the prefix, 0 the count alone
    for capacity in (0, 1, total - 1, total, total + 1):
        if capacity == 0:
            pairs, got = d.impacts(disp, 0)
            assert got == total and len(pairs) == 0
            continue
        pairs, time, got = d.impacts(disp, capacity, times=True)
        m = min(capacity, total)
        assert got == total and len(pairs) == m == len(time)
        np.testing.assert_array_equal(pairs, ref_p[:m])
        np.testing.assert_array_equal(bits(time, R), bits(ref_t[:m], R))
    d.close()


def check_dynamic(d, items, live, disp, ranges, precision, what):
    """impacts() on dynamic scene d, which holds `items` with `live`, against the Walker over a fresh static scene (host side only) made
    from the live items -- a dead slot is {0, 0, 0, 0}, which pair_impacts puts at +inf as the walk does the dead record -- and bounds()."""
    R = REAL[precision]
    live = np.asarray(live) != 0
    it = np.where(live[:, None], items, 0).astype(R)
    fresh = scene_of(it, d.bounds() if ranges is not None else None, ranges, precision)
    w = Walker(fresh)
    dead = np.flatnonzero(~live)
    pairs, time, st = assert_walk(d, w, disp, what)
    assert not np.isin(pairs, dead).any(), what
    if live.all():                                                               # ... and a fresh device scene says the same (it takes no dead slot)
        f = rta.DeviceScene(fresh)
        same_bytes(d.impacts(disp, times=True, offsets=True)[:3], f.impacts(disp, times=True, offsets=True)[:3])
        f.close()
    return pairs, st


@PRECISIONS
def test_dynamic_and_live_scenes_answer_as_a_fresh_scene(precision):
    R = REAL[precision]
    ranges = rta.balanced_ranges(CAPACITY, LEAF)
    d = rta.DeviceScene(rta.Scene.from_spheres_balanced(spheres_of(1, R), leaf_size=LEAF, precision=precision), 0, True)
    everyone = np.ones(CAPACITY, np.uint8)
    disp = displacements(spheres_of(1, R), 11, "fast", R)
    slow = displacements(spheres_of(1, R), 12, "slow", R)
    assert len(check_dynamic(d, spheres_of(1, R), everyone, disp, ranges, precision, "as created")[0]) > 0
    moved = spheres_of(2, R)
    d.update(moved)
    check_dynamic(d, moved, everyone, slow, ranges, precision, "update")
    sp = spheres_of(3, R, spread=2.0)
    order = d.rebuild(sp)
    check_dynamic(d, sp[order], everyone, disp, ranges, precision, "rebuild")
    _, st_all = check_dynamic(d, sp[order], everyone, slow, ranges, precision, "rebuild, slow")
    live = (np.random.default_rng(4).random(CAPACITY) < 0.5).astype(np.uint8)
    live[:8] = 0                                                                 # two whole leaves: dead groups
    garbage = sp[order].copy()
    garbage[live == 0] = np.nan                                                  # a dead slot may hold any bits
    d.update(garbage, live=live)
    pairs, st_slow = check_dynamic(d, sp[order], live, slow, ranges, precision, "50 % dead")
    # a killed slot with a huge displacement is in no pair and widens no bound: the same list, the same counters (the walker gives a dead
    # slot the length 0; a bound widened by 1e15 would be entered by every query)
    huge = slow.copy()
    huge[live == 0] = R(1e15)
    pairs_huge, st_huge = check_dynamic(d, sp[order], live, huge, ranges, precision, "50 % dead, their rows huge")
    np.testing.assert_array_equal(pairs_huge, pairs)
    assert st_huge == st_slow and st_huge["bound_tests"] < st_all["bound_tests"]
    check_dynamic(d, sp[order], live, disp, ranges, precision, "50 % dead, fast")
    half = CAPACITY // 2
    order = d.rebuild(sp, n=half)
    it = np.zeros((CAPACITY, 4), R)
    it[:half] = sp[:half][order]
    check_dynamic(d, it, np.arange(CAPACITY) < half, disp, ranges, precision, "rebuild of half")
    # n = 0: no slot is live, so no lane carries a query and no wave makes a test
    d.rebuild(sp, n=0)
    pairs, offsets, total, st = d.impacts(disp, offsets=True, stats=True)
    assert total == 0 and len(pairs) == 0 and not offsets.any()
    assert all(st[c] == 0 for c in COUNTERS)
    d.close()
    # a flat dynamic scene takes liveness too
    flat = rta.DeviceScene(rta.Scene(spheres_of(5, R, 40), rta.normalized(LIGHT, precision), EYE, precision=precision), 0, True)
    live = (np.arange(40) % 3 != 0).astype(np.uint8)
    items = spheres_of(6, R, 40, spread=0.4)
    flat.update(items, live=live)
    check_dynamic(flat, items, live, displacements(items, 13, "fast", R), None, precision, "flat, a third dead")
    flat.close()


def test_the_host_entry_refuses_displacements_outside_its_domain():
    s = scenes(rta.RT_F32)["refit0"][0]
    d = rta.DeviceScene(s)
    n = len(s.items)
    for bad in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        disp = np.zeros((n, 3), np.float32)
        disp[n - 1, 2] = bad
        with pytest.raises(rta.RtError) as err:
            d.impacts(disp)
        assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and "disp" in str(err.value)
    d.close()


def test_entries_buffers_streams_and_threads_agree():
    import torch
    R = np.float32
    s = scenes(rta.RT_F32)["refit1"][0]
    d = rta.DeviceScene(s)
    n = len(s.items)
    disp = displacements(s.items, 1, "fast", R)
    slow = displacements(s.items, 1, "slow", R)
    counters = lambda st: {c: st[c] for c in COUNTERS}
    ref = d.impacts(disp, times=True, offsets=True, stats=True)
    total = ref[3]
    assert total > 0
    same_bytes(ref[:3], d.impacts(disp, times=True, offsets=True)[:3])                               # two runs, with and without counters
    # a contacts call between two impacts calls disturbs neither, and is not disturbed
    touching = d.contacts(0.0, gaps=True, offsets=True)
    same_bytes(ref[:3], d.impacts(disp, times=True, offsets=True)[:3])
    same_bytes(touching[:3], d.contacts(0.0, gaps=True, offsets=True)[:3])
    # the device entry: counted first (an int), with a capacity (nothing waited for), with counters
    dt, st_ = torch.from_numpy(disp).cuda(), torch.from_numpy(slow).cuda()
    dev = d.impacts(dt, times=True, offsets=True)
    assert all(x.device.type == "cuda" for x in dev[:3]) and dev[3] == total
    same_bytes(ref[:3], dev[:3])
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    a = d.impacts(dt, total, times=True, offsets=True, stream=side)
    b = d.impacts(dt, total, times=True, offsets=True, stats=True, stream=side.cuda_stream)
    other = torch.cuda.Stream()
    c = d.impacts(st_, total, stream=other)                                      # other displacements on another stream, in between
    k = d.contacts(0.0, total, device=True, stream=other)                        # ... and a contacts call
    e = d.impacts(dt, total, times=True, offsets=True)
    side.synchronize()
    other.synchronize()
    torch.cuda.synchronize()
    for got in (a, b, e):
        same_bytes(ref[:3], got[:3])
        assert int(got[3].item()) == total
    assert counters(b[4]) == counters(ref[4])
    quiet = d.impacts(slow)
    assert int(c[1].item()) == quiet[1] and np.array_equal(c[0].cpu().numpy()[:min(total, quiet[1])], quiet[0][:total])
    assert int(k[1].item()) == touching[3] and np.array_equal(k[0].cpu().numpy()[:min(total, touching[3])], touching[0][:total])
    # pinned host buffers (used by the kernels directly) against pageable ones
    hb = [capi.HostBuffer(x) for x in (8 * total, 4 * total, 8 * (n + 1), 12 * n)]
    pairs, time, offsets = hb[0].array.view(np.int32).reshape(total, 2), hb[1].array.view(np.float32), hb[2].array.view(np.uint64)
    pinned = hb[3].array.view(np.float32).reshape(n, 3)
    pinned[:] = disp
    assert raw(d, pinned, total, pairs, time, offsets) == total
    same_bytes(ref[:3], (pairs, time, offsets))
    # a buffer in device memory is refused by the host entry
    t = torch.zeros((total, 2), dtype=torch.int32, device="cuda")
    with pytest.raises(rta.RtError) as err:
        raw(d, disp, total, t, None, None)
    assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(rta.RtError) as err:
        raw(d, dt, 0, None, None, None)
    assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT
    # four threads on one scene at once, two displacement sets, contacts in between
    calm = d.impacts(slow, times=True, offsets=True)
    results, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(5):
                results[k] = d.impacts(slow if k % 2 else disp, times=True, offsets=True)
                if k == 3:
                    same_bytes(touching[:3], d.contacts(0.0, gaps=True, offsets=True)[:3])
        except Exception as ex:          # noqa: BLE001 (reported below)
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k, r in enumerate(results):
        same_bytes((calm if k % 2 else ref)[:3], r[:3])
        assert r[3] == (calm if k % 2 else ref)[3]
    d.close()
