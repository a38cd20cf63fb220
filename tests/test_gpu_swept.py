"""Swept overlap lists on the GPU (rt_swept_overlaps / rt_swept_overlaps_device, csrc/rt_swept.hpp): every sphere of the
scene that each moving query sphere comes into contact with during one step, when, and with what normal -- bit for bit against a
restatement of the walk over the scene's node stream and its motion table with rta.swept_times as the metric, against brute force
wherever nothing grazes, against the overlap lists, the impact pairs and the sphere casts where those can answer, and at the edges of the
launch, the scan and the capacity."""
import ctypes as C
import threading

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests import scaled_scenes as ss
from tests.test_gpu_impacts import (FAMILIES, SEEDS, Walker as ImpactWalker, brute_force as impact_brute_force, displacements, scenes, two_clusters,
                                    whole_chunks_of)
from tests.test_gpu_near import CAPACITY, LEAF, LIGHT, EYE, same_bytes, scene_of, spheres_of
from tests.test_gpu_overlap import COUNTERS, counters, queries_for
from tests.test_gpu_query import REAL, bits

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
N_QUERIES = 80                                               # one full wave and a partly filled one
EPS = {np.float32: 1e-5, np.float64: 1e-12}                  # tests/test_gpu_impacts.py brute_force's grazing band


class Walker(ImpactWalker):
    """The definition of the swept walk (include/rtrace_hip.h), one query at a time, over node_stream(s) from node 0: the impact pairs'
    motion table (Walker.motion of tests/test_gpu_impacts.py), the overlap lists' loop, and rta.swept_times / rta.swept_normals over the
    node records as the metric, with the one S of everything the call is given."""

    def table(self, disp, whole_chunks=True):
        return self.motion(np.zeros((self.n_items, 3), self.R) if disp is None else np.asarray(disp, self.R), whole_chunks)

    def scale(self, queries, qdisp, disp, table=None):
        e, _ = self.table(disp) if table is None else table
        return rta.impact_scale(self.spheres[self.n_items:], e, queries, qdisp)

    def all(self, queries, qdisp, disp=None, exclude=None, table=None, S=None):
        """(items int32[m], times REAL[m], normals REAL[m, 3], offsets uint64[n + 1], counters); table: motion()'s, or another; S: the
        call's scale where it is not scale() of the queries given -- queries that count for S and that nobody carries."""
        R = self.R
        queries, qdisp = np.asarray(queries, R), np.asarray(qdisp, R)
        n, n_nodes = len(queries), len(self.bound)
        e, E = self.table(disp) if table is None else table
        records = self.spheres[self.n_items:]
        with np.errstate(invalid="ignore"):
            carried = queries[:, 3] >= 0
        items, times, normals, counts = [], [], [], np.zeros(n, np.uint64)
        tests_items = tests_bounds = 0
        if n_nodes:
            S = self.scale(queries, qdisp, disp, (e, E)) if S is None else S
            tm = rta.swept_times(queries, qdisp, records, e, E, S)
            nm = rta.swept_normals(queries, qdisp, records, e, E, S)
        for g in range(n):
            if not carried[g] or not n_nodes:
                continue
            row = tm[g].tolist()
            ex = -1 if exclude is None else int(exclude[g])
            i = 0
            while i < n_nodes:
                t = row[i]
                if self.bound[i]:
                    tests_bounds += 1
                    i = i + 1 if t <= 1.0 else self.skip[i]
                    continue
                tests_items += 1
                if self.item[i] != ex and t <= 1.0:
                    items.append(self.item[i])
                    times.append(t)
                    normals.append(nm[g, i])
                    counts[g] += 1
                i += 1
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        st = {c: 0 for c in COUNTERS}
        st.update(primary=int(carried.sum()), hits=int((counts > 0).sum()), sphere_tests=tests_items, bound_tests=tests_bounds,
                  tests_executed=tests_items + tests_bounds)
        return np.array(items, np.int32), np.array(times, R), np.array(normals, R).reshape(-1, 3), offsets, st


def assert_walk(d, w, queries, qdisp, disp, what, exclude=None, order=None):
    items, time, normal, offsets, total, st = d.swept_overlaps(queries, qdisp, disp, exclude=exclude, order=order, times=True, normals=True, offsets=True,
                                                               stats=True)
    ref_i, ref_t, ref_n, ref_o, ref_st = w.all(queries, qdisp, disp, exclude)
    np.testing.assert_array_equal(items, ref_i, err_msg=str(what))
    np.testing.assert_array_equal(bits(time, w.R), bits(ref_t, w.R), err_msg=str(what))
    np.testing.assert_array_equal(bits(normal, w.R), bits(ref_n, w.R), err_msg=str(what))
    np.testing.assert_array_equal(offsets, ref_o, err_msg=str(what))
    assert total == len(ref_i) == int(offsets[-1]), what
    assert counters(st) == ref_st, what
    assert (time >= 0).all() and (time <= 1).all(), what
    for g in range(len(queries)):                                                # ascending within a query
        assert (np.diff(items[int(offsets[g]):int(offsets[g + 1])]) > 0).all(), (what, g)
    return items, time, normal, offsets, counters(st)


def queries_of(s, seed, family, n=N_QUERIES):
    """(queries REAL[n, 4], qdisp REAL[n, 3]): tests/test_gpu_overlap.py's queries_for (default_rng(77 + seed)) and, for their motion,
    tests/test_gpu_impacts.py's displacements of those spheres -- "slow": factors of the median q, "fast": of the queries' extent."""
    R = REAL[s.precision]
    queries = queries_for(s, n, 77 + seed)
    return queries, displacements(queries, seed, family, R)


def scene_disp(s, seed, family):
    """The scene's own motion for a swept call: None (it stands still), or the impact tests' displacements of its items."""
    return None if family is None else displacements(s.items, seed, family, REAL[s.precision])


MOTIONS = (("slow", None), ("fast", None), ("slow", "slow"), ("fast", "fast"), ("fast", "slow"))      # (the queries' family, the scene's)


@PRECISIONS
def test_the_list_restates_the_walk_bit_for_bit(precision):
    for name, (s, seed) in scenes(precision).items():
        if name.startswith(("refit", "flat")) and seed > 1:
            continue
        d = rta.DeviceScene(s)
        w = Walker(s)
        for qfam, sfam in MOTIONS:
            queries, qdisp = queries_of(s, seed, qfam)
            items, *_ = assert_walk(d, w, queries, qdisp, scene_disp(s, seed, sfam), (name, qfam, sfam))
            assert 0 < len(items) < len(queries) * len(s.items), (name, qfam, sfam)
        d.close()


def brute_force(queries, qdisp, items, disp, R):
    """(t REAL[n, m], grazing bool[n, m]) over every (query, item).  grazing is tests/test_gpu_impacts.py brute_force's own band, asked of
    the records queries + items with the displacements qdisp + disp: in float64 c > 0, b > 0 and either |t - 1| <= 1e-5 or
    |disc| <= 1e-5 (b*b + a |c|) (f64: 1e-12 for both)."""
    n, m = len(queries), len(items)
    d = np.zeros((m, 3), R) if disp is None else disp
    t = rta.swept_times(queries, qdisp, items, d)
    i, j, _, g = impact_brute_force(np.concatenate([queries, items]), np.concatenate([qdisp, d]), R)
    cross = (i < n) & (j >= n)
    grazing = np.zeros((n, m), bool)
    grazing[i[cross], j[cross] - n] = g[cross]
    return t, grazing


def brute_cases(precision):
    """(name, Scene, seed) of the comparison with brute force: the refit twins (their bounds enclose), the clump, the scenes without bounds."""
    return [(name, s, seed) for name, (s, seed) in scenes(precision).items() if name.startswith(("refit", "flat")) or name == "clump"]


def check_brute(d, s, queries, qdisp, disp, what):
    R = REAL[s.precision]
    t, grazing = brute_force(queries, qdisp, s.items, disp, R)
    listed = t <= 1
    assert (listed & grazing).sum() <= 0.05 * max(listed.sum(), 1), what
    items, time, offsets, total = d.swept_overlaps(queries, qdisp, disp, times=True, offsets=True)
    m = len(s.items)
    rows = np.repeat(np.arange(len(queries)), np.diff(offsets.astype(np.int64)))
    got_key = rows * m + items
    keep = ~grazing[rows, items]
    ref = listed & ~grazing
    gi, gj = np.nonzero(ref)                                                     # row-major: sorted by (g, item slot)
    np.testing.assert_array_equal(got_key[keep], gi * m + gj, err_msg=str(what))
    np.testing.assert_array_equal(bits(time[keep], R), bits(t[ref], R), err_msg=str(what))
    assert (np.diff(got_key) > 0).all() and total == len(items), what
    return items, time, offsets, rows


@PRECISIONS
def test_the_walk_is_brute_force_where_nothing_grazes(precision):
    for name, s, seed in brute_cases(precision):
        d = rta.DeviceScene(s)
        for qfam, sfam in MOTIONS:
            queries, qdisp = queries_of(s, seed, qfam)
            items, *_ = check_brute(d, s, queries, qdisp, scene_disp(s, seed, sfam), (name, qfam, sfam))
            assert len(items) > 0
        d.close()


def standing_band(queries, items, R):
    """bool[n, m]: the (query, item) whose start poses are within 1e-5 max(1, r + q) (f64: 1e-12) of touching, in float64 -- the band the
    impact tests leave out when they compare a standing list with a contacts list."""
    qs, it = queries.astype(np.float64), items.astype(np.float64)
    dist = np.sqrt(((it[None, :, :3] - qs[:, None, :3]) ** 2).sum(axis=2))
    reach = it[None, :, 3] + qs[:, None, 3]
    return np.abs(dist - reach) <= EPS[R] * np.maximum(1.0, reach)


@PRECISIONS
def test_standing_queries_are_the_overlap_lists(precision):
    R = REAL[precision]
    for seed in SEEDS:
        s = scenes(precision)["refit%d" % seed][0]
        d = rta.DeviceScene(s)
        m = len(s.items)
        queries = queries_for(s, N_QUERIES, 77 + seed)
        zero = np.zeros((N_QUERIES, 3), R)
        items, time, offsets, total = d.swept_overlaps(queries, zero, None, times=True, offsets=True)
        assert total == len(items) > 0 and (time == 0).all(), seed
        o_items, o_offsets, _ = d.overlaps(queries, 0.0, offsets=True)
        band = standing_band(queries, s.items, R)
        key = lambda it, off: [k for k in (np.repeat(np.arange(N_QUERIES), np.diff(off.astype(np.int64))) * m + it).tolist() if not band.flat[k]]
        assert key(items, offsets) == key(o_items, o_offsets), seed
        d.close()


@PRECISIONS
def test_the_scenes_own_spheres_as_queries_give_the_impact_pairs(precision):
    R = REAL[precision]
    for seed in SEEDS:
        s = scenes(precision)["refit%d" % seed][0]
        d = rta.DeviceScene(s)
        n = len(s.items)
        me = np.arange(n, dtype=np.int32)
        own = np.ascontiguousarray(s.items.astype(R))
        for family in FAMILIES:
            disp = displacements(s.items, seed, family, R)
            items, time, offsets, total = d.swept_overlaps(own, disp, disp, exclude=me, times=True, offsets=True)
            pairs, ptime, ptotal = d.impacts(disp, times=True)
            i, j, _, grazing = impact_brute_force(s.items, disp, R)
            graze = set((i[grazing] * n + j[grazing]).tolist())
            rows = np.repeat(np.arange(n), np.diff(offsets.astype(np.int64)))
            assert (items != rows).all() and total > 0 and ptotal > 0, (seed, family)
            lo, hi = np.minimum(rows, items).astype(np.int64), np.maximum(rows, items).astype(np.int64)
            both = {}
            for k, row, tb in zip((lo * n + hi).tolist(), rows.tolist(), bits(time, R).tolist()):
                both.setdefault(k, []).append((row, tb))
            impact = dict(zip((pairs[:, 0].astype(np.int64) * n + pairs[:, 1]).tolist(), bits(ptime, R).tolist()))
            clear = lambda keys: {k for k in keys if k not in graze}
            assert clear(both) == clear(impact), (seed, family)                  # row i is the set of impact pairs that contain i ...
            for k in clear(both):
                assert len(both[k]) == 2 and {r for r, _ in both[k]} == {k // n, k % n}, (seed, family, k)      # ... seen from both of its ends
            common = set(both) & set(impact)
            assert common and all(tb == impact[k] for k in common for _, tb in both[k]), (seed, family)          # the same bits on every common pair
        d.close()


@PRECISIONS
def test_a_row_is_not_empty_exactly_where_a_cast_finds_a_contact(precision):
    R = REAL[precision]
    for seed in SEEDS:
        s = scenes(precision)["refit%d" % seed][0]
        d = rta.DeviceScene(s)
        for family in FAMILIES:
            queries, qdisp = queries_of(s, seed, family)
            items, offsets, total = d.swept_overlaps(queries, qdisp, None, offsets=True)
            t, grazing = brute_force(queries, qdisp, s.items, None, R)
            length = np.sqrt((qdisp.astype(np.float64) ** 2).sum(axis=1))
            moving = length > 0
            clear = moving & ~grazing.any(axis=1) & ~standing_band(queries, s.items, R).any(axis=1)
            assert clear.sum() >= 0.4 * N_QUERIES, (seed, family, int(clear.sum()))
            unit = np.where(moving[:, None], qdisp.astype(np.float64) / np.where(moving, length, 1.0)[:, None], [1.0, 0.0, 0.0])
            rays = np.ascontiguousarray(np.concatenate([queries[:, :3], unit.astype(R)], axis=1))
            dist, _, item = d.sweep(rays, np.ascontiguousarray(queries[:, 3]), length.astype(R), any_hit=True)
            rows = np.diff(offsets.astype(np.int64))
            np.testing.assert_array_equal(rows[clear] > 0, item[clear] >= 0, err_msg=str((seed, family)))
            assert (rows[clear] > 0).any() and (rows[clear] == 0).any(), (seed, family)
        d.close()


def tunnelled(d, s, queries, qdisp, R):
    """The entries of a swept call against the standing scene that are in neither overlap list, of the start pose and of the end pose, away
    from the bands: (keys, times)."""
    m = len(s.items)
    items, time, offsets, total = d.swept_overlaps(queries, qdisp, None, times=True, offsets=True)
    rows = np.repeat(np.arange(len(queries)), np.diff(offsets.astype(np.int64)))
    moved = queries.copy()
    moved[:, :3] = queries[:, :3] + qdisp
    _, grazing = brute_force(queries, qdisp, s.items, None, R)
    band = grazing | standing_band(queries, s.items, R) | standing_band(moved, s.items, R)
    seen = set()
    for pose in (queries, moved):
        it, off, _ = d.overlaps(np.ascontiguousarray(pose), 0.0, offsets=True)
        seen |= set((np.repeat(np.arange(len(pose)), np.diff(off.astype(np.int64))) * m + it).tolist())
    keys = rows * m + items
    through = np.array([k not in seen and not band.flat[k] for k in keys.tolist()], bool)
    return keys[through], time[through]


@PRECISIONS
def test_fast_queries_that_tunnel_are_listed_and_in_no_overlap_list(precision):
    R = REAL[precision]
    for seed in SEEDS:
        s = scenes(precision)["refit%d" % seed][0]
        d = rta.DeviceScene(s)
        queries, qdisp = queries_of(s, seed, "fast")
        keys, time = tunnelled(d, s, queries, qdisp, R)
        print("seed %d: %d entries apart at the start and at the end" % (seed, len(keys)))
        assert len(keys) >= 1 and (time > 0).all() and (time < 1).all(), seed
        d.close()


def arrival_queries(s, disp, R, q=0.01):
    """Standing queries where the second cluster's movers of two_clusters arrive: in the first cluster, outside every bound of the second."""
    n = len(s.items)
    movers = np.flatnonzero((np.abs(disp).sum(axis=1) > 0) & (np.arange(n) >= n // 2))
    queries = np.concatenate([s.items[movers, :3] + disp[movers], np.full((len(movers), 1), q)], axis=1)
    return np.ascontiguousarray(queries.astype(R)), np.zeros((len(movers), 3), R), movers


@PRECISIONS
def test_standing_queries_are_reached_through_the_chunk_maxima(precision):
    R = REAL[precision]
    s, disp, iw = two_clusters(precision)
    w = Walker(s)
    queries, qdisp, movers = arrival_queries(s, disp, R)
    assert len(queries) >= 20 and (queries[:, 0] < 0).mean() > 0.5               # most of them stand in the first cluster
    (e, E), (_, E_cut) = w.table(disp), w.table(disp, whole_chunks=False)
    spanning = [k for k in range(1, len(w.bound)) if w.bound[k] and np.diff(whole_chunks_of(k, w.skip[k]))[0] > 0]
    assert len(spanning) >= 6 and all(E[k] > 0 and E_cut[k] == 0 for k in spanning), spanning
    full, cut = w.all(queries, qdisp, disp), w.all(queries, qdisp, disp, table=(e, E_cut))
    lost = set(zip(np.repeat(np.arange(len(queries)), np.diff(full[3].astype(np.int64))).tolist(), full[0].tolist())) - \
        set(zip(np.repeat(np.arange(len(queries)), np.diff(cut[3].astype(np.int64))).tolist(), cut[0].tolist()))
    assert len(cut[0]) < len(full[0]) and lost and all(item >= len(s.items) // 2 for _, item in lost)       # movers of the second cluster
    d = rta.DeviceScene(s)
    items, time, normal, offsets, _ = assert_walk(d, w, queries, qdisp, disp, "two clusters")
    got = set(zip(np.repeat(np.arange(len(queries)), np.diff(offsets.astype(np.int64))).tolist(), items.tolist()))
    assert lost <= got
    # every query is touched by the mover it was put in the way of, at the end of the step or before
    assert all((g, int(j)) in got or brute_force(queries[g:g + 1], qdisp[g:g + 1], s.items[j:j + 1], disp[j:j + 1], R)[1].any() for g, j in enumerate(movers))
    d.close()


def check_dynamic(d, items, live, ranges, precision, what, disp, queries, qdisp):
    """swept_overlaps() on dynamic scene d, which holds `items` with `live`, against the Walker over a fresh static scene (host side only)
    made from the live items -- a dead slot is {0, 0, 0, 0}, which swept_times puts at +inf as the walk does the dead record -- and
    bounds()."""
    R = REAL[precision]
    live = np.asarray(live) != 0
    it = np.where(live[:, None], items, 0).astype(R)
    fresh = scene_of(it, d.bounds() if ranges is not None else None, ranges, precision)
    w = Walker(fresh)
    got = assert_walk(d, w, queries, qdisp, disp, what)
    assert not np.isin(got[0], np.flatnonzero(~live)).any(), what
    if live.all():                                                               # ... and a fresh device scene says the same (it takes no dead slot)
        f = rta.DeviceScene(fresh)
        kw = dict(times=True, normals=True, offsets=True)
        same_bytes(d.swept_overlaps(queries, qdisp, disp, **kw)[:4], f.swept_overlaps(queries, qdisp, disp, **kw)[:4])
        f.close()
    return got


def unit_queries(seed, family, R, n=N_QUERIES):
    rng = np.random.default_rng(78 + seed)
    queries = np.concatenate([rng.uniform(-1.2, 1.2, (n, 3)), rng.uniform(0.0, 0.3, (n, 1))], axis=1).astype(R)
    queries[::10, 3] = 0
    return np.ascontiguousarray(queries), displacements(queries, seed, family, R)


@PRECISIONS
def test_dynamic_and_live_scenes_answer_as_a_fresh_scene(precision):
    R = REAL[precision]
    ranges = rta.balanced_ranges(CAPACITY, LEAF)
    d = rta.DeviceScene(rta.Scene.from_spheres_balanced(spheres_of(1, R), leaf_size=LEAF, precision=precision), 0, True)
    everyone = np.ones(CAPACITY, np.uint8)
    fast = displacements(spheres_of(1, R), 11, "fast", R)
    slow = displacements(spheres_of(1, R), 12, "slow", R)
    queries, qdisp = unit_queries(0, "fast", R)
    _, qslow = unit_queries(0, "slow", R)
    assert len(check_dynamic(d, spheres_of(1, R), everyone, ranges, precision, "as created", fast, queries, qdisp)[0]) > 0
    check_dynamic(d, spheres_of(1, R), everyone, ranges, precision, "as created, standing", None, queries, qslow)
    moved = spheres_of(2, R)
    d.update(moved)
    check_dynamic(d, moved, everyone, ranges, precision, "update", slow, queries, qdisp)
    sp = spheres_of(3, R, spread=2.0)
    order = d.rebuild(sp)
    check_dynamic(d, sp[order], everyone, ranges, precision, "rebuild", fast, queries, qslow)
    st_all = check_dynamic(d, sp[order], everyone, ranges, precision, "rebuild, slow", slow, queries, qslow)[4]
    live = (np.random.default_rng(4).random(CAPACITY) < 0.5).astype(np.uint8)
    live[:8] = 0                                                                 # two whole leaves: dead groups
    garbage = sp[order].copy()
    garbage[live == 0] = np.nan                                                  # a dead slot may hold any bits
    d.update(garbage, live=live)
    half_dead = check_dynamic(d, sp[order], live, ranges, precision, "50 % dead", slow, queries, qslow)
    # a dead slot with a huge displacement is never listed and widens no bound: the same entries, the same counters
    huge = slow.copy()
    huge[live == 0] = R(1e15)
    with_huge = check_dynamic(d, sp[order], live, ranges, precision, "50 % dead, their rows huge", huge, queries, qslow)
    same_bytes(half_dead[:4], with_huge[:4])
    assert with_huge[4] == half_dead[4] and with_huge[4]["bound_tests"] < st_all["bound_tests"]
    check_dynamic(d, sp[order], live, ranges, precision, "50 % dead, fast", fast, queries, qdisp)
    check_dynamic(d, sp[order], live, ranges, precision, "50 % dead, standing", None, queries, qdisp)
    half = CAPACITY // 2
    order = d.rebuild(sp, n=half)
    it = np.zeros((CAPACITY, 4), R)
    it[:half] = sp[:half][order]
    check_dynamic(d, it, np.arange(CAPACITY) < half, ranges, precision, "rebuild of half", fast, queries, qdisp)
    # n = 0: every query still walks, and the dead root culls at its one test -- the walker says so too
    d.rebuild(sp, n=0)
    empty = Walker(scene_of(np.zeros((CAPACITY, 4), R), d.bounds(), ranges, precision)).all(queries, qdisp, fast)
    assert len(empty[0]) == 0 and empty[4]["sphere_tests"] == 0 and empty[4]["primary"] == len(queries) and empty[4]["hits"] == 0
    for disp in (fast, None):
        items, offsets, total, st = d.swept_overlaps(queries, qdisp, disp, offsets=True, stats=True)
        assert total == 0 and len(items) == 0 and not offsets.any() and len(offsets) == len(queries) + 1
        assert counters(st) == empty[4]
    d.close()
    # a flat dynamic scene takes liveness too
    flat = rta.DeviceScene(rta.Scene(spheres_of(5, R, 40), rta.normalized(LIGHT, precision), EYE, precision=precision), 0, True)
    live = (np.arange(40) % 3 != 0).astype(np.uint8)
    items = spheres_of(6, R, 40, spread=0.4)
    flat.update(items, live=live)
    check_dynamic(flat, items, live, None, precision, "flat, a third dead", displacements(items, 13, "fast", R), queries, qdisp)
    flat.close()


# the launch: 64 lanes a wave, 256 threads a block; the scan: 256 counts a block, 256 block sums a turn of the spine (65,536 counts)
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 65537)


@PRECISIONS
def test_the_edges_of_the_launch_and_of_the_scan(precision):
    R = REAL[precision]
    s, seed = scenes(precision)["refit0"]
    d = rta.DeviceScene(s)
    w = Walker(s)
    base, base_d = queries_of(s, seed, "fast", 257)
    disp = scene_disp(s, seed, "slow")
    ref_i, ref_t, ref_n, ref_o, _ = w.all(base, base_d, disp)                     # rows are independent (one S: the same queries, repeated)
    cut = lambda a: [a[int(ref_o[g]):int(ref_o[g + 1])] for g in range(257)]
    rows, times, normals = cut(ref_i), cut(ref_t), cut(ref_n)
    assert sum(len(x) for x in rows) > 0 and min(len(x) for x in rows) == 0
    S = w.scale(base, base_d, disp)
    for n in EDGE_SIZES:
        pick = np.arange(n) % 257
        queries, qdisp = np.ascontiguousarray(base[pick]), np.ascontiguousarray(base_d[pick])
        if w.scale(queries, qdisp, disp) != S:                                   # (fewer queries, another M: their own reference)
            assert n < 257
            r = w.all(queries, qdisp, disp)
            want = (r[0], r[1], r[2], r[3])
        else:
            counts = np.array([len(rows[g]) for g in pick], np.uint64)
            want = (np.concatenate([rows[g] for g in pick]).astype(np.int32), np.concatenate([times[g] for g in pick]).astype(R),
                    np.concatenate([normals[g] for g in pick]).astype(R).reshape(-1, 3), np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64))
        items, time, normal, offsets, total = d.swept_overlaps(queries, qdisp, disp, times=True, normals=True, offsets=True)
        assert total == len(want[0]) == len(items), n
        same_bytes(want, (items, time, normal, offsets))
    d.close()


def line(n, precision):
    """tests/test_gpu_impacts.py's line of n spheres of diameter 1 at spacing 1.5 (every odd one moves one spacing to the left), and one
    query of radius 0.5 two units above every sphere that comes down by 1.5."""
    R = REAL[precision]
    sp = np.zeros((n, 4), R)
    sp[:, 0] = 1.5 * np.arange(n)
    sp[:, 3] = 0.5
    disp = np.zeros((n, 3), R)
    disp[1::2, 0] = -1.5
    queries = sp.copy()
    queries[:, 1] = 2.0
    qdisp = np.zeros((n, 3), R)
    qdisp[:, 1] = -1.5
    return sp, disp, queries, qdisp


def test_a_line_of_65537_spheres_under_as_many_queries():
    # 257 block sums in the scan, hundreds of chunks under the root in the motion table.  Every coordinate is a multiple of 0.5 below 2^17,
    # so all differences are exact and a query meets only the spheres within two places of its own: brute force over those is the answer
    precision, n = rta.RT_F32, 65537
    R = REAL[precision]
    sp, disp, queries, qdisp = line(n, precision)
    d = rta.DeviceScene(rta.Scene.from_spheres_balanced(sp, leaf_size=4, precision=precision))
    for moving in (None, disp):
        S = rta.impact_scale(sp, moving, queries, qdisp)
        assert S == R(2.0 ** -17)
        want_i, want_t, counts = [], [], np.zeros(n, np.uint64)
        for lo in range(0, n, 256):
            hi = min(n, lo + 256)
            a, b = max(0, lo - 2), min(n, hi + 2)
            t = rta.swept_times(queries[lo:hi], qdisp[lo:hi], sp[a:b], None if moving is None else moving[a:b], None, S)
            g, j = np.nonzero(t <= 1)
            want_i.append(j + a)
            want_t.append(t[g, j])
            counts[lo:hi] = np.bincount(g, minlength=hi - lo)
        items, time, offsets, total = d.swept_overlaps(queries, qdisp, moving, times=True, offsets=True)
        assert total == int(counts.sum()) >= n and len(items) == total
        np.testing.assert_array_equal(items, np.concatenate(want_i).astype(np.int32))
        np.testing.assert_array_equal(bits(time, R), bits(np.concatenate(want_t).astype(R), R))
        np.testing.assert_array_equal(offsets, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64))
        if moving is None:                                                       # v = (0, -2), w = (0, -1.5): a = 2.25, b = 3, cc = 3, disc = 2.25, all exact
            assert total == n and (items == np.arange(n)).all() and (bits(time, R) == bits(R(3.0) / R(4.5), R)).all()
    d.close()


def raw(d, queries, qdisp, disp, capacity, items, time, normal, offsets, entry="host", exclude=None, order=None, stream=None):
    """One call of the C entry with the caller's own buffers (numpy arrays for "host", torch tensors for "device"); None: NULL -> total."""
    ptr = lambda x: None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data)
    n = len(queries)
    if entry == "host":
        total = C.c_uint64(0)
        capi.check(capi.lib.rt_swept_overlaps(d._h, ptr(queries), ptr(qdisp), n, ptr(disp), ptr(exclude), ptr(order), capacity, ptr(items), ptr(time), ptr(normal),
                                              ptr(offsets), C.byref(total), None), "rt_swept_overlaps")
        return int(total.value)
    import torch
    total = torch.full((), -1, dtype=torch.int64, device="cuda")
    qs = torch.cuda.current_stream() if stream is None else stream
    capi.check(capi.lib.rt_swept_overlaps_device(d._h, ptr(queries), ptr(qdisp), n, ptr(disp), ptr(exclude), ptr(order), capacity, ptr(items), ptr(time),
                                                 ptr(normal), ptr(offsets), ptr(total), None, C.c_void_p(qs.cuda_stream)), "rt_swept_overlaps_device")
    qs.synchronize()
    return int(total.item())


@PRECISIONS
def test_every_capacity_gets_the_exact_prefix(precision):
    import torch
    R = REAL[precision]
    s, seed = scenes(precision)["refit2"]
    d = rta.DeviceScene(s)
    queries, qdisp = queries_of(s, seed, "slow", 40)
    disp = scene_disp(s, seed, "slow")
    n = len(queries)
    ref_i, ref_t, ref_n, ref_o, total = d.swept_overlaps(queries, qdisp, disp, times=True, normals=True, offsets=True)
    assert 16 < total < 200 and len(ref_i) == total
    dev = [torch.from_numpy(x).cuda() for x in (queries, qdisp, disp)]
    GUARD = 16
    for capacity in range(0, total + 2):
        for given in ("all", "time", "normal", "none") if capacity in (0, 1, total - 1, total, total + 1) else ("all",):
            for entry in ("host", "device"):
                items = np.full(capacity + GUARD, -77, np.int32)
                time = np.full(capacity + GUARD, -77.0, R)
                normal = np.full(3 * (capacity + GUARD), -77.0, R)
                offsets = np.full(n + 1 + GUARD, 77, np.uint64)
                if entry == "device":
                    items, time, normal, offsets = (torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (items, time, normal, offsets))
                q, qd, dd = dev if entry == "device" else (queries, qdisp, disp)
                got = raw(d, q, qd, dd, capacity, None if given == "none" else items, time if given in ("all", "time") else None,
                          normal if given in ("all", "normal") else None, offsets, entry)
                if entry == "device":
                    items, time, normal, offsets = items.cpu().numpy(), time.cpu().numpy(), normal.cpu().numpy(), offsets.cpu().numpy().view(np.uint64)
                what = (capacity, given, entry)
                assert got == total, what
                np.testing.assert_array_equal(offsets[:n + 1], ref_o, err_msg=str(what))
                assert (offsets[n + 1:] == 77).all(), what
                m = min(capacity, total) if given != "none" else 0
                mt, mn = (m if given in ("all", "time") else 0), (m if given in ("all", "normal") else 0)
                np.testing.assert_array_equal(items[:m], ref_i[:m], err_msg=str(what))
                np.testing.assert_array_equal(bits(time[:mt], R), bits(ref_t[:mt], R), err_msg=str(what))
                np.testing.assert_array_equal(bits(normal[:3 * mn], R), bits(ref_n[:mn].reshape(-1), R), err_msg=str(what))
                assert (items[m:] == -77).all() and (time[mt:] == -77.0).all() and (normal[3 * mn:] == -77.0).all(), what      # nothing behind the list
    # through the wrapper: a capacity gives the prefix, 0 the count alone
    for capacity in (0, 1, total - 1, total, total + 7):
        if capacity == 0:
            items, got = d.swept_overlaps(queries, qdisp, disp, capacity=0)
            assert got == total and len(items) == 0
            continue
        items, time, normal, got = d.swept_overlaps(queries, qdisp, disp, capacity=capacity, times=True, normals=True)
        m = min(capacity, total)
        assert got == total and len(items) == m == len(time) == len(normal)
        same_bytes((items, time, normal), (ref_i[:m], ref_t[:m], ref_n[:m]))
    d.close()


@PRECISIONS
def test_exclude_and_any_order_give_the_same_bytes(precision):
    import torch
    R = REAL[precision]
    s, seed = scenes(precision)["refit1"]
    d = rta.DeviceScene(s)
    w = Walker(s)
    queries, qdisp = queries_of(s, seed, "fast", 200)
    disp = scene_disp(s, seed, "slow")
    n = len(queries)
    kw = dict(times=True, normals=True, offsets=True, stats=True)
    plain = d.swept_overlaps(queries, qdisp, disp, **kw)
    exclude = np.random.default_rng(5).integers(-1, len(s.items) + 3, n).astype(np.int32)
    for g in range(0, n, 2):                                                      # every other query that lists something excludes its first entry
        if plain[3][g + 1] > plain[3][g]:
            exclude[g] = plain[0][int(plain[3][g])]
    assert_walk(d, w, queries, qdisp, disp, "exclude", exclude=exclude)
    ref = d.swept_overlaps(queries, qdisp, disp, exclude=exclude, **kw)
    assert ref[4] < plain[4]                                                      # something was excluded
    rows = np.repeat(np.arange(n), np.diff(ref[3].astype(np.int64)))
    assert (ref[0] != exclude[rows]).all()
    orders = {"identity": np.arange(n, dtype=np.uint32), "reversed": np.arange(n, dtype=np.uint32)[::-1].copy(),
              "random": np.random.default_rng(6).permutation(n).astype(np.uint32)}
    for name, order in orders.items():
        got = d.swept_overlaps(queries, qdisp, disp, exclude=exclude, order=order, **kw)
        same_bytes(ref[:4], got[:4])
        assert got[4] == ref[4] and counters(got[5]) == counters(ref[5]), name
    got = d.swept_overlaps(queries, qdisp, disp, exclude=exclude, order=True, **kw)
    same_bytes(ref[:4], got[:4])
    assert counters(got[5]) == counters(ref[5])
    # the device entry: the same in every order; an entry >= n carries no query, and a query nobody carries has count 0 -- but counts for S
    dq, dqd, dd, dex = (torch.from_numpy(x).cuda() for x in (queries, qdisp, disp, exclude))
    got = d.swept_overlaps(dq, dqd, dd, exclude=dex, order=torch.from_numpy(orders["random"].astype(np.int32)).cuda(), **kw)
    same_bytes(ref[:4], got[:4])
    assert got[4] == ref[4] and counters(got[5]) == counters(ref[5])
    got = d.swept_overlaps(dq, dqd, dd, exclude=dex, order=True, **kw)
    same_bytes(ref[:4], got[:4])
    holes = orders["random"].astype(np.int64)
    dropped = holes[::7].copy()
    holes[::7] = n                                                                # nobody carries these queries
    holes[7] = 0x7FFFFFFF
    dropped = np.append(dropped, orders["random"][7])
    kept = np.ones(n, bool)
    kept[dropped] = False
    S = w.scale(queries, qdisp, disp)
    sub = queries.copy()
    sub[~kept, 3] = -1                                                            # the walker's way to say "no query"
    assert w.scale(sub, qdisp, disp) == S                                         # (the dropped queries are not the largest of anything)
    r = w.all(sub, qdisp, disp, exclude)
    got = d.swept_overlaps(dq, dqd, dd, exclude=dex, order=torch.from_numpy(holes.astype(np.int32)).cuda(), **kw)
    same_bytes(r[:4], got[:4])
    assert got[4] == len(r[0]) and counters(got[5]) == r[4]
    # a query with q = -1 or NaN on the device entry: an empty row and no test
    for value in (-1.0, np.nan, -np.inf):
        odd = queries.copy()
        odd[3::5, 3] = value
        r = w.all(odd, qdisp, disp, exclude)
        assert r[4]["primary"] == n - len(odd[3::5]) and (np.diff(r[3].astype(np.int64))[3::5] == 0).all()
        got = d.swept_overlaps(torch.from_numpy(odd).cuda(), dqd, dd, exclude=dex, **kw)
        same_bytes(r[:4], got[:4])
        assert counters(got[5]) == r[4]
    d.close()


CASES = pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)


def placed_inputs(c, family):
    """(queries, qdisp, disp) of Case c: its overlap queries, moved by the impact tests' displacements of those spheres, and its own
    displacements of the same family."""
    queries = ss.overlap_queries(c)
    return queries, displacements(queries, 950 + ss._index(c), family, REAL[c.precision]), ss.displacements(c, family)


@CASES
def test_the_list_of_a_placed_scene_restates_the_walk_bit_for_bit(param):
    precision, placement = param
    for c in ss.case(precision, placement):
        d = rta.DeviceScene(c.scene)
        w = Walker(c.scene)
        for family in FAMILIES:
            queries, qdisp, disp = placed_inputs(c, family)
            for moving in (disp, None):
                items, *_ = assert_walk(d, w, queries, qdisp, moving, (ss.case_id(param), c.name, family, moving is not None))
                assert 0 < len(items) < len(queries) * len(c.scene.items)
        d.close()


POW2 = (-66, -40, 33, 45)
POW2_CASES = [(p, k) for p in (rta.RT_F32, rta.RT_F64) for k in POW2]


def pow2_inputs(index, family, k, R):
    """(items, bounds or None, ranges, queries, qdisp, disp) of base scene `index` of tests/scaled_scenes.py, every length times 2^k."""
    name, items0, bounds0, ranges = ss.base_scenes()[index]
    as_real = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 4).astype(R))
    items0 = as_real(items0)
    rng = np.random.default_rng(800 + index)
    queries0 = np.concatenate([rng.uniform(-1.2, 1.2, (N_QUERIES, 3)), rng.uniform(0.0, 0.3, (N_QUERIES, 1))], axis=1).astype(R)
    queries0[::10, 3] = 0
    qdisp0 = displacements(queries0, 950 + index, family, R)
    disp0 = displacements(items0, 900 + index, family, R)
    up = lambda a: None if a is None else np.ascontiguousarray(np.ldexp(a, k).astype(R))
    out = [up(items0), None if bounds0 is None else up(as_real(bounds0)), ranges, up(queries0), up(qdisp0), up(disp0)]
    for a, a0 in zip(out, (items0, None if bounds0 is None else as_real(bounds0), None, queries0, qdisp0, disp0)):
        assert a0 is None or (np.isfinite(a).all() and (np.ldexp(a, -k) == a0).all())       # exact
    return out


@pytest.mark.parametrize("precision,k", POW2_CASES, ids=["%s-2^%d" % ("f32" if p == rta.RT_F32 else "f64", k) for p, k in POW2_CASES])
def test_a_power_of_two_scaling_changes_no_byte_of_the_list(precision, k):
    R = REAL[precision]
    for index in (0, 2):                                                         # nested, and the same items without bounds
        for family in FAMILIES:
            results = []
            for factor in (0, k):
                items, bounds, ranges, queries, qdisp, disp = pow2_inputs(index, family, factor, R)
                s = scene_of(items, bounds, ranges, precision)
                d = rta.DeviceScene(s)
                got = assert_walk(d, Walker(s), queries, qdisp, disp, (index, family, factor))
                d.close()
                results.append(got)
            assert len(results[0][0]) > 0
            # items, time bits, normal bits, offsets.  (Not the counters: a displacement shorter than the square root of refit_tiny takes its
            # length from the L1 rule, so a bound's D -- never an item's time -- depends on the scale, and each walk matches its own walker.)
            same_bytes(results[0][:4], results[1][:4])


@PRECISIONS
def test_a_lone_far_query_sets_the_scale(precision):
    R = REAL[precision]
    s, seed = scenes(precision)["refit0"]
    d = rta.DeviceScene(s)
    w = Walker(s)
    queries, qdisp = queries_of(s, seed, "slow")
    disp = scene_disp(s, seed, "slow")
    near = w.scale(queries, qdisp, disp)
    far, far_d = queries.copy(), qdisp.copy()
    far[-1] = (1e15, 0.0, 0.0, 0.25)
    far_d[-1] = (-0.5, 0.0, 0.0)
    S = w.scale(far, far_d, disp)
    assert S == rta.impact_scale(s.items, disp, far, far_d) == R(2.0 ** -50) and near >= R(0.125)       # 1e15 = 0.888 2^50; the unit scene's own S
    got = assert_walk(d, w, far, far_d, disp, "a query at 1e15")
    ref = assert_walk(d, w, queries, qdisp, disp, "without it")
    rows, far_rows = np.diff(ref[3].astype(np.int64)), np.diff(got[3].astype(np.int64))
    assert far_rows[-1] == 0 and len(got[0]) > 0
    if R == np.float64:                                                          # 2^-255 M is far below the scene: the other rows keep their items
        np.testing.assert_array_equal(far_rows[:-1], rows[:-1])
    # ... and the same query with q = -1 carries no query and does not count (the device entry: the host entry refuses such a q)
    import torch
    far[-1, 3] = -1
    assert w.scale(far, far_d, disp) == near
    gone = d.swept_overlaps(*(torch.from_numpy(x).cuda() for x in (far, far_d, disp)), times=True, normals=True, offsets=True, stats=True)
    want = w.all(far, far_d, disp)
    same_bytes(want[:4], gone[:4])
    assert gone[4] == len(want[0]) and counters(gone[5]) == want[4]
    same_bytes(ref[:3], want[:3])                                                # the last row was empty before, too
    assert rows[-1] == 0
    d.close()


def far_query_inputs(precision, x=1e15):
    """(Scene, queries, qdisp, disp, sub, S_far, S_near) for the tests of "S counts a query nobody carries": refit0 with its slow inputs and
    the last query at (x, 0, 0, 0.25); sub is the walker's way to say that nobody carries that query (q = -1), S_far the scale with it
    counted (2^-50 for 1e15) and S_near the scale without it."""
    R = REAL[precision]
    s, seed = scenes(precision)["refit0"]
    w = Walker(s)
    queries, qdisp = queries_of(s, seed, "slow")
    disp = scene_disp(s, seed, "slow")
    far, far_d = queries.copy(), qdisp.copy()
    far[-1] = (x, 0.0, 0.0, 0.25)
    far_d[-1] = (-0.5, 0.0, 0.0)
    sub = far.copy()
    sub[-1, 3] = -1
    S_far, S_near = w.scale(far, far_d, disp), w.scale(sub, far_d, disp)
    assert (S_far == R(2.0 ** -50) or x != 1e15) and S_far < R(2.0 ** -49) and S_near >= R(0.125) and S_near == w.scale(queries, qdisp, disp)
    return s, far, far_d, disp, sub, S_far, S_near


@PRECISIONS
def test_a_far_query_that_nobody_carries_still_sets_the_scale(precision):
    """S is folded by query index, whatever the order: the last query lies at 1e15 and the device entry's `order` has a hole exactly for
    it.  It walks nowhere and lists nothing, and every other row is the walk's at S = 2^-50 -- in f32 other bytes than at the near S, which
    a magnitude kernel that folded only the carried queries would give."""
    import torch
    s, far, far_d, disp, sub, S_far, S_near = far_query_inputs(precision)
    d = rta.DeviceScene(s)
    w = Walker(s)
    n = len(far)
    want, near = w.all(sub, far_d, disp, S=S_far), w.all(sub, far_d, disp, S=S_near)
    differ = len(want[0]) != len(near[0]) or (want[0] != near[0]).any() or (bits(want[1], w.R) != bits(near[1], w.R)).any()
    if precision == rta.RT_F32:                                                   # (f64: 2^-50 is an exact scaling of a unit scene, the same bits)
        assert differ
    order = np.arange(n, dtype=np.int32)
    order[n - 1] = n                                                             # nobody carries the far query
    kw = dict(times=True, normals=True, offsets=True, stats=True)
    dev = [torch.from_numpy(x).cuda() for x in (far, far_d, disp)]
    got = d.swept_overlaps(*dev, order=torch.from_numpy(order).cuda(), **kw)
    same_bytes(want[:4], got[:4])
    assert got[4] == len(want[0]) > 0 and counters(got[5]) == want[4] and want[4]["primary"] == n - 1
    if differ:
        assert not (len(got[0]) == len(near[0]) and np.array_equal(got[0].cpu().numpy(), near[0]) and
                    np.array_equal(bits(got[1].cpu().numpy(), w.R), bits(near[1], w.R)))
    d.close()


def test_entries_buffers_streams_and_threads_agree():
    import torch
    R = np.float32
    s, seed = scenes(rta.RT_F32)["refit1"]
    d = rta.DeviceScene(s)
    n_items = len(s.items)
    queries, qdisp = queries_of(s, seed, "fast", 200)
    _, qslow = queries_of(s, seed, "slow", 200)
    disp, slow = scene_disp(s, seed, "fast"), scene_disp(s, seed, "slow")
    n = len(queries)
    kw = dict(times=True, normals=True, offsets=True)
    ref = d.swept_overlaps(queries, qdisp, disp, stats=True, **kw)
    total = ref[4]
    assert total > 0
    same_bytes(ref[:4], d.swept_overlaps(queries, qdisp, disp, **kw)[:4])                            # two runs, with and without counters
    # calls of all five list entries on one scene, interleaved: each gives its own bytes
    margin = float(np.median(s.items[:, 3]))
    touching = d.contacts(0.0, gaps=True, offsets=True)
    hitting = d.impacts(disp, times=True, offsets=True)
    over = d.overlaps(queries, margin, gaps=True, offsets=True)
    near = d.near(np.ascontiguousarray(queries[:, :3]), 8, np.full(n, margin, R), all_within=True)
    same_bytes(ref[:4], d.swept_overlaps(queries, qdisp, disp, **kw)[:4])
    same_bytes(over[:3], d.overlaps(queries, margin, gaps=True, offsets=True)[:3])
    same_bytes(ref[:4], d.swept_overlaps(queries, qdisp, disp, **kw)[:4])
    same_bytes(hitting[:3], d.impacts(disp, times=True, offsets=True)[:3])
    same_bytes(touching[:3], d.contacts(0.0, gaps=True, offsets=True)[:3])
    same_bytes(near[:3], d.near(np.ascontiguousarray(queries[:, :3]), 8, np.full(n, margin, R), all_within=True)[:3])
    same_bytes(ref[:4], d.swept_overlaps(queries, qdisp, disp, **kw)[:4])
    # the device entry: counted first (an int), with a capacity (nothing waited for), with counters
    dq, dqd, dqs, dd, ds = (torch.from_numpy(x).cuda() for x in (queries, qdisp, qslow, disp, slow))
    dev = d.swept_overlaps(dq, dqd, dd, **kw)
    assert all(x.device.type == "cuda" for x in dev[:4]) and dev[4] == total
    same_bytes(ref[:4], dev[:4])
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    a = d.swept_overlaps(dq, dqd, dd, capacity=total, stream=side, **kw)
    b = d.swept_overlaps(dq, dqd, dd, capacity=total, stats=True, stream=side.cuda_stream, **kw)
    other = torch.cuda.Stream()
    c = d.swept_overlaps(dq, dqs, ds, capacity=total, stream=other)              # other motions on another stream, in between
    k = d.impacts(dd, hitting[3], stream=other)                                  # ... an impacts call, whose table is another
    o = d.overlaps(dq, margin, capacity=over[3], stream=other)                   # ... and an overlap call, whose counts are the same
    e = d.swept_overlaps(dq, dqd, dd, capacity=total, **kw)
    side.synchronize()
    other.synchronize()
    torch.cuda.synchronize()
    for got in (a, b, e):
        same_bytes(ref[:4], got[:4])
        assert int(got[4].item()) == total
    assert counters(b[5]) == counters(ref[5])
    quiet = d.swept_overlaps(queries, qslow, slow)
    assert int(c[1].item()) == quiet[1] and np.array_equal(c[0].cpu().numpy()[:min(total, quiet[1])], quiet[0][:total])
    assert int(k[1].item()) == hitting[3] and np.array_equal(k[0].cpu().numpy(), hitting[0])
    assert int(o[1].item()) == over[3] and np.array_equal(o[0].cpu().numpy(), over[0])
    # pinned host buffers (read and written by the kernels directly) against pageable ones
    hb = [capi.HostBuffer(x) for x in (16 * n, 12 * n, 12 * n_items, 4 * total, 4 * total, 12 * total, 8 * (n + 1))]
    f = lambda k, shape: hb[k].array.view(np.float32).reshape(shape)
    pq, pqd, pd, items, time, normal, offsets = f(0, (n, 4)), f(1, (n, 3)), f(2, (n_items, 3)), hb[3].array.view(np.int32), f(4, total), f(5, (total, 3)), \
        hb[6].array.view(np.uint64)
    pq[:], pqd[:], pd[:] = queries, qdisp, disp
    assert raw(d, pq, pqd, pd, total, items, time, normal, offsets) == total
    same_bytes(ref[:4], (items, time, normal, offsets))
    # a buffer in device memory is refused by the host entry
    for args in ((queries, qdisp, disp, total, torch.zeros(total, dtype=torch.int32, device="cuda"), None, None, None), (dq, qdisp, disp, 0, None, None, None, None),
                 (queries, dqd, disp, 0, None, None, None, None), (queries, qdisp, dd, 0, None, None, None, None)):
        with pytest.raises(rta.RtError) as err:
            raw(d, *args)
        assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and "device memory" in str(err.value)
    # a call that grows the workspace, then a smaller one: the same bytes as fresh calls
    grown_q, grown_d = np.ascontiguousarray(np.concatenate([queries] * 5)[:937]), np.ascontiguousarray(np.concatenate([qdisp] * 5)[:937])
    many = d.swept_overlaps(grown_q, grown_d, disp, **kw)
    same_bytes(ref[:4], d.swept_overlaps(queries, qdisp, disp, **kw)[:4])
    same_bytes(ref[:4], d.swept_overlaps(dq, dqd, dd, **kw)[:4])
    fresh = rta.DeviceScene(s)
    same_bytes(many[:4], fresh.swept_overlaps(grown_q, grown_d, disp, **kw)[:4])
    fresh.close()
    assert many[4] == int(np.diff(ref[3].astype(np.int64))[np.arange(937) % n].sum())
    # four threads on one scene at once: two swept inputs, and the other list entries in between
    calm = d.swept_overlaps(queries, qslow, None, **kw)
    results, errors = [None] * 4, []

    def work(t):
        try:
            for _ in range(5):
                results[t] = d.swept_overlaps(queries, qslow, None, **kw) if t % 2 else d.swept_overlaps(queries, qdisp, disp, **kw)
                if t == 2:
                    same_bytes(over[:3], d.overlaps(queries, margin, gaps=True, offsets=True)[:3])
                if t == 3:
                    same_bytes(hitting[:3], d.impacts(disp, times=True, offsets=True)[:3])
                    same_bytes(touching[:3], d.contacts(0.0, gaps=True, offsets=True)[:3])
        except Exception as ex:          # noqa: BLE001 (reported below)
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t, r in enumerate(results):
        same_bytes((calm if t % 2 else ref)[:4], r[:4])
        assert r[4] == (calm if t % 2 else ref)[4]
    d.close()


def test_the_host_entry_refuses_motions_outside_its_domain():
    s, seed = scenes(rta.RT_F32)["refit0"]
    d = rta.DeviceScene(s)
    n_items = len(s.items)
    queries, qdisp = queries_of(s, seed, "slow")
    for bad in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        disp = np.zeros((n_items, 3), np.float32)
        disp[n_items - 1, 2] = bad
        with pytest.raises(rta.RtError) as err:
            d.swept_overlaps(queries, qdisp, disp)
        assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and " disp" in str(err.value)
        moved = qdisp.copy()
        moved[len(queries) - 1, 0] = bad
        with pytest.raises(rta.RtError) as err:
            d.swept_overlaps(queries, moved)
        assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and "qdisp" in str(err.value)
    assert d.swept_overlaps(queries, qdisp)[1] > 0                                # ... and the scene answers the next call
    d.close()
