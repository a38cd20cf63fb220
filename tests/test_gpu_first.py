"""First contacts on the GPU (rt_first_contacts / rt_first_contacts_device, csrc/rt_first.hpp): the earliest contact of each
moving query sphere with the scene during one step -- bit for bit against FirstWalker, a restatement of the walk over the scene's node
stream and its motion table with rta.swept_times / rta.swept_normals as the metric; against the swept overlap lists of the same inputs
(the result is the row's smallest time at its lowest slot), the overlap lists and the sphere casts where those can answer; and at the
edges of the launch.  The shapes are the swept tests': 80 queries (one full wave and a part of one) over scenes of about 120 items."""
import ctypes as C
import threading

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.test_gpu_impacts import SEEDS, displacements, scenes, two_clusters
from tests.test_gpu_near import CAPACITY, LEAF, LIGHT, EYE, same_bytes, scene_of, spheres_of
from tests.test_gpu_overlap import COUNTERS, counters, queries_for
from tests.test_gpu_query import REAL, bits
from tests.test_gpu_swept import (MOTIONS, N_QUERIES, Walker, arrival_queries, brute_force, queries_of, scene_disp, standing_band, unit_queries)

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
ANY = pytest.mark.parametrize("any_hit", [False, True], ids=["nearest", "any"])
SCENES = ("nested0", "refit0", "refit1", "flat0", "flat1", "clump")


class FirstWalker(Walker):
    """The definition of the first-contacts walk (include/rtrace_hip.h), one query at a time: the swept walk's stream, motion table, S and
    metric (rta.swept_times / rta.swept_normals over the node records), with the window that shrinks -- best = 1, found = False, and
    beats(t) = t < best if found else t <= best for bounds and items alike."""

    def first(self, queries, qdisp, disp=None, exclude=None, any_hit=False, table=None, S=None):
        """(time REAL[n], item int32[n], normal REAL[n, 3], counters); table: motion()'s, or another; S: the call's scale where it is not
        scale() of the queries given -- queries that count for S and that nobody carries."""
        R = self.R
        queries, qdisp = np.asarray(queries, R), np.asarray(qdisp, R)
        n, n_nodes = len(queries), len(self.bound)
        e, E = self.table(disp) if table is None else table
        records = self.spheres[self.n_items:]
        with np.errstate(invalid="ignore"):
            carried = queries[:, 3] >= 0
        time, item, normal = np.full(n, np.inf, R), np.full(n, -1, np.int32), np.zeros((n, 3), R)
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
            best, found, i = 1.0, False, 0
            while i < n_nodes:
                t = row[i]
                beats = t < best if found else t <= best
                if self.bound[i]:
                    tests_bounds += 1
                    i = i + 1 if beats else self.skip[i]
                    continue
                tests_items += 1
                if self.item[i] != ex and beats:
                    best, found = t, True
                    time[g], item[g], normal[g] = tm[g, i], self.item[i], nm[g, i]
                    if any_hit or t == 0.0:
                        break
                i += 1
        st = {c: 0 for c in COUNTERS}
        st.update(primary=int(carried.sum()), hits=int((item >= 0).sum()), sphere_tests=tests_items, bound_tests=tests_bounds,
                  tests_executed=tests_items + tests_bounds)
        return time, item, normal, st


def assert_first(d, w, queries, qdisp, disp, what, any_hit=False, exclude=None, order=None, args=None):
    """first_contacts() of d against w.first(); args: what to call with instead of (queries, qdisp, disp, exclude) -- tensors."""
    q, qd, dd, ex = (queries, qdisp, disp, exclude) if args is None else args
    time, item, normal, st = d.first_contacts(q, qd, dd, any_hit=any_hit, exclude=ex, order=order, normals=True, stats=True)
    ref_t, ref_i, ref_n, ref_st = w.first(queries, qdisp, disp, exclude, any_hit)
    if hasattr(time, "cpu"):
        time, item, normal = (x.cpu().numpy() for x in (time, item, normal))
    np.testing.assert_array_equal(bits(time, w.R), bits(ref_t, w.R), err_msg=str(what))
    np.testing.assert_array_equal(item, ref_i, err_msg=str(what))
    np.testing.assert_array_equal(bits(normal, w.R), bits(ref_n, w.R), err_msg=str(what))
    assert counters(st) == ref_st, what
    hit = item >= 0
    assert (time[hit] >= 0).all() and (time[hit] <= 1).all() and np.isinf(time[~hit]).all() and not normal[~hit].any(), what
    return time, item, normal, counters(st)


@PRECISIONS
@ANY
def test_the_result_restates_the_walk_bit_for_bit(precision, any_hit):
    import torch
    for name in SCENES:
        s, seed = scenes(precision)[name]
        d = rta.DeviceScene(s)
        w = FirstWalker(s)
        for k, (qfam, sfam) in enumerate(MOTIONS):
            queries, qdisp = queries_of(s, seed, qfam)
            disp = scene_disp(s, seed, sfam)
            what = (name, qfam, sfam)
            _, item, _, st = assert_first(d, w, queries, qdisp, disp, what, any_hit)
            assert (item >= 0).any() and (item < 0).any() and st["tests_executed"] > 0, what
            if k == 0:                                                           # ... and the device entry with tensors: the same bytes
                dev = [None if x is None else torch.from_numpy(x).cuda() for x in (queries, qdisp, disp)]
                assert_first(d, w, queries, qdisp, disp, what + ("device",), any_hit, args=(*dev, None))
        d.close()


@PRECISIONS
@ANY
def test_exclude_and_any_order_give_the_same_bytes(precision, any_hit):
    import torch
    s, seed = scenes(precision)["refit1"]
    d = rta.DeviceScene(s)
    w = FirstWalker(s)
    queries, qdisp = queries_of(s, seed, "fast", 200)
    disp = scene_disp(s, seed, "slow")
    n = len(queries)
    plain = assert_first(d, w, queries, qdisp, disp, "plain", any_hit)
    exclude = np.random.default_rng(5).integers(-1, len(s.items) + 3, n).astype(np.int32)
    exclude[::2] = plain[1][::2]                                                  # every other query excludes what it found (-1: nothing)
    ref = assert_first(d, w, queries, qdisp, disp, "exclude", any_hit, exclude=exclude)
    assert (ref[1] != exclude)[ref[1] >= 0].all() and (ref[1] != plain[1]).any()
    orders = {"identity": np.arange(n, dtype=np.uint32), "reversed": np.arange(n, dtype=np.uint32)[::-1].copy(),
              "random": np.random.default_rng(6).permutation(n).astype(np.uint32)}
    for name, order in orders.items():                                           # the host entry: a permutation
        got = d.first_contacts(queries, qdisp, disp, any_hit=any_hit, exclude=exclude, order=order, normals=True, stats=True)
        same_bytes(ref[:3], got[:3])
        assert counters(got[3]) == ref[3], name
    # the device entry: the same in every order; an entry >= n carries no query and leaves that thread's outputs alone -- but counts for S
    dq, dqd, dd, dex = (torch.from_numpy(x).cuda() for x in (queries, qdisp, disp, exclude))
    got = d.first_contacts(dq, dqd, dd, any_hit=any_hit, exclude=dex, order=torch.from_numpy(orders["random"].astype(np.int32)).cuda(), normals=True, stats=True)
    same_bytes(ref[:3], got[:3])
    assert counters(got[3]) == ref[3]
    holes = orders["random"].astype(np.int64)
    dropped = holes[::7].copy()
    holes[::7] = n                                                                # nobody carries these queries
    holes[7] = 0x7FFFFFFF
    dropped = np.append(dropped, orders["random"][7])
    kept = np.ones(n, bool)
    kept[dropped] = False
    sub = queries.copy()
    sub[~kept, 3] = -1                                                            # the walker's way to say "no query"
    assert w.scale(sub, qdisp, disp) == w.scale(queries, qdisp, disp)             # (the dropped queries are not the largest of anything)
    r = w.first(sub, qdisp, disp, exclude, any_hit)
    R = REAL[precision]
    out = (torch.full((n,), -77.0, dtype=dq.dtype, device="cuda"), torch.full((n,), -77, dtype=torch.int32, device="cuda"),
           torch.full((n, 3), -77.0, dtype=dq.dtype, device="cuda"))
    got = d.first_contacts(dq, dqd, dd, any_hit=any_hit, exclude=dex, order=torch.from_numpy(holes.astype(np.int32)).cuda(), normals=True, stats=True, out=out)
    time, item, normal = (x.cpu().numpy() for x in got[:3])
    same_bytes((r[0][kept], r[1][kept], r[2][kept]), (time[kept], item[kept], normal[kept]))
    assert (time[~kept] == R(-77.0)).all() and (item[~kept] == -77).all() and (normal[~kept] == R(-77.0)).all()
    assert counters(got[3]) == r[3]
    # a query with q = -1, NaN or -inf on the device entry: +inf, -1, a zero normal and no test
    for value in (-1.0, np.nan, -np.inf):
        odd = queries.copy()
        odd[3::5, 3] = value
        r = w.first(odd, qdisp, disp, exclude, any_hit)
        assert r[3]["primary"] == n - len(odd[3::5]) and np.isinf(r[0][3::5]).all() and (r[1][3::5] == -1).all() and not r[2][3::5].any()
        got = d.first_contacts(torch.from_numpy(odd).cuda(), dqd, dd, any_hit=any_hit, exclude=dex, normals=True, stats=True)
        same_bytes(r[:3], got[:3])
        assert counters(got[3]) == r[3]
    d.close()


def rows_of(d, queries, qdisp, disp, exclude=None):
    """The swept overlap list of the inputs, cut into rows: [(items, time bits, normal bits)] per query, and the count pass's counters."""
    R = REAL[d.scene.precision]
    items, time, normal, offsets, _, st = d.swept_overlaps(queries, qdisp, disp, exclude=exclude, times=True, normals=True, offsets=True, stats=True)
    o = offsets.astype(np.int64)
    return [(items[o[g]:o[g + 1]], time[o[g]:o[g + 1]], bits(normal[o[g]:o[g + 1]], R)) for g in range(len(queries))], counters(st)


def check_links(rows, time, item, normal, any_time, any_item, R, what):
    """A result exists exactly where the row is not empty; it is an entry of the row with that entry's bits; ANY is an entry of the row;
    NEAREST is the row's smallest time at its lowest slot, for every query."""
    for g, (r_items, r_time, r_normal) in enumerate(rows):
        assert (item[g] >= 0) == (any_item[g] >= 0) == (len(r_items) > 0), (what, g)
        if item[g] < 0:
            continue
        k = int(np.flatnonzero(r_items == item[g])[0])
        assert bits(time[g:g + 1], R)[0] == bits(r_time[k:k + 1], R)[0] and (bits(normal[g], R) == r_normal[k]).all(), (what, g)
        first = int(np.flatnonzero(r_time == r_time.min())[0])                   # (ascending slots: the first of the smallest)
        assert k == first, (what, g, r_items, r_time, item[g])
        ka = int(np.flatnonzero(r_items == any_item[g])[0])
        assert bits(any_time[g:g + 1], R)[0] == bits(r_time[ka:ka + 1], R)[0], (what, g)


@PRECISIONS
def test_the_result_is_the_smallest_time_of_the_swept_row_at_its_lowest_slot(precision):
    R = REAL[precision]
    fewer = 0
    for name in SCENES:
        s, seed = scenes(precision)[name]
        d = rta.DeviceScene(s)
        for qfam, sfam in MOTIONS:
            queries, qdisp = queries_of(s, seed, qfam)
            disp = scene_disp(s, seed, sfam)
            rows, list_st = rows_of(d, queries, qdisp, disp)
            time, item, normal, st = d.first_contacts(queries, qdisp, disp, normals=True, stats=True)
            a_time, a_item, a_st = d.first_contacts(queries, qdisp, disp, any_hit=True, stats=True)
            check_links(rows, time, item, normal, a_time, a_item, R, (name, qfam, sfam))
            assert a_st["tests_executed"] <= st["tests_executed"] <= list_st["tests_executed"], (name, qfam, sfam)
            fewer += qfam == "fast" and st["tests_executed"] < list_st["tests_executed"]
        d.close()
    assert fewer > 0


@PRECISIONS
def test_standing_queries_touch_at_zero_exactly_where_they_overlap(precision):
    R = REAL[precision]
    for seed in SEEDS[:2]:
        s = scenes(precision)["refit%d" % seed][0]
        d = rta.DeviceScene(s)
        queries = queries_for(s, N_QUERIES, 77 + seed)
        time, item = d.first_contacts(queries, np.zeros((N_QUERIES, 3), R))
        assert ((time == 0) == (item >= 0)).all() and np.isinf(time[item < 0]).all(), seed      # nothing moves: a contact is one at the start
        o_items, o_offsets, _ = d.overlaps(queries, 0.0, offsets=True)
        rows = np.diff(o_offsets.astype(np.int64))
        clear = ~standing_band(queries, s.items, R).any(axis=1)                  # (the two metrics may differ within rounding of touching)
        assert clear.sum() >= 0.8 * N_QUERIES
        np.testing.assert_array_equal((time == 0)[clear], (rows > 0)[clear], err_msg=str(seed))
        assert (rows[clear] > 0).any() and (rows[clear] == 0).any()
        first = np.array([o_items[int(o_offsets[g])] if rows[g] else -1 for g in range(N_QUERIES)])
        np.testing.assert_array_equal(item[clear], first[clear])                 # the lowest slot of the row
        d.close()


@PRECISIONS
def test_a_result_exists_exactly_where_a_cast_finds_a_contact(precision):
    R = REAL[precision]
    for seed in SEEDS[:2]:
        s = scenes(precision)["refit%d" % seed][0]
        d = rta.DeviceScene(s)
        for family in ("slow", "fast"):
            queries, qdisp = queries_of(s, seed, family)
            time, item = d.first_contacts(queries, qdisp)
            _, grazing = brute_force(queries, qdisp, s.items, None, R)
            length = np.sqrt((qdisp.astype(np.float64) ** 2).sum(axis=1))
            moving = length > 0
            clear = moving & ~grazing.any(axis=1) & ~standing_band(queries, s.items, R).any(axis=1)
            assert clear.sum() >= 0.4 * N_QUERIES, (seed, family, int(clear.sum()))
            unit = np.where(moving[:, None], qdisp.astype(np.float64) / np.where(moving, length, 1.0)[:, None], [1.0, 0.0, 0.0])
            rays = np.ascontiguousarray(np.concatenate([queries[:, :3], unit.astype(R)], axis=1))
            _, _, cast = d.sweep(rays, np.ascontiguousarray(queries[:, 3]), length.astype(R), any_hit=True)
            np.testing.assert_array_equal(item[clear] >= 0, cast[clear] >= 0, err_msg=str((seed, family)))
            assert (item[clear] >= 0).any() and (item[clear] < 0).any(), (seed, family)
        d.close()


@PRECISIONS
def test_a_fast_query_that_tunnels_is_found_between_the_poses(precision):
    R = REAL[precision]
    through = 0
    for seed in SEEDS[:2]:
        s = scenes(precision)["refit%d" % seed][0]
        d = rta.DeviceScene(s)
        m = len(s.items)
        queries, qdisp = queries_of(s, seed, "fast")
        time, item = d.first_contacts(queries, qdisp)
        moved = queries.copy()
        moved[:, :3] = queries[:, :3] + qdisp
        _, grazing = brute_force(queries, qdisp, s.items, None, R)
        band = grazing | standing_band(queries, s.items, R) | standing_band(moved, s.items, R)
        seen = set()
        for pose in (queries, moved):
            it, off, _ = d.overlaps(np.ascontiguousarray(pose), 0.0, offsets=True)
            seen |= set((np.repeat(np.arange(len(pose)), np.diff(off.astype(np.int64))) * m + it).tolist())
        for g in np.flatnonzero(item >= 0):
            k = int(g) * m + int(item[g])
            if k not in seen and not band.flat[k]:                               # apart at the start and at the end, touching in between
                assert 0 < time[g] < 1, (seed, g)
                through += 1
        d.close()
    assert through >= 1


@PRECISIONS
def test_a_standing_query_is_reached_through_the_chunk_maxima(precision):
    R = REAL[precision]
    s, disp, _ = two_clusters(precision)
    w = FirstWalker(s)
    queries, qdisp, movers = arrival_queries(s, disp, R)
    (e, E), (_, E_cut) = w.table(disp), w.table(disp, whole_chunks=False)
    full, cut = w.first(queries, qdisp, disp), w.first(queries, qdisp, disp, table=(e, E_cut))
    lost = np.flatnonzero((full[1] >= 0) & (cut[1] != full[1]))                   # found only through the whole chunks' maxima
    assert len(lost) >= 1 and (full[1][lost] >= len(s.items) // 2).all()
    d = rta.DeviceScene(s)
    time, item, _, _ = assert_first(d, w, queries, qdisp, disp, "two clusters")
    assert (item[lost] == full[1][lost]).all() and (time[lost] <= 1).all()
    d.close()


def check_dynamic(d, items, live, ranges, precision, what, disp, queries, qdisp):
    """first_contacts() on dynamic scene d, which holds `items` with `live`, against FirstWalker over a fresh static scene (host side only)
    made from the live items (a dead slot is {0, 0, 0, 0}: swept_times puts it at +inf as the walk does the dead record) and bounds()."""
    R = REAL[precision]
    live = np.asarray(live) != 0
    it = np.where(live[:, None], items, 0).astype(R)
    fresh = scene_of(it, d.bounds() if ranges is not None else None, ranges, precision)
    w = FirstWalker(fresh)
    got = assert_first(d, w, queries, qdisp, disp, what)
    assert_first(d, w, queries, qdisp, disp, (what, "any"), any_hit=True)
    assert not np.isin(got[1], np.flatnonzero(~live)).any(), what
    if live.all():                                                               # ... and a fresh device scene says the same (it takes no dead slot)
        f = rta.DeviceScene(fresh)
        same_bytes(d.first_contacts(queries, qdisp, disp, normals=True), f.first_contacts(queries, qdisp, disp, normals=True))
        f.close()
    return got


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
    assert (check_dynamic(d, spheres_of(1, R), everyone, ranges, precision, "as created", fast, queries, qdisp)[1] >= 0).any()
    check_dynamic(d, spheres_of(1, R), everyone, ranges, precision, "as created, standing", None, queries, qslow)
    moved = spheres_of(2, R)
    d.update(moved)                                                              # new items, refit bounds
    check_dynamic(d, moved, everyone, ranges, precision, "update", slow, queries, qdisp)
    sp = spheres_of(3, R, spread=2.0)
    order = d.rebuild(sp)
    check_dynamic(d, sp[order], everyone, ranges, precision, "rebuild", fast, queries, qslow)
    live = (np.random.default_rng(4).random(CAPACITY) < 0.5).astype(np.uint8)
    live[:8] = 0                                                                 # two whole leaves: dead groups
    garbage = sp[order].copy()
    garbage[live == 0] = np.nan                                                  # a dead slot may hold any bits
    d.update(garbage, live=live)
    half_dead = check_dynamic(d, sp[order], live, ranges, precision, "50 % dead", slow, queries, qslow)
    huge = slow.copy()
    huge[live == 0] = R(1e15)                                                    # a dead slot's row is never used and widens no bound
    with_huge = check_dynamic(d, sp[order], live, ranges, precision, "50 % dead, their rows huge", huge, queries, qslow)
    same_bytes(half_dead[:3], with_huge[:3])
    assert with_huge[3] == half_dead[3]
    check_dynamic(d, sp[order], live, ranges, precision, "50 % dead, fast", fast, queries, qdisp)
    half = CAPACITY // 2
    order = d.rebuild(sp, n=half)
    it = np.zeros((CAPACITY, 4), R)
    it[:half] = sp[:half][order]
    check_dynamic(d, it, np.arange(CAPACITY) < half, ranges, precision, "rebuild of half", fast, queries, qdisp)
    d.rebuild(sp, n=0)                                                           # every query still walks, and the dead root culls at its one test
    time, item, st = d.first_contacts(queries, qdisp, fast, stats=True)
    assert np.isinf(time).all() and (item == -1).all() and st["sphere_tests"] == 0 and st["primary"] == len(queries) == st["bound_tests"] and st["hits"] == 0
    d.close()
    flat = rta.DeviceScene(rta.Scene(spheres_of(5, R, 40), rta.normalized(LIGHT, precision), EYE, precision=precision), 0, True)
    live = (np.arange(40) % 3 != 0).astype(np.uint8)
    items = spheres_of(6, R, 40, spread=0.4)
    flat.update(items, live=live)
    check_dynamic(flat, items, live, None, precision, "flat, a third dead", displacements(items, 13, "fast", R), queries, qdisp)
    flat.close()


def raw(d, mode, queries, qdisp, disp, time, item, normal, entry="host", exclude=None, order=None, stream=None):
    """One call of the C entry with the caller's own buffers (numpy arrays for "host", torch tensors for "device"); None: NULL."""
    ptr = lambda x: None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x.ctypes.data)
    n = len(queries)
    if entry == "host":
        capi.check(capi.lib.rt_first_contacts(d._h, mode, ptr(queries), ptr(qdisp), n, ptr(disp), ptr(exclude), ptr(order), ptr(time), ptr(item), ptr(normal), None),
                   "rt_first_contacts")
        return
    import torch
    qs = torch.cuda.current_stream() if stream is None else stream
    capi.check(capi.lib.rt_first_contacts_device(d._h, mode, ptr(queries), ptr(qdisp), n, ptr(disp), ptr(exclude), ptr(order), ptr(time), ptr(item), ptr(normal),
                                                 None, C.c_void_p(qs.cuda_stream)), "rt_first_contacts_device")
    qs.synchronize()


EDGE_SIZES = (1, 63, 64, 65, 256, 257)           # 64 lanes a wave, 256 threads a block


@PRECISIONS
def test_the_edges_of_the_launch(precision):
    import torch
    R = REAL[precision]
    s, seed = scenes(precision)["refit0"]
    d = rta.DeviceScene(s)
    w = FirstWalker(s)
    base, base_d = queries_of(s, seed, "fast", 257)
    disp = scene_disp(s, seed, "slow")
    for n in EDGE_SIZES:
        queries, qdisp = np.ascontiguousarray(base[:n]), np.ascontiguousarray(base_d[:n])
        assert_first(d, w, queries, qdisp, disp, n)
    # a wave whose queries all carry nothing, in front of one that does (the device entry: the host entry refuses such a q)
    odd = base[:130].copy()
    odd[:64, 3] = -1
    odd[64:128:2, 3] = np.nan
    ref = w.first(odd, base_d[:130], disp)
    assert ref[3]["primary"] == 34 and (ref[1] >= 0).any()
    got = d.first_contacts(torch.from_numpy(odd).cuda(), torch.from_numpy(base_d[:130].copy()).cuda(), torch.from_numpy(disp).cuda(), normals=True, stats=True)
    same_bytes(ref[:3], got[:3])
    assert counters(got[3]) == ref[3]
    nobody = odd[:64].copy()                                                      # ... and a call in which nobody carries one
    got = d.first_contacts(torch.from_numpy(nobody).cuda(), torch.from_numpy(base_d[:64].copy()).cuda(), None, normals=True, stats=True)
    assert np.isinf(got[0].cpu().numpy()).all() and (got[1].cpu().numpy() == -1).all() and not got[2].cpu().numpy().any()
    assert counters(got[3]) == {c: 0 for c in COUNTERS}
    # time_out alone: the other outputs NULL, on both entries, and nothing behind the n results is touched
    queries, qdisp = np.ascontiguousarray(base[:65]), np.ascontiguousarray(base_d[:65])
    ref = w.first(queries, qdisp, disp)
    for mode, want in ((capi.RT_SWEEP_NEAREST, ref), (capi.RT_SWEEP_ANY, w.first(queries, qdisp, disp, any_hit=True))):
        time = np.full(65 + 16, -77.0, R)
        raw(d, mode, queries, qdisp, disp, time, None, None)
        same_bytes((want[0],), (time[:65],))
        assert (time[65:] == -77.0).all()
        dev = torch.from_numpy(np.full(65 + 16, -77.0, R)).cuda()
        raw(d, mode, *(torch.from_numpy(x).cuda() for x in (queries, qdisp, disp)), dev, None, None, entry="device")
        same_bytes((time,), (dev,))
    d.close()
    # a scene of one item without bounds: the stream is that item
    one = rta.Scene(np.array([[4, 0, 0, 1]], R), rta.normalized(LIGHT, precision), EYE, precision=precision)
    d = rta.DeviceScene(one)
    time, item, normal, st = d.first_contacts(np.array([[0, 0, 0, 1], [0, 9, 0, 1]], R), np.array([[2, 0, 0], [2, 0, 0]], R), normals=True, stats=True)
    assert time.tolist() == [1.0, np.inf] and item.tolist() == [0, -1] and normal.tolist() == [[-1, 0, 0], [0, 0, 0]]
    assert (st["primary"], st["hits"], st["sphere_tests"], st["bound_tests"]) == (2, 1, 2, 0)
    assert_first(d, FirstWalker(one), np.array([[0, 0, 0, 1], [0, 9, 0, 1]], R), np.array([[2, 0, 0], [2, 0, 0]], R), None, "one item")
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
    w = FirstWalker(s)
    ref = assert_first(d, w, queries, qdisp, disp, "reference")
    calm = assert_first(d, w, queries, qslow, None, "calm")
    assert (ref[1] != calm[1]).any()
    same_bytes(ref[:2], d.first_contacts(queries, qdisp, disp))                   # with and without counters, with and without the normal
    # calls of the list entries on one scene, interleaved: each gives its own bytes
    kw = dict(times=True, normals=True, offsets=True)
    margin = float(np.median(s.items[:, 3]))
    swept = d.swept_overlaps(queries, qdisp, disp, **kw)
    touching = d.contacts(0.0, gaps=True, offsets=True)
    hitting = d.impacts(disp, times=True, offsets=True)
    over = d.overlaps(queries, margin, gaps=True, offsets=True)
    same_bytes(ref[:3], d.first_contacts(queries, qdisp, disp, normals=True))
    same_bytes(swept[:4], d.swept_overlaps(queries, qdisp, disp, **kw)[:4])       # (the table the two share: made again by each call)
    same_bytes(calm[:3], d.first_contacts(queries, qslow, None, normals=True))
    same_bytes(over[:3], d.overlaps(queries, margin, gaps=True, offsets=True)[:3])
    same_bytes(ref[:3], d.first_contacts(queries, qdisp, disp, normals=True))
    # the device entry on two streams, the list entries' device calls in between
    dq, dqd, dqs, dd, ds = (torch.from_numpy(x).cuda() for x in (queries, qdisp, qslow, disp, slow))
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    a = d.first_contacts(dq, dqd, dd, normals=True, stream=side)
    c = d.swept_overlaps(dq, dqs, ds, capacity=swept[4], stream=other)            # other motions in the same table, on another stream
    b = d.first_contacts(dq, dqs, None, normals=True, stats=True, stream=other.cuda_stream)
    k = d.impacts(dd, hitting[3], stream=other)
    o = d.overlaps(dq, margin, capacity=over[3], stream=side)
    e = d.first_contacts(dq, dqd, dd, any_hit=True, normals=True)
    t = d.contacts(0.0, capacity=touching[3], device=True, stream=side)
    f = d.first_contacts(dq, dqd, dd, normals=True, stream=other)
    side.synchronize()
    other.synchronize()
    torch.cuda.synchronize()
    for got in (a, f):
        same_bytes(ref[:3], got[:3])
    same_bytes(calm[:3], b[:3])
    assert counters(b[3]) == calm[3]
    same_bytes(w.first(queries, qdisp, disp, any_hit=True)[:3], e[:3])
    quiet = d.swept_overlaps(queries, qslow, slow)
    assert int(c[1].item()) == quiet[1] and np.array_equal(c[0].cpu().numpy()[:min(swept[4], quiet[1])], quiet[0][:swept[4]])
    assert int(k[1].item()) == hitting[3] and np.array_equal(k[0].cpu().numpy(), hitting[0])
    assert int(o[1].item()) == over[3] and np.array_equal(o[0].cpu().numpy(), over[0])
    assert int(t[1].item()) == touching[3] and np.array_equal(t[0].cpu().numpy(), touching[0])
    # pinned host buffers (read and written by the kernels directly) against pageable ones
    hb = [capi.HostBuffer(x) for x in (16 * n, 12 * n, 12 * n_items, 4 * n, 4 * n, 12 * n)]
    v = lambda k, shape: hb[k].array.view(np.float32).reshape(shape)
    pq, pqd, pd, time, item, normal = v(0, (n, 4)), v(1, (n, 3)), v(2, (n_items, 3)), v(3, n), hb[4].array.view(np.int32), v(5, (n, 3))
    pq[:], pqd[:], pd[:] = queries, qdisp, disp
    raw(d, capi.RT_SWEEP_NEAREST, pq, pqd, pd, time, item, normal)
    same_bytes(ref[:3], (time, item, normal))
    # a buffer in device memory is refused by the host entry
    ht, hi = np.zeros(n, R), np.zeros(n, np.int32)
    for args in ((dq, qdisp, disp, ht, hi, None), (queries, dqd, disp, ht, hi, None), (queries, qdisp, dd, ht, hi, None),
                 (queries, qdisp, disp, torch.zeros(n, device="cuda"), hi, None), (queries, qdisp, disp, ht, torch.zeros(n, dtype=torch.int32, device="cuda"), None),
                 (queries, qdisp, disp, ht, hi, torch.zeros(3 * n, device="cuda"))):
        with pytest.raises(rta.RtError) as err:
            raw(d, capi.RT_SWEEP_NEAREST, *args)
        assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and "device memory" in str(err.value)
    # four threads on one scene at once: two inputs, and the list entries in between
    results, errors = [None] * 4, []

    def work(t):
        try:
            for _ in range(5):
                results[t] = d.first_contacts(queries, qslow, None, normals=True) if t % 2 else d.first_contacts(queries, qdisp, disp, normals=True)
                if t == 1:
                    same_bytes(swept[:4], d.swept_overlaps(queries, qdisp, disp, **kw)[:4])
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
        same_bytes((calm if t % 2 else ref)[:3], r[:3])
    d.close()


def test_the_host_entry_refuses_motions_outside_its_domain_and_a_short_disp():
    s, seed = scenes(rta.RT_F32)["refit0"]
    d = rta.DeviceScene(s)
    n_items = len(s.items)
    queries, qdisp = queries_of(s, seed, "slow")
    for bad in (np.nan, np.inf, -np.inf, 2e15, -2e15):
        disp = np.zeros((n_items, 3), np.float32)
        disp[n_items - 1, 2] = bad                                               # the last row: the entry reads one per item slot
        with pytest.raises(rta.RtError) as err:
            d.first_contacts(queries, qdisp, disp)
        assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and " disp" in str(err.value)
        moved = qdisp.copy()
        moved[len(queries) - 1, 0] = bad
        with pytest.raises(rta.RtError) as err:
            d.first_contacts(queries, moved)
        assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and "qdisp" in str(err.value)
    for rows in (n_items - 1, n_items + 1, len(queries)):
        with pytest.raises(ValueError, match="disp"):
            d.first_contacts(queries, qdisp, np.zeros((rows, 3), np.float32))
    with pytest.raises(rta.RtError) as err:
        raw(d, 2, queries, qdisp, None, np.zeros(len(queries), np.float32), None, None)
    assert err.value.status == capi.RT_ERR_INVALID_ARGUMENT and "mode" in str(err.value)
    assert (d.first_contacts(queries, qdisp)[1] >= 0).any()                       # ... and the scene answers the next call
    d.close()


FAR = (1e15, 2.0 ** 72)


@PRECISIONS
@ANY
def test_a_far_query_that_nobody_carries_still_sets_the_scale(precision, any_hit):
    """S is folded by query index, whatever the order (tests/test_gpu_swept.py's test of the same name, for this entry): the last query
    lies far away, the device entry's `order` has a hole exactly for it, and the other queries get the bytes of the walk at the far S.
    At 1e15 (S = 2^-50) that changes one entry of the swept lists of these inputs in f32 and none that is a row's first or smallest, so
    only the counters tell the far S from the near one; at 2^72 -- the device entry checks no values, and the walk is defined for any
    bits -- seven of the 79 results are other items in f32, and the test requires that the GPU's are not the near ones.  (f64: both are
    exact scalings of a unit scene, the same bits.)  The same query with q = -1 neither counts nor walks: the near bytes come back."""
    import torch
    from tests.test_gpu_swept import far_query_inputs
    for x in FAR:
        s, far, far_d, disp, sub, S_far, S_near = far_query_inputs(precision, x)
        d = rta.DeviceScene(s)
        w = FirstWalker(s)
        n = len(far)
        want, near = w.first(sub, far_d, disp, any_hit=any_hit, S=S_far), w.first(sub, far_d, disp, any_hit=any_hit)
        differ = bool((want[1] != near[1]).any() or (bits(want[0], w.R) != bits(near[0], w.R)).any())
        assert differ == (precision == rta.RT_F32 and x != 1e15), (x, differ)
        assert (want[3] != near[3]) == (precision == rta.RT_F32), x              # (f32: the two walks differ in their tests at 1e15 already)
        order = np.arange(n, dtype=np.int32)
        order[n - 1] = n                                                         # nobody carries the far query
        dev = [torch.from_numpy(a).cuda() for a in (far, far_d, disp)]
        got = d.first_contacts(*dev, any_hit=any_hit, order=torch.from_numpy(order).cuda(), normals=True, stats=True)
        time, item, normal = (a.cpu().numpy()[:n - 1] for a in got[:3])          # (the thread without a query leaves its outputs alone)
        same_bytes((want[0][:n - 1], want[1][:n - 1], want[2][:n - 1]), (time, item, normal))
        assert counters(got[3]) == want[3] and want[3]["primary"] == n - 1 and want[3]["hits"] > 0, x
        if differ:
            assert not (np.array_equal(item, near[1][:n - 1]) and np.array_equal(bits(time, w.R), bits(near[0][:n - 1], w.R))), x
        gone = d.first_contacts(*(torch.from_numpy(a).cuda() for a in (sub, far_d, disp)), any_hit=any_hit, normals=True, stats=True)
        same_bytes(near[:3], gone[:3])
        assert counters(gone[3]) == near[3] and gone[1].cpu().numpy()[-1] == -1, x
        d.close()


LINES = [(rta.RT_F32, 65537), (rta.RT_F64, 1025)]


@pytest.mark.parametrize("precision,n", LINES, ids=["f32-65537", "f64-1025"])
def test_a_line_of_spheres_under_as_many_queries(precision, n):
    """tests/test_gpu_swept.py's line under from_spheres_balanced(leaf_size=4), as a dynamic scene -- whose bounds are refit from the items:
    the topology alone has none, and a static scene made from it is walked flat -- so the winning node's index passes 2^16 in a real
    hierarchy and the root's subtree spans hundreds of chunks of the motion table.  Every coordinate is a multiple of 0.5 below 2^17, so
    all differences are exact and a query meets only the spheres within two places of its own.  Standing scene: query g touches item g at R(3) / R(4.5) with the normal (0, 1, 0) -- v = (0, -2),
    w = (0, -1.5): a = 2.25, b = 3, cc = 3, disc = 2.25, all exact.  Moving scene: rta.swept_times over each query's five neighbours, the
    smallest time at the lowest slot (ANY: the lowest slot that touches), with rta.swept_normals' normal; no result where none touches."""
    from tests.test_gpu_swept import line
    R = REAL[precision]
    sp, disp, queries, qdisp = line(n, precision)
    d = rta.DeviceScene(rta.Scene.from_spheres_balanced(sp, leaf_size=4, precision=precision), 0, True)
    assert len(d.bounds()) > n // 4 and (d.bounds()[:, 3] > 0).all()
    for any_hit in (False, True):
        time, item, normal = d.first_contacts(queries, qdisp, None, any_hit=any_hit, normals=True)
        assert (item == np.arange(n)).all() and (bits(time, R) == bits(R(3.0) / R(4.5), R)).all() and (normal == np.array([0, 1, 0], R)).all(), any_hit
        S = rta.impact_scale(sp, disp, queries, qdisp)
        want_t, want_i, want_n = np.empty(n, R), np.empty(n, np.int32), np.empty((n, 3), R)
        for lo in range(0, n, 256):
            hi = min(n, lo + 256)
            a, b = max(0, lo - 2), min(n, hi + 2)
            t = rta.swept_times(queries[lo:hi], qdisp[lo:hi], sp[a:b], disp[a:b], None, S)
            nm = rta.swept_normals(queries[lo:hi], qdisp[lo:hi], sp[a:b], disp[a:b], None, S)
            k = np.argmax(t <= 1, axis=1) if any_hit else np.argmin(t, axis=1)  # (both: the first of equals)
            rows = np.arange(hi - lo)
            some = t[rows, k] <= 1
            want_t[lo:hi], want_i[lo:hi], want_n[lo:hi] = np.where(some, t[rows, k], R(np.inf)), np.where(some, k + a, -1), np.where(some[:, None], nm[rows, k], R(0.0))
        time, item, normal = d.first_contacts(queries, qdisp, disp, any_hit=any_hit, normals=True)
        np.testing.assert_array_equal(item, want_i, err_msg=str(any_hit))
        np.testing.assert_array_equal(bits(time, R), bits(want_t, R), err_msg=str(any_hit))
        np.testing.assert_array_equal(bits(normal, R), bits(want_n, R), err_msg=str(any_hit))
        assert (want_i < 0).any() and (want_i >= 0).any()                        # (an odd sphere leaves before its query arrives)
        if n <= 1025:                                                            # ... and the walker over the refit bounds: the counters too
            ranges = rta.balanced_ranges(n, 4)
            w = FirstWalker(scene_of(sp, d.bounds(), ranges, precision))
            for moving in (None, disp):
                assert_first(d, w, queries, qdisp, moving, (n, any_hit, moving is not None), any_hit)
    d.close()


def hand_waves(R):
    """name -> (queries, qdisp, balanced, sphere_tests (NEAREST, ANY) or None) over 300 spheres of radius 1 at (10 k, 0, 0) -- but item 101,
    which is a copy of item 100 --, for one wave of 64 queries of radius 0.25 that move by (0.5, 0, 0): towards the items behind them,
    away from those in front, whose tm is +inf."""
    lane = np.arange(64)
    col = lambda x, y: np.stack([x, y, np.zeros(64), np.full(64, 0.25)], axis=1).astype(R)
    qdisp = np.tile(np.array([0.5, 0.0, 0.0], R), (64, 1))
    at_zero = col(0.1 + 0.01 * lane, 0.01 * lane)                                # all in contact with item 0 at the start
    own = col(10.0 * lane + 0.1, 0.01 * lane)                                    # lane k in contact with item k only
    alone = at_zero.copy()
    alone[63] = (2985.0, 5.0, 0.0, 0.25)                                         # beside the far end of the line ...
    away = qdisp.copy()
    away[63] = (0.0, 1.0, 0.0)                                                   # ... and leaving: it touches nothing
    twins = col(996.0 - 0.01 * lane, 0.01 * lane)                                # 4 in front of items 100 and 101, which are one sphere ...
    reach = np.tile(np.array([6.0, 0.0, 0.0], R), (64, 1))                       # ... met at the same time inside the step: the lower slot
    every = sum(k + 1 for k in range(64))
    return {"all at item 0": (at_zero, qdisp, False, (64, 64)), "lane k at item k": (own, qdisp, False, (every, every)),
            "one lane awake": (alone, away, False, (63 + 300, 63 + 300)), "one lane awake, balanced": (alone, away, True, None),
            "twins": (twins, reach, False, (64 * 300, 64 * 101))}


@PRECISIONS
@ANY
def test_hand_built_waves_finish_where_the_walk_says(precision, any_hit):
    """One wave on a scene of 300 items without bounds, FirstWalker the reference and the counters in closed form: (a) 64 queries that all
    start in contact with item 0 -- the whole wave finishes at node 0 after 64 tests; (b) lane k in contact with item k only, +inf against
    the items before it -- sum (k + 1) tests, the wave loses a lane at every node; (c) 63 lanes as in (a) and one that touches nothing --
    one lane awake among 63 finished, 63 + 300 tests; (d) as (c) under balanced ranges with refit bounds, where the lone lane culls and its
    `resume` lies behind the node the others finish on (it stands inside the root, culls the half the others walk down, and walks the
    other half alone): the walker's counters; (e) 64 lanes that move by (6, 0, 0) and meet items 100 and 101, two copies of one sphere,
    at the same time inside the step -- the lower slot is the result, NEAREST tests all 300 items and ANY stops at the first.  The
    flavour without counters gives the same bytes."""
    R = REAL[precision]
    items = np.zeros((300, 4), R)
    items[:, 0], items[:, 3] = 10.0 * np.arange(300), 1.0
    items[101] = items[100]
    flat = rta.Scene(items, rta.normalized(LIGHT, precision), EYE, precision=precision)
    ranges = rta.balanced_ranges(len(items), 4)
    balanced = scene_of(items, rta.refit_bounds(items, ranges, precision), ranges, precision)
    for name, (queries, qdisp, tree, tests) in hand_waves(R).items():
        s = balanced if tree else flat
        d = rta.DeviceScene(s)
        w = FirstWalker(s)
        time, item, normal, st = assert_first(d, w, queries, qdisp, None, (name, any_hit), any_hit)
        if tests is not None:
            assert st["sphere_tests"] == tests[any_hit] and st["bound_tests"] == 0, (name, st)
        else:
            assert 0 < st["bound_tests"] and st["sphere_tests"] < 63 + 300, (name, st)
        if name == "lane k at item k":
            assert (item == np.arange(64)).all() and (time == 0).all(), name
        elif name == "twins":
            assert (item == 100).all() and (time > 0).all() and (time < 1).all(), name
        else:
            assert (item[:63] == 0).all() and (time[:63] == 0).all() and (item[63] == (0 if name == "all at item 0" else -1)), name
        same_bytes((time, item, normal), d.first_contacts(queries, qdisp, None, any_hit=any_hit, normals=True))
        d.close()
