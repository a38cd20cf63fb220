"""Sphere casts on the GPU (rt_sweep_spheres / rt_sweep_spheres_device, csrc/rt_sweep.hpp): the first contact of a moving
sphere with the scene, bit for bit against a restatement of the walk over the scene's node stream with rta.sweep_distances as its metric,
against brute force over all items wherever no distance grazes a cutoff, and -- with radius 0 from outside the root -- against
DeviceScene.intersect and the reference."""
import threading

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.scenes import random_nested_scene
from tests.test_gpu_multihit import node_stream
from tests.test_gpu_near import CAPACITY, LEAF, LIGHT, EYE, cases, same_bytes, scene_of, spheres_of
from tests.test_gpu_query import PREC, REAL, bits, check_nearest

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
FAMILIES = ("outside, aimed at items", "inside the root", "next to an item", "outside, aimed away")
RADII = ("0", "a quarter of the median", "0.5 - 2 medians", "half the root", "three roots")
COUNTERS = ("primary", "hits", "sphere_tests", "bound_tests", "tests_executed")


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def counters(st):
    return {c: st[c] for c in COUNTERS}


def cast_families(scene, rng, n_each=40, live=None):
    """(rays REAL[4 n_each, 6], radius REAL[4 n_each], which int[4 n_each]), family f in rows [f n_each, (f + 1) n_each): from outside the
    root (1.2 - 3 root radii) aimed at items; from inside the root in random directions; from 1.05 - 2 radii off an item's centre in
    random directions; from outside, aimed away.  Radii in turn (which = 0 .. 4): 0, a quarter of the median item radius, 0.5 - 2
    median radii, half the root radius, three root radii."""
    items = scene.items.astype(np.float64)
    if live is not None:
        items = items[np.asarray(live) != 0]
    bounds = None
    if scene.bounds is not None and len(scene.bounds):
        bounds = scene.bounds.astype(np.float64)
        bounds = bounds[bounds[:, 3] > 0]                                       # (a dead group reports {0, 0, 0, 0})
    if bounds is None or len(bounds) == 0:
        c = items[:, :3].mean(axis=0)
        bounds = np.array([[c[0], c[1], c[2], np.max(np.linalg.norm(items[:, :3] - c, axis=1) + items[:, 3])]])
    root_c, root_r = bounds[0, :3], bounds[0, 3]
    pick = lambda: items[rng.integers(0, len(items), n_each)]
    rnd = lambda: _unit(rng.normal(size=(n_each, 3)))
    outside = root_c + rnd() * root_r * rng.uniform(1.2, 3.0, (n_each, 1))
    inside = root_c + rnd() * root_r * rng.uniform(0.0, 0.9, (n_each, 1))
    s = pick()
    beside = s[:, :3] + rnd() * s[:, 3:] * rng.uniform(1.05, 2.0, (n_each, 1))
    away = root_c + rnd() * root_r * rng.uniform(1.2, 3.0, (n_each, 1))
    pos = [outside, inside, beside, away]
    dirs = [_unit(pick()[:, :3] - outside), rnd(), rnd(), _unit(away - root_c)]
    R = REAL[scene.precision]
    rays = np.ascontiguousarray(np.concatenate([np.concatenate(pos), np.concatenate(dirs)], axis=1).astype(R))
    n = len(rays)
    which = (np.arange(n) + rng.integers(0, 5)) % 5
    med = np.median(items[:, 3])
    radius = np.choose(which, [np.zeros(n), np.full(n, 0.25 * med), rng.uniform(0.5, 2.0, n) * med, np.full(n, 0.5 * root_r),
                               np.full(n, 3.0 * root_r)]).astype(R)
    return rays, np.ascontiguousarray(radius), which


def two_smallest(rays, radius, spheres):
    """(first[n], slot[n], second[n]): the row minimum of sweep_distances over `spheres`, its lowest slot and the next smallest distance,
    a few rows at a time (the 100,000 spheres)."""
    R = rays.dtype.type
    first, slot, second = np.empty(len(rays), R), np.empty(len(rays), np.int32), np.full(len(rays), np.inf, R)
    for a in range(0, len(rays), 16):
        t = rta.sweep_distances(rays[a:a + 16], radius[a:a + 16], spheres)
        rows = np.arange(len(t))
        slot[a:a + 16] = np.argmin(t, axis=1)
        first[a:a + 16] = t[rows, slot[a:a + 16]]
        if t.shape[1] > 1:
            t[rows, slot[a:a + 16]] = np.inf
            second[a:a + 16] = t.min(axis=1)
    return first, slot, second


def cutoffs(rays, radius, spheres, rng):
    """tmax REAL[n]: +inf, and 0.3 - 3 times the brute-force first contact (1.0 where there is none or it is 0), about half each."""
    R = rays.dtype.type
    first = two_smallest(rays, radius, spheres)[0].astype(np.float64)
    first = np.where(np.isfinite(first) & (first > 0), first, 1.0)
    return np.where(rng.integers(0, 2, len(rays)) == 0, np.inf, first * rng.uniform(0.3, 3.0, len(rays))).astype(R)


def normals(rays, dist, item, items):
    """normalized(pos + (dir * t - c)) with the winner's centre, every operation rounded once; {0, 0, 0} without a winner."""
    R = rays.dtype.type
    hit = item >= 0
    c = items[np.where(hit, item, 0), :3]
    with np.errstate(invalid="ignore", divide="ignore"):
        x = rays[:, :3] + (rays[:, 3:] * dist[:, None] - c)
        ln = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        out = x * (R(1.0) / ln)[:, None]
    return np.where(hit[:, None], out, R(0.0)).astype(R)


def assert_reals(a, b, R, what=""):
    """The same bits, and NaN where NaN (a normal at distance 0 from the touched sphere's own centre is 0 * inf)."""
    a, b = np.asarray(a, R), np.asarray(b, R)
    nan = np.isnan(b)
    np.testing.assert_array_equal(np.isnan(a), nan, err_msg=str(what))
    np.testing.assert_array_equal(bits(a[~nan], R), bits(b[~nan], R), err_msg=str(what))


class Walker:
    """The definition of the cast walk (include/rtrace_hip.h), one cast at a time, over node_stream(s); every distance is
    rta.sweep_distances' in the scene's precision (made once for all casts and nodes: the walks of both modes share them)."""

    def __init__(self, s, rays, radius):
        R = REAL[s.precision]
        nodes = node_stream(s)
        self.bound = [x[1] for x in nodes]
        self.skip = [x[2] for x in nodes]
        self.item = [x[3] for x in nodes]
        self.rays, self.items = rays, s.items
        spheres = np.array([x[0] for x in nodes], dtype=np.float64).reshape(-1, 4).astype(R)        # (exact: they were REAL)
        self.t = [row.tolist() for row in rta.sweep_distances(rays, radius, spheres)] if len(nodes) else [[] for _ in rays]
        self.lowest = np.inf                                                     # the smallest distance any walk has tested

    def walk(self, g, tmax, any_hit, exclude=-1):
        t = self.t[g]
        best, item = float(tmax), -1
        tests_items = tests_bounds = 0
        i, n = 0, len(t)
        while i < n:
            d = t[i]
            self.lowest = min(self.lowest, d)
            if self.bound[i]:
                tests_bounds += 1
                i = self.skip[i] if d >= best else i + 1
                continue
            tests_items += 1
            if self.item[i] != exclude and not d >= best:
                best, item = d, self.item[i]
                if any_hit:
                    break
            i += 1
        return best, item, tests_items, tests_bounds

    def all(self, tmax, any_hit, exclude=None):
        return [self.walk(g, tmax[g], any_hit, -1 if exclude is None else int(exclude[g])) for g in range(len(tmax))]


def assert_walk(res, ref, w, R, what):
    dist, nrm, item, st = res
    ref_d, ref_i = np.array([x[0] for x in ref], R), np.array([x[1] for x in ref], np.int32)
    np.testing.assert_array_equal(bits(dist, R), bits(ref_d, R), err_msg=str(what))
    np.testing.assert_array_equal(item, ref_i, err_msg=str(what))
    assert_reals(nrm, normals(w.rays, ref_d, ref_i, w.items), R, what)
    assert st["sphere_tests"] == sum(x[2] for x in ref), what
    assert st["bound_tests"] == sum(x[3] for x in ref), what
    assert st["tests_executed"] == st["sphere_tests"] + st["bound_tests"], what
    assert st["primary"] == len(ref) and st["hits"] == int((ref_i >= 0).sum()), what


@PRECISIONS
def test_the_casts_restate_the_walk_bit_for_bit(precision):
    R = REAL[precision]
    rng = np.random.default_rng(71 + precision)
    for name in ("default_L3", "nested", "100k"):
        s = cases(precision)[name]
        d = rta.DeviceScene(s)
        n_each = 3 if name == "100k" else 40
        rays, radius, which = cast_families(s, rng, n_each)
        tmax = cutoffs(rays, radius, s.items, rng)
        w = Walker(s, rays, radius)
        family = np.arange(len(rays)) // n_each
        for any_hit in (False, True):
            res = d.sweep(rays, radius, tmax, any_hit=any_hit, want_stats=True)
            assert_walk(res, w.all(tmax, any_hit), w, R, (name, any_hit))
            dist, nrm, item = res[:3]
            np.testing.assert_array_equal(item >= 0, dist < tmax)
            np.testing.assert_array_equal(bits(dist[item < 0], R), bits(tmax[item < 0], R))
            assert not nrm[item < 0].any()
        dist, nrm, item = d.sweep(rays, radius)                                  # no cutoff: what is there to be touched
        d.close()
        if n_each < 40:
            continue
        for r in range(5):
            assert (item[(family == 0) & (which == r)] >= 0).any(), (name, RADII[r])             # aimed at items: contacts for every radius
        for f in range(4):
            assert (item[(family == f) & (which == 4)] >= 0).any(), (name, FAMILIES[f])          # three root radii reach from anywhere
        for r in (0, 1):
            assert (item[(family == 3) & (which == r)] < 0).any(), (name, RADII[r])              # aimed away with a small radius: misses
        for f in (1, 2):                                                         # a large sphere inside the root overlaps at its start
            for r in (3, 4):
                cell = (family == f) & (which == r)
                assert ((dist[cell] == 0) & (item[cell] >= 0)).any(), (name, FAMILIES[f], RADII[r])


def brute_force(s, rays, radius, tmax):
    """(distance[n], item[n], left_out[n]) over all items: the row minimum of sweep_distances below tmax, ties to the lowest slot; left
    out are the casts whose smallest distance lies within 1e-5 max(1, |t|) (f64: 1e-12) of tmax, or whose two smallest distances lie
    that close to each other while the smallest is > 0."""
    R = rays.dtype.type
    eps = 1e-5 if R == np.float32 else 1e-12
    first, item, second = two_smallest(rays, radius, s.items)
    hit = first < tmax
    one, two = first.astype(np.float64), second.astype(np.float64)
    with np.errstate(invalid="ignore"):
        tol = eps * np.maximum(1.0, np.abs(one))
        left_out = np.abs(one - tmax.astype(np.float64)) <= tol
        left_out |= (one > 0) & (two - one <= tol)
        left_out &= np.isfinite(one)                                             # (a cast that misses everything grazes nothing)
    return np.where(hit, first, tmax).astype(R), np.where(hit, item, -1).astype(np.int32), left_out


@PRECISIONS
def test_the_walk_is_brute_force_where_no_distance_grazes_a_cutoff(precision):
    R = REAL[precision]
    rng = np.random.default_rng(81 + precision)
    for name in (("refit", "100k") if precision == rta.RT_F64 else ("refit",)):
        s = cases(precision)[name]
        d = rta.DeviceScene(s)
        n_each = 20 if name == "100k" else 40
        rays, radius, which = cast_families(s, rng, n_each)
        tmax = cutoffs(rays, radius, s.items, rng)
        ref_d, ref_i, left_out = brute_force(s, rays, radius, tmax)
        for f, family in enumerate(FAMILIES):
            assert left_out[f * n_each:(f + 1) * n_each].sum() <= 0.05 * n_each, (name, family)
        keep = ~left_out
        dist, nrm, item, st = d.sweep(rays, radius, tmax, want_stats=True)
        np.testing.assert_array_equal(bits(dist[keep], R), bits(ref_d[keep], R), err_msg=name)
        np.testing.assert_array_equal(item[keep], ref_i[keep], err_msg=name)
        assert_reals(nrm[keep], normals(rays, ref_d, ref_i, s.items)[keep], R, name)
        assert (ref_i[keep] >= 0).any() and (ref_i[keep] < 0).any() and ((ref_d[keep] == 0) & (ref_i[keep] >= 0)).any()
        assert st["tests_executed"] < 0.5 * len(rays) * len(s.items), name      # the hierarchy culls
        d.close()


@PRECISIONS
def test_radius_0_from_outside_the_root_is_the_ray_query(precision):
    R = REAL[precision]
    rng = np.random.default_rng(91 + precision)
    for name in ("default_L3", "refit"):
        s = cases(precision)[name]
        o = oracle.Scene.from_ranges(s.items.astype(np.float64), s.bounds.astype(np.float64), s.ranges, prec=PREC[precision])
        d = s.device()
        n_each = 40
        rays, _, _ = cast_families(s, rng, n_each)
        rays = np.ascontiguousarray(np.concatenate([rays[:n_each], rays[3 * n_each:]]))            # the two families from outside the root
        n = len(rays)
        zeros = np.zeros(n, R)
        tmax = cutoffs(rays, zeros, s.items, rng)
        # the anchor's condition: every record these rays reach is missed or entered at b - sqrt(disc) > 0, and has rr > 0
        w = Walker(s, rays, zeros)
        for any_hit in (False, True):
            w.all(tmax, any_hit)
            w.all(np.full(n, np.inf, R), any_hit)
        assert w.lowest > 0
        assert (np.array([x[0][3] for x in node_stream(s)]) > 0).all()
        check_nearest(s, o, rays, tmax)                                          # DeviceScene.intersect against the reference
        for t in (tmax, None):
            for any_hit in (False, True):
                want = d.intersect(rays, t, any_hit=any_hit, want_stats=True)
                for q in (None, zeros, 0.0):
                    got = d.sweep(rays, q, t, any_hit=any_hit, want_stats=True)
                    same_bytes(want[:3], got[:3])
                    assert counters(got[3]) == counters(want[3]), (name, any_hit)
                assert (want[2] >= 0).any() and (want[2] < 0).any()
        d.close()


@PRECISIONS
def test_self_casts_and_exclude(precision):
    """Every item of the refit scene cast from its own centre with its own radius.  (In ANY mode a cast that finds nothing keeps tmax as
    its cutoff to the end, so its tests are NEAREST's and the Walker's: the excluded item among them, counted and never returned.)"""
    R = REAL[precision]
    s = cases(precision)["refit"]
    d = rta.DeviceScene(s)
    n = len(s.items)
    rng = np.random.default_rng(19)
    rays = np.ascontiguousarray(np.concatenate([s.items[:, :3].astype(np.float64), _unit(rng.normal(size=(n, 3)))], axis=1).astype(R))
    radius = np.ascontiguousarray(s.items[:, 3])
    me = np.arange(n, dtype=np.int32)
    # without exclude a cast overlaps its own sphere at its start (ANY reports some contact below tmax: only a start overlap lies below
    # the smallest positive number)
    for any_hit, tmax in ((False, None), (True, np.finfo(R).tiny)):
        dist, nrm, item = d.sweep(rays, radius, tmax, any_hit=any_hit)
        assert (dist == 0).all() and (item >= 0).all()
    w = Walker(s, rays, radius)
    t = rta.sweep_distances(rays, radius, s.items)
    t[me, me] = np.inf
    first = t.min(axis=1).astype(np.float64)
    tmax = np.where(np.arange(n) % 3 == 0, np.inf, np.where(np.isfinite(first) & (first > 0), first, 1.0) * rng.uniform(0.3, 3.0, n)).astype(R)
    for any_hit in (False, True):
        res = d.sweep(rays, radius, tmax, any_hit=any_hit, exclude=me, want_stats=True)
        assert_walk(res, w.all(tmax, any_hit, me), w, R, ("self", any_hit))
        assert not (res[2] == me).any()
    assert (res[2] >= 0).any() and (res[2] < 0).any()
    # -1 and slots outside the scene exclude nothing
    plain = d.sweep(rays, radius, tmax, want_stats=True)
    for none in (np.full(n, -1, np.int32), np.full(n, n, np.int32), np.full(n, -2 ** 31, np.int32), np.full(n, 2 ** 31 - 1, np.int32)):
        got = d.sweep(rays, radius, tmax, exclude=none, want_stats=True)
        same_bytes(plain[:3], got[:3])
        assert counters(got[3]) == counters(plain[3])
    # ANY where nothing retires early: below half the first other contact neither mode finds anything with exclude, and both make the
    # same tests; with a cutoff of 0 nothing retires with or without exclude, and the counters do not move
    quiet = np.where(np.isfinite(first) & (first > 0), 0.5 * first, 0.0).astype(R)
    a = d.sweep(rays, radius, quiet, any_hit=True, exclude=me, want_stats=True)
    b = d.sweep(rays, radius, quiet, any_hit=False, exclude=me, want_stats=True)
    assert (a[2] == -1).all() and a[3]["hits"] == 0
    assert counters(a[3]) == counters(b[3]) and a[3]["sphere_tests"] == sum(x[2] for x in w.all(quiet, True, me)) > 0
    zero = np.zeros(n, R)
    a = d.sweep(rays, radius, zero, any_hit=True, exclude=me, want_stats=True)
    b = d.sweep(rays, radius, zero, any_hit=True, want_stats=True)
    same_bytes(a[:3], b[:3])
    assert counters(a[3]) == counters(b[3]) and (b[2] == -1).all()
    d.close()


def test_any_order_gives_the_same_bytes_and_counters():
    import torch
    s = cases(rta.RT_F32)["refit"]
    d = rta.DeviceScene(s)
    rng = np.random.default_rng(13)
    rays, radius, _ = cast_families(s, rng, 80)                                  # 320 casts: two blocks, the second one partly filled
    tmax = cutoffs(rays, radius, s.items, rng)
    n = len(rays)
    exclude = rng.integers(-1, len(s.items), n).astype(np.int32)
    for any_hit in (False, True):
        ref = d.sweep(rays, radius, tmax, any_hit=any_hit, exclude=exclude, want_stats=True)
        perm = np.random.default_rng(14).permutation(n).astype(np.uint32)
        coherent = d.sphere_order(np.concatenate([rays[:, :3], np.ones((n, 1), rays.dtype)], axis=1))
        assert sorted(coherent.tolist()) == list(range(n))
        for order in (np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)[::-1], perm, coherent, perm.astype(np.int64)):
            got = d.sweep(rays, radius, tmax, any_hit=any_hit, exclude=exclude, want_stats=True, order=order)
            same_bytes(ref[:3], got[:3])
            assert counters(got[3]) == counters(ref[3])
        with pytest.raises(rta.RtError):                                         # the host entry wants a permutation
            d.sweep(rays, radius, tmax, order=np.zeros(n, np.uint32))
        # the device entry: entries >= n carry no cast, and what they would have written keeps the caller's bytes
        carried = np.random.default_rng(15).random(n) < 0.7
        partial = perm.copy()
        partial[~carried[perm]] = np.where(np.arange((~carried).sum()) % 2 == 0, n, 0xFFFFFFFF).astype(np.uint32)
        ty, tq, tt, te = (torch.from_numpy(x).cuda() for x in (rays, radius, tmax, exclude))
        out = (torch.full((n,), -77.0, dtype=torch.float32, device="cuda"), torch.full((n, 3), -77.0, dtype=torch.float32, device="cuda"),
               torch.full((n,), -77, dtype=torch.int32, device="cuda"))
        got = d.sweep(ty, tq, tt, any_hit=any_hit, exclude=te, want_stats=True, out=out,
                      order=torch.from_numpy(partial.view(np.int32)).cuda().view(torch.uint32))
        torch.cuda.synchronize()
        dist, nrm, item = (x.cpu().numpy() for x in got[:3])
        same_bytes([x[carried] for x in ref[:3]], (dist[carried], nrm[carried], item[carried]))
        assert (dist[~carried] == -77.0).all() and (nrm[~carried] == -77.0).all() and (item[~carried] == -77).all()
        part = d.sweep(*(np.ascontiguousarray(x[carried]) for x in (rays, radius, tmax)), any_hit=any_hit,
                       exclude=np.ascontiguousarray(exclude[carried]), want_stats=True)
        assert counters(got[3]) == counters(part[3])
        full = d.sweep(ty, tq, tt, any_hit=any_hit, exclude=te, want_stats=True, order=torch.from_numpy(perm.view(np.int32)).cuda())
        same_bytes(ref[:3], full[:3])
        assert counters(full[3]) == counters(ref[3])
    d.close()
    # every flavour of the walk -- precision, mode, in an order or not, counting or not -- on 65 casts: two waves, the second with one live
    # lane.  The counting unordered call is held to the host walker, the other three to its bytes and counters.
    for precision in (rta.RT_F32, rta.RT_F64):
        s = cases(precision)["refit"]
        d = rta.DeviceScene(s)
        rng = np.random.default_rng(13)
        rays, radius, _ = cast_families(s, rng, 80)
        tmax = cutoffs(rays, radius, s.items, rng)
        rays, radius, tmax = (np.ascontiguousarray(x[:65]) for x in (rays, radius, tmax))
        perm = np.random.default_rng(14).permutation(65).astype(np.uint32)
        w = Walker(s, rays, radius)
        for any_hit in (False, True):
            ref = d.sweep(rays, radius, tmax, any_hit=any_hit, want_stats=True)
            assert_walk(ref, w.all(tmax, any_hit), w, REAL[precision], ("refit, 65 casts", precision, any_hit))
            same_bytes(ref[:3], d.sweep(rays, radius, tmax, any_hit=any_hit))
            same_bytes(ref[:3], d.sweep(rays, radius, tmax, any_hit=any_hit, order=perm))
            got = d.sweep(rays, radius, tmax, any_hit=any_hit, want_stats=True, order=perm)
            same_bytes(ref[:3], got[:3])
            assert counters(got[3]) == counters(ref[3]), (precision, any_hit)
        d.close()


@PRECISIONS
def test_scenes_without_bounds_give_the_brute_force_answer(precision):
    R = REAL[precision]
    light = rta.normalized(LIGHT, precision)
    it, _, _ = random_nested_scene(3)
    nested = rta.Scene(it, light, EYE, precision=precision)
    ten = rta.Scene(it[:10], light, EYE, precision=precision)
    # exact ties: three bit-identical spheres (items 0, 2, 6), two more (1, 3) at the same distance from the origin
    ties = rta.Scene([(0.0, 0.0, 0.0, 1.0), (3.0, 0.0, 0.0, 0.5), (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, -3.0, 0.5), (0.0, 4.0, 0.0, 0.5),
                      (0.0, -3.0, 4.0, 0.5), (0.0, 0.0, 0.0, 1.0)], light, EYE, precision=precision)
    for s in (nested, ten, ties):
        d = s.device()
        rng = np.random.default_rng(17)
        rays, radius, _ = cast_families(s, rng, 12)
        tmax = cutoffs(rays, radius, s.items, rng)
        ref_d, ref_i, _ = brute_force(s, rays, radius, tmax)                     # the flat stream is never culled: no cast is left out
        dist, nrm, item, st = d.sweep(rays, radius, tmax, want_stats=True)
        np.testing.assert_array_equal(bits(dist, R), bits(ref_d, R))
        np.testing.assert_array_equal(item, ref_i)
        assert_reals(nrm, normals(rays, ref_d, ref_i, s.items), R)
        assert st["bound_tests"] == 0 and st["sphere_tests"] == len(rays) * len(s.items)
        dist, nrm, item, st = d.sweep(rays, radius, tmax, any_hit=True, want_stats=True)
        np.testing.assert_array_equal(item >= 0, ref_i >= 0)
        assert st["bound_tests"] == 0 and st["sphere_tests"] == sum(int(i) + 1 if i >= 0 else len(s.items) for i in item)
    # equal distances go to the first item in DFS order, several items at 0 included
    d = ties.device()
    ray = np.array([[0, 0, -5, 0, 0, 1]], R)
    dist, nrm, item = d.sweep(ray, 0.5)                                          # (0, 0, -3) r 0.5 is touched at t = 1, in front of the unit spheres
    assert dist[0] == 1.0 and item[0] == 3 and nrm[0].tolist() == [0.0, 0.0, -1.0]
    dist, nrm, item = d.sweep(ray, 0.5, exclude=np.array([3], np.int32))
    assert dist[0] == 3.5 and item[0] == 0
    dist, nrm, item = d.sweep(np.array([[0, 0, 0.5, 0, 0, 1]], R), 0.25)        # inside the three unit spheres
    assert dist[0] == 0 and item[0] == 0
    dist, nrm, item = d.sweep(np.array([[0, 0, 0.5, 0, 0, 1]], R), 0.25, exclude=np.array([0], np.int32))
    assert dist[0] == 0 and item[0] == 2
    dist, nrm, item = d.sweep(ray, 0.5, 1.0)                                     # strictly below tmax
    assert dist[0] == 1.0 and item[0] == -1 and not nrm.any()
    for s in (nested, ten, ties):
        s.device().close()


def check_dynamic(d, items, live, ranges, precision, what):
    """sweep() on dynamic scene d, which holds `items` with `live`, against the Walker over a fresh static scene (host side only) made from
    the live items -- a dead slot is {0, 0, 0, 0}, which sweep_distances puts at +inf as the walk does the dead record -- and bounds()."""
    R = REAL[precision]
    live = np.asarray(live) != 0
    np.testing.assert_array_equal(d.live(), live.astype(np.uint8), err_msg=what)
    it = np.where(live[:, None], items, 0).astype(R)
    fresh = scene_of(it, d.bounds() if ranges is not None else None, ranges, precision)
    rng = np.random.default_rng(23)
    rays, radius, which = cast_families(fresh, rng, 20, live=live)
    rays[0] = (0, 0, 0, 0, 0, 1)                                                 # from where the dead record's centre sits
    tmax = cutoffs(rays, radius, it, rng)
    w = Walker(fresh, rays, radius)
    dead = np.flatnonzero(~live)
    for any_hit in (False, True):
        res = d.sweep(rays, radius, tmax, any_hit=any_hit, want_stats=True)
        assert_walk(res, w.all(tmax, any_hit), w, R, (what, any_hit))
        assert not np.isin(res[2], dead).any(), (what, any_hit)
    dist, nrm, item = d.sweep(rays, radius)                                      # three root radii, no cutoff: still never a dead slot
    within = (which == 4) & (np.arange(len(rays)) // 20 != 0) & (np.arange(len(rays)) // 20 != 3)     # started inside the root or next to an item
    assert (item[within] >= 0).all() and (dist[within] == 0).all() and not np.isin(item, dead).any(), what


@PRECISIONS
def test_dynamic_and_live_scenes_answer_as_a_fresh_scene(precision):
    R = REAL[precision]
    ranges = rta.balanced_ranges(CAPACITY, LEAF)
    d = rta.DeviceScene(rta.Scene.from_spheres_balanced(spheres_of(1, R), leaf_size=LEAF, precision=precision), 0, True)
    everyone = np.ones(CAPACITY, np.uint8)
    moved = spheres_of(2, R)
    d.update(moved)
    check_dynamic(d, moved, everyone, ranges, precision, "update")
    sp = spheres_of(3, R, spread=2.0)
    order = d.rebuild(sp)
    check_dynamic(d, sp[order], everyone, ranges, precision, "rebuild")
    live = (np.random.default_rng(4).random(CAPACITY) < 0.5).astype(np.uint8)
    live[:8] = 0                                                                 # two whole leaves: dead groups
    garbage = sp[order].copy()
    garbage[live == 0] = np.nan                                                  # a dead slot may hold any bits
    d.update(garbage, live=live)
    check_dynamic(d, sp[order], live, ranges, precision, "50 % dead")
    half = CAPACITY // 2
    order = d.rebuild(sp, n=half)
    it = np.zeros((CAPACITY, 4), R)
    it[:half] = sp[:half][order]
    check_dynamic(d, it, np.arange(CAPACITY) < half, ranges, precision, "rebuild of half")
    # n = 0: every cast ends at the dead root
    d.rebuild(sp, n=0)
    assert not d.live().any() and not d.bounds().any()
    rays = np.ascontiguousarray(np.concatenate([sp[:100, :3], np.tile(np.array([[0, 0, 1]], R), (100, 1))], axis=1))
    for any_hit in (False, True):
        for q in (None, R(100.0)):
            dist, nrm, item, st = d.sweep(rays, q, any_hit=any_hit, want_stats=True)
            assert (item == -1).all() and np.isinf(dist).all() and not nrm.any()
            assert st["bound_tests"] == len(rays) and st["sphere_tests"] == 0 and st["hits"] == 0
    d.close()
    # a flat dynamic scene takes liveness too
    flat = rta.DeviceScene(rta.Scene(spheres_of(5, R, 40), rta.normalized(LIGHT, precision), EYE, precision=precision), 0, True)
    live = (np.arange(40) % 3 != 0).astype(np.uint8)
    items = spheres_of(6, R, 40)
    flat.update(items, live=live)
    check_dynamic(flat, items, live, None, precision, "flat, a third dead")
    flat.close()


@PRECISIONS
def test_batch_sizes_at_the_wave_and_block_edges(precision):
    s = cases(precision)["refit"]
    d = rta.DeviceScene(s)
    rng = np.random.default_rng(29)
    rays, radius, _ = cast_families(s, rng, 250)                                 # 1,000 casts
    tmax = cutoffs(rays, radius, s.items, rng)
    keep = rng.permutation(len(rays))                                            # (every family at the front of the batch)
    rays, radius, tmax = (np.ascontiguousarray(x[keep]) for x in (rays, radius, tmax))
    for any_hit in (False, True):
        ref = d.sweep(rays, radius, tmax, any_hit=any_hit)
        for n in (1, 63, 64, 65, 255, 256, 257):
            got = d.sweep(np.ascontiguousarray(rays[:n]), radius[:n].copy(), tmax[:n].copy(), any_hit=any_hit)
            same_bytes([x[:n] for x in ref], got)
    d.close()


@PRECISIONS
def test_any_finds_a_result_exactly_where_nearest_does(precision):
    rng = np.random.default_rng(31 + precision)
    for name in ("default_L3", "nested", "refit"):
        s = cases(precision)[name]
        d = rta.DeviceScene(s)
        rays, radius, _ = cast_families(s, rng, 40)
        tmax = cutoffs(rays, radius, s.items, rng)
        nd, nn, ni = d.sweep(rays, radius, tmax)
        ad, an, ai = d.sweep(rays, radius, tmax, any_hit=True)
        np.testing.assert_array_equal(ai >= 0, ni >= 0, err_msg=name)
        assert (ad >= nd).all() and (ad[ai >= 0] < tmax[ai >= 0]).all(), name
        assert (ai >= 0).any() and (ai < 0).any(), name
        t = rta.sweep_distances(rays, radius, s.items)                           # the reported item reproduces the distance on its own
        hit = ai >= 0
        np.testing.assert_array_equal(t[np.flatnonzero(hit), ai[hit]], ad[hit])
        d.close()


def test_entries_buffers_streams_and_threads_agree():
    import torch
    s = cases(rta.RT_F32)["default_L3"]
    d = rta.DeviceScene(s)
    rng = np.random.default_rng(3)
    rays, radius, _ = cast_families(s, rng, 75)
    tmax = cutoffs(rays, radius, s.items, rng)
    n = len(rays)
    exclude = rng.integers(-1, len(s.items), n).astype(np.int32)
    for any_hit in (False, True):
        ref = d.sweep(rays, radius, tmax, any_hit=any_hit, exclude=exclude)
        counted = d.sweep(rays, radius, tmax, any_hit=any_hit, exclude=exclude, want_stats=True)
        same_bytes(ref, counted[:3])
        # the device entry, torch tensors made on a stream of their own
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            ty, tq, tt, te = (torch.from_numpy(x).cuda() for x in (rays, radius, tmax, exclude))
            dev = d.sweep(ty, tq, tt, any_hit=any_hit, exclude=te, stream=stream)
            dev_counted = d.sweep(ty, tq, tt, any_hit=any_hit, exclude=te, stream=stream, want_stats=True)
        stream.synchronize()
        assert all(x.device.type == "cuda" for x in dev)
        same_bytes(ref, dev)
        same_bytes(ref, dev_counted[:3])
        assert counters(dev_counted[3]) == counters(counted[3])
        # a stream that is not the current one, inputs made on the current one, given as a torch stream and as a raw handle
        side = torch.cuda.Stream()
        assert side != torch.cuda.current_stream()
        ty = torch.from_numpy(rays).cuda() * 1.0
        a = d.sweep(ty, torch.from_numpy(radius).cuda(), torch.from_numpy(tmax).cuda(), any_hit=any_hit, exclude=te, stream=side)
        b = d.sweep(ty, radius, tmax, any_hit=any_hit, exclude=te, stream=side.cuda_stream)
        del ty
        side.synchronize()
        same_bytes(ref, a)
        same_bytes(ref, b)
        # one radius and one cutoff for every cast, as values; none at all
        same_bytes(d.sweep(rays, np.full(n, 0.25, np.float32), np.full(n, 2.0, np.float32), any_hit=any_hit), d.sweep(rays, 0.25, 2.0, any_hit=any_hit))
        same_bytes(d.sweep(rays, np.zeros(n, np.float32), np.full(n, np.inf, np.float32), any_hit=any_hit), d.sweep(rays, any_hit=any_hit))
        # pinned host buffers (read and written by the kernel directly) against pageable ones
        hb = [capi.HostBuffer(x) for x in (rays.nbytes, radius.nbytes, tmax.nbytes, exclude.nbytes, 4 * n, 12 * n, 4 * n)]
        py, pq, pt, pe = hb[0].array.view(np.float32).reshape(n, 6), hb[1].array.view(np.float32), hb[2].array.view(np.float32), hb[3].array.view(np.int32)
        py[:], pq[:], pt[:], pe[:] = rays, radius, tmax, exclude
        out = (hb[4].array.view(np.float32), hb[5].array.view(np.float32).reshape(n, 3), hb[6].array.view(np.int32))
        got = d.sweep(py, pq, pt, any_hit=any_hit, exclude=pe, out=out)
        assert got[0] is out[0] and got[2] is out[2]
        same_bytes(ref, got)
    # two threads on one scene at once
    ref = d.sweep(rays, radius, tmax)
    results, errors = [None] * 2, []

    def work(j):
        try:
            for _ in range(5):
                results[j] = d.sweep(rays, radius, tmax)
        except Exception as e:          # noqa: BLE001 (reported below)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for r in results:
        same_bytes(ref, r)
    d.close()


@PRECISIONS
def test_the_host_entry_rejects_casts_outside_the_domain(precision):
    R = REAL[precision]
    d = rta.Scene.three_spheres(precision).device()
    good = np.array([[0, 0, -4, 0, 0, 1]] * 4, dtype=R)
    dist, nrm, item = d.sweep(good, 0.5)
    assert (item >= 0).all() and (dist > 0).all() and np.isfinite(dist).all()

    def refused(*args, **kw):
        with pytest.raises(rta.RtError) as e:
            d.sweep(*args, **kw)
        assert e.value.status == capi.RT_ERR_INVALID_ARGUMENT

    for q in (-0.5, np.nan, np.inf, -np.inf, 2e15):
        refused(good, np.array([0.5, 0.5, q, 0.5], dtype=R))
    bad = good.copy()
    bad[2, 3:] = (0, 0, 1.5)                                                     # no unit vector
    refused(bad, 0.5)
    bad = good.copy()
    bad[2, 3:] = 0
    refused(bad, 0.5)
    for c, v in ((1, 2e15), (0, -2e15), (2, np.inf), (4, np.nan)):
        bad = good.copy()
        bad[2, c] = v
        refused(bad, 0.5)
    refused(good, 0.5, np.array([1, np.nan, 1, 1], dtype=R))
    # every other cutoff is valid: at or below 0 nothing is found; the largest radius of the domain overlaps everything
    dist, nrm, item = d.sweep(good, 0.5, np.array([0, -1, -np.inf, np.inf], dtype=R))
    assert item[:3].tolist() == [-1, -1, -1] and item[3] >= 0 and dist[:3].tolist() == [0, -1, -np.inf]
    dist, nrm, item = d.sweep(good, 1e15)
    assert (dist == 0).all() and (item == 0).all()
    d.close()
