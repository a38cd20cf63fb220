"""The calls DeviceScene's wrappers make into the library, without a GPU and without the library: capi.lib is replaced by a stand-in that
records every call -- the entry's name, its arguments, and the bytes behind the pointers it is told to read while the call is in progress
-- writes a chosen total through a byref(c_uint64) argument and returns RT_OK.  Held here, through the numpy side of every wrapper: which
entry is called and how often, which arguments are NULL, the integers, the bytes of the staged inputs (a scalar radius / tmax rounded and
broadcast, an order cast to uint32, exclude as int32), and the shapes and dtypes of everything returned.  Every expectation is written
out below; none comes from the code under test."""
import ctypes as C

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from rust_tracer_amd.scene import DeviceScene

N, ITEMS, GROUPS, TOTAL = 3, 7, 2, 5
PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])


class _Recorder:
    """Stands in for capi.lib: any attribute is an entry that returns RT_OK.  snap[entry] = {argument index: bytes to copy from that pointer
    during the call}; fill[entry] = {argument index: bytes to write to that pointer}; every byref(c_uint64) argument receives `total`."""

    def __init__(self, real, total=TOTAL):
        self.real, self.calls, self.total, self.snap, self.fill = real, [], total, {}, {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if name == "rt_scene_destroy":                                           # (a scene of another test, collected while this one runs)
            return getattr(self.real, name)

        def entry(*args):
            seen = {i: C.string_at(args[i], nbytes) for i, nbytes in self.snap.get(name, {}).items() if args[i] is not None}
            for a in args:
                if isinstance(getattr(a, "_obj", None), C.c_uint64):
                    a._obj.value = self.total
            for i, data in self.fill.get(name, {}).items():
                C.memmove(args[i], data, len(data))
            self.calls.append((name, args, seen))
            return capi.RT_OK
        return entry

    def take(self):
        calls, self.calls = self.calls, []
        return calls


class _Handle:
    """An rt_scene* that DeviceScene.close() leaves alone."""
    def __bool__(self):
        return False


class _Stand:
    def __init__(self, precision):
        self.precision = precision
        self.items = np.zeros((ITEMS, 4), np.float32 if precision == rta.RT_F32 else np.float64)


@pytest.fixture
def lib(monkeypatch):
    rec = _Recorder(capi.lib)
    monkeypatch.setattr(capi, "lib", rec)
    return rec


def _device_scene(precision):
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h, d._n_bounds = _Stand(precision), 0, _Handle(), GROUPS
    return d


def _real(precision):
    return np.float32 if precision == rta.RT_F32 else np.float64


def _is_stats(a):
    return isinstance(getattr(a, "_obj", None), capi.Stats)


def _nulls(args):
    return [i for i, a in enumerate(args) if a is None]


def _shapes(res):
    return [(a.shape, a.dtype) for a in res]


def _inputs(R):
    rng = np.random.default_rng(11)
    rays = rng.standard_normal((N, 6)).astype(R)
    points = rng.standard_normal((N, 3)).astype(R)
    queries = np.abs(rng.standard_normal((N, 4))).astype(R)
    return rays, points, queries


ORDER = [2, 0, 1]
ORDER_BYTES = np.array(ORDER, np.uint32).tobytes()
EXCLUDE = np.array([4, -1, 6], np.int32)


@PRECISIONS
def test_intersect_and_intersect_multi(lib, precision):
    R, d = _real(precision), _device_scene(precision)
    rays = _inputs(R)[0]
    w = rays.itemsize
    fixed = [((N,), R), ((N, 3), R), ((N,), np.int32)]
    # no option: the plain entry, tmax NULL, stats NULL
    lib.snap = {"rt_intersect_rays": {2: rays.nbytes}}
    res = d.intersect(rays)
    (name, args, seen), = lib.take()
    assert name == "rt_intersect_rays" and len(args) == 9 and args[0] is d._h
    assert (args[1], args[4]) == (capi.RT_QUERY_NEAREST, N) and _nulls(args) == [3, 8]
    assert seen[2] == rays.tobytes()
    assert isinstance(res, tuple) and _shapes(res) == fixed
    assert [args[5], args[6], args[7]] == [a.ctypes.data for a in res]
    # a rounded, broadcast tmax; occlusion; counters; a rays array that is not contiguous is staged
    lib.snap = {"rt_intersect_rays": {2: rays.nbytes, 3: N * w}}
    res = d.intersect(np.asfortranarray(rays), tmax=0.1, any_hit=True, want_stats=True)
    (name, args, seen), = lib.take()
    assert name == "rt_intersect_rays" and (args[1], args[4]) == (capi.RT_QUERY_ANY, N) and _nulls(args) == [] and _is_stats(args[8])
    assert seen[2] == rays.tobytes() and seen[3] == np.full(N, 0.1, R).tobytes()
    assert len(res) == 4 and _shapes(res[:3]) == fixed and set(res[3]) == {n for n, _ in capi.Stats._fields_}
    # tmax per ray, of the scene's REAL: as given
    tm = np.array([1.5, 2.5, 0.1], R)
    d.intersect(rays, tmax=tm)
    (name, args, seen), = lib.take()
    assert seen[3] == tm.tobytes()
    # an order: the _ordered entry, whose order pointer follows n -- NULL for True, uint32 indices otherwise
    for order, want in ((True, None), (ORDER, ORDER_BYTES), (np.array(ORDER, np.int64), ORDER_BYTES)):
        lib.snap = {"rt_intersect_rays_ordered": {5: 4 * N}}
        res = d.intersect(rays, order=order)
        (name, args, seen), = lib.take()
        assert name == "rt_intersect_rays_ordered" and len(args) == 10 and (args[1], args[4]) == (0, N)
        assert _nulls(args) == ([3, 5, 9] if want is None else [3, 9])
        assert seen.get(5) == want and _shapes(res) == fixed
    # out: filled in place
    out = (np.empty(N, R), np.empty((N, 3), R), np.empty(N, np.int32))
    res = d.intersect(rays, out=out)
    (name, args, seen), = lib.take()
    assert all(a is b for a, b in zip(res, out)) and [args[5], args[6], args[7]] == [a.ctypes.data for a in out]
    # the k closest
    k = 4
    multi = [((N, k), R), ((N, k, 3), R), ((N, k), np.int32), ((N,), np.uint32)]
    lib.snap = {"rt_intersect_rays_multi": {3: rays.nbytes, 4: N * w}}
    res = d.intersect_multi(rays, k, tmax=np.float64(0.1))
    (name, args, seen), = lib.take()
    assert name == "rt_intersect_rays_multi" and len(args) == 11 and args[0] is d._h
    assert (args[1], args[2], args[5]) == (capi.RT_MULTIHIT_CLOSEST, k, N) and _nulls(args) == [10]
    assert seen[3] == rays.tobytes() and seen[4] == np.full(N, 0.1, R).tobytes()
    assert _shapes(res) == multi and [args[6], args[7], args[8], args[9]] == [a.ctypes.data for a in res]
    lib.snap = {"rt_intersect_rays_multi_ordered": {6: 4 * N}}
    res = d.intersect_multi(rays, k, all_hits=True, want_stats=True, order=ORDER)
    (name, args, seen), = lib.take()
    assert name == "rt_intersect_rays_multi_ordered" and len(args) == 12
    assert (args[1], args[2], args[5]) == (capi.RT_MULTIHIT_ALL, k, N) and _nulls(args) == [4] and _is_stats(args[11])
    assert seen[6] == ORDER_BYTES and len(res) == 5 and _shapes(res[:4]) == multi
    d.intersect_multi(rays, k, order=True)
    (name, args, seen), = lib.take()
    assert name == "rt_intersect_rays_multi_ordered" and _nulls(args) == [4, 6, 11]


@PRECISIONS
def test_trace(lib, precision):
    R, d = _real(precision), _device_scene(precision)
    rays = _inputs(R)[0]
    shapes = [((N, 3), R), ((N,), R)]
    lib.snap = {"rt_trace_rays": {1: rays.nbytes}}
    res = d.trace(rays)
    (name, args, seen), = lib.take()
    assert name == "rt_trace_rays" and len(args) == 6 and args[0] is d._h and args[2] == N and _nulls(args) == [5]
    assert seen[1] == rays.tobytes() and isinstance(res, tuple) and _shapes(res) == shapes
    assert [args[3], args[4]] == [a.ctypes.data for a in res]
    res = d.trace(rays, want_stats=True)
    (name, args, seen), = lib.take()
    assert _is_stats(args[5]) and len(res) == 3 and _shapes(res[:2]) == shapes and isinstance(res[2], dict)
    for order, want in ((True, None), (ORDER, ORDER_BYTES)):
        lib.snap = {"rt_trace_rays_ordered": {3: 4 * N}}
        res = d.trace(rays, order=order)
        (name, args, seen), = lib.take()
        assert name == "rt_trace_rays_ordered" and len(args) == 7 and args[2] == N
        assert _nulls(args) == ([3, 6] if want is None else [6]) and seen.get(3) == want and _shapes(res) == shapes
    out = (np.empty((N, 3), R), np.empty(N, R))
    res = d.trace(rays, out=out)
    (name, args, seen), = lib.take()
    assert res[0] is out[0] and res[1] is out[1] and [args[3], args[4]] == [a.ctypes.data for a in out]


@PRECISIONS
def test_near_and_sweep(lib, precision):
    R, d = _real(precision), _device_scene(precision)
    rays, points, _ = _inputs(R)
    w, k = rays.itemsize, 4
    near = [((N, k), R), ((N, k), np.int32), ((N,), np.uint32)]
    # near: the order pointer is always there
    lib.snap = {"rt_near_spheres": {3: points.nbytes}}
    res = d.near(points, k)
    (name, args, seen), = lib.take()
    assert name == "rt_near_spheres" and len(args) == 12 and args[0] is d._h
    assert (args[1], args[2], args[5]) == (capi.RT_NEAR_CLOSEST, k, N) and _nulls(args) == [4, 6, 7, 11]
    assert seen[3] == points.tobytes() and isinstance(res, tuple) and _shapes(res) == near
    assert [args[8], args[9], args[10]] == [a.ctypes.data for a in res]
    lib.snap = {"rt_near_spheres": {3: points.nbytes, 4: N * w, 6: 4 * N, 7: 4 * N}}
    res = d.near(points, k, radius=0.1, all_within=True, exclude=EXCLUDE, want_stats=True, order=ORDER)
    (name, args, seen), = lib.take()
    assert (args[1], args[2], args[5]) == (capi.RT_NEAR_ALL, k, N) and _nulls(args) == [] and _is_stats(args[11])
    assert seen[4] == np.full(N, 0.1, R).tobytes() and seen[6] == EXCLUDE.tobytes() and seen[7] == ORDER_BYTES
    assert len(res) == 4 and _shapes(res[:3]) == near and isinstance(res[3], dict)
    radius = np.array([0.5, 0.1, 2.0], R)
    d.near(points, k, radius=radius)
    (name, args, seen), = lib.take()
    assert seen[4] == radius.tobytes()
    out = tuple(np.empty(shape, dt) for shape, dt in near)
    res = d.near(points, k, out=out)
    (name, args, seen), = lib.take()
    assert all(a is b for a, b in zip(res, out)) and [args[8], args[9], args[10]] == [a.ctypes.data for a in out]
    with pytest.raises(ValueError, match="order"):                               # near and sweep take indices only
        d.near(points, k, order=True)
    assert lib.take() == []
    # sweep
    sweep = [((N,), R), ((N, 3), R), ((N,), np.int32)]
    lib.snap = {"rt_sweep_spheres": {2: rays.nbytes}}
    res = d.sweep(rays)
    (name, args, seen), = lib.take()
    assert name == "rt_sweep_spheres" and len(args) == 12 and args[0] is d._h
    assert (args[1], args[5]) == (capi.RT_SWEEP_NEAREST, N) and _nulls(args) == [3, 4, 6, 7, 11]
    assert seen[2] == rays.tobytes() and isinstance(res, tuple) and _shapes(res) == sweep
    assert [args[8], args[9], args[10]] == [a.ctypes.data for a in res]
    lib.snap = {"rt_sweep_spheres": {3: N * w, 4: N * w, 6: 4 * N, 7: 4 * N}}
    res = d.sweep(rays, radius=0.3, tmax=0.1, any_hit=True, exclude=EXCLUDE, order=np.array(ORDER, np.int32), want_stats=True)
    (name, args, seen), = lib.take()
    assert (args[1], args[5]) == (capi.RT_SWEEP_ANY, N) and _nulls(args) == [] and _is_stats(args[11])
    assert seen[3] == np.full(N, 0.3, R).tobytes() and seen[4] == np.full(N, 0.1, R).tobytes()
    assert seen[6] == EXCLUDE.tobytes() and seen[7] == ORDER_BYTES
    assert len(res) == 4 and _shapes(res[:3]) == sweep and isinstance(res[3], dict)
    lib.snap = {"rt_sweep_spheres": {4: N * w}}
    d.sweep(rays, tmax=radius)                                                      # radius NULL, tmax per cast
    (name, args, seen), = lib.take()
    assert _nulls(args) == [3, 6, 7, 11] and seen[4] == radius.tobytes()
    out = tuple(np.empty(shape, dt) for shape, dt in sweep)
    res = d.sweep(rays, out=out)
    (name, args, seen), = lib.take()
    assert all(a is b for a, b in zip(res, out)) and [args[8], args[9], args[10]] == [a.ctypes.data for a in out]
    with pytest.raises(ValueError, match="order"):
        d.sweep(rays, order=True)
    assert lib.take() == []


def _list_calls(lib, entry, capacity, call, cap_at, outs_at, total_at):
    """Runs `call` and holds the count-then-fill shape of a list query: with capacity None a counting call (capacity 0, no list, no stats)
    and then one for `total` entries; with a capacity one call, whose list pointers are NULL when it is 0 -> (result, the last call's args,
    what the first call saw, m)."""
    res = call()
    calls = lib.take()
    calls = [c for c in calls if c[0] != "rt_sphere_order"]
    assert [c[0] for c in calls] == [entry] * (2 if capacity is None else 1)
    if capacity is None:
        first = calls[0][1]
        assert first[cap_at] == 0 and all(first[i] is None for i in outs_at) and first[-1] is None
        assert isinstance(first[total_at]._obj, C.c_uint64)
        assert first[:cap_at] == calls[1][1][:cap_at]                                # the same inputs both times
    args = calls[-1][1]
    want = TOTAL if capacity is None else capacity
    assert args[cap_at] == want and isinstance(args[total_at]._obj, C.c_uint64)
    return res, args, calls[0][2], min(want, TOTAL)


@PRECISIONS
@pytest.mark.parametrize("capacity", [None, 0, 2])
def test_contacts_and_impacts(lib, precision, capacity):
    R, d = _real(precision), _device_scene(precision)
    # contacts(margin, capacity, pairs, gap, offsets, total, stats)
    res, args, _, m = _list_calls(lib, "rt_scene_contacts", capacity, lambda: d.contacts(0.25, capacity), 2, (3, 4, 5), 6)
    assert len(args) == 8 and args[0] is d._h and args[1] == 0.25 and _nulls(args) == ([4, 5, 7] if m else [3, 4, 5, 7])
    assert _shapes(res[:1]) == [((m, 2), np.int32)] and res[1:] == (TOTAL,) and type(res[1]) is int
    res, args, _, m = _list_calls(lib, "rt_scene_contacts", capacity,
                                  lambda: d.contacts(np.inf, capacity, gaps=True, offsets=True, stats=True), 2, (3, 4, 5), 6)
    assert args[1] == float("inf") and _nulls(args) == ([] if m else [3, 4]) and _is_stats(args[7])
    assert len(res) == 5 and _shapes(res[:3]) == [((m, 2), np.int32), ((m,), R), ((ITEMS + 1,), np.uint64)]
    assert res[3] == TOTAL and isinstance(res[4], dict) and args[5] == res[2].ctypes.data
    # impacts(disp, capacity, pairs, time, offsets, total, stats)
    disp = np.random.default_rng(5).standard_normal((ITEMS, 3)).astype(R)
    lib.snap = {"rt_scene_impacts": {1: disp.nbytes}}
    res, args, seen, m = _list_calls(lib, "rt_scene_impacts", capacity, lambda: d.impacts(disp, capacity), 2, (3, 4, 5), 6)
    assert len(args) == 8 and args[0] is d._h and _nulls(args) == ([4, 5, 7] if m else [3, 4, 5, 7]) and seen[1] == disp.tobytes()
    assert _shapes(res[:1]) == [((m, 2), np.int32)] and res[1:] == (TOTAL,) and type(res[1]) is int
    if capacity == 0:
        with pytest.raises(ValueError, match="times"):
            d.impacts(disp, 0, times=True)
        assert lib.take() == []
        res, args, seen, m = _list_calls(lib, "rt_scene_impacts", 0, lambda: d.impacts(disp, 0, offsets=True, stats=True), 2, (3, 4, 5), 6)
        assert _nulls(args) == [3, 4] and _shapes(res[:2]) == [((0, 2), np.int32), ((ITEMS + 1,), np.uint64)] and res[2] == TOTAL
    else:
        res, args, seen, m = _list_calls(lib, "rt_scene_impacts", capacity,
                                         lambda: d.impacts(disp, capacity, times=True, offsets=True, stats=True), 2, (3, 4, 5), 6)
        assert _nulls(args) == [] and _is_stats(args[7])
        assert len(res) == 5 and _shapes(res[:3]) == [((m, 2), np.int32), ((m,), R), ((ITEMS + 1,), np.uint64)]
        assert res[3] == TOTAL and isinstance(res[4], dict)


@PRECISIONS
@pytest.mark.parametrize("capacity", [None, 0, 2])
def test_overlaps_and_swept_overlaps(lib, precision, capacity):
    R, d = _real(precision), _device_scene(precision)
    queries = _inputs(R)[2]
    rng = np.random.default_rng(6)
    qdisp, disp = rng.standard_normal((N, 3)).astype(R), rng.standard_normal((ITEMS, 3)).astype(R)
    unit = queries.copy()
    unit[:, 3] = 1
    # overlaps(queries, n, margin, exclude, order, capacity, items, gap, offsets, total, stats)
    lib.snap = {"rt_overlap_spheres": {1: queries.nbytes}}
    res, args, seen, m = _list_calls(lib, "rt_overlap_spheres", capacity, lambda: d.overlaps(queries, capacity=capacity), 6, (7, 8, 9), 10)
    assert len(args) == 12 and args[0] is d._h and (args[2], args[3]) == (N, 0.0)
    assert _nulls(args) == ([4, 5, 8, 9, 11] if m else [4, 5, 7, 8, 9, 11]) and seen[1] == queries.tobytes()
    assert _shapes(res[:1]) == [((m,), np.int32)] and res[1:] == (TOTAL,) and type(res[1]) is int
    lib.snap = {"rt_overlap_spheres": {4: 4 * N, 5: 4 * N}}
    res, args, seen, m = _list_calls(lib, "rt_overlap_spheres", capacity,
                                     lambda: d.overlaps(queries, -0.5, exclude=EXCLUDE, order=ORDER, capacity=capacity, gaps=True, offsets=True,
                                                        stats=True), 6, (7, 8, 9), 10)
    assert args[3] == -0.5 and _nulls(args) == ([] if m else [7, 8]) and _is_stats(args[11])
    assert seen[4] == EXCLUDE.tobytes() and seen[5] == ORDER_BYTES
    assert len(res) == 5 and _shapes(res[:3]) == [((m,), np.int32), ((m,), R), ((N + 1,), np.uint64)] and res[3] == TOTAL and isinstance(res[4], dict)
    # order=True: the sphere order of the queries with unit radii, taken first
    lib.snap = {"rt_sphere_order": {1: unit.nbytes}, "rt_overlap_spheres": {5: 4 * N}}
    lib.fill = {"rt_sphere_order": {3: ORDER_BYTES}}
    d.overlaps(queries, order=True, capacity=capacity)
    calls = lib.take()
    assert [c[0] for c in calls] == ["rt_sphere_order"] + ["rt_overlap_spheres"] * (2 if capacity is None else 1)
    assert calls[0][1][2] == N and _nulls(calls[0][1]) == [] and calls[0][2][1] == unit.tobytes()
    assert all(c[2][5] == ORDER_BYTES for c in calls[1:])
    # swept_overlaps(queries, qdisp, n, disp, exclude, order, capacity, items, time, normal, offsets, total, stats)
    lib.snap = {"rt_swept_overlaps": {1: queries.nbytes, 2: qdisp.nbytes}}
    res, args, seen, m = _list_calls(lib, "rt_swept_overlaps", capacity, lambda: d.swept_overlaps(queries, qdisp, capacity=capacity), 7, (8, 9, 10, 11), 12)
    assert len(args) == 14 and args[0] is d._h and args[3] == N
    assert _nulls(args) == ([4, 5, 6, 9, 10, 11, 13] if m else [4, 5, 6, 8, 9, 10, 11, 13])
    assert seen[1] == queries.tobytes() and seen[2] == qdisp.tobytes()
    assert _shapes(res[:1]) == [((m,), np.int32)] and res[1:] == (TOTAL,) and type(res[1]) is int
    if capacity == 0:
        with pytest.raises(ValueError, match="times and normals"):
            d.swept_overlaps(queries, qdisp, capacity=0, normals=True)
        assert lib.take() == []
        return
    lib.snap = {"rt_swept_overlaps": {4: disp.nbytes, 5: 4 * N, 6: 4 * N}}
    res, args, seen, m = _list_calls(lib, "rt_swept_overlaps", capacity,
                                     lambda: d.swept_overlaps(queries, qdisp, disp, exclude=EXCLUDE, order=np.array(ORDER, np.uint32), capacity=capacity,
                                                              times=True, normals=True, offsets=True, stats=True), 7, (8, 9, 10, 11), 12)
    assert _nulls(args) == [] and _is_stats(args[13])
    assert seen[4] == disp.tobytes() and seen[5] == EXCLUDE.tobytes() and seen[6] == ORDER_BYTES
    assert len(res) == 6 and _shapes(res[:4]) == [((m,), np.int32), ((m,), R), ((m, 3), R), ((N + 1,), np.uint64)]
    assert res[4] == TOTAL and isinstance(res[5], dict)
    lib.snap = {"rt_sphere_order": {1: unit.nbytes}, "rt_swept_overlaps": {6: 4 * N}}
    d.swept_overlaps(queries, qdisp, order=True, capacity=capacity, normals=True)
    calls = lib.take()
    assert [c[0] for c in calls] == ["rt_sphere_order"] + ["rt_swept_overlaps"] * (2 if capacity is None else 1)
    assert calls[0][2][1] == unit.tobytes() and all(c[2][6] == ORDER_BYTES for c in calls[1:])
    assert _nulls(calls[-1][1]) == [4, 5, 9, 11, 13]


@PRECISIONS
def test_orders_rebuild_and_update(lib, precision):
    R, d = _real(precision), _device_scene(precision)
    rays = _inputs(R)[0]
    rng = np.random.default_rng(7)
    spheres = np.abs(rng.standard_normal((ITEMS, 4))).astype(R)
    perm = np.array([3, 1, 0, 6, 5, 2, 4], np.uint32)
    # ray_order(rays, n, order_out)
    lib.snap, lib.fill = {"rt_ray_order": {1: rays.nbytes}}, {"rt_ray_order": {3: ORDER_BYTES}}
    order = d.ray_order(rays)
    (name, args, seen), = lib.take()
    assert name == "rt_ray_order" and len(args) == 4 and args[0] is d._h and args[2] == N and _nulls(args) == []
    assert seen[1] == rays.tobytes() and (order.shape, order.dtype) == ((N,), np.uint32) and order.tolist() == ORDER
    # sphere_order(spheres, n, order_out): any n
    for n in (ITEMS, 2):
        lib.snap, lib.fill = {"rt_sphere_order": {1: 4 * n * rays.itemsize}}, {"rt_sphere_order": {3: perm[:n].tobytes()}}
        order = d.sphere_order(spheres[:n])
        (name, args, seen), = lib.take()
        assert name == "rt_sphere_order" and len(args) == 4 and args[0] is d._h and args[2] == n and _nulls(args) == []
        assert seen[1] == spheres[:n].tobytes() and (order.shape, order.dtype) == ((n,), np.uint32) and order.tolist() == perm[:n].tolist()
    # rebuild(spheres, order_out)
    lib.snap, lib.fill = {"rt_scene_rebuild": {1: spheres.nbytes}}, {"rt_scene_rebuild": {2: perm.tobytes()}}
    order = d.rebuild(spheres)
    (name, args, seen), = lib.take()
    assert name == "rt_scene_rebuild" and len(args) == 3 and args[0] is d._h and _nulls(args) == []
    assert seen[1] == spheres.tobytes() and (order.shape, order.dtype) == ((ITEMS,), np.uint32) and order.tolist() == perm.tolist()
    # rebuild of the first n (spheres, n, order_out); n = 0 reads and writes nothing
    lib.snap = {"rt_scene_rebuild_n": {1: 3 * 4 * rays.itemsize}}
    order = d.rebuild(spheres, n=3)
    (name, args, seen), = lib.take()
    assert name == "rt_scene_rebuild_n" and len(args) == 4 and args[0] is d._h and args[2] == 3 and _nulls(args) == []
    assert seen[1] == spheres[:3].tobytes() and (order.shape, order.dtype) == ((3,), np.uint32)
    order = d.rebuild(spheres, n=0)
    (name, args, seen), = lib.take()
    assert name == "rt_scene_rebuild_n" and args[2] == 0 and _nulls(args) == [1, 3] and (order.shape, order.dtype) == ((0,), np.uint32)
    # update(items, bounds or NULL); with live, the _live entry (items, bounds or NULL, live as bytes)
    bounds = np.abs(rng.standard_normal((GROUPS, 4))).astype(R)
    lib.snap = {"rt_scene_update": {1: spheres.nbytes, 2: bounds.nbytes}}
    assert d.update(spheres) is None
    (name, args, seen), = lib.take()
    assert name == "rt_scene_update" and len(args) == 3 and args[0] is d._h and _nulls(args) == [2] and seen[1] == spheres.tobytes()
    assert d.update(spheres, bounds) is None
    (name, args, seen), = lib.take()
    assert name == "rt_scene_update" and _nulls(args) == [] and seen[1] == spheres.tobytes() and seen[2] == bounds.tobytes()
    live = np.array([1, 0, 1, 1, 0, 0, 1], np.uint8)
    lib.snap = {"rt_scene_update_live": {1: spheres.nbytes, 2: bounds.nbytes, 3: ITEMS}}
    for lv in (live, live.astype(bool)):
        assert d.update(spheres, live=lv) is None
        (name, args, seen), = lib.take()
        assert name == "rt_scene_update_live" and len(args) == 4 and args[0] is d._h and _nulls(args) == [2]
        assert seen[1] == spheres.tobytes() and seen[3] == live.tobytes()
    assert d.update(spheres, bounds, live=live) is None
    (name, args, seen), = lib.take()
    assert name == "rt_scene_update_live" and _nulls(args) == [] and seen[2] == bounds.tobytes() and seen[3] == live.tobytes()
