"""Traced rays and camera frames on the GPU (rt_trace_rays* / rt_render_camera*, csrc/rt_trace.hpp): the identity camera against the render
(bytes and counters), any camera and any ray bit for bit against a restatement of render.rs over the oracle's intersect, and every entry,
buffer kind, stream and thread giving the same bytes."""
import threading

import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests import util
from tests.scenes import random_nested_scene
from tests.test_gpu_query import camera_rays, ray_families

pytestmark = pytest.mark.gpu

PREC = {rta.RT_F32: oracle.F32, rta.RT_F64: oracle.F64}
REAL = {rta.RT_F32: np.float32, rta.RT_F64: np.float64}
SKIP, FLAT = rta.RT_TRAVERSAL_SKIP, rta.RT_TRAVERSAL_FLAT
COUNTERS = ("primary", "hits", "shadow", "occluded", "sphere_tests", "bound_tests", "primary_tests")
MISS, AMBIENT, LIT, SHADOWED = 0, 1, 2, 3


def identity(s):
    R = REAL[s.precision]
    return np.concatenate([s.eye, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=R)]).astype(R)


# ---- the restatement: render.rs:171-255 for a camera, in numpy REAL arithmetic over the oracle's intersect ----

def camera_sample_rays(w, h, spp, xs, ys, ssx, ssy, cam, R):
    """The camera formula of include/rtrace_hip.h for samples (ssx, ssy) of pixels (xs, ys) -> REAL[n, 6]."""
    ssf = R(spp)
    xres = xs.astype(R) + R(ssx) / ssf
    yres = ys.astype(R) + R(ssy) / ssf
    u = xres - R(w) / R(2)
    v = (R(h) - yres) - R(h) / R(2)
    f = R(w)
    c = cam.astype(R)
    d = [(c[3 + k] * u + c[6 + k] * v) + c[9 + k] * f for k in range(3)]
    inv = R(1) / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    out = np.empty((len(xs), 6), dtype=R)
    out[:, :3] = c[:3]
    for k in range(3):
        out[:, 3 + k] = d[k] * inv
    return out


def restate_rays(o, mode, rays, light, R):
    """raytrace() per ray: (exit, n.light) -- the oracle's nearest hit, the shading of render.rs:190-199, the shadow ray's any hit."""
    state, gdot = np.zeros(len(rays), dtype=np.uint8), np.zeros(len(rays), dtype=R)
    k_eps = R(np.sqrt(R(np.finfo(R).eps)))
    for k, r in enumerate(rays):
        d, nrm = o.intersect(r.astype(np.float64), float("inf"), mode)
        if not d < float("inf"):
            continue
        d, n = R(d), np.asarray(nrm).astype(R)
        g = (n[0] * light[0] + n[1] * light[1]) + n[2] * light[2]
        gdot[k] = g
        if g >= R(0):
            state[k] = AMBIENT
            continue
        p = (r[:3] + r[3:] * d) + n * (d * k_eps)
        sd, _ = o.intersect(np.concatenate([p, -light]).astype(np.float64), float("inf"), mode)
        state[k] = SHADOWED if sd < float("inf") else LIT
    return state, gdot


def accumulate(g, alpha, state, gdot, R):
    """*c = *c + ... for each exit (render.rs:191-213), element by element; alpha += the return value."""
    obj = np.array([0xae, 0x31, 0x31], dtype=R) / R(255)
    bg = np.array([0x22, 0x0a, 0x0a], dtype=R) / R(255)
    amb = bg * R(0.8)
    ng = (-gdot)[:, None]
    for s, add in ((MISS, lambda m: g[m] + bg), (AMBIENT, lambda m: g[m] + amb), (LIT, lambda m: (g[m] + obj * ng[m]) + amb),
                   (SHADOWED, lambda m: (g[m] + bg) + amb * ng[m])):
        m = state == s
        g[m] = add(m)
    lit = state == LIT
    alpha[lit] = alpha[lit] + R(1)


def scale_u8(v, R):
    r = R(0.5) + R(255) * v
    safe = np.where(r > R(0), r, R(0))
    return np.where(r > R(255), 255, np.where(r > R(0), np.trunc(np.minimum(safe, R(255))), 0)).astype(np.uint8)


def restate_frame(o, mode, w, h, spp, cam, light, regions, R):
    out = []
    for (l, t, r, b) in regions:
        ys, xs = np.meshgrid(np.arange(b, t), np.arange(l, r), indexing="ij")
        xs, ys = xs.ravel(), ys.ravel()
        g, alpha = np.zeros((len(xs), 3), dtype=R), np.zeros(len(xs), dtype=R)
        for ssx in range(spp):
            for ssy in range(spp):
                rays = camera_sample_rays(w, h, spp, xs, ys, ssx, ssy, cam, R)
                state, gdot = restate_rays(o, mode, rays, light, R)
                accumulate(g, alpha, state, gdot, R)
        if spp == 0:
            out.append(np.zeros(len(xs) * 4, dtype=np.uint8))
            continue
        rc = R(1) / (R(spp) * R(spp))
        g, alpha = g * rc, alpha * rc
        out.append(np.stack([scale_u8(g[:, 0], R), scale_u8(g[:, 1], R), scale_u8(g[:, 2], R), scale_u8(alpha, R)], axis=1).ravel())
    return np.concatenate(out)


def restate_colors(o, mode, rays, light, R):
    state, gdot = restate_rays(o, mode, rays, light, R)
    g, alpha = np.zeros((len(rays), 3), dtype=R), np.zeros(len(rays), dtype=R)
    accumulate(g, alpha, state, gdot, R)
    return g, alpha


def bits(a, R):
    a = np.ascontiguousarray(np.asarray(a, dtype=R))
    return a.view(np.uint32 if R == np.float32 else np.uint64)


# ---- the identity camera is the render ----

@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_the_identity_camera_renders_the_frame(precision):
    s = rta.Scene.default(precision=precision)
    d = s.device()
    cam = identity(s)
    cases = [((1920, 1080, 1), None), ((800, 600, 1), None), ((1024, 768, 1), None), ((1024, 768, 2), None), ((1024, 768, 4), None),
             ((1024, 768, 0), None), ((800, 600, 1), "buckets")]
    for opts, kind in cases:
        w, h, _ = opts
        regions = [(r.l, r.t, r.r, r.b) for r in rta.buckets(rta.RenderOptions(w, h, 1), 48)] if kind else [(0, h, w, 0)]
        ref, rst = d.render_tiles(opts, regions, SKIP, want_stats=True)
        got, st = d.render_camera(opts, cam, regions, want_stats=True)
        np.testing.assert_array_equal(got, ref, err_msg=str(opts))
        assert tuple(st[k] for k in COUNTERS) == tuple(rst[k] for k in COUNTERS), (opts, st, rst)
        assert st["tests_executed"] == st["sphere_tests"] + st["bound_tests"] and st["longest_wave_cycles"] == 0
        if opts[2]:
            assert st["primary"] == w * h * opts[2] ** 2 and st["device_ms"] > 0
        plain, none = d.render_camera(opts, cam, regions, want_stats=False)
        assert none is None
        np.testing.assert_array_equal(plain, ref, err_msg=str(opts))


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_the_identity_camera_on_a_scene_without_bounds_is_the_flat_scan(precision):
    it, _, _ = random_nested_scene(5)
    s = rta.Scene(it, rta.normalized((-1.0, -3.0, 2.0), precision), (0.0, 0.0, -4.0), precision=precision)
    d = s.device()
    for opts in ((320, 240, 1), (200, 120, 2)):
        regions = [(0, opts[1], opts[0], 0)]
        ref, rst = d.render_tiles(opts, regions, FLAT, want_stats=True)
        got, st = d.render_camera(opts, identity(s), regions, want_stats=True)
        np.testing.assert_array_equal(got, ref)
        assert util.ray_stats(st) == util.ray_stats(rst)
        assert st["hits"] > 0 and st["occluded"] > 0


# ---- any camera is the oracle's ----

def camera_views(s, precision):
    """(name, camera REAL[12]) from outside the root bound, inside it, inside an inner bound, rolled, wide and narrow, and skewed."""
    R = REAL[precision]
    items = s.items.astype(np.float64)
    if s.bounds is not None and len(s.bounds):
        bounds = s.bounds.astype(np.float64)
    else:
        c = items[:, :3].mean(axis=0)
        bounds = np.array([[c[0], c[1], c[2], np.max(np.linalg.norm(items[:, :3] - c, axis=1) + items[:, 3])]])
    c, r = bounds[0, :3], bounds[0, 3]
    la = lambda e, t, **kw: rta.look_at(e, t, precision=precision, **kw)
    views = [("outside", la(c + r * np.array([1.6, 0.9, -1.8]), c)),
             ("inside_root", la(c + r * np.array([0.2, -0.3, -0.5]), c + r * np.array([0.0, 0.1, 0.4]))),
             ("rolled", la(c + r * np.array([-1.5, 0.4, -1.7]), c, up=(np.sin(0.7), np.cos(0.7), 0.0))),
             ("wide", la(c + r * np.array([0.0, 0.5, -2.2]), c, hfov_deg=120.0)),
             ("narrow", la(c + r * np.array([0.3, 0.2, -2.5]), c, hfov_deg=20.0))]
    if len(bounds) > 1:
        k = len(bounds) // 2
        bc, br = bounds[k, :3], bounds[k, 3]
        views.append(("inside_inner", la(bc + br * np.array([0.1, 0.2, -0.3]), bc + np.array([0.0, 0.0, 1.0]))))
    e = c + r * np.array([0.5, 0.8, -2.4])
    views.append(("skewed", np.concatenate([e, [1.1, 0.25, 0.0], [0.2, 0.9, 0.15], [-0.2, -0.3, 1.3]]).astype(R)))
    return views


def oracle_scenes(precision):
    out = [("pyramid_L5",) + util.scene_pair_default(precision, 5)]
    it, bd, rg = random_nested_scene(8)
    out.append(("nested",) + util.scene_pair_ranges(it, bd, rg, precision))
    out.append(("three_spheres",) + util.scene_pair_spheres([(0.0, -1.0, 0.0, 1.0), (-1.2, 0.2, 0.0, 0.5), (1.2, 0.2, 0.0, 0.5)],
                                                             (0.0, -1.0, 0.0, 3.0), precision))
    it, bd, rg = random_nested_scene(3)
    flat = rta.Scene(it, rta.normalized((-1.0, -3.0, 2.0), precision), (0.0, 0.0, -4.0), precision=precision)
    out.append(("no_bounds", flat, oracle.Scene.from_ranges(it, bd, rg, prec=PREC[precision])))
    return out


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_any_camera_matches_the_oracle(precision):
    R = REAL[precision]
    w, h = 48, 32
    regions = [(0, 32, 48, 0)]
    for name, s, o in oracle_scenes(precision):
        mode = oracle.MODE_FLAT if s.bounds is None or not len(s.bounds) else oracle.MODE_HIERARCHY
        light = s.directional_light.astype(R)
        d = s.device()
        for view, cam in camera_views(s, precision):
            for spp in ((1, 2) if view in ("outside", "inside_root", "skewed") else (1,)):
                got, st = d.render_camera((w, h, spp), cam, regions, want_stats=True)
                ref = restate_frame(o, mode, w, h, spp, cam, light, regions, R)
                np.testing.assert_array_equal(got, ref, err_msg="%s %s spp %d" % (name, view, spp))
                assert st["primary"] == w * h * spp * spp
        d.close()


def test_a_camera_inside_a_bound_sees_what_the_reference_sees():
    # SURVEY.md H2 (tests/util.py INSIDE_ITEMS): from inside group A's bound, A's "distance" is its exit distance and A is culled although it
    # holds the nearer item -- the camera path walks the reference's hierarchy, so it makes the same choice, unlike the flat scan
    s, o = util.scene_pair_ranges(util.INSIDE_ITEMS, util.INSIDE_BOUNDS, util.INSIDE_RANGES)
    regions = [(0, 30, 40, 0)]
    for cam in (rta.look_at((0.0, 0.0, -4.0), (0.0, 0.0, 0.0)), rta.look_at((0.05, -0.02, -4.0), (0.0, 0.0, -1.0), hfov_deg=40.0)):
        got, _ = s.device().render_camera((40, 30, 1), cam, regions)
        np.testing.assert_array_equal(got, restate_frame(o, oracle.MODE_HIERARCHY, 40, 30, 1, cam, s.directional_light, regions, np.float32))
        assert not np.array_equal(got, restate_frame(o, oracle.MODE_FLAT, 40, 30, 1, cam, s.directional_light, regions, np.float32))


# ---- rt_trace_rays ----

def test_traced_camera_rays_give_the_rendered_frame():
    s = rta.Scene.default()
    d = s.device()
    w, h = 1920, 1080
    ref, rst = d.render_tiles((w, h, 1), [(0, h, w, 0)], SKIP, want_stats=True)
    color, alpha, st = d.trace(camera_rays(w, h, s.eye), want_stats=True)
    got = np.stack([scale_u8(color[:, 0], np.float32), scale_u8(color[:, 1], np.float32), scale_u8(color[:, 2], np.float32),
                    scale_u8(alpha, np.float32)], axis=1).ravel()
    np.testing.assert_array_equal(got, ref)
    assert tuple(st[k] for k in COUNTERS) == tuple(rst[k] for k in COUNTERS)
    assert set(np.unique(alpha)) <= {0.0, 1.0}


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_traced_rays_match_the_oracle(precision):
    R = REAL[precision]
    rng = np.random.default_rng(21 + precision)
    for name, s, o in oracle_scenes(precision):
        mode = oracle.MODE_FLAT if s.bounds is None or not len(s.bounds) else oracle.MODE_HIERARCHY
        rays, _ = ray_families(s, rng, 30)
        color, alpha = s.device().trace(rays)
        ref_c, ref_a = restate_colors(o, mode, rays, s.directional_light.astype(R), R)
        np.testing.assert_array_equal(bits(color, R), bits(ref_c, R), err_msg=name)
        np.testing.assert_array_equal(bits(alpha, R), bits(ref_a, R), err_msg=name)
        assert (alpha == 1).any() or name == "no_bounds", name
        s.device().close()


# ---- entries, buffers, streams and threads ----

def test_trace_entries_buffers_streams_and_threads_agree():
    import torch
    s = rta.Scene.default()
    d = s.device()
    rays, _ = ray_families(s, np.random.default_rng(4), 200)
    n = len(rays)
    ref = d.trace(rays)
    for a, b in zip(ref, d.trace(rays, want_stats=True)[:2]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    side = torch.cuda.Stream()
    for stream in (None, side, side.cuda_stream):
        tr = torch.from_numpy(rays).cuda()
        dev = d.trace(tr, stream=stream)
        if stream is not None:
            side.synchronize()
        for a, b in zip(ref, dev):
            assert b.device.type == "cuda"
            np.testing.assert_array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))
    hb = [capi.HostBuffer(k) for k in (rays.nbytes, 12 * n, 4 * n)]
    pr = hb[0].array.view(np.float32).reshape(n, 6)
    pr[:] = rays
    out = (hb[1].array.view(np.float32).reshape(n, 3), hb[2].array.view(np.float32))
    pinned = d.trace(pr, out=out)
    for a, b in zip(ref, pinned):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    results, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(5):
                results[k] = d.trace(rays)
        except Exception as e:          # noqa: BLE001 (reported below)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for r in results:
        for a, b in zip(ref, r):
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_trace_on_a_side_stream_and_on_its_handle_is_the_default_stream_trace(precision):
    import torch
    R = np.float32 if precision == rta.RT_F32 else np.float64
    s = rta.Scene.three_spheres(precision)
    d = s.device()
    rng = np.random.default_rng(65)
    rays = np.concatenate([np.tile(s.eye.astype(np.float64), (65, 1)), rng.normal(size=(65, 3)) * (0.3, 0.3, 0.0) + (0.0, -0.1, 1.0)], axis=1)      # one wave and one lane
    rays[:, 3:] /= np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
    tr = torch.from_numpy(rays.astype(R)).cuda()
    order = torch.from_numpy(rng.permutation(65).astype(np.int32)).cuda()
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    for o in (None, True, order):
        ref = [a.cpu().numpy().view(np.uint8) for a in d.trace(tr, order=o)]
        assert ref[1].any()                                                          # some ray hits
        for stream in (side, side.cuda_stream):
            got = d.trace(tr * 1.0, stream=stream, order=None if o is None else (o if o is True else o.clone()))      # inputs made on the current stream
            side.synchronize()
            for a, b in zip(ref, got):
                assert b.device.type == "cuda"
                np.testing.assert_array_equal(a, b.cpu().numpy().view(np.uint8))


def test_trace_host_entry_rejects_rays_outside_the_domain():
    d = rta.Scene.three_spheres().device()
    good = np.array([[0, 0, -4, 0, 0, 1]] * 4, dtype=np.float32)
    d.trace(good)
    for k, v in ((1, np.nan), (5, np.inf), (0, 2e15), (3, 0.5)):
        r = good.copy(); r[2, k] = v
        with pytest.raises(rta.RtError) as e:
            d.trace(r)
        assert e.value.status == capi.RT_ERR_INVALID_ARGUMENT


def test_camera_entries_buffers_streams_and_threads_agree():
    import torch
    s = rta.Scene.default()
    d = s.device()
    opts = (640, 480, 2)
    regions = [(r.l, r.t, r.r, r.b) for r in rta.buckets(rta.RenderOptions(640, 480, 2), 64)]
    cam = rta.look_at((2.0, 1.5, -4.5), (0.0, -0.5, 0.0))
    ref, _ = d.render_camera(opts, cam, regions, want_stats=False)
    nbytes = ref.size
    counted, _ = d.render_camera(opts, cam, regions, want_stats=True)
    np.testing.assert_array_equal(counted, ref)
    hb = capi.HostBuffer(nbytes)
    pinned, _ = d.render_camera(opts, cam, regions, want_stats=False, out=hb.array)
    np.testing.assert_array_equal(pinned, ref)
    side = torch.cuda.Stream()
    for stream, stats in ((0, False), (side.cuda_stream, False), (side.cuda_stream, True)):
        buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        d.render_camera_device(opts, cam, regions, buf.data_ptr(), stream=stream, want_stats=stats)
        side.synchronize()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(buf.cpu().numpy(), ref)
    results, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(3):
                results[k] = d.render_camera(opts, cam, regions, want_stats=False)[0].copy()
        except Exception as e:          # noqa: BLE001 (reported below)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for r in results:
        np.testing.assert_array_equal(r, ref)
    # the host entry checks the camera too, and a region outside the image is the render's error
    with pytest.raises(rta.RtError) as e:
        d.render_camera(opts, np.zeros(12, dtype=np.float32), regions)
    assert e.value.status == capi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(rta.RtError) as e:
        d.render_camera(opts, cam, [(0, 481, 640, 0)])
    assert e.value.status == capi.RT_ERR_INVALID_REGION
    with pytest.raises(ValueError):
        d.render_camera(opts, cam.astype(np.float64), regions)
