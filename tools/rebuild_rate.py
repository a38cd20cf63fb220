#!/usr/bin/env python3
"""What a rebuild of a dynamic scene costs (rt_scene_rebuild*, csrc/rt_rebuild.hpp) next to what it replaces, and what the
rebuilt hierarchy is worth to a frame.

Per scene (default L8 and L9, the 100,000-sphere scene: their spheres in a seeded random order under rt_balanced_ranges' topology, leaf
size 4) and precision (f32, f64), after warm-up:
  rebuild_ms             rt_scene_rebuild_device on one stream: a pair of events around every call, the median (rebuild_mean_ms: one pair
                         around all of them, back to back)
  update_refit_ms        rt_scene_update_device (refit) on the same scene in the same run, measured the same way: the part of a rebuild
                         that is not the order and the gather
  host_rebuild_ms        rt_scene_rebuild from pageable host memory, on the host clock (it returns when the scene is in place)
  replaced_ms            what a rebuild replaces, on the host clock: rt_build_hierarchy + rt_scene_destroy + rt_scene_create_dynamic
                         (build_hierarchy_ms of it is the builder); median of 3
and for the 100,000 spheres, the 1920x1080 spp-1 rt_render_camera_device frame (identity camera) and its tests per ray (sphere + bound
tests over primary rays, from the counting flavour of the same frame) over three hierarchies of the same spheres:
  frames.rebuilt         balanced ranges, rebuilt
  frames.build_hierarchy rt_build_hierarchy's median-split tree with its own bounds (nearer half first)
  frames.shuffled        balanced ranges over the caller's random order, refit but not rebuilt (three frames: each tests nearly everything)

usage: rebuild_rate.py [iterations] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/b01_rebuild_rate.json)"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
import rust_tracer_amd as rta  # noqa: E402
from rust_tracer_amd import capi  # noqa: E402
from tests.scenes import hundred_thousand_spheres  # noqa: E402


def warm(fn, stream, least=3, seconds=0.2):
    t0 = time.perf_counter()
    k = 0
    while k < least or time.perf_counter() - t0 < seconds:
        fn()
        k += 1
        if k % 8 == 0:
            stream.synchronize()
    stream.synchronize()


def timed_each(fn, iters, stream):
    """(median, mean of a back-to-back run) in ms: events around every call, then one pair around `iters` calls."""
    warm(fn, stream)
    each = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        each.append(e0.elapsed_time(e1))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return round(float(np.median(each)), 4), round(e0.elapsed_time(e1) / iters, 4)


def host_timed(fn, iters):
    t0 = time.perf_counter()
    k = 0
    while k < 3 or time.perf_counter() - t0 < 0.2:
        fn()
        k += 1
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4)


def frame_of(d, scene, R, stream, buf, iters, warm_least=3):
    """The 1080p identity-camera frame on device scene d: ms (median) and tests per ray."""
    w, h = 1920, 1080
    ident = np.concatenate([scene.eye, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=R)]).astype(R)
    opts, regions = (w, h, 1), [(0, h, w, 0)]
    frame = lambda: d.render_camera_device(opts, ident, regions, buf.data_ptr(), stream=stream.cuda_stream)
    if warm_least:
        warm(frame, stream, warm_least)
    else:
        frame()
        stream.synchronize()
    each = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        frame()
        e1.record(stream)
        e1.synchronize()
        each.append(e0.elapsed_time(e1))
    _, st = d.render_camera(opts, ident, regions, want_stats=True)
    return {"frame_ms": round(float(np.median(each)), 4), "frames_timed": iters,
            "tests_per_ray": round((st["sphere_tests"] + st["bound_tests"]) / max(1, st["primary"]), 2), "hits": int(st["hits"])}


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "b01_rebuild_rate.json")
    if "--out" in args:
        k = args.index("--out")
        out_path = args[k + 1]
        del args[k:k + 2]
    iters = int(args[0]) if args else 50
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    buf = torch.empty(1920 * 1080 * 4, dtype=torch.uint8, device=dev)
    out = {"workload": "rt_scene_rebuild_device / rt_scene_rebuild of spheres in a seeded random order under rt_balanced_ranges(n, 4), against the "
                       "refit update in the same run and against rt_build_hierarchy + rt_scene_destroy + rt_scene_create_dynamic; the 1920x1080 "
                       "spp-1 rt_render_camera_device frame over three hierarchies of the 100,000 spheres",
           "iterations": iters, "build": capi.build_info(), "scenes": {}}
    for prec, pname in ((rta.RT_F32, "f32"), (rta.RT_F64, "f64")):
        R = np.float32 if prec == rta.RT_F32 else np.float64
        for name, spheres_of in (("default_L8", lambda: rta.Scene.default(8, prec).items), ("default_L9", lambda: rta.Scene.default(9, prec).items),
                                 ("100k", hundred_thousand_spheres)):
            spheres = np.asarray(spheres_of(), dtype=np.float64)
            n = len(spheres)
            shuffled = np.ascontiguousarray(spheres[np.random.default_rng(17).permutation(n)].astype(R))
            s = rta.Scene.from_spheres_balanced(shuffled, precision=prec)
            d = s.device(dynamic=True)
            r = {"items": n, "groups": int(s.ranges.shape[0])}
            if name == "100k":
                r["frames"] = {"shuffled": frame_of(d, s, R, stream, buf, 3, warm_least=0)}
            t_sph = torch.from_numpy(shuffled).to(dev)
            t_order = torch.empty(n, dtype=torch.uint32, device=dev)
            torch.cuda.synchronize()
            hs = C.c_void_p(stream.cuda_stream)
            ps, po = C.c_void_p(t_sph.data_ptr()), C.c_void_p(t_order.data_ptr())
            rebuild = lambda: capi.check(capi.lib.rt_scene_rebuild_device(d._h, ps, po, hs), "rt_scene_rebuild_device")
            update = lambda: capi.check(capi.lib.rt_scene_update_device(d._h, ps, None, hs), "rt_scene_update_device")
            r["update_refit_ms"], r["update_refit_mean_ms"] = timed_each(update, iters, stream)
            r["rebuild_ms"], r["rebuild_mean_ms"] = timed_each(rebuild, iters, stream)
            order = t_order.cpu().numpy()
            want = np.argsort(rta.sphere_keys(shuffled), kind="stable")
            np.testing.assert_array_equal(order, want)                                                   # (what was timed is the stated order
            np.testing.assert_array_equal(d.bounds(), rta.refit_bounds(shuffled[want], s.ranges, prec))  # ... and the stated refit)
            r["host_rebuild_ms"] = host_timed(lambda: d.rebuild(shuffled), iters)
            if name == "100k":
                r["frames"]["rebuilt"] = frame_of(d, s, R, stream, buf, iters)
            d.close()

            def replaced():
                t0 = time.perf_counter()
                items, bounds, ranges, _ = rta.build_hierarchy(shuffled, 4, prec, eye=s.eye)
                t1 = time.perf_counter()
                fresh = rta.DeviceScene(rta.Scene(items, s.directional_light, s.eye, bounds, ranges, prec), dynamic=True)
                t2 = time.perf_counter()
                return fresh, (t1 - t0) * 1e3, (t2 - t0) * 1e3

            held, builds, totals = rta.DeviceScene(s, dynamic=True), [], []
            for _ in range(3):
                t0 = time.perf_counter()
                held.close()                                                                              # rt_scene_destroy of the scene in use
                t_destroy = (time.perf_counter() - t0) * 1e3
                held, b, t = replaced()
                builds.append(b); totals.append(t + t_destroy)
            k = int(np.argsort(totals)[1])
            r["replaced_ms"], r["build_hierarchy_ms"] = round(totals[k], 4), round(builds[k], 4)
            if name == "100k":
                r["frames"]["build_hierarchy"] = frame_of(held, s, R, stream, buf, iters)
            held.close()
            out["scenes"]["%s_%s" % (name, pname)] = r
            print("%s_%s: %s" % (name, pname, json.dumps(r)), file=sys.stderr, flush=True)
            del t_sph, t_order
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
