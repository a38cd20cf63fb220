#!/usr/bin/env python3
"""What an update of a dynamic scene costs (rt_scene_update*, csrc/rt_dynamic.hpp) next to the rt_scene_create it replaces.

Per scene (default L8 and L9, the 100,000-sphere scene) and precision (f32, f64), with device events after warm-up, on one stream:
  update_refit_ms        rt_scene_update_device, bounds refit on the device: box, reach and rewrite kernels
  update_bounds_ms       rt_scene_update_device with the caller's bounds: the rewrite kernel alone
  frame_ms               rt_render_camera_device, 1920x1080 spp 1 through the identity camera, on the dynamic scene
  update_frame_ms        update (refit) + that frame, back to back on the stream: one animation step
and on the host clock (the calls return when the scene is in place):
  host_update_refit_ms   rt_scene_update from pageable host memory, refit
  host_update_bounds_ms  rt_scene_update with the caller's bounds
  create_total_ms        rt_scene_setup_cost total of rt_scene_create for the same scene in this run (median of 3; create_stream_ms of it is
                         the scene's stream, create_library_ms the rest): what moving a sphere cost before
  create_dynamic_ms      the same for rt_scene_create_dynamic

usage: update_rate.py [iterations] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/u01_update_rate.json)"""
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


def timed(fn, iters, stream):
    # warm-up: at least 3 calls and 0.2 s of them (an idle GPU's clocks take a while to ramp: the first leg of a run otherwise reads slow)
    t0 = time.perf_counter()
    k = 0
    while k < 3 or time.perf_counter() - t0 < 0.2:
        fn()
        k += 1
        if k % 8 == 0:
            stream.synchronize()
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def host_timed(fn, iters):
    t0 = time.perf_counter()
    k = 0
    while k < 3 or time.perf_counter() - t0 < 0.2:
        fn()
        k += 1
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return round((time.perf_counter() - t0) * 1e3 / iters, 4)


def setup_costs(scene, dynamic):
    tot, strm = [], []
    for _ in range(3):
        d = rta.DeviceScene(scene, dynamic=dynamic)
        t, s = d.setup_cost()
        tot.append(t); strm.append(s)
        d.close()
    k = int(np.argsort(tot)[1])
    return round(tot[k], 4), round(strm[k], 4)


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "u01_update_rate.json")
    if "--out" in args:
        k = args.index("--out")
        out_path = args[k + 1]
        del args[k:k + 2]
    iters = int(args[0]) if args else 50
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    w, h = 1920, 1080
    buf = torch.empty(w * h * 4, dtype=torch.uint8, device=dev)
    out = {"workload": "rt_scene_update_device / rt_scene_update (refit and caller's bounds), alone and in front of a 1920x1080 spp-1 "
                       "rt_render_camera_device frame, against rt_scene_create of the same scene",
           "iterations": iters, "scenes": {}}
    for prec, pname in ((rta.RT_F32, "f32"), (rta.RT_F64, "f64")):
        R = np.float32 if prec == rta.RT_F32 else np.float64
        for name, make in (("default_L8", lambda: rta.Scene.default(8, prec)), ("default_L9", lambda: rta.Scene.default(9, prec)),
                           ("100k", lambda: rta.Scene.from_spheres_auto(hundred_thousand_spheres(), precision=prec))):
            s = make()
            d = s.device(dynamic=True)
            opts, regions = (w, h, 1), [(0, h, w, 0)]
            ident = np.concatenate([s.eye, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=R)]).astype(R)
            # a second set of values to move to: every radius 1 % smaller (the refit bounds then differ from the scene's own)
            moved = s.items.copy()
            moved[:, 3] *= R(0.99)
            t_items, t_bounds = torch.from_numpy(moved).to(dev), torch.from_numpy(s.bounds).to(dev)
            torch.cuda.synchronize()
            hs = C.c_void_p(stream.cuda_stream)
            pi, pb = C.c_void_p(t_items.data_ptr()), C.c_void_p(t_bounds.data_ptr())
            upd = lambda bounds: capi.check(capi.lib.rt_scene_update_device(d._h, pi, bounds, hs), "rt_scene_update_device")
            frame = lambda: d.render_camera_device(opts, ident, regions, buf.data_ptr(), stream=stream.cuda_stream)
            r = {"items": int(s.items.shape[0]), "groups": int(s.bounds.shape[0])}
            r["update_refit_ms"] = timed(lambda: upd(None), iters, stream)
            r["update_bounds_ms"] = timed(lambda: upd(pb), iters, stream)
            r["frame_ms"] = timed(frame, iters, stream)
            r["update_frame_ms"] = timed(lambda: (upd(None), frame()), iters, stream)
            r["host_update_refit_ms"] = host_timed(lambda: d.update(moved), iters)
            r["host_update_bounds_ms"] = host_timed(lambda: d.update(moved, s.bounds), iters)
            np.testing.assert_array_equal(d.bounds(), s.bounds)
            d.update(moved)
            np.testing.assert_array_equal(d.bounds(), rta.refit_bounds(moved, s.ranges, prec))      # (what was timed is the rule)
            r["create_total_ms"], r["create_stream_ms"] = setup_costs(s, False)
            r["create_library_ms"] = round(r["create_total_ms"] - r["create_stream_ms"], 4)
            r["create_dynamic_ms"], _ = setup_costs(s, True)
            r["update_cheaper_than_create"] = bool(max(r["update_refit_ms"], r["host_update_refit_ms"]) < r["create_library_ms"])
            out["scenes"]["%s_%s" % (name, pname)] = r
            del t_items, t_bounds
            d.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
