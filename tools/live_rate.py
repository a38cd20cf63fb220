#!/usr/bin/env python3
"""What live and dead slots cost (rt_scene_update_live_device / rt_scene_rebuild_n_device, csrc/rt_dynamic.hpp) next to the
entries that keep every slot live, in the same run.

Per scene (default L8 and L9, the 100,000-sphere scene) and precision (f32, f64), with device events after warm-up, on one stream:
  update_ms                rt_scene_update_device, refit: the three kernels of 4.11
  update_live_<p>_ms       rt_scene_update_live_device at p = 100, 50, 1 % live slots (seeded random liveness): their live-aware siblings
  rebuild_ms               rt_scene_rebuild_device of the scene's spheres in a seeded random order, under rt_balanced_ranges
  rebuild_n_<f>_ms         rt_scene_rebuild_n_device of the first n = capacity, capacity / 2, capacity / 100 of them (f = 1, 2, 100)
and behind each of them the 1920x1080 spp-1 identity-camera frame: frame_*_ms, and tests_per_ray_* from a counting frame.

usage: live_rate.py [iterations] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/l01_live_rate.json)"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
import rust_tracer_amd as rta  # noqa: E402
from rust_tracer_amd import capi  # noqa: E402
from tests.scenes import hundred_thousand_spheres  # noqa: E402
from tools.update_rate import timed  # noqa: E402


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "l01_live_rate.json")
    if "--out" in args:
        k = args.index("--out")
        out_path = args[k + 1]
        del args[k:k + 2]
    iters = int(args[0]) if args else 50
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    hs = C.c_void_p(stream.cuda_stream)
    w, h = 1920, 1080
    opts, regions = (w, h, 1), [(0, h, w, 0)]
    buf = torch.empty(w * h * 4, dtype=torch.uint8, device=dev)
    out = {"workload": "rt_scene_update_live_device at 100 / 50 / 1 % live next to rt_scene_update_device, rt_scene_rebuild_n_device at n = "
                       "capacity, / 2, / 100 next to rt_scene_rebuild_device, each with the 1920x1080 spp-1 identity-camera frame behind it",
           "iterations": iters, "scenes": {}}
    for prec, pname in ((rta.RT_F32, "f32"), (rta.RT_F64, "f64")):
        R = np.float32 if prec == rta.RT_F32 else np.float64
        for name, make in (("default_L8", lambda: rta.Scene.default(8, prec)), ("default_L9", lambda: rta.Scene.default(9, prec)),
                           ("100k", lambda: rta.Scene.from_spheres_auto(hundred_thousand_spheres(), precision=prec))):
            s = make()
            n = int(s.items.shape[0])
            ident = np.concatenate([s.eye, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=R)]).astype(R)
            rng = np.random.default_rng(13)
            r = {"items": n, "groups": int(s.bounds.shape[0])}

            def measure(d, key, write):
                """`write` alone, then the frame behind it (the scene is what `write` left), then its tests per ray."""
                r[key + "_ms"] = timed(write, iters, stream)
                r["frame_" + key + "_ms"] = timed(lambda: d.render_camera_device(opts, ident, regions, buf.data_ptr(), stream=stream.cuda_stream), iters, stream)
                st = d.render_camera_device(opts, ident, regions, buf.data_ptr(), stream=stream.cuda_stream, want_stats=True)
                stream.synchronize()
                r["tests_per_ray_" + key] = round(st["tests_executed"] / max(1, st["primary"]), 2)

            # ---- updates: the scene's own topology, refit bounds ----
            d = s.device(dynamic=True)
            t_items = torch.from_numpy(s.items).to(dev)
            pi = C.c_void_p(t_items.data_ptr())
            torch.cuda.synchronize()
            measure(d, "update", lambda: capi.check(capi.lib.rt_scene_update_device(d._h, pi, None, hs), "rt_scene_update_device"))
            for pc in (100, 50, 1):
                live = (rng.random(n) < pc / 100.0).astype(np.uint8) if pc < 100 else np.ones(n, dtype=np.uint8)
                t_live = torch.from_numpy(live).to(dev)
                torch.cuda.synchronize()
                pl = C.c_void_p(t_live.data_ptr())
                measure(d, "update_live_%d" % pc, lambda: capi.check(capi.lib.rt_scene_update_live_device(d._h, pi, None, pl, hs), "rt_scene_update_live_device"))
                np.testing.assert_array_equal(d.live(), live)
                np.testing.assert_array_equal(d.bounds(), rta.refit_bounds(s.items, s.ranges, prec, live=live))      # (what was timed is the rule)
            d.close()
            # ---- rebuilds: the same spheres in a random order under the balanced topology ----
            caller = np.ascontiguousarray(s.items[rng.permutation(n)])
            b = rta.Scene.from_spheres_balanced(caller, precision=prec)
            d = b.device(dynamic=True)
            t_caller = torch.from_numpy(caller).to(dev)
            pc_ = C.c_void_p(t_caller.data_ptr())
            torch.cuda.synchronize()
            measure(d, "rebuild", lambda: capi.check(capi.lib.rt_scene_rebuild_device(d._h, pc_, None, hs), "rt_scene_rebuild_device"))
            for f in (1, 2, 100):
                m = n // f
                measure(d, "rebuild_n_%d" % f, lambda: capi.check(capi.lib.rt_scene_rebuild_n_device(d._h, pc_, m, None, hs), "rt_scene_rebuild_n_device"))
                assert int(d.live().sum()) == m
            d.close()
            out["scenes"]["%s_%s" % (name, pname)] = r
            del t_items, t_caller
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
