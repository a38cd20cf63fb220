#!/usr/bin/env python3
"""Rates of the camera path (rt_render_camera_device, csrc/rt_trace.hpp), timed with device events after warm-up.

Per scene (default L8 and L9, the 100,000-sphere scene) and precision (f32, f64), for the 1920x1080 frame at spp 1 through the identity camera:
  camera_ms   rt_render_camera_device: primary walk, shading and shadow walk in one kernel, RGBA out
  query_ms    what the same frame costs through the ray queries: rt_intersect_rays_device nearest over its camera rays plus any-hit over its
              shadow rays, as `nearest_ms` + `any_ms` -- the bar the camera frame is held to
  render_ms   rt_render_tiles_device, the render's own specialised kernels for Scene::eye
and on L8 f32 also 1024x768 at spp 4 (identity), an orbit view from outside the pyramid and a view from inside it (camera and render only).

usage: camera_rate.py [iterations] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/c01_camera_rate.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
import rust_tracer_amd as rta  # noqa: E402
from tests.scenes import hundred_thousand_spheres  # noqa: E402

SKIP = rta.RT_TRAVERSAL_SKIP


def camera_rays(w, h, eye, R):
    """render.rs:231-241 at spp 1, pixel order (y outer), in REAL."""
    y, x = np.meshgrid(np.arange(h, dtype=R), np.arange(w, dtype=R), indexing="ij")
    fw, fh = R(w), R(h)
    dx, dy, dz = x - fw / R(2), (fh - y) - fh / R(2), np.full_like(x, fw)
    inv = R(1) / np.sqrt((dx * dx + dy * dy) + dz * dz)
    rays = np.empty((w * h, 6), dtype=R)
    rays[:, :3] = eye
    rays[:, 3], rays[:, 4], rays[:, 5] = (dx * inv).ravel(), (dy * inv).ravel(), (dz * inv).ravel()
    return rays


def shadow_rays(rays, dist, nrm, item, light, R):
    g = (nrm[:, 0] * light[0] + nrm[:, 1] * light[1]) + nrm[:, 2] * light[2]
    sh = (item >= 0) & (g < R(0))
    dd = dist[sh][:, None]
    p = (rays[sh, :3] + rays[sh, 3:] * dd) + nrm[sh] * (dd * R(np.sqrt(np.finfo(R).eps)))
    return np.concatenate([p, np.broadcast_to(-light, p.shape)], axis=1).astype(R)


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


def frame_legs(d, opts, cam, iters, stream, buf):
    regions = [(0, opts[1], opts[0], 0)]
    h = stream.cuda_stream
    return {"camera_ms": timed(lambda: d.render_camera_device(opts, cam, regions, buf.data_ptr(), stream=h), iters, stream)}


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "c01_camera_rate.json")
    if "--out" in args:
        k = args.index("--out")
        out_path = args[k + 1]
        del args[k:k + 2]
    iters = int(args[0]) if args else 20
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    w, h = 1920, 1080
    buf = torch.empty(w * h * 4, dtype=torch.uint8, device=dev)
    out = {"workload": "rt_render_camera_device against rt_intersect_rays_device (nearest + any-hit) and rt_render_tiles_device, 1920x1080 spp 1",
           "iterations": iters, "scenes": {}}
    for prec, pname in ((rta.RT_F32, "f32"), (rta.RT_F64, "f64")):
        R = np.float32 if prec == rta.RT_F32 else np.float64
        for name, make in (("default_L8", lambda: rta.Scene.default(8, prec)), ("default_L9", lambda: rta.Scene.default(9, prec)),
                           ("100k", lambda: rta.Scene.from_spheres_auto(hundred_thousand_spheres(), precision=prec))):
            s = make()
            d = s.device()
            opts = (w, h, 1)
            regions = [(0, h, w, 0)]
            ident = np.concatenate([s.eye, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=R)]).astype(R)
            r = frame_legs(d, opts, ident, iters, stream, buf)
            cam = camera_rays(w, h, s.eye, R)
            dist, nrm, item = d.intersect(cam)
            sh = shadow_rays(cam, dist, nrm, item, s.directional_light, R)
            cam_t = torch.from_numpy(cam).to(dev)
            sh_t = torch.from_numpy(sh).to(dev)
            r["nearest_ms"] = timed(lambda: d.intersect(cam_t, stream=stream), iters, stream)
            r["any_ms"] = timed(lambda: d.intersect(sh_t, any_hit=True, stream=stream), iters, stream)
            r["query_ms"] = round(r["nearest_ms"] + r["any_ms"], 4)
            r["render_ms"] = timed(lambda: d.render_tiles_device(opts, regions, buf.data_ptr(), stream=stream.cuda_stream, traversal=SKIP), iters, stream)
            r["camera_vs_query"] = round(r["camera_ms"] / r["query_ms"], 3)
            # the fused kernel's rays against the query's: the same frame traced through rt_trace_rays_device (colours, no quantisation)
            r["trace_rays_ms"] = timed(lambda: d.trace(cam_t, stream=stream), iters, stream)
            _, st = d.render_camera(opts, ident, regions, want_stats=True)
            r["shadow_rays"] = st["shadow"]
            r["tests_per_ray"] = round(st["tests_executed"] / (st["primary"] + st["shadow"]), 2)
            if prec == rta.RT_F32 and name == "default_L8":
                o4 = (1024, 768, 4)
                r["spp4_1024x768"] = {"camera_ms": timed(lambda: d.render_camera_device(o4, ident, [(0, 768, 1024, 0)], buf.data_ptr(), stream=stream.cuda_stream),
                                                         iters, stream),
                                      "render_ms": timed(lambda: d.render_tiles_device(o4, [(0, 768, 1024, 0)], buf.data_ptr(), stream=stream.cuda_stream,
                                                                                       traversal=SKIP), iters, stream)}
                for view, c in (("orbit_outside", rta.look_at((3.5, 2.0, -3.0), (0.0, -0.3, 0.0), hfov_deg=60.0)),
                                ("inside", rta.look_at((0.1, -0.2, -0.3), (0.3, -0.5, 1.0), hfov_deg=90.0))):
                    r[view] = frame_legs(d, opts, c, iters, stream, buf)
            del cam_t, sh_t
            out["scenes"]["%s_%s" % (name, pname)] = r
            d.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
