#!/usr/bin/env python3
"""Rates of the ray-query entry point rt_intersect_rays_device on torch tensors, timed with device events after warm-up:

  camera   1920x1080 primary rays in pixel order (render.rs:231-241 in f32), nearest hit
  shuffled the same rays in a random order
  random   2M rays with origins inside the scene's root bound and random unit directions
  shadow   the any-hit shadow rays of `camera` (render.rs:190-207)

on the default scene at L8 and L9 and on the 100,000-sphere scene.  Per batch: rays/s, tests/s (from one counting launch) and the host
time of one call.  `render_count_ms`: the counting render of the same 1080p frame (primary + shadow walks, counters on) -- the query of
`camera` without counters should not be slower.

usage: query_rate.py [iterations]      prints one JSON line"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
import rust_tracer_amd as rta  # noqa: E402
from tests.scenes import hundred_thousand_spheres  # noqa: E402


def camera_rays(w, h, eye):
    f = np.float32
    y, x = np.meshgrid(np.arange(h, dtype=f), np.arange(w, dtype=f), indexing="ij")
    fw, fh = f(w), f(h)
    dx, dy, dz = x - fw / f(2), (fh - y) - fh / f(2), np.full_like(x, fw)
    inv = f(1) / np.sqrt((dx * dx + dy * dy) + dz * dz)
    rays = np.empty((w * h, 6), dtype=f)
    rays[:, :3] = eye
    rays[:, 3], rays[:, 4], rays[:, 5] = (dx * inv).ravel(), (dy * inv).ravel(), (dz * inv).ravel()
    return rays


def shadow_rays(rays, dist, nrm, item, light):
    f = np.float32
    g = (nrm[:, 0] * light[0] + nrm[:, 1] * light[1]) + nrm[:, 2] * light[2]
    sh = (item >= 0) & (g < f(0))
    dd = dist[sh][:, None]
    p = (rays[sh, :3] + rays[sh, 3:] * dd) + nrm[sh] * (dd * np.sqrt(np.finfo(f).eps))
    return np.concatenate([p, np.broadcast_to(-light, p.shape)], axis=1).astype(f)


def time_query(d, rays_t, any_hit, iters, stream):
    for _ in range(3):
        d.intersect(rays_t, any_hit=any_hit, stream=stream)
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    host = 0.0
    e0.record(stream)
    for _ in range(iters):
        t0 = time.perf_counter()
        d.intersect(rays_t, any_hit=any_hit, stream=stream)
        host += time.perf_counter() - t0
    e1.record(stream)
    e1.synchronize()
    ms = e0.elapsed_time(e1) / iters
    _, _, _, st = d.intersect(rays_t, any_hit=any_hit, want_stats=True, stream=stream)
    n = rays_t.shape[0]
    return {"rays": n, "device_ms": round(ms, 4), "rays_per_s": round(n / ms * 1e3), "tests_per_s": round(st["tests_executed"] / ms * 1e3),
            "tests_per_ray": round(st["tests_executed"] / n, 2), "hits": st["hits"], "call_us": round(host / iters * 1e6, 1)}


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rng = np.random.default_rng(1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    scenes = [("default_L8", rta.Scene.default(8)), ("default_L9", rta.Scene.default(9)),
              ("100k", rta.Scene.from_spheres_auto(hundred_thousand_spheres()))]
    out = {"workload": "rt_intersect_rays_device, f32, torch tensors", "iterations": iters, "scenes": {}}
    for name, s in scenes:
        d = s.device()
        w, h = 1920, 1080
        _, rst = d.render_tiles((w, h, 1), [(0, h, w, 0)], rta.RT_TRAVERSAL_SKIP, want_stats=True)
        cam = camera_rays(w, h, s.eye)
        dist, nrm, item = d.intersect(cam)
        shadow = shadow_rays(cam, dist, nrm, item, s.directional_light)
        root = s.bounds[0].astype(np.float64)
        n = 2 << 20
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = root[:3] + rng.normal(size=(n, 3)) / np.sqrt(3) * root[3] * 0.5
        o = np.where(np.linalg.norm(o - root[:3], axis=1, keepdims=True) < root[3], o, root[:3])
        rnd = np.concatenate([o, u], axis=1).astype(np.float32)
        r = {"render_count_ms": round(rst["device_ms"], 4)}
        for batch, rays, any_hit in (("camera", cam, False), ("shuffled", cam[rng.permutation(len(cam))], False), ("random", rnd, False),
                                     ("shadow", shadow, True)):
            rays_t = torch.from_numpy(np.ascontiguousarray(rays)).to(dev)
            r[batch] = time_query(d, rays_t, any_hit, iters, stream)
        out["scenes"][name] = r
        d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
