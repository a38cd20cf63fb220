#!/usr/bin/env python3
"""Rates of the multi-hit ray query rt_intersect_rays_multi_device on torch tensors, timed with device events after
warm-up, against the nearest query (rt_intersect_rays_device) on the same rays in the same run:

  nearest      RT_QUERY_NEAREST
  closest_k    RT_MULTIHIT_CLOSEST, k = 1, 4, 8, 16
  all_16       RT_MULTIHIT_ALL, k = 16

over 1920x1080 primary rays (render.rs:231-241 in f32) in pixel order and shuffled, on the default scene at L8 and L9 and on the
100,000-sphere scene.  The variants are timed in interleaved rounds (median and minimum over the rounds); tests/s come from one
counting launch each.  `closest_1_vs_nearest`: the k = 1 list's time over the nearest query's (medians).

usage: multihit_rate.py [iterations] [--rounds R] [--out PATH]      prints one JSON line and writes it to PATH
                                                                    (default profiles/m01_multihit_rate.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
import rust_tracer_amd as rta  # noqa: E402
from query_rate import camera_rays  # noqa: E402
from tests.scenes import hundred_thousand_spheres  # noqa: E402

VARIANTS = [("nearest", None, False), ("closest_1", 1, False), ("closest_4", 4, False), ("closest_8", 8, False), ("closest_16", 16, False),
            ("all_16", 16, True)]


def call(d, rays_t, k, all_hits, stream, want_stats=False):
    if k is None:
        return d.intersect(rays_t, stream=stream, want_stats=want_stats)
    return d.intersect_multi(rays_t, k, all_hits=all_hits, stream=stream, want_stats=want_stats)


def time_once(d, rays_t, k, all_hits, iters, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        call(d, rays_t, k, all_hits, stream)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "m01_multihit_rate.json")
    rounds = 5
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    if "--rounds" in args:
        i = args.index("--rounds")
        rounds = int(args[i + 1])
        del args[i:i + 2]
    iters = int(args[0]) if args else 20
    rng = np.random.default_rng(1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    scenes = [("default_L8", rta.Scene.default(8)), ("default_L9", rta.Scene.default(9)),
              ("100k", rta.Scene.from_spheres_auto(hundred_thousand_spheres()))]
    out = {"workload": "rt_intersect_rays_multi_device vs rt_intersect_rays_device, f32, 1080p camera rays, torch tensors",
           "iterations": iters, "rounds": rounds, "scenes": {}}
    for name, s in scenes:
        d = s.device()
        cam = camera_rays(1920, 1080, s.eye)
        r = {}
        for batch, rays in (("camera", cam), ("shuffled", cam[rng.permutation(len(cam))])):
            rays_t = torch.from_numpy(np.ascontiguousarray(rays)).to(dev)
            for _, k, a in VARIANTS:
                for _ in range(3):
                    call(d, rays_t, k, a, stream)
            stream.synchronize()
            times = {v[0]: [] for v in VARIANTS}
            for _ in range(rounds):
                for v, k, a in VARIANTS:
                    times[v].append(time_once(d, rays_t, k, a, iters, stream))
            res = {}
            n = rays_t.shape[0]
            for v, k, a in VARIANTS:
                st = call(d, rays_t, k, a, stream, want_stats=True)[-1]
                med, best = float(np.median(times[v])), min(times[v])
                res[v] = {"device_ms": round(med, 4), "device_ms_min": round(best, 4), "rays_per_s": round(n / med * 1e3),
                          "tests_per_s": round(st["tests_executed"] / med * 1e3), "tests_per_ray": round(st["tests_executed"] / n, 2),
                          "hits": st["hits"]}
            res["closest_1_vs_nearest"] = round(res["closest_1"]["device_ms"] / res["nearest"]["device_ms"], 3)
            r[batch] = res
        out["scenes"][name] = r
        d.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
