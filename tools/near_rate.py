#!/usr/bin/env python3
"""Rates of the proximity query rt_near_spheres_device on torch tensors, timed with device events after warm-up.  The
queries are the scene's own item centres with exclude = self -- every sphere asks for its neighbours -- shuffled, and the same queries
walked in the sphere order of {p, 1} (DeviceScene.sphere_order):

  closest_k    RT_NEAR_CLOSEST, k = 1, 4, 16, radius +inf
  all_16       RT_NEAR_ALL, k = 16, radius = 2 x the median item radius

The bars, measured in the same run on the same device and not the code under test:

  torch_topk_k / torch_count   the all-pairs pass a caller writes today: cdist(points, centres) - radii with the own sphere masked out, then
                               topk(k, smallest) / a count below the radius, in chunks of 8,192 queries
  multihit_k                   rt_intersect_rays_multi_device at the same k over as many rays (from the eye towards each centre): the
                               cost of a walk step with the ray metric

on the default scene at L8 and L9 and on the 100,000-sphere scene, f32.  Every leg is warmed up for 0.2 s, then timed in interleaved
rounds (median and minimum over the rounds); tests per query come from one counting launch each.

usage: near_rate.py [--rounds R] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/n01_near_rate.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
import rust_tracer_amd as rta  # noqa: E402
from tests.scenes import hundred_thousand_spheres  # noqa: E402

WARM_S, SAMPLE_S, CHUNK = 0.2, 0.05, 8192
NEAR = [("closest_1", 1, False), ("closest_4", 4, False), ("closest_16", 16, False), ("all_16", 16, True)]


def torch_pass(points, me, centres, radii, k, rho):
    """The all-pairs bar: per chunk of queries, cdist minus radii with the own sphere at +inf, then the k smallest or the count below rho."""
    out = []
    for a in range(0, points.shape[0], CHUNK):
        gap = torch.cdist(points[a:a + CHUNK], centres) - radii[None, :]
        gap.scatter_(1, me[a:a + CHUNK, None], float("inf"))
        out.append((gap < rho).sum(dim=1) if k is None else torch.topk(gap, k, dim=1, largest=False))
    return out


def timed(fn, stream, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def warm(fn, stream):
    """Runs fn for WARM_S and returns how many calls make one timed sample of about SAMPLE_S."""
    t0, calls = time.perf_counter(), 0
    while True:
        fn()
        stream.synchronize()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= WARM_S:
            return max(1, min(50, int(SAMPLE_S / (dt / calls))))


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "n01_near_rate.json")
    rounds = 5
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    if "--rounds" in args:
        i = args.index("--rounds")
        rounds = int(args[i + 1])
        del args[i:i + 2]
    rng = np.random.default_rng(1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    scenes = [("default_L8", rta.Scene.default(8)), ("default_L9", rta.Scene.default(9)),
              ("100k", rta.Scene.from_spheres_auto(hundred_thousand_spheres()))]
    out = {"workload": "rt_near_spheres_device, f32, the scene's own centres with exclude = self, torch tensors; bars: torch all-pairs, "
                       "rt_intersect_rays_multi_device", "rounds": rounds, "warm_s": WARM_S, "scenes": {}}
    for name, s in scenes:
        d = s.device()
        n = len(s.items)
        perm = rng.permutation(n)
        items = np.ascontiguousarray(s.items[perm])
        rho = float(2.0 * np.median(s.items[:, 3]))
        with torch.cuda.stream(stream):
            points = torch.from_numpy(np.ascontiguousarray(items[:, :3])).to(dev)
            me = torch.from_numpy(perm.astype(np.int32)).to(dev)
            me64 = me.to(torch.int64)
            centres = torch.from_numpy(np.ascontiguousarray(s.items[:, :3])).to(dev)
            radii = torch.from_numpy(np.ascontiguousarray(s.items[:, 3])).to(dev)
            rho_t = torch.full((n,), rho, dtype=torch.float32, device=dev)
            order = d.sphere_order(torch.cat([points, torch.ones((n, 1), dtype=torch.float32, device=dev)], dim=1), stream=stream)
            to = centres[me64] - torch.tensor(s.eye, dtype=torch.float32, device=dev)
            rays = torch.cat([torch.tensor(s.eye, dtype=torch.float32, device=dev).expand(n, 3), to / to.norm(dim=1, keepdim=True)], dim=1).contiguous()
        stream.synchronize()
        legs = {}
        for v, k, a in NEAR:
            for batch, o in (("shuffled", None), ("sphere_order", order)):
                legs["%s/%s" % (v, batch)] = (lambda k=k, a=a, o=o: d.near(points, k, rho_t if a else None, all_within=a, exclude=me, stream=stream, order=o))
        with torch.cuda.stream(stream):
            for k in (1, 4, 16):
                legs["torch_topk_%d" % k] = (lambda k=k: torch_pass(points, me64, centres, radii, k, rho))
                legs["multihit_%d" % k] = (lambda k=k: d.intersect_multi(rays, k, stream=stream))
            legs["torch_count"] = (lambda: torch_pass(points, me64, centres, radii, None, rho))

            def on_stream(fn):
                def run():
                    with torch.cuda.stream(stream):
                        return fn()
                return run
            legs = {v: on_stream(fn) for v, fn in legs.items()}
        iters = {v: warm(fn, stream) for v, fn in legs.items()}
        times = {v: [] for v in legs}
        for _ in range(rounds):
            for v, fn in legs.items():
                times[v].append(timed(fn, stream, iters[v]))
        res = {"queries": n, "radius_all": rho}
        for v in legs:
            med, best = float(np.median(times[v])), min(times[v])
            res[v] = {"device_ms": round(med, 4), "device_ms_min": round(best, 4), "per_s": round(n / med * 1e3), "calls_per_sample": iters[v]}
        for v, k, a in NEAR:
            st = d.near(points, k, rho_t if a else None, all_within=a, exclude=me, stream=stream, want_stats=True)[-1]
            for batch in ("shuffled", "sphere_order"):
                res["%s/%s" % (v, batch)].update(tests_per_query=round(st["tests_executed"] / n, 2), found_any=st["hits"])
            bar = "torch_count" if a else "torch_topk_%d" % k
            res["%s/sphere_order" % v]["vs_torch"] = round(res[bar]["device_ms"] / res["%s/sphere_order" % v]["device_ms"], 2)
            res["%s/shuffled" % v]["vs_torch"] = round(res[bar]["device_ms"] / res["%s/shuffled" % v]["device_ms"], 2)
        for k in (1, 4, 16):
            st = d.intersect_multi(rays, k, stream=stream, want_stats=True)[-1]
            res["multihit_%d" % k]["tests_per_ray"] = round(st["tests_executed"] / n, 2)
        # the bar answers the same question: the nearest neighbour of every sphere, wherever the two agree to 1e-5
        g, it, _ = d.near(points, 1, exclude=me, stream=stream)
        tk = torch_pass(points, me64, centres, radii, 1, rho)
        tg = torch.cat([x.values for x in tk])[:, 0]
        stream.synchronize()
        torch.cuda.synchronize()
        res["nearest_gap_max_abs_diff_vs_torch"] = float((g[:, 0] - tg).abs().max())
        out["scenes"][name] = res
        d.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
