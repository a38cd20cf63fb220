#!/usr/bin/env python3
"""Rates of the sphere cast rt_sweep_spheres_device on torch tensors, timed with device events after warm-up.  The casts
are the scene's own spheres: every sphere is cast from its own centre with its own radius and exclude = itself, in a random direction --
one step of a particle update -- shuffled, and the same casts walked in the sphere order of {pos, 1} (DeviceScene.sphere_order):

  nearest_T / any_T    RT_SWEEP_NEAREST / RT_SWEEP_ANY with tmax = T median item radii, T = 1, 10 and +inf

The bars, measured in the same run on the same device:

  torch_toi_T          the all-pairs pass a caller writes today: per chunk of 2,048 casts, the time of impact with every sphere (the
                       quadratic with the radii added, the own sphere masked out), then the minimum below tmax
  ray_query / cast_q0  rt_intersect_rays_device and the cast with radius 0 over the same rays, from the scene's eye towards every centre:
                       from outside the root the two make the same tests (checked here from one counting launch each), so their ratio is
                       the cost of the instructions a cast adds per node

on the default scene at L8 and L9 and on the 100,000-sphere scene, f32.  Every leg is warmed up for 0.2 s, then timed in interleaved
rounds (median and minimum over the rounds); tests per cast come from one counting launch each.

usage: sweep_rate.py [--rounds R] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/s01_sweep_rate.json)"""
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

WARM_S, SAMPLE_S, CHUNK = 0.2, 0.05, 2048
STEPS = [("1", 1.0), ("10", 10.0), ("inf", None)]


def torch_pass(pos, dirs, q, me, centres, radii, tmax):
    """The all-pairs bar: per chunk of casts, the time of impact with every sphere (own sphere at +inf), then the first one below tmax."""
    out = []
    cc = (centres * centres).sum(dim=1)
    for a in range(0, pos.shape[0], CHUNK):
        p, d = pos[a:a + CHUNK], dirs[a:a + CHUNK]
        b = d @ centres.T - (p * d).sum(dim=1, keepdim=True)
        vv = cc[None, :] - 2.0 * (p @ centres.T) + (p * p).sum(dim=1, keepdim=True)
        reach = radii[None, :] + q[a:a + CHUNK, None]
        disc = b * b - vv + reach * reach
        root = disc.clamp_min(0.0).sqrt()
        t = torch.where((disc >= 0) & (b + root >= 0), (b - root).clamp_min(0.0), torch.full_like(b, float("inf")))
        t.scatter_(1, me[a:a + CHUNK, None], float("inf"))
        first = t.min(dim=1)
        out.append((torch.where(first.values < tmax, first.values, torch.full_like(first.values, tmax)), first.indices))
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
    out_path = os.path.join(ROOT, "profiles", "s01_sweep_rate.json")
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
    out = {"workload": "rt_sweep_spheres_device, f32, the scene's own spheres cast from their own centres with exclude = self in random directions, "
                       "torch tensors; bars: torch all-pairs time of impact, rt_intersect_rays_device against the cast with radius 0",
           "rounds": rounds, "warm_s": WARM_S, "scenes": {}}
    for name, s in scenes:
        d = s.device()
        n = len(s.items)
        perm = rng.permutation(n)
        items = np.ascontiguousarray(s.items[perm])
        median = float(np.median(s.items[:, 3]))
        dirs_np = rng.normal(size=(n, 3))
        dirs_np = (dirs_np / np.linalg.norm(dirs_np, axis=1, keepdims=True)).astype(np.float32)
        with torch.cuda.stream(stream):
            pos = torch.from_numpy(np.ascontiguousarray(items[:, :3])).to(dev)
            dirs = torch.from_numpy(dirs_np).to(dev)
            casts = torch.cat([pos, dirs], dim=1).contiguous()
            q = torch.from_numpy(np.ascontiguousarray(items[:, 3])).to(dev)
            me = torch.from_numpy(perm.astype(np.int32)).to(dev)
            me64 = me.to(torch.int64)
            centres = torch.from_numpy(np.ascontiguousarray(s.items[:, :3])).to(dev)
            radii = torch.from_numpy(np.ascontiguousarray(s.items[:, 3])).to(dev)
            cut = {v: None if m is None else torch.full((n,), m * median, dtype=torch.float32, device=dev) for v, m in STEPS}
            order = d.sphere_order(torch.cat([pos, torch.ones((n, 1), dtype=torch.float32, device=dev)], dim=1), stream=stream)
            eye = torch.tensor(s.eye, dtype=torch.float32, device=dev)
            to = pos - eye
            eye_rays = torch.cat([eye.expand(n, 3), to / to.norm(dim=1, keepdim=True)], dim=1).contiguous()
        stream.synchronize()
        legs = {}
        for v, m in STEPS:
            for mode, a in (("nearest", False), ("any", True)):
                for batch, o in (("shuffled", None), ("sphere_order", order)):
                    legs["%s_%s/%s" % (mode, v, batch)] = (lambda v=v, a=a, o=o: d.sweep(casts, q, cut[v], any_hit=a, exclude=me, order=o, stream=stream))
            legs["torch_toi_%s" % v] = (lambda m=m: torch_pass(pos, dirs, q, me64, centres, radii, float("inf") if m is None else m * median))
        for mode, a in (("nearest", False), ("any", True)):
            legs["ray_query/%s" % mode] = (lambda a=a: d.intersect(eye_rays, any_hit=a, stream=stream))
            legs["cast_q0/%s" % mode] = (lambda a=a: d.sweep(eye_rays, any_hit=a, stream=stream))

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
        res = {"casts": n, "median_radius": median}
        for v in legs:
            med, best = float(np.median(times[v])), min(times[v])
            res[v] = {"device_ms": round(med, 4), "device_ms_min": round(best, 4), "device_ms_max": round(max(times[v]), 4), "per_s": round(n / med * 1e3),
                      "calls_per_sample": iters[v]}
        with torch.cuda.stream(stream):
            for v, m in STEPS:
                for mode, a in (("nearest", False), ("any", True)):
                    st = d.sweep(casts, q, cut[v], any_hit=a, exclude=me, stream=stream, want_stats=True)[-1]
                    for batch in ("shuffled", "sphere_order"):
                        leg = res["%s_%s/%s" % (mode, v, batch)]
                        leg.update(tests_per_cast=round(st["tests_executed"] / n, 2), contacts=st["hits"],
                                   vs_torch=round(res["torch_toi_%s" % v]["device_ms"] / leg["device_ms"], 2))
            for mode, a in (("nearest", False), ("any", True)):
                sq = d.intersect(eye_rays, any_hit=a, stream=stream, want_stats=True)[-1]
                sc = d.sweep(eye_rays, any_hit=a, stream=stream, want_stats=True)[-1]
                res["ray_query/%s" % mode]["tests_per_ray"] = round(sq["tests_executed"] / n, 2)
                res["cast_q0/%s" % mode].update(tests_per_cast=round(sc["tests_executed"] / n, 2), same_tests_as_ray_query=sc["tests_executed"] == sq["tests_executed"],
                                                vs_ray_query=round(res["cast_q0/%s" % mode]["device_ms"] / res["ray_query/%s" % mode]["device_ms"], 3))
            # the bar answers the same question: the first contact of every cast, wherever the two agree to 1e-4
            dist, _, _ = d.sweep(casts, q, cut["10"], exclude=me, stream=stream)
            tp = torch_pass(pos, dirs, q, me64, centres, radii, 10.0 * median)
            td = torch.cat([x[0] for x in tp])
        stream.synchronize()
        torch.cuda.synchronize()
        res["first_contact_max_abs_diff_vs_torch"] = float((dist - td).abs().max())
        out["scenes"][name] = res
        d.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
