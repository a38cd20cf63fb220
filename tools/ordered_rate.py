#!/usr/bin/env python3
"""What ordering a ray batch on the device buys (rt_ray_order_device, rt_*_ordered_device; csrc/rt_order.hpp), timed with
device events after warm-up, the legs of a case interleaved round by round, medians over the rounds (the method of undersample_rate.py).

Per scene (default L8, L9, the 100,000-sphere scene; f32), query (nearest hit, multi-hit k = 16 closest) and batch (tools/query_rate.py's:
"camera" 1920x1080 primary rays in pixel order, "shuffled" the same rays in a random order, "random" 2M rays inside the root bound):
  a_unordered_ms     the unordered entry: the bar, today's kernel in the same run; a_spread_ms = its largest minus its smallest round
  b_ordered_ms       the ordered walk with a precomputed order (rt_ray_order_device's)
  c_order_ms         rt_ray_order_device alone: box, keys and the radix sort
  d_one_call_ms      the one-call form (order == NULL): c + b in one call
  d_beats_a          d < a by more than a's spread
"random" also walks in the order of a 6-D interleave of origin and direction bits (5 bits each, made with numpy): b6_interleave_ms, the
layout the shipped key was measured against.

usage: ordered_rate.py [iterations] [--rounds N] [--out PATH]
       prints one JSON line and writes it to PATH (default profiles/o01_ordered_rate.json)"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
import rust_tracer_amd as rta  # noqa: E402
from rust_tracer_amd import capi  # noqa: E402
from tests.scenes import hundred_thousand_spheres  # noqa: E402
from tools.query_rate import camera_rays  # noqa: E402
from tools.undersample_rate import warm, once  # noqa: E402

K = 16


def interleave6_order(rays):
    """The alternative layout: 5 bits of each of pos.xyz (over the batch's box) and dir.xyz, bit-interleaved, most significant first."""
    r = rays.astype(np.float64)
    lo, hi = r[:, :3].min(axis=0), r[:, :3].max(axis=0)
    ext = np.where(hi > lo, hi - lo, 1.0)
    q = np.concatenate([np.minimum(((r[:, :3] - lo) / ext * 32).astype(np.uint32), 31), np.minimum(((r[:, 3:] + 1.0) * 16).astype(np.uint32), 31)], axis=1)
    key = np.zeros(len(r), dtype=np.uint32)
    for bit in range(5):
        for c in range(6):
            key |= ((q[:, c] >> np.uint32(bit)) & np.uint32(1)) << np.uint32(6 * bit + c)
    return np.argsort(key, kind="stable").astype(np.uint32)


def case(d, rays, query, batch, iters, rounds, stream, dev):
    n = len(rays)
    lib, h, hs = capi.lib, d._h, C.c_void_p(stream.cuda_stream)
    with torch.cuda.stream(stream):
        tr = torch.from_numpy(np.ascontiguousarray(rays)).to(dev)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        k = K if query == "multi16" else 1
        dist = torch.empty(n * k, dtype=torch.float32, device=dev)
        nrm = torch.empty(n * k * 3, dtype=torch.float32, device=dev)
        item = torch.empty(n * k, dtype=torch.int32, device=dev)
        hits = torch.empty(n, dtype=torch.int32, device=dev)
        o6 = torch.from_numpy(interleave6_order(rays).view(np.int32)).to(dev) if batch == "random" else None
    p = lambda t: C.c_void_p(t.data_ptr())

    def walk(ordered, ordp):
        if query == "nearest":
            if not ordered:
                return lib.rt_intersect_rays_device(h, capi.RT_QUERY_NEAREST, p(tr), None, n, p(dist), p(nrm), p(item), hs, None)
            return lib.rt_intersect_rays_ordered_device(h, capi.RT_QUERY_NEAREST, p(tr), None, n, ordp, p(dist), p(nrm), p(item), hs, None)
        if not ordered:
            return lib.rt_intersect_rays_multi_device(h, capi.RT_MULTIHIT_CLOSEST, K, p(tr), None, n, p(dist), p(nrm), p(item), p(hits), hs, None)
        return lib.rt_intersect_rays_multi_ordered_device(h, capi.RT_MULTIHIT_CLOSEST, K, p(tr), None, n, ordp, p(dist), p(nrm), p(item), p(hits), hs, None)

    def checked(rc):
        capi.check(rc, "ordered_rate")

    checked(lib.rt_ray_order_device(h, p(tr), n, p(order), hs))
    legs = {"a": lambda: checked(walk(False, None)), "b": lambda: checked(walk(True, p(order))),
            "c": lambda: checked(lib.rt_ray_order_device(h, p(tr), n, p(order), hs)), "d": lambda: checked(walk(True, None))}
    if o6 is not None:
        legs["b6"] = lambda: checked(walk(True, p(o6)))
    times = {name: [] for name in legs}
    its = {}
    for name, fn in legs.items():
        warm(fn, stream)
        its[name] = max(2, min(iters, int(60.0 / max(once(fn, 1, stream), 1e-3))))       # (about 60 ms of device time per timed round)
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(once(fn, its[name], stream))
    med = {name: statistics.median(v) for name, v in times.items()}
    spread = max(times["a"]) - min(times["a"])
    r = {"rays": n, "a_unordered_ms": round(med["a"], 4), "a_spread_ms": round(spread, 4), "b_ordered_ms": round(med["b"], 4),
         "c_order_ms": round(med["c"], 4), "d_one_call_ms": round(med["d"], 4), "d_over_a": round(med["d"] / med["a"], 4),
         "d_beats_a": bool(med["d"] < med["a"] - spread),
         "spreads_ms": {name: round(max(v) - min(v), 4) for name, v in times.items()}}
    if o6 is not None:
        r["b6_interleave_ms"] = round(med["b6"], 4)
    return r


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "o01_ordered_rate.json")
    rounds = 5
    for flag in ("--out", "--rounds"):
        if flag in args:
            k = args.index(flag)
            if flag == "--out":
                out_path = args[k + 1]
            else:
                rounds = int(args[k + 1])
            del args[k:k + 2]
    iters = int(args[0]) if args else 20
    rng = np.random.default_rng(1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    info = capi.build_info()
    out = {"workload": "rt_ray_order_device and the ordered walks against the unordered entries, f32, torch tensors",
           "iterations": iters, "rounds": rounds, "kernel_src_sha": info.split("kernel sources ")[-1].split()[0] if "kernel sources " in info else "",
           "cases": {}}
    scenes = [("default_L8", lambda: rta.Scene.default(8)), ("default_L9", lambda: rta.Scene.default(9)),
              ("100k", lambda: rta.Scene.from_spheres_auto(hundred_thousand_spheres()))]
    for name, make in scenes:
        s = make()
        d = s.device()
        cam = camera_rays(1920, 1080, s.eye)
        root = s.bounds[0].astype(np.float64)
        n = 2 << 20
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = root[:3] + rng.normal(size=(n, 3)) / np.sqrt(3) * root[3] * 0.5
        o = np.where(np.linalg.norm(o - root[:3], axis=1, keepdims=True) < root[3], o, root[:3])
        batches = (("camera", cam), ("shuffled", cam[rng.permutation(len(cam))]), ("random", np.concatenate([o, u], axis=1).astype(np.float32)))
        for query in ("nearest", "multi16"):
            for batch, rays in batches:
                out["cases"]["%s_%s_%s" % (name, query, batch)] = case(d, rays, query, batch, iters, rounds, stream, dev)
        # the price of the gather and the scatter: the ordered walk of the shuffled batch against the unordered walk of the camera batch
        for query in ("nearest", "multi16"):
            c = out["cases"]
            c["%s_%s_shuffled" % (name, query)]["b_over_camera_a"] = round(
                c["%s_%s_shuffled" % (name, query)]["b_ordered_ms"] / c["%s_%s_camera" % (name, query)]["a_unordered_ms"], 4)
        d.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
