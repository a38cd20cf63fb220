#!/usr/bin/env python3
"""Rates of the overlap-list query rt_overlap_spheres_device on torch tensors, timed with device events after warm-up:
every sphere of the scene within a margin of each query sphere, margins 0 and one skin (the median item radius).  Two sets of queries
per scene, each as many as the scene has items, in the order they come in (no `order`):

  own              the scene's own spheres put in as outside queries (no exclude: every sphere lists itself too)
  jittered         copies of them, every centre moved by a normal step of one median radius

  overlap_count    capacity 0: the counting walk and the scan -- "how many"
  overlap_list     capacity = the total, gaps and offsets too: the counting walk, the scan and the fill walk of the queries that counted
                   something -- the whole list

The bars, measured in the same run on the same device:

  near_all_16      rt_near_spheres_device RT_NEAR_ALL k = 16 over the same centres with radius = margin + q: the same tests as the counting
                   walk, one walk, and a query with more than 16 entries gets 16 of them (`truncated` counts those queries)
  torch_cdist      cdist(query centres, scene centres) - r - q < margin, then nonzero, in chunks of 8,192 rows
  contacts_count   rt_scene_contacts_device on the same scene and margin, capacity 0 ...
  contacts_list    ... and the whole list: the parent of the two-pass scheme, whose list walks everything twice

on the default scene at L8 and L9 (static scenes) and on the 100,000 arbitrary spheres after DeviceScene.rebuild (a dynamic scene), f32.
Every leg is warmed up for 0.2 s, then timed in interleaved rounds (median and minimum over the rounds); tests per query come from one
counting call.  `list_over_count` is the ratio the fill pass's skip is about, next to the contacts legs' of the same run.
`entries_vs_near` is the entry count minus the sum of near's `found` (0: both walks make the same decisions); `entries_vs_torch` the
difference to the torch pass, which forms its distances through a matrix product (gaps within its error of the margin fall on either
side: the pyramid's spheres touch their parents exactly).

usage: overlap_rate.py [--rounds R] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/o01_overlap_rate.json)"""
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


def torch_pass(qc, qr, centres, radii, margin):
    """The all-pairs bar: per chunk of queries, cdist minus both radii below the margin, nonzero."""
    out = []
    for a in range(0, qc.shape[0], CHUNK):
        gap = torch.cdist(qc[a:a + CHUNK], centres) - radii[None, :] - qr[a:a + CHUNK, None]
        out.append((gap < margin).nonzero())
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
    out_path = os.path.join(ROOT, "profiles", "o01_overlap_rate.json")
    rounds = 5
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    if "--rounds" in args:
        i = args.index("--rounds")
        rounds = int(args[i + 1])
        del args[i:i + 2]
    if rta.device_count() < 1:
        raise SystemExit("overlap_rate.py: no gfx950 device visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)

    def static(level):
        s = rta.Scene.default(level)
        return s.device(), np.asarray(s.items)

    def rebuilt():
        sp = np.ascontiguousarray(hundred_thousand_spheres(), dtype=np.float32)
        d = rta.DeviceScene(rta.Scene.from_spheres_balanced(sp, leaf_size=4), 0, True)
        order = d.rebuild(sp)
        return d, sp[order]

    def on_stream(fn):
        def run():
            with torch.cuda.stream(stream):
                return fn()
        return run

    scenes = [("default_L8", lambda: static(8)), ("default_L9", lambda: static(9)), ("100k_rebuilt", rebuilt)]
    out = {"workload": "rt_overlap_spheres_device, f32, torch tensors; bars: rt_near_spheres_device ALL k = 16 over the same centres, torch cdist, "
                       "rt_scene_contacts_device on the same scene",
           "rounds": rounds, "warm_s": WARM_S, "scenes": {}}
    for name, make in scenes:
        d, items = make()
        n = len(items)
        r_med = float(np.median(items[:, 3]))
        own = np.ascontiguousarray(items, dtype=np.float32).copy()
        own[:, 3] = np.sqrt(own[:, 3] * own[:, 3])
        jit = own.copy()
        jit[:, :3] += (np.random.default_rng(17).normal(size=(n, 3)) * r_med).astype(np.float32)
        with torch.cuda.stream(stream):
            centres = torch.from_numpy(np.ascontiguousarray(items[:, :3])).to(dev)
            radii = torch.from_numpy(np.ascontiguousarray(items[:, 3])).to(dev)
        stream.synchronize()
        res = {"items": n, "queries": n, "median_radius": r_med}
        for label, margin in (("margin_0", 0.0), ("margin_median_radius", r_med)):
            row = {}
            for qname, q in (("own", own), ("jittered", jit)):
                with torch.cuda.stream(stream):
                    dq = torch.from_numpy(q).to(dev)
                    qc = dq[:, :3].contiguous()
                    qr = dq[:, 3].contiguous()
                    rho = (qr + np.float32(margin)).contiguous()
                total = d.overlaps(dq, margin, capacity=0, stream=stream)[1]
                stream.synchronize()                                 # (the count belongs to `stream`)
                total = int(total.item())
                legs = {"overlap_count": on_stream(lambda: d.overlaps(dq, margin, capacity=0, stream=stream)),
                        "overlap_list": on_stream(lambda: d.overlaps(dq, margin, capacity=total, gaps=True, offsets=True, stream=stream)),
                        "near_all_16": on_stream(lambda: d.near(qc, 16, rho, all_within=True, stream=stream)),
                        "torch_cdist": on_stream(lambda: torch_pass(qc, qr, centres, radii, margin))}
                if qname == "own":
                    pairs = d.contacts(margin, 0, device=True, stream=stream)[1]
                    stream.synchronize()
                    pairs = int(pairs.item())
                    legs["contacts_count"] = on_stream(lambda: d.contacts(margin, 0, device=True, stream=stream))
                    legs["contacts_list"] = on_stream(lambda: d.contacts(margin, pairs, gaps=True, offsets=True, device=True, stream=stream))
                iters = {v: warm(fn, stream) for v, fn in legs.items()}
                times = {v: [] for v in legs}
                for _ in range(rounds):
                    for v, fn in legs.items():
                        times[v].append(timed(fn, stream, iters[v]))
                leg = {"entries": total}
                for v in legs:
                    med, best = float(np.median(times[v])), min(times[v])
                    leg[v] = {"device_ms": round(med, 4), "device_ms_min": round(best, 4), "calls_per_sample": iters[v]}
                for v in ("overlap_count", "overlap_list"):
                    for bar in ("near_all_16", "torch_cdist"):
                        leg[v]["vs_" + bar] = round(leg[bar]["device_ms"] / leg[v]["device_ms"], 2)
                leg["list_over_count"] = round(leg["overlap_list"]["device_ms"] / leg["overlap_count"]["device_ms"], 2)
                if qname == "own":
                    leg["contact_pairs"] = pairs
                    leg["contacts_list_over_count"] = round(leg["contacts_list"]["device_ms"] / leg["contacts_count"]["device_ms"], 2)
                st = d.overlaps(dq, margin, capacity=0, stats=True, stream=stream)[-1]
                leg["tests_per_query"] = round(st["tests_executed"] / n, 2)
                leg["queries_with_an_entry"] = st["hits"]
                found = legs["near_all_16"]()[2]
                nz = legs["torch_cdist"]()
                stream.synchronize()
                found = found.cpu().numpy().astype(np.int64)
                leg["near_all_16"].update(found_sum=int(found.sum()), truncated=int((found > 16).sum()), longest_row=int(found.max()))
                leg["entries_vs_near"] = total - int(found.sum())
                leg["entries_vs_torch"] = total - sum(int(x.shape[0]) for x in nz)
                row[qname] = leg
            res[label] = row
        out["scenes"][name] = res
        d.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
