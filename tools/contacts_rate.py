#!/usr/bin/env python3
"""Rates of the contact-pair query rt_scene_contacts_device on torch tensors, timed with device events after warm-up:
every pair of spheres of the scene closer than a margin, margins 0 and one median item radius.

  contacts_count   capacity 0: the counting walk and the scan -- "how many"
  contacts_list    capacity = the total, gaps and offsets too: both walks and the scan, the whole list

The bars, measured in the same run on the same device, are what a caller had before this entry:

  near_all_16      rt_near_spheres_device RT_NEAR_ALL k = 16 over every centre with exclude = self and radius = margin + the sphere's own
                   radius: every pair is found twice, and a sphere with more than 16 neighbours gets 16 of them (`truncated` counts those)
  torch_all_pairs  cdist(centres, centres) - r_i - r_j < margin over j > i, then nonzero, in chunks of 8,192 rows

on the default scene at L8 and L9 (static scenes) and on the 100,000 arbitrary spheres after DeviceScene.rebuild (a dynamic scene), f32.
Every leg is warmed up for 0.2 s, then timed in interleaved rounds (median and minimum over the rounds); tests per item come from one
counting call.  `pairs_vs_near` is twice the pair count minus the sum of near's `found` (0 unless a gap grazes the margin);
`pairs_vs_torch` is the difference of the two pair counts -- cdist forms its distances through a matrix product, so pairs whose gap is
within its error of the margin fall on either side (the pyramid's spheres touch their parents exactly: at margin 0 all of those do).

usage: contacts_rate.py [--rounds R] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/c01_contacts_rate.json)"""
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


def torch_pass(centres, radii, margin):
    """The all-pairs bar: per chunk of rows, cdist minus both radii below the margin, the upper triangle, nonzero."""
    out = []
    n = centres.shape[0]
    cols = torch.arange(n, device=centres.device)
    for a in range(0, n, CHUNK):
        gap = torch.cdist(centres[a:a + CHUNK], centres) - radii[None, :] - radii[a:a + CHUNK, None]
        hit = (gap < margin) & (cols[None, :] > cols[a:a + CHUNK, None])
        out.append(hit.nonzero())
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
    out_path = os.path.join(ROOT, "profiles", "c01_contacts_rate.json")
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
        raise SystemExit("contacts_rate.py: no gfx950 device visible; nothing is measured without one")
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

    scenes = [("default_L8", lambda: static(8)), ("default_L9", lambda: static(9)), ("100k_rebuilt", rebuilt)]
    out = {"workload": "rt_scene_contacts_device, f32, torch tensors; bars: rt_near_spheres_device ALL k = 16 over every centre, torch all-pairs",
           "rounds": rounds, "warm_s": WARM_S, "scenes": {}}
    for name, make in scenes:
        d, items = make()
        n = len(items)
        r_med = float(np.median(items[:, 3]))
        with torch.cuda.stream(stream):
            centres = torch.from_numpy(np.ascontiguousarray(items[:, :3])).to(dev)
            radii = torch.from_numpy(np.ascontiguousarray(items[:, 3])).to(dev)
            me = torch.arange(n, dtype=torch.int32, device=dev)
        stream.synchronize()
        res = {"items": n, "median_radius": r_med}
        for label, margin in (("margin_0", 0.0), ("margin_median_radius", r_med)):
            total = d.contacts(margin, 0, device=True, stream=stream)[1]
            stream.synchronize()                                     # (the count belongs to `stream`)
            total = int(total.item())
            with torch.cuda.stream(stream):
                rho = (radii + np.float32(margin)).contiguous()

            def on_stream(fn):
                def run():
                    with torch.cuda.stream(stream):
                        return fn()
                return run
            legs = {"contacts_count": on_stream(lambda: d.contacts(margin, 0, device=True, stream=stream)),
                    "contacts_list": on_stream(lambda: d.contacts(margin, total, gaps=True, offsets=True, device=True, stream=stream)),
                    "near_all_16": on_stream(lambda: d.near(centres, 16, rho, all_within=True, exclude=me, stream=stream)),
                    "torch_all_pairs": on_stream(lambda: torch_pass(centres, radii, margin))}
            iters = {v: warm(fn, stream) for v, fn in legs.items()}
            times = {v: [] for v in legs}
            for _ in range(rounds):
                for v, fn in legs.items():
                    times[v].append(timed(fn, stream, iters[v]))
            leg = {"pairs": total}
            for v in legs:
                med, best = float(np.median(times[v])), min(times[v])
                leg[v] = {"device_ms": round(med, 4), "device_ms_min": round(best, 4), "calls_per_sample": iters[v]}
            for v in ("contacts_count", "contacts_list"):
                for bar in ("near_all_16", "torch_all_pairs"):
                    leg[v]["vs_" + bar] = round(leg[bar]["device_ms"] / leg[v]["device_ms"], 2)
            st = d.contacts(margin, 0, stats=True, device=True, stream=stream)[-1]
            leg["tests_per_item"] = round(st["tests_executed"] / n, 2)
            leg["items_with_a_pair_as_lower_slot"] = st["hits"]
            found = legs["near_all_16"]()[2]
            nz = legs["torch_all_pairs"]()
            stream.synchronize()
            found = found.cpu().numpy().astype(np.int64)
            leg["near_all_16"].update(found_sum=int(found.sum()), truncated=int((found > 16).sum()), most_neighbours=int(found.max()))
            leg["pairs_vs_near"] = 2 * total - int(found.sum())     # every pair twice, counted in full even where the list is truncated
            leg["pairs_vs_torch"] = total - sum(int(x.shape[0]) for x in nz)
            res[label] = leg
        out["scenes"][name] = res
        d.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
