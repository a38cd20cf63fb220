#!/usr/bin/env python3
"""Rates of the contact-island query rt_scene_islands_device on torch tensors: the connected groups of the scene's
contacts, margins 0 and one median item radius, measured in one process on one device against what the walk costs without the unions
and against what a caller had before this entry.

  islands_label    (a) the device entry, label and n_islands: init, the hook walk, the labels, the scan
  islands_full     (a) ... with index and size too: one more kernel
  contacts_count   (b) rt_scene_contacts_device with capacity 0: the counting walk and the scan -- the same walk, test for test, without
                   the unions
  host_islands     (c) what a caller had: the whole pair list (a counting call, then the list), its copy to the host and
                   rta.pair_islands there

(a) and (b) are timed with device events after 0.2 s of warm-up, in interleaved rounds (median and minimum over the rounds).  (c) ends
on the host, so it is timed with the host's clock around the whole call; `wall_ms` gives (a) and (b) by that clock too -- the call
and a synchronisation of its stream -- and the ratio (c) / (a) is taken on it.  The labels of (a) are compared with those of (c) once.

on the default scene (L8, a static scene) and on the 100,000 arbitrary spheres after DeviceScene.rebuild (a dynamic scene), f32.

usage: islands_rate.py [--rounds R] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/i01_islands_rate.json)"""
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
from contacts_rate import timed, warm  # noqa: E402
from tests.scenes import hundred_thousand_spheres  # noqa: E402


def wall(fn, stream, calls):
    """The median and the minimum of `calls` host-clock times of fn() followed by a synchronisation of the stream, in ms."""
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts)


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "i01_islands_rate.json")
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
        raise SystemExit("islands_rate.py: no gfx950 device visible; nothing is measured without one")
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

    scenes = [("default_L8", lambda: static(8)), ("100k_rebuilt", rebuilt)]
    out = {"workload": "rt_scene_islands_device, f32, torch tensors; (b) rt_scene_contacts_device capacity 0; (c) the pair list, its host copy, rta.pair_islands",
           "rounds": rounds, "scenes": {}}
    for name, make in scenes:
        d, items = make()
        n = len(items)
        r_med = float(np.median(items[:, 3]))
        res = {"items": n, "median_radius": r_med}
        for label, margin in (("margin_0", 0.0), ("margin_median_radius", r_med)):
            def on_stream(fn):
                def run():
                    with torch.cuda.stream(stream):
                        return fn()
                return run

            def host_islands():
                pairs, total = d.contacts(margin, device=True, stream=stream)    # counts, reads the count back, lists
                return rta.pair_islands(pairs.cpu().numpy(), n), total
            legs = {"islands_label": on_stream(lambda: d.islands(margin, device=True, stream=stream)),
                    "islands_full": on_stream(lambda: d.islands(margin, index=True, sizes=True, device=True, stream=stream)),
                    "contacts_count": on_stream(lambda: d.contacts(margin, 0, device=True, stream=stream))}
            iters = {v: warm(fn, stream) for v, fn in legs.items()}
            times = {v: [] for v in legs}
            for _ in range(rounds):
                for v, fn in legs.items():
                    times[v].append(timed(fn, stream, iters[v]))
            legs["host_islands"] = on_stream(host_islands)
            legs["host_islands"]()                                               # (warm: the first list call sizes torch's pool)
            stream.synchronize()
            walls = {v: wall(fn, stream, 5 * rounds) for v, fn in legs.items()}
            ref, total = legs["host_islands"]()
            got = legs["islands_full"]()
            stream.synchronize()
            leg = {"pairs": total, "islands": ref[3], "largest_island": int(ref[2].max()),
                   "labels_agree": bool(np.array_equal(got[0].cpu().numpy(), ref[0]) and np.array_equal(got[1].cpu().numpy(), ref[1])
                                        and np.array_equal(got[2].cpu().numpy(), ref[2]) and int(got[3].item()) == ref[3])}
            for v in legs:
                leg[v] = {"wall_ms": round(walls[v][0], 4), "wall_ms_min": round(walls[v][1], 4)}
                if v in times:
                    leg[v].update(device_ms=round(float(np.median(times[v])), 4), device_ms_min=round(min(times[v]), 4), calls_per_sample=iters[v])
            for v in ("islands_label", "islands_full"):
                leg[v]["a_over_b_device"] = round(leg[v]["device_ms"] / leg["contacts_count"]["device_ms"], 3)
                leg[v]["a_over_b_wall"] = round(leg[v]["wall_ms"] / leg["contacts_count"]["wall_ms"], 3)
                leg[v]["c_over_a_wall"] = round(leg["host_islands"]["wall_ms"] / leg[v]["wall_ms"], 2)
            st = d.islands(margin, stats=True, device=True, stream=stream)[-1]
            leg["tests_per_item"] = round(st["tests_executed"] / n, 2)
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
