#!/usr/bin/env python3
"""Rates of the box overlap lists rt_overlap_boxes_device on torch tensors, timed with device events after warm-up: every
sphere of the scene that touches each query box (margin 0).  Three sets of boxes per scene, in the order they come in (no `order`):

  cubes            the items' own bounding cubes [c - r, c + r], as many boxes as the scene has items
  flat             boxes of the same volume about the same centres, 8 x 8 x 1/64 of the cube's side: a trigger volume, a floor tile
  large            64 boxes of half the scene's extent on every axis -- an eighth of its volume each -- at seeded places inside it: the
                   case one box per lane serves worst (one lane lists thousands of entries)

  box_count        capacity 0: the counting walk and the scan -- "how many"
  box_list         capacity = the total, gaps and offsets too: the counting walk, the scan and the fill walk -- the whole list

The bars, measured in the same run on the same device:

  sphere_list      what a caller had before: rt_overlap_spheres_device with each box's circumscribed sphere, the whole list.  Its entry
                   count stands next to the box list's (`sphere_entries`, `superset`): the caller still has to copy that superset and
                   filter it, which is not timed
  torch_all_pairs  the distance from every box to every centre minus the radius, below the margin, then nonzero, in chunks of 2,048 boxes

and one more row per scene, `points`: the items' centres as point boxes against rt_overlap_spheres_device with q = 0 -- the same entries,
and what two more registers of query cost.

on the default scene at L8 and L9 (static scenes) and on the 100,000 arbitrary spheres after DeviceScene.rebuild (a dynamic scene), f32.
Every leg is warmed up for 0.2 s, then timed in interleaved rounds (median and minimum over the rounds); tests per box come from one
counting call.  A list of more than 2^29 entries is not made: its leg reads null.

usage: box_rate.py [--rounds R] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/b02_box_rate.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
import rust_tracer_amd as rta  # noqa: E402
from overlap_rate import WARM_S, timed, warm  # noqa: E402
from tests.scenes import hundred_thousand_spheres  # noqa: E402

CHUNK, MOST = 2048, 1 << 29


def torch_pass(lo, hi, centres, radii, margin):
    """The all-pairs bar: per chunk of boxes, the distance to every centre minus the radius below the margin, nonzero."""
    out = []
    for a in range(0, lo.shape[0], CHUNK):
        dd = None
        for k in range(3):
            c = centres[None, :, k]
            e = torch.maximum(lo[a:a + CHUNK, k, None] - c, c - hi[a:a + CHUNK, k, None]).clamp_(min=0)
            dd = e * e if dd is None else dd.addcmul_(e, e)
        out.append(((dd.sqrt_() - radii[None, :]) < margin).nonzero())
    return out


def box_sets(items):
    """name -> float32[n, 6]"""
    c, r = items[:, :3].astype(np.float64), items[:, 3:4].astype(np.float64)
    flat = r * np.array([8.0, 8.0, 1.0 / 64.0])
    lo, hi = (c - r).min(axis=0), (c + r).max(axis=0)
    size = 0.5 * (hi - lo)
    at = lo + np.random.default_rng(19).uniform(0.0, 1.0, (64, 3)) * (hi - lo - size)
    sets = {"cubes": np.concatenate([c - r, c + r], axis=1), "flat": np.concatenate([c - flat, c + flat], axis=1), "large": np.concatenate([at, at + size], axis=1)}
    return {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in sets.items()}


def circumscribed(boxes):
    """float32[n, 4]: the smallest sphere around each box, rounded up"""
    b = boxes.astype(np.float64)
    q = 0.5 * np.sqrt(((b[:, 3:] - b[:, :3]) ** 2).sum(axis=1))
    return np.ascontiguousarray(np.concatenate([0.5 * (b[:, :3] + b[:, 3:]), q[:, None] * (1.0 + 1e-6)], axis=1).astype(np.float32))


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "b02_box_rate.json")
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
        raise SystemExit("box_rate.py: no gfx950 device visible; nothing is measured without one")
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

    def count_of(call):
        total = call()[1]
        stream.synchronize()                                         # (the count belongs to `stream`)
        return int(total.item())

    def measure(legs):
        """name -> {device_ms, device_ms_min, calls_per_sample}; a leg that is None reads None"""
        legs = {v: fn for v, fn in legs.items() if fn is not None}
        iters = {v: warm(fn, stream) for v, fn in legs.items()}
        times = {v: [] for v in legs}
        for _ in range(rounds):
            for v, fn in legs.items():
                times[v].append(timed(fn, stream, iters[v]))
        return {v: {"device_ms": round(float(np.median(times[v])), 4), "device_ms_min": round(min(times[v]), 4), "calls_per_sample": iters[v]} for v in legs}

    margin = 0.0
    scenes = [("default_L8", lambda: static(8)), ("default_L9", lambda: static(9)), ("100k_rebuilt", rebuilt)]
    out = {"workload": "rt_overlap_boxes_device, f32, torch tensors, margin 0; bars: rt_overlap_spheres_device with each box's circumscribed sphere, "
                       "a torch all-pairs pass",
           "rounds": rounds, "warm_s": WARM_S, "scenes": {}}
    for name, make in scenes:
        d, items = make()
        n = len(items)
        with torch.cuda.stream(stream):
            centres = torch.from_numpy(np.ascontiguousarray(items[:, :3], dtype=np.float32)).to(dev)
            radii = torch.from_numpy(np.ascontiguousarray(items[:, 3], dtype=np.float32)).to(dev)
        stream.synchronize()
        res = {"items": n}
        for set_name, boxes in box_sets(items).items():
            with torch.cuda.stream(stream):
                db = torch.from_numpy(boxes).to(dev)
                dq = torch.from_numpy(circumscribed(boxes)).to(dev)
                lo, hi = db[:, :3].contiguous(), db[:, 3:].contiguous()
            total = count_of(lambda: d.box_overlaps(db, margin, capacity=0, stream=stream))
            superset = count_of(lambda: d.overlaps(dq, margin, capacity=0, stream=stream))
            legs = {"box_count": on_stream(lambda: d.box_overlaps(db, margin, capacity=0, stream=stream)),
                    "box_list": on_stream(lambda: d.box_overlaps(db, margin, capacity=total, gaps=True, offsets=True, stream=stream)) if total <= MOST else None,
                    "sphere_list": on_stream(lambda: d.overlaps(dq, margin, capacity=superset, gaps=True, offsets=True, stream=stream)) if superset <= MOST else None,
                    "torch_all_pairs": on_stream(lambda: torch_pass(lo, hi, centres, radii, margin))}
            leg = {"boxes": len(boxes), "entries": total, "sphere_entries": superset, "superset": round(superset / max(total, 1), 2)}
            leg.update({v: None for v in legs})
            leg.update(measure(legs))
            for v in ("box_count", "box_list"):
                for bar in ("sphere_list", "torch_all_pairs"):
                    if leg[v] and leg[bar]:
                        leg[v]["vs_" + bar] = round(leg[bar]["device_ms"] / leg[v]["device_ms"], 2)
            if leg["box_list"]:
                leg["list_over_count"] = round(leg["box_list"]["device_ms"] / leg["box_count"]["device_ms"], 2)
            st = d.box_overlaps(db, margin, capacity=0, stats=True, stream=stream)[-1]
            leg["tests_per_box"] = round(st["tests_executed"] / len(boxes), 2)
            leg["boxes_with_an_entry"] = st["hits"]
            offsets = d.box_overlaps(db, margin, capacity=0, offsets=True, stream=stream)[1]
            nz = legs["torch_all_pairs"]()
            stream.synchronize()
            leg["longest_row"] = int(np.diff(offsets.cpu().numpy()).max())
            leg["entries_vs_torch"] = total - sum(int(x.shape[0]) for x in nz)
            res[set_name] = leg
        # point boxes against the overlap lists at q = 0: the same entries, two more registers of query
        with torch.cuda.stream(stream):
            dp = torch.cat([centres, centres], dim=1).contiguous()
            dz = torch.cat([centres, torch.zeros_like(radii)[:, None]], dim=1).contiguous()
        total = count_of(lambda: d.box_overlaps(dp, margin, capacity=0, stream=stream))
        same = count_of(lambda: d.overlaps(dz, margin, capacity=0, stream=stream))
        leg = {"boxes": n, "entries": total, "sphere_entries": same}
        leg.update(measure({"box_count": on_stream(lambda: d.box_overlaps(dp, margin, capacity=0, stream=stream)),
                            "box_list": on_stream(lambda: d.box_overlaps(dp, margin, capacity=total, gaps=True, offsets=True, stream=stream)),
                            "sphere_count": on_stream(lambda: d.overlaps(dz, margin, capacity=0, stream=stream)),
                            "sphere_list": on_stream(lambda: d.overlaps(dz, margin, capacity=same, gaps=True, offsets=True, stream=stream))}))
        leg["box_over_sphere_count"] = round(leg["box_count"]["device_ms"] / leg["sphere_count"]["device_ms"], 3)
        leg["box_over_sphere_list"] = round(leg["box_list"]["device_ms"] / leg["sphere_list"]["device_ms"], 3)
        res["points"] = leg
        out["scenes"][name] = res
        d.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
