#!/usr/bin/env python3
"""Rates of the region overlap lists rt_overlap_regions_device on torch tensors, timed with device events after warm-up
(tools/box_rate.py's method): every sphere of the scene that reaches into each convex region of six planes (margin 0).  Sets of regions
per scene:

  frusta_1 / _8 / _64   the frame of a look_at camera that sees the whole scene, as one frustum (rta.camera_planes), and cut into 4 x 2 and
                        8 x 8 screen rectangles: the question a renderer asks first
  large                 the 64 `large` boxes of tools/box_rate.py (half the scene's extent on every axis each) as six planes each
                        (rta.box_planes): the row of profiles/b02_box_rate.json the wide walk was built for
  small                 the items' own bounding cubes, each turned about its centre by a seeded rotation: as many regions as items --
                        the case one volume per lane serves best

  region_count          capacity 0, sections 0 (the library's rule): the counting walk, the scan and the rows -- "how many"
  region_list           capacity = the total, gaps and offsets too: the whole list
  sweep                 region_list with sections = 1, 2, 4, ... as far as the stream and n * J <= 2^26 allow (frusta_1, large and, up to
                        64, small): what fixed the constants of the rule for sections = 0

The bars, measured in the same run on the same device:

  box_list              large and small: rt_overlap_boxes_device, the whole list, on the same boxes (small: the cubes before they are turned) --
                        one volume per lane
  torch_all_pairs       the region metric for every (region, centre) in torch, below the margin, then nonzero, in chunks of 2,048 regions

on the default scene at L8 and L9 (static scenes) and on the 100,000 arbitrary spheres after DeviceScene.rebuild (a dynamic scene), f32.
Every leg is warmed up for 0.2 s, then timed in interleaved rounds (median and minimum over the rounds); tests per region come from one
counting call each at the rule's J and at J = 1, the one-lane walk.

usage: region_rate.py [--rounds R] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/g01_region_rate.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
import rust_tracer_amd as rta  # noqa: E402
from rust_tracer_amd.scene import REGION_LANES, REGION_MAX_COUNTS, REGION_SECTION_NODES  # noqa: E402
from box_rate import box_sets  # noqa: E402
from overlap_rate import WARM_S, timed, warm  # noqa: E402
from tests.scenes import hundred_thousand_spheres  # noqa: E402

CHUNK, MOST = 2048, 1 << 29
WIDTH, HEIGHT = 1920, 1080


def torch_pass(planes, centres, radii, margin):
    """The all-pairs bar: per chunk of regions the largest of the six plane distances of every centre, minus the radius, below the margin,
    nonzero.  planes: [n, 6, 4]."""
    out = []
    for a in range(0, planes.shape[0], CHUNK):
        p = planes[a:a + CHUNK]
        m = None
        for k in range(6):
            s = torch.addmm(p[:, k, 3:4].expand(-1, centres.shape[0]), p[:, k, :3], centres.t())      # n_k . c + d_k
            m = s if m is None else torch.maximum(m, s)
        out.append(((m - radii[None, :]) < margin).nonzero())
    return out


def region_sets(items):
    """name -> (float32[n, 6, 4], float32[n, 6] boxes for the box entry or None)"""
    c, r = items[:, :3].astype(np.float64), items[:, 3:4].astype(np.float64)
    lo, hi = (c - r).min(axis=0), (c + r).max(axis=0)
    mid, ext = 0.5 * (lo + hi), float(0.5 * (hi - lo).max())
    cam = rta.look_at(mid + ext * np.array([0.9, 0.7, -2.2]), mid, hfov_deg=60.0)
    sets = {"frusta_1": (rta.camera_planes(cam, WIDTH, HEIGHT), None)}
    for name, (nx, ny) in (("frusta_8", (4, 2)), ("frusta_64", (8, 8))):
        w, h = WIDTH // nx, HEIGHT // ny
        rects = [(x * w, (y + 1) * h, (x + 1) * w, y * h) for y in range(ny) for x in range(nx)]
        sets[name] = (np.concatenate([rta.camera_planes(cam, WIDTH, HEIGHT, rect) for rect in rects]), None)
    large = box_sets(items)["large"]
    sets["large"] = (rta.box_planes(large[:, :3], large[:, 3:]), large)
    rng = np.random.default_rng(23)
    rot = np.linalg.qr(rng.normal(size=(len(items), 3, 3)))[0]
    cubes = np.ascontiguousarray(np.concatenate([c - r, c + r], axis=1).astype(np.float32))
    sets["small"] = (rta.box_planes(cubes[:, :3], cubes[:, 3:], rot), cubes)
    return {k: (np.ascontiguousarray(p, dtype=np.float32), b) for k, (p, b) in sets.items()}


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "g01_region_rate.json")
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
        raise SystemExit("region_rate.py: no gfx950 device visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)

    def static(level):
        s = rta.Scene.default(level)
        return s.device(), np.asarray(s.items), len(s.items) + sum(1 for rg in s.ranges if rg[1] > 0)

    def rebuilt():
        sp = np.ascontiguousarray(hundred_thousand_spheres(), dtype=np.float32)
        s = rta.Scene.from_spheres_balanced(sp, leaf_size=4)
        d = rta.DeviceScene(s, 0, True)
        order = d.rebuild(sp)
        return d, sp[order], len(s.items) + sum(1 for rg in s.ranges if rg[1] > 0)

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
    out = {"workload": "rt_overlap_regions_device, f32, torch tensors, margin 0; bars: rt_overlap_boxes_device on the same boxes, a torch all-pairs pass "
                       "of the region metric", "rounds": rounds, "warm_s": WARM_S,
           "rule": {"lanes": REGION_LANES, "section_nodes": REGION_SECTION_NODES}, "scenes": {}}
    for name, make in scenes:
        d, items, n_nodes = make()
        with torch.cuda.stream(stream):
            centres = torch.from_numpy(np.ascontiguousarray(items[:, :3], dtype=np.float32)).to(dev)
            radii = torch.from_numpy(np.ascontiguousarray(items[:, 3], dtype=np.float32)).to(dev)
        stream.synchronize()
        res = {"items": len(items), "n_nodes": n_nodes}
        for set_name, (planes, boxes) in region_sets(items).items():
            n = len(planes)
            with torch.cuda.stream(stream):
                dp = torch.from_numpy(planes).to(dev)
                db = None if boxes is None else torch.from_numpy(boxes).to(dev)
            listing = lambda J, total: on_stream(lambda: d.region_overlaps(dp, margin, sections=J, capacity=total, gaps=True, offsets=True, stream=stream))
            total = count_of(lambda: d.region_overlaps(dp, margin, capacity=0, stream=stream))
            box_total = None if db is None else count_of(lambda: d.box_overlaps(db, margin, capacity=0, stream=stream))
            legs = {"region_count": on_stream(lambda: d.region_overlaps(dp, margin, capacity=0, stream=stream)),
                    "region_list": listing(0, total) if total <= MOST else None,
                    "box_list": on_stream(lambda: d.box_overlaps(db, margin, capacity=box_total, gaps=True, offsets=True, stream=stream)) if db is not None and box_total <= MOST else None,
                    "torch_all_pairs": on_stream(lambda: torch_pass(dp, centres, radii, margin))}
            J0 = rta.region_sections(n, n_nodes)
            leg = {"regions": n, "entries": total, "box_entries": box_total, "sections": J0}
            leg.update({v: None for v in legs})
            leg.update(measure(legs))
            for v in ("region_count", "region_list"):
                for bar in ("box_list", "torch_all_pairs"):
                    if leg[v] and leg[bar]:
                        leg[v]["vs_" + bar] = round(leg[bar]["device_ms"] / leg[v]["device_ms"], 2)
            if set_name in ("frusta_1", "large", "small") and total <= MOST:
                most = 64 if set_name == "small" else n_nodes
                Js = [1 << k for k in range(0, 27) if (1 << k) <= most and n * (1 << k) <= REGION_MAX_COUNTS]
                sweep = measure({str(J): listing(J, total) for J in Js})
                leg["sweep_ms"] = {J: v["device_ms"] for J, v in sweep.items()}
                leg["sweep_best"] = int(min(sweep, key=lambda J: sweep[J]["device_ms"]))
            for label, J in (("tests_per_region", 0), ("tests_per_region_one_lane", 1)):
                st = d.region_overlaps(dp, margin, sections=J, capacity=0, stats=True, stream=stream)[-1]
                leg[label] = round(st["tests_executed"] / n, 2)
            leg["regions_with_an_entry"] = st["hits"]
            offsets = d.region_overlaps(dp, margin, capacity=0, offsets=True, stream=stream)[1]
            nz = legs["torch_all_pairs"]()
            stream.synchronize()
            leg["longest_row"] = int(np.diff(offsets.cpu().numpy()).max())
            leg["entries_vs_torch"] = total - sum(int(x.shape[0]) for x in nz)
            res[set_name] = leg
        out["scenes"][name] = res
        d.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
