#!/usr/bin/env python3
"""Rates of the first contacts rt_first_contacts_device on torch tensors, timed with device events after warm-up: the
earliest contact of each of a second set of moving spheres with the scene during one step.  The scenes, the queries and the three
families of motion are tools/swept_rate.py's, row for row (its inputs(): as many queries as the scene has items, `slow`,
`one_percent_fast`, `standing_scene`; default scene at L8 and L9, 100,000 arbitrary spheres after DeviceScene.rebuild; f32).

  first_nearest      rt_first_contacts_device, RT_SWEEP_NEAREST: time, item and normal of the earliest contact
  first_any          the same, RT_SWEEP_ANY: some contact of the step

The bar, measured in the same run on the same device, is what a caller had before this entry:

  swept_then_min     rt_swept_overlaps_device with its capacity known (items, times, normals and offsets: both walks, the whole list),
                     followed by a torch per-row minimum: scatter_reduce amin of the times over the rows, the first entry of each row that
                     equals it, and a gather of its item and normal

Every leg is warmed up for 0.2 s, then timed in interleaved rounds (median and minimum over the rounds).  Tests per query of the
first-contact walks and of the list's counting walk come from one counting call each.  `differ` counts the queries whose NEAREST result
is not their row's (smallest time, lowest slot), in time bits or in item: the result is the walk's, and a bound whose time lies within
rounding of an item's below it can hide that item from the shrinking window, so this is reported, not required to be 0.  `not_in_row`
counts what no rounding explains -- a NEAREST or ANY result that is no entry of its row, a result beside an empty row, no result beside
an entry (until a walk has found something it makes the list's own decisions) -- and ends the tool with an error after the JSON is
written.

usage: first_contact_rate.py [--rounds R] [--out PATH]      prints one JSON line and writes it to PATH (default
profiles/f01_first_contact_rate.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
from impacts_rate import WARM_S, timed, warm  # noqa: E402
from swept_rate import inputs  # noqa: E402


def row_minimum(items, time, normal, off, n, total):
    """(time[n], item[n], normal[n, 3]) of every row's smallest time at its lowest slot (+inf, -1, 0 for an empty row), on the device."""
    dev = time.device
    if total == 0:
        return (torch.full((n,), float("inf"), dtype=time.dtype, device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev),
                torch.zeros((n, 3), dtype=time.dtype, device=dev))
    rows = torch.repeat_interleave(torch.arange(n, device=dev), off[1:] - off[:-1], output_size=total)
    best = torch.full((n,), float("inf"), dtype=time.dtype, device=dev).scatter_reduce(0, rows, time, "amin")
    at = torch.arange(total, device=dev)
    first = torch.full((n,), total, dtype=torch.int64, device=dev).scatter_reduce(0, rows, torch.where(time == best[rows], at, total), "amin")
    found = first < total
    pick = first.clamp_max(max(total - 1, 0))
    item = torch.where(found, items[pick], -1)
    nrm = torch.where(found[:, None], normal[pick], 0.0)
    return best, item, nrm


def main():
    import rust_tracer_amd as rta
    from tests.scenes import hundred_thousand_spheres
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "f01_first_contact_rate.json")
    rounds = 3
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    if "--rounds" in args:
        i = args.index("--rounds")
        rounds = int(args[i + 1])
        del args[i:i + 2]
    if rta.device_count() < 1:
        raise SystemExit("first_contact_rate.py: no gfx950 device visible; nothing is measured without one")
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
    out = {"workload": "rt_first_contacts_device, f32, torch tensors, as many queries as items (tools/swept_rate.py's inputs); bar: rt_swept_overlaps_device "
                       "with its capacity known + a torch per-row minimum",
           "rounds": rounds, "warm_s": WARM_S, "scenes": {}}
    wrong_total = 0
    for name, make in scenes:
        d, items = make()
        items = np.ascontiguousarray(items, dtype=np.float32)
        n = len(items)
        queries_np, fams, r_med, ext = inputs(items)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        with torch.cuda.stream(stream):
            queries = up(queries_np)
        stream.synchronize()
        res = {"items": n, "queries": n, "median_radius": r_med, "extent": ext}
        for label, (qdisp_np, disp_np) in fams.items():
            print("first_contact_rate.py: %s, %s" % (name, label), file=sys.stderr, flush=True)
            with torch.cuda.stream(stream):
                qdisp = up(qdisp_np)
                disp = None if disp_np is None else up(disp_np)
            total = d.swept_overlaps(queries, qdisp, disp, capacity=0, stream=stream)[1]
            stream.synchronize()                                     # (the count belongs to `stream`)
            total = int(total.item())
            listing = dict(times=True, normals=True, offsets=True, stream=stream)

            def swept_then_min():
                it, tm, nm, off, _ = d.swept_overlaps(queries, qdisp, disp, capacity=total, **listing)
                return row_minimum(it, tm, nm, off, n, total)

            def on_stream(fn):
                def run():
                    with torch.cuda.stream(stream):
                        return fn()
                return run
            legs = {"first_nearest": on_stream(lambda: d.first_contacts(queries, qdisp, disp, normals=True, stream=stream)),
                    "first_any": on_stream(lambda: d.first_contacts(queries, qdisp, disp, any_hit=True, normals=True, stream=stream)),
                    "swept_then_min": on_stream(swept_then_min)}
            iters = {v: warm(fn, stream) for v, fn in legs.items()}
            times = {v: [] for v in legs}
            for _ in range(rounds):
                for v, fn in legs.items():
                    times[v].append(timed(fn, stream, iters[v]))
            leg = {"entries": total}
            for v in legs:
                med, best = float(np.median(times[v])), min(times[v])
                leg[v] = {"device_ms": round(med, 4), "device_ms_min": round(best, 4), "calls_per_sample": iters[v]}
            for v in ("first_nearest", "first_any"):
                leg[v]["vs_swept_then_min"] = round(leg["swept_then_min"]["device_ms"] / leg[v]["device_ms"], 2)
            st = d.first_contacts(queries, qdisp, disp, stats=True, stream=stream)[-1]
            leg["first_nearest"]["tests_per_query"] = round(st["tests_executed"] / n, 2)
            leg["queries_with_a_result"] = st["hits"]
            st = d.first_contacts(queries, qdisp, disp, any_hit=True, stats=True, stream=stream)[-1]
            leg["first_any"]["tests_per_query"] = round(st["tests_executed"] / n, 2)
            st = d.swept_overlaps(queries, qdisp, disp, capacity=0, stats=True, stream=stream)[-1]
            leg["swept_then_min"]["tests_per_query_of_the_count_walk"] = round(st["tests_executed"] / n, 2)
            # every query's result against its row
            with torch.cuda.stream(stream):
                time, item, _ = legs["first_nearest"]()
                a_time, a_item, _ = legs["first_any"]()
                ref_t, ref_i, _ = swept_then_min()
                differ = (time.view(torch.int32) != ref_t.view(torch.int32)) | (item != ref_i)
                it, tm, _, off, _ = d.swept_overlaps(queries, qdisp, disp, capacity=total, **listing)
                rows = torch.repeat_interleave(torch.arange(n, device=dev), off[1:] - off[:-1], output_size=total)
                empty = (off[1:] - off[:-1]) == 0
                wrong = 0
                for r_time, r_item in ((time, item), (a_time, a_item)):
                    member = torch.zeros(n, dtype=torch.bool, device=dev)
                    member[rows[(it == r_item[rows]) & (tm.view(torch.int32) == r_time.view(torch.int32)[rows])]] = True
                    wrong += int(torch.where(empty, r_item >= 0, ~member).sum())
                leg["differ"], leg["not_in_row"] = int(differ.sum()), wrong
            stream.synchronize()
            wrong_total += wrong
            res[label] = leg
        out["scenes"][name] = res
        d.close()
    out["wrong_total"] = wrong_total
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    if wrong_total:
        raise SystemExit("first_contact_rate.py: %d results that are no entry of their query's row, or rows with an entry and no result" % wrong_total)


if __name__ == "__main__":
    main()
