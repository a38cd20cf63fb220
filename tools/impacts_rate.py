#!/usr/bin/env python3
"""Rates of the impact-pair query rt_scene_impacts_device on torch tensors, timed with device events after warm-up: every
pair of spheres of the scene that comes into contact during one step, for two families of displacements --

  median_radius      every sphere moves one median item radius in a random direction
  one_percent_fast   the same, but 1 % of the spheres move one scene extent (the largest extent of the spheres along an axis)

  impacts_count      capacity 0: the motion table, the counting walk and the scan -- "how many"
  impacts_list       capacity = the total, times and offsets too: the motion table, both walks and the scan, the whole list

The bars, measured in the same run on the same device, are what a caller had before this entry:

  contacts_then_toi  rt_scene_contacts_device at margin 2 max|d| -- the skin that no pair can cross in one step -- with its capacity known,
                     followed by a torch narrow phase over its pairs: the time of impact of every candidate, then t <= 1.  One fast
                     sphere makes the skin the scene's own size; where the candidates exceed MAX_CANDIDATES (or the 2^31 - 1 pairs one
                     call can list) the leg is not run and the JSON says how many candidates there were
  torch_all_pairs    the time of impact of all j > i in chunks of CHUNK rows, then t <= 1, then nonzero

on the default scene at L8 and L9 (static scenes) and on the 100,000 arbitrary spheres after DeviceScene.rebuild (a dynamic scene), f32.
Every leg is warmed up for 0.2 s, then timed in interleaved rounds (median and minimum over the rounds); tests per item come from one
counting call.  The tool checks that the three pair sets agree away from grazes: a pair that one leg lists and another does not must have,
in float64, |c| <= 1e-5 (vv + RR), or c > 0, b > 0 and |t - 1| <= 1e-5 or |disc| <= 1e-5 (b*b + a |c|) (torch contracts to FMA, and the
contacts leg's skin has roundings of its own).  `disagree_grazing` / `disagree_clear` count them; a clear disagreement ends the tool with
an error after the JSON is written.

usage: impacts_rate.py [--rounds R] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/i01_impacts_rate.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402

WARM_S, SAMPLE_S, CHUNK, MAX_CANDIDATES = 0.2, 0.05, 1024, 200_000_000


def toi(ci, ri, di, cj, rj, dj):
    """The time of impact of sphere records (c, r, d) i against j, broadcast; the definition's formula in the tensors' dtype."""
    v, w = cj - ci, di - dj
    rad = rj + ri
    a, b = (w * w).sum(-1), (v * w).sum(-1)
    c = (v * v).sum(-1) - rad * rad
    disc = b * b - a * c
    inf = torch.full_like(c, float("inf"))
    t = torch.where((b > 0) & ~(disc < 0), c / (b + torch.sqrt(disc.clamp_min(0))), inf)
    t = torch.where(c > 0, t, torch.zeros_like(c))
    return torch.where((ri > 0) & (rj > 0), t, inf)


def torch_all_pairs(centres, radii, disp, chunk=CHUNK):
    """The all-pairs bar: per chunk of rows the time of impact against every sphere, the upper triangle, t <= 1, nonzero -> int64 keys."""
    n = centres.shape[0]
    cols = torch.arange(n, device=centres.device)
    out = []
    for a in range(0, n, chunk):
        t = toi(centres[a:a + chunk, None, :], radii[a:a + chunk, None], disp[a:a + chunk, None, :], centres[None], radii[None], disp[None])
        hit = ((t <= 1) & (cols[None, :] > cols[a:a + chunk, None])).nonzero()
        out.append((hit[:, 0] + a) * n + hit[:, 1])
    return torch.cat(out)


def narrow_phase(pairs, m, centres, radii, disp):
    """The time of impact of the first m candidate pairs, then t <= 1 -> int64 keys."""
    i, j = pairs[:m, 0].long(), pairs[:m, 1].long()
    t = toi(centres[i], radii[i], disp[i], centres[j], radii[j], disp[j])
    keep = t <= 1
    return i[keep] * centres.shape[0] + j[keep]


def disagreements(keys_a, keys_b, centres, radii, disp):
    """(grazing, clear): the pairs in exactly one of the two key sets, judged in float64."""
    both = torch.cat([torch.unique(keys_a), torch.unique(keys_b)])
    k, cnt = torch.unique(both, return_counts=True)
    odd = k[cnt == 1]
    if odd.numel() == 0:
        return 0, 0
    n = centres.shape[0]
    i, j = odd // n, odd % n
    c64, r64, d64 = centres.double(), radii.double(), disp.double()
    v, w = c64[j] - c64[i], d64[i] - d64[j]
    rad = r64[j] + r64[i]
    a, b, vv = (w * w).sum(-1), (v * w).sum(-1), (v * v).sum(-1)
    c = vv - rad * rad
    disc = b * b - a * c
    t = c / (b + torch.sqrt(disc.abs()))
    eps = 1e-5
    graze = (c.abs() <= eps * (vv + rad * rad)) | ((c > 0) & (b > 0) & (((t - 1).abs() <= eps) | (disc.abs() <= eps * (b * b + a * c.abs()))))
    return int(graze.sum()), int((~graze).sum())


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


def families(items, seed=100):
    """name -> float32[n, 3]."""
    rng = np.random.default_rng(seed)
    n = len(items)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r_med = float(np.median(items[:, 3]))
    ext = float(((items[:, :3] + items[:, 3:]).max(axis=0) - (items[:, :3] - items[:, 3:]).min(axis=0)).max())
    slow = u * r_med
    fast = slow.copy()
    pick = rng.random(n) < 0.01
    fast[pick] = u[pick] * ext
    return {"median_radius": np.ascontiguousarray(slow, dtype=np.float32), "one_percent_fast": np.ascontiguousarray(fast, dtype=np.float32)}, r_med, ext


def main():
    import rust_tracer_amd as rta
    from tests.scenes import hundred_thousand_spheres
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "i01_impacts_rate.json")
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
        raise SystemExit("impacts_rate.py: no gfx950 device visible; nothing is measured without one")
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
    out = {"workload": "rt_scene_impacts_device, f32, torch tensors; bars: rt_scene_contacts_device at margin 2 max|d| + a torch narrow phase, torch all-pairs",
           "rounds": rounds, "warm_s": WARM_S, "chunk": CHUNK, "max_candidates": MAX_CANDIDATES, "scenes": {}}
    clear_total = 0
    for name, make in scenes:
        d, items = make()
        items = np.ascontiguousarray(items, dtype=np.float32)
        n = len(items)
        fams, r_med, ext = families(items)
        with torch.cuda.stream(stream):
            centres = torch.from_numpy(np.ascontiguousarray(items[:, :3])).to(dev)
            radii = torch.from_numpy(np.ascontiguousarray(items[:, 3])).to(dev)
        stream.synchronize()
        res = {"items": n, "median_radius": r_med, "extent": ext}
        for label, disp_np in fams.items():
            print("impacts_rate.py: %s, %s" % (name, label), file=sys.stderr, flush=True)
            with torch.cuda.stream(stream):
                disp = torch.from_numpy(disp_np).to(dev)
            total = d.impacts(disp, 0, stream=stream)[1]
            stream.synchronize()                                     # (the count belongs to `stream`)
            total = int(total.item())
            margin = 2.0 * float(np.sqrt((disp_np.astype(np.float64) ** 2).sum(axis=1)).max())
            candidates = d.contacts(margin, 0, device=True, stream=stream)[1]
            stream.synchronize()
            candidates = int(candidates.item())
            feasible = candidates <= MAX_CANDIDATES

            def on_stream(fn):
                def run():
                    with torch.cuda.stream(stream):
                        return fn()
                return run

            def broad_then_narrow():
                pairs, m = d.contacts(margin, candidates, device=True, stream=stream)
                return narrow_phase(pairs, candidates, centres, radii, disp)
            legs = {"impacts_count": on_stream(lambda: d.impacts(disp, 0, stream=stream)),
                    "impacts_list": on_stream(lambda: d.impacts(disp, total, times=True, offsets=True, stream=stream) if total else d.impacts(disp, 0, stream=stream)),
                    "torch_all_pairs": on_stream(lambda: torch_all_pairs(centres, radii, disp))}
            if feasible:
                legs["contacts_then_toi"] = on_stream(broad_then_narrow)
            iters = {v: warm(fn, stream) for v, fn in legs.items()}
            times = {v: [] for v in legs}
            for _ in range(rounds):
                for v, fn in legs.items():
                    times[v].append(timed(fn, stream, iters[v]))
            leg = {"impacts": total, "skin_margin": margin, "skin_candidates": candidates}
            for v in legs:
                med, best = float(np.median(times[v])), min(times[v])
                leg[v] = {"device_ms": round(med, 4), "device_ms_min": round(best, 4), "calls_per_sample": iters[v]}
            if not feasible:
                leg["contacts_then_toi"] = {"not_run": "%d candidate pairs at margin 2 max|d|, more than %d" % (candidates, MAX_CANDIDATES)}
            for v in ("impacts_count", "impacts_list"):
                for bar in ("contacts_then_toi", "torch_all_pairs"):
                    if bar in legs:
                        leg[v]["vs_" + bar] = round(leg[bar]["device_ms"] / leg[v]["device_ms"], 2)
            st = d.impacts(disp, 0, stats=True, stream=stream)[-1]
            leg["tests_per_item"] = round(st["tests_executed"] / n, 2)
            leg["items_with_an_impact_as_lower_slot"] = st["hits"]
            if total:
                pairs = d.impacts(disp, total, stream=stream)[0]
                with torch.cuda.stream(stream):
                    mine = pairs[:, 0].long() * n + pairs[:, 1].long()
            else:
                mine = torch.zeros(0, dtype=torch.int64, device=dev)
            theirs = {"torch_all_pairs": legs["torch_all_pairs"]()}
            if feasible:
                theirs["contacts_then_toi"] = legs["contacts_then_toi"]()
            with torch.cuda.stream(stream):
                for bar, keys in theirs.items():
                    grazing, clear = disagreements(mine, keys, centres, radii, disp)
                    leg[bar].update(pairs=int(keys.numel()), disagree_grazing=grazing, disagree_clear=clear)
                    clear_total += clear
            stream.synchronize()
            res[label] = leg
        out["scenes"][name] = res
        d.close()
    out["disagree_clear_total"] = clear_total
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    if clear_total:
        raise SystemExit("impacts_rate.py: %d pairs away from every graze are listed by one leg and not by another" % clear_total)


if __name__ == "__main__":
    main()
