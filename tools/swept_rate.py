#!/usr/bin/env python3
"""Rates of the swept overlap lists rt_swept_overlaps_device on torch tensors, timed with device events after warm-up: every
sphere of the scene that each of a second set of moving spheres comes into contact with during one step.  The queries are as many as
the scene has items: its own spheres, each moved off its place by two median radii in a random direction (a second set of bodies in
among the first).  Three families of motion --

  slow               every query and every item moves one median item radius in a random direction
  one_percent_fast   the same, but 1 % of the queries and 1 % of the items move one scene extent
  standing_scene     the queries move as in `slow`, the scene stands still (disp = NULL)

  swept_count        capacity 0: the queries' magnitude, the motion table, the counting walk and the scan -- "how many"
  swept_list         capacity = the total, times, normals and offsets too: both walks, the whole list

The bars, measured in the same run on the same device, are what a caller had before this entry:

  overlaps_then_toi  rt_overlap_spheres_device at margin max|dq| + max|d| -- the skin that no query and item can cross in one step -- with
                     its capacity known, followed by a torch narrow phase over its entries: the time of impact of every candidate, then
                     t <= 1.  One fast body makes the skin the scene's own size; where the candidates exceed MAX_CANDIDATES (or the
                     2^31 - 1 entries one call can list) the leg is not run and the JSON says how many candidates there were
  torch_all_pairs    the time of impact of every query against every item in chunks of CHUNK rows, then t <= 1, then nonzero

on the default scene at L8 and L9 (static scenes) and on the 100,000 arbitrary spheres after DeviceScene.rebuild (a dynamic scene), f32.
Every leg is warmed up for 0.2 s, then timed in interleaved rounds (median and minimum over the rounds); tests per query come from one
counting call.  The tool checks that the three entry sets agree away from grazes, judged in float64 as tools/impacts_rate.py judges its
pairs: `disagree_grazing` / `disagree_clear` count the entries that one leg lists and another does not; a clear disagreement ends the tool
with an error after the JSON is written.

usage: swept_rate.py [--rounds R] [--out PATH]      prints one JSON line and writes it to PATH (default profiles/s01_swept_rate.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
from impacts_rate import CHUNK, MAX_CANDIDATES, WARM_S, timed, toi, warm  # noqa: E402


def torch_all_pairs(q, items, chunk=CHUNK):
    """The all-pairs bar: per chunk of queries the time of impact against every item, t <= 1, nonzero -> int64 keys g * m + item."""
    (qc, qr, qd), (c, r, d) = q, items
    m = c.shape[0]
    out = []
    for a in range(0, qc.shape[0], chunk):
        t = toi(qc[a:a + chunk, None, :], qr[a:a + chunk, None], qd[a:a + chunk, None, :], c[None], r[None], d[None])
        hit = (t <= 1).nonzero()
        out.append((hit[:, 0] + a) * m + hit[:, 1])
    return torch.cat(out)


def narrow_phase(rows, cand, m_entries, q, items):
    """The time of impact of the first m_entries candidates (query rows[e], item cand[e]), then t <= 1 -> int64 keys."""
    (qc, qr, qd), (c, r, d) = q, items
    g, j = rows[:m_entries], cand[:m_entries].long()
    t = toi(qc[g], qr[g], qd[g], c[j], r[j], d[j])
    keep = t <= 1
    return g[keep] * c.shape[0] + j[keep]


def disagreements(keys_a, keys_b, q, items):
    """(grazing, clear): the entries in exactly one of the two key sets, judged in float64."""
    both = torch.cat([torch.unique(keys_a), torch.unique(keys_b)])
    k, cnt = torch.unique(both, return_counts=True)
    odd = k[cnt == 1]
    if odd.numel() == 0:
        return 0, 0
    (qc, qr, qd), (c, r, d) = q, items
    m = c.shape[0]
    g, j = odd // m, odd % m
    v, w = c[j].double() - qc[g].double(), qd[g].double() - d[j].double()
    rad = r[j].double() + qr[g].double()
    a, b, vv = (w * w).sum(-1), (v * w).sum(-1), (v * v).sum(-1)
    cc = vv - rad * rad
    disc = b * b - a * cc
    t = cc / (b + torch.sqrt(disc.abs()))
    eps = 1e-5
    graze = (cc.abs() <= eps * (vv + rad * rad)) | ((cc > 0) & (b > 0) & (((t - 1).abs() <= eps) | (disc.abs() <= eps * (b * b + a * cc.abs()))))
    return int(graze.sum()), int((~graze).sum())


def inputs(items, seed=100):
    """(queries float32[n, 4], {family: (qdisp float32[n, 3], disp float32[n, 3] or None)}, median radius, extent)."""
    rng = np.random.default_rng(seed)
    n = len(items)

    def unit():
        u = rng.normal(size=(n, 3))
        return u / np.linalg.norm(u, axis=1, keepdims=True)
    r_med = float(np.median(items[:, 3]))
    ext = float(((items[:, :3] + items[:, 3:]).max(axis=0) - (items[:, :3] - items[:, 3:]).min(axis=0)).max())
    queries = items.astype(np.float64).copy()
    queries[:, :3] += 2.0 * r_med * unit()
    uq, ud = unit(), unit()
    slow_q, slow_d = uq * r_med, ud * r_med
    fast_q, fast_d = slow_q.copy(), slow_d.copy()
    pq, pd = rng.random(n) < 0.01, rng.random(n) < 0.01
    fast_q[pq], fast_d[pd] = uq[pq] * ext, ud[pd] * ext
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    fams = {"slow": (f32(slow_q), f32(slow_d)), "one_percent_fast": (f32(fast_q), f32(fast_d)), "standing_scene": (f32(slow_q), None)}
    return f32(queries), fams, r_med, ext


def main():
    import rust_tracer_amd as rta
    from tests.scenes import hundred_thousand_spheres
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "s01_swept_rate.json")
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
        raise SystemExit("swept_rate.py: no gfx950 device visible; nothing is measured without one")
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
    out = {"workload": "rt_swept_overlaps_device, f32, torch tensors, as many queries as items; bars: rt_overlap_spheres_device at margin max|dq| + max|d| + a torch "
                       "narrow phase, torch all-pairs",
           "rounds": rounds, "warm_s": WARM_S, "chunk": CHUNK, "max_candidates": MAX_CANDIDATES, "scenes": {}}
    clear_total = 0
    for name, make in scenes:
        d, items = make()
        items = np.ascontiguousarray(items, dtype=np.float32)
        n = len(items)
        queries_np, fams, r_med, ext = inputs(items)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        with torch.cuda.stream(stream):
            centres, radii, queries = up(items[:, :3]), up(items[:, 3]), up(queries_np)
            qc, qr = queries[:, :3].contiguous(), queries[:, 3].contiguous()
            zero = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        stream.synchronize()
        res = {"items": n, "queries": n, "median_radius": r_med, "extent": ext}
        for label, (qdisp_np, disp_np) in fams.items():
            print("swept_rate.py: %s, %s" % (name, label), file=sys.stderr, flush=True)
            with torch.cuda.stream(stream):
                qdisp = up(qdisp_np)
                disp = None if disp_np is None else up(disp_np)
            q, it = (qc, qr, qdisp), (centres, radii, zero if disp is None else disp)
            total = d.swept_overlaps(queries, qdisp, disp, capacity=0, stream=stream)[1]
            stream.synchronize()                                     # (the count belongs to `stream`)
            total = int(total.item())
            longest = lambda a: 0.0 if a is None else float(np.sqrt((a.astype(np.float64) ** 2).sum(axis=1)).max())
            margin = longest(qdisp_np) + longest(disp_np)
            candidates = d.overlaps(queries, margin, capacity=0, stream=stream)[1]
            stream.synchronize()
            candidates = int(candidates.item())
            feasible = candidates <= MAX_CANDIDATES

            def on_stream(fn):
                def run():
                    with torch.cuda.stream(stream):
                        return fn()
                return run

            def broad_then_narrow():
                cand, off, _ = d.overlaps(queries, margin, capacity=candidates, offsets=True, stream=stream)
                rows = torch.repeat_interleave(torch.arange(n, device=dev), off[1:] - off[:-1], output_size=candidates)
                return narrow_phase(rows, cand, candidates, q, it)
            listing = dict(times=True, normals=True, offsets=True, stream=stream)
            legs = {"swept_count": on_stream(lambda: d.swept_overlaps(queries, qdisp, disp, capacity=0, stream=stream)),
                    "swept_list": on_stream(lambda: d.swept_overlaps(queries, qdisp, disp, capacity=total, **listing) if total
                                            else d.swept_overlaps(queries, qdisp, disp, capacity=0, stream=stream)),
                    "torch_all_pairs": on_stream(lambda: torch_all_pairs(q, it))}
            if feasible:
                legs["overlaps_then_toi"] = on_stream(broad_then_narrow)
            iters = {v: warm(fn, stream) for v, fn in legs.items()}
            times = {v: [] for v in legs}
            for _ in range(rounds):
                for v, fn in legs.items():
                    times[v].append(timed(fn, stream, iters[v]))
            leg = {"entries": total, "skin_margin": margin, "skin_candidates": candidates}
            for v in legs:
                med, best = float(np.median(times[v])), min(times[v])
                leg[v] = {"device_ms": round(med, 4), "device_ms_min": round(best, 4), "calls_per_sample": iters[v]}
            if not feasible:
                leg["overlaps_then_toi"] = {"not_run": "%d candidate entries at margin max|dq| + max|d|, more than %d" % (candidates, MAX_CANDIDATES)}
            for v in ("swept_count", "swept_list"):
                for bar in ("overlaps_then_toi", "torch_all_pairs"):
                    if bar in legs:
                        leg[v]["vs_" + bar] = round(leg[bar]["device_ms"] / leg[v]["device_ms"], 2)
            st = d.swept_overlaps(queries, qdisp, disp, capacity=0, stats=True, stream=stream)[-1]
            leg["tests_per_query"] = round(st["tests_executed"] / n, 2)
            leg["queries_with_an_entry"] = st["hits"]
            if total:
                mine_items, off, _ = d.swept_overlaps(queries, qdisp, disp, capacity=total, offsets=True, stream=stream)
                with torch.cuda.stream(stream):
                    rows = torch.repeat_interleave(torch.arange(n, device=dev), off[1:] - off[:-1], output_size=total)
                    mine = rows * n + mine_items.long()
            else:
                mine = torch.zeros(0, dtype=torch.int64, device=dev)
            theirs = {"torch_all_pairs": legs["torch_all_pairs"]()}
            if feasible:
                theirs["overlaps_then_toi"] = legs["overlaps_then_toi"]()
            with torch.cuda.stream(stream):
                for bar, keys in theirs.items():
                    grazing, clear = disagreements(mine, keys, q, it)
                    leg[bar].update(entries=int(keys.numel()), disagree_grazing=grazing, disagree_clear=clear)
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
        raise SystemExit("swept_rate.py: %d entries away from every graze are listed by one leg and not by another" % clear_total)


if __name__ == "__main__":
    main()
