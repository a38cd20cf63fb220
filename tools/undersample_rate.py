#!/usr/bin/env python3
"""Rates of the undersampled camera path (rt_render_camera_undersampled_device, csrc/rt_undersample.hpp), timed with device
events after warm-up, the legs of a case interleaved round by round, medians over the rounds.

Per frame (1920x1080, 4096x4096; spp 1, one full-image region), scene (default L8, the 100,000-sphere scene), precision (f32, f64) and view
(the identity camera, one look_at orbit view):
  bar_ms             rt_render_camera_device on the same frame -- the bar; bar_spread_ms = its largest minus its smallest round
  fresh_ms[s]        a fresh step-s frame, s = 8, 4, 2, 1; fresh_over_bar[s] next to 1 / s^2
  refine_ms["8>4"]   the refinement passes 8 -> 4, 4 -> 2, 2 -> 1
  chain_ms           fresh step 8 + the three passes: every sample of the frame traced once; chain_over_bar
  tests_per_ray      tests_executed / (primary + shadow rays) of the counting flavour, per fresh step and per pass, and of the bar: what the
                     wider wave patches of a coarse pass cost in traversal shows here, what the fills cost does not

usage: undersample_rate.py [iterations] [--rounds N] [--out PATH]
       prints one JSON line and writes it to PATH (default profiles/u01_undersample_rate.json)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: both bring a libamdhip64 with the same SONAME, torch's must win)
import numpy as np  # noqa: E402
import rust_tracer_amd as rta  # noqa: E402
from tests.scenes import hundred_thousand_spheres  # noqa: E402

STEPS = (8, 4, 2, 1)


def warm(fn, stream):
    # at least 3 calls and 0.2 s of them (an idle GPU's clocks take a while to ramp: the first leg of a run otherwise reads slow)
    t0 = time.perf_counter()
    k = 0
    while k < 3 or time.perf_counter() - t0 < 0.2:
        fn()
        k += 1
        if k % 8 == 0:
            stream.synchronize()
    stream.synchronize()


def once(fn, iters, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(legs, iters, rounds, stream):
    """{name: fn} -> {name: [ms of round 0, ...]}: every leg warmed, then `rounds` rounds that time each leg once, in turn."""
    for fn in legs.values():
        warm(fn, stream)
    out = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            out[k].append(once(fn, iters, stream))
    return out


def per_ray(st):
    rays = st["primary"] + st["shadow"]
    return round(st["tests_executed"] / rays, 2) if rays else 0.0


def case(d, opts, cam, iters, rounds, stream, buf):
    w, h, _ = opts
    regions = [(0, h, w, 0)]
    hs, p = stream.cuda_stream, buf.data_ptr()
    legs = {"bar": lambda: d.render_camera_device(opts, cam, regions, p, stream=hs)}
    for s in STEPS:
        legs["fresh%d" % s] = lambda s=s: d.render_camera_undersampled_device(opts, cam, regions, s, p, stream=hs)
    for s in STEPS[1:]:
        legs["%d>%d" % (2 * s, s)] = lambda s=s: d.render_camera_undersampled_device(opts, cam, regions, s, p, prev_step=2 * s, stream=hs)
    t = interleaved(legs, iters, rounds, stream)
    med = {k: statistics.median(v) for k, v in t.items()}
    chain = med["fresh8"] + sum(med["%d>%d" % (2 * s, s)] for s in STEPS[1:])
    r = {"bar_ms": round(med["bar"], 4), "bar_spread_ms": round(max(t["bar"]) - min(t["bar"]), 4),
         "fresh_ms": {str(s): round(med["fresh%d" % s], 4) for s in STEPS},
         "fresh_over_bar": {str(s): round(med["fresh%d" % s] / med["bar"], 4) for s in STEPS},
         "one_over_s2": {str(s): round(1.0 / (s * s), 4) for s in STEPS},
         "refine_ms": {"%d>%d" % (2 * s, s): round(med["%d>%d" % (2 * s, s)], 4) for s in STEPS[1:]},
         "chain_ms": round(chain, 4), "chain_over_bar": round(chain / med["bar"], 4)}
    # the counting flavour: tests per traced ray, per step (a fresh buffer first, so that each pass refines the frame it expects)
    tests = {"bar": per_ray(d.render_camera_device(opts, cam, regions, p, stream=hs, want_stats=True))}
    for s in STEPS:
        tests["fresh%d" % s] = per_ray(d.render_camera_undersampled_device(opts, cam, regions, s, p, stream=hs, want_stats=True))
    d.render_camera_undersampled_device(opts, cam, regions, 8, p, stream=hs, want_stats=True)
    for s in STEPS[1:]:
        tests["%d>%d" % (2 * s, s)] = per_ray(d.render_camera_undersampled_device(opts, cam, regions, s, p, prev_step=2 * s, stream=hs, want_stats=True))
    r["tests_per_ray"] = tests
    return r


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "u01_undersample_rate.json")
    rounds = 5
    for flag in ("--out", "--rounds"):
        if flag in args:
            k = args.index(flag)
            if flag == "--out":
                out_path = args[k + 1]
            else:
                rounds = int(args[k + 1])
            del args[k:k + 2]
    iters = int(args[0]) if args else 10
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    buf = torch.empty(4096 * 4096 * 4, dtype=torch.uint8, device=dev)
    info = rta.capi.build_info()
    out = {"workload": "rt_render_camera_undersampled_device: fresh step-s frames and refinement passes against rt_render_camera_device, spp 1, one region",
           "iterations": iters, "rounds": rounds, "kernel_src_sha": info.split("kernel sources ")[-1].split()[0] if "kernel sources " in info else "",
           "cases": {}}
    for prec, pname in ((rta.RT_F32, "f32"), (rta.RT_F64, "f64")):
        R = np.float32 if prec == rta.RT_F32 else np.float64
        for name, make in (("default_L8", lambda: rta.Scene.default(8, prec)),
                           ("100k", lambda: rta.Scene.from_spheres_auto(hundred_thousand_spheres(), precision=prec))):
            s = make()
            d = s.device()
            ident = np.concatenate([s.eye, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=R)]).astype(R)
            orbit = rta.look_at((3.5, 2.0, -3.0), (0.0, -0.3, 0.0), hfov_deg=60.0, precision=prec)
            for w, h in ((1920, 1080), (4096, 4096)):
                for view, cam in (("identity", ident), ("orbit", orbit)):
                    out["cases"]["%s_%s_%dx%d_%s" % (name, pname, w, h, view)] = case(d, (w, h, 1), cam, iters, rounds, stream, buf)
            d.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
