"""Helpers of the per-walk-record tests (tests/test_walk_host.py, tests/test_gpu_walk.py; rust-tracer_amd/csrc/rt_tight.hpp build_walk,
NOTES.md "Per-walk bounds").  The scenes are those of tests/tight_scenes.py.

  walk_of(): capi.walk_bounds of an rta.Scene -- per bound the sphere and threshold the primary per-walk stream carries, T', the light disc
      (w1', w2', cl', R2o', R2i') and which of the two the bound has;
  fma32(), b_prime(), shadow_verdict(): the two filters as the f32 loops form them (rt_skip.hpp primary_filter_pass, shadow_filter_origin,
      shadow_p2<true>, shadow_filter_verdict), restated in numpy with a correctly rounded f32 fma;
  check_scene(): the claims asked of the REFERENCE's f32 sphere test on rays that graze the items -- whenever an item's distance is finite,
      b' >= T' of every enclosing bound with an eye sphere, and the filter's verdict on every enclosing light disc is not MISS;
  disc_rim_rays(): shadow-type rays that pass an item where its disc touches its bound's light disc, one origin coordinate tuned to the
      ulp where the reference's verdict on the item flips;
  frames(): the GPU side -- a frame over the tight streams with RT_DEBUG_WALK_BOUNDS 0 and 2 against the oracle's, the launch flag, the
      counting launch."""
import numpy as np

from tests import tight_scenes as ts

EYE_SPHERE, LIGHT_DISC = 1, 2
F32 = np.float32


def walk_of(scene, slack=True):
    from rust_tracer_amd import capi
    return capi.walk_bounds(scene.items, scene.directional_light, scene.eye, scene.bounds, [tuple(r) for r in scene.ranges], slack=slack)


def flags_of(records):
    return records[:, 11].astype(np.int64)


def fma32(a, b, c):
    """fl32(a * b + c) for f32 a, b, c, rounded once: the product is exact in float64, the sum is rounded to odd there (two-sum), and 53
    bits rounded to odd round to 24 bits as the exact value does."""
    p = float(F32(a)) * float(F32(b))
    c = float(F32(c))
    s = p + c
    if np.isfinite(s):
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        if e != 0.0 and (np.float64(s).view(np.uint64) & np.uint64(1)) == 0:
            s = float(np.nextafter(s, np.inf if e > 0.0 else -np.inf))
    return F32(s)


def b_prime(sphere, eye, d):
    """fma(vz, dz, fma(vy, dy, vx * dx)) with v = fl(c - eye): the loops' fused chain (rt_skip.hpp primary_filter_pass)."""
    v = np.asarray(sphere[:3], dtype=F32) - np.asarray(eye, dtype=F32)
    d = np.asarray(d, dtype=F32)
    return fma32(v[2], d[2], fma32(v[1], d[1], F32(v[0] * d[0])))


def shadow_verdict(rec, fr, origin):
    """rt_skip.hpp shadow_filter_origin + shadow_filter_verdict<true> on a light disc: 0 MISS, 1 cannot tell, 2 HIT; and P2 as the one-ray
    loops form it."""
    o = np.asarray(origin, dtype=F32)
    x, y, z = (o - fr["m0"]).astype(F32)
    e1, e2, l = fr["e1"], fr["e2"], fr["l"]
    q1 = fma32(z, e1[2], fma32(y, e1[1], F32(x * e1[0])))
    q2 = fma32(z, e2[2], fma32(y, e2[1], F32(x * e2[0])))
    ol = fma32(z, l[2], fma32(y, l[1], F32(x * l[0])))
    d2 = fma32(z, z, fma32(y, y, F32(x * x)))
    if not d2 <= fr["ro2"]:
        q1 = F32(np.nan)
    w1, w2, cl, r2o, r2i = (F32(v) for v in rec[6:11])
    t0, t1 = F32(w1 - q1), F32(w2 - q2)
    p2 = F32(F32(t0 * t0) + F32(t1 * t1))
    if p2 > abs(r2o):
        return 0, p2
    av = F32(cl - ol)
    inn = fma32(av, av, p2)
    if fma32(inn, fr["k1"], p2) <= r2i and (fr["a0"] <= av or inn <= r2i):
        return 2, p2
    return (0 if (av <= -fr["a0"] and abs(r2o) <= F32(fr["kc"] * inn)) else 1), p2


class Tally:
    def __init__(self):
        self.rays = self.hits = self.primary_asked = self.shadow_asked = 0
        self.cone, self.disc = [], []          # violations: (bound, item, ray, value, limit)

    @property
    def violations(self):
        return self.cone + self.disc


def enclosing(scene, i):
    """Indices of the bounds whose subtree holds item i."""
    return [b for b, (first, count) in enumerate(scene.ranges) if first <= i < first + count]


def ask(tally, scene, records, fr, i, rays, primary):
    """Every ray on item i: where the reference's f32 distance is finite, every enclosing bound's record must let the ray through."""
    import oracle
    fl = flags_of(records)
    item = np.asarray(scene.items[i], dtype=np.float64)
    for ray in rays:
        tally.rays += 1
        if not np.isfinite(oracle.sphere_distance_from_ray(item, ray, oracle.F32)):
            continue
        tally.hits += 1
        for b in enclosing(scene, i):
            if primary and fl[b] & EYE_SPHERE:
                tally.primary_asked += 1
                bp = b_prime(records[b, :4], scene.eye, ray[3:])
                if not bp >= records[b, 4]:
                    tally.cone.append((b, i, tuple(ray), float(bp), float(records[b, 4])))
            if not primary and fl[b] & LIGHT_DISC:
                tally.shadow_asked += 1
                verdict, p2 = shadow_verdict(records[b], fr, ray[:3])
                if verdict == 0:
                    tally.disc.append((b, i, tuple(ray), float(p2), float(records[b, 9])))


def check_scene(scene, slack=True, records=None, fr=None):
    """The grazing rays of tests/tight_scenes.py (impact parameters (1 +- 1e-6, 1 +- 3e-6, 1 - 1e-3, 0.8) r, four azimuths) from the eye and
    along the light from another item's surface, for every bound with a record and every item of its subtree.  -> Tally"""
    if records is None:
        records, fr = walk_of(scene, slack)
    fl = flags_of(records)
    items = np.asarray(scene.items, dtype=np.float64)
    eye = np.asarray(scene.eye, dtype=np.float64)
    to_light = -np.asarray(scene.directional_light, dtype=np.float32).astype(np.float64)
    tally = Tally()
    done = set()
    for b in np.nonzero(fl)[0]:
        first, count = (int(v) for v in scene.ranges[b])
        for i in range(first, first + count):
            if i in done:               # (ask() looks at every enclosing bound of the item at once)
                continue
            done.add(i)
            away = items[i, :3] - records[b, :3].astype(np.float64)
            ask(tally, scene, records, fr, i, ts.primary_rays(eye, items[i], away), True)
            ask(tally, scene, records, fr, i, ts.shadow_rays(items, i, away, to_light), False)
    return tally


def _verdict_flips(item, o, l, axis):
    """Tunes coordinate `axis` of the f32 origin o of a ray along l so that the reference's verdict on `item` flips between two adjacent f32
    values; -> (origin where it is finite, origin where it is not) or None."""
    import oracle
    finite = lambda p: bool(np.isfinite(oracle.sphere_distance_from_ray(item, np.concatenate([p.astype(np.float64), l]), oracle.F32)))
    c = np.asarray(item[:3], dtype=np.float64)
    lu = l / np.linalg.norm(l)
    rel = o.astype(np.float64) - c
    perp = rel - (rel @ lu) * lu
    lo, hi = o.copy(), o.copy()
    lo[axis] = F32(o[axis] - 0.5 * perp[axis])          # towards the centre: inside the silhouette
    hi[axis] = F32(o[axis] + 0.5 * perp[axis])          # away from it: outside
    if not finite(lo) or finite(hi):
        return None
    while True:
        mid = lo.copy()
        mid[axis] = F32(0.5 * (float(lo[axis]) + float(hi[axis])))
        if mid[axis] == lo[axis] or mid[axis] == hi[axis]:
            return lo, hi
        if finite(mid):
            lo = mid
        else:
            hi = mid


def disc_rim_rays(scene, records, fr):
    """For every bound with a light disc: the item whose disc reaches furthest from the disc's centre, and a ray along the light that passes
    that item at its silhouette on the far side, from `back` radii behind it -- tuned to the ulp.  -> [(bound, item, hit ray, miss ray)]"""
    fl = flags_of(records)
    items = np.asarray(scene.items, dtype=np.float64)
    l = -np.asarray(scene.directional_light, dtype=np.float32).astype(np.float64)
    lu = l / np.linalg.norm(l)
    e1, e2, m0 = (fr[k].astype(np.float64) for k in ("e1", "e2", "m0"))
    out = []
    for b in np.nonzero(fl & LIGHT_DISC)[0]:
        first, count = (int(v) for v in scene.ranges[b])
        sub = items[first:first + count]
        w = np.stack([(sub[:, :3] - m0) @ e1, (sub[:, :3] - m0) @ e2], axis=1) - records[b, 6:8].astype(np.float64)
        reach = np.linalg.norm(w, axis=1) + sub[:, 3]
        k = int(np.argmax(reach))
        n = np.linalg.norm(w[k])
        if not n > 1e-3 * sub[k, 3]:
            continue
        out_dir = (w[k, 0] * e1 + w[k, 1] * e2) / n                      # in the plane across the light, from the disc's centre outwards
        out_dir = out_dir - (out_dir @ lu) * lu
        out_dir /= np.linalg.norm(out_dir)
        for back in (3.0, 40.0):
            o = (sub[k, :3] + sub[k, 3] * out_dir - back * sub[k, 3] * lu).astype(F32)
            axis = int(np.argmax(np.abs(out_dir)))
            pair = _verdict_flips(sub[k], o, l, axis)
            if pair is not None:
                out.append((int(b), first + k, np.concatenate([pair[0].astype(np.float64), l]), np.concatenate([pair[1].astype(np.float64), l])))
    return out


# ---- the GPU side ----------------------------------------------------------------------------------------------------------------------

WALKS = ("generic", "lean", "lean_coop")          # the generic filtered kernel, k_render_skip_fast, k_render_skip_fast_coop


def frames(d, ref, opts, regs, expect_walk, controls=(), count=True):
    """Renders `regs` on DeviceScene d over the tight streams (RT_DEBUG_TIGHT_BOUNDS 2) with the per-walk filter streams off and on
    (RT_DEBUG_WALK_BOUNDS 0 and 2) under `controls`: both equal the oracle's frame where a tile covers it; the launch says `walk_bounds`
    exactly for 2 where the scene has a record.  count: the counting launch behind them, which holds every ITEM test against the records.
    -> launches that read the per-walk streams."""
    import rust_tracer_amd as rta
    from rust_tracer_amd import capi
    from tests import util
    covered = np.zeros(ref.shape[:2], dtype=bool)
    for (l, t, r, b) in regs:
        covered[b:t, l:r] = True
    walked = 0
    for wb in (0, 2):
        with capi.debug(capi.DEBUG_TIGHT_BOUNDS, 2), capi.debug(capi.DEBUG_WALK_BOUNDS, wb):
            for key, value in controls:
                capi.debug_set(key, value)
            try:
                data, st = d.render_tiles(opts, regs, rta.RT_TRAVERSAL_SKIP, want_stats=False)
                flags = capi.last_launch()
            finally:
                for key, _ in controls:
                    capi.debug_set(key, -1)
        frame = util.stitch(opts, regs, data)
        np.testing.assert_array_equal(frame[covered], ref[covered], err_msg="RT_DEBUG_WALK_BOUNDS %d" % wb)
        assert ("walk_bounds" in flags) == (wb == 2 and expect_walk), (wb, flags)
        assert "walk_bounds" not in flags or "tight_bounds" in flags, flags
        walked += "walk_bounds" in flags
    if count:
        before = capi.debug_count(capi.DEBUG_COUNT_FILTER_VIOLATIONS)
        data, st = d.render_tiles(opts, regs, rta.RT_TRAVERSAL_SKIP, want_stats=True)
        np.testing.assert_array_equal(util.stitch(opts, regs, data)[covered], ref[covered])
        assert capi.debug_count(capi.DEBUG_COUNT_TIGHT_VIOLATIONS) == 0
        assert capi.debug_count(capi.DEBUG_COUNT_FILTER_VIOLATIONS) == before
    return walked
