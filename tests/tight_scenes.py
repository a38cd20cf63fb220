"""Fixtures of the tight-stream tests (tests/test_tight_host.py, tests/test_gpu_tight.py): small f32 scenes in which single bounds must keep
the sphere they were given (rust-tracer_amd/csrc/rt_tight.hpp, rules (b) and (c)) while others of the same scene get a tight one.

For tests/test_tight_poses_host.py and tests/test_gpu_tight_poses.py, which hold the tight streams to the oracle away from the home pose:
  posed_inputs() / placed_inputs() / edge_inputs(): every f32 scene of the frame tests (tests/posed_scenes.py, tests/scaled_scenes.py,
      tests/edge_scenes.py) with the selection rule it must get;
  eye_outside(): rt_tight.hpp's "the eye is clearly outside", restated;
  Tally, primary_rays(), shadow_rays(), check_bound(): the theorem of NOTES.md T asked of the REFERENCE's f32 sphere test
      (oracle.sphere_distance_from_ray) -- (1) an item's finite distance implies its bound's, (2) from the eye the bound's is not larger --
      on rays that graze the items;
  RIM / rim_scene(): scenes whose tight balls are known in closed form, with an item on the rim and a frame pixel's ray through the
      outer tangent point, tuned to the ulp where the reference's verdict on the item flips;
  MODES / frames(): the GPU side -- a frame under RT_DEBUG_TIGHT_BOUNDS 0 and 2 against the oracle's, the launch flag, the counting launch."""
import functools

import numpy as np

LIGHT = (-1.0, -3.0, 2.0)
EYE = (0.0, 0.0, -4.0)

# rule (b): the inner bound (index 1) leaves parts of both of its items outside -- the reference culls them visibly, and only the given record
# does the same; the loose root (index 0) encloses everything and gets a tight sphere
OUTSIDE_ITEMS = [(0.0, -1.0, 0.0, 1.0), (-1.2, 0.2, 0.0, 0.5), (1.2, 0.2, 0.0, 0.5)]
OUTSIDE_BOUNDS = [(0.0, -1.0, 0.0, 3.0), (0.0, 0.2, 0.0, 1.0)]
OUTSIDE_RANGES = [(0, 3), (1, 2)]
OUTSIDE_KEEPS = [1]

# rule (c): the eye lies inside the root (index 0) and inside the bound of the second item (index 1; SURVEY.md H2: that group is culled by its
# exit distance); the loose bound of the far pair (index 2) has the eye outside and gets a tight sphere
INSIDE_ITEMS = [(0.0, 0.0, -1.7, 0.4), (0.0, 0.0, -2.0, 0.5), (1.5, 0.3, 1.0, 0.4), (2.1, 0.3, 1.0, 0.4)]
INSIDE_BOUNDS = [(0.0, 0.0, -2.0, 10.0), (0.0, 0.0, -3.7, 2.3), (1.8, 0.3, 1.0, 2.0)]
INSIDE_RANGES = [(0, 4), (1, 1), (2, 2)]
INSIDE_KEEPS = [0, 1]

FIXTURES = {"outside": (OUTSIDE_ITEMS, OUTSIDE_BOUNDS, OUTSIDE_RANGES, OUTSIDE_KEEPS),
            "inside": (INSIDE_ITEMS, INSIDE_BOUNDS, INSIDE_RANGES, INSIDE_KEEPS)}

EPS = 2.0 ** -24


def encloses_with_inflation(sphere, items, S, eta):
    """rt_tight.hpp's statement of "sphere X encloses item I with the inflation", in float64, for every item of `items`."""
    A = 13.0 * EPS + 1.02 * eta
    AS2 = A * S * S
    g = (16.0 * EPS + eta) * S
    c, r = np.asarray(sphere[:3], dtype=np.float64), float(sphere[3])
    it = np.asarray(items, dtype=np.float64).reshape(-1, 4)
    D = np.sqrt(((it[:, :3] - c) ** 2).sum(axis=1))
    need = (D + np.sqrt(it[:, 3] ** 2 * (1.0 + 2.0 * EPS) + AS2) + g) ** 2
    return bool(np.all(r * r * (1.0 - 2.0 * EPS) - AS2 >= need))


# ---- the inputs the frame tests already have, and the rule each must get -------------------------------------------------------------

INSIDE_EYES = ("inside_root", "centre", "inside_item")       # tests/posed_scenes.py: the eye inside the root bound


def tight_of(scene):
    """capi.tight_bounds of an rta.Scene (host side): (spheres f32[n, 4], tight u8[n], {S, eta, volume_ratio, by_rule, rule})."""
    from rust_tracer_amd import capi
    return capi.tight_bounds(scene.items, scene.directional_light, scene.eye, scene.bounds, [tuple(r) for r in scene.ranges])


def posed_inputs():
    """[(scene, light, eye, placement)]: every distinct f32 scene of posed_scenes.CASES, in their order, and the special eyes (which CASES has
    on the concentric scene only) on the nested one: tests/test_gpu_tight_poses.py renders those too."""
    import rust_tracer_amd as rta
    from tests import posed_scenes as ps
    more = [("nested", l, e, placement) for placement in ("id", "moved") for l, e in ps.SPECIAL_POSES]
    return list(dict.fromkeys([p[:4] for p in ps.CASES if p[4] == rta.RT_F32] + more))


def posed_scene(key):
    import rust_tracer_amd as rta
    from tests import posed_scenes as ps
    return ps.case(*key, rta.RT_F32, ps.SHAPE).scene


def posed_rule(key):
    """The selection rule of a posed scene (rt_capi_scene.hpp tight_rule): the eye inside the root leaves the largest volume as it is, and
    nothing qualifies at 1e-10 (eye_outside's absolute vv >= 4e-14): 0; else the plain-stream scene walks its tight streams wherever it
    can (1), the fused one -- 34 of 40 qualify, fewer than nine in ten -- in large one-sample passes only (2)."""
    scene, _, eye, placement = key
    if eye in INSIDE_EYES or placement == "x1e-10":
        return 0
    return 2 if scene == "concentric" else 1


PLACED_TIGHT = ("x1e+06", "x5e+13", "+3e3")                   # tests/scaled_scenes.py: the f32 placements at which bounds qualify
PLACED_NONE = ("x1e-20", "x1e-10")


def placed_inputs():
    """[(placement, scene name)]: the bounded f32 cases of scaled_scenes."""
    import rust_tracer_amd as rta
    from tests import scaled_scenes as ss
    return [(pl, name) for pl in ss.placement_ids(rta.RT_F32) for name in ("nested", "concentric")]


def placed_case(key):
    import rust_tracer_amd as rta
    from tests import scaled_scenes as ss
    return next(c for c in ss.case(rta.RT_F32, key[0]) if c.name == key[1])


def placed_rule(key):
    return 0 if key[0] in PLACED_NONE else (2 if key[1] == "concentric" else 1)


EDGE_TIGHT = ("P2", "P3", "S2", "O")                           # tests/edge_scenes.py: the families with bounds that qualify
EDGE_RULE = {"P3": 1}                                          # (the others: the root holds the eye and nearly all the volume: 0)


@functools.lru_cache(maxsize=None)
def edge_pair(family, spp):
    """(EdgeScene, rta.Scene, oracle.Scene) of one f32 edge scene."""
    import oracle
    import rust_tracer_amd as rta
    from tests import edge_scenes as es
    from tests import util
    sc = es.scene(family, oracle.F32, spp)
    s, o = util.scene_pair_ranges(sc.items, sc.bounds, sc.ranges, rta.RT_F32, light=sc.light, eye=sc.eye)
    return sc, s, o


def eye_outside(sphere, eye):
    """rt_tight.hpp's eye_outside: v = fl(c - eye) in f32, vv and rr exact for it (float64); clearly outside when vv >= 4e-14 and
    vv - rr >= 128 eps (vv + rr)."""
    c, e = np.asarray(sphere[:3], dtype=np.float32), np.asarray(eye, dtype=np.float32)
    v = (c - e).astype(np.float64)
    vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    rr = float(sphere[3]) * float(sphere[3])
    return bool(vv >= 4e-14 and vv - rr >= 128.0 * EPS * (vv + rr))


def round_up(v):
    f = np.float32(v)
    return f if float(f) >= v else np.nextafter(f, np.float32(np.inf))


# ---- the theorem against the reference's arithmetic -----------------------------------------------------------------------------------

BAND = (1.0 - 3e-6, 1.0 - 1e-6, 1.0 + 1e-6, 1.0 + 3e-6)     # impact parameters rho r: a few 1e-6 either side of the silhouette ...
INSIDE = (1.0 - 1e-3, 0.8)                                   # ... and further inside
RHOS = BAND + INSIDE
AZIMUTHS = (0.0, 90.0, 180.0, 270.0)                         # degrees from the direction that points away from the bound's centre


class Tally:
    """What check_bound saw: rays (unordered: those asked (1) only), hits (the ITEM's distance finite) and misses, and the violations of (1) "finite" and (2) "order" as
    (tag, kind, item, sphere, ray, d_item, d_sphere)."""

    def __init__(self):
        self.rays = self.hits = self.misses = self.unordered = 0
        self.finite, self.order = [], []

    @property
    def violations(self):
        return self.finite + self.order

    def shares(self):
        return self.hits / max(self.rays, 1), self.misses / max(self.rays, 1)


def _perp_frame(axis, away):
    """Unit w0 across `axis` (unit) nearest to `away`, and w1 = axis x w0; any w0 where `away` has no part across the axis."""
    w0 = away - (away @ axis) * axis
    if not np.linalg.norm(w0) > 1e-9 * max(np.linalg.norm(away), 1e-300):
        k = int(np.argmin(np.abs(axis)))
        w0 = np.eye(3)[k] - axis[k] * axis
    w0 = w0 / np.linalg.norm(w0)
    return w0, np.cross(axis, w0)


def primary_rays(eye, item, away, rhos=RHOS, azimuths=AZIMUTHS):
    """Rays from `eye` past `item` at impact parameters rho r, at `azimuths` around the eye-item axis counted from the side that `away`
    (a vector; the item's centre minus its bound's) points to.  Directions are made in float64, rounded to f32 and normalised by the
    reference's vec_normalized in f32, as a primary ray's is.  float64[n, 6] of f32 values; none where the eye is inside rho r."""
    import oracle
    e = np.asarray(eye, dtype=np.float64)
    c, r = np.asarray(item[:3], dtype=np.float64), float(item[3])
    v = c - e
    L = float(np.linalg.norm(v))
    if not L > 0.0:
        return np.zeros((0, 6))
    u = v / L
    w0, w1 = _perp_frame(u, np.asarray(away, dtype=np.float64))
    out = []
    for az in azimuths:
        w = np.cos(np.radians(az)) * w0 + np.sin(np.radians(az)) * w1
        for rho in rhos:
            s = rho * r / L
            if s >= 1.0:
                continue
            d = (np.sqrt(1.0 - s * s) * u + s * w).astype(np.float32)
            out.append(np.concatenate([e, oracle.vec_normalized(d, oracle.F32)[0]]))
    return np.array(out).reshape(-1, 6)


def shadow_rays(items, i, away, to_light, rhos=RHOS, azimuths=AZIMUTHS, toward=2):
    """Rays along `to_light` (the scene's unit light, negated: a shadow ray's direction) that pass item i at impact parameters rho r and
    START ON THE SURFACE of another item of the scene that lies behind i as the light sees it: the point where the line leaves that item
    towards the light, rounded to f32.  Azimuths as primary_rays, and for up to `toward` such items the azimuth that points at them.
    Lines that meet no other item give no ray.  float64[n, 6]."""
    it = np.asarray(items, dtype=np.float64).reshape(-1, 4)
    l = np.asarray(to_light, dtype=np.float64)
    lu = l / np.linalg.norm(l)
    c, r = it[i, :3], it[i, 3]
    rel = it[:, :3] - c
    along = rel @ lu
    perp = rel - along[:, None] * lu
    pm = np.linalg.norm(perp, axis=1)
    behind = along < 0.0
    behind[i] = False
    w0, w1 = _perp_frame(lu, np.asarray(away, dtype=np.float64))
    ws = [np.cos(np.radians(az)) * w0 + np.sin(np.radians(az)) * w1 for az in azimuths]
    near = np.nonzero(behind & (np.abs(pm - r) < 0.9 * it[:, 3]) & (pm > 1e-6 * r))[0]
    ws += [perp[j] / pm[j] for j in near[np.argsort(-along[near])][:toward]]
    out = []
    for w in ws:
        for rho in rhos:
            q = rho * r * w
            off = np.linalg.norm(perp - q, axis=1)
            hit = np.nonzero(behind & (off < 0.95 * it[:, 3]))[0]
            if not len(hit):
                continue
            j = hit[np.argmax(along[hit])]                     # the nearest one behind
            s = along[j] + np.sqrt(it[j, 3] ** 2 - off[j] ** 2)
            o = (c + q + s * lu).astype(np.float32).astype(np.float64)
            out.append(np.concatenate([o, l]))
    return np.array(out).reshape(-1, 6)


def check_bound(tally, item, spheres, rays, ordered):
    """The reference's f32 test of `item` and of each (tag, sphere) of `spheres` on every ray: where the item's distance is finite, each
    sphere's must be (1), and -- `ordered`: rays from an origin clearly outside the spheres -- not larger (2).  Violations go to `tally`."""
    import oracle
    for ray in rays:
        d_i = oracle.sphere_distance_from_ray(item, ray, oracle.F32)
        tally.rays += 1
        tally.unordered += not ordered
        if not np.isfinite(d_i):
            tally.misses += 1
            continue
        tally.hits += 1
        for tag, x in spheres:
            d_x = oracle.sphere_distance_from_ray(x, ray, oracle.F32)
            if not np.isfinite(d_x):
                tally.finite.append((tag, "finite", tuple(item), tuple(x), tuple(ray), d_i, d_x))
            elif ordered and d_x > d_i:
                tally.order.append((tag, "order", tuple(item), tuple(x), tuple(ray), d_i, d_x))


def check_scene(scene, spheres=None, tight=None, shadow=True):
    """check_bound for every tight bound of an rta.Scene (f32), its given sphere and every item of its subtree: primary-type rays from the
    scene's eye with (1) and (2), shadow-type rays along the scene's light with (1).  -> Tally."""
    if spheres is None:
        spheres, tight, _ = tight_of(scene)
    items = np.asarray(scene.items, dtype=np.float64)
    given = np.asarray(scene.bounds, dtype=np.float64)
    eye = np.asarray(scene.eye, dtype=np.float64)
    to_light = -np.asarray(scene.directional_light, dtype=np.float32).astype(np.float64)
    tally = Tally()
    for b in np.nonzero(tight)[0]:
        first, count = (int(v) for v in scene.ranges[b])
        x = np.asarray(spheres[b], dtype=np.float64)
        pair = (("tight", x), ("given", given[b]))
        for i in range(first, first + count):
            away = items[i, :3] - x[:3]
            check_bound(tally, items[i], pair, primary_rays(eye, items[i], away), ordered=True)
            if shadow:
                check_bound(tally, items[i], pair, shadow_rays(items, i, away, to_light), ordered=False)
    return tally


# ---- rim fixtures: tight balls known in closed form ------------------------------------------------------------------------------------

# name -> (items on the rim's circle, |v| / r of the rim item).  Every scene is a root with blocks, one per target pixel as in
# tests/edge_scenes.py, and a receiver behind them as the light sees it.  A block is a loose bound over equal spheres whose centres lie at
# one distance R from a point m: two opposite each other (m is their midpoint, exact in f32: centres are m +- h on a grid of 2^-20), or
# three on a circle, 120 degrees apart.  The smallest ball around them is {m, R + r}.  The first item touches it where the target pixel's
# ray passes: the ray is tangent to the item at its outermost point, and the radius (of all the block's items) is tuned to within 2 ulps of
# where the reference's verdict on it flips.
RIM = {"rim_pair": (2, 25.0), "rim_triple": (3, 40.0), "rim_far": (2, 1000.0)}
RIM_GRID = 2.0 ** -20
RIM_RECEIVER = (-3.7, -11.2, 8.5, 8.0)                        # downstream of the blocks along the light (-1, -3, 2)
RIM_ROOT = (-1.5, -4.5, 4.0, 20.0)                            # holds the eye: it keeps its record (rule (c))
RIM_MIN_TARGETS = 32


def _grid(v):
    return np.round(np.asarray(v, dtype=np.float64) / RIM_GRID) * RIM_GRID


@functools.lru_cache(maxsize=None)
def rim_scene(name):
    """The EdgeScene (tests/edge_scenes.py: f32, 128 x 128, one sample) of one rim fixture; .rim = one record per case: {case, ray, item, items,
    bound (indices in DFS order), centre (m), plain (the un-inflated ball {m, max |c - m| + r rounded up})}."""
    import oracle
    from tests import edge_scenes as es
    prec = oracle.F32
    n_items, ratio = RIM[name]
    rng = np.random.default_rng([17, sorted(RIM).index(name)])
    blocks = []
    for n, t in enumerate(es._targets(1, rng)[::2]):
        ray = es.sample_ray(es.W, es.H, 1, t[0], t[1], t[2], t[3], es.EYE, prec)
        o, d = np.asarray(ray[:3]), np.asarray(ray[3:])
        at = float(rng.uniform(2.5, 7.0))
        out = es._perp(d, rng)                                  # from m to the rim item; the ray is tangent there
        r = at / ratio
        R = r * float(rng.uniform(2.5, 4.0))
        m = _grid(o + at * d - (r + R) * out)
        if n_items == 2:
            dirs = [out, -out]
        else:
            q = es._perp(out, rng)
            dirs = [out, -0.5 * out + np.sqrt(0.75) * q, -0.5 * out - np.sqrt(0.75) * q]
        hs = [_grid(R * k) for k in dirs]
        if n_items == 2:
            hs[1] = -hs[0]
        centres = [m + h for h in hs]
        assert all(np.array_equal(c.astype(np.float32).astype(np.float64), c) for c in centres + [m]), (name, n)
        c0 = [float(x) for x in centres[0]]
        pred = lambda x, c0=c0, ray=ray: es._finite(prec, ray)(c0 + [x])
        flip = es.tune(pred, es.clearance(c0, ray), prec, hi_limit=at / 4)
        if flip is None:
            continue
        objs = [es.Item([float(x) for x in c] + [0.0]) for c in centres]
        reach = R + r
        loose = es._round(list(m + 0.3 * R * es._unit(rng.normal(size=3))) + [2.2 * reach + 0.12], prec)
        bd = es.Group(loose, objs)
        cs = es._case(name, prec, 1, t, "primary", ray, objs, es._offset(n), flip, pred)
        blocks.append((t, [bd], [cs], [ray], m))
    kept = es._screen([b[:4] for b in blocks], prec)
    centre_of = {id(b[2][0]): b[4] for b in blocks}
    root = es.Group(RIM_ROOT)
    for b in kept:
        root.children.extend(b[1])
    root.children.append(es.Item(RIM_RECEIVER))
    items, bounds, ranges, where = es._flatten(root)
    sc = es.EdgeScene(name, prec, 1, items, bounds, ranges, [])
    sc.rim = []
    for t, objs, cases, rays in kept:
        cs = cases[0]
        cs.nodes = [where[id(x)] for x in cs._objs]
        sc.cases.append(cs)
        idx = [i for _, i in cs.nodes]
        m = centre_of[id(cs)]
        reach = max(float(np.linalg.norm(items[i, :3] - m)) + float(items[i, 3]) for i in idx)
        sc.rim.append({"case": cs, "ray": cs.ray, "item": idx[0], "items": idx, "bound": where[id(objs[0])][1], "centre": m,
                       "plain": np.concatenate([m, [float(round_up(reach))]])})
    return sc


@functools.lru_cache(maxsize=None)
def rim_pair(name):
    """(EdgeScene, rta.Scene, oracle.Scene) of one rim fixture."""
    import rust_tracer_amd as rta
    from tests import util
    sc = rim_scene(name)
    s, o = util.scene_pair_ranges(sc.items, sc.bounds, sc.ranges, rta.RT_F32, light=sc.light, eye=sc.eye)
    return sc, s, o


# ---- the GPU side: a frame over the given and over the tight streams ---------------------------------------------------------------------

def _modes():
    from rust_tracer_amd import capi
    return {"generic": ((capi.DEBUG_FAST_KERNEL, 0), (capi.DEBUG_COOP, 0)),
            "lean": ((capi.DEBUG_FAST_KERNEL, 2), (capi.DEBUG_COOP, 0)),
            "lean_coop": ((capi.DEBUG_FAST_KERNEL, 2), (capi.DEBUG_COOP, 2)),
            "generic_coop": ((capi.DEBUG_FAST_KERNEL, 0), (capi.DEBUG_COOP, 2)),
            "one_ray": ((capi.DEBUG_SKIP_RAYS, 1),)}


MODES = _modes()                                               # name -> controls of csrc/rt_debug.h that pick the kernel of a launch
WALKS = ("generic", "lean", "lean_coop", "generic_coop")      # every kernel a one-sample pass can take; passes of more samples: + one_ray


def frames(d, ref, opts, regs, expect_tight=True, controls=(), count=True):
    """Renders `regs` on DeviceScene d with the given and with the tight streams (RT_DEBUG_TIGHT_BOUNDS 0 and 2) under `controls`; both must
    equal the oracle's frame `ref` where a tile covers it, and the launch says `tight_bounds` exactly for 2 where the scene has tight
    bounds.  count: the counting launch behind them, which must find no ITEM test where a tight bound would have culled.  -> launches
    that walked the tight streams."""
    import rust_tracer_amd as rta
    from rust_tracer_amd import capi
    from tests import util
    covered = np.zeros(ref.shape[:2], dtype=bool)
    for (l, t, r, b) in regs:
        covered[b:t, l:r] = True
    walked = 0
    for tb in (0, 2):
        with capi.debug(capi.DEBUG_TIGHT_BOUNDS, tb):
            for key, value in controls:
                capi.debug_set(key, value)
            try:
                data, st = d.render_tiles(opts, regs, rta.RT_TRAVERSAL_SKIP, want_stats=False)
                flags = capi.last_launch()
            finally:
                for key, _ in controls:
                    capi.debug_set(key, -1)
        frame = util.stitch(opts, regs, data)
        np.testing.assert_array_equal(frame[covered], ref[covered], err_msg="RT_DEBUG_TIGHT_BOUNDS %d" % tb)
        assert ("tight_bounds" in flags) == (tb == 2 and expect_tight), (tb, flags)
        walked += "tight_bounds" in flags
    if count:
        # ... and the counting launch (the given streams, the C++ loops): the same bytes, no bound's verdict violated (tests/conftest.py asserts the counter)
        data, st = d.render_tiles(opts, regs, rta.RT_TRAVERSAL_SKIP, want_stats=True)
        np.testing.assert_array_equal(util.stitch(opts, regs, data)[covered], ref[covered])
        # ... and no ITEM test of it counted where a tight bound would have put its lane to sleep
        assert capi.debug_count(capi.DEBUG_COUNT_TIGHT_VIOLATIONS) == 0
    return walked
