"""Scenes away from unit scale and away from the origin, for the ray, proximity and dynamic-scene entries (tests/test_scales_host.py checks
the inputs on the CPU, tests/test_gpu_scales.py runs them on the GPU).  numpy, the oracle and the host side of the package only.

placements(precision) -> [(name, f)]: f maps float64 (items, bounds, eye) to the placed values, each rounded once to the scene's REAL and
returned as float64 (what tests/test_gpu_fuzz.py test_scaled_scenes_every_loop_flavour's `sc` does).  bounds may be None.
  - uniform scales 1e-20, 1e-10, 1e6, 5e13: the frame tests' own.  At 1e-20 every f32 square (rr, vv, b*b ~ 1e-40) is a denormal; 5e13
    puts coordinates just under the 1e15 validation bound, squares at 1e29.
  - translations, radii unchanged: +(3000, -5000, 7000) in f32 (one ulp of a coordinate ~ 5e-4, the smallest radius 0.016), +(3e9, -5e9,
    7e9) in f64 (ulp ~ 1e-6), and in f64 the scene scaled by 1e3 and moved by +(0, 0, 9e14) (ulp 0.125, the smallest radius 16): c - o
    cancels, which no scaled scene does.

base_scenes() -> [(name, items, bounds, ranges)]: random_nested_scene(31) and the concentric random_nested_scene(32) of the frame tests
(depth 3, fan 3, two leaf items: 80 / 120 items under 40 bounds, some of which do not enclose their items, so that culling changes
answers), and the same items with no bounds at all: the flat walk.

case(precision, placement) -> [Case]: every base scene placed, with its oracle, 84 rays (ray_families, n_each = 12: one full wave and a
partly filled one) and 80 query points (query_families, n_each = 20).  Made once per process; nothing in a Case is written to.

casts(c) -> (rays, radius, which, tmax): the 80 sphere casts of a Case (cast_families and cutoffs of tests/test_gpu_sweep.py, n_each = 20: one
full wave and a partly filled one; radii 0, a quarter of the median, 0.5 - 2 medians, half the root and three roots), and margins(c): the
contact margins (0, r, -0.25 r, 4 r, +inf, -inf) with r the median placed item radius; ray_casts(c) -> (rays, zeros, tmax): the casts from
outside the root with radius 0 and cutoffs of their own (default_rng(400 + k)), which are ray queries.  Made on first use, once per process, for the
cast and contact tests (tests/test_scales_contact_host.py, tests/test_gpu_scales_contact.py); the other tests pay nothing for them.

overlap_queries(c) -> REAL[80, 4]: the query spheres of a Case for the overlap lists, drawn in the base scene's own frame and placed with
the scene, so that under the translations c - p cancels as c - o does for rays; displacements(c, family) -> REAL[n, 3]: the "slow" and
"fast" displacements of tests/test_gpu_impacts.py for the placed items; refit_twin(c) -> rta.Scene: the placed items under the case's
ranges with refit bounds, which enclose (brute force applies); POW2 and pow2_scaled(items0, disp0, k, R): exact power-of-two scalings of a
unit-scale scene and its displacements, under which the time of impact may not change a bit.  Made on first use, once per process, for
tests/test_scales_overlap_host.py and tests/test_gpu_scales_overlap.py."""
import functools

import numpy as np

import oracle
import rust_tracer_amd as rta
from tests import util
from tests.test_gpu_near import query_families
from tests.test_gpu_query import PREC, REAL, ray_families

SCALES = (1e-20, 1e-10, 1e6, 5e13)
EYE = (0.07, -0.12, -3.1)                    # the scaled frame tests' eye
LIGHT = (-1.0, -3.0, 2.0)
N_EACH_RAYS, N_EACH_POINTS = 12, 20
N_EACH_CASTS = 20
AIMED_FAMILIES = (0, 4)                      # ray_families: "outside the root, aimed at items" and "inside the root, aimed at items"


def _placement(R, scale=1.0, shift=(0.0, 0.0, 0.0)):
    shift = np.asarray(shift, dtype=np.float64)

    def f(items, bounds, eye):
        def spheres(a):
            if a is None:
                return None
            a = np.asarray(a, dtype=np.float64).reshape(-1, 4) * scale
            a[:, :3] += shift
            return a.astype(R).astype(np.float64)
        e = (np.asarray(eye, dtype=np.float64) * scale + shift).astype(R).astype(np.float64)
        return spheres(items), spheres(bounds), tuple(float(v) for v in e)
    return f


def placements(precision):
    R = REAL[precision]
    out = [("x%g" % s, _placement(R, scale=s)) for s in SCALES]
    if precision == rta.RT_F32:
        out.append(("+3e3", _placement(R, shift=(3000.0, -5000.0, 7000.0))))
    else:
        out.append(("+3e9", _placement(R, shift=(3e9, -5e9, 7e9))))
        out.append(("x1e3+9e14", _placement(R, scale=1e3, shift=(0.0, 0.0, 9e14))))
    return out


def placement_ids(precision):
    return [name for name, _ in placements(precision)]


def cases_of():
    """(precision, placement name) for every placement: the parameters of the tests."""
    return [(p, name) for p in (rta.RT_F32, rta.RT_F64) for name in placement_ids(p)]


def case_id(param):
    return "%s-%s" % ("f32" if param[0] == rta.RT_F32 else "f64", param[1])


def base_scenes():
    out = []
    for name, seed, concentric in (("nested", 31, False), ("concentric", 32, True)):
        items, bounds, ranges = util.random_nested_scene(seed, depth=3, fan=3, leaf_items=2, concentric=concentric)
        out.append((name, items, bounds, ranges))
    return out + [(name + "_flat", items, None, None) for name, items, _, _ in out]


class Case:
    """One base scene at one placement: .name, .scene (rta.Scene, host side), .oracle, .mode (the oracle's walk: hierarchy, or flat for the
    scene without bounds), .rays / .tmax, .points / .radius, and the unplaced and placed float64 arrays."""


@functools.lru_cache(maxsize=None)
def case(precision, placement):
    f = dict(placements(precision))[placement]
    light = rta.normalized(LIGHT, precision)
    out = []
    for k, (name, items0, bounds0, ranges) in enumerate(base_scenes()):
        c = Case()
        c.name, c.precision, c.placement = name, precision, placement
        c.items0, c.ranges = items0, ranges
        c.items, c.bounds, c.eye = f(items0, bounds0, EYE)
        if bounds0 is not None:
            c.scene, c.oracle = util.scene_pair_ranges(c.items, c.bounds, ranges, precision, light=LIGHT, eye=c.eye)
            c.mode = oracle.MODE_HIERARCHY
        else:
            c.scene = rta.Scene(c.items, light, c.eye, precision=precision)
            # the oracle wants a group: the bounded twin's, which its flat mode never looks at
            _, twin_bounds, twin_ranges = next(b[1:] for b in base_scenes() if b[0] == name[:-len("_flat")])
            c.oracle = oracle.Scene.from_ranges(c.items, f(items0, twin_bounds, EYE)[1], twin_ranges, LIGHT, c.eye, PREC[precision])
            c.mode = oracle.MODE_FLAT
        c.rays, c.tmax = ray_families(c.scene, np.random.default_rng(100 + k), N_EACH_RAYS)
        c.points, c.radius = query_families(c.scene, np.random.default_rng(200 + k), N_EACH_POINTS)
        out.append(c)
    return tuple(out)


_CASTS = {}


def casts(c):
    """(rays REAL[80, 6], radius REAL[80], which int[80], tmax REAL[80]) of Case c; family f in rows [20 f, 20 (f + 1))."""
    from tests.test_gpu_sweep import cast_families, cutoffs
    key = (c.precision, c.placement, c.name)
    if key not in _CASTS:
        k = [b[0] for b in base_scenes()].index(c.name)
        rng = np.random.default_rng(300 + k)
        rays, radius, which = cast_families(c.scene, rng, N_EACH_CASTS)
        tmax = cutoffs(rays, radius, c.scene.items, rng)
        for a in (rays, radius, which, tmax):
            a.setflags(write=False)
        _CASTS[key] = (rays, radius, which, tmax)
    return _CASTS[key]


def ray_casts(c):
    """(rays REAL[40, 6], zeros REAL[40], tmax REAL[40]): the casts of families 0 and 3 of Case c (from outside the root, aimed at items and aimed
    away) with radius 0 and cutoffs of their own: the casts that are ray queries."""
    from tests.test_gpu_sweep import cutoffs
    key = (c.precision, c.placement, c.name, "rays")
    if key not in _CASTS:
        k = [b[0] for b in base_scenes()].index(c.name)
        rays = casts(c)[0]
        rays = np.ascontiguousarray(np.concatenate([rays[:N_EACH_CASTS], rays[3 * N_EACH_CASTS:]]))
        zeros = np.zeros(len(rays), rays.dtype)
        tmax = cutoffs(rays, zeros, c.scene.items, np.random.default_rng(400 + k))
        for a in (rays, zeros, tmax):
            a.setflags(write=False)
        _CASTS[key] = (rays, zeros, tmax)
    return _CASTS[key]


def margins(c):
    """The contact margins of Case c: (0, r, -0.25 r, 4 r, +inf, -inf), r the median placed item radius."""
    r = float(np.median(c.scene.items[:, 3]))
    return (0.0, r, -0.25 * r, 4.0 * r, np.inf, -np.inf)


def oracle_nearest(c, rays=None, tmax=None):
    """(distance[n], normal[n, 3]) of the oracle's own walk, ray by ray, in float64."""
    rays = c.rays if rays is None else rays
    tmax = c.tmax if tmax is None else tmax
    out = [c.oracle.intersect(r.astype(np.float64), float(t), c.mode) for r, t in zip(rays, tmax)]
    return np.array([x[0] for x in out]), np.array([x[1] for x in out])


def shuffled(items, R, seed=7):
    """The placed items in a seeded random caller order, as a rebuild takes them."""
    it = np.ascontiguousarray(np.asarray(items).astype(R))
    return np.ascontiguousarray(it[np.random.default_rng(seed).permutation(len(it))])


def sort_inputs(precision, n=300001, duplicates=1000, seed=41):
    """n spheres with centres uniform in a box, `duplicates` of them exact copies of other centres (other radii), in a seeded random order:
    more than the 262,144 threads of one pass of the sphere sort's strided kernels."""
    R = REAL[precision]
    rng = np.random.default_rng(seed)
    s = np.concatenate([rng.uniform([-3.0, -2.0, 0.0], [3.0, 2.0, 6.0], (n, 3)), rng.uniform(0.01, 0.03, (n, 1))], axis=1)
    s[n - duplicates:, :3] = s[rng.choice(n - duplicates, duplicates, replace=False), :3]
    return np.ascontiguousarray(s[rng.permutation(n)].astype(R))


N_OVERLAP_QUERIES = 80                       # one full wave and a partly filled one
POW2 = (-66, -40, -33, 33, 45)               # exponents k of the exact scalings by 2^k of pow2_scaled


def _index(c):
    return [b[0] for b in base_scenes()].index(c.name)


def overlap_queries(c):
    """REAL[80, 4] of Case c: centres uniform in 1.2 times the base items' box about its centre, q uniform in [0, 0.3 extent] with every
    tenth q = 0, drawn from default_rng(800 + k) in the base scene's frame and mapped through the case's placement, rounded once."""
    from tests.test_gpu_impacts import extent
    key = (c.precision, c.placement, c.name, "overlap queries")
    if key not in _CASTS:
        rng = np.random.default_rng(800 + _index(c))
        it = np.asarray(c.items0, dtype=np.float64).reshape(-1, 4)
        lo, hi = (it[:, :3] - it[:, 3:]).min(axis=0), (it[:, :3] + it[:, 3:]).max(axis=0)
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        centres = mid + rng.uniform(-1.2, 1.2, (N_OVERLAP_QUERIES, 3)) * half
        q = rng.uniform(0.0, 0.3 * extent(it), N_OVERLAP_QUERIES)
        q[::10] = 0.0
        f = dict(placements(c.precision))[c.placement]
        placed = f(np.concatenate([centres, q[:, None]], axis=1), None, EYE)[0]
        queries = np.ascontiguousarray(placed.astype(REAL[c.precision]))
        queries.setflags(write=False)
        _CASTS[key] = queries
    return _CASTS[key]


def displacements(c, family):
    """REAL[n, 3] of Case c: tests/test_gpu_impacts.py's displacements of the placed items, seed 900 + k; family "slow" (factors of the placed
    median radius) or "fast" (of the placed extent)."""
    from tests.test_gpu_impacts import displacements as make
    key = (c.precision, c.placement, c.name, "displacements", family)
    if key not in _CASTS:
        disp = make(c.scene.items, 900 + _index(c), family, REAL[c.precision])
        disp.setflags(write=False)
        _CASTS[key] = disp
    return _CASTS[key]


def refit_twin(c):
    """rta.Scene (host side): the items of Case c under its ranges -- the bounded twin's for a scene without bounds -- with
    rta.refit_bounds, which enclose their items."""
    key = (c.precision, c.placement, c.name, "refit twin")
    if key not in _CASTS:
        R = REAL[c.precision]
        name = c.name[:-len("_flat")] if c.name.endswith("_flat") else c.name
        ranges = next(b[3] for b in base_scenes() if b[0] == name)
        items = np.ascontiguousarray(c.scene.items.astype(R))
        bounds = rta.refit_bounds(items, ranges, c.precision)
        _CASTS[key] = rta.Scene(items, rta.normalized(LIGHT, c.precision), c.eye, bounds, ranges, c.precision)
    return _CASTS[key]


def pow2_scaled(items0, disp0, k, R):
    """(items REAL[n, 4], disp REAL[n, 3]): items0 and disp0, both already REAL, times 2^k -- exact as long as nothing leaves the normal range."""
    items = np.ascontiguousarray(np.ldexp(np.asarray(items0, dtype=R), k).astype(R))
    disp = np.ascontiguousarray(np.ldexp(np.asarray(disp0, dtype=R), k).astype(R))
    return items, disp
