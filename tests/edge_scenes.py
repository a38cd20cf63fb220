"""Deterministic edge-case scenes for the traversal's conservative bounds (NOTES.md "Edge scenes").

Every case is one node of a small scene tuned, ulp by ulp, to the point where the reference's own result for one target sample ray flips:
an item or a bound that a primary or a shadow ray only just grazes, or a bound whose entry distance lands on the best hit so far.  The
oracle (the C restatement of the reference) decides where the flip is; mpmath gives the exact geometry the walk starts from.  A case sits
`offset` ulps from its flip (offset >= 0: the side where the reference says HIT / ENTER), so a bound whose margin is too small, or a
comparison of the wrong strictness, decides one of them differently from the reference.

Families (each at f32 and f64, for sample rays of spp 1, 2 and 4):
  P1  items grazing primary sample rays, |v| / r from 40 to 1e6; P1c the eye just outside a sphere, on both sides of the primary filter's
      64 eps cut-off (four such spheres per scene, one per edge of the frame: each fills the frame beyond its target ray), P1 grazes between
  P2  bounds grazing primary rays (an item inside: entering adds a test)
  P3  a bound whose entry t1 lands on the distance D of an item hit earlier in DFS order (the root-free BOUND decision at its edge)
  S1  occluders grazing the shadow ray of a receiver's hit, from just past the origin to the far side of the scene; occluders beside the
      origin (centre at a = (c - o) . l within +-3e-4 of 0, where the shadow bounds' a0 lies); occluders just behind the origin, tuned to
      the origin on their surface (the cases on the HIT side have the origin just inside)
  S2  bounds grazing shadow rays
  O   fused scenes (every bound followed by an item with its centre): own items grazing primary and shadow rays, the own radius smaller
      than, bit-equal to or larger than the bound's
  T   the terminator: a receiver's centre coordinate tuned until the reference's g = n . light changes sign at the target sample; on the
      lit side the shadow ray leaves its own sphere almost tangentially

numpy + mpmath + oracle only: no GPU.
"""
import functools
from dataclasses import dataclass, field

import mpmath
import numpy as np

import oracle

W = H = 128
STRIDE = 8                                   # target pixels: one per STRIDE x STRIDE block
EYE = (0.0, 0.0, -4.0)
LIGHT = (-1.0, -3.0, 2.0)
K = 2                                        # cases sit at flip - K .. flip + K ulps
FAMILIES = ("P1", "P1c", "P2", "P3", "S1", "S2", "O", "T")
PRECS = (oracle.F32, oracle.F64)
SPPS = (1, 2, 4)
REAL = {oracle.F32: np.float32, oracle.F64: np.float64}
UINT = {oracle.F32: np.uint32, oracle.F64: np.uint64}
REPS = {oracle.F32: float(np.finfo(np.float32).eps), oracle.F64: float(np.finfo(np.float64).eps)}


# ---- the reference's rays, restated --------------------------------------------------------------------------------------------------

def sample_rays(w, h, spp, x, y, ssx, ssy, eye, prec):
    """Primary rays of samples (ssx, ssy) of pixels (x, y) (arrays, broadcast; render.rs:231-241): pos = eye, dir = (x + ssx/spp - w/2,
    (h - (y + ssy/spp)) - h/2, w) normalised as vec.rs:87-95 (times 1 / sqrt((x*x + y*y) + z*z)), REAL arithmetic -> REAL[..., 6]."""
    R = REAL[prec]
    ssf = R(spp)
    xres = np.asarray(x).astype(R) + np.asarray(ssx).astype(R) / ssf
    yres = np.asarray(y).astype(R) + np.asarray(ssy).astype(R) / ssf
    dx, dy = xres - R(w) / R(2), (R(h) - yres) - R(h) / R(2)
    dx, dy = np.broadcast_arrays(dx, dy)
    dz = np.full_like(dx, R(w))
    inv = R(1) / np.sqrt((dx * dx + dy * dy) + dz * dz)
    out = np.empty(dx.shape + (6,), dtype=R)
    out[..., :3] = np.asarray(eye, dtype=R)
    out[..., 3], out[..., 4], out[..., 5] = dx * inv, dy * inv, dz * inv
    return out


def sample_ray(w, h, spp, x, y, ssx, ssy, eye, prec):
    """One sample ray (sample_rays), as float64[6] of REAL values."""
    return sample_rays(w, h, spp, x, y, ssx, ssy, eye, prec).astype(np.float64)


def light_of(prec, light=LIGHT):
    """The scene's directional light as the reference normalises it (render.rs:154-159)."""
    return oracle.vec_normalized(np.asarray(light, dtype=np.float64), prec)[0]


def shade(sphere, ray, prec, light=LIGHT):
    """What render.rs:186-207 makes of `ray` hitting `sphere` (as the nearest hit): (distance, g = n . light, shadow ray float64[6] or None
    where g >= 0).  The shadow ray starts at (pos + dir d) + n (d sqrt(EPSILON)) (rt_oracle_impl.h raytrace) and runs along -light."""
    R = REAL[prec]
    d, n = oracle.sphere_intersect(sphere, ray, float("inf"), prec)
    if not np.isfinite(d):
        return d, None, None
    d, n = R(d), n.astype(R)
    lt = light_of(prec, light).astype(R)
    g = (n[0] * lt[0] + n[1] * lt[1]) + n[2] * lt[2]
    if not g < 0:
        return float(d), float(g), None
    return float(d), float(g), shadow_ray(ray, d, n, prec, light)


def shadow_ray(ray, d, n, prec, light=LIGHT):
    """The shadow ray of a primary hit at distance d with unit normal n (render.rs:199-207), float64[6]."""
    R = REAL[prec]
    pos, dr = np.asarray(ray[:3], dtype=R), np.asarray(ray[3:], dtype=R)
    n = np.asarray(n, dtype=R)
    k = R(d) * R(np.sqrt(R(REPS[prec])))
    p = (pos + dr * R(d)) + n * k
    return np.concatenate([p, -light_of(prec, light).astype(R)]).astype(np.float64)


# ---- exact geometry ------------------------------------------------------------------------------------------------------------------

def exact_terms(sphere, ray, bits=240):
    """(b, vv, rr, disc) of primitive.rs:55-72 in exact arithmetic on the given (REAL) values -- the reference's formula, no rounding."""
    with mpmath.workprec(bits):
        c = [mpmath.mpf(float(x)) for x in sphere[:3]]
        o = [mpmath.mpf(float(x)) for x in ray[:3]]
        dr = [mpmath.mpf(float(x)) for x in ray[3:6]]
        v = [c[i] - o[i] for i in range(3)]
        b = sum(v[i] * dr[i] for i in range(3))
        vv = sum(x * x for x in v)
        rr = mpmath.mpf(float(sphere[3])) ** 2
        return b, vv, rr, b * b - vv + rr


def exact_distance(sphere, ray, bits=240):
    """Sphere::distance_from_ray evaluated exactly: t1 if t1 > 0, else t2 if t2 >= 0, else +inf (as an mpf, or inf)."""
    with mpmath.workprec(bits):
        b, vv, rr, disc = exact_terms(sphere, ray, bits)
        if disc < 0:
            return mpmath.inf
        s = mpmath.sqrt(disc)
        if b + s < 0:
            return mpmath.inf
        return b - s if b - s > 0 else b + s


def clearance(centre, ray, bits=240):
    """Exact distance of `centre` from the line of `ray` (the direction need not be exactly unit), as a float."""
    with mpmath.workprec(bits):
        b, vv, _, _ = exact_terms(list(centre) + [0.0], ray, bits)
        dd = sum(mpmath.mpf(float(x)) ** 2 for x in ray[3:6])
        return float(mpmath.sqrt(max(vv - b * b / dd, mpmath.mpf(0))))


# ---- tuning to the flip --------------------------------------------------------------------------------------------------------------

def _bits(x, prec):
    """The REAL's bit pattern as an integer in the order of the values (negative values: minus their magnitude's pattern)."""
    k = int(np.array(x, dtype=REAL[prec]).view(UINT[prec]))
    sign = 1 << (8 * np.dtype(REAL[prec]).itemsize - 1)
    return k if k < sign else -(k - sign)


def _val(k, prec):
    sign = 1 << (8 * np.dtype(REAL[prec]).itemsize - 1)
    return float(np.array(k if k >= 0 else sign - k, dtype=UINT[prec]).view(REAL[prec]))


def step_ulps(x, k, prec):
    """x moved k ulps (finite x)."""
    return _val(_bits(x, prec) + k, prec)


def bisect(pred, lo, hi, prec):
    """The smallest REAL in (lo, hi] with pred, for pred(lo) False and pred(hi) True: a flip (the first one, if pred is monotone)."""
    a, b = _bits(lo, prec), _bits(hi, prec)
    while b - a > 1:
        m = (a + b) // 2
        if pred(_val(m, prec)):
            b = m
        else:
            a = m
    return _val(b, prec)


def tune(pred, x0, prec, hi_limit):
    """The smallest positive REAL x <= hi_limit with pred(x), for pred monotone in x (False below the flip, True from it on), searched from
    x0 by doubling / halving and then bisection of the bit pattern.  None if pred is True down to the smallest normal or False up to
    hi_limit."""
    R = REAL[prec]
    x = float(R(x0))
    tiny = float(np.finfo(R).tiny)
    if pred(x):
        hi = x
        lo = x / 2
        while pred(lo):
            if lo < tiny:
                return None
            hi, lo = lo, lo / 2
        lo = float(R(lo))
    else:
        lo = x
        hi = x * 2
        while not pred(hi):
            if hi > hi_limit:
                return None
            lo, hi = hi, hi * 2
        hi = float(R(hi))
    return bisect(pred, lo, hi, prec)


# ---- scenes --------------------------------------------------------------------------------------------------------------------------

class Group:
    def __init__(self, sphere, children=()):
        self.sphere = [float(x) for x in sphere]
        self.children = list(children)


class Item:
    def __init__(self, sphere):
        self.sphere = [float(x) for x in sphere]


@dataclass
class Case:
    family: str
    prec: int
    spp: int
    pixel: tuple                 # (x, y)
    sample: tuple                # (ssx, ssy)
    kind: str                    # "primary" / "shadow": which ray of the target sample the node is tuned against
    ray: np.ndarray              # that ray (float64[6] of REAL values)
    nodes: list                  # [("items" | "bounds", DFS index), ...]: the tuned node(s) (O: a bound and its own item bit-equal)
    offset: int                  # ulps from the flip; >= 0: the reference says HIT / ENTER
    flip: float                  # the smallest radius for which it does
    value: float                 # the node's radius in the scene (flip moved `offset` ulps)
    other: float                 # the nearest radius on the other side of the flip
    outcome: bool                # the reference's verdict at `value`
    best: float = float("inf")   # P3: the distance the bound's entry is compared with
    note: str = ""
    col: int = 3                 # the tuned column of the node's (cx, cy, cz, r): the radius; T: a centre coordinate
    sense: bool = True           # T: the verdict is "g >= 0" (True) or "g < 0" (False)
    _objs: list = field(default_factory=list, repr=False)


@dataclass
class EdgeScene:
    family: str
    prec: int
    spp: int
    items: np.ndarray
    bounds: np.ndarray
    ranges: np.ndarray
    cases: list
    w: int = W
    h: int = H
    eye: tuple = EYE
    light: tuple = LIGHT

    def oracle(self, items=None, bounds=None):
        return oracle.Scene.from_ranges(self.items if items is None else items, self.bounds if bounds is None else bounds, self.ranges,
                                        self.light, self.eye, self.prec)

    def moved(self, case, value):
        """(items, bounds) with the case's node(s) at radius `value`."""
        items, bounds = self.items.copy(), self.bounds.copy()
        for kind, i in case.nodes:
            (items if kind == "items" else bounds)[i, case.col] = value
        return items, bounds

    @property
    def name(self):
        return "%s-%s-spp%d" % (self.family, "f32" if self.prec == oracle.F32 else "f64", self.spp)


def _flatten(root):
    items, bounds, ranges, where = [], [], [], {}

    def rec(g):
        bi = len(bounds)
        bounds.append(g.sphere)
        ranges.append(None)
        where[id(g)] = ("bounds", bi)
        first = len(items)
        for c in g.children:
            if isinstance(c, Group):
                rec(c)
            else:
                where[id(c)] = ("items", len(items))
                items.append(c.sphere)
        assert len(items) > first, "a group without items"
        ranges[bi] = (first, len(items) - first)

    rec(root)
    return np.array(items, dtype=np.float64), np.array(bounds, dtype=np.float64), np.array(ranges, dtype=np.int32), where


def _targets(spp, rng):
    """(x, y, ssx, ssy) per STRIDE block.  One column / row of blocks aims at x = w/2 / y = h/2 with sample 0: direction components that
    are exactly zero; the rest spread over the four quadrants (mixed signs)."""
    out = []
    for j in range(H // STRIDE):
        for i in range(W // STRIDE):
            x, y = STRIDE * i + int(rng.integers(2, STRIDE - 2)), STRIDE * j + int(rng.integers(2, STRIDE - 2))
            ssx, ssy = int(rng.integers(0, spp)), int(rng.integers(0, spp))
            if i == W // STRIDE // 2:
                x, ssx = W // 2, 0
            if j == H // STRIDE // 2:
                y, ssy = H // 2, 0
            out.append((x, y, ssx, ssy))
    return out


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _perp(d, rng):
    u = np.cross(d, rng.normal(size=3))
    return _unit(u)


def _round(sphere, prec):
    return [float(REAL[prec](x)) for x in sphere]


def _finite(prec, ray):
    return lambda sph: np.isfinite(oracle.sphere_distance_from_ray(sph, ray, prec))


def _graze(rng, prec, ray, at, rho_lo, rho_hi, pred_for=None):
    """A centre at distance `at` along `ray`, off the line by the radius it gets, |centre - origin| / r log-uniform in [rho_lo, rho_hi];
    the radius tuned to the reference's flip for pred(sphere) (default: a finite distance).  (centre, flip) or None."""
    d = np.asarray(ray[3:], dtype=np.float64)
    rho = 10 ** rng.uniform(np.log10(rho_lo), np.log10(rho_hi))
    r = at / rho
    c = _round(np.asarray(ray[:3]) + at * d + r * _perp(d, rng), prec)
    r0 = clearance(c, ray)
    pred = (pred_for or _finite)(prec, ray)
    flip = tune(lambda x: pred(c + [x]), r0 if r0 > 0 else r, prec, hi_limit=at / 4)
    return (c, flip) if flip is not None else None


def _offset(n):
    return (n % (2 * K + 1)) - K


def _case(family, prec, spp, t, kind, ray, objs, off, flip, pred_of, note="", best=float("inf"), col=3, sense=True):
    value = step_ulps(flip, off, prec)
    other = step_ulps(flip, -1, prec) if off >= 0 else flip
    for o in objs:
        o.sphere[col] = value
    c = Case(family, prec, spp, (t[0], t[1]), (t[2], t[3]), kind, ray, [], off, flip, value, other, bool(pred_of(value)), best, note, col,
             sense)
    c._objs = objs
    return c


def _receiver(ray, at, prec, rng, want=None):
    """An item hit by `ray` at about `at`, where the normal faces both the eye and the light (g < 0: the sample casts a shadow ray)."""
    d = np.asarray(ray[3:], dtype=np.float64)
    if want is None:
        want = _unit(-light_of(prec) - d + 0.1 * rng.normal(size=3))
    rad = at / 150.0
    sph = _round(list(np.asarray(ray[:3]) + at * d - rad * want) + [rad], prec)
    dist, g, sray = shade(sph, ray, prec)
    return sph, sray


def _near_log(prec):
    """log10 of the nearest an occluder is put to a shadow ray's origin.  The origin is pushed off the hit by d sqrt(EPSILON) (render.rs:199),
    about as far as the primary ray's own rounding band reaches at that distance (~ sqrt(u) d): an occluder much nearer than a few times
    that is "hit" by the sample's primary ray too, at either precision."""
    return -2.3 if prec == oracle.F32 else -6.0


def _near_origin(rng, prec, ray, sray, rec, beside):
    """An occluder next to the shadow ray's origin o, its centre at a = (c - o) . l along the ray and P off it.  beside: |a| from 1e-7 to
    3e-4, either sign (the shadow bounds' a0 = 11 2^-24 S is about 1e-5 here), P from 5e-3 to 0.03 or (tiny) from 3e-6 to 3e-5; else just behind the origin (the bounds' kc test), radius
    3e-3 to 0.05, its surface through o.  The radius is tuned to the flip: a grazing ray for a > 0, the origin on the surface for a < 0 (the cases
    on the HIT side then start inside).  The origin lies d sqrt(EPSILON) off the primary hit, inside the primary ray's own rounding band, so
    the geometric screen cannot clear such an occluder: the reference's test of the sample's primary ray against it must not beat the
    receiver, at every radius within a few ulps of the flip.  The occluder goes to the side of the light's plane away from the primary ray.
    (centre, flip, note) or None."""
    o, l, dr = np.asarray(sray[:3]), np.asarray(sray[3:]), np.asarray(ray[3:])
    side = _unit(np.cross(l, dr))
    n_rec = _unit(o - np.asarray(rec[:3]))
    d_rec = oracle.sphere_distance_from_ray(rec, ray, prec)
    for _ in range(16):
        if beside and rng.uniform() < 0.4:
            # tiny: r within 1e-5.5 .. 1e-4.5, where the inner bound's (1 + 2^-10) margin leaves s = sqrt(rr - P^2) comparable with a0
            a = float(rng.choice([-1.0, 1.0]) * 10 ** rng.uniform(-7, -5.3))
            P = float(10 ** rng.uniform(-5.5, -4.5))
        elif beside:
            a = float(rng.choice([-1.0, 1.0]) * 10 ** rng.uniform(-7, np.log10(3e-4)))
            P = float(10 ** rng.uniform(-2.3, -1.5))
        else:
            # the surface through o, its outward normal w there perpendicular to the primary ray and turned towards the receiver (o lies
            # off the hit along the receiver's normal, so the primary ray then passes o on the outside) and along l (centre behind o)
            lp, mp = _unit(l - (l @ dr) * dr), _unit(n_rec - (n_rec @ dr) * dr)
            w = _unit(lp - (lp @ mp + float(rng.uniform(0.15, 0.4))) * mp)
            if not (w @ l > 0.05 and w @ n_rec < -0.05):
                continue
            rad = float(10 ** rng.uniform(-2.5, -1.3))
            a, P = -rad * float(w @ l), rad * float(np.sqrt(max(1.0 - (w @ l) ** 2, 0.0)))
            c = _round(o - rad * w, prec)
        if beside:
            u = _unit(float(rng.choice([-1.0, 1.0])) * side + 0.3 * _perp(l, rng))
            u = _unit(u - (u @ l) * l)
            c = _round(o + a * l + P * u, prec)
        pred = lambda x, c=c: _finite(prec, sray)(c + [x])
        flip = tune(pred, float(np.sqrt(P * P + (a * a if a < 0 else 0.0))), prec, hi_limit=1.0)
        if flip is None:
            continue
        if all(not oracle.sphere_distance_from_ray(c + [step_ulps(flip, k, prec)], ray, prec) < d_rec for k in range(-K - 2, K + 3)):
            return c, flip, ("a=%.3g" % a) if beside else ("behind=%.3g" % a)
    return None


def _terminator(rng, prec, ray, at):
    """A receiver whose surface normal at the target sample's hit is perpendicular to the light (g = n . light ~ 0), and the centre
    coordinate along which g moves fastest bracketed around its sign change.  (sphere, column, lo, hi, sense, pred) or None."""
    d = np.asarray(ray[3:], dtype=np.float64)
    lt = light_of(prec)
    n0 = _unit(-d - (-d @ lt) * lt + 0.02 * rng.normal(size=3))
    rad = at / 150.0
    sph = _round(list(np.asarray(ray[:3]) + at * d - rad * n0) + [rad], prec)
    col = int(np.argmax(np.abs(lt)))

    def g(x):
        s2 = list(sph)
        s2[col] = x
        r = shade(s2, ray, prec)
        return r[1]
    lo, hi = float(REAL[prec](sph[col] - 0.05 * rad)), float(REAL[prec](sph[col] + 0.05 * rad))
    glo, ghi = g(lo), g(hi)
    if glo is None or ghi is None or (glo >= 0) == (ghi >= 0):
        return None
    sense = ghi >= 0

    def pred(x):
        gx = g(x)
        return gx is not None and (gx >= 0) == sense
    return sph, col, lo, hi, sense, pred


def node_sphere(sc, case, value):
    """The case's (first) node with its tuned column at `value`, as [cx, cy, cz, r]."""
    kind, i = case.nodes[0]
    row = [float(x) for x in (sc.items if kind == "items" else sc.bounds)[i]]
    row[case.col] = value
    return row


def verdict(sc, case, value):
    """The reference's verdict for the case's node at `value`: a finite distance (a primary ray's item or bound with nothing hit yet, every
    shadow test), a distance below the best hit so far (P3: the bound is entered), or (T) the sign of g = n . light at the hit."""
    sph = node_sphere(sc, case, value)
    if case.kind == "terminator":
        g = shade(sph, case.ray, case.prec)[1]
        return g is not None and (g >= 0) == case.sense
    return oracle.sphere_distance_from_ray(sph, case.ray, case.prec) < case.best


def _blocks(family, prec, spp, rng):
    """[(target, block objects (children of the root), [cases], [(ray, exempt objects)])] for one scene."""
    out = []
    for n, t in enumerate(_targets(spp, rng)):
        ray = sample_ray(W, H, spp, t[0], t[1], t[2], t[3], EYE, prec)
        at = float(rng.uniform(2.5, 8.0))
        off = _offset(n)
        if family == "P1":
            g = _graze(rng, prec, ray, at, 40.0, 1e6)
            if g is None:
                continue
            it = Item(g[0] + [0.0])
            out.append((t, [it], [_case(family, prec, spp, t, "primary", ray, [it], off, g[1], lambda x, c=g[0]: _finite(prec, ray)(c + [x]))],
                        [ray]))
        elif family == "P2":
            g = _graze(rng, prec, ray, at, 40.0, 1e6)
            if g is None:
                continue
            inner = Item(g[0] + [0.0])
            bd = Group(g[0] + [0.0], [inner])
            cs = _case(family, prec, spp, t, "primary", ray, [bd], off, g[1], lambda x, c=g[0]: _finite(prec, ray)(c + [x]))
            inner.sphere[3] = float(REAL[prec](bd.sphere[3] * 0.5))
            out.append((t, [bd], [cs], [ray]))
        elif family == "P3":
            d = np.asarray(ray[3:], dtype=np.float64)
            ra = at / 150.0
            a = _round(list(np.asarray(ray[:3]) + (at + ra) * d) + [ra], prec)
            best = oracle.sphere_distance_from_ray(a, ray, prec)
            if not np.isfinite(best):
                continue
            # b - best: from a few ulps of best (b ~ best) up to 1/300 of it; or (every other case) beyond best, b > 2 best, where b - best
            # itself is rounded -- chosen rounded UP: there the reference's root enters with RN(sqrt(disc)) = RN(b - best) and disc just
            # below (b - best)^2, the window that only the decision's 2^-20 margin keeps it out of
            for _ in range(40):
                far = n % 2 == 0
                delta = at * (rng.uniform(1.1, 3.0) if far else 10 ** rng.uniform(-7, np.log10(1 / 300.0)))
                hh = delta * 10 ** rng.uniform(-3, np.log10(0.5)) if n % 4 else 0.0   # off the ray (some head-on)
                c = _round(np.asarray(ray[:3]) + (best + delta) * d + hh * _perp(d, rng), prec)
                if not far or _rounded_up_gap(c, ray, best, prec):
                    break
            else:
                continue

            def enters(x, c=c, best=best):
                return oracle.sphere_distance_from_ray(c + [x], ray, prec) < best
            flip = tune(enters, np.sqrt(delta * delta + hh * hh), prec, hi_limit=4 * at)
            if flip is None:
                continue
            inner = Item(c + [0.0])
            bd = Group(c + [0.0], [inner])
            cs = _case(family, prec, spp, t, "primary", ray, [bd], off, flip, enters, note="b-best=%.3g" % delta, best=best)
            inner.sphere[3] = float(REAL[prec](min(bd.sphere[3] * 0.25, at / 300.0)))
            out.append((t, [Item(a), bd], [cs], [ray]))
        elif family == "S1" and n % 3:
            m = None
            if n % 3 == 2:
                # behind: the receiver's normal, seen along the primary ray, turned 50 - 80 degrees away from the light's direction, so
                # that a sphere through the shadow origin can lie behind it and still leave the primary ray outside
                dd = np.asarray(ray[3:])
                lp = -light_of(prec) - (-light_of(prec) @ dd) * dd
                q = _unit(np.cross(dd, lp))
                th = np.radians(rng.uniform(50.0, 80.0))
                m = np.cos(th) * _unit(lp) + np.sin(th) * q
                m = _unit(-dd + m)
            rec, sray = _receiver(ray, at, prec, rng, m)
            if sray is None:
                continue
            blk = _near_origin(rng, prec, ray, sray, rec, beside=n % 3 == 1)
            if blk is None:
                continue
            c, flip, note = blk
            occ = Item(c + [0.0])
            cs = _case(family, prec, spp, t, "shadow", sray, [occ], off, flip, lambda x, c=c: _finite(prec, sray)(c + [x]), note=note)
            out.append((t, [Item(rec), occ], [cs], [ray, sray]))
        elif family == "T":
            blk = _terminator(rng, prec, ray, at)
            if blk is None:
                continue
            rec, col, lo, hi, sense, pred = blk
            flip = bisect(pred, lo, hi, prec)
            value = step_ulps(flip, off, prec)
            # g jitters with the centre at the scale of its rounding: keep the case only where the ulps around it are on one side
            if any(pred(step_ulps(flip, k, prec)) != (k >= 0) for k in range(min(off, -1) - 1, max(off, 0) + 2)):
                continue
            it = Item(rec)
            cs = _case(family, prec, spp, t, "terminator", ray, [it], off, flip, pred, note="c%d" % col, col=col, sense=sense)
            assert value == cs.value
            out.append((t, [it], [cs], [ray]))
        elif family in ("S1", "S2"):
            rec, sray = _receiver(ray, at, prec, rng)
            if sray is None:
                continue
            far = float(10 ** rng.uniform(_near_log(prec), 0.7))             # from just past the origin to across the scene
            g = _graze(rng, prec, sray, far, 20.0 if far > 1e-2 else 4.0, 1e5)
            if g is None or _near(ray, g[0] + [g[1] * 1.05], prec):       # (the sample's own primary ray must not find it)
                continue
            if family == "S1":
                occ = Item(g[0] + [0.0])
                node = occ
                cs = _case(family, prec, spp, t, "shadow", sray, [occ], off, g[1], lambda x, c=g[0]: _finite(prec, sray)(c + [x]),
                           note="t=%.3g" % far)
            else:
                inner = Item(g[0] + [0.0])
                node = Group(g[0] + [0.0], [inner])
                cs = _case(family, prec, spp, t, "shadow", sray, [node], off, g[1], lambda x, c=g[0]: _finite(prec, sray)(c + [x]),
                           note="t=%.3g" % far)
                inner.sphere[3] = float(REAL[prec](node.sphere[3] * 0.5))
            out.append((t, [Item(rec), node], [cs], [ray, sray]))
        elif family == "O":
            kind = ("primary", "shadow")[n % 2]
            rel = (n // 2) % 3                                               # own radius < / == / > the bound's
            lead, rays = [], [ray]
            tray = ray
            if kind == "shadow":
                rec, tray = _receiver(ray, at, prec, rng)
                if tray is None:
                    continue
                lead = [Item(rec)]
                rays = [ray, tray]
                at = float(10 ** rng.uniform(_near_log(prec), 0.5))
            g = _graze(rng, prec, tray, at, 40.0, 1e5)
            if g is None or (kind == "shadow" and _near(ray, g[0] + [g[1] * 1.05], prec)):
                continue
            own = Item(g[0] + [0.0])
            bd = Group(g[0] + [0.0], [own])
            pred = lambda x, c=g[0], tr=tray: _finite(prec, tr)(c + [x])
            if rel == 0:            # own smaller: the bound is entered either way (tuned: the own item)
                cs = _case(family, prec, spp, t, kind, tray, [own], off, g[1], pred, note="own<bound")
                bd.sphere[3] = float(REAL[prec](own.sphere[3] * float(rng.uniform(1.5, 3.0))))
            elif rel == 1:          # bit-equal: bound and own item move together
                cs = _case(family, prec, spp, t, kind, tray, [own, bd], off, g[1], pred, note="own==bound")
            else:                   # own larger: the bound decides whether the own item is tested (tuned: the bound)
                cs = _case(family, prec, spp, t, kind, tray, [bd], off, g[1], pred, note="own>bound")
                own.sphere[3] = float(REAL[prec](bd.sphere[3] * float(rng.uniform(1.5, 3.0))))
            out.append((t, lead + [bd], [cs], rays))
    return out


def _rounded_up_gap(c, ray, best, prec):
    """Is w = RN(b - best) above the exact b - best, for b = dot(c - pos, dir) as the reference rounds it?"""
    from fractions import Fraction
    R = REAL[prec]
    v = np.asarray(c, dtype=R) - np.asarray(ray[:3], dtype=R)
    dr = np.asarray(ray[3:], dtype=R)
    b = (v[0] * dr[0] + v[1] * dr[1]) + v[2] * dr[2]
    return Fraction(float(b - R(best))) > Fraction(float(b)) - Fraction(float(best))


def _cutoff_block(prec, spp, rng, idx, where):
    """P1c: the eye just outside a sphere, |v| - r within a few 2^-18 |v| of the primary filter's cut-off (vv - rr < 64 eps (vv + rr),
    eps = 2^-24, at either precision).  Such a sphere fills about half the view: one per edge of the frame (`where`), its silhouette through
    the target ray, which lies near that edge; the sphere covers the frame beyond it."""
    lo, hi = (16, 28) if where in ("left", "top") else (100, 112)
    across = int(rng.integers(40, 88))
    x, y = (int(rng.integers(lo, hi)), across) if where in ("left", "right") else (across, int(rng.integers(lo, hi)))
    t = (x, y, int(rng.integers(0, spp)), int(rng.integers(0, spp)))
    ray = sample_ray(W, H, spp, t[0], t[1], t[2], t[3], EYE, prec)
    d = np.asarray(ray[3:], dtype=np.float64)
    axis, k = ((0.0, 1.0, 0.0), 0) if where in ("left", "right") else ((1.0, 0.0, 0.0), 1)
    side = _unit(np.cross(d, axis))
    if (side[k] > 0) != (where in ("right", "top")):
        side = -side
    q = 2.0 ** -18 * float(rng.choice([0.25, 0.5, 0.9, 0.99, 1.01, 1.1, 2.0, 4.0]))   # (|v| - r) / |v|: both sides of the cut-off
    vlen = float(rng.uniform(2.0, 6.0))
    ang = np.arccos(1.0 - q)                            # the tangent cone's half-angle is pi/2 - ang for r = |v| (1 - q)
    cen = _unit(np.cos(ang) * side + np.sin(ang) * d)   # the centre's direction: at pi/2 - ang from the ray
    c = _round(np.asarray(ray[:3]) + vlen * cen, prec)
    flip = tune(lambda x: _finite(prec, ray)(c + [x]), clearance(c, ray), prec, hi_limit=vlen)
    if flip is None:
        return None
    it = Item(c + [0.0])
    cs = _case("P1c", prec, spp, t, "primary", ray, [it], _offset(idx), flip, lambda x: _finite(prec, ray)(c + [x]),
               note="(|v|-r)/|v|=%.3g*2^-18" % (q * 2 ** 18))
    return (t, [it], [cs], [ray])


def _screen(blocks, prec):
    """Drops blocks whose items another block's target rays could hit (float64 geometry, the sphere widened by the reference's rounding
    band): each case must be decided by its own block alone.  Greedy, in order."""
    kept = []
    for blk in blocks:
        t, objs, cases, rays = blk
        mine = [o for o in _walk(objs) if isinstance(o, Item)]
        ok = True
        for other in kept:
            theirs = [o for o in _walk(other[1]) if isinstance(o, Item)]
            if any(_near(ry, o.sphere, prec) for ry in rays for o in theirs) or any(_near(ry, o.sphere, prec) for ry in other[3] for o in mine):
                ok = False
                break
        if ok:
            kept.append(blk)
    return kept


def _walk(objs):
    for o in objs:
        yield o
        if isinstance(o, Group):
            yield from _walk(o.children)


def _near(ray, sphere, prec, margin=1.05):
    """Could the reference's test of `sphere` return a finite distance for `ray`?  Its disc = b*b - vv + rr is rounded at the scale of vv
    (a few u vv, u = the unit roundoff): far from the origin a tiny sphere is "hit" well outside its radius.  Widened by 16 u vv + 5 %."""
    o, d = np.asarray(ray[:3]), np.asarray(ray[3:])
    v = np.asarray(sphere[:3]) - o
    b, vv = v @ d, v @ v
    u = 2.0 ** -24 if prec == oracle.F32 else 2.0 ** -53
    reff2 = (sphere[3] * margin) ** 2 + 16.0 * u * vv + 1e-30
    disc = b * b - vv + reff2
    return disc >= 0 and b + np.sqrt(disc) >= 0


@functools.lru_cache(maxsize=None)
def scene(family, prec, spp, seed=0):
    """The family's scene at one precision and sample count (deterministic: seeded by its parameters)."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), prec, spp])
    if family == "P1c":
        # four cut-off spheres (the frame's edges) and, in the middle of the frame that they leave alone, ordinary P1 grazes
        edges = [b for b in (_cutoff_block(prec, spp, rng, i, e) for i, e in enumerate(("left", "right", "top", "bottom"))) if b is not None]
        more = [b for b in _blocks("P1", prec, spp, rng) if 32 < b[0][0] < 96 and 32 < b[0][1] < 96]
        for b in more:
            for c in b[2]:
                c.family = "P1c"
        blocks = edges + _screen(more, prec)
    else:
        blocks = _screen(_blocks(family, prec, spp, rng), prec)
    fused = family == "O"
    if fused:
        # the root is followed by an item at its centre too (behind the eye: nothing sees it), so every bound is
        root = Group((0.0, 0.0, -30.0, 60.0), [Item((0.0, 0.0, -30.0, 0.25))])
    else:
        root = Group((0.0, 0.0, 3.0, 40.0))
    for b in blocks:
        root.children.extend(b[1])
    items, bounds, ranges, where = _flatten(root)
    cases = []
    for b in blocks:
        for c in b[2]:
            c.nodes = [where[id(o)] for o in c._objs]
            cases.append(c)
    return EdgeScene(family, prec, spp, items, bounds, ranges, cases)


def all_scenes(families=FAMILIES, precs=PRECS, spps=SPPS):
    return [scene(f, p, s) for f in families for p in precs for s in spps]


def pixel_result(osc, case, w=W, h=H, spp=None, mode=oracle.MODE_HIERARCHY | oracle.MODE_ANYHIT_EXIT):
    """The oracle's bytes and counters for the case's target pixel."""
    x, y = case.pixel
    px, st = osc.render_region(w, h, spp or case.spp, x, y + 1, x + 1, y, mode)
    return px.tobytes(), tuple(st[k] for k in ("primary", "hits", "shadow", "occluded", "sphere_tests", "bound_tests"))
