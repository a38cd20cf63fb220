"""The edge-case scenes of tests/edge_scenes.py checked on the CPU: every case sits where the reference's own verdict flips, every case
changes its target pixel when its node moves across the flip, and the oracle's sphere test (at f32 and, for the first time independently
of the oracle itself, f64) agrees with exact arithmetic wherever the exact answer is clear of the rounding band."""
import mpmath
import numpy as np
import pytest

import oracle
from tests import edge_scenes as es

PREC_IDS = {oracle.F32: "f32", oracle.F64: "f64"}
MIN_CASES = 100


_verdict = es.verdict


@pytest.mark.parametrize("prec", es.PRECS, ids=PREC_IDS.get)
@pytest.mark.parametrize("family", es.FAMILIES)
def test_every_case_sits_on_the_references_flip(family, prec):
    n = 0
    offsets = set()
    for spp in es.SPPS:
        sc = es.scene(family, prec, spp)
        for c in sc.cases:
            assert es.node_sphere(sc, c, c.value) == [float(x) for x in (sc.items if c.nodes[0][0] == "items" else sc.bounds)[c.nodes[0][1]]], c
            # the flip: HIT / ENTER from `flip` on, not one ulp below it; the case itself on the side its offset says
            assert _verdict(sc, c, c.flip) and not _verdict(sc, c, es.step_ulps(c.flip, -1, prec)), c
            assert _verdict(sc, c, c.value) == c.outcome == (c.offset >= 0), c
            assert _verdict(sc, c, c.other) != c.outcome and abs(es._bits(c.other, prec) - es._bits(c.value, prec)) <= es.K + 1, c
            assert -es.K <= c.offset <= es.K
            offsets.add(c.offset)
            n += 1
    assert offsets == set(range(-es.K, es.K + 1))
    assert n >= MIN_CASES, "%s %s: %d cases" % (family, PREC_IDS[prec], n)


def test_families_cover_their_sub_cases():
    # P1c: the cut-off on both sides; O: the own sphere smaller than, bit-equal to and larger than its bound, against primary and shadow rays;
    # P3: b - best from a few ulps of best up; S1: occluders from just past the origin to across the scene; exact zero direction components
    for prec in es.PRECS:
        cut = [float(c.note.split("=")[1].split("*")[0]) for spp in es.SPPS for c in es.scene("P1c", prec, spp).cases if c.note]
        assert len(cut) >= 8 and min(cut) < 1.0 < max(cut), cut
        own = {(c.kind, c.note) for spp in es.SPPS for c in es.scene("O", prec, spp).cases}
        assert own == {(k, n) for k in ("primary", "shadow") for n in ("own<bound", "own==bound", "own>bound")}, own
        gaps = [float(c.note.split("=")[1]) / c.best for spp in es.SPPS for c in es.scene("P3", prec, spp).cases]
        assert min(gaps) < 1e-6 and max(gaps) > 1e-3
        s1 = [c for spp in es.SPPS for c in es.scene("S1", prec, spp).cases]
        far = [float(c.note.split("=")[1]) for c in s1 if c.note.startswith("t=")]
        assert min(far) < 10 ** (es._near_log(prec) + 0.3) and max(far) > 1.0
        # occluders beside the origin, a = (c - o) . l of either sign from 1e-7 to 3e-4 (the bounds' a0 is ~1e-5 here) ...
        beside = [float(c.note.split("=")[1]) for c in s1 if c.note.startswith("a=")]
        assert len(beside) >= 60 and min(beside) < -1e-4 and max(beside) > 1e-4 and min(abs(x) for x in beside) < 1e-6, sorted(beside)
        # ... and just behind it, the HIT side with the origin inside the occluder
        behind = [c for c in s1 if c.note.startswith("behind=")]
        inside = [c for c in behind if c.offset >= 0 and np.sum((np.array(es.node_sphere(es.scene("S1", prec, c.spp), c, c.value)[:3]) -
                                                                 c.ray[:3]) ** 2) < c.value ** 2]
        assert len(behind) >= 60 and len(inside) >= 20, (len(behind), len(inside))
        # T: the terminator on both sides, the target's receiver nudged along a centre coordinate
        t = [c for spp in es.SPPS for c in es.scene("T", prec, spp).cases]
        assert {c.offset >= 0 for c in t} == {True, False} and {c.sense for c in t} <= {True, False}
        zero = [c for spp in es.SPPS for c in es.scene("P1", prec, spp).cases if c.ray[3] == 0.0 or c.ray[4] == 0.0]
        assert len(zero) >= 6


@pytest.mark.parametrize("spp", es.SPPS)
@pytest.mark.parametrize("prec", es.PRECS, ids=PREC_IDS.get)
@pytest.mark.parametrize("family", es.FAMILIES)
def test_every_case_is_observable_in_its_final_scene(family, prec, spp):
    # The case's node moved to the other side of its flip, the scene rebuilt: the oracle's bytes or counters for the target pixel change.
    # This also proves the restated rays (sample and shadow) and the node's place in the hierarchy: a case whose node the walk never tests
    # for that ray, or tests against another best, changes nothing and fails here.
    sc = es.scene(family, prec, spp)
    base = sc.oracle()
    for c in sc.cases:
        before = es.pixel_result(base, c)
        after = es.pixel_result(sc.oracle(*sc.moved(c, c.other)), c)
        assert before != after, (sc.name, c.pixel, c.sample, c.kind, c.offset, c.note)
        # ... and one more ulp away on its own side the walk makes the same tests with the same outcome (the shade may move a little)
        again = es.step_ulps(c.value, 1 if c.offset >= 0 else -1, prec)
        assert es.pixel_result(sc.oracle(*sc.moved(c, again)), c)[1] == before[1], (sc.name, c.pixel, c.offset)


def _pairs(prec, rng):
    """(sphere, ray) pairs: the families' target rays against their nodes' centres with radii well away from the flip, and random ones."""
    out = []
    for fam in ("P1", "P3", "S1", "O"):
        for spp in es.SPPS:
            sc = es.scene(fam, prec, spp)
            for c in sc.cases[::3]:
                for f in (0.25, 0.9, 1.1, 4.0):
                    out.append((es.node_sphere(sc, c, float(es.REAL[prec](c.value * f))), c.ray))
    R = es.REAL[prec]
    for _ in range(1500):
        o = rng.uniform(-5, 5, 3)
        d = rng.normal(size=3)
        d = oracle.vec_normalized(d, prec)[0]
        c = o + d * rng.uniform(-3, 10) + rng.normal(size=3) * rng.uniform(0, 2)
        r = rng.uniform(0.01, 3.0)
        out.append(([float(R(x)) for x in list(c) + [r]], np.concatenate([np.asarray(o, dtype=R), d]).astype(np.float64)))
    return out


@pytest.mark.parametrize("prec", es.PRECS, ids=PREC_IDS.get)
def test_oracle_sphere_test_matches_exact_arithmetic(prec):
    """oracle.sphere_distance_from_ray against the same formula evaluated exactly (mpmath, 240 bits) on the same REAL inputs.

    Error bound, u = 2^-24 (f32) or 2^-53 (f64), K = |b| + |v| + r (exact b, v = c - o):
      v = c - o: one rounding per component; b = v . d: two products... -> |b^ - b| <= 4.01 u |v| |d| <= 4.02 u |v|  (|d| <= 1 + 2u)
      vv^ = (v . v)^: |vv^ - vv| <= 5.01 u vv;  rr^ = RN(r r): u rr
      disc^ = RN(RN(b^ b^ - vv^) + rr^): |disc^ - disc| <= u (b^2 + 8.02 |b||v| + 5.01 vv + |b^2 - vv| + rr + |disc|) (1 + 8u)
                                                       <= 8.1 u K^2 =: E
    so the hit / miss verdict (the sign of disc) agrees wherever |disc| > E.  With s = sqrt(disc) >= K / 8:
      |s^ - s| <= E / s + u s^ <= 64.8 u K + 1.01 u K, and t1^ = RN(b^ - s^) (or t2^): |t^ - t| <= 4.02 u K + 65.9 u K + 2.02 u K < 80 u K,
    the bound asserted below (and the branch t1 > 0 / t2 < 0 agrees wherever the exact t1 and t2 are further than that from 0).  Where
    E < disc but s < K / 8: |s^ - s| <= E / s + u K <= 2.7 sqrt(u) K + u K, which still fixes INF versus finite wherever t2 is clear of it.
    """
    rng = np.random.default_rng(71 + prec)
    u = 2.0 ** -24 if prec == oracle.F32 else 2.0 ** -53
    checked = dist_checked = 0
    with mpmath.workprec(240):
        for sph, ray in _pairs(prec, rng):
            b, vv, rr, disc = es.exact_terms(sph, ray)
            Kf = float(abs(b) + mpmath.sqrt(vv) + abs(mpmath.mpf(sph[3])))
            E = 8.1 * u * Kf * Kf
            got = oracle.sphere_distance_from_ray(sph, ray, prec)
            if abs(float(disc)) <= E:
                continue                                        # in the rounding band: the reference may go either way
            if disc < 0:
                assert got == float("inf"), (sph, ray)
                checked += 1
                continue
            s = mpmath.sqrt(disc)
            band = 80 * u * Kf if float(s) >= Kf / 8 else 2.8 * np.sqrt(u) * Kf + 7 * u * Kf
            t1, t2 = float(b - s), float(b + s)
            if abs(t2) <= band or abs(t1) <= band:
                continue
            exact = es.exact_distance(sph, ray)
            if t2 < 0:
                assert got == float("inf"), (sph, ray)
            else:
                assert np.isfinite(got), (sph, ray)
                if float(s) >= Kf / 8:
                    assert abs(got - float(exact)) <= 80 * u * Kf, (sph, ray, got, float(exact))
                    dist_checked += 1
            checked += 1
    assert checked >= 2000 and dist_checked >= 300, (checked, dist_checked)
