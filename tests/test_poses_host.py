"""The inputs of tests/test_gpu_poses.py, checked without a GPU: under every light, from every eye and at every placement of
tests/posed_scenes.py the oracle's frame still shows the scene, casts shadow rays and has some of them blocked -- with the oracle and numpy
alone, so that no GPU comparison can pass on a frame that shows nothing.  These are conditions on the inputs, found to hold on the oracle
for all 14 lights x 6 eyes x 2 scenes at both placements and precisions (672 frames of 128 x 96 at spp 1): a pose that misses one is
answered by another pose, never by another floor."""
import numpy as np
import pytest

import oracle
import rust_tracer_amd as rta
from tests import posed_scenes as ps
from tests import scaled_scenes as ss
from tests.test_gpu_query import PREC, REAL

HITS, SHADOW, OCCLUDED_PER_NAME = 150, 40, 10


def test_the_pose_list_is_the_star_and_every_case_is_distinct():
    assert list(ps.LIGHTS) == ["home", "-y", "+y", "+x", "-x", "+z", "-z", "up", "side_up", "toward_eye_up", "xy_tie", "xyz_tie", "near_axis",
                               "graze_z"]
    assert list(ps.EYES) == ["home", "left", "high", "low_right", "far", "inside_root"]
    assert ps.LIGHTS["home"] == ss.LIGHT and ps.EYES["home"] == ss.EYE
    poses = set(ps.POSES)
    assert len(poses) == len(ps.POSES) == 2 * 14 + 4 * 4
    assert all((l, e) in poses for l in ps.LIGHTS for e in ("home", "left"))
    assert all((l, e) in poses for l in ("home", "+y", "-x", "up") for e in ps.EYES)
    assert set(ps.SPECIAL_POSES) == {(l, e) for l in ("home", "+y", "up") for e in ("centre", "inside_item")}
    assert len(set(ps.CASES)) == len(ps.CASES) and len({ps.case_id(p) for p in ps.CASES}) == len(ps.CASES)
    # every pose on both scenes, at the identity and moved, in f32 and f64; the special eyes on the concentric scene only
    for precision in (rta.RT_F32, rta.RT_F64):
        for placement in ("id", "moved"):
            for scene in ps.SCENES:
                for light, eye in ps.POSES:
                    assert (scene, light, eye, placement, precision, ps.SHAPE) in ps.CASES
            for pose in ps.SPECIAL_POSES:
                assert ("concentric",) + pose + (placement, precision, ps.SHAPE) in ps.CASES
                assert ("nested",) + pose + (placement, precision, ps.SHAPE) not in ps.CASES
        # the ragged sample-packed shapes and the scaled placements (under lights that are not the home light) are there in both precisions
        for shape in ps.RAGGED_SHAPES:
            assert sum(1 for p in ps.CASES if p[4] == precision and p[5] == shape and p[3] == "moved") >= 4
        scaled = [p for p in ps.CASES if p[4] == precision and p[3].startswith("x")]
        assert {p[3] for p in scaled} == {"x1e-10", "x1e+06"} and all(p[1] != "home" for p in scaled) and {p[0] for p in scaled} == set(ps.SCENES)
    assert ps.MOVES[rta.RT_F32] == (3000.0, -5000.0, 7000.0) and ps.MOVES[rta.RT_F64] == (3e9, -5e9, 7e9)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_every_normalised_light_is_one_the_library_accepts(precision):
    # rt_scene_create wants a light whose squared length is within 2e-3 of 1; rta.normalized is the reference's own normalisation
    items, bounds, ranges = ps.base_scene("nested")
    for name, raw in ps.LIGHTS.items():
        l = rta.normalized(raw, precision)
        assert l.dtype == REAL[precision] and np.isfinite(l).all(), name
        l2 = float(np.sum(l.astype(np.float64) ** 2))
        assert abs(l2 - 1.0) <= 2e-3, (name, l2)
        assert abs(l2 - 1.0) <= 8 * np.finfo(REAL[precision]).eps, (name, l2)               # ... by far
        s = rta.Scene(items, l, ps.EYES["home"], bounds, ranges, precision)                 # the host side takes it as it is
        assert np.array_equal(s.directional_light, l)
        # the direction survives: every component keeps its sign, an exact zero stays an exact zero
        assert np.array_equal(np.sign(l), np.sign(np.asarray(raw))), name


def test_the_lights_named_as_ties_are_ties_after_normalisation():
    # filter_constants (csrc/rt_capi_scene.hpp) picks the axis of the light's smallest magnitude by a strict `<`: what it meets in these
    # lights must be exactly equal magnitudes, not nearly equal ones
    for precision in (rta.RT_F32, rta.RT_F64):
        mag = {name: np.abs(rta.normalized(raw, precision)) for name, raw in ps.LIGHTS.items()}
        for name in ps.AXIS_LIGHTS:                              # two exact zeros: the smallest magnitude is a two-way tie
            m = np.sort(mag[name])
            assert m[0] == 0.0 and m[1] == 0.0 and m[2] == 1.0, (name, m)
        m = mag["xyz_tie"]
        assert m[0] == m[1] == m[2] > 0.5, m                     # the smallest magnitude is a three-way tie
        m = mag["xy_tie"]
        assert m[0] == m[1] > m[2] > 0.0, m                      # the two LARGEST are equal; the smallest (z) stands alone
        # ... and the lights that are nobody's tie have three distinct magnitudes, or (near_axis) a tie between its two tiny components
        for name in ("home", "up", "side_up", "toward_eye_up", "graze_z"):
            assert len(set(mag[name].tolist())) == 3, (name, mag[name])
        m = mag["near_axis"]
        assert m[0] == m[2] and 0.0 < m[0] < 2e-4 and m[1] > 0.999, m


def test_the_oracle_normalises_the_light_it_is_given():
    # why the package's scene gets rta.normalized(light) and the oracle the raw vector -- and why a light of another length (tests/test_gpu_seam.py,
    # the edges of the accepted length) has no oracle frame to be compared with: the oracle's scene never holds such a light
    items, bounds, ranges = ps.base_scene("concentric")
    for raw in ((-1.0, -3.0, 2.0), (0.0, 1.0, 0.0), (1.0, -1.0, 0.25)):
        unit = rta.normalized(raw, rta.RT_F32)
        for scale in (1.0 - 1.9e-3, 1.0 + 1.9e-3):
            off = (unit.astype(np.float64) * np.sqrt(scale)).astype(np.float32)
            assert abs(float(np.sum(off.astype(np.float64) ** 2)) - 1.0) > 1.8e-3
            held, _ = oracle.Scene.from_ranges(items, bounds, ranges, tuple(float(v) for v in off), ps.EYES["home"], oracle.F32).light_eye()
            assert abs(float(np.sum(held.astype(np.float64) ** 2)) - 1.0) < 1e-6 and not np.array_equal(held, off)
        held, _ = oracle.Scene.from_ranges(items, bounds, ranges, raw, ps.EYES["home"], oracle.F32).light_eye()
        assert np.array_equal(held, unit)                        # both sides normalise the raw vector to the same bits


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_every_placed_scene_keeps_its_radii_and_the_special_eyes_their_place(precision):
    R = REAL[precision]
    seen = set()
    for p in ps.CASES:
        if p[4] != precision or p[:4] in seen:
            continue
        seen.add(p[:4])
        c = ps.case(*p)
        for a in (c.scene.items, c.scene.bounds):
            assert a.dtype == R and np.isfinite(a).all() and (a[:, 3] > 0).all() and (a[:, 3] * a[:, 3] > 0).all(), ps.case_id(p)
            assert np.abs(a).max() <= 1e15
        assert np.array_equal(c.scene.items.astype(np.float64), c.items) and np.array_equal(c.scene.eye.astype(np.float64), np.array(c.eye))
        assert len(np.unique(c.scene.items, axis=0)) == len(c.scene.items), ps.case_id(p)
        if p[2] == "centre":
            # bit-equal to the first item's centre and to the root bound's: v = 0, vv = 0 for both
            assert np.array_equal(c.scene.eye, c.scene.items[0, :3]) and np.array_equal(c.scene.eye, c.scene.bounds[0, :3]), ps.case_id(p)
        if p[2] == "inside_item":
            it = c.scene.items[ps.inside_item_index()]
            v = it[:3] - c.scene.eye                                   # primitive.rs:56-58 in the scene's REAL
            vv, rr = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], it[3] * it[3]
            assert R(0) < vv < rr, (ps.case_id(p), vv, rr)                 # inside, and not at the centre
            assert 0.2 * rr < vv < 0.3 * rr, (ps.case_id(p), vv / rr)      # half a radius out
            # "not clearly outside" (primary_filter_threshold, csrc/rt_skip.hpp): vv - rr < 64 eps (vv + rr), so T = -inf
            assert not (float(vv) - float(rr) >= 64.0 * 2.0 ** -24 * (float(vv) + float(rr)))
    assert len(seen) >= 2 * 2 * len(ps.POSES) + 2 * len(ps.SPECIAL_POSES)


@pytest.mark.parametrize("param", ps.CASES, ids=ps.case_id)
def test_a_posed_frame_shows_the_scene_and_casts_shadow_rays(param):
    scene, light, eye, placement, precision, (w, h, spp) = param
    _, st = ps.frame(param)
    assert st["primary"] == w * h * spp * spp
    if eye in ps.SPECIAL_EYES:
        # from inside an item every ray hits (the item itself, at the latest).  Under the home light every such hit is on a face turned
        # away from the light as the reference sees it: the ambient exit, the named exception; under +y and up shadow rays are cast
        assert st["hits"] == st["primary"], st
        if light == "home":
            assert st["hits"] - st["shadow"] >= HITS, st
        else:
            assert st["shadow"] >= SHADOW, st
        return
    assert st["hits"] >= HITS, st
    if light == ps.AMBIENT_LIGHT:
        assert st["hits"] - st["shadow"] >= HITS, st                   # the ambient exit
    else:
        assert st["shadow"] >= SHADOW, st


def test_the_eye_at_a_centre_sees_that_item_in_every_pixel():
    items, bounds, ranges = ps.base_scene("concentric")
    o = oracle.Scene.from_ranges(items, bounds, ranges, ps.LIGHTS["home"], ps.eye_of("centre"), oracle.F32)
    _, st, _ = o.render(96, 72, 1, 1, ps.HIER_EXIT)
    assert st["hits"] == 96 * 72 == 6912


@pytest.mark.parametrize("by", [1, 2], ids=["light", "eye"])
def test_shadow_rays_are_blocked_under_every_light_and_from_every_eye(by):
    # occluded >= 1 does not hold frame by frame (the nested scene from `low_right` and `inside_root` under `up`, from `inside_root`
    # under `xy_tie`): asserted over the frames of each light, and over the frames of each eye.  Under -z hardly a shadow ray is cast.
    total = {}
    for p in ps.CASES:
        if p[1] != ps.AMBIENT_LIGHT:
            total[p[by]] = total.get(p[by], 0) + ps.frame(p)[1]["occluded"]
    names = (set(ps.LIGHTS) - {ps.AMBIENT_LIGHT}) if by == 1 else set(ps.EYES) | set(ps.SPECIAL_EYES)
    assert set(total) == names
    for name, n in total.items():
        assert n >= OCCLUDED_PER_NAME, (name, n)
    # ... and at the identity placement alone (moved, the push-out of a shadow ray's origin is below an ulp of a coordinate and many a ray
    # hits the sphere it starts on: blocked rays are plentiful there for another reason).  Not `centre`: from the innermost sphere's
    # centre every shadow ray starts on that sphere, and at the identity nothing blocks one.
    home = {}
    for p in ps.CASES:
        if p[1] != ps.AMBIENT_LIGHT and p[3] == "id" and p[2] != "centre":
            home[p[by]] = home.get(p[by], 0) + ps.frame(p)[1]["occluded"]
    assert set(home) == names - {"centre"} and min(home.values()) >= OCCLUDED_PER_NAME, home


def test_moving_the_scene_changes_the_frame_but_not_what_it_shows():
    # what the moved placement is for: the frame is the same picture, with the roundings of coordinates a thousand (f32) or a billion
    # (f64 against 2^-52) times coarser -- different bytes, about the same counts
    for precision in (rta.RT_F32, rta.RT_F64):
        differ = 0
        for scene in ps.SCENES:
            a, sa = ps.frame((scene, "up", "left", "id", precision, ps.SHAPE))
            b, sb = ps.frame((scene, "up", "left", "moved", precision, ps.SHAPE))
            differ += int(not np.array_equal(a, b))
            assert abs(sa["hits"] - sb["hits"]) <= 0.05 * sa["hits"], (sa, sb)
        assert differ
