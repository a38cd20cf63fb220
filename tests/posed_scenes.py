"""Frames away from the home pose: the frame tests' two scenes under lights of every kind (axis lights, lights that point up, ties between
components), eyes off the axis, far away, inside the root bound, at and inside an item, and with scene and eye moved away from the origin
(tests/test_poses_host.py checks the inputs on the CPU, tests/test_gpu_poses.py renders them on the GPU).  numpy, the oracle and the host
side of the package only.

LIGHTS / EYES: name -> vector.  A light is given un-normalised: the package's scene takes rta.normalized(light, precision), the oracle the
raw vector and normalises it itself (util.scene_pair_ranges).  The camera looks along +z from the eye, so every eye stays where the scene
(about 3 units across, around the origin) is in view.  SPECIAL_EYES are computed from the concentric scene: `centre` IS its first item's
centre -- which is also the root bound's -- so v = c - eye = 0 exactly for both, at every placement; `inside_item` lies half a radius
from the centre of INSIDE_ITEM, inside it, so that node's primary threshold T is -inf ("not clearly outside").

POSES: a star, not the cross product -- every light at the eyes `home` and `left`, every eye at the lights `home`, `+y`, `-x` and `up`;
SPECIAL_POSES the special eyes at `home`, `+y` and `up`, on the concentric scene only.

placements(precision): `id`; `moved`, the translation of tests/scaled_scenes.py (+(3000, -5000, 7000) in f32, +(3e9, -5e9, 7e9) in f64:
c - eye cancels and the centroid m0 is far from 0); and the scales `x1e-10` and `x1e+06` for SCALED_POSES, whose lights are not the
home light.  Items, bounds and eye are placed together and rounded once to the scene's REAL (scaled_scenes._placement).

CASES: (scene, light, eye, placement, precision, (w, h, spp)) -- every pose on both scenes at `id` and `moved` in f32 and f64 at
128 x 96 spp 1; RAGGED_POSES once more at 75 x 50 spp 2 and 40 x 33 spp 4 (partly filled blocks, the sample-packed passes); SCALED_POSES.
case(*params) -> Case, made once per process; frame(params, mode) -> the oracle's (image, stats) of that case, computed once."""
import functools
import os

import numpy as np

import oracle
import rust_tracer_amd as rta
from tests import scaled_scenes as ss
from tests import util
from tests.test_gpu_query import PREC, REAL

HIER_EXIT = oracle.MODE_HIERARCHY | oracle.MODE_ANYHIT_EXIT

SCENES = {"nested": (31, False), "concentric": (32, True)}        # plain-stream loops / fused loops

LIGHTS = {
    "home": (-1.0, -3.0, 2.0),
    "-y": (0.0, -1.0, 0.0), "+y": (0.0, 1.0, 0.0), "+x": (1.0, 0.0, 0.0), "-x": (-1.0, 0.0, 0.0),
    "+z": (0.0, 0.0, 1.0),                       # along the view axis: every visible face is lit
    "-z": (0.0, 0.0, -1.0),                      # against it: almost every hit takes the ambient exit
    "up": (1.0, 3.0, -2.0), "side_up": (-2.0, 0.5, 0.3), "toward_eye_up": (0.3, 1.0, -0.2),
    "xy_tie": (1.0, -1.0, 0.25),                 # two equal magnitudes (the largest two)
    "xyz_tie": (-1.0, -1.0, 1.0),                # three equal magnitudes: the smallest is a three-way tie
    "near_axis": (1e-4, -1.0, -1e-4),            # e1's normalisation with one tiny component
    "graze_z": (0.02, -0.03, 1.0),               # almost along the view axis
}
AXIS_LIGHTS = ("-y", "+y", "+x", "-x", "+z", "-z")                # two exact zeros: the smallest magnitude is a two-way tie
AMBIENT_LIGHT = "-z"

EYES = {
    "home": (0.07, -0.12, -3.1),
    "left": (-1.3, 0.3, -3.4), "high": (0.4, 1.3, -3.6), "low_right": (1.1, -0.9, -3.0),
    "far": (0.5, -0.4, -12.0),                   # the scene covers a few hundred pixels
    "inside_root": (0.1, 0.1, -1.0),
}
SPECIAL_EYES = ("centre", "inside_item")
STAR_EYES, STAR_LIGHTS = ("home", "left"), ("home", "+y", "-x", "up")

POSES = tuple([(l, e) for e in STAR_EYES for l in LIGHTS] + [(l, e) for l in STAR_LIGHTS for e in EYES if e not in STAR_EYES])
SPECIAL_POSES = tuple((l, e) for e in SPECIAL_EYES for l in ("home", "+y", "up"))
RAGGED_POSES = (("+y", "left"), ("up", "home"), ("xyz_tie", "left"), ("-x", "low_right"))
RAGGED_SHAPES = ((75, 50, 2), (40, 33, 4))
SCALED_POSES = (("concentric", "+y", "home", "x1e-10"), ("nested", "-x", "home", "x1e-10"),
                ("concentric", "xyz_tie", "home", "x1e+06"), ("nested", "up", "left", "x1e+06"))
SHAPE = (128, 96, 1)
MOVES = {rta.RT_F32: (3000.0, -5000.0, 7000.0), rta.RT_F64: (3e9, -5e9, 7e9)}


def placements(precision):
    R = REAL[precision]
    assert 1e-10 in ss.SCALES and 1e6 in ss.SCALES
    return {"id": ss._placement(R), "moved": ss._placement(R, shift=MOVES[precision]),
            "x1e-10": ss._placement(R, scale=1e-10), "x1e+06": ss._placement(R, scale=1e6)}


@functools.lru_cache(maxsize=None)
def base_scene(name):
    seed, concentric = SCENES[name]
    return util.random_nested_scene(seed, depth=3, fan=3, leaf_items=2, concentric=concentric)


def inside_item_index():
    """The item `inside_item` sits in: the concentric scene's first sub-group's own sphere (at the centre of that group's bound)."""
    _, _, ranges = base_scene("concentric")
    return int(ranges[1][0])


def eye_of(name):
    """The unplaced eye, float64."""
    if name in EYES:
        return EYES[name]
    items, _, _ = base_scene("concentric")
    if name == "centre":
        return tuple(float(v) for v in items[0, :3])
    assert name == "inside_item"
    c = items[inside_item_index()]
    # half a radius from the centre (|(0.6, -0.8, 0)| = 1): inside at every placement, the f32 rounding of the sum moves it by 1e-7 radii
    return (float(c[0] + 0.3 * c[3]), float(c[1] - 0.4 * c[3]), float(c[2]))


def _cases():
    out = []
    for precision in (rta.RT_F32, rta.RT_F64):
        for placement in ("id", "moved"):
            for scene in SCENES:
                for light, eye in POSES + (SPECIAL_POSES if scene == "concentric" else ()):
                    out.append((scene, light, eye, placement, precision, SHAPE))
                for light, eye in RAGGED_POSES:
                    out.extend((scene, light, eye, placement, precision, shape) for shape in RAGGED_SHAPES)
        out.extend((scene, light, eye, placement, precision, SHAPE) for scene, light, eye, placement in SCALED_POSES)
    return tuple(out)


CASES = _cases()


def case_id(param):
    scene, light, eye, placement, precision, (w, h, spp) = param
    return "%s-%s-%s-%s-%s-%dx%dx%d" % (scene, light, eye, placement, "f32" if precision == rta.RT_F32 else "f64", w, h, spp)


class Case:
    """One pose of one scene at one placement: .param, .scene (rta.Scene, host side), .oracle, .light (the normalised light the package's
    scene holds), the placed float64 .items / .bounds / .eye, .ranges and .shape = (w, h, spp)."""


@functools.lru_cache(maxsize=None)
def _posed(scene, light, eye, placement, precision):
    items0, bounds0, ranges = base_scene(scene)
    c = Case()
    c.items, c.bounds, c.eye = placements(precision)[placement](items0, bounds0, eye_of(eye))
    c.ranges = ranges
    c.scene, c.oracle = util.scene_pair_ranges(c.items, c.bounds, ranges, precision, light=LIGHTS[light], eye=c.eye)
    c.light = c.scene.directional_light
    return c


def case(scene, light, eye, placement, precision, shape):
    """The Case of one element of CASES (cases that differ in the frame's shape only share their scenes)."""
    p = _posed(scene, light, eye, placement, precision)
    c = Case()
    c.__dict__.update(p.__dict__)
    c.param, c.shape = (scene, light, eye, placement, precision, shape), tuple(shape)
    return c


@functools.lru_cache(maxsize=None)
def frame(param, mode=HIER_EXIT):
    """(image uint8[h, w, 4], stats dict) of the oracle for one element of CASES; nothing in it is written to."""
    c = case(*param)
    w, h, spp = c.shape
    img, st, _ = c.oracle.render(w, h, spp, os.cpu_count() or 1, mode)
    img.setflags(write=False)
    return img, dict(st)


def regions(shape):
    return [tuple(r) for r in rta.buckets(rta.RenderOptions(*shape))]
