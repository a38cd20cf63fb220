"""Fixtures of the tight-stream tests (tests/test_tight_host.py, tests/test_gpu_tight.py): small f32 scenes in which single bounds must keep
the sphere they were given (rust-tracer_amd/csrc/rt_tight.hpp, rules (b) and (c)) while others of the same scene get a tight one."""
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
