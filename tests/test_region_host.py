"""Region overlap lists (rt_overlap_regions / rt_overlap_regions_device, csrc/rt_region.hpp) without a GPU: the ABI, the
argument and domain checks made before any device is touched, the residency of the kernel's flavours read back from the code object,
rta.region_gaps -- the metric's definition in numpy -- against a scalar restatement and against the geometry away from unit scale, the
one-lane walk and its sectioned form restated in Python (equal lists for every number of sections, equal counters at one), the walk
against brute force where nothing grazes, rta.camera_planes against the camera's own sample rays, rta.box_planes against rta.box_gaps,
rta.region_sections, and the calls the Python wrapper makes.  (The one refusal that needs a device -- a buffer in device memory -- is
held by tests/test_gpu_region.py, which also holds the kernels to the walkers of this file.)"""
import ctypes
import os
import re

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from rust_tracer_amd.scene import DeviceScene
from tests import scaled_scenes as ss
from tests.test_gpu_multihit import node_stream
from tests.test_gpu_overlap import COUNTERS, Walker as OverlapWalker, five_scenes, median_radius, scale_of
from tests.test_gpu_query import REAL, bits
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB
from tests.test_scales_contact_host import DENORMAL_SQUARES, higher
from tests.test_wrapper_calls_host import _Recorder, _device_scene, _is_stats, TOTAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_overlap_regions", "rt_overlap_regions_device")
BAD = capi.RT_ERR_INVALID_ARGUMENT
CASES = pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)
PRECISIONS = pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
MARGINS = (("0", lambda r: 0.0), ("r", lambda r: r), ("-r/4", lambda r: -0.25 * r), ("4r", lambda r: 4.0 * r))
ABSENT = (0.0, 0.0, 0.0, -np.inf)
SCENES = ("default_L3", "nested", "refit", "nested3", "clump")


# ---- the regions of the tests, and the two walkers ----

def unit_regions(n, seed=91):
    """float64[n, 6, 4] for a scene of unit size: per region a centre uniform in +-1.2, half-extents uniform in [0.02, 0.5] and a rotation,
    the Q of the QR factorisation of a normal 3 x 3 matrix.  Three of every four are rotated boxes; every fourth is a four-sided pyramid
    with its apex at the centre, opening along the rotation's third axis with tangents uniform in [0.1, 0.6], a near plane 0.05 behind
    the apex and one absent plane."""
    rng = np.random.default_rng(seed)
    P = np.zeros((n, 6, 4))
    for g in range(n):
        c, h = rng.uniform(-1.2, 1.2, 3), rng.uniform(0.02, 0.5, 3)
        A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        if g % 4 == 3:
            ta, tb = rng.uniform(0.1, 0.6, 2)
            for k, nn in enumerate((A[0] - ta * A[2], -A[0] - ta * A[2], A[1] - tb * A[2], -A[1] - tb * A[2])):
                nn = nn / np.linalg.norm(nn)
                P[g, k, :3], P[g, k, 3] = nn, -nn @ c
            P[g, 4, :3], P[g, 4, 3] = -A[2], A[2] @ c + 0.05
            P[g, 5] = ABSENT
        else:
            for k in range(3):
                P[g, 2 * k, :3], P[g, 2 * k, 3] = A[k], -(A[k] @ c) - h[k]
                P[g, 2 * k + 1, :3], P[g, 2 * k + 1, 3] = -A[k], (A[k] @ c) - h[k]
    return P


def regions_for(s, n=80, seed=91):
    """n regions, unit_regions scaled to the scene's extent (a power of two: the normals stay, every d scales exactly), in the scene's REAL."""
    P = unit_regions(n, seed)
    P[:, :, 3] *= scale_of(s)
    return np.ascontiguousarray(P.astype(REAL[s.precision]))


def carried_of(planes):
    return ~np.isnan(planes.reshape(len(planes), 24)).any(axis=1)


class Walker(OverlapWalker):
    """The definition of the region walk (include/rtrace_hip.h): tests/test_gpu_overlap.py's Walker -- one query at a time over
    node_stream(s) from node 0 -- with rta.region_gaps as the metric and "no NaN among the 24 reals" as "carried"."""

    def __init__(self, s, planes):
        self.R = R = REAL[s.precision]
        nodes = node_stream(s)
        self.bound = [x[1] for x in nodes]
        self.skip = [x[2] for x in nodes]
        self.item = [x[3] for x in nodes]
        self.node_of = {x[3]: k for k, x in enumerate(nodes) if not x[1]}
        self.queries = self.planes = p = np.asarray(planes, dtype=R)
        records = np.array([x[0] for x in nodes], dtype=np.float64).reshape(-1, 4).astype(R)         # (exact: they were REAL)
        self.gaps = [row.tolist() for row in rta.region_gaps(p, records)] if len(nodes) else [[] for _ in p]
        self.carried = carried_of(p)
        self.n_nodes = len(nodes)

    def sectioned(self, margin, J):
        """The same list made by J sections per region, as rt_region.hpp's lanes make it -> (items, gaps, offsets[n + 1], counters).
        Section j is the nodes [j N // J, (j + 1) N // J).  Its lane first DESCENDS from node 0 while i < s: a bound with skip > s is an
        ancestor of s -- tested and counted; culling continues behind it and ends the descent -- any other node is stepped over
        untested.  Then it walks to e as the one-lane walk does."""
        m = float(self.R(margin))
        n, N = len(self.planes), self.n_nodes
        J = max(1, min(int(J), max(N, 1)))
        bound, skip, item = self.bound, self.skip, self.item
        items, gaps, counts = [], [], np.zeros(n, np.uint64)
        tests_items = tests_bounds = 0
        for g in range(n):
            if not self.carried[g]:
                continue
            gap = self.gaps[g]
            for j in range(J):
                s, e = j * N // J, (j + 1) * N // J
                if s == e:
                    continue
                i = 0
                while i < s:
                    if bound[i] and skip[i] > s:
                        tests_bounds += 1
                        if gap[i] >= m:
                            i = skip[i]
                            break
                        i += 1
                    else:
                        i = skip[i]
                else:
                    assert i == s, (g, j, i, s)                              # a descent that does not leave early ends at exactly s
                while i < e:
                    d = gap[i]
                    if bound[i]:
                        tests_bounds += 1
                        i = skip[i] if d >= m else i + 1
                        continue
                    tests_items += 1
                    if not d >= m:
                        items.append(item[i])
                        gaps.append(d)
                        counts[g] += 1
                    i += 1
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        st = {c: 0 for c in COUNTERS}
        st.update(primary=int(self.carried.sum()), hits=int((counts > 0).sum()), sphere_tests=tests_items, bound_tests=tests_bounds,
                  tests_executed=tests_items + tests_bounds)
        return np.array(items, np.int32), np.array(gaps, self.R), offsets, st


def section_counts(n_nodes):
    return (1, 2, 3, 7, 64, 65, n_nodes - 1, n_nodes)


# ---- the ABI and the checks in front of the device ----

def test_both_libraries_export_the_region_entries_at_abi_5():
    assert capi.ABI_VERSION == 5
    assert set(ENTRIES) <= set(capi.SYMBOLS)
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert lib.rt_abi_version() == 5
        for name in ENTRIES:
            assert getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "rtrace_hip.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z_]+)\s*\(", header))
    assert set(ENTRIES) <= declared and declared == set(capi.SYMBOLS), declared ^ set(capi.SYMBOLS)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert getattr(capi.lib, name).argtypes, name
        assert re.search(r"\bfn %s\(" % name, integration), name
    assert len(capi.lib.rt_overlap_regions_device.argtypes) == len(capi.lib.rt_overlap_regions.argtypes) + 1 == 12
    for name in ("region_gaps", "box_planes", "camera_planes", "region_sections"):
        assert callable(getattr(rta, name)) and name in rta.__all__, name
    assert callable(DeviceScene.region_overlaps)


def _call(entry, scene, planes, n, margin, sections, capacity, items, gap, offsets, total):
    f = getattr(capi.lib, entry)
    args = (scene, planes, n, margin, sections, capacity, items, gap, offsets, total, None)
    return f(*args) if entry == "rt_overlap_regions" else f(*args, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check pointers, n, the margin, the capacity, alignment and n * sections before they use the device: a stand-in handle will do
    stand_in = ctypes.create_string_buffer(8192)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    words = (ctypes.c_uint64 * 128)()
    at = lambda k: ctypes.c_void_p(ctypes.addressof(words) + k)
    planes, items, gap, offsets, total = at(0), at(384), at(512), at(640), at(768)
    message = capi.lib.rt_last_error_message
    good = dict(scene=handle, planes=planes, n=1, margin=0.0, sections=0, capacity=4, items=items, gap=gap, offsets=offsets, total=total)
    call = lambda **kw: _call(entry, **{**good, **kw})
    assert call(scene=None) == BAD
    assert b"scene" in message() and entry.encode() + b":" in message()
    assert call(planes=None) == BAD
    assert b"planes" in message()
    assert call(total=None) == BAD
    assert b"total_out" in message()
    assert call(n=0) == BAD
    assert b"n == 0" in message()
    assert call(margin=float("nan")) == BAD
    assert b"margin" in message() and b"NaN" in message()
    assert call(items=None) == BAD                                               # gap_out without items_out
    assert b"gap_out without items_out" in message()
    for capacity in (1 << 31, 0xFFFFFFFF):
        assert call(capacity=capacity) == BAD
        assert b"capacity" in message()
    for k in (1, 2, 3):
        for name, base in (("items", 384), ("planes", 0), ("gap", 512)):
            assert call(**{name: at(base + k)}) == BAD
            assert (name.encode() if name == "planes" else name.encode() + b"_out") in message(), name
            assert b"aligned" in message()
    for k in (1, 4, 7):
        assert call(offsets=at(640 + k)) == BAD
        assert b"offsets_out" in message()
        assert call(total=at(768 + k)) == BAD
        assert b"total_out" in message()
    # n * J above 2^26 (the stand-in scene has no nodes: J is 1 whatever is asked for)
    for sections in (0, 1, 1000):
        assert call(n=(1 << 26) + 1, sections=sections) == BAD
        assert b"2^26" in message()


def _good_regions(R=np.float32):
    p = unit_regions(4).astype(R)
    p[1, 5] = ABSENT
    p[2, 0, 3] = -np.inf                                                         # a unit normal with d = -inf: a plane that never wins
    return p


def test_the_host_entry_checks_its_domain_before_any_device_is_touched():
    # the planes are read on the host before the scene's device is used (a stand-in handle of zero bytes: precision 0 is RT_F32)
    stand_in = ctypes.create_string_buffer(8192)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    total = ctypes.c_uint64(0)
    message = capi.lib.rt_last_error_message

    def call(p):
        p = np.ascontiguousarray(p, np.float32)
        return capi.lib.rt_overlap_regions(handle, p.ctypes.data, len(p), 0.0, 0, 0, None, None, None, ctypes.byref(total), None)
    good = _good_regions()
    cases = [((0, 0, 0), np.nan, b"NaN"), ((1, 3, 3), np.nan, b"NaN"), ((3, 5, 2), np.nan, b"NaN"),
             ((0, 1, 1), np.inf, b"infinite normal"), ((2, 4, 0), -np.inf, b"infinite normal"),
             ((1, 2, 3), np.inf, b"+inf"), ((0, 0, 3), 2e15, b"1e15"), ((3, 1, 3), -1.5e15, b"1e15")]
    for (g, k, c), value, word in cases:
        p = good.copy()
        p[g, k, c] = value
        assert call(p) == BAD, (g, k, c, value)
        assert word in message() and b"region %d" % g in message() and b"plane %d" % k in message(), message()
    p = good.copy()
    p[1, 2, :3] = 0                                                              # a zero normal with a finite d
    assert call(p) == BAD and b"zero normal" in message() and b"region 1" in message() and b"plane 2" in message()
    for scale in (1.0 + 2.0 ** -9, 1.0 - 2.0 ** -9, 2.0, 0.5, 1e-3):             # |n.n - 1| above 2^-10: never normalised
        p = good.copy()
        p[2, 3, :3] *= np.float32(scale)
        assert call(p) == BAD, scale
        assert b"length 1" in message() and b"region 2" in message() and b"plane 3" in message()
    # of two violations the one at the lower index is reported
    p = good.copy()
    p[3, 0, 0], p[1, 4, 3] = np.nan, np.inf
    assert call(p) == BAD and b"region 1" in message() and b"plane 4" in message()


def test_the_region_flavours_and_their_residency(tmp_path):
    # every flavour exists in both libraries, without scratch and within eight waves per SIMD; the register counts are reported
    want = sorted("rt::k_overlap_regions<%s, %s>" % (t, f) for t in ("float", "double") for f in ("true, false", "false, false", "false, true"))
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_overlap_regions<")]
        assert sorted(flavours) == want, flavours
        for n in flavours + ["rt::k_region_rows"]:
            r = k[n]
            print("%s: %s: %d scalar, %d vector registers, %d bytes of scratch" % (os.path.basename(path), n, r["sgpr"], r["vgpr"], r["scratch"]))
            assert r["scratch"] == 0 and r["sgpr"] <= 80 and r["vgpr"] <= 64, (n, r)


# ---- the metric ----

def scalar_region_gap(R, p, s):
    """The definition, one operation at a time on numpy scalars of type R (each rounds once)."""
    rr = R(s[3] * s[3])
    if not rr > 0:
        return R(np.inf)
    m = R(-np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(6):
            nx, ny, nz, d = p[4 * k:4 * k + 4]
            sk = R(R(R(R(nx * s[0]) + R(ny * s[1])) + R(nz * s[2])) + d)
            m = sk if sk > m else m
        return R(m - np.sqrt(rr))


def _inputs(R):
    rng = np.random.default_rng(7)
    s = np.concatenate([rng.uniform(-1, 1, (40, 3)), rng.uniform(0.01, 0.4, (40, 1))], axis=1).astype(R)
    s[5, 3] = 0                                                                  # a dead slot as the tests hold it: {.., 0}
    s[9] = 0
    s[11, 3] = R(1e-30) if R == np.float32 else R(1e-200)                        # rr rounds to 0: no positive rr
    p = unit_regions(40, 8).astype(R)
    p[4, :] = ABSENT                                                             # six absent planes
    p[6, 1:] = ABSENT                                                            # a half-space
    return p, s


DEAD = [5, 9, 11]


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_region_gaps_is_the_definition(R):
    U = np.uint32 if R == np.float32 else np.uint64
    # everything exact: the cube [0, 1]^3 as six planes; a centre 3 and 4 outside two faces -> 4 - 1.5 (the LARGEST excess, not their root);
    # one 2 outside a face and touching; one inside: the depth to the nearest face counts, -0.25 - 0.125
    cube = np.array([[[-1, 0, 0, 0], [1, 0, 0, -1], [0, -1, 0, 0], [0, 1, 0, -1], [0, 0, -1, 0], [0, 0, 1, -1]]], R)
    s = np.array([[4, 5, 0.5, 1.5], [0.5, 0.5, 3, 2], [0.25, 0.5, 0.75, 0.125], [-3, 0.5, -4, 1]], R)
    g = rta.region_gaps(cube, s)
    assert g.dtype == R and g.shape == (1, 4) and g[0].tolist() == [2.5, 0.0, -0.375, 3.0]
    np.testing.assert_array_equal(rta.region_gaps(cube.reshape(1, 24), s), g)
    p, s = _inputs(R)
    assert R(s[11, 3] * s[11, 3]) == 0
    got = rta.region_gaps(p, s)
    ref = np.array([[scalar_region_gap(R, x.reshape(24), y) for y in s] for x in p], R)
    np.testing.assert_array_equal(got.view(U), ref.view(U))
    assert (got[:, DEAD] == R(np.inf)).all()
    live = np.delete(np.arange(40), DEAD)
    # six absent planes: -inf for every live sphere, listed at every margin above -inf; a dead one stays at +inf
    assert (got[4, live] == -np.inf).all() and (got[4, DEAD] == np.inf).all()
    assert np.isfinite(np.delete(got, 4, axis=0)[:, live]).all()
    # a half-space: its one plane's distance minus the radius
    n, d = p[6, 0, :3], p[6, 0, 3]
    one = ((n[0] * s[live, 0] + n[1] * s[live, 1]) + n[2] * s[live, 2]) + d
    np.testing.assert_array_equal(got[6, live].view(U), (one - np.sqrt(s[live, 3] * s[live, 3])).view(U))
    # a NaN region carries no query on the device; here its row is what the arithmetic gives: a NaN s_k fails the comparison and never wins
    odd = cube.copy()
    odd[0, 1, 3] = np.nan
    assert rta.region_gaps(odd, s[:1] * 0 + np.array([4, 0.5, 0.5, 1], R)).tolist() == [[-1.5]]
    assert rta.region_gaps(np.zeros((0, 24), R), s).shape == (0, 40) and rta.region_gaps(p, np.zeros((0, 4), R)).shape == (40, 0)


def test_region_gaps_checks_its_arguments():
    p, s = np.zeros((4, 6, 4), np.float32), np.zeros((4, 4), np.float32)
    for bad in (p.astype(np.float16), p[:, :, :3], p.reshape(-1), p.astype(np.int32), p.astype(np.float64), s, p.reshape(4, 4, 6)):
        with pytest.raises(ValueError, match="planes"):
            rta.region_gaps(bad, s)
    for bad in (s.astype(np.float16), s[:, :3], s.reshape(-1), s.astype(np.int32), s.astype(np.float64), p):
        with pytest.raises(ValueError, match="planes"):
            rta.region_gaps(p, bad)


N_REGIONS = 80


def placed_regions(c):
    """(REAL[80, 6, 4], float64 points[80, 6, 3]) of Case c: unit_regions' shapes drawn in the base scene's frame -- centres in 1.2 times
    the base items' box about its centre, half-extents and the pyramids' near distance in units of that box's half-size -- with one point of
    every plane mapped through the case's placement and rounded to REAL; the normal is the rotation's axis rounded to REAL (the placements
    do not turn), d = -(n . point) formed in float64 from those REAL values and rounded once."""
    R = REAL[c.precision]
    k = [b[0] for b in ss.base_scenes()].index(c.name)
    it = np.asarray(c.items0, dtype=np.float64).reshape(-1, 4)
    lo, hi = (it[:, :3] - it[:, 3:]).min(axis=0), (it[:, :3] + it[:, 3:]).max(axis=0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    unit = unit_regions(N_REGIONS, 2000 + k)
    f = dict(ss.placements(c.precision))[c.placement]
    out = np.zeros((N_REGIONS, 6, 4), R)
    size = float(half.mean())
    for g in range(N_REGIONS):
        for j in range(6):
            n64 = unit[g, j, :3]
            if not n64.any():
                out[g, j] = ABSENT
                continue
            point = mid + (-unit[g, j, 3] * n64) * size                             # a point of the plane, in the base frame
            placed = f(np.concatenate([point, [0.0]])[None, :], None, ss.EYE)[0][0, :3]
            nR = n64.astype(R)
            out[g, j, :3] = nR
            out[g, j, 3] = R(-(nR.astype(np.float64) @ placed))
    return out


@CASES
def test_region_gaps_is_the_largest_plane_distance_minus_the_radius(param):
    """Every (region, item) of the two base scenes at every placement, against the same expression in higher precision from the placed
    REAL inputs: ref = max_k (n_k . c + d_k) - r.  The bound is derived from the chain -- three products, three additions, one root, one
    subtraction -- with u the unit roundoff:
      s_k   three rounded products summed left to right and + d: the first two products pass three additions, the third two, d one, so
            |s_k - exact| <= ((1 + u)^4 - 1) A_k,  A_k = |n.x c.x| + |n.y c.y| + |n.z c.z| + |d_k|
      m     comparisons are exact and a maximum is 1-Lipschitz in the sup norm: |m - exact| <= ((1 + u)^4 - 1) A,  A = max_k A_k
      root  rr = r*r (1 + d1), its root r (1 + d1)^(1/2) (1 + d2): within ((1 + u)^(3/2) - 1) r <= 2 u r of r
      gap   one more rounding of a value that is at most A + r in size
    together ((1 + u)^4 - 1) A + 2 u r + u (1 + 5 u) (A + r) <= 6 u (A + r).  f32 at 1e-20 is DESIGN.md 4.16's stated exception: rr is a
    denormal, so no value is asserted there, only that every gap is a number with the sign of the reference wherever the reference is
    more than a quarter of A + r.
    Worst observed share of the bound: 0.370 in f32 (the concentric scene at 5e13) and 0.389 in f64 (the nested scene at 1e-10)."""
    precision, placement = param
    R = REAL[precision]
    H, u = higher(precision)
    for c in ss.case(precision, placement)[:2]:
        what = (ss.case_id(param), c.name)
        items, planes = c.scene.items, placed_regions(c)
        got = rta.region_gaps(planes, items)
        gap = got.astype(H)
        it, pl = items.astype(H), planes.astype(H)
        cc = it[None, :, None, :3]                                              # [1, m, 1, 3]
        nn, dd = pl[:, None, :, :3], pl[:, None, :, 3]                          # [n, 1, 6, 3], [n, 1, 6]
        with np.errstate(invalid="ignore"):
            sk = (nn * cc).sum(axis=3) + dd
            A = np.where(np.isfinite(dd), np.abs(nn * cc).sum(axis=3) + np.abs(dd), H(0)).max(axis=2)
        ref = sk.max(axis=2) - it[None, :, 3]
        reach = A + it[None, :, 3]
        bound = H(6.0) * H(u) * reach
        assert np.isfinite(gap).all() and (ref < 0).any() and (ref > 0).any(), what
        worst = float(np.max(np.abs(gap - ref) / bound))
        print("%s %s: %d gaps, %d reach in; the worst error is %.3f of its bound" % (what + (gap.size, int((ref < 0).sum()), worst)))
        if param != DENORMAL_SQUARES:
            assert (np.abs(gap - ref) <= bound).all(), (what, worst)
        else:
            far = np.abs(ref) > 0.25 * reach
            assert far.any() and (np.sign(gap[far]) == np.sign(ref[far])).all(), what


# ---- the sectioned walk is the one-lane walk ----

@pytest.mark.parametrize("name", SCENES)
def test_the_sections_lists_are_the_one_lane_walks(name):
    """For J in 1, 2, 3, 7, 64, 65, N - 1 and N, at three margins: the same items, gap bits and offsets as the walk from node 0; at J = 1
    the same counters too.  (f32 at every J; f64 at 1, 3 and 65.)"""
    for precision, n_regions in ((rta.RT_F32, 40), (rta.RT_F64, 16)):
        s = five_scenes(precision)[name]
        w = Walker(s, regions_for(s, n_regions))
        r, N = median_radius(s), w.n_nodes
        assert N > 7 and (name != "refit" or N > 65)                          # (a J above N is clamped to N, as the library clamps it)
        for margin in (0.0, 4.0 * r, -0.25 * r):
            ref_i, ref_g, ref_o, ref_st = w.all(margin)
            assert len(ref_i) > 0 or margin < 0
            for J in section_counts(N) if precision == rta.RT_F32 else (1, 3, 65):
                items, gaps, offsets, st = w.sectioned(margin, J)
                np.testing.assert_array_equal(items, ref_i, err_msg=str((name, margin, J)))
                np.testing.assert_array_equal(bits(gaps, w.R), bits(ref_g, w.R), err_msg=str((name, margin, J)))
                np.testing.assert_array_equal(offsets, ref_o, err_msg=str((name, margin, J)))
                assert (st["primary"], st["hits"]) == (ref_st["primary"], ref_st["hits"])
                if J == 1:
                    assert st == ref_st, (name, margin)
                else:
                    assert st["tests_executed"] >= ref_st["sphere_tests"]        # every item the walk tests is tested by exactly one section
                    assert st["sphere_tests"] == ref_st["sphere_tests"], (name, margin, J)


# ---- the walk against brute force ----

# the 300 refit spheres and the 80 regions of default_rng(91), worked out in numpy in both precisions: entries and the longest row
REFIT_ENTRIES = {"0": (431, None), "r": (776, None), "-r/4": (362, None), "4r": (2466, 113)}


def brute_force(s, planes, margin):
    """(gap[n, m], listed, closest): every item's own test; closest = how near any finite gap comes to the margin, relative to their sizes."""
    R = REAL[s.precision]
    gap = rta.region_gaps(planes, s.items)
    m = R(margin)
    listed = ~(gap >= m)
    live = gap[np.isfinite(gap)].astype(np.float64)
    closest = float(np.min(np.abs(live - float(m)) / (np.abs(live) + abs(float(m)) + 1e-300)))
    return gap, listed, closest


@PRECISIONS
def test_the_walk_is_brute_force_where_nothing_grazes(precision):
    """default_L3, refit and clump at four margins: NO gap of the reference comes within a relative 1e-5 of the margin (the closest is
    6e-5, far above rounding) -- a condition on the reference alone, not a tolerance -- and the walk's list is brute force's entry for
    entry.  nested and nested3 have bounds that do not enclose their items: there the list is the walk's, and no more is asked."""
    R = REAL[precision]
    scenes = five_scenes(precision)
    for name in ("default_L3", "refit", "clump"):
        s = scenes[name]
        planes = regions_for(s)
        w = Walker(s, planes)
        r = median_radius(s)
        for label, margin in MARGINS:
            gap, listed, closest = brute_force(s, planes, margin(r))
            assert closest > 1e-5, (name, label, closest)                        # nothing grazes: if a changed helper moves a case here, change the seed
            items, gaps, offsets, _ = w.all(margin(r))
            gi, gj = np.nonzero(listed)
            np.testing.assert_array_equal(items, gj, err_msg=str((name, label)))
            np.testing.assert_array_equal(offsets, np.concatenate([[0], np.cumsum(listed.sum(axis=1))]), err_msg=str((name, label)))
            np.testing.assert_array_equal(bits(gaps, R), bits(gap[listed], R), err_msg=str((name, label)))
            assert len(items) > 0
            if name == "refit":
                entries, longest = REFIT_ENTRIES[label]
                assert len(items) == entries, (label, len(items))
                assert longest is None or int(np.diff(offsets.astype(np.int64)).max()) == longest
    for name in ("nested", "nested3"):
        s = scenes[name]
        planes = regions_for(s)
        items, _, _, _ = Walker(s, planes).all(0.0)
        _, listed, _ = brute_force(s, planes, 0.0)
        assert len(items) <= listed.sum()                                        # the walk can only leave out what a bound culled


# ---- the helpers that make regions ----

@PRECISIONS
def test_camera_planes_enclose_the_cameras_own_sample_rays(precision):
    R = REAL[precision]
    w, h = 32, 24
    for eye, target, hfov in (((0.3, 1.5, -4.0), (0.0, 0.0, 0.0), 60.0), ((0.1, 0.05, -0.2), (0.0, 0.3, 1.0), 90.0), ((0, 0, -4), (0, 0, 0), None)):
        cam = rta.look_at(eye, target, hfov_deg=hfov, precision=precision)
        e, right, up, fwd = (cam[3 * k:3 * k + 3].astype(np.float64) for k in range(4))
        for rect in (None, (8, 16, 16, 8), (0, 24, 1, 23), (31, 1, 32, 0)):
            planes = rta.camera_planes(cam, w, h, rect, near=0.05, far=40.0)
            assert planes.dtype == R and planes.shape == (1, 6, 4)
            assert np.abs((planes[0, :, :3].astype(np.float64) ** 2).sum(axis=1) - 1).max() < 2.0 ** -10
            bare = rta.camera_planes(cam, w, h, rect)
            assert (bare[0, 4:] == np.array(ABSENT, R)).all() and (bare[0, :4] == planes[0, :4]).all()
            l, t, r, b = (0, h, w, 0) if rect is None else rect
            xs, ys = np.meshgrid(np.arange(l, r), np.arange(b, t))
            worst = -np.inf
            for sub in (0.0, 0.5, 0.75):                                         # the samples of spp 1, 2 and 4 (xres = x + ssx / spp)
                u = (xs + sub) - w / 2.0
                v = (h - (ys + sub)) - h / 2.0
                d = right[None, None] * u[..., None] + up[None, None] * v[..., None] + fwd[None, None] * float(w)
                d /= np.sqrt((d * d).sum(axis=2, keepdims=True))
                for tt in (0.2, 1.0, 7.0, 39.0):                                 # (0.2 along a corner ray of the 90 degree view is 0.1 deep: behind the near plane)
                    p = e + tt * d
                    # s_k in float64 from the REAL planes, and the metric itself for a sphere of radius 0+ at the point
                    sk = np.einsum("kc,yxc->yxk", planes[0, :, :3].astype(np.float64), p) + planes[0, :, 3].astype(np.float64)
                    worst = max(worst, float(sk.max()))
                    pts = np.concatenate([p.reshape(-1, 3), np.full((p.size // 3, 1), 1e-3)], axis=1).astype(R)
                    assert (rta.region_gaps(planes, pts) < 0).all()
            assert worst <= 0.0, (eye, rect, worst)
    for bad in ((0, 24, 0, 0), (0, 25, 32, 0), (-1, 24, 32, 0), (0, 10, 32, 10)):
        with pytest.raises(ValueError, match="rect"):
            rta.camera_planes(cam, w, h, bad)
    with pytest.raises(ValueError, match="camera"):
        rta.camera_planes(cam[:9], w, h)


@PRECISIONS
def test_box_planes_of_an_axis_aligned_box_stay_below_box_gaps(precision):
    R = REAL[precision]
    rng = np.random.default_rng(5)
    c, hh = rng.uniform(-1, 1, (30, 3)), rng.uniform(0.0, 0.6, (30, 3))
    lo, hi = (c - hh).astype(R), (c + hh).astype(R)
    lo[3, 0] = lo[4, 1] = -np.inf
    hi[4, 2] = hi[5, 0] = np.inf
    lo[6], hi[6] = -np.inf, np.inf
    planes = rta.box_planes(lo, hi)
    assert planes.dtype == R and planes.shape == (30, 6, 4)
    assert (planes[3, 0] == np.array(ABSENT, R)).all() and (planes[4, 5] == np.array(ABSENT, R)).all() and (planes[6] == np.array(ABSENT, R)).all()
    s = np.concatenate([rng.uniform(-2, 2, (200, 3)), rng.uniform(0.01, 0.5, (200, 1))], axis=1).astype(R)
    rg, bg = rta.region_gaps(planes, s), rta.box_gaps(np.concatenate([lo, hi], axis=1), s)
    assert (rg <= bg).all()
    outside_one_face = (rg > -s[None, :, 3]) & (rg == bg)
    assert outside_one_face.any() and (rg < bg).any()
    # a rotated box: unit normals, the centre inside, and with the identity rotation the axis-aligned planes
    rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    turned = rta.box_planes(lo[10:], hi[10:], rot)
    assert np.abs((turned[:, :, :3].astype(np.float64) ** 2).sum(axis=2) - 1).max() < 2.0 ** -10
    centres = np.concatenate([0.5 * (lo[10:].astype(np.float64) + hi[10:]), np.full((20, 1), 1e-6)], axis=1).astype(R)
    assert (np.diagonal(rta.region_gaps(turned, centres)) <= 0).all()
    same = rta.box_planes(lo[10:], hi[10:], np.eye(3))
    np.testing.assert_allclose(same, planes[10:], rtol=0, atol=4 * np.finfo(R).eps)
    with pytest.raises(ValueError, match="lo"):
        rta.box_planes(hi[:3], lo[:3] - 1)
    with pytest.raises(ValueError, match="orthonormal"):
        rta.box_planes(lo[10:], hi[10:], 2 * np.eye(3))


def test_region_sections_stays_within_its_clamps():
    for n in (1, 2, 7, 64, 65, 1000, 1 << 18, (1 << 18) + 1, 1 << 26):
        for n_nodes in (1, 2, 31, 32, 33, 63, 64, 1000, 29127, 116509, 200000, 1 << 30):
            J = rta.region_sections(n, n_nodes)
            assert 1 <= J <= n_nodes and isinstance(J, int)
            assert J == max(1, min((1 << 18) // n, n_nodes // 8))               # the rule of include/rtrace_hip.h
            assert J == 1 or (n * J <= 1 << 18 and n_nodes // J >= 8)            # at most 2^18 lanes, no section under 8 nodes
            for asked in (1, 2, 64, n_nodes - 1, n_nodes, n_nodes + 1, 0xFFFFFFFF):
                if asked >= 1:
                    assert rta.region_sections(n, n_nodes, asked) == min(asked, n_nodes)
    assert rta.region_sections(5, 0) == 1 and rta.region_sections(5, 0, 9) == 1   # (no stream: one empty section)
    header = open(os.path.join(ROOT, "include", "rtrace_hip.h")).read()
    assert "J = max(1, min(floor(2^18 / n), floor(N / 8)))" in header
    for bad in ((0, 10), (-1, 10), (1, 10, -1)):
        with pytest.raises(ValueError):
            rta.region_sections(*bad)


# ---- the calls the wrapper makes ----

@pytest.fixture
def lib(monkeypatch):
    rec = _Recorder(capi.lib)
    monkeypatch.setattr(capi, "lib", rec)
    return rec


@PRECISIONS
@pytest.mark.parametrize("capacity", [None, 3])
def test_region_overlaps_calls(lib, precision, capacity):
    R = REAL[precision]
    d = _device_scene(precision)
    planes = _good_regions(R)
    n = len(planes)
    lib.snap["rt_overlap_regions"] = {1: planes.nbytes}
    for given, sections, want_sections in ((planes, None, 0), (planes.reshape(n, 24), 0, 0), (planes, 65, 65)):
        res = d.region_overlaps(given, 0.25, sections=sections, capacity=capacity, gaps=True, offsets=True, stats=True)
        calls = lib.take()
        assert [c[0] for c in calls] == ["rt_overlap_regions"] * (2 if capacity is None else 1)
        for k, (name, args, seen) in enumerate(calls):
            assert len(args) == 11 and seen[1] == planes.tobytes()
            assert (args[2], args[3], args[4]) == (n, 0.25, want_sections)
            counting = capacity is None and k == 0
            assert args[5] == (0 if counting else TOTAL if capacity is None else capacity)
            assert (args[6] is None) == (args[7] is None) == (args[8] is None) == counting
            assert _is_stats(args[10]) != counting
        items, gap, offsets, total, st = res
        m = TOTAL if capacity is None else min(capacity, TOTAL)
        assert items.dtype == np.int32 and items.shape == (m,) and gap.dtype == R and gap.shape == (m,)
        assert offsets.dtype == np.uint64 and offsets.shape == (n + 1,) and total == TOTAL and isinstance(st, dict)
    items, total = d.region_overlaps(planes, capacity=2)
    assert items.shape == (2,) and total == TOTAL
    (name, args, _), = lib.take()
    assert args[3] == 0.0 and args[7] is None and args[8] is None and args[10] is None


@PRECISIONS
def test_region_overlaps_checks_its_arguments_before_the_library(lib, precision):
    R = REAL[precision]
    d = _device_scene(precision)
    p = _good_regions(R)
    with pytest.raises(ValueError, match="margin"):
        d.region_overlaps(p, float("nan"))
    with pytest.raises((TypeError, ValueError)):
        d.region_overlaps(p, "near")
    for sections in (-1, 1 << 32):
        with pytest.raises(ValueError, match="sections"):
            d.region_overlaps(p, sections=sections)
    for capacity in (-1, 1 << 31, 1 << 40):
        with pytest.raises(ValueError, match="capacity"):
            d.region_overlaps(p, 0.0, capacity=capacity)
    other = np.float64 if R == np.float32 else np.float32
    for bad in (p.astype(other), p[:, :, :3], p.reshape(-1), p[:0], p.tolist(), None, np.zeros((5, 6), R), p.reshape(len(p), 4, 6)):
        with pytest.raises(ValueError, match="planes"):
            d.region_overlaps(bad)
    with pytest.raises(TypeError):
        d.region_overlaps(p, exclude=np.zeros(len(p), np.int32))                 # regions are no items: there is no exclude and no order
    with pytest.raises(TypeError):
        d.region_overlaps(p, order=True)
    assert lib.take() == []
