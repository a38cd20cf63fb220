"""Box overlap lists (rt_overlap_boxes / rt_overlap_boxes_device, csrc/rt_box.hpp) without a GPU: the ABI, the argument
checks made before any device is touched, the residency of the kernel's flavours read back from the code object, rta.box_gaps -- the
metric's definition in numpy -- against a scalar restatement, against the overlap lists' metric for point boxes and against the geometry
away from unit scale, and the checks the Python wrapper makes before it calls the library.  (The one refusal that needs a device -- a
buffer in device memory -- is held by tests/test_gpu_box.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from rust_tracer_amd.scene import DeviceScene
from tests import scaled_scenes as ss
from tests.test_gpu_overlap import five_scenes, queries_for
from tests.test_gpu_query import REAL, bits
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB
from tests.test_scales_contact_host import DENORMAL_SQUARES, higher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_overlap_boxes", "rt_overlap_boxes_device")
BAD = capi.RT_ERR_INVALID_ARGUMENT
CASES = pytest.mark.parametrize("param", ss.cases_of(), ids=ss.case_id)


def test_both_libraries_export_the_box_entries_at_abi_5():
    assert capi.ABI_VERSION == 5
    assert set(ENTRIES) <= set(capi.SYMBOLS)
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert lib.rt_abi_version() == 5
        for name in ENTRIES:
            assert getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "rtrace_hip.h")).read()
    assert "#define RTRACE_HIP_ABI_VERSION 5" in header
    declared = set(re.findall(r"\b(rt_[a-z_]+)\s*\(", header))
    assert set(ENTRIES) <= declared and declared == set(capi.SYMBOLS), declared ^ set(capi.SYMBOLS)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert getattr(capi.lib, name).argtypes, name
        assert re.search(r"\bfn %s\(" % name, integration), name
    assert len(capi.lib.rt_overlap_boxes_device.argtypes) == len(capi.lib.rt_overlap_boxes.argtypes) + 1 == 13
    assert list(capi.lib.rt_overlap_boxes.argtypes) == list(capi.lib.rt_overlap_spheres.argtypes)
    assert callable(rta.box_gaps) and "box_gaps" in rta.__all__ and callable(DeviceScene.box_overlaps)


def _call(entry, scene, boxes, n, margin, exclude, order, capacity, items, gap, offsets, total):
    f = getattr(capi.lib, entry)
    args = (scene, boxes, n, margin, exclude, order, capacity, items, gap, offsets, total, None)
    return f(*args) if entry == "rt_overlap_boxes" else f(*args, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check pointers, n, the margin, the capacity and alignment before they use the scene: a stand-in handle will do
    stand_in = ctypes.create_string_buffer(8192)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    words = (ctypes.c_uint64 * 128)()
    at = lambda k: ctypes.c_void_p(ctypes.addressof(words) + k)
    boxes, exclude, order, items, gap, offsets, total = at(0), at(128), at(256), at(384), at(512), at(640), at(768)
    message = capi.lib.rt_last_error_message
    good = dict(scene=handle, boxes=boxes, n=4, margin=0.0, exclude=exclude, order=order, capacity=4, items=items, gap=gap, offsets=offsets, total=total)
    call = lambda **kw: _call(entry, **{**good, **kw})
    assert call(scene=None) == BAD
    assert b"scene" in message() and entry.encode() + b":" in message()
    assert call(boxes=None) == BAD
    assert b"boxes" in message()
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
        for name, base in (("items", 384), ("exclude", 128), ("order", 256), ("boxes", 0), ("gap", 512)):
            assert call(**{name: at(base + k)}) == BAD
            assert (name.encode() if name in ("exclude", "order", "boxes") else name.encode() + b"_out") in message(), name
            assert b"aligned" in message()
    for k in (1, 4, 7):
        assert call(offsets=at(640 + k)) == BAD
        assert b"offsets_out" in message()
        assert call(total=at(768 + k)) == BAD
        assert b"total_out" in message()


def test_the_host_entry_checks_its_domain_before_any_device_is_touched():
    # the boxes and the order are read on the host before the scene's device is used (a stand-in handle of zero bytes: precision 0 is RT_F32)
    stand_in = ctypes.create_string_buffer(8192)
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    total = ctypes.c_uint64(0)
    good = np.array([[0, 0, 0, 0.5, 1, 2], [1, 0, -3, 1, 0, -3], [-1, 2, 0, 1.0, 2.5, 0.25]], np.float32)
    message = capi.lib.rt_last_error_message

    def call(b, order=None):
        o = None if order is None else np.asarray(order, np.uint32)
        return capi.lib.rt_overlap_boxes(handle, b.ctypes.data, len(b), 0.0, None, None if o is None else o.ctypes.data, 0, None, None, None,
                                         ctypes.byref(total), None)
    for row, col, value in ((0, 0, np.nan), (1, 4, np.nan), (2, 5, np.nan), (0, 1, -2e15), (1, 3, 2e15), (2, 2, -1.5e15)):
        b = good.copy()
        b[row, col] = value
        assert call(b) == BAD, (row, col, value)
        assert b"coordinate" in message() and b"box %d" % row in message()
    for row, axis in ((0, 0), (1, 1), (2, 2)):
        b = good.copy()
        b[row, axis], b[row, 3 + axis] = 4.0, 3.0
        assert call(b) == BAD, (row, axis)
        assert b"inverted" in message() and b"box %d" % row in message() and b"axis %d" % axis in message()
    b = good.copy()
    b[1, 0], b[1, 3] = np.inf, -np.inf                                           # infinite AND inverted: the coordinates pass, the order of the corners does not
    assert call(b) == BAD and b"inverted" in message() and b"box 1" in message()
    # +-inf sides and lo == hi are in the domain: the call gets as far as the next refusal in line, an order that is no permutation
    inf = np.inf
    wide = np.array([[-inf, -inf, -inf, inf, inf, inf], [-inf, 0, 0, 0.5, inf, 0], [2, 2, 2, 2, 2, 2], [inf, 0, 0, inf, 1, 1], [-inf, 0, 0, -inf, 1, 1]], np.float32)
    for boxes, orders in ((good, ([0, 1, 1], [0, 1, 3], [2, 2, 2])), (wide, ([0, 1, 1, 3, 4], [0, 1, 5, 2, 3], [2, 2, 2, 2, 2]))):
        for order in orders:
            assert call(boxes, order) == BAD, order
            assert b"permutation" in message()


def test_the_box_flavours_and_their_residency(tmp_path):
    # every flavour exists in both libraries, without scratch and within k_contact_pairs's budget: eight waves per SIMD
    want = sorted("rt::k_overlap_boxes<%s, %s>" % (t, f) for t in ("float", "double") for f in ("true, false", "false, false", "false, true"))
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_overlap_boxes<")]
        assert sorted(flavours) == want, flavours
        for n in flavours:
            r = k[n]
            assert r["scratch"] == 0 and r["sgpr"] <= 80 and r["vgpr"] <= 64, (n, r)


def scalar_box_gap(R, b, s):
    """The definition, one operation at a time on numpy scalars of type R (each rounds once)."""
    rr = R(s[3] * s[3])
    if not rr > 0:
        return R(np.inf)
    e = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            ek = R(b[k] - s[k])
            fk = R(s[k] - b[3 + k])
            ek = fk if fk > ek else ek
            e.append(ek if ek > 0 else R(0.0))
        dd = R(R(R(e[0] * e[0]) + R(e[1] * e[1])) + R(e[2] * e[2]))
        return R(np.sqrt(dd) - np.sqrt(rr))


def _inputs(R):
    """test_overlap_host.py's spheres, and as many boxes: every tenth a point, some with infinite sides."""
    rng = np.random.default_rng(7)
    s = np.concatenate([rng.uniform(-1, 1, (40, 3)), rng.uniform(0.01, 0.4, (40, 1))], axis=1).astype(R)
    s[5, 3] = 0                                                                  # a dead slot as the tests hold it: {.., 0}
    s[9] = 0
    s[11, 3] = R(1e-30) if R == np.float32 else R(1e-200)                        # rr rounds to 0: no positive rr
    c, h = rng.uniform(-1.2, 1.2, (40, 3)), rng.uniform(0.0, 0.3, (40, 3))
    h[::10] = 0
    b = np.concatenate([c - h, c + h], axis=1).astype(R)
    b[3, 0] = b[13, 1] = b[23, 2] = -np.inf
    b[4, 3] = b[13, 4] = b[24, 5] = np.inf
    b[33] = [-np.inf] * 3 + [np.inf] * 3
    return b, s


DEAD = [5, 9, 11]


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_box_gaps_is_the_definition(R):
    U = np.uint32 if R == np.float32 else np.uint64
    inf = R(np.inf)
    # everything exact: the box [0, 1]^3; a centre 3 and 4 outside two faces -> 5 - 1.5; one 2 outside a face and touching; one inside
    s = np.array([[4, 5, 0.5, 1.5], [0.5, 0.5, 3, 2], [0.25, 0.5, 0.75, 0.125], [-3, 0.5, -4, 1]], R)
    g = rta.box_gaps(np.array([[0, 0, 0, 1, 1, 1]], R), s)
    assert g.dtype == R and g.shape == (1, 4) and g[0].tolist() == [3.5, 0.0, -0.125, 4.0]
    b, s = _inputs(R)
    assert R(s[11, 3] * s[11, 3]) == 0
    got = rta.box_gaps(b, s)
    ref = np.array([[scalar_box_gap(R, x, y) for y in s] for x in b], R)
    np.testing.assert_array_equal(got.view(U), ref.view(U))
    # a dead record is at +inf from every box, everything else is finite -- infinite sides make neither an inf nor a NaN
    assert (got[:, DEAD] == inf).all()
    live = np.delete(np.arange(40), DEAD)
    assert np.isfinite(got[:, live]).all()
    # the all-infinite box: -sqrt(rr), bit for bit; a centre inside a box: the same
    rr = s[live, 3] * s[live, 3]
    np.testing.assert_array_equal(got[33, live].view(U), (-np.sqrt(rr)).view(U))
    # half-infinite boxes against the finite box whose side lies beyond every centre: the same bits
    far = b.copy()
    far[far == -np.inf] = -64
    far[far == np.inf] = 64
    np.testing.assert_array_equal(got.view(U), rta.box_gaps(far, s).view(U))
    # against a restatement in extended precision: |gap - (dist(box, c) - r)| <= 8 u (dist + r), DESIGN.md 4.16's bound
    L = np.longdouble
    u = L(np.finfo(R).eps) / 2
    c = s[live, :3].astype(L)
    fb = far.astype(L)
    e = np.maximum(np.maximum(fb[:, None, :3] - c[None], c[None] - fb[:, None, 3:]), 0)
    dist = np.sqrt((e * e).sum(axis=2))
    r = s[live, 3].astype(L)[None]
    assert (np.abs(got[:, live].astype(L) - (dist - r)) <= 8 * u * (dist + r)).all()
    assert (dist == 0).any() and (dist > 0).any()
    # a tiny f32 radius in the scene: the root of the rounded square, not the radius
    if R == np.float32:
        r = R(3e-23)
        root = np.sqrt(R(r * r))
        assert root != r
        g = rta.box_gaps(np.array([[0, 0, 0, 0, 0, 0]], R), np.array([[0, 0, 0, r]], R))
        assert g[0, 0] == R(R(0.0) - root)
    # an inverted box and a NaN carry no query on the device; here the row is what the arithmetic gives, and a NaN excess ends as 0
    odd = np.array([[1, 0, 0, -1, 1, 1], [np.nan, 0, 0, 1, 1, 1]], R)
    g = rta.box_gaps(odd, np.array([[0, 0.5, 0.5, 0.25], [3, 0.5, 0.5, 0.25]], R))
    assert g.tolist() == [[0.75, 3.75], [-0.25, -0.25]]                          # (f > NaN fails, NaN > 0 fails)
    assert rta.box_gaps(np.zeros((0, 6), R), s).shape == (0, 40) and rta.box_gaps(b, np.zeros((0, 4), R)).shape == (40, 0)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_a_point_box_is_the_overlap_gap_with_q_zero(precision):
    R = REAL[precision]
    for name, s in five_scenes(precision).items():
        q = queries_for(s)
        q[:, 3] = 0
        p = np.ascontiguousarray(np.concatenate([q[:, :3], q[:, :3]], axis=1))
        got, ref = rta.box_gaps(p, s.items), rta.overlap_gaps(q, s.items)
        assert got.shape == (200, len(s.items))
        np.testing.assert_array_equal(bits(got, R), bits(ref, R), err_msg=name)


def test_box_gaps_checks_its_arguments():
    b, s = np.zeros((4, 6), np.float32), np.zeros((4, 4), np.float32)
    for bad in (b.astype(np.float16), b[:, :4], b.reshape(-1), b.astype(np.int32), b.astype(np.float64), s):
        with pytest.raises(ValueError, match="boxes"):
            rta.box_gaps(bad, s)
    for bad in (s.astype(np.float16), s[:, :3], s.reshape(-1), s.astype(np.int32), s.astype(np.float64), b):
        with pytest.raises(ValueError, match="boxes"):
            rta.box_gaps(b, bad)


N_BOXES = 80


def placed_boxes(c):
    """REAL[80, 6] of Case c: centres uniform in 1.2 times the base items' box about its centre, half-extents uniform in [0, 0.3] of that
    box's half-size per axis, every tenth a point, rows 5::10 a slab across the scene in x; drawn from default_rng(1000 + k) in the base
    scene's frame and mapped corner by corner through the case's placement, rounded once (rounding is monotonic: lo <= hi stays)."""
    R = REAL[c.precision]
    k = [b[0] for b in ss.base_scenes()].index(c.name)
    rng = np.random.default_rng(1000 + k)
    it = np.asarray(c.items0, dtype=np.float64).reshape(-1, 4)
    lo, hi = (it[:, :3] - it[:, 3:]).min(axis=0), (it[:, :3] + it[:, 3:]).max(axis=0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    centres = mid + rng.uniform(-1.2, 1.2, (N_BOXES, 3)) * half
    h = rng.uniform(0.0, 0.3, (N_BOXES, 3)) * half
    h[0::10] = 0
    h[5::10, 0] = 2.5 * half[0]
    f = dict(ss.placements(c.precision))[c.placement]
    corner = lambda x: f(np.concatenate([x, np.zeros((N_BOXES, 1))], axis=1), None, ss.EYE)[0][:, :3]
    return np.ascontiguousarray(np.concatenate([corner(centres - h), corner(centres + h)], axis=1).astype(R))


@CASES
def test_box_gaps_is_the_distance_from_the_box_to_the_surface(param):
    """Every (box, item) of the two base scenes at every placement: |box_gaps - (dist(box, c) - r)| <= 8 u (dist(box, c) + r), the
    reference in higher precision from the placed REAL inputs -- DESIGN.md 4.16's bound for this chain of operations (a sum of three
    squares, two roots, one subtraction) with one rounded subtraction per axis in front, which is the rounded difference that chain starts
    with.  f32 at 1e-20 is 4.16's stated exception: rr and dd are denormals, so no value is asserted there, only that every gap is a
    number with the sign of the reference wherever the reference is more than a quarter of dist + r.
    Worst observed share of the bound: 0.370 in f32 and 0.378 in f64, both on the concentric scene at 5e13."""
    precision, placement = param
    R = REAL[precision]
    H, u = higher(precision)
    for c in ss.case(precision, placement)[:2]:
        what = (ss.case_id(param), c.name)
        items, boxes = c.scene.items, placed_boxes(c)
        assert (boxes[:, :3] <= boxes[:, 3:]).all() and (boxes[0::10, :3] == boxes[0::10, 3:]).all()
        got = rta.box_gaps(boxes, items)
        gap = got.astype(H)
        it, bx = items.astype(H), boxes.astype(H)
        cc = it[None, :, :3]
        e = np.maximum(np.maximum(bx[:, None, :3] - cc, cc - bx[:, None, 3:]), H(0))
        dist = np.sqrt((e * e).sum(axis=2))
        ref = dist - it[None, :, 3]
        reach = dist + it[None, :, 3]
        bound = H(8.0) * H(u) * reach
        assert np.isfinite(gap).all() and (ref < 0).any() and (ref > 0).any() and (dist == 0).any(), what
        worst = float(np.max(np.abs(gap - ref) / bound))
        print("%s %s: %d gaps, %d touch, %d centres inside; the worst error is %.3f of its bound" % (what + (gap.size, int((ref < 0).sum()), int((dist == 0).sum()), worst)))
        if param != DENORMAL_SQUARES:
            assert (np.abs(gap - ref) <= bound).all(), (what, worst)
        else:
            far = np.abs(ref) > 0.25 * reach
            assert far.any() and (np.sign(gap[far]) == np.sign(ref[far])).all(), what


class _Stand:
    """Enough of a Scene for DeviceScene's checks, which come before any call into the library."""
    def __init__(self, precision):
        self.precision = precision
        self.items = np.zeros((3, 4), np.float32 if precision == rta.RT_F32 else np.float64)


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_box_overlaps_checks_its_arguments_before_the_library(precision):
    R = np.float32 if precision == rta.RT_F32 else np.float64
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h = _Stand(precision), 0, None
    b = np.zeros((5, 6), R)
    with pytest.raises(ValueError, match="margin"):
        d.box_overlaps(b, float("nan"))
    with pytest.raises((TypeError, ValueError)):
        d.box_overlaps(b, "near")
    with pytest.raises(ValueError, match="order"):
        d.box_overlaps(b, order=True)
    for capacity in (-1, 1 << 31, 1 << 40):
        with pytest.raises(ValueError, match="capacity"):
            d.box_overlaps(b, 0.0, capacity=capacity)
    with pytest.raises((TypeError, ValueError)):
        d.box_overlaps(b, 0.0, capacity="all")
    other = np.float64 if R == np.float32 else np.float32
    for bad in (b.astype(other), b[:, :4], b.reshape(-1), b[:0], b.tolist(), None, np.zeros((5, 4), R)):
        with pytest.raises(ValueError, match="boxes"):
            d.box_overlaps(bad)
    for bad in (np.zeros(5, np.int64), np.zeros(4, np.int32), np.zeros((5, 1), np.int32)):
        with pytest.raises(ValueError, match="exclude"):
            d.box_overlaps(b, exclude=bad)
    for bad in (np.zeros(5, R), np.zeros(4, np.uint32), np.array([0, 1, 2, 3, -1])):
        with pytest.raises(ValueError, match="order"):
            d.box_overlaps(b, order=bad)
    # (a tensor chooses the device side, whose checks run inside the call's stream scope: numpy boxes with tensor companions, and the other
    # way round, are refused in tests/test_gpu_box.py)
