"""Coherent ray batches (rt_ray_order*, rt_*_ordered*; csrc/rt_order.hpp) without a GPU: the ABI, the argument checks made
before any device is touched, the new kernels' resources read back from the code object, and the sort key restated in numpy -- its
properties and the coherence it gives a shuffled camera batch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from rust_tracer_amd.scene import DeviceScene
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB, LLVM, ROOT

ENTRIES = ("rt_ray_order", "rt_ray_order_device", "rt_intersect_rays_ordered", "rt_intersect_rays_ordered_device",
           "rt_intersect_rays_multi_ordered", "rt_intersect_rays_multi_ordered_device", "rt_trace_rays_ordered", "rt_trace_rays_ordered_device")
BAD = capi.RT_ERR_INVALID_ARGUMENT


def test_both_libraries_export_the_eight_entries_at_abi_5():
    assert capi.ABI_VERSION == 5
    assert set(ENTRIES) <= set(capi.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "rtrace_hip.h")).read()
    assert "#define RTRACE_HIP_ABI_VERSION 5" in header
    for name in ENTRIES:
        assert re.search(r"\brt_status %s\(" % name, header), name
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert lib.rt_abi_version() == 5
        for name in ENTRIES:
            assert getattr(lib, name) is not None


def _stand_in():
    # the entries check pointers, sizes, modes and a host order before they look at the scene's device: a zeroed stand-in handle (an f32
    # scene, as far as the checks read it) is never handed to the runtime
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _call(entry, scene, rays, n, order, out, mode=0, k=4):
    f = getattr(capi.lib, entry)
    dev = entry.endswith("_device")
    tail = (None, None) if dev else (None,)            # [hip_stream,] stats
    if entry.startswith("rt_ray_order"):
        return f(scene, rays, n, out, None) if dev else f(scene, rays, n, out)
    if entry.startswith("rt_intersect_rays_ordered"):
        return f(scene, mode, rays, None, n, order, out, None, None, *tail)
    if entry.startswith("rt_intersect_rays_multi_ordered"):
        return f(scene, mode, k, rays, None, n, order, out, None, None, None, *tail)
    return f(scene, rays, n, order, out, None, *tail)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    keep, handle = _stand_in()
    rays = (ctypes.c_float * 12)(0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0)
    out = (ctypes.c_float * 64)()
    assert _call(entry, None, rays, 2, None, out) == BAD                       # NULL scene
    assert _call(entry, handle, None, 2, None, out) == BAD                     # NULL rays
    assert _call(entry, handle, rays, 2, None, None) == BAD                    # NULL distance_out / color_out / order_out
    assert _call(entry, handle, rays, 0, None, out) == BAD                     # n == 0
    misaligned = ctypes.c_void_p(ctypes.addressof(out) + 2)
    if entry.startswith("rt_ray_order"):
        assert _call(entry, handle, rays, 2, None, misaligned) == BAD          # misaligned order_out
        assert b"order_out" in capi.lib.rt_last_error_message()
        return
    assert _call(entry, handle, rays, 2, misaligned, out) == BAD               # misaligned order
    assert b"order" in capi.lib.rt_last_error_message()
    if "multi" in entry:
        for k in (0, 17):
            assert _call(entry, handle, rays, 2, None, out, k=k) == BAD        # k outside 1 .. RT_MULTIHIT_MAX_K
            assert b"k must be" in capi.lib.rt_last_error_message()
    if "intersect" in entry:
        for mode in (2, -1, 7):
            assert _call(entry, handle, rays, 2, None, out, mode=mode) == BAD  # unknown mode
            assert b"mode" in capi.lib.rt_last_error_message()
    if not entry.endswith("_device"):
        # a host order must be a permutation of 0 .. n-1
        for bad, word in (((0, 0), b"repeated"), ((1, 1), b"repeated"), ((0, 2), b"out of range"), ((0xFFFFFFFF, 0), b"out of range")):
            order = (ctypes.c_uint32 * 2)(*bad)
            assert _call(entry, handle, rays, 2, order, out) == BAD, bad
            msg = capi.lib.rt_last_error_message()
            assert word in msg and b"permutation" in msg, msg


def _lds_bytes(tmp_path, lib):
    """.group_segment_fixed_size of every kernel of `lib`, by demangled name (the other resources: test_kernel_resources._kernels)."""
    _kernels(tmp_path, lib)                                                     # unbundles the code object into tmp_path (or skips)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / "gfx950.co")], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n.split("(")[0].replace("void ", ""): v for n, v in zip(names, out.values())}


def test_the_new_kernels_and_their_residency(tmp_path):
    reals, flags = ("float", "double"), ("true", "false")
    want_query = sorted("rt::k_query_rays_ordered<%s, %s, %s>" % (t, c, a) for t in reals for c in flags for a in flags)
    want_multi = sorted("rt::k_multihit_rays_ordered<%s, %s, %s, %d>" % (t, c, a, b) for t in reals for c in flags for a in flags for b in (1, 4, 8, 16))
    want_trace = sorted("rt::k_trace_rays_ordered<%s, %s>" % (t, c) for t in reals for c in flags)
    want_sort = ["rt::k_ray_box<double>", "rt::k_ray_box<float>", "rt::k_ray_keys<double>", "rt::k_ray_keys<float>", "rt::k_sort_hist", "rt::k_sort_plan",
                 "rt::k_sort_scan", "rt::k_sort_scatter"]
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        # the ordered walks: the residency of their unordered twins (test_query_host, test_multihit_host, test_camera_host), no scratch
        assert sorted(n for n in k if n.startswith("rt::k_query_rays_ordered<")) == want_query
        for n in want_query:
            assert k[n]["sgpr"] <= 80 and k[n]["vgpr"] <= 64 and k[n]["scratch"] == 0, (n, k[n])
        assert sorted(n for n in k if n.startswith("rt::k_multihit_rays_ordered<")) == want_multi
        for n in want_multi:
            assert k[n]["scratch"] == 0, (n, k[n])
            if int(n.rstrip(">").split(",")[-1]) <= 4:
                assert k[n]["sgpr"] <= 80 and k[n]["vgpr"] <= 64, (n, k[n])
            else:
                assert k[n]["vgpr"] <= 128, (n, k[n])
        assert sorted(n for n in k if n.startswith("rt::k_trace_rays_ordered<")) == want_trace
        for n in want_trace:
            assert k[n]["scratch"] == 0, (n, k[n])
            if n.endswith(", false>"):
                assert k[n]["sgpr"] <= 80 and k[n]["vgpr"] <= 64, (n, k[n])
        # the order itself: box, keys and the radix sort -- eight waves per SIMD, no scratch, LDS within a workgroup's 64 KB
        lds = _lds_bytes(tmp_path, path)
        for n in want_sort:
            assert n in k, n
            assert k[n]["sgpr"] <= 80 and k[n]["vgpr"] <= 64 and k[n]["scratch"] == 0, (n, k[n])
            assert lds[n] <= 64 * 1024, (n, lds[n])
        assert lds["rt::k_sort_scatter"] > 0 and lds["rt::k_sort_hist"] > 0 and lds["rt::k_sort_scan"] > 0


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=["f32", "f64"])
def test_ray_keys_properties(R):
    rng = np.random.default_rng(3)
    n = 5000
    rays = np.concatenate([rng.normal(size=(n, 3)) * 7.0, _unit(rng.normal(size=(n, 3)))], axis=1).astype(R)
    k = rta.ray_keys(rays)
    assert k.dtype == np.uint32 and k.shape == (n,)
    assert np.array_equal(k, rta.ray_keys(rays.copy()))                        # deterministic
    assert len(np.unique(k >> 23)) > 100                                       # the origin cells are used ...
    assert set(np.unique((k >> 20) & 7)) == set(range(6))                      # ... and all six dominant axes / signs, never 6 or 7
    # the key depends on the ray and the batch's origin box only: a permuted batch has the permuted keys
    p = rng.permutation(n)
    assert np.array_equal(rta.ray_keys(rays[p]), k[p])
    # one origin: every origin bit is 0 -- no NaN, no division by zero -- and the direction bits are those of the full batch
    one = rays.copy()
    one[:, :3] = R(0.3), R(-2.0), R(1e6)
    k1 = rta.ray_keys(one)
    assert not (k1 >> 23).any() and np.array_equal(k1 & 0x7FFFFF, k & 0x7FFFFF)
    assert rta.ray_keys(rays[:1]).shape == (1,) and not (rta.ray_keys(rays[:1]) >> 23).any()
    # the corners of the box: the low corner is cell 0, the high corner's largest extent lands in the upper half of the 8 cells (the scale
    # is a power of two: ext < 2^e <= 2 ext), whatever the extent is -- tiny, huge, different per axis
    for scale in (1e-30, 1.0, 3e14):
        box = np.zeros((2, 6), dtype=R)
        box[:, 5] = 1
        box[1, :3] = R(scale), R(scale) / R(2), R(scale) / R(1024)
        kb = rta.ray_keys(box) >> 23
        cell = [sum(((int(kb[1]) >> (3 * i + a)) & 1) << i for i in range(3)) for a in range(3)]
        assert kb[0] == 0 and 4 <= cell[0] <= 7 and cell[1] == cell[0] // 2 and cell[2] == 0, (scale, cell)
    # a box thinner than 2^-1000 (f64 denormals) is one cell: the scale stays finite
    thin = np.zeros((2, 6), dtype=np.float64)
    thin[:, 5], thin[1, 0] = 1, 1e-310
    assert not (rta.ray_keys(thin) >> 23).any()
    # directions: the dominant axis and its sign, the lower axis on a tie
    t = 0.5 ** 0.5
    dirs = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.6, 0.6, 0.52915), (0.0, -t, t), (-0.0, 0.0, -1.0)])
    kd = rta.ray_keys(np.concatenate([np.zeros((len(dirs), 3)), dirs], axis=1).astype(R))
    assert list((kd >> 20) & 7) == [0, 1, 2, 3, 4, 5, 0, 3, 5]
    assert (kd[0] & 0xFFFFF) == (kd[1] & 0xFFFFF) == 0b11 << 18                # both other components 0 -> q = 512 each
    for bad in (rays.astype(np.float16), rays[:, :5], rays[:0], rays.reshape(-1)):
        with pytest.raises(ValueError):
            rta.ray_keys(bad)


def camera_rays(w, h, eye):
    """tools/query_rate.py's camera batch: the render's 1920x1080 primary rays (render.rs:231-241 in f32), row-major."""
    f = np.float32
    y, x = np.meshgrid(np.arange(h, dtype=f), np.arange(w, dtype=f), indexing="ij")
    fw, fh = f(w), f(h)
    dx, dy, dz = x - fw / f(2), (fh - y) - fh / f(2), np.full_like(x, fw)
    inv = f(1) / np.sqrt((dx * dx + dy * dy) + dz * dz)
    rays = np.empty((w * h, 6), dtype=f)
    rays[:, :3] = eye
    rays[:, 3], rays[:, 4], rays[:, 5] = (dx * inv).ravel(), (dy * inv).ravel(), (dz * inv).ravel()
    return rays


def patches_per_run(pixels, w):
    """Mean number of distinct 8x8-pixel patches a run of 64 consecutive entries of `pixels` (row-major pixel indices) touches."""
    patch = (pixels // w // 8) * (w // 8) + (pixels % w) // 8
    runs = np.sort(patch[:len(patch) // 64 * 64].reshape(-1, 64), axis=1)
    return float((1 + (np.diff(runs, axis=1) != 0).sum(axis=1)).mean())


def test_the_key_orders_a_shuffled_camera_batch_no_worse_than_pixel_order():
    """The key's coherence, measured on the CPU: the 1920x1080 camera rays shuffled (seed 1), ordered by the key, cut into runs of 64 -- one
    wave each.  Row-major pixel order, the layout behind every "pixel order" figure of DESIGN.md 4.6 - 4.8, touches exactly 8 patches of
    8x8 pixels per run; a shuffle about 64.  The key that ships must not be worse than the order the project calls coherent: mean <= 8.
    Measured: 4.735 (10 bits per direction component)."""
    w, h = 1920, 1080
    rays = camera_rays(w, h, rta.Scene.default().eye)
    perm = np.random.default_rng(1).permutation(w * h)
    assert patches_per_run(np.arange(w * h), w) == 8.0
    assert patches_per_run(perm, w) > 60.0
    order = np.argsort(rta.ray_keys(rays[perm]), kind="stable")
    score = patches_per_run(perm[order], w)
    print("patches per run of 64, ordered by the key: %.3f (row-major 8.0, shuffled %.1f)" % (score, patches_per_run(perm, w)))
    assert score <= 8.0, score


class _Stand:
    def __init__(self, precision):
        self.precision = precision


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_the_order_argument_is_checked_before_the_library(precision):
    R = np.float32 if precision == rta.RT_F32 else np.float64
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h = _Stand(precision), 0, None
    good = np.array([[0, 0, -4, 0, 0, 1]] * 3, dtype=R)
    for order in (np.zeros(2, np.uint32), np.zeros((3, 1), np.uint32), np.zeros(3, np.float32), [0.5, 1, 2], "abc"):
        for call in (lambda o: d.intersect(good, order=o), lambda o: d.intersect_multi(good, 4, order=o), lambda o: d.trace(good, order=o)):
            with pytest.raises(ValueError, match="order"):
                call(order)
    for rays in (good.astype(np.float16), good[:, :5], good[:0], good.tolist()):
        with pytest.raises(ValueError, match="rays"):
            d.ray_order(rays)
