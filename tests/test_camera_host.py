"""Traced rays and camera frames (rt_trace_rays* / rt_render_camera*, csrc/rt_trace.hpp) without a GPU: the ABI, the argument and camera
checks made before any device is touched, the residency of the k_trace_rays flavours read back from the code object, and look_at."""
import ctypes

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB

ENTRIES = ("rt_trace_rays", "rt_trace_rays_device", "rt_render_camera", "rt_render_camera_device")
IDENTITY = (0.0, 0.0, -4.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def test_both_libraries_export_the_camera_entries_at_abi_5():
    assert capi.ABI_VERSION == 5
    assert set(ENTRIES) <= set(capi.SYMBOLS)
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert lib.rt_abi_version() == 5
        for name in ENTRIES:
            assert getattr(lib, name) is not None


def _stand_in():
    # the entries check pointers, sizes, regions and the camera before they look at the scene: a stand-in handle is never read here
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _trace(entry, scene, rays, n, color):
    f = getattr(capi.lib, entry)
    if entry == "rt_trace_rays":
        return f(scene, rays, n, color, None, None)
    return f(scene, rays, n, color, None, None, None)


@pytest.mark.parametrize("entry", ["rt_trace_rays", "rt_trace_rays_device"])
def test_trace_argument_errors_are_reported_before_any_device_is_touched(entry):
    _keep, handle = _stand_in()
    rays = (ctypes.c_float * 6)(0, 0, 0, 0, 0, 1)
    color = (ctypes.c_float * 3)()
    assert _trace(entry, None, rays, 1, color) == capi.RT_ERR_INVALID_ARGUMENT          # NULL scene
    assert _trace(entry, handle, None, 1, color) == capi.RT_ERR_INVALID_ARGUMENT        # NULL rays
    assert _trace(entry, handle, rays, 1, None) == capi.RT_ERR_INVALID_ARGUMENT         # NULL color_out
    assert _trace(entry, handle, rays, 0, color) == capi.RT_ERR_INVALID_ARGUMENT        # n == 0


def _camera_call(entry, scene, cam, regions, n, out, opts=(64, 48, 1)):
    o = capi.Options(*opts)
    f = getattr(capi.lib, entry)
    if entry == "rt_render_camera":
        return f(scene, ctypes.byref(o), cam, regions, n, out, None)
    return f(scene, ctypes.byref(o), cam, regions, n, out, None, None)


def _cam(values):
    return (ctypes.c_float * 12)(*values)


def bad_cameras():
    """Cameras outside the domain of include/rtrace_hip.h, each with what is wrong with it."""
    out = []
    for k in (0, 4, 11):
        c = list(IDENTITY); c[k] = float("nan"); out.append(("nan%d" % k, c))
    c = list(IDENTITY); c[5] = float("inf"); out.append(("inf", c))
    c = list(IDENTITY); c[1] = 2e15; out.append(("far_eye", c))
    c = list(IDENTITY); c[2] = -1.5e15; out.append(("far_eye_neg", c))
    c = list(IDENTITY); c[3:6] = (0.0, 0.0, 0.0); out.append(("zero_right", c))
    c = list(IDENTITY); c[9:12] = (0.0, 0.0, 0.0); out.append(("zero_forward", c))
    c = list(IDENTITY); c[6:9] = (0.0, 0.005, 0.0); out.append(("short_up", c))
    c = list(IDENTITY); c[9:12] = (0.0, 0.0, 150.0); out.append(("long_forward", c))
    c = list(IDENTITY); c[6:9] = (1.0, 0.0, 0.0); out.append(("collinear", c))
    c = list(IDENTITY); c[9:12] = (0.6, 0.8, 0.0); out.append(("coplanar", c))
    # det / (|r||u||f|) = 0.005, below 1e-2: forward tilted to within a third of a degree of the right-up plane
    c = list(IDENTITY); c[9:12] = (0.0, float(np.sqrt(1 - 0.005 ** 2)), 0.005); out.append(("near_flat", c))
    return out


@pytest.mark.parametrize("entry", ["rt_render_camera", "rt_render_camera_device"])
def test_camera_argument_errors_are_reported_before_any_device_is_touched(entry):
    _keep, handle = _stand_in()
    regions = (capi.Region * 1)(capi.Region(0, 48, 64, 0))
    out = ctypes.create_string_buffer(64 * 48 * 4)
    cam = _cam(IDENTITY)
    assert _camera_call(entry, None, cam, regions, 1, out) == capi.RT_ERR_INVALID_ARGUMENT          # NULL scene
    assert _camera_call(entry, handle, None, regions, 1, out) == capi.RT_ERR_INVALID_ARGUMENT       # NULL camera
    assert b"camera" in capi.lib.rt_last_error_message()
    assert _camera_call(entry, handle, cam, None, 1, out) == capi.RT_ERR_INVALID_ARGUMENT           # NULL regions
    assert _camera_call(entry, handle, cam, regions, 1, None) == capi.RT_ERR_INVALID_ARGUMENT       # NULL output
    assert _camera_call(entry, handle, cam, regions, 0, out) == capi.RT_ERR_INVALID_ARGUMENT        # n_tiles == 0
    assert _camera_call(entry, handle, cam, regions, 1, out, (0, 48, 1)) == capi.RT_ERR_INVALID_ARGUMENT      # width 0
    for name, c in bad_cameras():
        assert _camera_call(entry, handle, _cam(c), regions, 1, out) == capi.RT_ERR_INVALID_ARGUMENT, name
        assert b"camera" in capi.lib.rt_last_error_message(), name


def test_a_bad_region_is_reported_before_any_device_is_touched():
    # a valid camera gets as far as the tile table, which no region outside the image passes; a left-handed basis within the bound is
    # accepted (it reaches the same tile table check)
    _keep, handle = _stand_in()
    out = ctypes.create_string_buffer(64 * 48 * 4)
    left = list(IDENTITY); left[3:6] = (-1.0, 0.0, 0.0)
    skew = list(IDENTITY); skew[9:12] = (0.0, float(np.sqrt(1 - 0.02 ** 2)), 0.02)          # det / product = 0.02
    for cam in (IDENTITY, left, skew):
        for entry in ("rt_render_camera", "rt_render_camera_device"):
            for reg in ((0, 49, 64, 0), (0, 48, 65, 0), (10, 48, 10, 0), (0, 20, 64, 20)):
                regions = (capi.Region * 1)(capi.Region(*reg))
                assert _camera_call(entry, handle, _cam(cam), regions, 1, out) == capi.RT_ERR_INVALID_REGION, (entry, reg, cam)


def test_the_trace_kernels_keep_eight_waves_per_simd(tmp_path):
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_trace_rays<")]
        assert sorted(flavours) == sorted("rt::k_trace_rays<%s, %s, %d>" % (t, c, s) for t in ("float", "double")
                                          for c in ("true", "false") for s in (0, 1)), flavours
        for n in flavours:
            assert k[n]["scratch"] == 0, (n, k[n])
            if ", false, " in n:
                assert k[n]["sgpr"] <= 80 and k[n]["vgpr"] <= 64, (n, k[n])


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_look_at_gives_the_identity_camera_and_scales_the_field_of_view(precision):
    R = np.float32 if precision == rta.RT_F32 else np.float64
    cam = rta.look_at((0, 0, -4), (0, 0, 0), precision=precision)
    assert cam.dtype == R and cam.shape == (12,)
    bits = np.uint32 if R == np.float32 else np.uint64
    np.testing.assert_array_equal(cam.view(bits), np.array(IDENTITY, dtype=R).view(bits))       # +0, never -0
    # hfov: forward scaled to 0.5 / tan(hfov / 2); the reference's own view is 2 atan(0.5)
    for hfov in (30.0, 90.0, 120.0):
        c = rta.look_at((0, 0, -4), (0, 0, 0), hfov_deg=hfov, precision=precision)
        assert c[11] == R(0.5 / np.tan(np.radians(hfov) / 2)) and list(c[3:9]) == [1, 0, 0, 0, 1, 0]
    c = rta.look_at((0, 0, -4), (0, 0, 0), hfov_deg=np.degrees(2 * np.arctan(0.5)), precision=precision)
    assert abs(float(c[11]) - 1.0) < 1e-6
    # an orbit view: an orthonormal, right-handed basis (right = up x forward), forward towards the target
    c = rta.look_at((3.0, 2.0, -5.0), (0.0, -0.5, 0.0), up=(0, 1, 0), precision=precision).astype(np.float64)
    r, u, f = c[3:6], c[6:9], c[9:12]
    for v in (r, u, f):
        assert abs(np.linalg.norm(v) - 1) < 1e-6
    assert abs(r @ u) < 1e-6 and abs(r @ f) < 1e-6 and abs(u @ f) < 1e-6
    assert np.allclose(np.cross(u, f), r, atol=1e-6) and u[1] > 0
    np.testing.assert_allclose(f, -np.array([3.0, 2.5, -5.0]) / np.linalg.norm([3.0, 2.5, -5.0]), atol=1e-6)


def test_look_at_rejects_degenerate_views():
    with pytest.raises(ValueError):
        rta.look_at((1, 2, 3), (1, 2, 3))                     # eye == target
    with pytest.raises(ValueError):
        rta.look_at((0, 0, 0), (0, 5, 0))                     # up parallel to the view
    with pytest.raises(ValueError):
        rta.look_at((0, 0, 0), (0, -5, 0), up=(0, 2, 0))      # ... antiparallel
    with pytest.raises(ValueError):
        rta.look_at((0, 0, 0), (0, 0, 1), up=(0, 0, 0))       # no up at all
    with pytest.raises(ValueError):
        rta.look_at((0, 0, 0), (0, 0, 1), hfov_deg=180.0)
