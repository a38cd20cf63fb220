"""Multi-hit ray queries (rt_intersect_rays_multi / rt_intersect_rays_multi_device, csrc/rt_multihit.hpp) without a GPU: the ABI, the
argument checks made before any device is touched, the residency of the kernel's flavours read back from the code object, and the
checks DeviceScene.intersect_multi makes before it calls the library."""
import ctypes

import numpy as np
import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from rust_tracer_amd.scene import DeviceScene
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB

BUCKETS = (1, 4, 8, 16)


def test_both_libraries_export_the_multihit_entries_at_abi_5():
    assert capi.ABI_VERSION == 5
    assert {"rt_intersect_rays_multi", "rt_intersect_rays_multi_device"} <= set(capi.SYMBOLS)
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert lib.rt_abi_version() == 5
        assert lib.rt_intersect_rays_multi is not None and lib.rt_intersect_rays_multi_device is not None
    assert (rta.RT_MULTIHIT_CLOSEST, rta.RT_MULTIHIT_ALL, rta.RT_MULTIHIT_MAX_K) == (0, 1, 16)


def _call(entry, scene, mode, k, rays, n, dist, hits=None):
    f = getattr(capi.lib, entry)
    if entry == "rt_intersect_rays_multi":
        return f(scene, mode, k, rays, None, n, dist, None, None, hits, None)
    return f(scene, mode, k, rays, None, n, dist, None, None, hits, None, None)


@pytest.mark.parametrize("entry", ["rt_intersect_rays_multi", "rt_intersect_rays_multi_device"])
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check pointers, n, k, the mode and alignment before they look at the scene: a stand-in handle is never read here
    stand_in = ctypes.create_string_buffer(4096)
    rays = (ctypes.c_float * 6)(0, 0, 0, 0, 0, 1)
    dist = (ctypes.c_float * 16)()
    hits = (ctypes.c_uint32 * 4)()
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    closest = capi.RT_MULTIHIT_CLOSEST
    bad = capi.RT_ERR_INVALID_ARGUMENT
    assert _call(entry, None, closest, 4, rays, 1, dist) == bad                # NULL scene
    assert _call(entry, handle, closest, 4, None, 1, dist) == bad              # NULL rays
    assert _call(entry, handle, closest, 4, rays, 1, None) == bad              # NULL distance_out
    assert _call(entry, handle, closest, 4, rays, 0, dist) == bad              # n == 0
    for k in (0, 17, 1 << 20):
        assert _call(entry, handle, closest, k, rays, 1, dist) == bad          # k outside 1 .. RT_MULTIHIT_MAX_K
        assert b"k must be" in capi.lib.rt_last_error_message()
    for mode in (2, -1, 7):
        assert _call(entry, handle, mode, 4, rays, 1, dist) == bad             # unknown mode
        assert b"mode" in capi.lib.rt_last_error_message()
    misaligned = ctypes.c_void_p(ctypes.addressof(hits) + 1)
    assert _call(entry, handle, closest, 4, rays, 1, dist, misaligned) == bad  # misaligned hits_out
    assert b"hits_out" in capi.lib.rt_last_error_message()


def test_the_multihit_flavours_and_their_residency(tmp_path):
    # every flavour exists in both libraries without scratch; capacities up to 4 keep eight waves per SIMD, larger ones four or more
    want = sorted("rt::k_multihit_rays<%s, %s, %s, %d>" % (t, c, a, b) for t in ("float", "double") for c in ("true", "false")
                  for a in ("true", "false") for b in BUCKETS)
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_multihit_rays<")]
        assert sorted(flavours) == want, flavours
        for n in flavours:
            b = int(n.rstrip(">").split(",")[-1])
            r = k[n]
            assert r["scratch"] == 0, (n, r)
            if b <= 4:
                assert r["sgpr"] <= 80 and r["vgpr"] <= 64, (n, r)
            else:
                assert r["vgpr"] <= 128, (n, r)


class _Stand:
    """Enough of a Scene for DeviceScene's checks, which come before any call into the library."""
    def __init__(self, precision):
        self.precision = precision


def _device_scene(precision):
    d = DeviceScene.__new__(DeviceScene)
    d.scene, d.device, d._h = _Stand(precision), 0, None
    return d


@pytest.mark.parametrize("precision", [rta.RT_F32, rta.RT_F64], ids=["f32", "f64"])
def test_intersect_multi_checks_shapes_and_dtypes_before_the_library(precision):
    R = np.float32 if precision == rta.RT_F32 else np.float64
    other = np.float64 if R == np.float32 else np.float32
    d = _device_scene(precision)
    good = np.array([[0, 0, -4, 0, 0, 1]] * 3, dtype=R)
    for k in (0, 17, -1):
        with pytest.raises(ValueError, match="k must be"):
            d.intersect_multi(good, k)
    for rays in (good.astype(other), good[:, :5], good[:0], good.reshape(-1), good.tolist()):
        with pytest.raises(ValueError, match="rays"):
            d.intersect_multi(rays, 4)
    with pytest.raises(ValueError, match="tmax"):
        d.intersect_multi(good, 4, tmax=np.ones(3, dtype=other))
    with pytest.raises(ValueError, match="tmax"):
        d.intersect_multi(good, 4, tmax=np.ones(2, dtype=R))
    n, k = 3, 4
    ok = (np.empty((n, k), R), np.empty((n, k, 3), R), np.empty((n, k), np.int32), np.empty(n, np.uint32))
    wrong = [
        ok[:3],                                                                        # hits missing
        (np.empty((n, k + 1), R),) + ok[1:],                                           # distance for another k
        (ok[0], np.empty((n, k, 3), other)) + ok[2:],                                  # normal of the other REAL
        ok[:2] + (np.empty((n, k), np.int64), ok[3]),                                  # item not int32
        ok[:3] + (np.empty(n, np.int32),),                                             # hits not uint32
        (np.empty((k, n), R).T,) + ok[1:],                                             # not contiguous
    ]
    for out in wrong:
        with pytest.raises(ValueError, match="out"):
            d.intersect_multi(good, k, out=out)
