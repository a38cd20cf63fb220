"""Ray queries (rt_intersect_rays / rt_intersect_rays_device, csrc/rt_query.hpp) without a GPU: the ABI, the argument checks made before
any device is touched, and the residency of the query kernels read back from the code object."""
import ctypes

import pytest

import rust_tracer_amd as rta
from rust_tracer_amd import capi
from tests.test_kernel_resources import _kernels, LIB, TEST_LIB


def test_both_libraries_export_the_query_entries_at_abi_5():
    assert capi.ABI_VERSION == 5
    assert {"rt_intersect_rays", "rt_intersect_rays_device"} <= set(capi.SYMBOLS)
    for path in (capi.PRODUCT_LIB_PATH, capi.TEST_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert lib.rt_abi_version() == 5
        assert lib.rt_intersect_rays is not None and lib.rt_intersect_rays_device is not None
    assert (rta.RT_QUERY_NEAREST, rta.RT_QUERY_ANY) == (0, 1)


def _call(entry, scene, mode, rays, n, dist):
    f = getattr(capi.lib, entry)
    if entry == "rt_intersect_rays":
        return f(scene, mode, rays, None, n, dist, None, None, None)
    return f(scene, mode, rays, None, n, dist, None, None, None, None)


@pytest.mark.parametrize("entry", ["rt_intersect_rays", "rt_intersect_rays_device"])
def test_argument_errors_are_reported_before_any_device_is_touched(entry):
    # the entries check their pointers, n and the mode before they look at the scene: a stand-in handle is never read here
    stand_in = ctypes.create_string_buffer(4096)
    rays = (ctypes.c_float * 6)(0, 0, 0, 0, 0, 1)
    dist = (ctypes.c_float * 1)()
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    assert _call(entry, None, capi.RT_QUERY_NEAREST, rays, 1, dist) == capi.RT_ERR_INVALID_ARGUMENT          # NULL scene
    assert _call(entry, handle, capi.RT_QUERY_NEAREST, None, 1, dist) == capi.RT_ERR_INVALID_ARGUMENT        # NULL rays
    assert _call(entry, handle, capi.RT_QUERY_NEAREST, rays, 1, None) == capi.RT_ERR_INVALID_ARGUMENT        # NULL distance_out
    assert _call(entry, handle, capi.RT_QUERY_NEAREST, rays, 0, dist) == capi.RT_ERR_INVALID_ARGUMENT        # n == 0
    for mode in (2, -1, 7):
        assert _call(entry, handle, mode, rays, 1, dist) == capi.RT_ERR_INVALID_ARGUMENT                      # unknown mode
    assert b"mode" in capi.lib.rt_last_error_message()


def test_the_query_kernels_keep_eight_waves_per_simd(tmp_path):
    for path in (LIB, TEST_LIB):
        k = _kernels(tmp_path, path)
        flavours = [n for n in k if n.startswith("rt::k_query_rays<")]
        assert sorted(flavours) == sorted("rt::k_query_rays<%s, %s, %s>" % (t, c, a) for t in ("float", "double")
                                          for c in ("true", "false") for a in ("true", "false")), flavours
        for n in flavours:
            assert k[n]["sgpr"] <= 80 and k[n]["vgpr"] <= 64 and k[n]["scratch"] == 0, (n, k[n])



def test_one_tmax_value_is_rounded_to_the_scenes_real_and_arrays_must_match():
    import numpy as np
    from rust_tracer_amd.scene import _tmax_array
    t = _tmax_array(1.5, np.float32, 3)
    assert t.dtype == np.float32 and t.flags.c_contiguous and list(t) == [1.5, 1.5, 1.5]
    assert _tmax_array(np.float64(0.1), np.float32, 2).tolist() == [np.float32(0.1)] * 2
    assert _tmax_array(2, np.float64, 1).dtype == np.float64
    assert list(_tmax_array(np.array([1, 2], dtype=np.float32), np.float32, 2)) == [1, 2]
    for bad in (np.array([1.0, 2.0]), np.zeros(3, dtype=np.float32)):      # float64 array on an f32 scene; wrong length
        with pytest.raises(ValueError):
            _tmax_array(bad, np.float32, 2)
