"""rust-tracer_amd: MI355X (gfx950) backend for rust-tracer's per-pixel ray-sphere hot path.

Layout: csrc/ (hand-written HIP kernels + C ABI -> librtrace_hip.so), capi.py (ctypes binding of
include/rtrace_hip.h), scene.py / render.py (host-side mirror of the reference's Scene / Renderer surface),
dist.py (tile sharding across GPUs + RCCL gather).  Importing this package requires the built library."""
from . import capi
from .capi import (RT_F32, RT_F64, RT_TRAVERSAL_FLAT, RT_TRAVERSAL_SKIP, RT_QUERY_NEAREST, RT_QUERY_ANY, RT_MULTIHIT_CLOSEST, RT_MULTIHIT_ALL,
                   RT_MULTIHIT_MAX_K, RT_UNDERSAMPLE_MAX_STEP, RT_NEAR_CLOSEST, RT_NEAR_ALL, RT_NEAR_MAX_K, RT_SWEEP_NEAREST, RT_SWEEP_ANY, RtError, device_count)
from .scene import Scene, DeviceScene, Gang, ray_keys, sphere_keys, balanced_ranges, balanced_ranges_reference, refit_bounds, sphere_gaps, sweep_distances, pair_gaps, overlap_gaps, box_gaps, region_gaps, box_planes, camera_planes, region_sections, pair_impacts, pair_islands, impact_scale, swept_times, swept_normals, pyramid, normalized, build_hierarchy, look_at, expand_undersampled, undersample_cells, progressive_steps
from .render import (RenderOptions, ImageRegion, RGBABuffer, RGBABufferWriter, PPMStdoutRGBABufferWriter,
                     Renderer, buckets, CHUNK_SIZE)

__all__ = ["capi", "RT_F32", "RT_F64", "RT_TRAVERSAL_FLAT", "RT_TRAVERSAL_SKIP", "RT_QUERY_NEAREST", "RT_QUERY_ANY", "RT_MULTIHIT_CLOSEST", "RT_MULTIHIT_ALL",
           "RT_MULTIHIT_MAX_K", "RT_UNDERSAMPLE_MAX_STEP", "RT_NEAR_CLOSEST", "RT_NEAR_ALL", "RT_NEAR_MAX_K", "RT_SWEEP_NEAREST", "RT_SWEEP_ANY", "RtError", "device_count",
           "Scene", "DeviceScene", "Gang", "pyramid", "normalized", "build_hierarchy", "look_at", "expand_undersampled", "undersample_cells",
           "progressive_steps", "ray_keys", "sphere_keys", "balanced_ranges", "balanced_ranges_reference", "refit_bounds", "sphere_gaps", "sweep_distances", "pair_gaps", "overlap_gaps", "box_gaps", "region_gaps", "box_planes", "camera_planes", "region_sections", "pair_impacts", "pair_islands", "impact_scale", "swept_times", "swept_normals", "RenderOptions", "ImageRegion", "RGBABuffer",
           "RGBABufferWriter", "PPMStdoutRGBABufferWriter", "Renderer", "buckets", "CHUNK_SIZE"]
