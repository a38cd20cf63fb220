/*
 * rt_debug.h -- diagnostic controls of librtrace_hip.so.  NOT part of the drop-in ABI (include/rtrace_hip.h): nothing a
 * renderer needs is here, and the library reads no environment variable.  The parity tests and tools/ use these to pick a
 * traversal-loop flavour or switch an optimisation off and prove that no byte and no counter changes.
 *
 * Every control is process-wide and atomic; set it between calls, not during one.
 */
#ifndef RTRACE_HIP_DEBUG_H
#define RTRACE_HIP_DEBUG_H

#include "../../include/rtrace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rt_debug_key {
    RT_DEBUG_SKIP_VARIANT = 0,   /* k_render_skip VAR bits (rt_skip.hpp): 0/1 C++ loops, 3 generated assembly loops, 7 their fused
                                    flavour (dropped for scenes that are not concentric), + 16 the filtered loops (f32: a conservative
                                    bound in front of every test).  Default 23 */
    RT_DEBUG_BLOCK_ORDER = 1,    /* 0: dispatch a pass's blocks in raster order instead of most-expensive-first.  Default 1 */
    RT_DEBUG_NARROW_MAX = 2,     /* cap on the number of blocks dealt out as narrow workgroups (read when a tile list is first seen) */
    RT_DEBUG_PACKED_SAMPLES = 3, /* 0: spp 2/4/8 use the plain sample-parallel mapping.  Default 1 */
    RT_DEBUG_PRINT_STEPS = 4,    /* 1: a counted call prints its node-step statistics on stderr */
    RT_DEBUG_PRINT_COSTS = 5,    /* 1: print the block cost estimates when a dispatch order is built */
    RT_DEBUG_HOST_COPY = 6,      /* how rt_render_tiles returns bytes to host memory: 0 the library's choice, 1 one copy to the
                                    caller's pointer, 2 pinned staging + CPU copy, 3 the kernel stores into pinned host memory */
    RT_DEBUG_COALESCE = 7,       /* 0: concurrent rt_render_region calls are not merged into shared passes; n > 0: at most n merged passes in flight.  Default 2 */
    RT_DEBUG_LDS_BYTES = 8,      /* dynamic LDS reserved per render workgroup: caps the waves per SIMD (160 KiB / n workgroups per CU) for
                                    occupancy experiments; the kernels do not touch it */
    RT_DEBUG_WG_POLICY = 9,      /* 0: one workgroup per block and sample (the dispatcher deals); n > 0: n x 2,048 workgroups per launch, blocks
                                    dealt on the host; default: dealt only past 32,768 workgroups (read when a tile list is first seen) */
    RT_DEBUG_NARROW_L2 = 10,     /* of the narrow blocks, how many of the most expensive go out as sixteen 2x2-pixel-per-wave workgroups
                                    (the rest as four 4x4 ones); default: all in a pass of <= 4,096 blocks, none otherwise */
    RT_DEBUG_FLAT_KERNELS = 11,  /* 0: the f32 flat traversal runs round 1's LDS-staged packed-math kernels (rt_flat_wf.hpp, what f64 always
                                    runs) instead of the scalar-fed scan (rt_flat_sc.hpp) */
    RT_DEBUG_SKIP_RAYS = 12,     /* rays per lane of the f32 hierarchy walk (assembly loops): 1 = k_render_skip always; 2 = k_render_skip2 (two rays per lane on
                                    packed math, rt_skip2.hpp) wherever it exists (spp 1, 2, 4, 8; launches that do not count tests);
                                    default: the library's choice per workload (large spp-1 frames, large scenes) */
    RT_DEBUG_FRAME_AHEAD = 13,   /* 0: rt_render_region never serves a bucket from a whole-grid pass rendered ahead (every call its own device pass,
                                    or merged with concurrent ones: RT_DEBUG_COALESCE); 1: whole-grid passes, each rendered when its frame is first
                                    asked for; default (2): the pass for the next frame is started as soon as the current one is being handed out */
    RT_DEBUG_FILTER_RO_PERCENT = 14, /* read by rt_scene_create: the radius around the scene's centroid in which the filtered loops' bounds cover
                                    shadow-ray origins, in percent of the library's own value.  A small value leaves real origins
                                    uncovered -- they must then fall back to the reference's arithmetic at every node (tests).  Default 100 */
    RT_DEBUG_COOP = 15,          /* the lane-cooperative walk of the heaviest quads (rt_coop.hpp; read when a tile list is first seen): 0 never,
                                    1 asked for at the default threshold (40 % of the pass's largest estimate) without the trial, 2 every quad of
                                    every block (parity tests); default: the library TRIES thresholds of 28 / 34 / 40 / 48 / 58 % against the plain
                                    dispatch over a list's first launches and keeps the fastest (rt_capi.hip build_orders, pick_order) */
    RT_DEBUG_COOP_THR = 16,      /* ... the cost-map value (tests per pixel) from which a quad is walked cooperatively; default: see RT_DEBUG_COOP */
    RT_DEBUG_COOP_MAX = 17,      /* ... cap on the number of 16x16 blocks that are split for it; default: an eighth of the pass */
    RT_DEBUG_COOP_LEVEL = 18,    /* ... rays per cooperative wave: 1 = 16 (4x4 pixels), 2 = 4 (2x2), 3 = one; default 2 */
    RT_DEBUG_COOP_REST = 19,     /* ... what is left of a block with cooperative quads: 0 = one descriptor (8x8 pixels per wave), 1 = four (4x4 per wave) */
    RT_DEBUG_ASYNC_ORDERS = 20,  /* 0: the dispatch orders of a tile list (and the scene's cost map) are made by the first call that uses the list, as they are
                                    whenever another dispatch control here is set; default: by a background thread, the first launches finding their blocks
                                    through the tile table */
    RT_DEBUG_FAST_KERNEL = 21,   /* the lean kernels (rt_skip_fast.hpp f32, rt_skip_fast64.hpp f64, rt_skip2_fast.hpp two rays per lane: one mode each, arguments fetched
                                    where they are needed): 0 never -- the generic kernels --, 2 wherever one exists; default: f32 where the list has cooperative
                                    quads, f64 every ordered spp-1 launch, two rays per lane every launch with a dispatch list but a dealt list of a
                                    plain-stream scene.  All must render the same bytes */
    RT_DEBUG_EXACT_COSTS = 22,   /* 0: cooperative quads are picked by the scene's 256 x 256 cost map only (small passes), not by counting a tile list's heaviest
                                    blocks again at the frame's own resolution (rt_capi.hip exact_block_costs).  Default 1 (read when a tile list is first seen) */
    RT_DEBUG_MULTIHIT_BUCKET = 23, /* the list capacity of rt_intersect_rays_multi* and rt_near_spheres* (rt_multihit.hpp, rt_near.hpp: 1, 4, 8 or 16) when it is >= k; default (and any
                                    other value): the smallest one >= k.  Every capacity must give the same bytes */
    RT_DEBUG_TIGHT_BOUNDS = 24,  /* the tight streams of an f32 scene (rt_tight.hpp: BOUND nodes carry a smaller sphere around their subtree's items; the un-fused filtered
                                    loops walk them): 0 never, 1 the library's rule, 2 wherever a scene has tight streams -- 1 and 2 make them at the launch if
                                    the scene's worker has not yet; default: the rule, from the launch on that finds them made.  All must render the same bytes */
    RT_DEBUG_TIGHT_COSTS = 25,   /* which costs the dispatch orders of a list whose launches walk the tight streams are built from (read when a tile list is first
                                    seen): 0 the given streams' (what every other list gets; A/B runs); default: the tight streams' */
    RT_DEBUG_WALK_BOUNDS = 26,   /* the per-walk streams of an f32 scene (rt_tight.hpp build_walk: an eye sphere with T' for the primary walk, a light disc for the
                                    shadow walk), for launches that walk the tight streams: 0 never, 1 the library's rule, 2 wherever a scene has them -- 1 and 2
                                    make them at the launch if the scene's worker has not yet; default: the rule, from the launch on that finds them made.
                                    All must render the same bytes */
    RT_DEBUG_LEAN_BOUNDS = 27,   /* the lean BOUND step of the per-walk primary stream (rt_filter_bounds.hpp lean_radius: a BOUND with an eye sphere carries Rq and is
                                    decided from the filter's b' alone), read when a scene's per-walk streams are made: 0 never -- the build kernel writes no flag --,
                                    1 the library's rule, 2 wherever a record exists; default: the rule, which is every eye sphere.  All must render the same bytes */
    RT_DEBUG_KEYS = 28
} rt_debug_key;

/* value < 0 restores the default. */
rt_status rt_debug_set(int key, long long value);

/* Process-wide event counts since load (diagnostic): how the merged rt_render_region passes went. */
typedef enum rt_debug_counter {
    RT_DEBUG_COUNT_REGION_CALLS = 0,    /* rt_render_region calls that went through the merging path */
    RT_DEBUG_COUNT_REGION_PASSES = 1,   /* device passes they were rendered in */
    RT_DEBUG_COUNT_FILTER_PASS = 2,     /* f32 hierarchy walk, calls that return rt_stats: per-ray tests the filtered loops' bound lets through */
    RT_DEBUG_COUNT_FILTER_VIOLATIONS = 3,   /* ... and tests with a finite distance that the bound would have ruled out: must stay 0 */
    RT_DEBUG_COUNT_PRIMARY_TESTS = 4,   /* hierarchy walk: of the LAST call that returned rt_stats, the tests (items + bounds) made for primary rays
                                           (the rest of sphere_tests + bound_tests were made for shadow rays); not cumulative */
    RT_DEBUG_COUNT_FRAME_AHEAD_PASSES = 5,  /* whole-grid passes rendered for rt_render_region's frame-ahead */
    RT_DEBUG_COUNT_TWO_RAY_LAUNCHES = 6,    /* hierarchy-walk passes that ran k_render_skip2 (two rays per lane) instead of k_render_skip */
    RT_DEBUG_COUNT_COOP_LAUNCHES = 7,       /* hierarchy-walk passes whose launch carried cooperative quads (k_render_skip<..., COOP>) */
    RT_DEBUG_COUNT_TIGHT_VIOLATIONS = 8,    /* counting launches of an f32 scene that has tight streams: ITEM tests that counted where a tight bound would have put the
                                               lane to sleep (also added to RT_DEBUG_COUNT_FILTER_VIOLATIONS): must stay 0 */
    RT_DEBUG_COUNT_TIGHT_RECOUNTS = 9,      /* exact recounts of a tile list's heaviest blocks that walked the scene's TIGHT streams (exact_block_costs) */
    RT_DEBUG_COUNTERS = 10
} rt_debug_counter;
long long rt_debug_count(int counter);

/* Per-wave timeline (tools/wave_timeline.py): while a path is set, every launch of the assembly loops records each wave's
 * start / end / placement and writes the records to the file (synchronous, overwritten per launch).  NULL switches it off. */
rt_status rt_debug_wave_trace(const char *path);

/* Test infrastructure for the flat scan's conservative filter (rt_flat_sc.hpp, flat_filter_constant): evaluates, for every primary
 * ray of a width x height x spp frame and every item of an f32 scene, the exact discriminant and the filter's bound.
 * counts = { pairs with disc >= 0, pairs with bound >= 0, pairs with disc >= 0 but bound < 0 } for the primary filter, then the same
 * three for the shadow filter on rays from a point of each primary ray towards the light: counts[2] and counts[5] must be 0. */
rt_status rt_debug_flat_filter_check(rt_scene *scene, uint32_t width, uint32_t height, uint32_t spp, unsigned long long counts[6]);

/* Test infrastructure for the tight streams (rt_tight.hpp), host only -- no device is looked for: the sphere every bound of an f32 scene with these
 * arguments (rt_scene_create's) carries in the tight streams, spheres_out[4 * n_bounds], and whether it is a tight one (1) or the given one, bit
 * for bit (0), tight_out[n_bounds].  consts_out (optional): { S, eta, summed-volume ratio tight / given, the selection rule's verdict: 0 never, 1 every launch that can, 2 one-sample passes of a million pixels or more }. */
rt_status rt_debug_tight_bounds(const float *dfs_items, uint32_t n_items, const float *light_unit, const float *eye, const float *bounds, const rt_range *ranges,
                                uint32_t n_bounds, float *spheres_out, uint8_t *tight_out, double consts_out[4]);
/* ... and for the per-walk streams (rt_tight.hpp build_walk), host only: per bound, records_out[12 * n_bounds] = { the sphere the primary per-walk stream
 * carries (4), the threshold it carries, T', w1', w2', cl', R2o', R2i', flags (1: eye sphere, 2: light disc) }.  slack = 0 takes the rounding terms out of
 * T', R2o' and cl' (what the rim fixtures must catch).  frame_out (optional): FilterConsts { m0, e1, e2, l (3 each), a0, k1, kc, ro2, S, eta }, then the
 * mean cone half-angle and disc radius of the records relative to the tight ball's. */
rt_status rt_debug_walk_bounds(const float *dfs_items, uint32_t n_items, const float *light_unit, const float *eye, const float *bounds, const rt_range *ranges,
                               uint32_t n_bounds, int slack, float *records_out, double frame_out[20]);
/* ... and for the lean BOUND step: the same records (slack 1) and rq_out[n_bounds], Rq of every bound with an eye sphere (0: none -- such a bound keeps
 * the reference's test).  The un-fused filtered f32 primary loop enters such a bound iff b' >= T' and b' - Rq < hit.distance. */
rt_status rt_debug_lean_bounds(const float *dfs_items, uint32_t n_items, const float *light_unit, const float *eye, const float *bounds, const rt_range *ranges,
                               uint32_t n_bounds, float *records_out, float *rq_out);

/* Test infrastructure for the multi-GPU paths.  rt_debug_gang_layout: the sharding arithmetic of rt_gang_render_frame(s) without a
 * device -- for bucket i its device (i % n_devices) and its first pixel inside that device's tile-major shard; per device the pixels
 * of its shard; the padded shard length every device sends.  rt_debug_shard_costs: what the scene's cost map predicts for the shards
 * (sum of tests per pixel under each device's buckets): cost[n_devices]. */
rt_status rt_debug_gang_layout(const rt_region *tiles, uint32_t n_tiles, uint32_t n_devices, uint32_t *device_of, uint32_t *px_offset,
                               uint64_t *shard_px, uint64_t *padded_px);
/* A stand-in for librccl.so (tests/c/fake_rccl.cpp), by path: gangs created while it is set bind ITS ncclCommInitAll / ncclGroupStart / ncclGather /
 * ... instead of librccl.so's and may list one device several times (several ranks on one GPU) -- how the N > 1 code of rt_gang_* is
 * executed on a one-GPU box.  NULL: librccl.so again.  A gang keeps the library it was created with. */
rt_status rt_debug_rccl_library(const char *path);
rt_status rt_debug_shard_costs(rt_scene *scene, const rt_options *options, const rt_region *tiles, uint32_t n_tiles, uint32_t n_devices, double *cost);
/* The scene's 256 x 256 cost map (tests per primary ray, its shadow ray included), out[65536]: tight = 0 counted on the scene's given streams,
 * tight = 1 on its tight streams (made here if nobody made them yet; RT_ERR_UNSUPPORTED for a scene that gets none).  Either map is counted
 * once per scene, by whoever asks first. */
rt_status rt_debug_cost_map(rt_scene *scene, int tight, uint32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* RTRACE_HIP_DEBUG_H */
