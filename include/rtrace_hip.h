/*
 * rtrace_hip.h -- C ABI of the MI355X (gfx950) backend for rust-tracer's per-tile hot path.
 *
 * Drop-in seam (there is no FFI in the reference today; this is the natural one):
 * the body of the closure the bucket scheduler hands to its thread pool,
 *
 *     /root/reference/src/rust/render.rs:283-294
 *         let mut b = RGBABuffer::new(&ImageRegion{l: x, r: x + 64, b: y, t: y + 64});
 *         Renderer::render_region(&opts, tscene.deref(), &mut b);          // render.rs:218-255
 *         tx.send(b)
 *
 * i.e. `pub fn render_region(o: &RenderOptions, scene: &Scene, buf: &mut RGBABuffer)` and everything it
 * calls (Renderer::raytrace render.rs:171-215, TypedGroup::intersect group.rs:72-83,
 * Sphere::intersect / distance_from_ray primitive.rs:55-84, RGBABuffer::set_pixel_from_vector render.rs:92-109).
 * A Rust maintainer binds these symbols from an `extern "C"` block (INTEGRATION.md shows the block);
 * plain pointers and sizes only, no C++ or torch types, never unwinds, returns integer status codes
 * where the reference panics.
 *
 * Results: the RGBA bytes are bit-identical to the reference CPU path for the same Scene / RenderOptions /
 * ImageRegion (f32; every + - * / sqrt individually rounded, no FMA contraction, reference operation order).
 *
 * Threading: every entry point may be called concurrently from several host threads on one rt_scene*
 * (the reference calls render_region from up to RTRACEMAXPROCS pool threads, render.rs:283); each call
 * works on its own HIP stream and workspace.
 */
#ifndef RTRACE_HIP_H
#define RTRACE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTRACE_HIP_ABI_VERSION 5

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARGUMENT = 1,  /* NULL pointer, n == 0, width or height 0, non-finite / non-positive-radius sphere ... (NOT
                                     samples_per_pixel == 0: that is the reference's black frame, see rt_options)           */
    RT_ERR_INVALID_REGION = 2,    /* region outside the image or t <= b / r <= l  (reference: assert!/index panic)  */
    RT_ERR_NO_DEVICE = 3,         /* no gfx950 device visible, or device index out of range                        */
    RT_ERR_HIP = 4,               /* a HIP runtime call or kernel launch failed; rt_last_error_message() has detail */
    RT_ERR_OUT_OF_MEMORY = 5,
    RT_ERR_UNSUPPORTED = 6        /* e.g. RT_TRAVERSAL_SKIP on a scene created without subtree bounds              */
} rt_status;

/* `pub type RFloat = f32` (vec.rs:6).  RT_F64 is the type-alias swap of BASELINE config 3 (every hard-coded
 * f32 constant promoted); the reference pins nothing for it. */
typedef enum rt_precision { RT_F32 = 0, RT_F64 = 1 } rt_precision;

/* How a ray visits the items.  Both give the reference's pixels on scenes whose bounds enclose their
 * subtrees and whose eye lies outside every bound (the default scene).
 *   FLAT : every item in DFS order, strict `<` nearest for primary rays, any-hit for shadow rays.
 *   SKIP : the same DFS array plus the reference's own group bounds as skip ranges, culled per ray with the
 *          reference's rule `bound.distance_from_ray(ray) >= hit.distance` (group.rs:73) -- reproduces the
 *          hierarchy exactly, including its inside-the-bound behaviour. */
typedef enum rt_traversal { RT_TRAVERSAL_FLAT = 0, RT_TRAVERSAL_SKIP = 1 } rt_traversal;

/* RenderOptions, render.rs:33-38 (u16 fields there too).  samples_per_pixel = k means k*k samples; k = 0 is the reference's black
 * frame (no sample taken, 0 * inf = NaN, `NaN as u8` = 0: every listed pixel {0, 0, 0, 0}).  width and height must be >= 1 at this
 * boundary: an empty image has no bucket to hand over (the host scheduler returns before calling, like render.rs:273-298). */
typedef struct rt_options {
    uint16_t width, height, samples_per_pixel;
} rt_options;

/* ImageRegion, render.rs:42-48: pixels x in [l, r), y in [b, t); y = 0 is the TOP image row and row 0 of
 * the tile buffer is y == b (buffer_offset render.rs:69-71). */
typedef struct rt_region {
    uint16_t l, t, r, b;
} rt_region;

/* A group's bound and the contiguous range of DFS item indices of its subtree (for RT_TRAVERSAL_SKIP). */
typedef struct rt_range {
    int32_t first, count;
} rt_range;

/* Ray counters with the reference's meaning (they must equal the CPU path's exactly) + device time. */
typedef struct rt_stats {
    uint64_t primary;       /* primary samples traced = sum(area) * spp^2                    */
    uint64_t hits;          /* primary rays that hit an item                                 */
    uint64_t shadow;        /* shadow rays cast (hit and n.light < 0), render.rs:199-207      */
    uint64_t occluded;      /* shadow rays that hit something                                */
    uint64_t sphere_tests;  /* ray x item tests (FLAT: rays * n_items; SKIP: Sphere::intersect calls the
                               reference's traversal makes, shadow rays stopping at their first hit)        */
    uint64_t bound_tests;   /* bound.distance_from_ray calls (group.rs:73); 0 for FLAT          */
    uint64_t tests_executed;/* ray x record tests the kernels actually ran: SKIP = sphere_tests + bound_tests;
                               FLAT = primary * n_items + (shadow rays) * first chunk + (survivors) * rest --
                               the any-hit passes stop early, so FLAT's figure is below sphere_tests         */
    uint64_t primary_tests; /* of sphere_tests + bound_tests (FLAT: of sphere_tests), the tests made for PRIMARY rays; the rest were made
                               for shadow rays (8 vs 16 arithmetic operations per test with the ray-independent terms pre-formed)  */
    double device_ms;       /* hipEvent time of all kernels of this call on its stream.  A call that asks for
                               stats runs the counting flavour of the kernels (same bytes, about 2.5x slower):
                               it is not the product's speed -- time calls without stats with your own events */
    uint64_t longest_wave_cycles, longest_wave_ref100mhz;   /* (ABI 4; SKIP) the counting launch's longest wave on the shader clock (s_memtime) and on the
                               constant 100 MHz reference (s_memrealtime): cycles / ref100mhz * 100 = the clock in MHz that launch ran at.
                               Diagnostic -- what bench.py prices its roofline's peak at next to the nominal 2.4 GHz; 0 for FLAT */
} rt_stats;

typedef struct rt_scene rt_scene;   /* opaque: device copies of a Scene (render.rs:138-142) */

/* (ABI 4; host-side, touches no device) The automatic bounding-sphere hierarchy for an ARBITRARY sphere list -- SURVEY.md 8f.4; the reference has
 * no such builder (group.rs:28-65 builds its pyramid only), so this is an input generator, not reference arithmetic: median splits along the
 * longest axis until at most leaf_size spheres remain, near-minimal enclosing spheres as bounds, the half nearer to `eye` first (eye = NULL:
 * the split's own order).  The one implementation both hosts use (csrc/host/hierarchy.hpp).
 *   spheres     double[4 * n]: cx, cy, cz, radius
 *   items_out   REAL[4 * n]  in the tree's DFS order;  order_out uint64[n] (optional): items_out[k] = spheres[order_out[k]]
 *   bounds_out  REAL[4 * 2n], ranges_out rt_range[2n]: room for the at most 2n - 1 groups; *n_groups_out of them are written (DFS pre-order)
 * ready for rt_scene_create(dfs_items = items_out, bounds = bounds_out, ranges = ranges_out, n_bounds = *n_groups_out). */
rt_status rt_build_hierarchy(const double *spheres, uint32_t n, uint32_t leaf_size, const double *eye, rt_precision precision,
                             void *items_out, void *bounds_out, rt_range *ranges_out, uint64_t *order_out, uint32_t *n_groups_out);

/* Number of usable devices (RT_ERR_NO_DEVICE and *n = 0 when there is none). */
rt_status rt_device_count(int *n);

/* Uploads a Scene.  Replaces Arc<Scene> construction for the device side (render.rs:144-166, main.rs:23).
 *   dfs_items   REAL[4*n_items] = {cx,cy,cz,radius} in traversal (DFS, insertion) order -- the order
 *               TypedGroup::intersect visits Pair::Item children (group.rs:77-82); ties between items at
 *               exactly equal distance go to the first in this order (primitive.rs:79).
 *   light_unit  REAL[3] Scene::directional_light, already normalised by the host in REAL (render.rs:154-159).
 *   eye         REAL[3] Scene::eye.
 *   bounds/ranges/n_bounds  optional (NULL/NULL/0): group bounds REAL[4*n_bounds] with their item ranges in DFS
 *               pre-order (outer group before the groups nested in it); required for RT_TRAVERSAL_SKIP.
 * REAL is float for RT_F32 and double for RT_F64.  All values must be finite, |coordinate| <= 1e15 (items, bounds, eye),
 * radius > 0, light_unit of squared length within 2e-3 of 1 (RT_ERR_INVALID_ARGUMENT otherwise): within these bounds no
 * intermediate of the path overflows, so no NaN can arise and every comparison agrees with the reference's whichever way it is written.
 * The caller keeps ownership of every host buffer; nothing is retained but the returned handle. */
rt_status rt_scene_create(int device, rt_precision precision,
                          const void *dfs_items, uint32_t n_items,
                          const void *light_unit, const void *eye,
                          const void *bounds, const rt_range *ranges, uint32_t n_bounds,
                          rt_scene **out);

rt_status rt_scene_destroy(rt_scene *scene);

/* What rt_scene_create found out about the scene (diagnostic; selects nothing the caller has to know about).
 *   RT_SCENE_HAS_BOUNDS      created with subtree bounds: RT_TRAVERSAL_SKIP is available
 *   RT_SCENE_CONCENTRIC      every group bound is directly followed by an item with the same centre, bit for bit (the
 *                            reference's pyramid, group.rs:37-41): the f32 traversal loops test that item inside the
 *                            bound's step -- same tests, same order, same values, one node step fewer per entered group */
/*   RT_SCENE_DYNAMIC         made by rt_scene_create_dynamic (below): its spheres can be replaced; the general-ray entries serve it */
enum { RT_SCENE_HAS_BOUNDS = 1u, RT_SCENE_CONCENTRIC = 2u, RT_SCENE_DYNAMIC = 4u };
rt_status rt_scene_traits(const rt_scene *scene, uint32_t *traits);

/* What rt_scene_create took on the host (diagnostic: a one-shot caller -- `make image` -- pays it once per process): total_ms for the whole
 * call, stream_ms of it for creating the scene's stream.  In a process that has no stream yet that is where the RUNTIME makes its first
 * hardware queue (~19 ms on MI355X / ROCm 7.2, whoever creates the first stream or launches the first kernel: tools/init_probe.hip); the
 * library's own work -- allocations, uploads, deriving the streams; its code object is loaded meanwhile -- is the difference. */
rt_status rt_scene_setup_cost(const rt_scene *scene, double *total_ms, double *stream_ms);

/* rt_render_tiles with delivery in completion order (the reference's channel, render.rs:271,301-307): the buckets are rendered in
 * batches that are all enqueued at once, and `callback` is invoked -- on the calling thread -- for every bucket of a batch as soon
 * as that batch is complete, while later batches are still rendering.  tile_index: the bucket's position in `tiles`; rgba: its
 * RGBABuffer bytes (row 0 = region.b), valid only during the callback.  Returns when every bucket has been delivered. */
typedef void (*rt_tile_callback)(void *user, uint32_t tile_index, const rt_region *region, const uint8_t *rgba);
rt_status rt_render_tiles_stream(rt_scene *scene, const rt_options *options, rt_traversal traversal,
                                 const rt_region *tiles, uint32_t n_tiles, rt_tile_callback callback, void *user);

/* The same pass for a writer that keeps its image in the FILE's pixel format (PPMStdoutRGBABufferWriter, render.rs:373-401): every listed
 * bucket is rendered and put -- converted on the device -- into its place in a row-major frame of options->width x options->height pixels:
 *   RT_FRAME_RGBA  4 B/px  what set_pixels_from_buffer leaves in the writer's image (render.rs:112-126, 422-424)
 *   RT_FRAME_RGB   3 B/px  R, G, B -- the P6 payload (render.rs:392-396: alpha dropped)
 *   RT_FRAME_GREY  1 B/px  ((r + g + b) as f32 / 3.0) as u8 -- the P5 payload (render.rs:399)
 * frame_out: HOST memory, 4-byte aligned, width * height * {4, 3, 1} bytes; bytes outside the listed buckets are left alone.  Memory from
 * rt_host_alloc / rt_host_register is written by the device directly (a 1080p P6 image: 6.2 MB over PCIe instead of 8.3 MB and no
 * conversion on the CPU); pageable memory goes through pinned staging and a CPU copy.  Batches as for rt_render_tiles_stream: `callback`
 * (may be NULL) is invoked on the calling thread after each batch is in place -- tiles [first_tile, first_tile + n_tiles) of the list --
 * while later batches are still rendering (the writer's once-per-second rewrite, render.rs:427-432, hangs off it). */
typedef enum rt_frame_format { RT_FRAME_RGBA = 0, RT_FRAME_RGB = 1, RT_FRAME_GREY = 2 } rt_frame_format;
typedef void (*rt_batch_callback)(void *user, uint32_t first_tile, uint32_t n_tiles);
rt_status rt_render_frame_stream(rt_scene *scene, const rt_options *options, rt_traversal traversal,
                                 const rt_region *tiles, uint32_t n_tiles, rt_frame_format format, uint8_t *frame_out,
                                 rt_batch_callback callback, void *user);

/* Host memory for RGBABuffer storage (render.rs:74-90 allocates it with vec![0; area * 4]) that the device can reach
 * directly.  rt_render_tiles / rt_render_region recognise such memory by address (any pointer inside a range this library
 * pinned -- memory pinned by other means counts as pageable) and then
 * the render kernel stores its pixels straight into it over PCIe: no device-side copy of the frame, no staging, no CPU copy.
 * Pageable memory (a plain Vec<u8>) works everywhere too, but every byte then takes a bounce through pinned staging and a CPU
 * copy (about 3x slower for a 1080p frame).
 *   rt_host_alloc / rt_host_free        pinned, device-mapped allocation
 *   rt_host_register / rt_host_unregister   pin memory the caller already owns (e.g. the writer's frame, render.rs:323);
 *                                       the caller keeps it alive and unregisters before freeing it */
rt_status rt_host_alloc(size_t bytes, void **out);
rt_status rt_host_free(void *p);
rt_status rt_host_register(void *p, size_t bytes);
rt_status rt_host_unregister(void *p);

/* Renderer::render_region for a batch of regions in ONE device pass (a literal launch per 64x64 bucket would
 * starve 256 CUs).  rgba_out (HOST memory, see rt_host_alloc) receives the tiles back to back
 * ("tile-major"): tile i starts at 4 * sum_{j<i} area(j) and is its own row-major RGBABuffer (render.rs:74-109).
 * A single region {0, height, width, 0} therefore yields the row-major frame.  stats may be NULL. */
rt_status rt_render_tiles(rt_scene *scene, const rt_options *options, rt_traversal traversal,
                          const rt_region *tiles, uint32_t n_tiles,
                          uint8_t *rgba_out, rt_stats *stats);

/* Same, but rgba_out is DEVICE memory on the scene's device and the work is enqueued on `hip_stream`
 * (a hipStream_t passed as void*; NULL = the null stream) without waiting for it: the caller synchronises
 * (and may hand the buffer straight to an RCCL gather).  stats (may be NULL) receives counters
 * only when the call can read them back, i.e. it is filled after an internal stream sync if non-NULL. */
rt_status rt_render_tiles_device(rt_scene *scene, const rt_options *options, rt_traversal traversal,
                                 const rt_region *tiles, uint32_t n_tiles,
                                 void *rgba_out_device, void *hip_stream, rt_stats *stats);

/* rt_render_tiles_device + rt_blit_tiles_device in one pass: every listed bucket is rendered straight into its place
 * in a row-major RGBA frame of options->width x options->height in device memory -- what the writer's image holds
 * after write_rgba_buffer() for each bucket (render.rs:422-424).  Pixels outside the listed buckets are left alone. */
rt_status rt_render_frame_device(rt_scene *scene, const rt_options *options, rt_traversal traversal,
                                 const rt_region *tiles, uint32_t n_tiles,
                                 void *frame_rgba_device, void *hip_stream, rt_stats *stats);

/* Single bucket: the exact shape of the reference call (render.rs:283-294), made from up to RTRACEMAXPROCS pool threads
 * at once.  A request for a bucket of the scheduler's own grid (64 x 64, row-major from (0, 0), edge buckets clipped:
 * render.rs:273-298) is served from a pass that renders the WHOLE grid once per frame into pinned staging -- the call is then a
 * 16 KB copy.  A bucket is handed out once per pass (asking for it again starts the caller's next frame), and the pass for the next
 * frame is started while the current one is being handed out: a scene is immutable, so its bytes are those of a pass started later;
 * one pass too many is rendered when the caller stops.  Other requests: concurrent calls on one scene are merged into shared device
 * passes (whoever finds no pass running leads the next one and renders every request waiting at that moment); a lone caller gets
 * one pass per call.  With stats != NULL the call runs on its own. */
rt_status rt_render_region(rt_scene *scene, const rt_options *options, rt_traversal traversal,
                           const rt_region *region, uint8_t *rgba_out, rt_stats *stats);

/* RGBABuffer::set_pixels_from_buffer (render.rs:112-126) on the device: row-wise blit of tile-major tiles (the
 * layout rt_render_tiles_device writes, or several such shards after an RCCL gather) into a row-major RGBA frame
 * of options->width x options->height, i.e. what PPMStdoutRGBABufferWriter::write_rgba_buffer does per bucket
 * (render.rs:422-424).  src_px_offset[i] is tile i's first pixel in src (in pixels, 4 B each); NULL means the
 * tiles lie back to back in list order.  Enqueued on hip_stream without waiting. */
rt_status rt_blit_tiles_device(rt_scene *scene, const rt_options *options, const rt_region *tiles, uint32_t n_tiles,
                               const uint32_t *src_px_offset, const void *src_tile_major_device,
                               void *frame_rgba_device, void *hip_stream);

/* ---- several GPUs of one node, one process -------------------------------------------------------------
 * The reference joins its pool threads' buckets through one channel (render.rs:271, 293, 301).  A gang does the same across
 * GPUs: the Scene is replicated on every listed device, the buckets of a frame are dealt round-robin in list order
 * (bucket i -> devices[i % n], the scheduler's row-major order render.rs:273-298), every device renders its shard
 * tile-major, and ONE RCCL gather of the equal-length u8 shards (ncclGather over xGMI, root = devices[0]; communicators from
 * ncclCommInitAll) brings them to the root GPU, which blits them into the row-major frame (set_pixels_from_buffer,
 * render.rs:112-126) and hands that frame to the host.  The bytes are identical for every n.  librccl.so is loaded when the
 * first gang is created (RT_ERR_UNSUPPORTED if it cannot be); single-GPU rendering never needs it. */
typedef struct rt_gang rt_gang;
rt_status rt_gang_create(const int *devices, int n_devices, rt_precision precision,
                         const void *dfs_items, uint32_t n_items, const void *light_unit, const void *eye,
                         const void *bounds, const rt_range *ranges, uint32_t n_bounds, rt_gang **out);
rt_status rt_gang_destroy(rt_gang *gang);
rt_status rt_gang_size(const rt_gang *gang, int *n_devices);
/* frame_rgba_host: width * height * 4 bytes, row-major (what the writer's image holds after write_rgba_buffer() for every
 * listed bucket; pixels outside the listed buckets are unspecified).  stats (may be NULL): counters summed over the devices,
 * device_ms = the slowest device's render. */
rt_status rt_gang_render_frame(rt_gang *gang, const rt_options *options, rt_traversal traversal,
                               const rt_region *tiles, uint32_t n_tiles, uint8_t *frame_rgba_host, rt_stats *stats);
/* n_frames frames of the same tile list, frame f to frames_rgba_host[f] (each as for rt_gang_render_frame): the gather, the blit and
 * the copy of frame f run under the render of frame f + 1 (double-buffered shards; what dist.py's run_pipeline does across
 * processes).  A frame buffer from rt_host_alloc / rt_host_register is written by the root GPU's blit kernel directly.
 * stats (may be NULL): the counters of ONE frame. */
rt_status rt_gang_render_frames(rt_gang *gang, const rt_options *options, rt_traversal traversal,
                                const rt_region *tiles, uint32_t n_tiles, uint8_t *const *frames_rgba_host, uint32_t n_frames,
                                rt_stats *stats);

/* ---- ray queries (ABI 5): TypedGroup::intersect(&mut hit, &ray) (group.rs:72-83 over primitive.rs:55-84) for a batch of ANY rays ----
 * Ray i is rays[6i .. 6i+6] = pos.xyz, dir.xyz and starts with hit.distance = tmax[i] (tmax NULL: +inf, Hit::missed(); a tmax <= 0
 * finds nothing).  The walk is the reference's hierarchy walk, test for test, in REAL (as for rt_scene_create); a scene created without
 * bounds has no hierarchy, and the query is then the flat nearest hit over all its items in DFS order.
 *   RT_QUERY_NEAREST  distance_out[i] = the final hit.distance (tmax[i] when nothing was closer); normal_out[3i..] = the final Hit.pos,
 *                     the unit normal primitive.rs:82 forms ({0, 0, 0} when nothing was closer); item_out[i] = the DFS index of the item
 *                     that won (the first in DFS order on equal distances), or -1
 *   RT_QUERY_ANY      occlusion: the walk stops at the first item closer than tmax[i] -- distance_out[i] = that item's distance, item_out[i]
 *                     its DFS index, normal_out its normal there; tmax[i], -1 and {0, 0, 0} when there is none (then the nearest
 *                     query finds nothing below tmax either, and the other way round).
 * normal_out and item_out may be NULL.  stats (may be NULL): primary = n, hits = rays with a result below tmax, sphere_tests / bound_tests /
 * tests_executed of the walk, every other counter 0; asking for it runs the counting flavour of the kernel (same bytes). */
typedef enum rt_query { RT_QUERY_NEAREST = 0, RT_QUERY_ANY = 1 } rt_query;
/* Host memory.  Returns when the results are in place.  RT_ERR_INVALID_ARGUMENT, before the device is touched, for a NULL scene, rays or
 * distance_out, n == 0, an unknown mode, and for rays outside the domain rt_scene_create puts on the light and the eye: a non-finite
 * component, |pos coordinate| > 1e15, a direction whose squared length is not within 2e-3 of 1, a NaN tmax.  Memory from rt_host_alloc /
 * rt_host_register is read and written by the kernel directly; pageable memory is copied through the call's device workspace. */
rt_status rt_intersect_rays(rt_scene *scene, rt_query mode, const void *rays, const void *tmax, uint32_t n,
                            void *distance_out, void *normal_out, int32_t *item_out, rt_stats *stats);
/* The same over DEVICE memory on the scene's device, enqueued on `hip_stream` (a hipStream_t as void*; NULL = the null stream) without
 * waiting for it.  Only pointers, alignment, n and mode are checked: a ray outside the domain above gives unspecified values, never a
 * fault -- the walk ends for any input bits.  stats != NULL: filled after an internal synchronisation of hip_stream. */
rt_status rt_intersect_rays_device(rt_scene *scene, rt_query mode, const void *rays, const void *tmax, uint32_t n,
                                   void *distance_out, void *normal_out, int32_t *item_out, void *hip_stream, rt_stats *stats);

/* ---- multi-hit ray queries (additive to ABI 5): the k closest hits along each ray, or every hit below tmax ----
 * Rays, tmax and the walk as rt_intersect_rays.  Each ray keeps a list of k slots (distance, item), sorted by distance, every slot
 * starting as (tmax[i], -1).  A bound culls its subtree when its distance is >= the cutoff: the last slot's distance (CLOSEST) or
 * tmax[i] (ALL).  An item whose distance is below the last slot's is inserted behind every slot whose distance is <= its own (equal
 * distances stay in DFS order) and the last slot drops out.
 *   RT_MULTIHIT_CLOSEST  the k closest items below tmax; hits_out[i] = the filled slots (<= k).  With k = 1 this is RT_QUERY_NEAREST,
 *                        test for test: the same bytes and counters.
 *   RT_MULTIHIT_ALL      no culling below tmax: the k closest of all items below tmax[i], and hits_out[i] = how many there are (may be > k).
 * Slot j of ray i is at index i*k + j: distance_out (REAL[n*k]), normal_out (REAL[3*n*k], the normal primitive.rs:82 forms for the slot's
 * item and distance), item_out (int32[n*k], DFS index).  An empty slot reads tmax[i], -1 and {0, 0, 0}.  normal_out, item_out and hits_out
 * (uint32[n]) may be NULL.  stats (may be NULL): primary = n, hits = rays with hits_out > 0, sphere_tests / bound_tests / tests_executed,
 * every other counter 0; asking for it runs the counting flavour (same bytes). */
typedef enum rt_multihit { RT_MULTIHIT_CLOSEST = 0, RT_MULTIHIT_ALL = 1 } rt_multihit;
#define RT_MULTIHIT_MAX_K 16
/* Host memory, validated as rt_intersect_rays validates it; also RT_ERR_INVALID_ARGUMENT, before the device is touched, for k == 0,
 * k > RT_MULTIHIT_MAX_K, an unknown mode and a misaligned hits_out.  Pinned memory is used in place, pageable memory goes through the
 * call's device workspace. */
rt_status rt_intersect_rays_multi(rt_scene *scene, rt_multihit mode, uint32_t k, const void *rays, const void *tmax, uint32_t n,
                                  void *distance_out, void *normal_out, int32_t *item_out, uint32_t *hits_out, rt_stats *stats);
/* The same over DEVICE memory, enqueued on `hip_stream` as rt_intersect_rays_device is: only pointers, alignment, n, k and mode are checked. */
rt_status rt_intersect_rays_multi_device(rt_scene *scene, rt_multihit mode, uint32_t k, const void *rays, const void *tmax, uint32_t n,
                                         void *distance_out, void *normal_out, int32_t *item_out, uint32_t *hits_out, void *hip_stream,
                                         rt_stats *stats);

/* ---- traced rays and camera frames (additive to ABI 5): Renderer::raytrace (render.rs:171-215) for ANY rays, render_region (render.rs:218-255)
 * for ANY pinhole camera ----
 * A ray is traced as the render traces a sample: the nearest hit from pos (the hierarchy walk of rt_intersect_rays; a scene created without
 * bounds: the flat nearest hit), the shading of render.rs:190-199 and, where n.light < 0, the any-hit shadow ray from
 * (pos + dir*d) + n*(d*sqrt(EPSILON)) along -light -- one kernel, in REAL, every operation in the reference's order.
 * stats (may be NULL): primary = rays (samples), hits / shadow / occluded as rt_render_tiles counts them, sphere_tests / bound_tests /
 * tests_executed / primary_tests of both walks, device_ms; the longest_wave_* fields 0.  Asking for it runs the counting flavour (same bytes). */
/* Ray i is rays[6i .. 6i+6] = pos.xyz, dir.xyz.  color_out[3i ..] (REAL) = the colour raytrace(s, r, &mut c) leaves in a c that starts at
 * {0, 0, 0}; alpha_out[i] (REAL, may be NULL) = its return value, 1 when lit, else 0.  Host memory, validated as rt_intersect_rays validates
 * its rays (RT_ERR_INVALID_ARGUMENT before the device is touched, also for a NULL scene, rays or color_out and n == 0); memory from
 * rt_host_alloc / rt_host_register is used in place, pageable memory goes through the call's device workspace. */
rt_status rt_trace_rays(rt_scene *scene, const void *rays, uint32_t n, void *color_out, void *alpha_out, rt_stats *stats);
/* The same over DEVICE memory, enqueued on `hip_stream` as rt_intersect_rays_device is: only pointers, alignment and n are checked. */
rt_status rt_trace_rays_device(rt_scene *scene, const void *rays, uint32_t n, void *color_out, void *alpha_out,
                               void *hip_stream, rt_stats *stats);
/* rt_render_tiles through a pinhole camera: `camera` is REAL[12] in HOST memory (both entries) = eye.xyz, right.xyz, up.xyz, forward.xyz.
 * Sample (x, y, ssx, ssy): u = xres - width/2, v = (height - yres) - height/2 (render.rs:238-242) and the ray from eye along
 * normalized((right*u + up*v) + forward*width), every operation rounded once.  The identity camera {Scene::eye, (1,0,0), (0,1,0), (0,0,1)}
 * renders the bytes of rt_render_tiles; |forward| sets the field of view (1: the reference's, horizontally 2*atan(0.5)).  Options, regions,
 * output layout and status codes as rt_render_tiles / rt_render_tiles_device; a scene with bounds is walked as the reference's hierarchy,
 * one without as the flat scan.  RT_ERR_INVALID_ARGUMENT before the device is touched for a camera with a non-finite value, an eye
 * coordinate beyond +-1e15, an axis whose length is outside [1e-2, 1e2], or |det(right, up, forward)| < 1e-2 |right| |up| |forward|. */
rt_status rt_render_camera(rt_scene *scene, const rt_options *options, const void *camera,
                           const rt_region *tiles, uint32_t n_tiles, uint8_t *rgba_out, rt_stats *stats);
rt_status rt_render_camera_device(rt_scene *scene, const rt_options *options, const void *camera,
                                  const rt_region *tiles, uint32_t n_tiles, void *rgba_out_device, void *hip_stream, rt_stats *stats);

/* ---- coherent ray batches (additive to ABI 5): order the rays on the device, walk them in that order ----
 * The query kernels put ray j of the batch into lane j % 64 of wave j / 64, and a wave walks the union of its lanes' subtrees: what a batch
 * costs depends on the order it is stored in.  An ORDER is uint32[n]: order[j] is the index of the ray lane j carries.  Each lane makes its
 * own ray's tests whatever its neighbours do, so the *_ordered entries below write, for ANY permutation, the bytes and the counters of the
 * entries they extend; only the time differs.
 *
 * rt_ray_order computes the stable ascending sort of one 32-bit key per ray (equal keys stay in the caller's order): unique, deterministic,
 * a permutation of 0 .. n-1.  The key depends on the ray's six values and on the batch's origin box, nothing else; the scene supplies the
 * device, REAL and the workspace.  All of it in double (a float converts exactly), every operation rounded once:
 *   lo[a], hi[a]  min / max of pos[a] over the batch, a = 0, 1, 2;  ext = max(hi[a] - lo[a])
 *   scale         0 if ext == 0 (one origin, a camera: every origin bit is 0); else 2^(3 - e), e = max(E - 1022, -1000) with E the 11-bit
 *                 biased exponent field of ext, so that ext < 2^e
 *   c[a]          trunc(min(max((pos[a] - lo[a]) * scale, 0), 7))                                       3 bits per axis
 *   axis          the component of dir with the largest |value|, the lowest such on a tie;  sign = 1 if that component < 0, else 0
 *   q[b]          trunc(min(max((dir[(axis + 1 + b) % 3] + 1) * 512, 0), 1023)), b = 0, 1              10 bits each
 *   key           M3 << 23 | (2 * axis + sign) << 20 | M2, where bit i of c[a] is bit 3i + a of M3 and bit i of q[b] is bit 2i + b of M2
 * rust_tracer_amd.ray_keys restates it in numpy; the order is numpy.argsort(ray_keys(rays), kind="stable") bit for bit. */
/* Host memory; rays validated as rt_intersect_rays validates them (RT_ERR_INVALID_ARGUMENT before the device is touched, also for a NULL
 * scene, rays or order_out and n == 0).  Returns when order_out[0 .. n) is in place. */
rt_status rt_ray_order(rt_scene *scene, const void *rays, uint32_t n, uint32_t *order_out);
/* The same over DEVICE memory, enqueued on `hip_stream` without waiting for it: only pointers, alignment and n are checked; the result is
 * a permutation whatever bits the rays hold.  The temporary storage is the scene's and is reused once the stream has passed the call. */
rt_status rt_ray_order_device(rt_scene *scene, const void *rays, uint32_t n, uint32_t *order_out, void *hip_stream);
/* rt_intersect_rays, rt_intersect_rays_multi and rt_trace_rays with the rays taken in `order`: thread j reads ray order[j] and its tmax and
 * writes every result at index order[j] -- the outputs are indexed by ray, exactly as the unordered entries leave them.
 *   order == NULL  the call computes rt_ray_order's order itself, in its workspace, and walks in it: the one-call form.
 *   order != NULL  host entries: must be a permutation of 0 .. n-1 (RT_ERR_INVALID_ARGUMENT before the device is touched for an index
 *                  >= n or a repeated one).  Device entries: pointer alignment only; a thread whose order[j] >= n carries no ray, so no
 *                  bits in `order` fault; a ray named twice gets unspecified values, one never named is not written.
 * Everything else as the entry each extends; stats->device_ms is the walk's time in every form (the one-call form's order is computed in
 * front of the timed span). */
rt_status rt_intersect_rays_ordered(rt_scene *scene, rt_query mode, const void *rays, const void *tmax, uint32_t n, const uint32_t *order,
                                    void *distance_out, void *normal_out, int32_t *item_out, rt_stats *stats);
rt_status rt_intersect_rays_ordered_device(rt_scene *scene, rt_query mode, const void *rays, const void *tmax, uint32_t n, const uint32_t *order,
                                           void *distance_out, void *normal_out, int32_t *item_out, void *hip_stream, rt_stats *stats);
rt_status rt_intersect_rays_multi_ordered(rt_scene *scene, rt_multihit mode, uint32_t k, const void *rays, const void *tmax, uint32_t n,
                                          const uint32_t *order, void *distance_out, void *normal_out, int32_t *item_out, uint32_t *hits_out,
                                          rt_stats *stats);
rt_status rt_intersect_rays_multi_ordered_device(rt_scene *scene, rt_multihit mode, uint32_t k, const void *rays, const void *tmax, uint32_t n,
                                                 const uint32_t *order, void *distance_out, void *normal_out, int32_t *item_out,
                                                 uint32_t *hits_out, void *hip_stream, rt_stats *stats);
rt_status rt_trace_rays_ordered(rt_scene *scene, const void *rays, uint32_t n, const uint32_t *order, void *color_out, void *alpha_out,
                                rt_stats *stats);
rt_status rt_trace_rays_ordered_device(rt_scene *scene, const void *rays, uint32_t n, const uint32_t *order, void *color_out, void *alpha_out,
                                       void *hip_stream, rt_stats *stats);

/* ---- undersampled camera frames that refine in place (additive to ABI 5) ----
 * F(x, y) is the pixel rt_render_camera writes for (x, y).  The LATTICE of a step s is every pixel with x % s == 0 and y % s == 0, anchored
 * at the image origin (not at a tile's corner); the anchor of (x, y) is (x - x % s, y - y % s).  The step-s frame holds F(anchor(x, y)) in
 * every pixel of every listed tile -- the same bytes whatever tile list it is rendered through; step 1 is rt_render_camera's frame.
 *   prev_step == 0         a fresh frame: every cell that meets a tile is traced from its anchor (inside the tile or not) and written.
 *   prev_step == 2 * step  the buffer holds the step-2s frame of the same scene, options, camera and tile list.  A cell whose anchor also
 *                          lies on the 2s lattice is correct already: it is neither traced nor written.  Every other cell that meets a
 *                          tile is traced and filled; afterwards the buffer holds the step-s frame.  The chain s0, s0/2, ..., 1 traces
 *                          each sample of the full frame exactly once when the tiles' l and b are multiples of s0.
 * step is any integer in [1, RT_UNDERSAMPLE_MAX_STEP]; any other step or prev_step is RT_ERR_INVALID_ARGUMENT before the device is touched.
 * Everything else -- options, camera, regions, the tile-major layout, status codes, stream and stats -- as rt_render_camera /
 * rt_render_camera_device; stats->primary counts the samples actually traced (traced cells x samples_per_pixel^2).  With prev_step != 0
 * the buffer is read-modify-write for the caller: pinned and device memory are refined in place, pageable memory goes up into the call's
 * device output first and comes back whole.  samples_per_pixel == 0 writes {0, 0, 0, 0} into the traced cells. */
#define RT_UNDERSAMPLE_MAX_STEP 64      /* the scheduler's bucket edge */
rt_status rt_render_camera_undersampled(rt_scene *scene, const rt_options *options, const void *camera,
                                        const rt_region *tiles, uint32_t n_tiles, uint32_t step, uint32_t prev_step,
                                        uint8_t *rgba_inout, rt_stats *stats);
rt_status rt_render_camera_undersampled_device(rt_scene *scene, const rt_options *options, const void *camera,
                                               const rt_region *tiles, uint32_t n_tiles, uint32_t step, uint32_t prev_step,
                                               void *rgba_inout_device, void *hip_stream, rt_stats *stats);

/* ---- dynamic scenes (additive to ABI 5): the topology fixed at creation, the spheres replaced in place, the bounds given or refit ----
 * A scene from rt_scene_create is immutable.  A DYNAMIC scene keeps the number of items, their DFS order and the ranges it was created
 * with, and takes new sphere values at any time; its group bounds are the caller's or are refit from the items on the device (the rule
 * below).  It holds what the general-ray entries read -- the items and one stream of the hierarchy (without bounds: of the items) -- and
 * the maps an update needs, all resident on the device: rt_intersect_rays*, rt_intersect_rays_multi*, rt_trace_rays*, rt_render_camera*,
 * rt_render_camera_undersampled*, rt_ray_order* and their *_ordered forms serve it; after any update they write the bytes and counters
 * a scene made by rt_scene_create from the same items, the bounds rt_scene_bounds reports and the same ranges writes.  rt_render_tiles*,
 * rt_render_frame*, rt_render_region and rt_render_tiles_stream return RT_ERR_UNSUPPORTED on it (their caches assume a scene that never
 * changes); rt_render_camera with the identity camera renders rt_render_tiles' bytes.  rt_gang_* has no dynamic form.
 *
 * ORDER.  An update is a WRITE of the scene, every other call a READ.  Device entries (update and queries alike) are ordered by the
 * stream they are enqueued on; across streams the caller orders them (an event, a synchronise).  A host update is exclusive against
 * host calls on the same scene -- a reader-writer lock inside the library: it waits for the host calls under way, and a host call that
 * runs concurrently with it sees the old scene or the new one, never a mix.
 *
 * THE REFIT RULE.  All arithmetic in REAL, every operation rounded once, no FMA, sqrt the IEEE one.  EPSILON and MIN_NORMAL are REAL's
 * machine epsilon (2^-23, 2^-52) and smallest normal number (2^-126, 2^-1022).  For a group over the items [first, first + count), count > 0,
 * item i = {c_i, r_i}, a = x, y, z:
 *   1. lo[a]     = min_i (c_i[a] - r_i)
 *   2. hi[a]     = max_i (c_i[a] + r_i)
 *   3. centre[a] = (lo[a] + hi[a]) * 0.5
 *   4. reach_i   = dist_i + r_i with d = c_i - centre, s = (dx*dx + dy*dy) + dz*dz and
 *                  dist_i = sqrt(s) if s >= MIN_NORMAL / EPSILON^2 (2^-80, 2^-918), else (|dx| + |dy|) + |dz|
 *   5. radius    = max_i (reach_i) * (1 + 8 * EPSILON)
 * and the bound is {centre, radius}.  min and max are exact, so the result does not depend on the order of the items or on how the
 * group is split for the reduction.  The bound encloses every item of the group in exact arithmetic (NOTES.md A derives the 8; the second
 * form of dist_i is what keeps that true where the squares underflow: it is never below the Euclidean distance and has no product in
 * it).  A group with count == 0 has no node in the hierarchy and keeps the bound it was given.  rust_tracer_amd.refit_bounds restates
 * the rule in numpy, bit for bit. */
/* Arguments and validation as rt_scene_create.  bounds == NULL with n_bounds > 0: the bounds are refit from the items; in that form a
 * range with count == 0 is RT_ERR_INVALID_ARGUMENT.  n_bounds == 0: a flat dynamic scene. */
rt_status rt_scene_create_dynamic(int device, rt_precision precision,
                                  const void *dfs_items, uint32_t n_items,
                                  const void *light_unit, const void *eye,
                                  const void *bounds, const rt_range *ranges, uint32_t n_bounds,
                                  rt_scene **out);
/* New values for every sphere, HOST memory: dfs_items REAL[4*n_items] in the same DFS order, bounds REAL[4*n_bounds] or NULL to refit.
 * Validated as creation validates them (finite, |coordinate| <= 1e15, radius > 0): RT_ERR_INVALID_ARGUMENT before the device is touched,
 * and the scene is unchanged.  Returns when the new scene is in place.  RT_ERR_UNSUPPORTED on a scene from rt_scene_create. */
rt_status rt_scene_update(rt_scene *scene, const void *dfs_items, const void *bounds);
/* The same from DEVICE memory, enqueued on `hip_stream` without waiting for it: no allocation and no host synchronisation in the call.
 * Only the pointers and their alignment (one {cx, cy, cz, r} record: 16 bytes for RT_F32, 32 for RT_F64) are checked.  Skip offsets and
 * item words come from the scene's resident topology, never from the caller's values: any bits give unspecified values in the results of
 * later queries, never a fault or an endless walk.  The buffers are read by the work this call enqueues, not after it. */
rt_status rt_scene_update_device(rt_scene *scene, const void *dfs_items_device, const void *bounds_device_or_null, void *hip_stream);
/* The scene's current bounds, REAL[4*n_bounds] into host memory, after waiting for the last update (whichever stream carried it).  A
 * scene from rt_scene_create reports the bounds it was created with. */
rt_status rt_scene_bounds(rt_scene *scene, void *bounds_out);

/* ---- rebuilds (additive to ABI 5): a dynamic scene's hierarchy rebuilt on the device from spheres in any order ----
 * An update keeps every sphere in its DFS slot.  Once the spheres have moved far -- or come in an order that means nothing in space --
 * the groups, which span fixed slots, are no longer compact and their refit bounds swell towards the scene's extent.  A REBUILD first
 * puts the spheres in a spatial order and then refits: the topology (item words, skip offsets, ranges) stays the resident one.
 *
 * THE SPHERE KEY.  One 30-bit key per sphere from its centre c and the batch's centre box; radii take no part.  All of it in double (a
 * float converts exactly), every operation rounded once:
 *   lo[a], hi[a]  min / max of c[a] over the batch, a = 0, 1, 2;  ext = max(hi[a] - lo[a])
 *   scale         0 if ext == 0 (every centre the same: every key is 0); else 2^(10 - e), e = max(E - 1022, -1000) with E the 11-bit
 *                 biased exponent field of ext, so that ext < 2^e
 *   q[a]          trunc(min(max((c[a] - lo[a]) * scale, 0), 1023))                                      10 bits per axis
 *   key           the Morton code of q: bit i of q[a] is bit 3i + a of the key
 * The SPHERE ORDER is the stable ascending sort of the keys (equal keys stay in the caller's order): unique, deterministic, a permutation
 * of 0 .. n-1.  rust_tracer_amd.sphere_keys restates the key in numpy; the order is numpy.argsort(sphere_keys(spheres), kind="stable")
 * bit for bit. */
/* Host memory: spheres REAL[4*n] as {cx, cy, cz, r}, validated as rt_scene_create validates items (finite, |v| <= 1e15, radius > 0):
 * RT_ERR_INVALID_ARGUMENT before the device is touched, also for a NULL scene, spheres or order_out and n == 0.  The scene supplies the
 * device, REAL and the workspace, as for rt_ray_order; any scene will do, static or dynamic, and n need not be its item count.  Returns
 * when order_out[0 .. n) is in place. */
rt_status rt_sphere_order(rt_scene *scene, const void *spheres, uint32_t n, uint32_t *order_out);
/* The same over DEVICE memory, enqueued on `hip_stream` without waiting for it: only pointers, alignment (spheres: one {cx, cy, cz, r}
 * record, 16 bytes for RT_F32, 32 for RT_F64) and n are checked; the result is a permutation whatever bits the spheres hold, and nothing
 * faults.  The temporary storage is the scene's and is reused once the stream has passed the call. */
rt_status rt_sphere_order_device(rt_scene *scene, const void *spheres, uint32_t n, uint32_t *order_out, void *hip_stream);
/* A topology that depends on the item count alone (host only, no device is touched): the groups of the recursive halving of
 * (first, count) = (0, n_items), in DFS pre-order.  Emit (first, count); if count > leaf_size, go on with (first, (count + 1) / 2) and
 * then with the remainder.  Leaves are groups too; there are at most 2 * n_items - 1 groups, and ranges_out has room for 2 * n_items.
 * The output is valid for rt_scene_create and for rt_scene_create_dynamic with bounds == NULL as it stands.  Over spheres in the sphere
 * order it is a median-split tree along the Morton curve.  n_items == 0 (or above 2^31 - 1), leaf_size == 0 or a NULL pointer:
 * RT_ERR_INVALID_ARGUMENT. */
rt_status rt_balanced_ranges(uint32_t n_items, uint32_t leaf_size, rt_range *ranges_out, uint32_t *n_groups_out);
/* The rebuild, HOST memory: spheres REAL[4*n_items] in ANY order, order_out uint32[n_items] or NULL.  Exactly
 * rt_scene_update(scene, spheres[order], NULL) with order = the sphere order of `spheres`: DFS slot k now holds spheres[order[k]] and
 * order_out[k] = order[k]; every group bound is refit by the rule above over the scene's own ranges, whatever ranges it was created
 * with (rt_balanced_ranges is the companion that makes the result a good hierarchy, not a precondition) and whether its bounds were
 * the caller's or refit.  Afterwards every general-ray entry and rt_scene_bounds answer with the bytes and counters of a scene made by
 * rt_scene_create from spheres[order], those bounds and the same ranges; item_out values are DFS slots as always, and order_out maps
 * them back to the caller's indices.  Validated as rt_scene_update validates (RT_ERR_INVALID_ARGUMENT before the device is touched, the
 * scene unchanged); takes the scene's write lock as a host update does; returns when the new scene is in place.  RT_ERR_UNSUPPORTED on a
 * scene from rt_scene_create, and on a dynamic scene created with n_bounds == 0 (nothing to refit: rt_last_error_message says so). */
rt_status rt_scene_rebuild(rt_scene *scene, const void *spheres, uint32_t *order_out);
/* The same from DEVICE memory, enqueued on `hip_stream` without waiting for it, a WRITE in the sense of ORDER above: no host
 * synchronisation, and no allocation except that the first rebuild of a scene makes that scene's rebuild workspace (sized by n_items
 * alone, kept with the scene, freed with it; rebuilds of one scene on different streams are the caller's to order, as all writes are).
 * Only the pointers and their alignment (spheres: one record; order_out: 4 bytes) are checked.  Skip offsets and item words still come
 * from the resident topology alone: any bits in the spheres give unspecified values in the results of later queries, never a fault or
 * an endless walk, and order_out is a permutation of 0 .. n_items-1 all the same. */
rt_status rt_scene_rebuild_device(rt_scene *scene, const void *spheres_device, uint32_t *order_out_device_or_null, void *hip_stream);

/* ---- live and dead slots (additive to ABI 5): a dynamic scene's n_items is a CAPACITY ----
 * Every slot of a dynamic scene is LIVE or DEAD.  Every entry above leaves every slot live; the entries below say which are.
 *   A DEAD ITEM is never hit: no general-ray entry (rt_intersect_rays*, rt_intersect_rays_multi*, rt_trace_rays* -- primary and shadow
 * walk --, rt_render_camera*, rt_render_camera_undersampled*, the *_ordered forms) reports its slot, its distance or a normal from it.
 * Its node stays in the hierarchy -- the topology is fixed --, so a walk that reaches it tests it, counts it in sphere_tests /
 * tests_executed, and misses.  Its values are never read into any result or bound: a dead slot may hold any bits, NaN included.
 *   THE REFIT RULE runs over a group's LIVE items only (steps 1, 2 and 4); min and max stay exact, so the result is still independent of
 * order and split, and rust_tracer_amd.refit_bounds(..., live=) restates it bit for bit.  A group without a live item is a DEAD GROUP:
 * its node culls its subtree for every ray at the cost of one bound test, and rt_scene_bounds reports {0, 0, 0, 0} for it (radius 0 is no
 * valid bound: it marks the group).  The caller's bounds (bounds != NULL) are validated and written as given; enclosing the live items
 * is then the caller's business, and the dead items under them are still never hit.
 *   After any of these calls the scene writes the bytes and counters of a scene made by rt_scene_create from the same ranges, with any
 * sphere no ray can reach in each dead slot and as each dead group's bound.  They are WRITES in the sense of ORDER above; a later
 * rt_scene_update* or rt_scene_rebuild* makes every slot live again. */
/* rt_scene_update with liveness, HOST memory: live is uint8[n_items], nonzero = live; NULL = every slot live, and the call is then exactly
 * rt_scene_update.  Only the live items are validated.  A flat dynamic scene (n_bounds == 0) takes liveness too.  RT_ERR_UNSUPPORTED on
 * a scene from rt_scene_create. */
rt_status rt_scene_update_live(rt_scene *scene, const void *dfs_items, const void *bounds, const uint8_t *live);
/* The same from DEVICE memory, under rt_scene_update_device's rules: pointers and alignment alone are checked, nothing is allocated or
 * waited for, and any bits in the items or the liveness bytes give unspecified query results, never a fault or an endless walk. */
rt_status rt_scene_update_live_device(rt_scene *scene, const void *dfs_items_device, const void *bounds_device_or_null,
                                      const uint8_t *live_device_or_null, void *hip_stream);
/* rt_scene_rebuild of n spheres into a scene of capacity n_items, 0 <= n <= n_items; HOST memory, spheres REAL[4*n] in ANY order,
 * order_out uint32[n] or NULL.  By contract rt_scene_update_live(scene, X, NULL, L) with order = the sphere order of the n spheres (the
 * same key, the same stable sort, over n records), X[k] = spheres[order[k]] and L[k] = 1 for k < n, slots k >= n dead; order_out[k] =
 * order[k] for k < n.  With n == n_items it is rt_scene_rebuild, byte for byte.  n == 0 empties the scene -- every query misses -- and
 * spheres may then be NULL: the one place where n == 0 is no error.  Over rt_balanced_ranges the live prefix is covered by live groups
 * and everything to its right is dead groups, culled at their first node.  NULL spheres with n > 0 and n > n_items are
 * RT_ERR_INVALID_ARGUMENT before the device is touched; RT_ERR_UNSUPPORTED as for rt_scene_rebuild (a scene from rt_scene_create, a flat
 * dynamic scene). */
rt_status rt_scene_rebuild_n(rt_scene *scene, const void *spheres, uint32_t n, uint32_t *order_out);
/* The same from DEVICE memory, under rt_scene_rebuild_device's rules: no host synchronisation, and no allocation beyond the scene's
 * rebuild workspace, which is sized by the capacity. */
rt_status rt_scene_rebuild_n_device(rt_scene *scene, const void *spheres_device, uint32_t n, uint32_t *order_out_device_or_null,
                                    void *hip_stream);
/* The current liveness, uint8[n_items] of 0 / 1 into host memory, after waiting for the last write as rt_scene_bounds does.  A scene
 * from rt_scene_create reports all ones. */
rt_status rt_scene_live(rt_scene *scene, uint8_t *live_out);

/* ---- proximity queries (additive to ABI 5): the k nearest spheres of a point, or every sphere within a radius ----
 * The question a caller that moves spheres asks before its next update: which spheres are near this one?  Query g is a point p =
 * points[3g .. 3g+3] (REAL) and a search radius rho = radius[g] (REAL; radius == NULL: +inf).  The metric is the surface GAP between p and
 * a sphere.  For a record {c, rr} of the scene's stream -- rr is the radius squared, rounded once -- in REAL, every operation rounded
 * once, no FMA, both roots the IEEE ones:
 *   v   = c - p                                       component-wise
 *   vv  = (v.x*v.x + v.y*v.y) + v.z*v.z
 *   gap = rr > 0 ? sqrt(vv) - sqrt(rr) : +inf
 * The gap is negative when p is inside the sphere.  The guard is part of the definition: a dead item and a dead group (rr = -inf, "live
 * and dead slots" above) have gap +inf, so a dead item is never reported or counted and a dead group culls its subtree at its one test.
 * rust_tracer_amd.sphere_gaps restates the gap in numpy, bit for bit.
 *   The walk is rt_intersect_rays_multi's over the same stream with the gap in place of the distance along a ray (a bound encloses its
 * items, so its gap is a lower bound of theirs).  Each query keeps k slots (gap, item), every slot starting as (rho, -1).  A bound culls
 * when its gap is >= the cutoff: the last slot's gap (CLOSEST) or rho (ALL).  An item whose gap is not >= the last slot's is inserted
 * behind every slot whose gap is <= its own (equal gaps stay in DFS order) and the last slot drops out.
 *   RT_NEAR_CLOSEST  the k nearest items below rho; found_out[g] = the filled slots (<= k).
 *   RT_NEAR_ALL      no culling below rho: the k nearest of all items below rho, and found_out[g] = how many there are (may be > k).
 * The result is the walk's: a bound that encloses its items only to within rounding can cull an item whose own test would have passed by
 * an ulp.  Whenever no item's gap lies within a few ulp of the cutoff it is the brute-force answer over all items.
 *   exclude (int32[n] or NULL): the item slot query g ignores -- the self-query of a sphere that lives in the scene.  That item is tested
 * and counted as a test, but never listed and never counted as found; -1 or any slot outside the scene excludes nothing.
 *   order (uint32[n] or NULL): thread j carries query order[j], with the rules of the *_ordered entries above -- host entry: a permutation
 * of 0 .. n-1; device entry: alignment only, and an entry >= n carries no query.  NULL: the caller's order.  The bytes and counters are
 * the same in every order; only the time differs.  A query is a sphere-shaped record: rt_sphere_order over {p, 1} gives a coherent order.
 *   Slot j of query g is at index g*k + j, nearest first: gap_out (REAL[n*k]; an empty slot reads rho), item_out (int32[n*k] or NULL, DFS
 * slot; an empty slot reads -1), found_out (uint32[n] or NULL).  stats (may be NULL): primary = n, hits = queries with found_out > 0,
 * sphere_tests / bound_tests / tests_executed, every other counter 0; asking for it runs the counting flavour (same bytes). */
typedef enum rt_near { RT_NEAR_CLOSEST = 0, RT_NEAR_ALL = 1 } rt_near;
#define RT_NEAR_MAX_K 16
/* Host memory.  RT_ERR_INVALID_ARGUMENT before the device is touched for a NULL scene, points or gap_out, n == 0, k == 0 or k >
 * RT_NEAR_MAX_K, an unknown mode, a misaligned buffer, a point with a non-finite coordinate or one beyond +-1e15 (the scene's own domain)
 * and a NaN radius; any other radius is valid -- a negative one finds only the spheres that contain the point that deep.  Pinned memory
 * is used in place, pageable memory goes through the call's device workspace.  On a dynamic scene the call is a READ in the sense of
 * ORDER above: behind a host update, rebuild or live update it sees the new scene. */
rt_status rt_near_spheres(rt_scene *scene, rt_near mode, uint32_t k, const void *points, const void *radius, uint32_t n,
                          const int32_t *exclude, const uint32_t *order, void *gap_out, int32_t *item_out, uint32_t *found_out,
                          rt_stats *stats);
/* The same over DEVICE memory, enqueued on `hip_stream` as rt_intersect_rays_device is: only pointers, alignment, n, k and mode are
 * checked.  A query outside the domain gives unspecified values, never a fault -- the walk ends for any input bits.  stats != NULL:
 * filled after an internal synchronisation of hip_stream. */
rt_status rt_near_spheres_device(rt_scene *scene, rt_near mode, uint32_t k, const void *points, const void *radius, uint32_t n,
                                 const int32_t *exclude, const uint32_t *order, void *gap_out, int32_t *item_out, uint32_t *found_out,
                                 rt_stats *stats, void *hip_stream);

/* ---- sphere casts (additive to ABI 5): the first contact of a moving sphere with the scene ----
 * The third question a caller that moves spheres asks, after "what does this ray hit" and "what is near this point": how far can this
 * sphere move along a direction before it touches something?  Cast g is a ray rays[6g .. 6g+6] = pos.xyz, dir.xyz (REAL; dir a unit
 * vector, as for rt_intersect_rays), a radius q = radius[g] (REAL; radius == NULL: 0) and a cutoff tmax[g] (REAL; tmax == NULL: +inf; a
 * tmax <= 0 finds nothing).  A sphere of radius q moving along a ray touches a sphere {c, r} exactly where the ray hits {c, r + q}.  The
 * CAST DISTANCE of a record {c, rr} of the scene's stream -- rr is the radius squared, rounded once -- in REAL, every operation rounded
 * once, no FMA, both roots the IEEE ones:
 *   rad  = sqrt(rr)
 *   RR   = (rr + (q + q) * rad) + q * q               (r + q)^2 expanded; q = 0 gives RR == rr bit for bit
 *   v    = c - pos ;  b = dot(v, dir) ;  disc = (b*b - dot(v, v)) + RR        dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z
 *   t    = +inf                  if !(rr > 0)  or  disc < 0  or  b + sqrt(disc) < 0
 *        = b - sqrt(disc)        if that is > 0
 *        = 0                     otherwise: the moving sphere touches or overlaps the record at its start
 * Two points differ from the ray query on purpose.  The start case is 0, not the exit distance b + sqrt(disc): the ray entries let a
 * bound that contains the origin be culled by its exit distance, as the reference does; with 0 the inflated bound's distance is a lower
 * bound of its inflated items' distances in exact arithmetic -- it is missed or behind only if they are, it is entered no later, and it
 * is 0 whenever the start is inside -- and a cast that starts in contact reports distance 0 and that item, which is what a collision
 * step needs.  And the guard rr > 0 is the proximity queries': a dead item and a dead group (rr = -inf, "live and dead slots" above) are
 * at +inf, so a dead item never wins and a dead group culls its subtree at its one test.  rust_tracer_amd.sweep_distances restates the
 * distance in numpy, bit for bit.
 *   The walk is rt_intersect_rays's over the same stream; `best` starts at tmax.  A bound culls when t >= best.
 *   RT_SWEEP_NEAREST  an item with !(t >= best) becomes the result: the first item in DFS order wins a tie, several items at 0 included.
 *   RT_SWEEP_ANY      the first item with !(t >= tmax) is the result, and the cast ends there.
 * The result is the walk's, as for every query here.  With q = 0, for rays on which every tested record has rr > 0 and b - sqrt(disc) >
 * 0 wherever it is hit, a cast is rt_intersect_rays test for test: the same bytes, the same counters.
 *   exclude (int32[n] or NULL): the item slot cast g ignores -- a sphere that lives in the scene and is cast from its own pose.  That
 * item is tested and counted as a test, but can never be the result; -1 or any slot outside the scene excludes nothing.
 *   order (uint32[n] or NULL): thread j carries cast order[j], with the rules of the *_ordered entries above -- host entry: a permutation
 * of 0 .. n-1; device entry: alignment only, and an entry >= n carries no cast.  NULL: the caller's order.  The bytes and counters are
 * the same in every order; only the time differs.
 *   distance_out (REAL[n]): the result's t, or tmax[g] when there is none.  item_out (int32[n] or NULL): its DFS slot, or -1.  normal_out
 * (REAL[3n] or NULL): normalized(pos + (dir * t - c)) with the result's own centre -- from the touched sphere towards the moving sphere's
 * centre at contact --, {0, 0, 0} when there is none.  stats (may be NULL): primary = n, hits = casts with a result, sphere_tests /
 * bound_tests / tests_executed, every other counter 0; asking for it runs the counting flavour (same bytes). */
typedef enum rt_sweep { RT_SWEEP_NEAREST = 0, RT_SWEEP_ANY = 1 } rt_sweep;
/* Host memory.  RT_ERR_INVALID_ARGUMENT before the device is touched for everything rt_intersect_rays rejects (a NULL scene, rays or
 * distance_out, n == 0, a misaligned REAL buffer or item_out, a ray with a non-finite component, |pos| > 1e15 or a direction that is
 * no unit vector, a NaN tmax, a buffer in device memory), an unknown mode, a misaligned exclude or order, an order that is no
 * permutation, and a radius that is NaN, negative, infinite or above 1e15 (a scene's own bound on a radius).  Pinned memory is used in
 * place, pageable memory goes through the call's device workspace.  On a dynamic scene the call is a READ in the sense of ORDER above. */
rt_status rt_sweep_spheres(rt_scene *scene, rt_sweep mode, const void *rays, const void *radius, const void *tmax, uint32_t n,
                           const int32_t *exclude, const uint32_t *order, void *distance_out, void *normal_out, int32_t *item_out,
                           rt_stats *stats);
/* The same over DEVICE memory, enqueued on `hip_stream` as rt_intersect_rays_device is: only pointers, alignment, n and mode are checked.
 * A cast outside the domain gives unspecified values, never a fault -- the walk ends for any input bits.  stats != NULL: filled after an
 * internal synchronisation of hip_stream. */
rt_status rt_sweep_spheres_device(rt_scene *scene, rt_sweep mode, const void *rays, const void *radius, const void *tmax, uint32_t n,
                                  const int32_t *exclude, const uint32_t *order, void *distance_out, void *normal_out, int32_t *item_out,
                                  rt_stats *stats, void *hip_stream);

/* ---- contact pairs (additive to ABI 5): every pair of spheres of the scene that is closer than a margin ----
 * The question a caller that moves spheres asks every step: which spheres of the scene touch each other?  The broad phase of a collision
 * step, the neighbour list of a relaxation step.  rt_near_spheres can only approximate it -- every centre has to come back in as a query,
 * every pair is found twice, and a query lists at most RT_NEAR_MAX_K neighbours.  This is a self-join over the scene's own stream: every
 * pair is tested once, and the list is as long as the data makes it.
 *   For two item slots i < j with stream records {c_i, rr_i} and {c_j, rr_j} -- rr is the radius squared, rounded once -- in REAL, every
 * operation rounded once, no FMA, every root the IEEE one:
 *   v   = c_j - c_i                                   component-wise
 *   vv  = (v.x*v.x + v.y*v.y) + v.z*v.z
 *   gap = (rr_i > 0 && rr_j > 0) ? (sqrt(vv) - sqrt(rr_j)) - sqrt(rr_i) : +inf
 * the proximity queries' gap of record j from the point c_i, minus the radius of sphere i.  The LOWER slot is always the query, so the
 * rounding of a pair is defined once.  The pair (i, j) is a CONTACT when !(gap >= margin): margin = 0 gives the overlapping spheres, a
 * positive margin is a skin, a negative one gives the pairs that overlap that deep, +inf every pair of live spheres.  A dead item (rr =
 * -inf, "live and dead slots" above) is never part of a pair, as i or as j; a sphere whose rr is 0 behaves like one, as for the proximity
 * queries.  rust_tracer_amd.pair_gaps restates the gap in numpy, bit for bit.
 *   The walk is the proximity queries' RT_NEAR_ALL walk with the scene's items as the queries: item i walks the part of the stream BEHIND
 * its own node -- items appear in the stream in ascending slot order, so that is every item j > i -- with q = sqrt(rr_i); a bound culls
 * when (sqrt(vv) - sqrt(rr)) - q >= margin (a bound without a positive rr: always), an item with !(gap >= margin) is a contact.  The
 * result is the walk's, as for every query here: a bound encloses its items, so a pair can differ from brute force over all i < j only
 * if its gap lies within a few ulp of the margin.
 *   The list is made in two passes, without an atomic append, so it is the same bytes every time: the walk counts the pairs of every
 * item, an exclusive scan of the counts gives offsets[n_items + 1], and the walk runs again and writes pair offsets[i] + (rank within i).
 * The pairs are sorted by (i, j).  pairs_out (int32[2 capacity] or NULL): pair p is pairs_out[2p] = i, pairs_out[2p + 1] = j; gap_out
 * (REAL[capacity] or NULL; needs pairs_out): its gap.  Only pairs p < min(capacity, total) are written -- a capacity that is too small
 * gets the exact prefix of the list, and nothing behind it is touched.  *total_out is always the full count: size a buffer from it and
 * call again.  capacity == 0 or pairs_out == NULL skips the second pass: the cheap "how many".  offsets_out (uint64[n_items + 1] or
 * NULL): item i is the lower slot of pairs offsets_out[i] .. offsets_out[i + 1], and offsets_out[n_items] == *total_out.  stats (may be
 * NULL): the counters of ONE walk, the counting pass -- primary = live items, hits = items with at least one pair as the lower slot,
 * sphere_tests / bound_tests / tests_executed, every other counter 0; asking for it runs the counting flavour (same bytes). */
/* Host memory.  RT_ERR_INVALID_ARGUMENT before the device is touched for a NULL scene or total_out, a NaN margin, a misaligned buffer
 * (pairs_out 4 bytes, gap_out REAL, offsets_out and total_out 8 bytes), gap_out without pairs_out, capacity > 2^31 - 1 and a buffer in
 * device memory.  Pinned memory is written in place, pageable memory goes through the call's device workspace.  Returns when the results
 * are in place.  The call is a READ in the sense of ORDER above, on static, dynamic, live and flat scenes alike.  Host calls on one scene
 * take turns (they share the scene's contacts workspace, made by the first call and freed with the scene). */
rt_status rt_scene_contacts(rt_scene *scene, double margin, uint32_t capacity, int32_t *pairs_out, void *gap_out, uint64_t *offsets_out,
                            uint64_t *total_out, rt_stats *stats);
/* The same over DEVICE memory (total_out too), enqueued on `hip_stream` without a host synchronisation: only pointers, alignment, the
 * margin and the capacity are checked.  Nothing is allocated beyond the scene's contacts workspace at the first call; a call goes behind
 * the contacts call before it, whichever stream that was on.  Pairs p >= *total_out keep the caller's bytes.  stats != NULL: filled after
 * an internal synchronisation of hip_stream. */
rt_status rt_scene_contacts_device(rt_scene *scene, double margin, uint32_t capacity, int32_t *pairs_out, void *gap_out, uint64_t *offsets_out,
                                   uint64_t *total_out, rt_stats *stats, void *hip_stream);

/* ---- overlap lists (additive to ABI 5): every sphere of the scene within a margin of each query sphere ----
 * The question of a sphere that is NOT an item of the scene: which spheres of the scene does it touch?  A second set of bodies against a
 * resident world, a sensor or trigger volume, a sphere about to be spawned.  rt_near_spheres takes outside queries but keeps at most
 * RT_NEAR_MAX_K slots per query; rt_scene_contacts has no cap but its queries are the scene's own records.  This entry takes outside
 * queries and gives a list as long as the data makes it.
 *   Query g is queries[4g .. 4g+4] = {p.x, p.y, p.z, q} in REAL: a centre and a radius, the layout of a scene's sphere array -- a second
 * scene's spheres go in as they are.  For a record {c, rr} of the scene's stream -- rr is the radius squared, rounded once -- in REAL,
 * every operation rounded once, no FMA, every root the IEEE one:
 *   v   = c - p                                       component-wise
 *   vv  = (v.x*v.x + v.y*v.y) + v.z*v.z
 *   gap = rr > 0 ? (sqrt(vv) - sqrt(rr)) - q : +inf
 * the proximity queries' gap minus the query's radius: the contact pairs' gap with q given by the caller instead of taken from the
 * stream.  With q = 0 it is the proximity queries' gap bit for bit (x - 0 == x).  An item is LISTED when !(gap >= margin): margin = 0
 * gives the spheres the query overlaps, a positive margin is a skin, a negative one asks for that much overlap, +inf lists every live
 * sphere.  A query whose q is not >= 0 (negative, NaN) carries no query: it makes no test and lists nothing.  A dead item (rr = -inf,
 * "live and dead slots" above) is at +inf and never listed, at margin = +inf too; a sphere whose rr is 0 behaves like one.
 * rust_tracer_amd.overlap_gaps restates the gap in numpy, bit for bit.
 *   The walk is the proximity queries' RT_NEAR_ALL walk over the whole stream: a bound culls when its gap >= margin (a bound without a
 * positive rr: always), an item with !(gap >= margin) is listed.  The result is the walk's, as for every query here: a bound encloses its
 * items, so a list can differ from brute force over all items only where a gap lies within a few ulp of the margin.  exclude and order
 * mean what they mean for rt_near_spheres: exclude (int32[n] or NULL) is the item slot query g never lists -- it is tested and counted as
 * a test, never listed or counted as found; order (uint32[n] or NULL): thread j carries query order[j], and the bytes and counters are
 * the same in every order.
 *   The list is made as the contact pairs' is, in two passes and without an atomic append, so it is the same bytes every time: the walk
 * counts the entries of every query, an exclusive scan of the counts gives offsets[n + 1], and the walk runs again -- only for the
 * queries that counted something -- and writes entry offsets[g] + (rank within g).  The entries are sorted by (g, item slot).  items_out
 * (int32[capacity] or NULL): the item slot of every entry; gap_out (REAL[capacity] or NULL; needs items_out): its gap.  Only entries
 * e < min(capacity, total) are written -- a capacity that is too small gets the exact prefix of the list, and nothing behind it is
 * touched.  *total_out is always the full count: size a buffer from it and call again.  capacity == 0 or items_out == NULL skips the
 * second pass: the cheap "how many".  offsets_out (uint64[n + 1] or NULL): query g owns entries offsets_out[g] .. offsets_out[g + 1], and
 * offsets_out[n] == *total_out.  stats (may be NULL): the counters of ONE walk, the counting pass -- primary = queries carried, hits =
 * queries with at least one entry, sphere_tests / bound_tests / tests_executed, every other counter 0; asking for it runs the counting
 * flavour (same bytes).
 *   The workspace of the two passes (counts, offsets, the scan's block sums) belongs to the scene: the first call makes it, and it grows
 * only when n exceeds the largest n any call on the scene has brought so far.  Growing is the one allocation a call can make, and it
 * waits for the overlap call before it.  The workspace is freed with the scene.  Calls on one scene are put in a row. */
/* Host memory.  RT_ERR_INVALID_ARGUMENT before the device is touched for a NULL scene, queries or total_out, n == 0, a NaN margin, a
 * misaligned buffer (items_out, exclude, order 4 bytes, queries and gap_out REAL, offsets_out and total_out 8 bytes), gap_out without
 * items_out, capacity > 2^31 - 1, a buffer in device memory, a centre coordinate that is not finite or beyond +-1e15, a q that is NaN,
 * negative, infinite or above 1e15 (the radius of rt_sweep_spheres) and an order that is no permutation of 0 .. n-1.  Pinned memory is
 * used in place, pageable memory goes through the call's device workspace.  Returns when the results are in place.  The call is a READ
 * in the sense of ORDER above, on static, dynamic, live and flat scenes alike. */
rt_status rt_overlap_spheres(rt_scene *scene, const void *queries, uint32_t n, double margin, const int32_t *exclude, const uint32_t *order,
                             uint32_t capacity, int32_t *items_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats);
/* The same over DEVICE memory (total_out too), enqueued on `hip_stream` without a host synchronisation (but see the workspace above):
 * only pointers, alignment, n, the margin and the capacity are checked.  An order entry >= n carries no query, and a query that no
 * thread carries has count 0; any input bits end the walk without a fault.  A call goes behind the overlap call before it, whichever
 * stream that was on.  Entries e >= *total_out keep the caller's bytes.  stats != NULL: filled after an internal synchronisation of
 * hip_stream. */
rt_status rt_overlap_spheres_device(rt_scene *scene, const void *queries, uint32_t n, double margin, const int32_t *exclude, const uint32_t *order,
                                    uint32_t capacity, int32_t *items_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats,
                                    void *hip_stream);

/* ---- box overlap lists (additive to ABI 5): every sphere of the scene within a margin of each axis-aligned query box ----
 * The other volume a caller holds: a trigger or kill volume, a selection rectangle, the broad-phase box of a body that is no sphere, a
 * grid cell, the world's bounds -- and, with infinite sides, a slab or a half-space ("everything below this floor").  Passing the box's
 * circumscribed sphere to rt_overlap_spheres and filtering on the host works, but a flat box or a slab makes that superset most of the
 * scene.
 *   Query g is boxes[6g .. 6g+6] = {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z} in REAL.  For a record {c, rr} of the scene's stream -- rr is the
 * radius squared, rounded once -- in REAL, every operation rounded once, no FMA, every root the IEEE one, per axis k:
 *   e_k = lo_k - c_k
 *   f_k = c_k - hi_k
 *   e_k = f_k > e_k ? f_k : e_k
 *   e_k = e_k > 0 ? e_k : 0                           comparisons, not fmax: a NaN fails them
 *   dd  = (e.x*e.x + e.y*e.y) + e.z*e.z
 *   gap = rr > 0 ? sqrt(dd) - sqrt(rr) : +inf
 * the distance from the box to the sphere's SURFACE, floored at -r: a centre inside the box has gap = -r however deep it lies.  This is
 * no signed depth: a negative margin -m lists the spheres that reach more than m into the box, a reach that counts as r at the most, and
 * says nothing about how far inside the box a sphere lies.  An item is LISTED when !(gap >= margin); a bound CULLS when gap >= margin, and a bound without a positive rr always
 * culls.  A box carries a query exactly when lo_k <= hi_k on all three axes; NaN fails the comparison.  An inverted box carries no query:
 * it makes no test and its row is empty.  Infinite sides are valid: lo = -inf and / or hi = +inf give slabs and half-spaces, the
 * all-infinite box lists every live sphere with gap = -sqrt(rr), and no step of the arithmetic above makes a NaN from them.  A point box
 * lo == hi == p gives the gap of rt_overlap_spheres with q = 0 bit for bit.  A dead item is at +inf and never listed, at margin = +inf
 * too; a dead bound culls at its one test.  rust_tracer_amd.box_gaps restates the gap in numpy, bit for bit.
 *   The walk, the two passes, capacity and the exact prefix, the sorted entries, the same bytes every time and in every order,
 * offsets_out, *total_out, stats (primary = boxes carried, hits = boxes with an entry), exclude, and the READ under the scene's lock on
 * static, dynamic, live and flat scenes are exactly those of rt_overlap_spheres.  The calls use that entry's workspace and take their
 * turn with the overlap, swept-overlap and first-contact calls of their scene. */
/* Host memory.  RT_ERR_INVALID_ARGUMENT before the device is touched for a NULL scene, boxes or total_out, n == 0, a NaN margin, a
 * misaligned buffer (items_out, exclude, order 4 bytes, boxes and gap_out REAL, offsets_out and total_out 8 bytes), gap_out without
 * items_out, capacity > 2^31 - 1, a buffer in device memory, a box coordinate that is NaN or finite and beyond +-1e15 (an infinite one is
 * accepted), a box with lo_k > hi_k on some axis and an order that is no permutation of 0 .. n-1. */
rt_status rt_overlap_boxes(rt_scene *scene, const void *boxes, uint32_t n, double margin, const int32_t *exclude, const uint32_t *order,
                           uint32_t capacity, int32_t *items_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats);
/* The same over DEVICE memory (total_out too), enqueued on `hip_stream` without a host synchronisation: only pointers, alignment, n, the
 * margin and the capacity are checked.  An inverted or NaN box and an order entry >= n carry no query, and a box that no thread carries
 * has count 0; any input bits end the walk without a fault. */
rt_status rt_overlap_boxes_device(rt_scene *scene, const void *boxes, uint32_t n, double margin, const int32_t *exclude, const uint32_t *order,
                                  uint32_t capacity, int32_t *items_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats,
                                  void *hip_stream);

/* ---- region overlap lists (additive to ABI 5): every sphere of the scene that reaches into each convex region of six planes ----
 * A renderer's first spatial question -- which spheres can this camera, this screen rectangle, this tilted trigger volume see -- and the
 * oriented box rt_overlap_boxes cannot hold.  It is asked with FEW regions that each cover much of the scene, so the walk is the inverse
 * of the other queries': one region per WAVE, and the lanes carry sections of the node stream (below).
 *   Region g is planes[24g .. 24g+24] = six planes {n.x, n.y, n.z, d} in REAL.  The OUTSIDE of a plane is where n.c + d > 0.  For a
 * record {c, rr} of the scene's stream -- rr is the radius squared, rounded once -- in REAL, every operation rounded once, no FMA, the
 * root the IEEE one:
 *   s_k = ((n_k.x*c.x + n_k.y*c.y) + n_k.z*c.z) + d_k        for k = 0 .. 5
 *   m   = -inf;  for k = 0 .. 5:  m = s_k > m ? s_k : m       a comparison, not fmax
 *   gap = rr > 0 ? m - sqrt(rr) : +inf
 * An item is LISTED when !(gap >= margin); a bound CULLS when gap >= margin, and a bound without a positive rr always culls.
 *   With unit normals m is the largest signed plane distance of the centre.  It is never above the true distance from the region to the
 * centre, so the list is a SUPERSET of the exact touch list: never short of it, and larger only for spheres outside the region near one
 * of its edges or corners.  This is the usual sphere / frustum test.  Normals are expected to have length 1; a shorter normal only
 * weakens its plane.  In exact arithmetic with |n_k| <= 1 a bound that encloses an item never culls what the item's own test lists: each
 * s_k is 1-Lipschitz in c and so is their maximum, so m(item) >= m(bound) - |c_item - c_bound| and the item's gap is at least the bound's.
 * In REAL the two sides round separately, and the walk can differ from a brute-force pass over the items only within a few ulp of the
 * margin.  As everywhere here, the result is DEFINED as the walk's: the one-lane walk of rt_overlap_spheres over the scene's plain
 * per-origin stream from node 0 with this metric.
 *   An ABSENT plane is {0, 0, 0, -inf}: s = -inf for every finite centre, which is how fewer than six planes are passed; six absent
 * planes list every live sphere.  A region carries a query exactly when none of its 24 reals is NaN; any other region makes no test and
 * has an empty row.  A dead item is at +inf and never listed; a dead bound culls at its one test.  rust_tracer_amd.region_gaps restates
 * the gap in numpy, bit for bit.
 *   sections: each region is cut into J sections of the stream, section j the nodes [floor(j N / J), floor((j + 1) N / J)), N the
 * stream's node count; 64 consecutive sections of one region make a wave.  A section's lane first descends from node 0 -- it tests
 * (and counts) only the bounds whose subtree holds its first node, and where one culls it continues behind that subtree -- then walks its
 * nodes as the one-lane walk does.  The sections' lists, in order, ARE the one-lane walk's list: the same bytes for every J.  The caller's
 * value is clamped to 1 .. N; 0 lets the library choose, by a rule that is a pure function of (n, N), never of the device:
 *   J = max(1, min(floor(2^18 / n), floor(N / 8)))
 * (rust_tracer_amd.region_sections restates it).  A product n * J above 2^26 is refused.
 *   The two passes, capacity and the exact prefix, the entries sorted by (g, item slot), the same bytes every time, offsets_out[n + 1],
 * *total_out and the READ under the scene's lock on static, dynamic, live and flat scenes are those of rt_overlap_spheres; there is no
 * exclude and no order (regions are no items, and there are few of them).  stats: primary = regions carried, hits = regions with an
 * entry, sphere_tests / bound_tests = the tests actually made, the descents' included -- they depend on J, and at J = 1 they are the
 * one-lane walk's.  The calls use rt_overlap_spheres's workspace, for n * J counts, and take their turn with the overlap, box,
 * swept-overlap and first-contact calls of their scene. */
/* Host memory.  RT_ERR_INVALID_ARGUMENT before the device is touched for a NULL scene, planes or total_out, n == 0, a NaN margin, a
 * misaligned buffer (items_out 4 bytes, planes and gap_out REAL, offsets_out and total_out 8 bytes), gap_out without items_out,
 * capacity > 2^31 - 1, n * J > 2^26, a buffer in device memory, and -- with the region's and the plane's index -- a NaN in a plane, an
 * infinite normal component, a zero normal whose d is not -inf, a d of +inf, a finite |d| above 1e15 and a normal with
 * |n.n - 1| > 2^-10 (this catches input that was never normalised; it is no tolerance of the metric). */
rt_status rt_overlap_regions(rt_scene *scene, const void *planes, uint32_t n, double margin, uint32_t sections, uint32_t capacity,
                             int32_t *items_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats);
/* The same over DEVICE memory (total_out too), enqueued on `hip_stream` without a host synchronisation: only pointers, alignment, n, the
 * margin, the capacity and n * J are checked.  A region with a NaN carries no query; any input bits end the walk without a fault. */
rt_status rt_overlap_regions_device(rt_scene *scene, const void *planes, uint32_t n, double margin, uint32_t sections, uint32_t capacity,
                                    int32_t *items_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats,
                                    void *hip_stream);

/* ---- impact pairs (additive to ABI 5): which spheres of the scene come into contact during one step, and when ----
 * The continuous form of rt_scene_contacts.  A contacts call sees one pose: a pair that is apart at the start of a step and apart at its
 * end but passes through each other in between is in neither list.  rt_sweep_spheres moves one sphere against a scene that stands still.
 * This entry takes one displacement per item slot for the step and lists every pair i < j that comes into contact at some t in [0, 1],
 * with that t: the contact pairs' self-join with the sphere cast as its metric, both spheres moving.
 *   disp is REAL[3 n_items]: sphere k is at c_k + t d_k for t in [0, 1], d_k = disp[3k .. 3k+3].  On a dynamic scene with live and dead
 * slots it covers the capacity; a dead slot's value is not used.  For two item slots i < j with stream records {c_i, rr_i} and {c_j, rr_j}
 * -- rr is the radius squared, rounded once -- in REAL, every operation rounded once, no FMA, every root the IEEE one, every dot product
 * (x*x' + y*y') + z*z':
 *   c' = c S    r' = r S           d' = d S    E' = E S       S: the call's power of two, r: the record's radius, see below
 *   v = c_j' - c_i'          w = d_i' - d_j'                   the lower slot is the query, as for the contact pairs
 *   R = (r_j' + E') + r_i'                  RR = R * R         E = 0 for an item; see the bounds below
 *   a = dot(w, w)    b = dot(v, w)    c = dot(v, v) - RR       disc = b*b - a*c
 *   t = +inf                     if !(rr_i > 0 && rr_j > 0)
 *     = 0                        else if !(c > 0)              in contact at the start (the sphere cast's rule)
 *     = +inf                     else if !(b > 0) or disc < 0  not approaching (this covers w = 0), or passing by
 *     = c / (b + sqrt(disc))     otherwise                     the smaller root; no division by a
 * The pair (i, j) is an IMPACT when t <= 1.  The root form never divides by a, so equal displacements need no special case, and it does
 * not cancel for slow relative motion.  A dead item (rr = -inf) is never part of a pair, as i or as j; a sphere whose rr is 0 behaves
 * like one.  rust_tracer_amd.pair_impacts restates t in numpy, bit for bit.
 *   S.  a, b and c are of the second degree in a length and disc of the fourth; t has none.  So that b*b and a*c stay normal numbers
 * wherever the scene is -- coordinates and displacements up to 1e15, no lower bound -- every input is first multiplied by S = 2^-e, which
 * is exact: M is the largest of |C.x|, |C.y|, |C.z| and r over the nodes {C, RRn} of THE SCENE'S STREAM that have RRn > 0 -- its
 * items and its bounds, as the call finds them -- and of |d.x|, |d.y|, |d.z| over its items with rr > 0; M = f 2^e with 0.5 <= f < 1, e
 * held to [MIN_EXP + 1, MAX_EXP - 2] of REAL so that S is a normal number, and S = 1 when M = 0.  A dead record contributes nothing, as
 * for D below.  Every scaled magnitude is below 1, and lengths down to 2^-31 M (f64: 2^-255 M) keep their fourth powers normal.  Wherever
 * nothing leaves the normal range S changes no bit of t: a scene and its displacements times a power of two have the same times.
 *   r.  rr decides whether a record is alive (rr > 0); the radius is the scene's own |r|, not sqrt(rr): the item's radius as the scene
 * holds it (rt_scene_create, rt_scene_update*, rt_scene_rebuild*), and a bound's as it was given or as the refit left it (rt_scene_bounds).
 * The two are the same number wherever r * r is a normal number; where it is a denormal (f32: r below 2^-63) sqrt(rr) keeps a few bits
 * of r and r keeps them all.
 * rust_tracer_amd.impact_scale restates S; pair_impacts takes it as `scale`, or computes it from the records it is given.
 *   A bound {C, RRn} that encloses its items at the start encloses them during the whole step once it is inflated by the largest
 * displacement below it.  Every call therefore first makes a MOTION TABLE parallel to the stream, one record {e.x, e.y, e.z, E} per node:
 * the ITEM node of slot j holds {d_j, 0}; a BOUND node holds {0, 0, 0, D} (stored times S, with r' added to the last field), D = max m_j * (1 + 8 EPSILON) over the live items of its
 * subtree, m_j = s >= TINY ? sqrt(s) : (|dx| + |dy|) + |dz| with s = dot(d_j, d_j) and TINY = MIN_NORMAL / EPSILON^2 (the refit's rule
 * for a length), m_j = 0 for a record without a positive rr.  max is exact: the table's bytes do not depend on how the reduction is
 * split.  The walk is the contact pairs' -- item i walks the stream BEHIND its own node -- and applies the ONE formula above to every
 * node with w = d_i' - e' and E' as stored: for an item that is the definition bit for bit; for a bound it is the cast of sphere i, with
 * its own motion, against a standing sphere of radius r + D, and the subtree is culled when !(t <= 1).  In exact arithmetic a bound's t
 * is no later than that of any item below it and is 0 whenever the query starts inside.  The result is the walk's, as for every query
 * here: it can differ from the definition over all i < j only where t lies within rounding of 1 or the pair grazes (disc within
 * rounding of 0).  A group whose live items all stand still has D = 0: its bound is the contact pairs' bound at margin 0.
 *   The list is made as the contact pairs' is -- count, exclusive scan, fill -- so it is sorted by (i, j) and the same bytes every time.
 * pairs_out (int32[2 capacity] or NULL): pair p is pairs_out[2p] = i, pairs_out[2p + 1] = j; time_out (REAL[capacity] or NULL; needs
 * pairs_out): its t.  capacity, the prefix, *total_out, offsets_out (uint64[n_items + 1] or NULL) and stats behave exactly as for
 * rt_scene_contacts.  The motion table lives in the scene's contacts workspace (made by the first impacts call, freed with the scene),
 * and impacts calls take their turn with contacts calls: they share the counts and the offsets. */
/* Host memory.  RT_ERR_INVALID_ARGUMENT before the device is touched for a NULL scene, disp or total_out, a misaligned buffer (pairs_out
 * 4 bytes, disp and time_out REAL, offsets_out and total_out 8 bytes), time_out without pairs_out, capacity > 2^31 - 1, a buffer in
 * device memory and a displacement component that is not finite or beyond +-1e15 (the scene's own bound on a length; dead slots
 * included).  Pinned memory is used in place, pageable memory goes through the call's device workspace.  Returns when the results are
 * in place.  The call is a READ in the sense of ORDER above, on static, dynamic, live and flat scenes alike. */
rt_status rt_scene_impacts(rt_scene *scene, const void *disp, uint32_t capacity, int32_t *pairs_out, void *time_out, uint64_t *offsets_out,
                           uint64_t *total_out, rt_stats *stats);
/* The same over DEVICE memory (disp and total_out too), enqueued on `hip_stream` without a host synchronisation: only pointers,
 * alignment and the capacity are checked.  Displacements outside the host entry's domain give unspecified values, never a fault: the
 * stream index only grows.  A call goes behind the contacts or impacts call before it, whichever stream that was on.  Pairs
 * p >= *total_out keep the caller's bytes.  stats != NULL: filled after an internal synchronisation of hip_stream. */
rt_status rt_scene_impacts_device(rt_scene *scene, const void *disp, uint32_t capacity, int32_t *pairs_out, void *time_out, uint64_t *offsets_out,
                                  uint64_t *total_out, rt_stats *stats, void *hip_stream);

/* ---- swept overlap lists (additive to ABI 5): what moving spheres from OUTSIDE the scene come into contact with during one step ----
 * rt_sweep_spheres moves an outside sphere against a standing scene and returns the first contact only.  rt_overlap_spheres lists every
 * item an outside sphere touches, at one pose.  rt_scene_impacts covers a whole step with both bodies moving, but its queries are the
 * scene's own items.  This entry takes a second set of bodies that moves during the step -- particles against level geometry, another
 * scene's spheres, a projectile, a swept trigger volume -- while the resident scene may move too, and lists for every body every item it
 * comes into contact with at some t in [0, 1], with that t and the contact normal.  The overlap lists' walk and list with the impact
 * pairs' metric, scale and motion table.
 *   queries is REAL[4n]: query g is {p.x, p.y, p.z, q}, the layout of a sphere array.  qdisp is REAL[3n]: query g is at p + t dq for t in
 * [0, 1], dq = qdisp[3g .. 3g+3].  disp is REAL[3 n_items] or NULL: the items' displacements exactly as rt_scene_impacts takes them (a
 * dead slot's row is not used); NULL means the scene stands still.  For a query and a node of the scene's stream with record {c, rr} and
 * motion record {e', r' + E'} (the impact pairs' motion table, below), in REAL, every operation rounded once, no FMA, every root the IEEE
 * one, every dot product (x*x' + y*y') + z*z':
 *   p' = p S    q' = q S    dq' = dq S                         c', r', d', E' as for the impact pairs
 *   v = c' - p'        w = dq' - e'         R = (r' + E') + q'      RR = R * R
 *   a = dot(w, w)   b = dot(v, w)   cc = dot(v, v) - RR   disc = b*b - a*cc
 *   t = +inf                       if !(rr > 0)
 *     = 0                          else if !(cc > 0)              in contact at the start
 *     = +inf                       else if !(b > 0) or disc < 0   not approaching (w = 0 too), or passing by
 *     = cc / (b + sqrt(disc))      otherwise
 * the impact pairs' formula with the query in the place of item i.  An item is LISTED when t <= 1; a bound CULLS when !(t <= 1).  A
 * query whose q is not >= 0 (negative, NaN) carries no query: it makes no test and its row is empty.  q = 0 is a valid query, a moving
 * point.  The excluded slot (exclude, as for rt_overlap_spheres) is tested and counted as a test, never listed and never counted as
 * found.  A dead item (rr = -inf) is never listed whatever its disp row holds, a dead bound culls at its one test, and neither adds to S
 * or to a bound's D.  rust_tracer_amd.swept_times restates t in numpy, bit for bit.
 *   The normal of an entry (normal_out) is normalized(u), u = {w.x*t - v.x, w.y*t - v.y, w.z*t - v.z}, each product and each difference
 * rounded once, normalized as everywhere here: u * (1 / sqrt(dot(u, u))).  u is the query's centre minus the touched sphere's centre at
 * time t (times S): the normal points from the touched sphere to the query, the direction rt_sweep_spheres uses.  Centres that coincide
 * at t = 0 give u = 0; the normal is then 0 * (1 / 0) = NaN in all three components -- there is no direction to report, and no special
 * case.  rust_tracer_amd.swept_normals restates it.
 *   S is the impact pairs' with the queries folded in: M is the largest of |C.x|, |C.y|, |C.z| and r over the stream's nodes with
 * RRn > 0, of |d.x|, |d.y|, |d.z| over the items with rr > 0 (absent when disp is NULL), and of |p.x|, |p.y|, |p.z|, q, |dq.x|, |dq.y|,
 * |dq.z| over ALL n queries with q >= 0 -- by query index, not through `order`, so S is the same in every order; S = 2^-e from M as
 * for the impact pairs.  A query far from the scene therefore raises M, and the floor of 2^-31 M (f64: 2^-255 M) below which a length
 * loses its fourth power counts from there: keep far-away bodies out of a batch whose scene is small.
 *   The MOTION TABLE is the impact pairs', byte for byte, for the same disp and the same S; with disp == NULL every e and D is 0 and a
 * bound is the static bound.  The walk is the overlap lists': every query walks the whole stream from node 0.  For an item the formula
 * is the definition; for a bound it is the cast of the moving query against a standing sphere of radius r + D.  The result is the
 * walk's: it differs from the definition over all items only where t lies within rounding of 1 or the pair grazes.
 *   items_out (int32[capacity] or NULL): the item slot of every entry; time_out (REAL[capacity] or NULL; needs items_out): its t;
 * normal_out (REAL[3 capacity] or NULL; needs items_out): its normal.  capacity, the exact prefix ("nothing behind it is touched"),
 * capacity == 0 or items_out == NULL (the second walk is skipped), the order of the entries -- sorted by (g, item slot) --, the same
 * bytes every time and in every order, offsets_out (uint64[n + 1] or NULL), *total_out (always the full count) and stats (primary =
 * queries carried, hits = queries with an entry, the tests of the counting pass) behave exactly as for rt_overlap_spheres.
 *   The counts, offsets and block sums are the overlap lists' workspace (it grows with the largest n seen); this entry's motion table is
 * a second table of that workspace, sized as the impact pairs', made by the first swept call and freed with the scene.  A swept call
 * takes its turn with overlap calls only and never waits for a contacts or impacts call. */
/* Host memory.  RT_ERR_INVALID_ARGUMENT before the device is touched for a NULL scene, queries, qdisp or total_out, n == 0, a
 * misaligned buffer (items_out, exclude, order 4 bytes; queries, qdisp, disp, time_out, normal_out REAL; offsets_out and total_out 8
 * bytes), time_out or normal_out without items_out, capacity > 2^31 - 1, a buffer in device memory, a centre, qdisp or disp component
 * that is not finite or beyond +-1e15, a q that is NaN, negative, infinite or above 1e15, and an order that is no permutation of
 * 0 .. n-1.  Pinned memory is used in place, pageable memory goes through the call's device workspace.  Returns when the results are
 * in place.  The call is a READ in the sense of ORDER above, on static, dynamic, live and flat scenes alike. */
rt_status rt_swept_overlaps(rt_scene *scene, const void *queries, const void *qdisp, uint32_t n, const void *disp, const int32_t *exclude,
                            const uint32_t *order, uint32_t capacity, int32_t *items_out, void *time_out, void *normal_out, uint64_t *offsets_out,
                            uint64_t *total_out, rt_stats *stats);
/* The same over DEVICE memory (total_out too), enqueued on `hip_stream` without a host synchronisation (but see the workspace above):
 * only pointers, alignment, n and the capacity are checked.  An order entry >= n carries no query, and a query that no thread carries
 * has count 0; any input bits give unspecified values, never a fault.  A call goes behind the overlap or swept call before it, whichever
 * stream that was on.  Entries e >= *total_out keep the caller's bytes.  stats != NULL: filled after an internal synchronisation of
 * hip_stream. */
rt_status rt_swept_overlaps_device(rt_scene *scene, const void *queries, const void *qdisp, uint32_t n, const void *disp, const int32_t *exclude,
                                   const uint32_t *order, uint32_t capacity, int32_t *items_out, void *time_out, void *normal_out,
                                   uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats, void *hip_stream);

/* ---- first contacts (additive to ABI 5): each moving outside sphere's EARLIEST contact with the scene during one step ----
 * rt_swept_overlaps lists every contact of the step: a count walk, a scan and a fill walk.  A caller that steps bodies asks first how far
 * each body can go before it touches anything, and what it touches -- conservative advancement, a projectile, a particle that stops or
 * bounces at its first hit, time-of-impact ordering.  rt_sweep_spheres answers that only against a scene that stands still.  This entry
 * is one walk with one fixed-size result per query: rt_sweep_spheres's shrinking window on rt_swept_overlaps's metric.
 *   queries (REAL[4n]), qdisp (REAL[3n]), disp (REAL[3 n_items] or NULL: the scene stands still), exclude (int32[n] or NULL) and order
 * (uint32[n] or NULL) are rt_swept_overlaps's, in layout, rules and meaning.  mode is rt_sweep_spheres's.  The time t of a query against
 * a stream node is rt_swept_overlaps's, bit for bit: the same formula, the same S -- the queries folded in by index whatever the order --,
 * the same motion table, the same dead records; q = 0 is a moving point, and a query whose q is not >= 0 carries no query: no test, no
 * result.
 *   The walk is rt_swept_overlaps's: from node 0, in stream order.  Every query carries best = 1, found = false, and one predicate serves
 * both kinds of node:  beats(t) = found ? t < best : t <= best.  A BOUND is entered when its t beats, else its subtree is culled.  An ITEM
 * whose slot is not the query's exclude and whose t beats becomes the result: best = t, found = true.  The excluded item is tested and
 * counted as a test, and never becomes the result.  The query is finished as soon as found && best == 0 (a start in contact: nothing
 * beats it) and, RT_SWEEP_ANY, as soon as found -- some contact of the step, found sooner; its t is that item's, not the earliest.  On
 * a tie the first item in stream order wins, which is the lowest slot; a contact at exactly t = 1 is found, and a later one at t = 1
 * does not replace it.  The result is the walk's, as for every query here.  In RT_SWEEP_NEAREST it is the smallest t of the query's
 * rt_swept_overlaps row at its lowest slot wherever no bound's t lies within rounding of an item's below it; a result exists exactly
 * where that row is not empty.
 *   time_out (REAL[n]): best, or +inf when nothing was found or no query was carried.  item_out (int32[n] or NULL): the slot, or -1.
 * normal_out (REAL[3n] or NULL): rt_swept_overlaps's normal of that (query, item) at best -- rust_tracer_amd.swept_normals restates it,
 * NaN where the centres coincide at t = 0 -- and {0, 0, 0} when there is no result.  The bytes and the counters are the same in every
 * order.  stats (may be NULL): primary = queries carried, hits = queries with a result, sphere_tests / bound_tests / tests_executed,
 * every other counter 0; asking for it runs the counting flavour (same bytes).
 *   The motion table and the magnitude word are rt_swept_overlaps's: a first-contacts call takes its turn with the overlap and swept
 * calls on its scene (and never waits for a contacts or impacts call); it brings no counts, and the list workspace does not grow for it. */
/* Host memory.  RT_ERR_INVALID_ARGUMENT before the device is touched for a NULL scene, queries, qdisp or time_out, an unknown mode,
 * n == 0, a misaligned buffer (item_out, exclude, order 4 bytes; queries, qdisp, disp, time_out, normal_out REAL), a buffer in device
 * memory, a centre, qdisp or disp component that is not finite or beyond +-1e15, a q that is NaN, negative, infinite or above 1e15, and
 * an order that is no permutation of 0 .. n-1.  Pinned memory is used in place, pageable memory goes through the call's device
 * workspace.  Returns when the results are in place.  The call is a READ in the sense of ORDER above, on static, dynamic, live and flat
 * scenes alike. */
rt_status rt_first_contacts(rt_scene *scene, rt_sweep mode, const void *queries, const void *qdisp, uint32_t n, const void *disp, const int32_t *exclude,
                            const uint32_t *order, void *time_out, int32_t *item_out, void *normal_out, rt_stats *stats);
/* The same over DEVICE memory, enqueued on `hip_stream` without a host synchronisation: only pointers, alignment, n and the mode are
 * checked.  An order entry >= n carries no query and leaves that thread's outputs alone; a query that no thread carries keeps the
 * caller's bytes, and still counts for S.  Any input bits end the walk without a fault.  A call goes behind the overlap, swept or
 * first-contacts call before it, whichever stream that was on.  stats != NULL: filled after an internal synchronisation of hip_stream. */
rt_status rt_first_contacts_device(rt_scene *scene, rt_sweep mode, const void *queries, const void *qdisp, uint32_t n, const void *disp,
                                   const int32_t *exclude, const uint32_t *order, void *time_out, int32_t *item_out, void *normal_out, rt_stats *stats,
                                   void *hip_stream);

/* ---- contact islands (additive to ABI 5): the connected groups of touching spheres ----
 * A caller that steps spheres wants one thing straight behind the pair list: which spheres belong together -- what it puts to sleep,
 * solves on its own, merges into a cluster or counts as one floating piece.  These entries give that without the pair list ever
 * existing: one int32 per sphere.
 *   E is the set of pairs rt_scene_contacts lists for this scene and `margin` -- the walk's pairs, lower slot as the query, its behaviour
 * on bounds that do not enclose included.  G is the graph on the LIVE item slots with the edges E; a slot is live exactly when the
 * contacts walk gives it a query: it has a node in the stream and its rr > 0.
 *   label_out (int32[n_items], required): label[i] = the smallest slot of i's connected component of G; -1 for a slot that is not live;
 *     a live slot without a contact is an island of one, label[i] = i.
 *   index_out (int32[n_items] or NULL): index[i] = the number of islands whose label is below label[i] -- dense, 0 .. n_islands - 1, in
 *     ascending label order; -1 where label[i] is -1.
 *   size_out (uint32[n_items] or NULL): size[i] = the slots of i's island; 0 where label[i] is -1.
 *   n_islands_out (uint64 or NULL): the number of i with label[i] == i.
 * The IMPACT form is the same with E the pairs rt_scene_impacts lists for `disp`: the groups a continuous-collision step has to resolve
 * together.
 *   The walk is the pair entries' own, test for test; where it would list a pair it unites the two slots in a union-find in which the
 * lower root always wins (a root changes only by a compare-and-swap from itself, so the root of every component ends as its minimum).
 * The labels are therefore one fixed function of the edge set, whatever order the lanes unite in: the same bytes every time, like every
 * query here.  stats (may be NULL) is exactly what the counting pass of rt_scene_contacts, or rt_scene_impacts, reports for the same
 * arguments: primary = live slots, hits = slots that are the lower slot of a pair, sphere_tests / bound_tests / tests_executed, every
 * other counter 0; asking for it runs the counting flavour (same bytes).
 *   The forest -- two uint32 per item slot -- is made by the first islands call and freed with the scene.  An islands call takes its
 * turn with the contacts and impacts calls of its scene: it uses their counts and offsets, and the impact form their motion table. */
/* Host memory.  RT_ERR_INVALID_ARGUMENT before the device is touched for a NULL scene or label_out, a NaN margin, a misaligned buffer
 * (label_out, index_out, size_out 4 bytes, n_islands_out 8 bytes) and a buffer in device memory.  Pinned memory is used in place,
 * pageable memory goes through the call's device workspace.  Returns when the results are in place.  The call is a READ in the sense of
 * ORDER above, on static, dynamic, live and flat scenes alike. */
rt_status rt_scene_islands(rt_scene *scene, double margin, int32_t *label_out, int32_t *index_out, uint32_t *size_out, uint64_t *n_islands_out,
                           rt_stats *stats);
/* The same over DEVICE memory (n_islands_out too), enqueued on `hip_stream` without a host synchronisation: only pointers and alignment
 * are checked.  A call goes behind the contacts, impacts or islands call before it, whichever stream that was on.  stats != NULL:
 * filled after an internal synchronisation of hip_stream. */
rt_status rt_scene_islands_device(rt_scene *scene, double margin, int32_t *label_out, int32_t *index_out, uint32_t *size_out, uint64_t *n_islands_out,
                                  rt_stats *stats, void *hip_stream);
/* The impact form, host memory: disp is REAL[3 n_items] exactly as rt_scene_impacts takes it, and is refused as there -- NULL,
 * misaligned, a component that is not finite or beyond +-1e15 -- next to what rt_scene_islands refuses. */
rt_status rt_scene_impact_islands(rt_scene *scene, const void *disp, int32_t *label_out, int32_t *index_out, uint32_t *size_out, uint64_t *n_islands_out,
                                  rt_stats *stats);
/* The impact form over DEVICE memory (disp too), as rt_scene_islands_device: displacements outside the host entry's domain give
 * unspecified labels, never a fault. */
rt_status rt_scene_impact_islands_device(rt_scene *scene, const void *disp, int32_t *label_out, int32_t *index_out, uint32_t *size_out,
                                         uint64_t *n_islands_out, rt_stats *stats, void *hip_stream);

/* Bytes rt_render_tiles writes for this tile list (4 * total area), or 0 on an invalid list. */
uint64_t rt_tiles_rgba_bytes(const rt_region *tiles, uint32_t n_tiles);

/* Device self-test: compares the traversal loops' lean correctly-rounded f32 sqrt with the compiler's IEEE sqrt on
 * ALL 2^32 bit patterns; *mismatches must come back 0 (first_bad_bits = 0xFFFFFFFF).  ~10 ms on an MI355X. */
rt_status rt_selftest_sqrt(int device, uint64_t *mismatches, uint32_t *first_bad_bits);
/* The same for the lean reciprocal of Vector::normalized (vec.rs:87-95, `len.recip()`): against the compiler's IEEE division
 * 1.0f / x on all 2^32 bit patterns, and through normalized() itself. */
rt_status rt_selftest_rcp(int device, uint64_t *mismatches, uint32_t *first_bad_bits);

const char *rt_strerror(rt_status status);
/* Detail of the last RT_ERR_HIP on the calling thread (static thread-local storage; never NULL). */
const char *rt_last_error_message(void);
int rt_abi_version(void);

/* Which kernels the LAST render call of the calling thread launched (read-only diagnostic; the bytes never depend on it):
 *   RT_LAUNCH_TWO_RAYS         the hierarchy walk with two rays per lane (k_render_skip2: large frames / large scenes)
 *   RT_LAUNCH_COOPERATIVE      the launch carried lane-cooperative quads (the heaviest 2x2-pixel quads of a small pass)
 *   RT_LAUNCH_SAMPLE_PARALLEL  one thread per SAMPLE + an ordered resolve pass (samples_per_pixel > 1)
 *   RT_LAUNCH_ORDERED          blocks dispatched most-expensive-first from the scene's cost map (else: through the tile table)
 *   RT_LAUNCH_FLAT_PIPELINE    RT_TRAVERSAL_FLAT's wavefront pipeline
 *   RT_LAUNCH_COUNTING         the counting flavour of the kernels (the call asked for rt_stats)
 *   RT_LAUNCH_FAST_KERNEL      the single-pass kernel of steady-state frames (f32, one sample per pixel, ordered: k_render_skip_fast)
 *   RT_LAUNCH_TIGHT_BOUNDS     the walk read the scene's tight streams: bounds shrunk around their items at no change to any byte
 *   RT_LAUNCH_TIGHT_COSTS      (with RT_LAUNCH_TIGHT_BOUNDS and RT_LAUNCH_ORDERED) the dispatch order was built from costs counted on those
 *                              tight streams, not on the scene's given ones
 *   RT_LAUNCH_WALK_BOUNDS      (with RT_LAUNCH_TIGHT_BOUNDS) the walk's filters read the scene's per-walk streams: a cone from the eye for
 *                              the primary rays, a disc across the light for the shadow rays, at no change to any byte
 *   RT_LAUNCH_LEAN_BOUNDS      (with RT_LAUNCH_WALK_BOUNDS) the primary walk settled the bounds that carry a cone from the filter's own dot product,
 *                              without the reference's arithmetic on the bound, at no change to any byte */
enum { RT_LAUNCH_TWO_RAYS = 1u, RT_LAUNCH_COOPERATIVE = 2u, RT_LAUNCH_SAMPLE_PARALLEL = 4u, RT_LAUNCH_ORDERED = 8u, RT_LAUNCH_FLAT_PIPELINE = 16u,
       RT_LAUNCH_COUNTING = 32u, RT_LAUNCH_FAST_KERNEL = 64u, RT_LAUNCH_TIGHT_BOUNDS = 128u, RT_LAUNCH_TIGHT_COSTS = 256u, RT_LAUNCH_WALK_BOUNDS = 512u,
       RT_LAUNCH_LEAN_BOUNDS = 1024u };
uint32_t rt_last_launch_flags(void);

/* The toolchain this library was built with, e.g. "hipcc: HIP version: 7.2.x ... | clang ... | kernels <sha1 of the kernel sources>"
 * (static storage).  The generated traversal loops are gfx950 assembly whose register windows were validated against THIS compiler:
 * tests/test_kernel_resources.py pins the string together with every hot kernel's register counts. */
const char *rt_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* RTRACE_HIP_H */
