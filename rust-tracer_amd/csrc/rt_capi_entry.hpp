// rt_capi_entry.hpp -- part of rt_capi.hip: the entry points of include/rtrace_hip.h (and, with -DRT_TEST_HOOKS, csrc/rt_debug.h) for one device.
// (included by rt_capi.hip where its text used to stand: nothing here is a header of its own)

int rt_abi_version(void) { return RTRACE_HIP_ABI_VERSION; }

#ifdef RT_TEST_HOOKS
rt_status rt_debug_set(int key, long long value)
{
    if (key < 0 || key >= RT_DEBUG_KEYS) { snprintf(g_err, sizeof g_err, "rt_debug_set: unknown key %d", key); return RT_ERR_INVALID_ARGUMENT; }
    g_knob[key].store(value < 0 ? -1 : value, std::memory_order_relaxed);
    return RT_OK;
}

long long rt_debug_count(int counter)
{
    return counter >= 0 && counter < RT_DEBUG_COUNTERS ? g_count[counter].load(std::memory_order_relaxed) : -1;
}

// Test infrastructure (csrc/rt_debug.h): the flat scan's conservative filter against the exact discriminant, for every primary
// ray of a width x height x spp frame and every item.  counts: {disc >= 0, bound >= 0, disc >= 0 && bound < 0} primary, then shadow.
rt_status rt_debug_flat_filter_check(rt_scene *s, uint32_t width, uint32_t height, uint32_t spp, unsigned long long counts[6])
{
    if (!s || !counts || !width || !height || !spp) return RT_ERR_INVALID_ARGUMENT;
    if (rt_status fst = ensure_flat(s); fst != RT_OK) return fst;
    HIP_TRY(hipSetDevice(s->device));
    unsigned long long *d = nullptr;
    HIP_TRY(hipMalloc(&d, 6 * sizeof(unsigned long long)));
    struct Free { unsigned long long *p; ~Free() { (void)hipFree(p); } } fr{ d };
    HIP_TRY(hipMemset(d, 0, 6 * sizeof(unsigned long long)));
    const uint64_t px = (uint64_t)width * height;
    if (s->precision != RT_F32) {
        hipLaunchKernelGGL(rt::k_flat_filter_check_f64, dim3((unsigned)((px + rt::kBlockThreads - 1) / rt::kBlockThreads), spp * spp), dim3(rt::kBlockThreads), 0,
                           nullptr, flat_view_of<double>(s), flat_f64_view_of(s), (const unsigned *)nullptr, width, height, spp, d);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(counts, d, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return RT_OK;
    }
    hipLaunchKernelGGL(rt::k_flat_filter_check, dim3((unsigned)((px + rt::kBlockThreads - 1) / rt::kBlockThreads), spp * spp), dim3(rt::kBlockThreads), 0,
                       nullptr, flat_sc_view_of(s), width, height, spp, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(counts, d, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RT_OK;
}

rt_status rt_debug_wave_trace(const char *path)
{
    std::lock_guard<std::mutex> lk(g_trace_mu);
    g_trace_path = path ? path : "";
    g_trace_on.store(!g_trace_path.empty(), std::memory_order_relaxed);
    return RT_OK;
}

#endif  // RT_TEST_HOOKS

const char *rt_last_error_message(void) { return g_err; }

uint32_t rt_last_launch_flags(void) { return g_launch_flags; }

#ifndef RT_BUILD_INFO
#define RT_BUILD_INFO "unknown toolchain (built without csrc/Makefile)"
#endif
const char *rt_build_info(void)
{
#ifdef RT_TEST_HOOKS
    return RT_BUILD_INFO " | RT_TEST_HOOKS";
#else
    return RT_BUILD_INFO;
#endif
}

const char *rt_strerror(rt_status st)
{
    switch (st) {
    case RT_OK: return "ok";
    case RT_ERR_INVALID_ARGUMENT: return "invalid argument";
    case RT_ERR_INVALID_REGION: return "image region empty or outside the image";
    case RT_ERR_NO_DEVICE: return "no usable gfx950 device";
    case RT_ERR_HIP: return "HIP runtime or kernel failure";
    case RT_ERR_OUT_OF_MEMORY: return "out of memory";
    case RT_ERR_UNSUPPORTED: return "unsupported request";
    }
    return "unknown status";
}

// The automatic hierarchy for an arbitrary sphere list: csrc/host/hierarchy.hpp, exported so that the Python host runs the same code as the C++ one.
rt_status rt_build_hierarchy(const double *spheres, uint32_t n, uint32_t leaf_size, const double *eye, rt_precision precision,
                             void *items_out, void *bounds_out, rt_range *ranges_out, uint64_t *order_out, uint32_t *n_groups_out)
{
    if (!spheres || n == 0 || !items_out || !bounds_out || !ranges_out || !n_groups_out || (precision != RT_F32 && precision != RT_F64)) {
        snprintf(g_err, sizeof g_err, "rt_build_hierarchy: NULL argument, n == 0 or bad precision");
        return RT_ERR_INVALID_ARGUMENT;
    }
    for (size_t i = 0; i < (size_t)n * 4; ++i)
        if (!std::isfinite(spheres[i])) { snprintf(g_err, sizeof g_err, "rt_build_hierarchy: sphere %zu is not finite", i / 4); return RT_ERR_INVALID_ARGUMENT; }
    try {
        const rt_host::FlatHierarchy h = rt_host::build_hierarchy(spheres, n, leaf_size, eye);
        const size_t g = h.ranges.size() / 2;
        if (precision == RT_F32) {
            for (size_t i = 0; i < h.items.size(); ++i) static_cast<float *>(items_out)[i] = (float)h.items[i];
            for (size_t i = 0; i < h.bounds.size(); ++i) static_cast<float *>(bounds_out)[i] = (float)h.bounds[i];
        } else {
            memcpy(items_out, h.items.data(), h.items.size() * sizeof(double));
            memcpy(bounds_out, h.bounds.data(), h.bounds.size() * sizeof(double));
        }
        for (size_t i = 0; i < g; ++i) ranges_out[i] = rt_range{ h.ranges[2 * i], h.ranges[2 * i + 1] };
        if (order_out) memcpy(order_out, h.order.data(), h.order.size() * sizeof(uint64_t));
        *n_groups_out = (uint32_t)g;
    } catch (const std::exception &e) {
        snprintf(g_err, sizeof g_err, "rt_build_hierarchy: %s", e.what());
        return RT_ERR_OUT_OF_MEMORY;
    }
    return RT_OK;
}

rt_status rt_device_count(int *n)
{
    if (!n) return RT_ERR_INVALID_ARGUMENT;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c <= 0) {
        *n = 0;
        snprintf(g_err, sizeof g_err, "hipGetDeviceCount: %s", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        (void)hipGetLastError();
        return RT_ERR_NO_DEVICE;
    }
    *n = c;
    return RT_OK;
}

uint64_t rt_tiles_rgba_bytes(const rt_region *tiles, uint32_t n_tiles)
{
    if (!tiles) return 0;
    uint64_t px = 0;
    for (uint32_t i = 0; i < n_tiles; ++i) {
        if (!(tiles[i].l < tiles[i].r && tiles[i].b < tiles[i].t)) return 0;
        px += (uint64_t)(tiles[i].r - tiles[i].l) * (tiles[i].t - tiles[i].b);
    }
    return px * 4;
}

// Scene::directional_light and Scene::eye into the scene, checked as rt_scene_create documents them.
static rt_status scene_view_ok(const char *what, rt_scene *s, const void *light_unit, const void *eye)
{
    const bool f32 = s->precision == RT_F32;
    for (int k = 0; k < 3; ++k) {
        s->light[k] = f32 ? (double)static_cast<const float *>(light_unit)[k] : static_cast<const double *>(light_unit)[k];
        s->eye[k] = f32 ? (double)static_cast<const float *>(eye)[k] : static_cast<const double *>(eye)[k];
        // Bounds that keep every intermediate of primitive.rs:55-72 finite in f32 (squares of sums of coordinates stay below
        // 2e33), so no inf - inf and no NaN can arise anywhere on the path: |eye| <= 1e15 like the items, and
        // light_unit is a unit vector by contract (|component| <= 2 leaves room for rounding).
        if (!std::isfinite(s->light[k]) || !std::isfinite(s->eye[k]) || std::fabs(s->eye[k]) > 1e15 || std::fabs(s->light[k]) > 2.0) {
            snprintf(g_err, sizeof g_err, "%s: eye must be finite with |coordinate| <= 1e15, light_unit a unit vector", what);
            return RT_ERR_INVALID_ARGUMENT;
        }
    }
    {
        // a unit vector as the host's `normalized` leaves it: the flat scan's shadow filter (rt_flat_sc.hpp) bounds its rounding
        // errors with |light_unit| <= 1 + 1e-3
        const double l2 = s->light[0] * s->light[0] + s->light[1] * s->light[1] + s->light[2] * s->light[2];
        if (std::fabs(l2 - 1.0) > 2e-3) {
            snprintf(g_err, sizeof g_err, "%s: light_unit must be a unit vector (its squared length is %.6g)", what, l2);
            return RT_ERR_INVALID_ARGUMENT;
        }
    }
    return RT_OK;
}

// What rt_scene_create and rt_scene_create_dynamic check of the items, bounds and ranges before any device is looked for.  refit: the
// dynamic form whose bounds are NULL (they are refit from the items), where a range without items is an error.
static rt_status scene_items_ok(const char *what, rt_precision precision, const void *dfs_items, uint32_t n_items, const void *light_unit, const void *eye,
                                const void *bounds, const rt_range *ranges, uint32_t n_bounds, bool refit, rt_scene **out)
{
    if (!out || !dfs_items || !light_unit || !eye || n_items == 0 || (precision != RT_F32 && precision != RT_F64)) {
        snprintf(g_err, sizeof g_err, "%s: NULL argument, n_items == 0 or bad precision", what);
        return RT_ERR_INVALID_ARGUMENT;
    }
    if ((n_bounds != 0) != ((bounds != nullptr || refit) && ranges != nullptr)) {
        snprintf(g_err, sizeof g_err, "%s: bounds, ranges and n_bounds must be given together", what);
        return RT_ERR_INVALID_ARGUMENT;
    }
    const bool f32 = precision == RT_F32;
    const bool ok = f32 ? (items_valid<float>(dfs_items, n_items, true) && (!n_bounds || refit || items_valid<float>(bounds, n_bounds, false)))
                        : (items_valid<double>(dfs_items, n_items, true) && (!n_bounds || refit || items_valid<double>(bounds, n_bounds, false)));
    if (!ok) {
        snprintf(g_err, sizeof g_err, "%s: items must be finite, |v| <= 1e15, radius > 0", what);
        return RT_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t i = 0; i < n_bounds; ++i) {
        if (ranges[i].first < 0 || ranges[i].count < 0 || (uint64_t)ranges[i].first + (uint64_t)ranges[i].count > n_items) {
            snprintf(g_err, sizeof g_err, "%s: range %u outside the item array", what, i);
            return RT_ERR_INVALID_ARGUMENT;
        }
        if (refit && ranges[i].count == 0) {
            snprintf(g_err, sizeof g_err, "%s: range %u has no items: there is nothing to refit its bound from", what, i);
            return RT_ERR_INVALID_ARGUMENT;
        }
    }
    return RT_OK;
}

#ifdef RT_TEST_HOOKS
// Test infrastructure (csrc/rt_debug.h): the tight spheres rt_scene_create's scene would get (rt_tight.hpp), on the host alone.
rt_status rt_debug_tight_bounds(const float *dfs_items, uint32_t n_items, const float *light_unit, const float *eye, const float *bounds, const rt_range *ranges,
                                uint32_t n_bounds, float *spheres_out, uint8_t *tight_out, double consts_out[4])
{
    rt_scene *none = nullptr;
    if (rt_status ast = scene_items_ok("rt_debug_tight_bounds", RT_F32, dfs_items, n_items, light_unit, eye, bounds, ranges, n_bounds, false, &none); ast != RT_OK) return ast;
    if (!n_bounds || !spheres_out || !tight_out) { snprintf(g_err, sizeof g_err, "rt_debug_tight_bounds: no bounds or no output"); return RT_ERR_INVALID_ARGUMENT; }
    std::unique_ptr<rt_scene> s(new (std::nothrow) rt_scene());      // (host fields only: nothing of it ever reaches a device)
    if (!s) return RT_ERR_OUT_OF_MEMORY;
    s->precision = RT_F32; s->n_items = n_items; s->n_bounds = n_bounds;
    if (rt_status vst = scene_view_ok("rt_debug_tight_bounds", s.get(), light_unit, eye); vst != RT_OK) return vst;
    std::vector<rt::RawNode<float>> raw;
    if (rt_status st = build_raw_stream<float>(dfs_items, n_items, bounds, ranges, n_bounds, raw); st != RT_OK) return st;
    filter_constants<float>(s.get(), raw, dfs_items);
    rt_tight::Result tr;
    tight_spheres_of(s.get(), raw, tr);
    memcpy(spheres_out, bounds, sizeof(float) * 4 * n_bounds);
    memset(tight_out, 0, n_bounds);
    uint32_t b = 0;
    for (size_t i = 0; i < raw.size(); ++i) {
        if (raw[i].skip == 0u) continue;
        while (b < n_bounds && ranges[b].count == 0) ++b;                // (groups without items have no node)
        if (b >= n_bounds) break;
        memcpy(spheres_out + 4 * b, &tr.sphere[4 * i], sizeof(float) * 4);
        tight_out[b++] = tr.tight[i];
    }
    if (consts_out) {
        const rt_tight::Params p = tight_params(s.get());
        consts_out[0] = p.S; consts_out[1] = p.eta; consts_out[2] = tr.volume_ratio; consts_out[3] = (double)tight_rule(tr, raw_is_fused<float>(raw));
    }
    return RT_OK;
}

// ... and the per-walk records it would get (rt_tight.hpp build_walk), on the host alone.
static rt_status debug_walk_records(const float *dfs_items, uint32_t n_items, const float *light_unit, const float *eye, const float *bounds, const rt_range *ranges,
                                    uint32_t n_bounds, int slack, float *records_out, double frame_out[20], float *rq_out)
{
    rt_scene *none = nullptr;
    if (rt_status ast = scene_items_ok("rt_debug_walk_bounds", RT_F32, dfs_items, n_items, light_unit, eye, bounds, ranges, n_bounds, false, &none); ast != RT_OK) return ast;
    if (!n_bounds || !records_out) { snprintf(g_err, sizeof g_err, "rt_debug_walk_bounds: no bounds or no output"); return RT_ERR_INVALID_ARGUMENT; }
    std::unique_ptr<rt_scene> s(new (std::nothrow) rt_scene());      // (host fields only: nothing of it ever reaches a device)
    if (!s) return RT_ERR_OUT_OF_MEMORY;
    s->precision = RT_F32; s->n_items = n_items; s->n_bounds = n_bounds;
    if (rt_status vst = scene_view_ok("rt_debug_walk_bounds", s.get(), light_unit, eye); vst != RT_OK) return vst;
    std::vector<rt::RawNode<float>> raw;
    if (rt_status st = build_raw_stream<float>(dfs_items, n_items, bounds, ranges, n_bounds, raw); st != RT_OK) return st;
    filter_constants<float>(s.get(), raw, dfs_items);
    rt_tight::Result tr;
    tight_spheres_of(s.get(), raw, tr);
    for (size_t i = 0; i < raw.size(); ++i)
        if (tr.tight[i]) { raw[i].cx = tr.sphere[4 * i]; raw[i].cy = tr.sphere[4 * i + 1]; raw[i].cz = tr.sphere[4 * i + 2]; raw[i].r = tr.sphere[4 * i + 3]; }
    rt_tight::WalkResult wr;
    walk_records_of(s.get(), raw, tr.tight, wr, slack != 0);
    memset(records_out, 0, sizeof(float) * 12 * n_bounds);
    uint32_t b = 0;
    for (size_t i = 0; i < raw.size(); ++i) {
        if (raw[i].skip == 0u) continue;
        while (b < n_bounds && ranges[b].count == 0) ++b;                // (groups without items have no node)
        if (b >= n_bounds) break;
        float *r = records_out + 12 * b++;
        const rt_bounds::WalkOverride &o = wr.ovr[i];
        memcpy(r, &wr.eye_sphere[4 * i], sizeof(float) * 4);
        // the threshold the stream carries: max(T of the eye sphere, T'), as k_build_streams / k_build_fstreams form it
        const float vx = r[0] - (float)s->eye[0], vy = r[1] - (float)s->eye[1], vz = r[2] - (float)s->eye[2];
        const float ts = rt_bounds::primary_threshold((vx * vx + vy * vy) + vz * vz, r[3] * r[3]);
        r[4] = (o.flags & rt_bounds::kWalkPrimary) && ts > -__builtin_huge_valf() && o.tp > ts ? o.tp : ts;
        r[5] = o.tp; r[6] = o.w1; r[7] = o.w2; r[8] = o.cl; r[9] = o.r2o; r[10] = o.r2i; r[11] = (float)o.flags;
        if (rq_out) rq_out[b - 1] = (o.flags & rt_bounds::kWalkPrimary) ? o.rq : 0.0f;
    }
    if (frame_out) {
        const rt::FilterConsts &fc = s->fc;
        for (int k = 0; k < 3; ++k) { frame_out[k] = fc.m0[k]; frame_out[3 + k] = fc.e1[k]; frame_out[6 + k] = fc.e2[k]; frame_out[9 + k] = fc.l[k]; }
        frame_out[12] = fc.a0; frame_out[13] = fc.k1; frame_out[14] = fc.kc; frame_out[15] = fc.ro2; frame_out[16] = fc.S; frame_out[17] = fc.eta;
        frame_out[18] = wr.cone_ratio; frame_out[19] = wr.disc_ratio;
    }
    return RT_OK;
}
rt_status rt_debug_walk_bounds(const float *dfs_items, uint32_t n_items, const float *light_unit, const float *eye, const float *bounds, const rt_range *ranges,
                               uint32_t n_bounds, int slack, float *records_out, double frame_out[20])
{
    return debug_walk_records(dfs_items, n_items, light_unit, eye, bounds, ranges, n_bounds, slack, records_out, frame_out, nullptr);
}
// ... with Rq of every bound that carries an eye sphere (rt_filter_bounds.hpp lean_radius; 0: the bound has none and keeps the reference's test).
rt_status rt_debug_lean_bounds(const float *dfs_items, uint32_t n_items, const float *light_unit, const float *eye, const float *bounds, const rt_range *ranges,
                               uint32_t n_bounds, float *records_out, float *rq_out)
{
    if (!rq_out) { snprintf(g_err, sizeof g_err, "rt_debug_lean_bounds: no output"); return RT_ERR_INVALID_ARGUMENT; }
    return debug_walk_records(dfs_items, n_items, light_unit, eye, bounds, ranges, n_bounds, 1, records_out, nullptr, rq_out);
}
#endif  // RT_TEST_HOOKS

rt_status rt_scene_create(int device, rt_precision precision, const void *dfs_items, uint32_t n_items,
                          const void *light_unit, const void *eye, const void *bounds, const rt_range *ranges,
                          uint32_t n_bounds, rt_scene **out)
{
    if (out) *out = nullptr;
    if (rt_status ast = scene_items_ok("rt_scene_create", precision, dfs_items, n_items, light_unit, eye, bounds, ranges, n_bounds, false, out); ast != RT_OK) return ast;
    const bool f32 = precision == RT_F32;
    int ndev = 0;
    rt_status st = rt_device_count(&ndev);
    if (st != RT_OK) return st;
    if (device < 0 || device >= ndev) {
        snprintf(g_err, sizeof g_err, "device %d out of range (%d visible)", device, ndev);
        return RT_ERR_NO_DEVICE;
    }
    StageClock clk;
    const auto t_setup = std::chrono::steady_clock::now();
    auto ms_since_setup = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_setup).count(); };
    HIP_TRY(hipSetDevice(device));
    clk.lap("scene: hipSetDevice");

    std::unique_ptr<rt_scene> s(new (std::nothrow) rt_scene());
    if (!s) return RT_ERR_OUT_OF_MEMORY;
    s->device = device; s->precision = precision; s->n_items = n_items; s->n_bounds = n_bounds;
    const size_t esz = f32 ? sizeof(float) : sizeof(double);
    if (rt_status vst = scene_view_ok("rt_scene_create", s.get(), light_unit, eye); vst != RT_OK) return vst;
    auto fail = [&](rt_status code) { rt_scene_destroy(s.release()); return code; };
    hipError_t e;
    s->h_items.assign(static_cast<const unsigned char *>(dfs_items), static_cast<const unsigned char *>(dfs_items) + esz * 4 * n_items);
    if (n_bounds) s->h_bounds.assign(static_cast<const unsigned char *>(bounds), static_cast<const unsigned char *>(bounds) + esz * 4 * n_bounds);      // rt_scene_bounds
    // ONE stream carries everything this call enqueues (uploads, the kernels that derive the streams, the cost map's counting render) and is
    // the first context's stream afterwards: the null stream is never touched
    // (the first stream of a process is ~19 ms -- the runtime makes its first hardware queue, tools/init_probe.hip --, and the library's code
    // object another ~3.5 ms at its first launch: a helper asks for a kernel's attributes meanwhile, which is what loads the code object)
    std::thread code_loader;
    try {
        code_loader = std::thread([device] {
            if (hipSetDevice(device) != hipSuccess) return;
            hipFuncAttributes fa;
            (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(rt::k_upload_words));
            (void)hipGetLastError();
        });
    } catch (...) {}                              // (no thread to be had: the first launch loads the code object, as it always did)
    const double t_before_stream = ms_since_setup();
    e = hipStreamCreateWithFlags(&s->cost_stream, hipStreamNonBlocking);
    s->setup_first_stream_ms = ms_since_setup() - t_before_stream;
    clk.lap("scene: stream");
    if (code_loader.joinable()) code_loader.join();
    clk.lap("scene: code object (helper)");
    if (e != hipSuccess) return fail(hip_fail(e, "hipStreamCreate(scene)", __LINE__));
    if ((e = hipMalloc(&s->d_items, esz * 4 * n_items)) != hipSuccess) return fail(hip_fail(e, "hipMalloc(items)", __LINE__));
    {
        // everything this call uploads goes through ONE pinned arena and k_upload_words: items, the raw streams (plain + compacted: a node per
        // item and per bound, twice), the cooperative copy's tables, the filter's constants -- no hipMemcpy on the way to the first frame
        const size_t nodes = (size_t)n_items + n_bounds;
        const size_t raw_sz = f32 ? sizeof(rt::RawNode<float>) : sizeof(rt::RawNode<double>);
        const size_t want = esz * 4 * n_items + 2 * nodes * raw_sz + nodes * (sizeof(uint32_t) + sizeof(uint2)) + 64 * 1024;
        if (want <= ((size_t)1 << 30) && hipHostMalloc(reinterpret_cast<void **>(&s->h_up), want, hipHostMallocDefault) == hipSuccess) { s->up_cap = want; s->up_used = 0; }
        else { (void)hipGetLastError(); s->h_up = nullptr; }
    }
    { rt_status ust = scene_upload(s.get(), s->d_items, s->h_items.data(), esz * 4 * n_items); if (ust != RT_OK) return fail(ust); }      // (the scene's own copy of the items)
    if ((e = hipStreamSynchronize(s->cost_stream)) != hipSuccess) return fail(hip_fail(e, "upload(items)", __LINE__));
    clk.lap("scene: items");
    if (n_bounds) {
        rt_status sst = f32 ? upload_streams<float>(s.get(), dfs_items, bounds, ranges) : upload_streams<double>(s.get(), dfs_items, bounds, ranges);
        if (sst != RT_OK) return fail(sst);
        clk.lap("scene: streams (total)");
        // the cost map the dispatch orders are made from is rendered when a tile list first wants orders (cost_map_of, from the scene's worker
        // thread); here only its pinned host side, which is also where new lists' tile tables are staged (failing only costs the ordering)
        if (alloc_cost_host(s.get()) != RT_OK) { (void)hipGetLastError(); s->h_cost = nullptr; s->h_tab_stage = nullptr; }
        try { s->worker = std::thread(worker_main, s.get()); note_builder(s.get()); } catch (...) {}      // (without it a new list starts a thread of its own)
        clk.lap("scene: pinned cost arena + worker");
    }
    // (every upload has been consumed: derive_streams and upload_coop synchronise the stream behind their kernels)
    if (s->h_up) { (void)hipStreamSynchronize(s->cost_stream); (void)hipHostFree(s->h_up); s->h_up = nullptr; s->up_cap = s->up_used = 0; }
    s->setup_total_ms = ms_since_setup();
    *out = s.release();
    return RT_OK;
}

rt_status rt_scene_destroy(rt_scene *s)
{
    if (!s) return RT_OK;
    (void)hipSetDevice(s->device);
    for (std::thread &b : s->builders) if (b.joinable()) b.join();          // dispatch orders still being made in the background
    stop_worker(s);
    forget_scene(s);
    if (s->ahead.stream) { (void)hipStreamSynchronize(s->ahead.stream); (void)hipStreamDestroy(s->ahead.stream); }      // a pass rendered ahead may still be running
    s->pool.clear();
    for (auto &t : s->tables) {
        (void)hipFree(t.dev);
        for (auto &od : t.orders) release_order(od);
        for (auto &od : t.retired_orders) release_order(od);
        if (t.order_arena) (void)hipFree(t.order_arena);
        for (void *a : t.retired_arenas) (void)hipFree(a);
        if (t.landed) (void)hipEventDestroy(t.landed);
    }
    if (s->dynamic) {                                      // (its stream is part of d_dyn)
        s->d_shad = s->d_query_items = nullptr;
        if (s->cost_stream) (void)hipStreamSynchronize(s->cost_stream);
        if (s->d_dyn) (void)hipFree(s->d_dyn);
        if (s->upd_ev) (void)hipEventDestroy(s->upd_ev);
        if (s->d_rebuild) (void)hipFree(s->d_rebuild);
    }
    if (s->d_items) (void)hipFree(s->d_items);
    if (s->d_prim) (void)hipFree(s->d_prim);
    if (s->d_shad) (void)hipFree(s->d_shad);
    if (s->d_query_items) (void)hipFree(s->d_query_items);
    if (s->query_items_ev) (void)hipEventDestroy(s->query_items_ev);
    s->contacts.free_all();
    if (s->d_impacts) (void)hipFree(s->d_impacts);
    if (s->d_islands) (void)hipFree(s->d_islands);
    s->overlap.free_all();
    if (s->d_swept) (void)hipFree(s->d_swept);
    if (s->d_cprim) (void)hipFree(s->d_cprim);
    if (s->d_cshad) (void)hipFree(s->d_cshad);
    for (void *p : { s->d_xprim, s->d_xshad, s->d_xcprim, s->d_xcshad, s->d_xown, s->d_fc, s->d_coop_prim, s->d_coop_shad, s->d_cost_arena, s->d_tight, s->d_walk }) if (p) (void)hipFree(p);
    if (s->cost_stream) { (void)hipStreamSynchronize(s->cost_stream); (void)hipStreamDestroy(s->cost_stream); }
    if (s->h_cost) (void)hipHostFree(s->h_cost);
    if (s->h_up) (void)hipHostFree(s->h_up);
    if (s->ahead.ev) (void)hipEventDestroy(s->ahead.ev);
    if (s->ahead.h) (void)rt_host_free(s->ahead.h);
    if (s->ahead.h_next) (void)rt_host_free(s->ahead.h_next);
    if (s->d_fprim) (void)hipFree(s->d_fprim);
    if (s->d_fprim_rr) (void)hipFree(s->d_fprim_rr);
    if (s->d_fshad) (void)hipFree(s->d_fshad);
    for (void *p : { s->d_f64_pf, s->d_f64_sf, s->d_f64_sg }) if (p) (void)hipFree(p);
    if (s->d_pf) (void)hipFree(s->d_pf);
    if (s->d_pe) (void)hipFree(s->d_pe);
    if (s->d_sg) (void)hipFree(s->d_sg);
    if (s->d_se) (void)hipFree(s->d_se);
    delete s;
    return RT_OK;
}

// ---- dynamic scenes: the topology fixed, the spheres replaced in place, the bounds given or refit on the device (rt_dynamic.hpp) ----

rt_status rt_scene_create_dynamic(int device, rt_precision precision, const void *dfs_items, uint32_t n_items, const void *light_unit, const void *eye,
                                  const void *bounds, const rt_range *ranges, uint32_t n_bounds, rt_scene **out)
{
    if (out) *out = nullptr;
    const bool refit = n_bounds != 0 && bounds == nullptr;
    if (rt_status ast = scene_items_ok("rt_scene_create_dynamic", precision, dfs_items, n_items, light_unit, eye, bounds, ranges, n_bounds, refit, out); ast != RT_OK)
        return ast;
    int ndev = 0;
    rt_status st = rt_device_count(&ndev);
    if (st != RT_OK) return st;
    if (device < 0 || device >= ndev) {
        snprintf(g_err, sizeof g_err, "device %d out of range (%d visible)", device, ndev);
        return RT_ERR_NO_DEVICE;
    }
    const auto t_setup = std::chrono::steady_clock::now();
    auto ms_since_setup = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_setup).count(); };
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<rt_scene> s(new (std::nothrow) rt_scene());
    if (!s) return RT_ERR_OUT_OF_MEMORY;
    s->device = device; s->precision = precision; s->n_items = n_items; s->n_bounds = n_bounds; s->dynamic = true;
    if (rt_status vst = scene_view_ok("rt_scene_create_dynamic", s.get(), light_unit, eye); vst != RT_OK) return vst;
    auto fail = [&](rt_status code) { rt_scene_destroy(s.release()); return code; };
    const bool f32 = precision == RT_F32;
    const double t_before_stream = ms_since_setup();
    hipError_t e = hipStreamCreateWithFlags(&s->cost_stream, hipStreamNonBlocking);      // the scene's stream: its own updates, and its first context's
    s->setup_first_stream_ms = ms_since_setup() - t_before_stream;
    if (e != hipSuccess) return fail(hip_fail(e, "hipStreamCreate(scene)", __LINE__));
    if ((e = hipMalloc(&s->d_items, (f32 ? sizeof(float) : sizeof(double)) * 4 * n_items)) != hipSuccess) return fail(hip_fail(e, "hipMalloc(items)", __LINE__));
    st = f32 ? upload_dynamic<float>(s.get(), dfs_items, bounds, ranges) : upload_dynamic<double>(s.get(), dfs_items, bounds, ranges);
    if (st != RT_OK) return fail(st);
    s->setup_total_ms = ms_since_setup();
    *out = s.release();
    return RT_OK;
}

static rt_status update_args_ok(rt_scene *s, const void *items, const char *what)
{
    if (!s || !items) { snprintf(g_err, sizeof g_err, "%s: NULL scene or items", what); return RT_ERR_INVALID_ARGUMENT; }
    if (!s->dynamic) {
        snprintf(g_err, sizeof g_err, "%s: the scene was made by rt_scene_create and is immutable; rt_scene_create_dynamic makes one that can be updated", what);
        return RT_ERR_UNSUPPORTED;
    }
    return RT_OK;
}

rt_status rt_scene_update(rt_scene *s, const void *dfs_items, const void *bounds)
{
    if (rt_status ast = update_args_ok(s, dfs_items, "rt_scene_update"); ast != RT_OK) return ast;
    const bool f32 = s->precision == RT_F32, with_bounds = bounds && s->n_bounds;
    const bool ok = f32 ? (items_valid<float>(dfs_items, s->n_items, true) && (!with_bounds || items_valid<float>(bounds, s->n_bounds, false)))
                        : (items_valid<double>(dfs_items, s->n_items, true) && (!with_bounds || items_valid<double>(bounds, s->n_bounds, false)));
    if (!ok) {
        snprintf(g_err, sizeof g_err, "rt_scene_update: items must be finite, |v| <= 1e15, radius > 0; the scene is unchanged");
        return RT_ERR_INVALID_ARGUMENT;
    }
    std::unique_lock<std::shared_mutex> lk(s->dyn_mu);               // every host call under way has returned; none starts before this one has
    HIP_TRY(hipSetDevice(s->device));
    return dynamic_update_host(s, dfs_items, bounds);
}

rt_status rt_scene_update_device(rt_scene *s, const void *dfs_items_device, const void *bounds_device, void *hip_stream)
{
    if (rt_status ast = update_args_ok(s, dfs_items_device, "rt_scene_update_device"); ast != RT_OK) return ast;
    const uintptr_t align = (s->precision == RT_F32 ? sizeof(float) : sizeof(double)) * 4;      // one {cx, cy, cz, r} record: the kernels load it whole
    if ((reinterpret_cast<uintptr_t>(dfs_items_device) % align) != 0 || (reinterpret_cast<uintptr_t>(bounds_device) % align) != 0) {
        snprintf(g_err, sizeof g_err, "rt_scene_update_device: items and bounds must be %u-byte aligned", (unsigned)align);
        return RT_ERR_INVALID_ARGUMENT;
    }
    const ReadLock rl(s);                                            // (not while a host update is replacing the scene)
    HIP_TRY(hipSetDevice(s->device));
    return enqueue_dynamic_update(s, dfs_items_device, bounds_device, static_cast<hipStream_t>(hip_stream));
}

rt_status rt_scene_bounds(rt_scene *s, void *bounds_out)
{
    if (!s || (!bounds_out && s->n_bounds)) { snprintf(g_err, sizeof g_err, "rt_scene_bounds: NULL argument"); return RT_ERR_INVALID_ARGUMENT; }
    if (s->n_bounds == 0) return RT_OK;
    const size_t bytes = (s->precision == RT_F32 ? sizeof(float) : sizeof(double)) * 4 * s->n_bounds;
    if (!s->dynamic) { memcpy(bounds_out, s->h_bounds.data(), bytes); return RT_OK; }
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    Context *c = nullptr;
    if (rt_status st = acquire(s, &c); st != RT_OK) return st;
    Lease lease{ s, c };
    HIP_TRY(hipStreamWaitEvent(c->stream, s->upd_ev, 0));             // behind the last update, whichever stream carried it
    hipError_t e = hipMemcpyAsync(bounds_out, s->d_bounds, bytes, hipMemcpyDeviceToHost, c->stream);
    const hipError_t se = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return hip_fail(e, "rt_scene_bounds(copy)", __LINE__);
    return RT_OK;
}

// ---- live and dead slots: a dynamic scene's n_items is a capacity ----

rt_status rt_scene_update_live(rt_scene *s, const void *dfs_items, const void *bounds, const uint8_t *live)
{
    if (!live) return rt_scene_update(s, dfs_items, bounds);
    if (rt_status ast = update_args_ok(s, dfs_items, "rt_scene_update_live"); ast != RT_OK) return ast;
    const bool f32 = s->precision == RT_F32, with_bounds = bounds && s->n_bounds;
    const bool ok = f32 ? (live_items_valid<float>(dfs_items, live, s->n_items) && (!with_bounds || items_valid<float>(bounds, s->n_bounds, false)))
                        : (live_items_valid<double>(dfs_items, live, s->n_items) && (!with_bounds || items_valid<double>(bounds, s->n_bounds, false)));
    if (!ok) {
        snprintf(g_err, sizeof g_err, "rt_scene_update_live: live items must be finite, |v| <= 1e15, radius > 0; the scene is unchanged");
        return RT_ERR_INVALID_ARGUMENT;
    }
    std::unique_lock<std::shared_mutex> lk(s->dyn_mu);               // as rt_scene_update
    HIP_TRY(hipSetDevice(s->device));
    return dynamic_update_live_host(s, dfs_items, bounds, live);
}

rt_status rt_scene_update_live_device(rt_scene *s, const void *dfs_items_device, const void *bounds_device, const uint8_t *live_device, void *hip_stream)
{
    if (!live_device) return rt_scene_update_device(s, dfs_items_device, bounds_device, hip_stream);
    if (rt_status ast = update_args_ok(s, dfs_items_device, "rt_scene_update_live_device"); ast != RT_OK) return ast;
    const uintptr_t align = (s->precision == RT_F32 ? sizeof(float) : sizeof(double)) * 4;      // one {cx, cy, cz, r} record: the kernels load it whole
    if ((reinterpret_cast<uintptr_t>(dfs_items_device) % align) != 0 || (reinterpret_cast<uintptr_t>(bounds_device) % align) != 0) {
        snprintf(g_err, sizeof g_err, "rt_scene_update_live_device: items and bounds must be %u-byte aligned", (unsigned)align);
        return RT_ERR_INVALID_ARGUMENT;
    }
    const ReadLock rl(s);                                            // (not while a host update is replacing the scene)
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    return s->precision == RT_F32 ? enqueue_dynamic_update_live<float, false>(s, dfs_items_device, bounds_device, live_device, 0u, stream)
                                  : enqueue_dynamic_update_live<double, false>(s, dfs_items_device, bounds_device, live_device, 0u, stream);
}

rt_status rt_scene_live(rt_scene *s, uint8_t *live_out)
{
    if (!s || !live_out) { snprintf(g_err, sizeof g_err, "rt_scene_live: NULL argument"); return RT_ERR_INVALID_ARGUMENT; }
    if (!s->dynamic) { memset(live_out, 1, s->n_items); return RT_OK; }
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    Context *c = nullptr;
    if (rt_status st = acquire(s, &c); st != RT_OK) return st;
    Lease lease{ s, c };
    const bool resident = s->live_resident.load();                   // (what the last update enqueued left, as upd_ev is that update's event)
    HIP_TRY(hipStreamWaitEvent(c->stream, s->upd_ev, 0));
    hipError_t e = resident ? hipMemcpyAsync(live_out, s->d_live, s->n_items, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    const hipError_t se = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return hip_fail(e, "rt_scene_live(copy)", __LINE__);
    if (!resident) memset(live_out, 1, s->n_items);
    return RT_OK;
}

// Shared body of rt_render_tiles_device (frame_w == 0, tile-major output) and rt_render_frame_device (row-major frame).
static rt_status render_device(rt_scene *s, const rt_options *o, rt_traversal trav, const rt_region *tiles, uint32_t n, void *out_device,
                               unsigned frame_w, void *hip_stream, rt_stats *stats)
{
    if (!check_common(s, o, tiles, n, out_device)) return RT_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(out_device) & 3u) != 0) {
        snprintf(g_err, sizeof g_err, "the device output buffer must be 4-byte aligned");
        return RT_ERR_INVALID_ARGUMENT;
    }
    rt_status st = check_traversal(s, trav);
    if (st != RT_OK) return st;
    std::vector<rt::TileDev> tab;
    uint64_t total_px = 0; uint32_t total_blocks = 0;
    const bool flat2 = trav == RT_TRAVERSAL_FLAT;
    st = build_tile_table(o, tiles, n, tab, &total_px, &total_blocks, flat2 ? rt::kFlatBlockW : rt::kBlockW, flat2 ? rt::kFlatBlockH : rt::kBlockH);
    if (st != RT_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint8_t *out = static_cast<uint8_t *>(out_device);
    // the flat wavefront pipeline resolves per pixel with the 16x16-block table
    const bool wavefront = flat2;
    std::vector<rt::TileDev> tab16;
    uint32_t blocks16 = 0;
    if (wavefront) {
        uint64_t px16 = 0;
        if ((st = build_tile_table(o, tiles, n, tab16, &px16, &blocks16)) != RT_OK) return st;
    }
    const bool split = trav == RT_TRAVERSAL_SKIP && use_split(o->samples_per_pixel);
    if (!stats && !split && !wavefront) {
        // Fast path: a cached tile table and no per-call device state -> the call enqueues exactly one kernel.
        const rt::TileDev *d_tab = nullptr;
        rt::BlockList order;
        if ((st = device_table(s, nullptr, tab, stream, &d_tab, 0, o, &order, true, trav == RT_TRAVERSAL_SKIP && o->samples_per_pixel != 0)) != RT_OK) return st;
        if (d_tab)
            return launch_render(s, nullptr, o, trav, d_tab, (unsigned)tab.size(), total_blocks, total_px, out, frame_w, stream, nullptr, nullptr, 0, order);
    }
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    st = enqueue_pass(s, c, o, trav, tab, total_blocks, total_px, out, frame_w, stream, stats != nullptr, wavefront ? &tab16 : nullptr, blocks16);
    if (st != RT_OK) {
        // some kernels of the pass may already be enqueued and using the context's buffers: it goes back to the pool marked
        // in flight behind everything that is on the stream now
        (void)hipEventRecord(c->ev1, stream);
        (void)hipGetLastError();
        lease.inflight = true;
        return st;
    }
    if (stats) return read_stats(s, c, stream, trav, stats);
    // Asynchronous return: the context's buffers are still in use by the enqueued work, so it goes back to the pool
    // marked in-flight and is only reused once its end event has completed.
    lease.inflight = true;
    return RT_OK;
}

rt_status rt_render_tiles_device(rt_scene *s, const rt_options *o, rt_traversal trav, const rt_region *tiles, uint32_t n,
                                 void *rgba_out_device, void *hip_stream, rt_stats *stats)
{
    return render_device(s, o, trav, tiles, n, rgba_out_device, 0u, hip_stream, stats);
}

rt_status rt_render_frame_device(rt_scene *s, const rt_options *o, rt_traversal trav, const rt_region *tiles, uint32_t n,
                                 void *frame_rgba_device, void *hip_stream, rt_stats *stats)
{
    return render_device(s, o, trav, tiles, n, frame_rgba_device, o ? (unsigned)o->width : 0u, hip_stream, stats);
}

// How the bytes of a pass get into the caller's HOST buffer.
//   pinned   (rt_host_alloc / rt_host_register memory, or any hipHostMalloc'd / registered range): the render kernel stores
//            straight into it over PCIe (no device copy of the frame, no separate D2H) or, as an alternative, renders
//            into device memory followed by ONE asynchronous D2H at full link speed;
//   pageable (Vec<u8>, malloc): the runtime has to bounce through pinned memory and a CPU copy whatever we do; one
//            hipMemcpyAsync to the caller's pointer, or our own pinned staging in 1 MiB chunks with the CPU copy of chunk k
//            overlapping the DMA of chunk k+1.
//   scattered (the merged rt_render_region passes: every tile has its own destination): the kernel stores into the context's
//            pinned staging and the CPU hands each caller its 16 KB.
enum HostCopy { kCopyAuto = 0, kCopyDirect = 1, kCopyStaged = 2, kCopyZero = 3, kCopyZeroStaged = 4 };

// (HostDest and classify_host_pointer, which tell the three apart: rt_capi_query.hpp)

constexpr size_t kStageChunk = 1u << 20;

// rt_render_tiles for a list of tiles whose bytes go to host memory.  `scatter` (optional, n entries): tile i's bytes go to
// scatter[i] instead of lying back to back at rgba_out (the coalesced rt_render_region path).
static rt_status render_tiles_host(rt_scene *s, const rt_options *o, rt_traversal trav, const rt_region *tiles, uint32_t n,
                                   uint8_t *rgba_out, uint8_t *const *scatter, rt_stats *stats, bool cacheable)
{
    rt_status st = check_traversal(s, trav);
    if (st != RT_OK) return st;
    std::vector<rt::TileDev> tab;
    uint64_t total_px = 0; uint32_t total_blocks = 0;
    const bool flat2 = trav == RT_TRAVERSAL_FLAT;
    st = build_tile_table(o, tiles, n, tab, &total_px, &total_blocks, flat2 ? rt::kFlatBlockW : rt::kBlockW,
                                    flat2 ? rt::kFlatBlockH : rt::kBlockH);
    if (st != RT_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    HostDest dest;
    if (!scatter) {
        dest = classify_host_pointer(rgba_out);
        if (dest.bad) {
            snprintf(g_err, sizeof g_err, "rt_render_tiles: rgba_out is device memory; use rt_render_tiles_device");
            return RT_ERR_INVALID_ARGUMENT;
        }
    }
    long long mode = knob(RT_DEBUG_HOST_COPY);
    if (mode <= 0) mode = dest.pinned ? (dest.dev_alias ? kCopyZero : kCopyDirect) : kCopyDirect;
    if (scatter) mode = kCopyZeroStaged;
    if (mode == kCopyZero && (!dest.dev_alias || dest.room < (size_t)total_px * 4)) mode = kCopyDirect;
    if (mode == kCopyStaged && dest.pinned) mode = kCopyDirect;          // staging a pinned destination is pointless

    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    const size_t bytes = (size_t)total_px * 4;
    uint8_t *d_target = nullptr;
    if (mode == kCopyStaged || mode == kCopyZeroStaged) {
        if (c->h_out_cap < bytes) {
            if (c->h_out) HIP_TRY(hipHostFree(c->h_out));
            c->h_out = nullptr; c->h_out_cap = 0;
            HIP_TRY(hipHostMalloc(&c->h_out, std::max(bytes, (size_t)1 << 20), hipHostMallocDefault));
            c->h_out_cap = std::max(bytes, (size_t)1 << 20);
        }
    }
    if (mode == kCopyZero) {
        d_target = dest.dev_alias;
    } else if (mode == kCopyZeroStaged) {
        void *alias = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&alias, c->h_out, 0));
        d_target = static_cast<uint8_t *>(alias);
    } else {
        if (c->out_cap < bytes) {
            if (c->d_out) HIP_TRY(hipFree(c->d_out));
            c->d_out = nullptr; c->out_cap = 0;
            HIP_TRY(hipMalloc(&c->d_out, bytes));
            c->out_cap = bytes;
        }
        d_target = c->d_out;
    }
    std::vector<rt::TileDev> tab16;
    uint32_t blocks16 = 0;
    const bool wavefront = flat2;
    if (wavefront) {
        uint64_t px16 = 0;
        if ((st = build_tile_table(o, tiles, n, tab16, &px16, &blocks16)) != RT_OK) return st;
    }
    st = enqueue_pass(s, c, o, trav, tab, total_blocks, total_px, d_target, 0u, c->stream, stats != nullptr, wavefront ? &tab16 : nullptr, blocks16,
                      cacheable);
    // from here on kernels of this pass may be running: an error return first waits for them (they write d_out / h_out or the caller's
    // pinned buffer), so that the context is not handed to the next caller with work in flight
#define HIP_DRAIN(expr)                                                                                                   \
    do {                                                                                                                  \
        hipError_t e__ = (expr);                                                                                          \
        if (e__ != hipSuccess) { (void)hipStreamSynchronize(c->stream); return hip_fail(e__, #expr, __LINE__); }          \
    } while (0)
    if (st != RT_OK) { (void)hipStreamSynchronize(c->stream); (void)hipGetLastError(); return st; }
    if (mode == kCopyDirect) {
        HIP_DRAIN(hipMemcpyAsync(rgba_out, c->d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    } else if (mode == kCopyStaged) {
        const size_t chunks = (bytes + kStageChunk - 1) / kStageChunk;
        while (c->chunk_ev.size() < chunks) {
            hipEvent_t e = nullptr;
            HIP_DRAIN(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            c->chunk_ev.push_back(e);
        }
        for (size_t k = 0; k < chunks; ++k) {
            const size_t off = k * kStageChunk, len = std::min(kStageChunk, bytes - off);
            HIP_DRAIN(hipMemcpyAsync(c->h_out + off, c->d_out + off, len, hipMemcpyDeviceToHost, c->stream));
            HIP_DRAIN(hipEventRecord(c->chunk_ev[k], c->stream));
        }
        // the CPU copy of chunk k runs while the DMA engine moves chunk k + 1
        size_t tile = 0, tile_off = 0;                    // scatter cursor: current tile and bytes of it already delivered
        for (size_t k = 0; k < chunks; ++k) {
            HIP_DRAIN(hipEventSynchronize(c->chunk_ev[k]));
            const size_t off = k * kStageChunk, len = std::min(kStageChunk, bytes - off);
            if (!scatter) { memcpy(rgba_out + off, c->h_out + off, len); continue; }
            size_t pos = off;
            while (pos < off + len) {
                const size_t tbytes = (size_t)(tiles[tile].r - tiles[tile].l) * (tiles[tile].t - tiles[tile].b) * 4;
                const size_t take = std::min(tbytes - tile_off, off + len - pos);
                memcpy(scatter[tile] + tile_off, c->h_out + pos, take);
                pos += take; tile_off += take;
                if (tile_off == tbytes) { ++tile; tile_off = 0; }
            }
        }
    }
    rt_status rst = RT_OK;
    if (stats) rst = read_stats(s, c, c->stream, trav, stats);          // synchronises the stream
    else HIP_DRAIN(hipStreamSynchronize(c->stream));
#undef HIP_DRAIN
    if (rst == RT_OK && mode == kCopyZeroStaged) {
        size_t off = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const size_t tbytes = (size_t)(tiles[i].r - tiles[i].l) * (tiles[i].t - tiles[i].b) * 4;
            memcpy(scatter ? scatter[i] : rgba_out + off, c->h_out + off, tbytes);
            off += tbytes;
        }
    }
    return rst;
}

rt_status rt_render_tiles(rt_scene *s, const rt_options *o, rt_traversal trav, const rt_region *tiles, uint32_t n,
                          uint8_t *rgba_out, rt_stats *stats)
{
    if (!check_common(s, o, tiles, n, rgba_out)) return RT_ERR_INVALID_ARGUMENT;
    return render_tiles_host(s, o, trav, tiles, n, rgba_out, nullptr, stats, true);
}


// rt_render_tiles with delivery in completion order: the list is cut into batches that are ALL enqueued at once (kernels storing
// into pinned staging), and each batch's buckets are handed to the callback as soon as that batch's event has fired -- while the
// later batches are still rendering.  What render.rs:301-307 does with its channel, without serialising launches behind host calls.
rt_status rt_render_tiles_stream(rt_scene *s, const rt_options *o, rt_traversal trav, const rt_region *tiles, uint32_t n,
                                 rt_tile_callback callback, void *user)
{
    if (!callback) { snprintf(g_err, sizeof g_err, "rt_render_tiles_stream: NULL callback"); return RT_ERR_INVALID_ARGUMENT; }
    if (!check_common(s, o, tiles, n, tiles)) return RT_ERR_INVALID_ARGUMENT;
    rt_status st = check_traversal(s, trav);
    if (st != RT_OK) return st;
    const bool flat2 = trav == RT_TRAVERSAL_FLAT;
    // batches: at least kStreamBatch buckets (enough workgroups to fill the device), at most kStreamMaxBatches of them (each batch keeps
    // a cached tile table on the device)
    constexpr uint32_t kStreamBatch = 64, kStreamMaxBatches = 16;
    const uint32_t per = std::max(kStreamBatch, (n + kStreamMaxBatches - 1) / kStreamMaxBatches), n_batches = (n + per - 1) / per;
    struct Batch { std::vector<rt::TileDev> tab, tab16; uint64_t px = 0; uint32_t blocks = 0, blocks16 = 0; size_t byte_off = 0; };
    std::vector<Batch> batches(n_batches);
    size_t total_bytes = 0;
    for (uint32_t k = 0; k < n_batches; ++k) {
        Batch &b = batches[k];
        const uint32_t first = k * per, cnt = std::min(per, n - first);
        if ((st = build_tile_table(o, tiles + first, cnt, b.tab, &b.px, &b.blocks, flat2 ? rt::kFlatBlockW : rt::kBlockW, flat2 ? rt::kFlatBlockH : rt::kBlockH)) != RT_OK) return st;
        if (flat2) { uint64_t px16 = 0; if ((st = build_tile_table(o, tiles + first, cnt, b.tab16, &px16, &b.blocks16)) != RT_OK) return st; }
        b.byte_off = total_bytes;
        total_bytes += (size_t)b.px * 4;
    }
    HIP_TRY(hipSetDevice(s->device));
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    if (c->h_out_cap < total_bytes) {
        if (c->h_out) HIP_TRY(hipHostFree(c->h_out));
        c->h_out = nullptr; c->h_out_cap = 0;
        HIP_TRY(hipHostMalloc(&c->h_out, std::max(total_bytes, (size_t)1 << 20), hipHostMallocDefault));
        c->h_out_cap = std::max(total_bytes, (size_t)1 << 20);
    }
    void *alias = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&alias, c->h_out, 0));
    while (c->chunk_ev.size() < n_batches) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->chunk_ev.push_back(e);
    }
    auto drain = [&](rt_status code) { (void)hipStreamSynchronize(c->stream); (void)hipGetLastError(); return code; };   // nothing may still be writing the staging
    for (uint32_t k = 0; k < n_batches; ++k) {
        Batch &b = batches[k];
        st = enqueue_pass(s, c, o, trav, b.tab, b.blocks, b.px, static_cast<uint8_t *>(alias) + b.byte_off, 0u, c->stream, false, flat2 ? &b.tab16 : nullptr,
                          b.blocks16, true);
        if (st != RT_OK) return drain(st);
        hipError_t e = hipEventRecord(c->chunk_ev[k], c->stream);
        if (e != hipSuccess) return drain(hip_fail(e, "hipEventRecord(stream batch)", __LINE__));
    }
    for (uint32_t k = 0; k < n_batches; ++k) {
        hipError_t e = hipEventSynchronize(c->chunk_ev[k]);
        if (e != hipSuccess) return drain(hip_fail(e, "hipEventSynchronize(stream batch)", __LINE__));
        const uint32_t first = k * per, cnt = std::min(per, n - first);
        size_t off = batches[k].byte_off;
        for (uint32_t i = first; i < first + cnt; ++i) {
            callback(user, i, &tiles[i], c->h_out + off);
            off += (size_t)(tiles[i].r - tiles[i].l) * (tiles[i].t - tiles[i].b) * 4;
        }
    }
    return RT_OK;
}

// The same streaming pass for a writer that keeps its image in the FILE's pixel format (render.rs:373-401): the buckets of a batch are
// rendered tile-major into device memory and k_encode_tiles puts them -- converted -- into their place in the caller's row-major frame;
// memory this library pinned is written by that kernel itself, anything else through pinned staging and a CPU copy of the batch's rows.
rt_status rt_render_frame_stream(rt_scene *s, const rt_options *o, rt_traversal trav, const rt_region *tiles, uint32_t n, rt_frame_format format,
                                 uint8_t *frame_out, rt_batch_callback callback, void *user)
{
    if (!check_common(s, o, tiles, n, frame_out)) return RT_ERR_INVALID_ARGUMENT;
    if (format != RT_FRAME_RGBA && format != RT_FRAME_RGB && format != RT_FRAME_GREY) { snprintf(g_err, sizeof g_err, "rt_render_frame_stream: unknown frame format %d", (int)format); return RT_ERR_INVALID_ARGUMENT; }
    if ((reinterpret_cast<uintptr_t>(frame_out) & 3u) != 0) { snprintf(g_err, sizeof g_err, "rt_render_frame_stream: frame_out must be 4-byte aligned"); return RT_ERR_INVALID_ARGUMENT; }
    rt_status st = check_traversal(s, trav);
    if (st != RT_OK) return st;
    const unsigned bpp = format == RT_FRAME_RGBA ? 4u : format == RT_FRAME_RGB ? 3u : 1u;
    const size_t frame_bytes = (size_t)o->width * o->height * bpp;
    const bool flat2 = trav == RT_TRAVERSAL_FLAT;
    // Batches: at most kStreamMaxBatches, each at least a million samples (a 1080p frame at one sample per pixel: two batches -- progress
    // reports matter for renders that take long, and a short batch leaves most of the chip idle), and -- where the list is the scheduler's
    // row-major grid (render.rs:273-298) -- whole bucket ROWS, so that what a batch delivers is complete rows of the image.
    constexpr uint32_t kStreamMaxBatches = 16;
    const uint64_t ns = (uint64_t)o->samples_per_pixel * o->samples_per_pixel;
    uint32_t per = std::max<uint32_t>((n + kStreamMaxBatches - 1) / kStreamMaxBatches, (uint32_t)std::clamp<uint64_t>((1ull << 20) / (4096ull * std::max<uint64_t>(ns, 1)), 16, 256));
    {
        uint32_t row = 1;
        while (row < n && tiles[row].b == tiles[0].b) ++row;
        bool grid = n % row == 0;
        for (uint32_t i = 0; grid && i < n; ++i) grid = tiles[i].b == tiles[i - i % row].b && tiles[i].t == tiles[i - i % row].t && tiles[i].l == tiles[i % row].l && tiles[i].r == tiles[i % row].r;
        if (grid) per = (per + row - 1) / row * row;
    }
    const uint32_t n_batches = (n + per - 1) / per;
    struct Batch { std::vector<rt::TileDev> tab, tab16; uint64_t px = 0; uint32_t blocks = 0, blocks16 = 0; size_t byte_off = 0; };
    std::vector<Batch> batches(n_batches);
    size_t total_bytes = 0;
    for (uint32_t k = 0; k < n_batches; ++k) {
        Batch &b = batches[k];
        const uint32_t first = k * per, cnt = std::min(per, n - first);
        if ((st = build_tile_table(o, tiles + first, cnt, b.tab, &b.px, &b.blocks, flat2 ? rt::kFlatBlockW : rt::kBlockW, flat2 ? rt::kFlatBlockH : rt::kBlockH)) != RT_OK) return st;
        if (flat2) { uint64_t px16 = 0; if ((st = build_tile_table(o, tiles + first, cnt, b.tab16, &px16, &b.blocks16)) != RT_OK) return st; }
        b.byte_off = total_bytes;
        total_bytes += (size_t)b.px * 4;
    }
    HIP_TRY(hipSetDevice(s->device));
    const HostDest dest = classify_host_pointer(frame_out);
    if (dest.bad) { snprintf(g_err, sizeof g_err, "rt_render_frame_stream: frame_out is device memory"); return RT_ERR_INVALID_ARGUMENT; }
    const bool direct = dest.pinned && dest.dev_alias && dest.room >= frame_bytes;
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    if (c->out_cap < total_bytes) {
        if (c->d_out) HIP_TRY(hipFree(c->d_out));
        c->d_out = nullptr; c->out_cap = 0;
        HIP_TRY(hipMalloc(&c->d_out, total_bytes));
        c->out_cap = total_bytes;
    }
    uint8_t *target = dest.dev_alias;
    if (!direct) {
        if (c->h_out_cap < frame_bytes) {
            if (c->h_out) HIP_TRY(hipHostFree(c->h_out));
            c->h_out = nullptr; c->h_out_cap = 0;
            HIP_TRY(hipHostMalloc(&c->h_out, std::max(frame_bytes, (size_t)1 << 20), hipHostMallocDefault));
            c->h_out_cap = std::max(frame_bytes, (size_t)1 << 20);
        }
        void *alias = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&alias, c->h_out, 0));
        target = static_cast<uint8_t *>(alias);
    }
    while (c->chunk_ev.size() < n_batches) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->chunk_ev.push_back(e);
    }
    // several batches: a batch is encoded (PCIe-bound, a handful of waves) on a second stream while the next one renders
    hipStream_t enc = c->stream;
    if (n_batches >= 4) {                                            // (a stream is a hardware queue: 5 - 9 ms to create, once per context)
        if (!c->stream2 && hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); c->stream2 = nullptr; }
        if (c->stream2) enc = c->stream2;
    }
    auto drain = [&](rt_status code) { (void)hipStreamSynchronize(c->stream); if (c->stream2) (void)hipStreamSynchronize(c->stream2); (void)hipGetLastError(); return code; };   // nothing may still be writing the frame
    for (uint32_t k = 0; k < n_batches; ++k) {
        Batch &b = batches[k];
        // the encode reads the very table the batch was rendered with (looking it up again could upload it a second time, unordered with
        // the encode: ADVICE r5); a table that is NOT the scene's immutable cached copy -- the cache is full, it went through the context's
        // one upload slot -- is only safe in stream order, so such a batch is encoded on the render stream
        const rt::TileDev *d_tab = nullptr;
        st = enqueue_pass(s, c, o, trav, b.tab, b.blocks, b.px, c->d_out + b.byte_off, 0u, c->stream, false, flat2 ? &b.tab16 : nullptr, b.blocks16, true, &d_tab);
        if (st != RT_OK) return drain(st);
        if (c->tiles_live[0]) enc = c->stream;
        if (enc != c->stream) {                                      // (enqueue_pass recorded ev1 behind the batch's kernels)
            const hipError_t we = hipStreamWaitEvent(enc, c->ev1, 0);
            if (we != hipSuccess) return drain(hip_fail(we, "rt_render_frame_stream(wait)", __LINE__));
        }
        const unsigned *src = reinterpret_cast<const unsigned *>(c->d_out + b.byte_off);
        const dim3 grid((unsigned)b.tab.size()), blk(rt::kBlockThreads);
        if (bpp == 4) hipLaunchKernelGGL((rt::k_encode_tiles<4>), grid, blk, 0, enc, (unsigned)o->width, d_tab, (unsigned)b.tab.size(), src, target);
        else if (bpp == 3) hipLaunchKernelGGL((rt::k_encode_tiles<3>), grid, blk, 0, enc, (unsigned)o->width, d_tab, (unsigned)b.tab.size(), src, target);
        else hipLaunchKernelGGL((rt::k_encode_tiles<1>), grid, blk, 0, enc, (unsigned)o->width, d_tab, (unsigned)b.tab.size(), src, target);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(c->chunk_ev[k], enc);
        if (e != hipSuccess) return drain(hip_fail(e, "rt_render_frame_stream(encode)", __LINE__));
    }
    for (uint32_t k = 0; k < n_batches; ++k) {
        hipError_t e = hipEventSynchronize(c->chunk_ev[k]);
        if (e != hipSuccess) return drain(hip_fail(e, "hipEventSynchronize(stream batch)", __LINE__));
        const uint32_t first = k * per, cnt = std::min(per, n - first);
        if (!direct)
            for (uint32_t i = first; i < first + cnt; ++i) {
                const size_t seg = (size_t)(tiles[i].r - tiles[i].l) * bpp;
                for (unsigned y = tiles[i].b; y < tiles[i].t; ++y) {
                    const size_t off = ((size_t)y * o->width + tiles[i].l) * bpp;
                    memcpy(frame_out + off, c->h_out + off, seg);
                }
            }
        if (callback) callback(user, first, cnt);
    }
    // (the last batch's event is behind everything on both streams: the context goes back idle)
    return RT_OK;
}

// ---- ray queries: TypedGroup::intersect(&mut hit, &ray) for a batch of arbitrary rays (rt_query.hpp) ----

// The ordered entries (rt_order.hpp) share the bodies of the entries they extend.  `ordered` with order == NULL: the call
// computes the order itself in its context's workspace, then walks; a device order is checked for alignment only.
static bool device_order_ok(const uint32_t *order, const char *what)
{
    if ((reinterpret_cast<uintptr_t>(order) & 3u) != 0) { snprintf(g_err, sizeof g_err, "%s: order must be 4-byte aligned", what); return false; }
    return true;
}

// What a device entry does when a step failed after the call's own order was enqueued: the context, whose workspace the sort uses, goes
// back behind what is enqueued.  (With nothing enqueued through the context a failure returns plainly, as the unordered entries always did.)
static rt_status behind_enqueued(Context *c, Lease &lease, hipStream_t stream, rt_status st)
{
    (void)hipEventRecord(c->ev1, stream);
    (void)hipGetLastError();
    lease.inflight = true;
    return st;
}

static rt_status intersect_rays_device(rt_scene *s, rt_query mode, const void *rays, const void *tmax, uint32_t n, void *distance_out, void *normal_out,
                                       int32_t *item_out, bool ordered, const uint32_t *order, void *hip_stream, rt_stats *stats, const char *what)
{
    if (!query_args_ok(s, mode, rays, tmax, n, distance_out, normal_out, item_out, what)) return RT_ERR_INVALID_ARGUMENT;
    if (ordered && !device_order_ok(order, what)) return RT_ERR_INVALID_ARGUMENT;
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const void *nodes = nullptr;
    uint32_t n_nodes = 0;
    rt_status st = query_stream(s, stream, &nodes, &n_nodes);
    if (st != RT_OK) return st;
    const bool sort = ordered && !order;
    if (!stats && !sort) return enqueue_query(s, nodes, n_nodes, mode, rays, tmax, n, distance_out, normal_out, item_out, nullptr, stream, order);
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    if (sort && (st = enqueue_ray_order(s, c, rays, n, nullptr, stream, &order)) != RT_OK) return behind_enqueued(c, lease, stream, st);
    if (stats) {
        if (hipError_t e = hipMemsetAsync(c->d_counters, 0, sizeof(rt::Counters) * rt::kCounterStripes, stream); e != hipSuccess)
            return sort ? behind_enqueued(c, lease, stream, hip_fail(e, "hipMemsetAsync(counters)", __LINE__)) : hip_fail(e, "hipMemsetAsync(counters)", __LINE__);
        if (hipError_t e = hipEventRecord(c->ev0, stream); e != hipSuccess)
            return sort ? behind_enqueued(c, lease, stream, hip_fail(e, "hipEventRecord", __LINE__)) : hip_fail(e, "hipEventRecord", __LINE__);
    }
    st = enqueue_query(s, nodes, n_nodes, mode, rays, tmax, n, distance_out, normal_out, item_out, stats ? c->d_counters : nullptr, stream, order);
    (void)hipEventRecord(c->ev1, stream);
    if (st != RT_OK) { (void)hipGetLastError(); lease.inflight = true; return st; }      // (the context goes back behind what is enqueued)
    if (stats) return read_query_stats(c, stream, stats);
    lease.inflight = true;                              // the order in the workspace is in use until ev1: asynchronous return
    return RT_OK;
}

rt_status rt_intersect_rays_device(rt_scene *s, rt_query mode, const void *rays, const void *tmax, uint32_t n, void *distance_out, void *normal_out,
                                   int32_t *item_out, void *hip_stream, rt_stats *stats)
{
    return intersect_rays_device(s, mode, rays, tmax, n, distance_out, normal_out, item_out, false, nullptr, hip_stream, stats, "rt_intersect_rays_device");
}

rt_status rt_intersect_rays_ordered_device(rt_scene *s, rt_query mode, const void *rays, const void *tmax, uint32_t n, const uint32_t *order,
                                           void *distance_out, void *normal_out, int32_t *item_out, void *hip_stream, rt_stats *stats)
{
    return intersect_rays_device(s, mode, rays, tmax, n, distance_out, normal_out, item_out, true, order, hip_stream, stats, "rt_intersect_rays_ordered_device");
}

static rt_status intersect_rays_host(rt_scene *s, rt_query mode, const void *rays, const void *tmax, uint32_t n, void *distance_out, void *normal_out,
                                     int32_t *item_out, bool ordered, const uint32_t *order, rt_stats *stats, const char *what)
{
    if (!query_args_ok(s, mode, rays, tmax, n, distance_out, normal_out, item_out, what)) return RT_ERR_INVALID_ARGUMENT;
    if (ordered && !device_order_ok(order, what)) return RT_ERR_INVALID_ARGUMENT;
    const size_t esz = real_size(s);
    HostStaging::Row rows[] = { { rays, 6 * esz * n, kStageIn }, { tmax, esz * n, kStageIn }, { distance_out, esz * n, kStageOut },
                                { normal_out, 3 * esz * n, kStageOut }, { item_out, sizeof(int32_t) * n, kStageOut }, { order, sizeof(uint32_t) * n, kStageIn } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what); pst != RT_OK) return pst;
    if (!query_rays_valid(s, rays, tmax, n)) return RT_ERR_INVALID_ARGUMENT;
    if (order && !order_is_permutation(order, n, what)) return RT_ERR_INVALID_ARGUMENT;
    const uint32_t *d_order = nullptr;
    return host_query(s, hs, stats, read_query_stats,
                      [&](Context *c) { d_order = hs.dev<const uint32_t>(5); return ordered && !order ? enqueue_ray_order(s, c, hs.dev(0), n, nullptr, c->stream, &d_order) : RT_OK; },
                      [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
                          return enqueue_query(s, nodes, n_nodes, mode, hs.dev(0), hs.dev(1), n, hs.dev(2), hs.dev(3), hs.dev<int32_t>(4), counters, stream, d_order);
                      });
}

rt_status rt_intersect_rays(rt_scene *s, rt_query mode, const void *rays, const void *tmax, uint32_t n, void *distance_out, void *normal_out,
                            int32_t *item_out, rt_stats *stats)
{
    return intersect_rays_host(s, mode, rays, tmax, n, distance_out, normal_out, item_out, false, nullptr, stats, "rt_intersect_rays");
}

rt_status rt_intersect_rays_ordered(rt_scene *s, rt_query mode, const void *rays, const void *tmax, uint32_t n, const uint32_t *order,
                                    void *distance_out, void *normal_out, int32_t *item_out, rt_stats *stats)
{
    return intersect_rays_host(s, mode, rays, tmax, n, distance_out, normal_out, item_out, true, order, stats, "rt_intersect_rays_ordered");
}

// ---- multi-hit ray queries: the k closest hits, or every hit below tmax, for a batch of arbitrary rays (rt_multihit.hpp) ----

static rt_status intersect_rays_multi_device(rt_scene *s, rt_multihit mode, uint32_t k, const void *rays, const void *tmax, uint32_t n, void *distance_out,
                                             void *normal_out, int32_t *item_out, uint32_t *hits_out, bool ordered, const uint32_t *order,
                                             void *hip_stream, rt_stats *stats, const char *what)
{
    if (!query_args_ok(s, RT_QUERY_NEAREST, rays, tmax, n, distance_out, normal_out, item_out, what) || !multihit_args_ok(mode, k, hits_out, what))
        return RT_ERR_INVALID_ARGUMENT;
    if (ordered && !device_order_ok(order, what)) return RT_ERR_INVALID_ARGUMENT;
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const void *nodes = nullptr;
    uint32_t n_nodes = 0;
    rt_status st = query_stream(s, stream, &nodes, &n_nodes);
    if (st != RT_OK) return st;
    const bool sort = ordered && !order;
    if (!stats && !sort)
        return enqueue_multihit(s, nodes, n_nodes, mode, k, rays, tmax, n, distance_out, normal_out, item_out, hits_out, nullptr, stream, order);
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    if (sort && (st = enqueue_ray_order(s, c, rays, n, nullptr, stream, &order)) != RT_OK) return behind_enqueued(c, lease, stream, st);
    if (stats) {
        if (hipError_t e = hipMemsetAsync(c->d_counters, 0, sizeof(rt::Counters) * rt::kCounterStripes, stream); e != hipSuccess)
            return sort ? behind_enqueued(c, lease, stream, hip_fail(e, "hipMemsetAsync(counters)", __LINE__)) : hip_fail(e, "hipMemsetAsync(counters)", __LINE__);
        if (hipError_t e = hipEventRecord(c->ev0, stream); e != hipSuccess)
            return sort ? behind_enqueued(c, lease, stream, hip_fail(e, "hipEventRecord", __LINE__)) : hip_fail(e, "hipEventRecord", __LINE__);
    }
    st = enqueue_multihit(s, nodes, n_nodes, mode, k, rays, tmax, n, distance_out, normal_out, item_out, hits_out, stats ? c->d_counters : nullptr, stream,
                          order);
    (void)hipEventRecord(c->ev1, stream);
    if (st != RT_OK) { (void)hipGetLastError(); lease.inflight = true; return st; }      // (the context goes back behind what is enqueued)
    if (stats) return read_query_stats(c, stream, stats);
    lease.inflight = true;                              // the order in the workspace is in use until ev1: asynchronous return
    return RT_OK;
}

rt_status rt_intersect_rays_multi_device(rt_scene *s, rt_multihit mode, uint32_t k, const void *rays, const void *tmax, uint32_t n, void *distance_out,
                                         void *normal_out, int32_t *item_out, uint32_t *hits_out, void *hip_stream, rt_stats *stats)
{
    return intersect_rays_multi_device(s, mode, k, rays, tmax, n, distance_out, normal_out, item_out, hits_out, false, nullptr, hip_stream, stats,
                                       "rt_intersect_rays_multi_device");
}

rt_status rt_intersect_rays_multi_ordered_device(rt_scene *s, rt_multihit mode, uint32_t k, const void *rays, const void *tmax, uint32_t n,
                                                 const uint32_t *order, void *distance_out, void *normal_out, int32_t *item_out, uint32_t *hits_out,
                                                 void *hip_stream, rt_stats *stats)
{
    return intersect_rays_multi_device(s, mode, k, rays, tmax, n, distance_out, normal_out, item_out, hits_out, true, order, hip_stream, stats,
                                       "rt_intersect_rays_multi_ordered_device");
}

static rt_status intersect_rays_multi_host(rt_scene *s, rt_multihit mode, uint32_t k, const void *rays, const void *tmax, uint32_t n, void *distance_out,
                                           void *normal_out, int32_t *item_out, uint32_t *hits_out, bool ordered, const uint32_t *order, rt_stats *stats,
                                           const char *what)
{
    if (!query_args_ok(s, RT_QUERY_NEAREST, rays, tmax, n, distance_out, normal_out, item_out, what) || !multihit_args_ok(mode, k, hits_out, what))
        return RT_ERR_INVALID_ARGUMENT;
    if (ordered && !device_order_ok(order, what)) return RT_ERR_INVALID_ARGUMENT;
    const size_t esz = real_size(s), nk = (size_t)n * k;
    HostStaging::Row rows[] = { { rays, 6 * esz * n, kStageIn }, { tmax, esz * n, kStageIn }, { distance_out, esz * nk, kStageOut }, { normal_out, 3 * esz * nk, kStageOut },
                                { item_out, sizeof(int32_t) * nk, kStageOut }, { hits_out, sizeof(uint32_t) * n, kStageOut }, { order, sizeof(uint32_t) * n, kStageIn } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what); pst != RT_OK) return pst;
    if (!query_rays_valid(s, rays, tmax, n)) return RT_ERR_INVALID_ARGUMENT;
    if (order && !order_is_permutation(order, n, what)) return RT_ERR_INVALID_ARGUMENT;
    const uint32_t *d_order = nullptr;
    return host_query(s, hs, stats, read_query_stats,
                      [&](Context *c) { d_order = hs.dev<const uint32_t>(6); return ordered && !order ? enqueue_ray_order(s, c, hs.dev(0), n, nullptr, c->stream, &d_order) : RT_OK; },
                      [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
                          return enqueue_multihit(s, nodes, n_nodes, mode, k, hs.dev(0), hs.dev(1), n, hs.dev(2), hs.dev(3), hs.dev<int32_t>(4), hs.dev<uint32_t>(5), counters,
                                                  stream, d_order);
                      });
}

rt_status rt_intersect_rays_multi(rt_scene *s, rt_multihit mode, uint32_t k, const void *rays, const void *tmax, uint32_t n, void *distance_out,
                                  void *normal_out, int32_t *item_out, uint32_t *hits_out, rt_stats *stats)
{
    return intersect_rays_multi_host(s, mode, k, rays, tmax, n, distance_out, normal_out, item_out, hits_out, false, nullptr, stats, "rt_intersect_rays_multi");
}

rt_status rt_intersect_rays_multi_ordered(rt_scene *s, rt_multihit mode, uint32_t k, const void *rays, const void *tmax, uint32_t n, const uint32_t *order,
                                          void *distance_out, void *normal_out, int32_t *item_out, uint32_t *hits_out, rt_stats *stats)
{
    return intersect_rays_multi_host(s, mode, k, rays, tmax, n, distance_out, normal_out, item_out, hits_out, true, order, stats,
                                     "rt_intersect_rays_multi_ordered");
}

// ---- proximity queries: the k nearest spheres of every point, or every sphere within a radius (rt_near.hpp) ----

rt_status rt_near_spheres_device(rt_scene *s, rt_near mode, uint32_t k, const void *points, const void *radius, uint32_t n, const int32_t *exclude,
                                 const uint32_t *order, void *gap_out, int32_t *item_out, uint32_t *found_out, rt_stats *stats, void *hip_stream)
{
    const char *const what = "rt_near_spheres_device";
    if (!near_args_ok(s, mode, k, points, radius, n, exclude, order, gap_out, item_out, found_out, what)) return RT_ERR_INVALID_ARGUMENT;
    return device_query(s, stats, static_cast<hipStream_t>(hip_stream), [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
        return enqueue_near(s, nodes, n_nodes, mode, k, points, radius, n, exclude, order, gap_out, item_out, found_out, counters, stream);
    });
}

rt_status rt_near_spheres(rt_scene *s, rt_near mode, uint32_t k, const void *points, const void *radius, uint32_t n, const int32_t *exclude,
                          const uint32_t *order, void *gap_out, int32_t *item_out, uint32_t *found_out, rt_stats *stats)
{
    const char *const what = "rt_near_spheres";
    if (!near_args_ok(s, mode, k, points, radius, n, exclude, order, gap_out, item_out, found_out, what)) return RT_ERR_INVALID_ARGUMENT;
    const size_t esz = real_size(s), nk = (size_t)n * k;
    HostStaging::Row rows[] = { { points, 3 * esz * n, kStageIn }, { radius, esz * n, kStageIn }, { exclude, sizeof(int32_t) * n, kStageIn }, { order, sizeof(uint32_t) * n, kStageIn },
                                { gap_out, esz * nk, kStageOut }, { item_out, sizeof(int32_t) * nk, kStageOut }, { found_out, sizeof(uint32_t) * n, kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what); pst != RT_OK) return pst;
    if (!near_points_valid(s, points, radius, n, what)) return RT_ERR_INVALID_ARGUMENT;
    if (order && !order_is_permutation(order, n, what)) return RT_ERR_INVALID_ARGUMENT;
    return host_query(s, hs, stats, read_query_stats, no_pre_step, [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
        return enqueue_near(s, nodes, n_nodes, mode, k, hs.dev(0), hs.dev(1), n, hs.dev<const int32_t>(2), hs.dev<const uint32_t>(3), hs.dev(4), hs.dev<int32_t>(5),
                            hs.dev<uint32_t>(6), counters, stream);
    });
}

// ---- sphere casts: the first contact of a moving sphere with the scene (rt_sweep.hpp) ----

rt_status rt_sweep_spheres_device(rt_scene *s, rt_sweep mode, const void *rays, const void *radius, const void *tmax, uint32_t n, const int32_t *exclude,
                                  const uint32_t *order, void *distance_out, void *normal_out, int32_t *item_out, rt_stats *stats, void *hip_stream)
{
    const char *const what = "rt_sweep_spheres_device";
    if (!sweep_args_ok(s, mode, rays, radius, tmax, n, exclude, order, distance_out, normal_out, item_out, what)) return RT_ERR_INVALID_ARGUMENT;
    return device_query(s, stats, static_cast<hipStream_t>(hip_stream), [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
        return enqueue_sweep(s, nodes, n_nodes, mode, rays, radius, tmax, n, exclude, order, distance_out, normal_out, item_out, counters, stream);
    });
}

rt_status rt_sweep_spheres(rt_scene *s, rt_sweep mode, const void *rays, const void *radius, const void *tmax, uint32_t n, const int32_t *exclude,
                           const uint32_t *order, void *distance_out, void *normal_out, int32_t *item_out, rt_stats *stats)
{
    const char *const what = "rt_sweep_spheres";
    if (!sweep_args_ok(s, mode, rays, radius, tmax, n, exclude, order, distance_out, normal_out, item_out, what)) return RT_ERR_INVALID_ARGUMENT;
    const size_t esz = real_size(s);
    HostStaging::Row rows[] = { { rays, 6 * esz * n, kStageIn }, { radius, esz * n, kStageIn }, { tmax, esz * n, kStageIn }, { exclude, sizeof(int32_t) * n, kStageIn },
                                { order, sizeof(uint32_t) * n, kStageIn }, { distance_out, esz * n, kStageOut }, { normal_out, 3 * esz * n, kStageOut },
                                { item_out, sizeof(int32_t) * n, kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what); pst != RT_OK) return pst;
    if (!sweep_casts_valid(s, rays, radius, tmax, n, what)) return RT_ERR_INVALID_ARGUMENT;
    if (order && !order_is_permutation(order, n, what)) return RT_ERR_INVALID_ARGUMENT;
    return host_query(s, hs, stats, read_query_stats, no_pre_step, [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
        return enqueue_sweep(s, nodes, n_nodes, mode, hs.dev(0), hs.dev(1), hs.dev(2), n, hs.dev<const int32_t>(3), hs.dev<const uint32_t>(4), hs.dev(5), hs.dev(6),
                             hs.dev<int32_t>(7), counters, stream);
    });
}

// ---- contact pairs: every pair of spheres of the scene closer than a margin (rt_contacts.hpp) ----

rt_status rt_scene_contacts_device(rt_scene *s, double margin, uint32_t capacity, int32_t *pairs_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out,
                                   rt_stats *stats, void *hip_stream)
{
    const char *const what = "rt_scene_contacts_device";
    if (!contacts_args_ok(s, margin, capacity, pairs_out, gap_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    return device_list_query(
        s, s->contacts, capacity != 0u && pairs_out, stats, static_cast<hipStream_t>(hip_stream),
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) { return contacts_begin(s, nodes, n_nodes, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_contacts_count(s, nodes, n_nodes, margin, offsets_out, total_out, counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) { return enqueue_contacts_fill(s, nodes, n_nodes, margin, capacity, pairs_out, gap_out, stream); });
}

rt_status rt_scene_contacts(rt_scene *s, double margin, uint32_t capacity, int32_t *pairs_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out,
                            rt_stats *stats)
{
    const char *const what = "rt_scene_contacts";
    if (!contacts_args_ok(s, margin, capacity, pairs_out, gap_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    const bool fill = capacity != 0u && pairs_out;
    const size_t esz = real_size(s);
    HostStaging::Row rows[] = { { fill ? pairs_out : nullptr, 2 * sizeof(int32_t) * (size_t)capacity, kStageOut, 2 * sizeof(int32_t) },
                                { fill ? gap_out : nullptr, esz * (size_t)capacity, kStageOut, esz },
                                { offsets_out, sizeof(uint64_t) * ((size_t)s->n_items + 1), kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what, total_out); pst != RT_OK) return pst;
    return host_list_query(
        s, s->contacts, hs, capacity, fill, total_out, stats,
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) { return contacts_begin(s, nodes, n_nodes, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_contacts_count(s, nodes, n_nodes, margin, hs.dev<uint64_t>(2), s->contacts.d_total, counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) {
            return enqueue_contacts_fill(s, nodes, n_nodes, margin, capacity, hs.dev<int32_t>(0), hs.dev(1), stream);
        });
}

// ---- impact pairs: every pair of spheres of the scene that comes into contact during one step, and when (rt_impacts.hpp) ----

rt_status rt_scene_impacts_device(rt_scene *s, const void *disp, uint32_t capacity, int32_t *pairs_out, void *time_out, uint64_t *offsets_out, uint64_t *total_out,
                                  rt_stats *stats, void *hip_stream)
{
    const char *const what = "rt_scene_impacts_device";
    if (!impacts_args_ok(s, disp, capacity, pairs_out, time_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    // impacts calls take their turn with contacts calls: they share the counts and the offsets
    return device_list_query(
        s, s->contacts, capacity != 0u && pairs_out, stats, static_cast<hipStream_t>(hip_stream),
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) { return impacts_begin(s, nodes, n_nodes, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_impacts_count(s, nodes, n_nodes, disp, offsets_out, total_out, counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) { return enqueue_impacts_fill(s, nodes, n_nodes, capacity, pairs_out, time_out, stream); });
}

rt_status rt_scene_impacts(rt_scene *s, const void *disp, uint32_t capacity, int32_t *pairs_out, void *time_out, uint64_t *offsets_out, uint64_t *total_out,
                           rt_stats *stats)
{
    const char *const what = "rt_scene_impacts";
    if (!impacts_args_ok(s, disp, capacity, pairs_out, time_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    const bool fill = capacity != 0u && pairs_out;
    const size_t esz = real_size(s);
    HostStaging::Row rows[] = { { disp, 3 * esz * (size_t)s->n_items, kStageIn },
                                { fill ? pairs_out : nullptr, 2 * sizeof(int32_t) * (size_t)capacity, kStageOut, 2 * sizeof(int32_t) },
                                { fill ? time_out : nullptr, esz * (size_t)capacity, kStageOut, esz },
                                { offsets_out, sizeof(uint64_t) * ((size_t)s->n_items + 1), kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what, total_out); pst != RT_OK) return pst;
    if (!impacts_disp_valid(s, disp, s->n_items, what)) return RT_ERR_INVALID_ARGUMENT;
    // (the contacts workspace: host calls on one scene take turns, contacts and impacts alike)
    return host_list_query(
        s, s->contacts, hs, capacity, fill, total_out, stats,
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) { return impacts_begin(s, nodes, n_nodes, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_impacts_count(s, nodes, n_nodes, hs.dev(0), hs.dev<uint64_t>(3), s->contacts.d_total, counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) {
            return enqueue_impacts_fill(s, nodes, n_nodes, capacity, hs.dev<int32_t>(1), hs.dev(2), stream);
        });
}

// ---- contact islands: the connected groups of the contacts, or of the impacts of one step (rt_islands.hpp) ----

// Both device entries: everything on the caller's stream, in the contacts workspace's turn; nothing is waited for unless stats is given.
static rt_status islands_device(rt_scene *s, bool moving, double margin, const void *disp, int32_t *label_out, int32_t *index_out, uint32_t *size_out,
                                uint64_t *n_islands_out, rt_stats *stats, void *hip_stream, const char *what)
{
    if (!islands_args_ok(s, moving, margin, disp, label_out, index_out, size_out, n_islands_out, what)) return RT_ERR_INVALID_ARGUMENT;
    return device_list_query(
        s, s->contacts, false, stats, static_cast<hipStream_t>(hip_stream),
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) { return islands_begin(s, moving, nodes, n_nodes, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_islands(s, nodes, n_nodes, moving, margin, disp, label_out, index_out, size_out, n_islands_out, counters, stream);
        },
        [](const void *, uint32_t, hipStream_t) { return RT_OK; });      // (one pass: there is no list to fill)
}

// Both host entries: the list skeleton with nothing to fill -- the scan's total, read through the workspace's pinned word, is n_islands.
static rt_status islands_host(rt_scene *s, bool moving, double margin, const void *disp, int32_t *label_out, int32_t *index_out, uint32_t *size_out,
                              uint64_t *n_islands_out, rt_stats *stats, const char *what)
{
    if (!islands_args_ok(s, moving, margin, disp, label_out, index_out, size_out, n_islands_out, what)) return RT_ERR_INVALID_ARGUMENT;
    const size_t esz = real_size(s), n = s->n_items;
    HostStaging::Row rows[] = { { disp, 3 * esz * n, kStageIn }, { label_out, sizeof(int32_t) * n, kStageOut }, { index_out, sizeof(int32_t) * n, kStageOut },
                                { size_out, sizeof(uint32_t) * n, kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what, n_islands_out); pst != RT_OK) return pst;
    if (moving && !impacts_disp_valid(s, disp, s->n_items, what)) return RT_ERR_INVALID_ARGUMENT;
    uint64_t n_islands = 0;
    return host_list_query(
        s, s->contacts, hs, 0u, false, n_islands_out ? n_islands_out : &n_islands, stats,
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) { return islands_begin(s, moving, nodes, n_nodes, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_islands(s, nodes, n_nodes, moving, margin, hs.dev(0), hs.dev<int32_t>(1), hs.dev<int32_t>(2), hs.dev<uint32_t>(3), s->contacts.d_total, counters,
                                   stream);
        },
        [](const void *, uint32_t, hipStream_t) { return RT_OK; });
}

rt_status rt_scene_islands_device(rt_scene *s, double margin, int32_t *label_out, int32_t *index_out, uint32_t *size_out, uint64_t *n_islands_out, rt_stats *stats,
                                  void *hip_stream)
{
    return islands_device(s, false, margin, nullptr, label_out, index_out, size_out, n_islands_out, stats, hip_stream, "rt_scene_islands_device");
}

rt_status rt_scene_islands(rt_scene *s, double margin, int32_t *label_out, int32_t *index_out, uint32_t *size_out, uint64_t *n_islands_out, rt_stats *stats)
{
    return islands_host(s, false, margin, nullptr, label_out, index_out, size_out, n_islands_out, stats, "rt_scene_islands");
}

rt_status rt_scene_impact_islands_device(rt_scene *s, const void *disp, int32_t *label_out, int32_t *index_out, uint32_t *size_out, uint64_t *n_islands_out,
                                         rt_stats *stats, void *hip_stream)
{
    return islands_device(s, true, 0.0, disp, label_out, index_out, size_out, n_islands_out, stats, hip_stream, "rt_scene_impact_islands_device");
}

rt_status rt_scene_impact_islands(rt_scene *s, const void *disp, int32_t *label_out, int32_t *index_out, uint32_t *size_out, uint64_t *n_islands_out, rt_stats *stats)
{
    return islands_host(s, true, 0.0, disp, label_out, index_out, size_out, n_islands_out, stats, "rt_scene_impact_islands");
}

// ---- overlap lists: every sphere of the scene within a margin of each query sphere (rt_overlap.hpp) ----

rt_status rt_overlap_spheres_device(rt_scene *s, const void *queries, uint32_t n, double margin, const int32_t *exclude, const uint32_t *order, uint32_t capacity,
                                    int32_t *items_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats, void *hip_stream)
{
    const char *const what = "rt_overlap_spheres_device";
    if (!overlap_args_ok(s, queries, n, margin, exclude, order, capacity, items_out, gap_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    return device_list_query(
        s, s->overlap, capacity != 0u && items_out, stats, static_cast<hipStream_t>(hip_stream),
        [&](const void *, uint32_t, hipStream_t stream) { return overlap_begin(s, n, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_overlap_count(s, nodes, n_nodes, queries, n, margin, exclude, order, offsets_out, total_out, counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) {
            return enqueue_overlap_fill(s, nodes, n_nodes, queries, n, margin, exclude, order, capacity, items_out, gap_out, stream);
        });
}

rt_status rt_overlap_spheres(rt_scene *s, const void *queries, uint32_t n, double margin, const int32_t *exclude, const uint32_t *order, uint32_t capacity,
                             int32_t *items_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats)
{
    const char *const what = "rt_overlap_spheres";
    if (!overlap_args_ok(s, queries, n, margin, exclude, order, capacity, items_out, gap_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    const bool fill = capacity != 0u && items_out;
    const size_t esz = real_size(s);
    HostStaging::Row rows[] = { { queries, 4 * esz * (size_t)n, kStageIn }, { exclude, sizeof(int32_t) * (size_t)n, kStageIn }, { order, sizeof(uint32_t) * (size_t)n, kStageIn },
                                { fill ? items_out : nullptr, sizeof(int32_t) * (size_t)capacity, kStageOut, sizeof(int32_t) },
                                { fill ? gap_out : nullptr, esz * (size_t)capacity, kStageOut, esz },
                                { offsets_out, sizeof(uint64_t) * ((size_t)n + 1), kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what, total_out); pst != RT_OK) return pst;
    if (!overlap_queries_valid(s, queries, n, what)) return RT_ERR_INVALID_ARGUMENT;
    if (order && !order_is_permutation(order, n, what)) return RT_ERR_INVALID_ARGUMENT;
    return host_list_query(
        s, s->overlap, hs, capacity, fill, total_out, stats,
        [&](const void *, uint32_t, hipStream_t stream) { return overlap_begin(s, n, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_overlap_count(s, nodes, n_nodes, hs.dev(0), n, margin, hs.dev<const int32_t>(1), hs.dev<const uint32_t>(2), hs.dev<uint64_t>(5), s->overlap.d_total,
                                         counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) {
            return enqueue_overlap_fill(s, nodes, n_nodes, hs.dev(0), n, margin, hs.dev<const int32_t>(1), hs.dev<const uint32_t>(2), capacity, hs.dev<int32_t>(3), hs.dev(4), stream);
        });
}

// ---- box overlap lists: every sphere of the scene within a margin of each axis-aligned query box (rt_box.hpp) ----

rt_status rt_overlap_boxes_device(rt_scene *s, const void *boxes, uint32_t n, double margin, const int32_t *exclude, const uint32_t *order, uint32_t capacity,
                                  int32_t *items_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats, void *hip_stream)
{
    const char *const what = "rt_overlap_boxes_device";
    if (!boxes_args_ok(s, boxes, n, margin, exclude, order, capacity, items_out, gap_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    // box calls take their turn with overlap, swept and first-contact calls: they share the counts and the offsets
    return device_list_query(
        s, s->overlap, capacity != 0u && items_out, stats, static_cast<hipStream_t>(hip_stream),
        [&](const void *, uint32_t, hipStream_t stream) { return overlap_begin(s, n, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_boxes_count(s, nodes, n_nodes, boxes, n, margin, exclude, order, offsets_out, total_out, counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) {
            return enqueue_boxes_fill(s, nodes, n_nodes, boxes, n, margin, exclude, order, capacity, items_out, gap_out, stream);
        });
}

rt_status rt_overlap_boxes(rt_scene *s, const void *boxes, uint32_t n, double margin, const int32_t *exclude, const uint32_t *order, uint32_t capacity,
                           int32_t *items_out, void *gap_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats)
{
    const char *const what = "rt_overlap_boxes";
    if (!boxes_args_ok(s, boxes, n, margin, exclude, order, capacity, items_out, gap_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    const bool fill = capacity != 0u && items_out;
    const size_t esz = real_size(s);
    HostStaging::Row rows[] = { { boxes, 6 * esz * (size_t)n, kStageIn }, { exclude, sizeof(int32_t) * (size_t)n, kStageIn }, { order, sizeof(uint32_t) * (size_t)n, kStageIn },
                                { fill ? items_out : nullptr, sizeof(int32_t) * (size_t)capacity, kStageOut, sizeof(int32_t) },
                                { fill ? gap_out : nullptr, esz * (size_t)capacity, kStageOut, esz },
                                { offsets_out, sizeof(uint64_t) * ((size_t)n + 1), kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what, total_out); pst != RT_OK) return pst;
    if (!boxes_valid(s, boxes, n, what)) return RT_ERR_INVALID_ARGUMENT;
    if (order && !order_is_permutation(order, n, what)) return RT_ERR_INVALID_ARGUMENT;
    return host_list_query(
        s, s->overlap, hs, capacity, fill, total_out, stats,
        [&](const void *, uint32_t, hipStream_t stream) { return overlap_begin(s, n, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_boxes_count(s, nodes, n_nodes, hs.dev(0), n, margin, hs.dev<const int32_t>(1), hs.dev<const uint32_t>(2), hs.dev<uint64_t>(5), s->overlap.d_total,
                                       counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) {
            return enqueue_boxes_fill(s, nodes, n_nodes, hs.dev(0), n, margin, hs.dev<const int32_t>(1), hs.dev<const uint32_t>(2), capacity, hs.dev<int32_t>(3), hs.dev(4), stream);
        });
}

// ---- region overlap lists: every sphere of the scene that reaches into each convex region of six planes (rt_region.hpp) ----

rt_status rt_overlap_regions_device(rt_scene *s, const void *planes, uint32_t n, double margin, uint32_t sections, uint32_t capacity, int32_t *items_out,
                                    void *gap_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats, void *hip_stream)
{
    const char *const what = "rt_overlap_regions_device";
    if (!regions_args_ok(s, planes, n, margin, sections, capacity, items_out, gap_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    const uint32_t J = region_sections_of(s, n, sections);
    // region calls take their turn with overlap, box, swept and first-contact calls: they share the counts and the offsets
    return device_list_query(
        s, s->overlap, capacity != 0u && items_out, stats, static_cast<hipStream_t>(hip_stream),
        [&](const void *, uint32_t, hipStream_t stream) { return overlap_begin(s, n * J, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_regions_count(s, nodes, n_nodes, planes, n, margin, J, offsets_out, total_out, counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) {
            return enqueue_regions_fill(s, nodes, n_nodes, planes, n, margin, J, capacity, items_out, gap_out, stream);
        });
}

rt_status rt_overlap_regions(rt_scene *s, const void *planes, uint32_t n, double margin, uint32_t sections, uint32_t capacity, int32_t *items_out, void *gap_out,
                             uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats)
{
    const char *const what = "rt_overlap_regions";
    if (!regions_args_ok(s, planes, n, margin, sections, capacity, items_out, gap_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    const uint32_t J = region_sections_of(s, n, sections);
    const bool fill = capacity != 0u && items_out;
    const size_t esz = real_size(s);
    HostStaging::Row rows[] = { { planes, 24 * esz * (size_t)n, kStageIn },
                                { fill ? items_out : nullptr, sizeof(int32_t) * (size_t)capacity, kStageOut, sizeof(int32_t) },
                                { fill ? gap_out : nullptr, esz * (size_t)capacity, kStageOut, esz },
                                { offsets_out, sizeof(uint64_t) * ((size_t)n + 1), kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what, total_out); pst != RT_OK) return pst;
    if (!regions_valid(s, planes, n, what)) return RT_ERR_INVALID_ARGUMENT;
    return host_list_query(
        s, s->overlap, hs, capacity, fill, total_out, stats,
        [&](const void *, uint32_t, hipStream_t stream) { return overlap_begin(s, n * J, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_regions_count(s, nodes, n_nodes, hs.dev(0), n, margin, J, hs.dev<uint64_t>(3), s->overlap.d_total, counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) {
            return enqueue_regions_fill(s, nodes, n_nodes, hs.dev(0), n, margin, J, capacity, hs.dev<int32_t>(1), hs.dev(2), stream);
        });
}

// ---- swept overlap lists: every sphere of the scene a moving outside sphere comes into contact with during one step (rt_swept.hpp) ----

rt_status rt_swept_overlaps_device(rt_scene *s, const void *queries, const void *qdisp, uint32_t n, const void *disp, const int32_t *exclude, const uint32_t *order,
                                   uint32_t capacity, int32_t *items_out, void *time_out, void *normal_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats,
                                   void *hip_stream)
{
    const char *const what = "rt_swept_overlaps_device";
    if (!swept_args_ok(s, queries, qdisp, n, disp, exclude, order, capacity, items_out, time_out, normal_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    // swept calls take their turn with overlap calls: they share the counts and the offsets
    return device_list_query(
        s, s->overlap, capacity != 0u && items_out, stats, static_cast<hipStream_t>(hip_stream),
        [&](const void *, uint32_t n_nodes, hipStream_t stream) { return swept_begin(s, n, n_nodes, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_swept_count(s, nodes, n_nodes, queries, qdisp, n, disp, exclude, order, offsets_out, total_out, counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) {
            return enqueue_swept_fill(s, nodes, n_nodes, queries, qdisp, n, exclude, order, capacity, items_out, time_out, normal_out, stream);
        });
}

rt_status rt_swept_overlaps(rt_scene *s, const void *queries, const void *qdisp, uint32_t n, const void *disp, const int32_t *exclude, const uint32_t *order,
                            uint32_t capacity, int32_t *items_out, void *time_out, void *normal_out, uint64_t *offsets_out, uint64_t *total_out, rt_stats *stats)
{
    const char *const what = "rt_swept_overlaps";
    if (!swept_args_ok(s, queries, qdisp, n, disp, exclude, order, capacity, items_out, time_out, normal_out, offsets_out, total_out, what)) return RT_ERR_INVALID_ARGUMENT;
    const bool fill = capacity != 0u && items_out;
    const size_t esz = real_size(s);
    HostStaging::Row rows[] = { { queries, 4 * esz * (size_t)n, kStageIn }, { qdisp, 3 * esz * (size_t)n, kStageIn }, { disp, 3 * esz * (size_t)s->n_items, kStageIn },
                                { exclude, sizeof(int32_t) * (size_t)n, kStageIn }, { order, sizeof(uint32_t) * (size_t)n, kStageIn },
                                { fill ? items_out : nullptr, sizeof(int32_t) * (size_t)capacity, kStageOut, sizeof(int32_t) },
                                { fill ? time_out : nullptr, esz * (size_t)capacity, kStageOut, esz },
                                { fill ? normal_out : nullptr, 3 * esz * (size_t)capacity, kStageOut, 3 * esz },
                                { offsets_out, sizeof(uint64_t) * ((size_t)n + 1), kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what, total_out); pst != RT_OK) return pst;
    if (!overlap_queries_valid(s, queries, n, what)) return RT_ERR_INVALID_ARGUMENT;
    if (!swept_qdisp_valid(s, qdisp, n, what)) return RT_ERR_INVALID_ARGUMENT;
    if (order && !order_is_permutation(order, n, what)) return RT_ERR_INVALID_ARGUMENT;
    if (disp && !impacts_disp_valid(s, disp, s->n_items, what)) return RT_ERR_INVALID_ARGUMENT;
    // (the overlap workspace: host calls on one scene take turns, overlap and swept alike)
    return host_list_query(
        s, s->overlap, hs, capacity, fill, total_out, stats,
        [&](const void *, uint32_t n_nodes, hipStream_t stream) { return swept_begin(s, n, n_nodes, stream); },
        [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
            return enqueue_swept_count(s, nodes, n_nodes, hs.dev(0), hs.dev(1), n, hs.dev(2), hs.dev<const int32_t>(3), hs.dev<const uint32_t>(4), hs.dev<uint64_t>(8),
                                       s->overlap.d_total, counters, stream);
        },
        [&](const void *nodes, uint32_t n_nodes, hipStream_t stream) {
            return enqueue_swept_fill(s, nodes, n_nodes, hs.dev(0), hs.dev(1), n, hs.dev<const int32_t>(3), hs.dev<const uint32_t>(4), capacity, hs.dev<int32_t>(5), hs.dev(6),
                                      hs.dev(7), stream);
        });
}

// ---- first contacts: the earliest contact of each moving outside sphere with the scene during one step (rt_first.hpp) ----

rt_status rt_first_contacts_device(rt_scene *s, rt_sweep mode, const void *queries, const void *qdisp, uint32_t n, const void *disp, const int32_t *exclude,
                                   const uint32_t *order, void *time_out, int32_t *item_out, void *normal_out, rt_stats *stats, void *hip_stream)
{
    const char *const what = "rt_first_contacts_device";
    if (!first_args_ok(s, mode, queries, qdisp, n, disp, exclude, order, time_out, item_out, normal_out, what)) return RT_ERR_INVALID_ARGUMENT;
    // first-contact calls take their turn with overlap and swept calls: they use the swept entry's motion table
    return device_query(s, stats, static_cast<hipStream_t>(hip_stream), [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
        return enqueue_first(s, nodes, n_nodes, mode, queries, qdisp, n, disp, exclude, order, time_out, item_out, normal_out, counters, stream);
    });
}

rt_status rt_first_contacts(rt_scene *s, rt_sweep mode, const void *queries, const void *qdisp, uint32_t n, const void *disp, const int32_t *exclude,
                            const uint32_t *order, void *time_out, int32_t *item_out, void *normal_out, rt_stats *stats)
{
    const char *const what = "rt_first_contacts";
    if (!first_args_ok(s, mode, queries, qdisp, n, disp, exclude, order, time_out, item_out, normal_out, what)) return RT_ERR_INVALID_ARGUMENT;
    const size_t esz = real_size(s);
    HostStaging::Row rows[] = { { queries, 4 * esz * (size_t)n, kStageIn }, { qdisp, 3 * esz * (size_t)n, kStageIn }, { disp, 3 * esz * (size_t)s->n_items, kStageIn },
                                { exclude, sizeof(int32_t) * (size_t)n, kStageIn }, { order, sizeof(uint32_t) * (size_t)n, kStageIn },
                                { time_out, esz * (size_t)n, kStageOut }, { item_out, sizeof(int32_t) * (size_t)n, kStageOut },
                                { normal_out, 3 * esz * (size_t)n, kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what); pst != RT_OK) return pst;
    if (!overlap_queries_valid(s, queries, n, what)) return RT_ERR_INVALID_ARGUMENT;
    if (!swept_qdisp_valid(s, qdisp, n, what)) return RT_ERR_INVALID_ARGUMENT;
    if (order && !order_is_permutation(order, n, what)) return RT_ERR_INVALID_ARGUMENT;
    if (disp && !impacts_disp_valid(s, disp, s->n_items, what)) return RT_ERR_INVALID_ARGUMENT;
    return host_query(s, hs, stats, read_query_stats, no_pre_step, [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
        return enqueue_first(s, nodes, n_nodes, mode, hs.dev(0), hs.dev(1), n, hs.dev(2), hs.dev<const int32_t>(3), hs.dev<const uint32_t>(4), hs.dev(5),
                             hs.dev<int32_t>(6), hs.dev(7), counters, stream);
    });
}

// ---- traced rays and camera frames: Renderer::raytrace for any ray, render_region for any pinhole camera (rt_trace.hpp) ----

static rt_status trace_rays_device(rt_scene *s, const void *rays, uint32_t n, void *color_out, void *alpha_out, bool ordered, const uint32_t *order,
                                   void *hip_stream, rt_stats *stats, const char *what)
{
    if (!trace_args_ok(s, rays, n, color_out, alpha_out, what)) return RT_ERR_INVALID_ARGUMENT;
    if (ordered && !device_order_ok(order, what)) return RT_ERR_INVALID_ARGUMENT;
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const void *nodes = nullptr;
    uint32_t n_nodes = 0;
    rt_status st = query_stream(s, stream, &nodes, &n_nodes);
    if (st != RT_OK) return st;
    const bool sort = ordered && !order;
    if (!stats && !sort)
        return enqueue_trace(s, nodes, n_nodes, rays, n, color_out, alpha_out, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, stream, order);
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    if (sort && (st = enqueue_ray_order(s, c, rays, n, nullptr, stream, &order)) != RT_OK) return behind_enqueued(c, lease, stream, st);
    if (stats) {
        if (hipError_t e = hipMemsetAsync(c->d_counters, 0, sizeof(rt::Counters) * rt::kCounterStripes, stream); e != hipSuccess)
            return sort ? behind_enqueued(c, lease, stream, hip_fail(e, "hipMemsetAsync(counters)", __LINE__)) : hip_fail(e, "hipMemsetAsync(counters)", __LINE__);
        if (hipError_t e = hipEventRecord(c->ev0, stream); e != hipSuccess)
            return sort ? behind_enqueued(c, lease, stream, hip_fail(e, "hipEventRecord", __LINE__)) : hip_fail(e, "hipEventRecord", __LINE__);
    }
    st = enqueue_trace(s, nodes, n_nodes, rays, n, color_out, alpha_out, nullptr, nullptr, nullptr, 0, 0, nullptr, stats ? c->d_counters : nullptr, stream,
                       order);
    (void)hipEventRecord(c->ev1, stream);
    if (st != RT_OK) { (void)hipGetLastError(); lease.inflight = true; return st; }      // (the context goes back behind what is enqueued)
    if (stats) return read_trace_stats(c, stream, stats);
    lease.inflight = true;                              // the order in the workspace is in use until ev1: asynchronous return
    return RT_OK;
}

rt_status rt_trace_rays_device(rt_scene *s, const void *rays, uint32_t n, void *color_out, void *alpha_out, void *hip_stream, rt_stats *stats)
{
    return trace_rays_device(s, rays, n, color_out, alpha_out, false, nullptr, hip_stream, stats, "rt_trace_rays_device");
}

rt_status rt_trace_rays_ordered_device(rt_scene *s, const void *rays, uint32_t n, const uint32_t *order, void *color_out, void *alpha_out,
                                       void *hip_stream, rt_stats *stats)
{
    return trace_rays_device(s, rays, n, color_out, alpha_out, true, order, hip_stream, stats, "rt_trace_rays_ordered_device");
}

static rt_status trace_rays_host(rt_scene *s, const void *rays, uint32_t n, void *color_out, void *alpha_out, bool ordered, const uint32_t *order,
                                 rt_stats *stats, const char *what)
{
    if (!trace_args_ok(s, rays, n, color_out, alpha_out, what)) return RT_ERR_INVALID_ARGUMENT;
    if (ordered && !device_order_ok(order, what)) return RT_ERR_INVALID_ARGUMENT;
    const size_t esz = real_size(s);
    HostStaging::Row rows[] = { { rays, 6 * esz * n, kStageIn }, { color_out, 3 * esz * n, kStageOut }, { alpha_out, esz * n, kStageOut }, { order, sizeof(uint32_t) * n, kStageIn } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan(what); pst != RT_OK) return pst;
    if (!query_rays_valid(s, rays, nullptr, n)) return RT_ERR_INVALID_ARGUMENT;
    if (order && !order_is_permutation(order, n, what)) return RT_ERR_INVALID_ARGUMENT;
    const uint32_t *d_order = nullptr;
    return host_query(s, hs, stats, read_trace_stats,
                      [&](Context *c) { d_order = hs.dev<const uint32_t>(3); return ordered && !order ? enqueue_ray_order(s, c, hs.dev(0), n, nullptr, c->stream, &d_order) : RT_OK; },
                      [&](const void *nodes, uint32_t n_nodes, rt::Counters *counters, hipStream_t stream) {
                          return enqueue_trace(s, nodes, n_nodes, hs.dev(0), n, hs.dev(1), hs.dev(2), nullptr, nullptr, nullptr, 0, 0, nullptr, counters, stream, d_order);
                      });
}

rt_status rt_trace_rays(rt_scene *s, const void *rays, uint32_t n, void *color_out, void *alpha_out, rt_stats *stats)
{
    return trace_rays_host(s, rays, n, color_out, alpha_out, false, nullptr, stats, "rt_trace_rays");
}

rt_status rt_trace_rays_ordered(rt_scene *s, const void *rays, uint32_t n, const uint32_t *order, void *color_out, void *alpha_out, rt_stats *stats)
{
    return trace_rays_host(s, rays, n, color_out, alpha_out, true, order, stats, "rt_trace_rays_ordered");
}

// ---- coherent ray batches: the order the *_ordered entries take, computed on the device (rt_order.hpp) ----

rt_status rt_ray_order_device(rt_scene *s, const void *rays, uint32_t n, uint32_t *order_out, void *hip_stream)
{
    if (!order_args_ok(s, rays, n, order_out, "rt_ray_order_device")) return RT_ERR_INVALID_ARGUMENT;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    Context *c = nullptr;
    rt_status st = acquire(s, &c);
    if (st != RT_OK) return st;
    Lease lease{ s, c };
    const uint32_t *used = nullptr;
    st = enqueue_ray_order(s, c, rays, n, order_out, stream, &used);
    (void)hipEventRecord(c->ev1, stream);               // (the context goes back behind what is enqueued: its workspace is in use until then)
    if (st != RT_OK) (void)hipGetLastError();
    lease.inflight = true;
    return st;
}

// Shared body of rt_ray_order and rt_sphere_order, `hs` planned: row 0 up, the order `enqueue` makes of it into row 1, and that back.
static rt_status order_host(rt_scene *s, HostStaging &hs, uint32_t n,
                            rt_status (*enqueue)(const rt_scene *, Context *, const void *, uint32_t, uint32_t *, hipStream_t, const uint32_t **))
{
    HIP_TRY(hipSetDevice(s->device));
    Context *c = nullptr;
    rt_status st = acquire(s, &c);
    if (st != RT_OK) return st;
    Lease lease{ s, c };
    if ((st = hs.bind(c)) != RT_OK) return st;
    if ((st = hs.upload(c)) != RT_OK) return st;
    const uint32_t *used = nullptr;
    if ((st = enqueue(s, c, hs.dev(0), n, hs.dev<uint32_t>(1), c->stream, &used)) != RT_OK) return drain(c, st);
    if ((st = hs.download(c)) != RT_OK) return st;
    HIP_TRY_DRAIN(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

rt_status rt_ray_order(rt_scene *s, const void *rays, uint32_t n, uint32_t *order_out)
{
    if (!order_args_ok(s, rays, n, order_out, "rt_ray_order")) return RT_ERR_INVALID_ARGUMENT;
    HostStaging::Row rows[] = { { rays, 6 * real_size(s) * n, kStageIn }, { order_out, sizeof(uint32_t) * n, kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan("rt_ray_order"); pst != RT_OK) return pst;
    if (!query_rays_valid(s, rays, nullptr, n)) return RT_ERR_INVALID_ARGUMENT;
    return order_host(s, hs, n, enqueue_ray_order);
}

// ---- sphere orders, balanced ranges and rebuilds: a dynamic scene's hierarchy rebuilt on the device (rt_rebuild.hpp) ----

// A topology from the item count alone: DFS pre-order of the halving of (0, n_items) down to leaf_size.  No device is touched.
rt_status rt_balanced_ranges(uint32_t n_items, uint32_t leaf_size, rt_range *ranges_out, uint32_t *n_groups_out)
{
    if (n_items == 0 || leaf_size == 0 || !ranges_out || !n_groups_out || n_items > 0x7FFFFFFFu) {
        snprintf(g_err, sizeof g_err, "rt_balanced_ranges: NULL argument, n_items == 0 (or above 2^31 - 1) or leaf_size == 0");
        return RT_ERR_INVALID_ARGUMENT;
    }
    uint32_t groups = 0, depth = 0;
    struct { uint32_t first, count; } todo[64];                      // the right halves still to emit: one per level, the levels are < 33
    todo[depth++] = { 0u, n_items };
    while (depth) {
        const uint32_t first = todo[depth - 1].first, count = todo[depth - 1].count;
        --depth;
        ranges_out[groups++] = rt_range{ (int32_t)first, (int32_t)count };
        if (count > leaf_size) {
            const uint32_t left = count / 2 + (count & 1u);          // (count + 1) / 2 without the carry
            todo[depth++] = { first + left, count - left };
            todo[depth++] = { first, left };
        }
    }
    *n_groups_out = groups;
    return RT_OK;
}

// spheres and order_out as both rt_sphere_order entries check them; `align`: what a spheres pointer must be a multiple of.
static bool sphere_order_args_ok(const rt_scene *s, const void *spheres, uint32_t n, const uint32_t *order_out, uintptr_t align, const char *what)
{
    if (!s || !spheres || !order_out || n == 0) { snprintf(g_err, sizeof g_err, "%s: NULL scene, spheres or order_out, or n == 0", what); return false; }
    if ((reinterpret_cast<uintptr_t>(spheres) % align) != 0) { snprintf(g_err, sizeof g_err, "%s: spheres must be %u-byte aligned", what, (unsigned)align); return false; }
    if ((reinterpret_cast<uintptr_t>(order_out) & 3u) != 0) { snprintf(g_err, sizeof g_err, "%s: order_out must be 4-byte aligned", what); return false; }
    return true;
}

rt_status rt_sphere_order_device(rt_scene *s, const void *spheres, uint32_t n, uint32_t *order_out, void *hip_stream)
{
    const uintptr_t record = s ? (s->precision == RT_F32 ? sizeof(float) : sizeof(double)) * 4 : 16;      // one {cx, cy, cz, r}: the kernels load it whole
    if (!sphere_order_args_ok(s, spheres, n, order_out, record, "rt_sphere_order_device")) return RT_ERR_INVALID_ARGUMENT;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    Context *c = nullptr;
    rt_status st = acquire(s, &c);
    if (st != RT_OK) return st;
    Lease lease{ s, c };
    const uint32_t *used = nullptr;
    st = enqueue_sphere_order(s, c, spheres, n, order_out, stream, &used);
    (void)hipEventRecord(c->ev1, stream);               // (the context goes back behind what is enqueued: its workspace is in use until then)
    if (st != RT_OK) (void)hipGetLastError();
    lease.inflight = true;
    return st;
}

rt_status rt_sphere_order(rt_scene *s, const void *spheres, uint32_t n, uint32_t *order_out)
{
    const uintptr_t esz = s && s->precision == RT_F64 ? sizeof(double) : sizeof(float);
    if (!sphere_order_args_ok(s, spheres, n, order_out, esz, "rt_sphere_order")) return RT_ERR_INVALID_ARGUMENT;
    // both buffers go through the call's workspace, whatever memory they are: the kernels load a sphere whole, and a host pointer need
    // only be aligned to one of its elements
    HostStaging::Row rows[] = { { spheres, 4 * esz * n, kStageIn }, { order_out, sizeof(uint32_t) * n, kStageOut } };
    HostStaging hs(rows);
    if (rt_status pst = hs.plan("rt_sphere_order", nullptr, false); pst != RT_OK) return pst;
    if (!(s->precision == RT_F32 ? items_valid<float>(spheres, n, true) : items_valid<double>(spheres, n, true))) {
        snprintf(g_err, sizeof g_err, "rt_sphere_order: spheres must be finite, |v| <= 1e15, radius > 0");
        return RT_ERR_INVALID_ARGUMENT;
    }
    return order_host(s, hs, n, enqueue_sphere_order);
}

rt_status rt_scene_rebuild(rt_scene *s, const void *spheres, uint32_t *order_out)
{
    if (rt_status ast = rebuild_scene_ok(s, spheres, "rt_scene_rebuild"); ast != RT_OK) return ast;
    const size_t esz = s->precision == RT_F32 ? sizeof(float) : sizeof(double);
    if ((reinterpret_cast<uintptr_t>(spheres) % esz) != 0 || (reinterpret_cast<uintptr_t>(order_out) & 3u) != 0) {
        snprintf(g_err, sizeof g_err, "rt_scene_rebuild: spheres must be %u-byte and order_out 4-byte aligned", (unsigned)esz);
        return RT_ERR_INVALID_ARGUMENT;
    }
    if (!(s->precision == RT_F32 ? items_valid<float>(spheres, s->n_items, true) : items_valid<double>(spheres, s->n_items, true))) {
        snprintf(g_err, sizeof g_err, "rt_scene_rebuild: spheres must be finite, |v| <= 1e15, radius > 0; the scene is unchanged");
        return RT_ERR_INVALID_ARGUMENT;
    }
    std::unique_lock<std::shared_mutex> lk(s->dyn_mu);               // as a host update: every host call under way has returned, none starts before this one has
    HIP_TRY(hipSetDevice(s->device));
    // the spheres into the scene's staging as a host update's items go, the rebuild behind them on the scene's stream
    memcpy(s->h_up, spheres, esz * 4 * s->n_items);
    HIP_TRY(hipStreamWaitEvent(s->cost_stream, s->upd_ev, 0));       // (a device rebuild still in flight on another stream is using the rebuild workspace)
    rt_status st = upload_words(s->d_stage, s->h_up, esz * 4 * s->n_items, s->cost_stream);
    const uint32_t *used = nullptr;
    if (st == RT_OK) st = enqueue_rebuild(s, s->d_stage, nullptr, s->cost_stream, &used);
    hipError_t e = hipSuccess;
    if (st == RT_OK && order_out) e = hipMemcpyAsync(order_out, used, sizeof(uint32_t) * s->n_items, hipMemcpyDeviceToHost, s->cost_stream);
    const hipError_t se = hipStreamSynchronize(s->cost_stream);
    if (st != RT_OK) { (void)hipGetLastError(); return st; }
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(order)", __LINE__);
    if (se != hipSuccess) return hip_fail(se, "hipStreamSynchronize(rebuild)", __LINE__);
    return RT_OK;
}

rt_status rt_scene_rebuild_device(rt_scene *s, const void *spheres_device, uint32_t *order_out_device, void *hip_stream)
{
    if (rt_status ast = rebuild_scene_ok(s, spheres_device, "rt_scene_rebuild_device"); ast != RT_OK) return ast;
    const uintptr_t align = (s->precision == RT_F32 ? sizeof(float) : sizeof(double)) * 4;      // one {cx, cy, cz, r} record: the kernels load it whole
    if ((reinterpret_cast<uintptr_t>(spheres_device) % align) != 0 || (reinterpret_cast<uintptr_t>(order_out_device) & 3u) != 0) {
        snprintf(g_err, sizeof g_err, "rt_scene_rebuild_device: spheres must be %u-byte and order_out 4-byte aligned", (unsigned)align);
        return RT_ERR_INVALID_ARGUMENT;
    }
    const ReadLock rl(s);                                            // (not while a host update is replacing the scene)
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t *used = nullptr;
    return enqueue_rebuild(s, spheres_device, order_out_device, static_cast<hipStream_t>(hip_stream), &used);
}

// What both rt_scene_rebuild_n entries check before the device is touched; `align`: what a spheres pointer must be a multiple of.
static rt_status rebuild_n_args_ok(const rt_scene *s, const void *spheres, uint32_t n, const uint32_t *order_out, uintptr_t align, const char *what)
{
    if (!s) { snprintf(g_err, sizeof g_err, "%s: NULL scene", what); return RT_ERR_INVALID_ARGUMENT; }
    if (n != 0u && !spheres) { snprintf(g_err, sizeof g_err, "%s: NULL spheres with n = %u", what, n); return RT_ERR_INVALID_ARGUMENT; }
    if (n > s->n_items) { snprintf(g_err, sizeof g_err, "%s: n = %u is above the scene's capacity of %u items", what, n, s->n_items); return RT_ERR_INVALID_ARGUMENT; }
    if (rt_status ast = rebuild_scene_ok(s, s, what); ast != RT_OK) return ast;      // (a dynamic scene with groups; the spheres are checked here)
    if ((reinterpret_cast<uintptr_t>(spheres) % align) != 0 || (reinterpret_cast<uintptr_t>(order_out) & 3u) != 0) {
        snprintf(g_err, sizeof g_err, "%s: spheres must be %u-byte and order_out 4-byte aligned", what, (unsigned)align);
        return RT_ERR_INVALID_ARGUMENT;
    }
    return RT_OK;
}

rt_status rt_scene_rebuild_n(rt_scene *s, const void *spheres, uint32_t n, uint32_t *order_out)
{
    const size_t esz = s && s->precision == RT_F64 ? sizeof(double) : sizeof(float);
    if (rt_status ast = rebuild_n_args_ok(s, spheres, n, order_out, esz, "rt_scene_rebuild_n"); ast != RT_OK) return ast;
    if (n != 0u && !(s->precision == RT_F32 ? items_valid<float>(spheres, n, true) : items_valid<double>(spheres, n, true))) {
        snprintf(g_err, sizeof g_err, "rt_scene_rebuild_n: spheres must be finite, |v| <= 1e15, radius > 0; the scene is unchanged");
        return RT_ERR_INVALID_ARGUMENT;
    }
    std::unique_lock<std::shared_mutex> lk(s->dyn_mu);               // as rt_scene_rebuild
    HIP_TRY(hipSetDevice(s->device));
    if (n != 0u) memcpy(s->h_up, spheres, esz * 4 * n);
    HIP_TRY(hipStreamWaitEvent(s->cost_stream, s->upd_ev, 0));       // (a device rebuild still in flight on another stream is using the rebuild workspace)
    rt_status st = n != 0u ? upload_words(s->d_stage, s->h_up, esz * 4 * n, s->cost_stream) : RT_OK;
    const uint32_t *used = nullptr;
    if (st == RT_OK) st = enqueue_rebuild_n(s, s->d_stage, n, nullptr, s->cost_stream, &used);
    hipError_t e = hipSuccess;
    if (st == RT_OK && order_out && n != 0u) e = hipMemcpyAsync(order_out, used, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s->cost_stream);
    const hipError_t se = hipStreamSynchronize(s->cost_stream);
    if (st != RT_OK) { (void)hipGetLastError(); return st; }
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(order)", __LINE__);
    if (se != hipSuccess) return hip_fail(se, "hipStreamSynchronize(rebuild)", __LINE__);
    return RT_OK;
}

rt_status rt_scene_rebuild_n_device(rt_scene *s, const void *spheres_device, uint32_t n, uint32_t *order_out_device, void *hip_stream)
{
    const uintptr_t align = (s && s->precision == RT_F64 ? sizeof(double) : sizeof(float)) * 4;      // one {cx, cy, cz, r} record: the kernels load it whole
    if (rt_status ast = rebuild_n_args_ok(s, spheres_device, n, order_out_device, align, "rt_scene_rebuild_n_device"); ast != RT_OK) return ast;
    const ReadLock rl(s);                                            // (not while a host update is replacing the scene)
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t *used = nullptr;
    return enqueue_rebuild_n(s, spheres_device, n, order_out_device, static_cast<hipStream_t>(hip_stream), &used);
}

// Shared body of both rt_render_camera entries: the frame into d_out (tile-major, 4 * total_px bytes) on `stream` through a leased
// context.  spp == 0 is the reference's black frame, as launch_render makes it.  On RT_OK the context's ev1 follows the frame.
static rt_status enqueue_camera(rt_scene *s, Context *c, const rt_options *o, const void *camera, const std::vector<rt::TileDev> &tab, uint32_t blocks,
                                uint64_t total_px, uint8_t *d_out, hipStream_t stream, bool counting)
{
    const void *nodes = nullptr;
    uint32_t n_nodes = 0;
    rt_status st = query_stream(s, stream, &nodes, &n_nodes);
    if (st != RT_OK) return st;
    const rt::TileDev *d_tab = nullptr;
    if ((st = upload_tiles(c, tab, stream, 0, &d_tab)) != RT_OK) return st;
    if (counting) {
        HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof(rt::Counters) * rt::kCounterStripes, stream));
        HIP_TRY(hipEventRecord(c->ev0, stream));
    }
    if (o->samples_per_pixel == 0) HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)total_px * 4, stream));
    else if ((st = enqueue_trace(s, nodes, n_nodes, nullptr, 0, nullptr, nullptr, o, camera, d_tab, (uint32_t)tab.size(), blocks, d_out,
                                 counting ? c->d_counters : nullptr, stream)) != RT_OK) return st;
    HIP_TRY(hipEventRecord(c->ev1, stream));
    return RT_OK;
}

static bool camera_args_ok(rt_scene *s, const rt_options *o, const void *camera, const rt_region *tiles, uint32_t n, const void *out, const char *what)
{
    if (!check_common(s, o, tiles, n, out)) return false;
    if (!camera) { snprintf(g_err, sizeof g_err, "%s: NULL camera", what); return false; }
    return camera_valid(s, camera, what);
}

rt_status rt_render_camera_device(rt_scene *s, const rt_options *o, const void *camera, const rt_region *tiles, uint32_t n, void *rgba_out_device,
                                  void *hip_stream, rt_stats *stats)
{
    if (!camera_args_ok(s, o, camera, tiles, n, rgba_out_device, "rt_render_camera_device")) return RT_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(rgba_out_device) & 3u) != 0) {
        snprintf(g_err, sizeof g_err, "the device output buffer must be 4-byte aligned");
        return RT_ERR_INVALID_ARGUMENT;
    }
    std::vector<rt::TileDev> tab;
    uint64_t total_px = 0; uint32_t total_blocks = 0;
    rt_status st = build_tile_table(o, tiles, n, tab, &total_px, &total_blocks);
    if (st != RT_OK) return st;
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    st = enqueue_camera(s, c, o, camera, tab, total_blocks, total_px, static_cast<uint8_t *>(rgba_out_device), stream, stats != nullptr);
    if (st != RT_OK) {
        (void)hipEventRecord(c->ev1, stream);           // (the context goes back behind what is enqueued)
        (void)hipGetLastError();
        lease.inflight = true;
        return st;
    }
    if (stats) return read_trace_stats(c, stream, stats);
    lease.inflight = true;                              // the tile table is in use until ev1: asynchronous return
    return RT_OK;
}

rt_status rt_render_camera(rt_scene *s, const rt_options *o, const void *camera, const rt_region *tiles, uint32_t n, uint8_t *rgba_out, rt_stats *stats)
{
    if (!camera_args_ok(s, o, camera, tiles, n, rgba_out, "rt_render_camera")) return RT_ERR_INVALID_ARGUMENT;
    std::vector<rt::TileDev> tab;
    uint64_t total_px = 0; uint32_t total_blocks = 0;
    rt_status st = build_tile_table(o, tiles, n, tab, &total_px, &total_blocks);
    if (st != RT_OK) return st;
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    const HostDest dest = classify_host_pointer(rgba_out);
    if (dest.bad) {
        snprintf(g_err, sizeof g_err, "rt_render_camera: rgba_out is device memory; use rt_render_camera_device");
        return RT_ERR_INVALID_ARGUMENT;
    }
    const size_t bytes = (size_t)total_px * 4;
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    // pinned memory is written by the kernel in place; anything else gets the context's device output and one copy back
    const bool direct = dest.pinned && dest.dev_alias && dest.room >= bytes;
    if (!direct && c->out_cap < bytes) {
        if (c->d_out) HIP_TRY(hipFree(c->d_out));
        c->d_out = nullptr; c->out_cap = 0;
        HIP_TRY(hipMalloc(&c->d_out, bytes));
        c->out_cap = bytes;
    }
    st = enqueue_camera(s, c, o, camera, tab, total_blocks, total_px, direct ? dest.dev_alias : c->d_out, c->stream, stats != nullptr);
    if (st != RT_OK) { (void)hipStreamSynchronize(c->stream); (void)hipGetLastError(); return st; }
    if (!direct) {
        const hipError_t e = hipMemcpyAsync(rgba_out, c->d_out, bytes, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return hip_fail(e, "hipMemcpyAsync", __LINE__); }
    }
    if (stats) return read_trace_stats(c, c->stream, stats);          // synchronises the stream
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RT_OK;
}

// ---- undersampled camera frames: one sample per step x step cell, refined in place (rt_undersample.hpp) ----

// Shared body of both rt_render_camera_undersampled entries, as enqueue_camera: the pass into d_out (which holds the step-2s frame when
// prev_step != 0) on `stream` through a leased context.  On RT_OK the context's ev1 follows the pass.
static rt_status enqueue_camera_undersampled(rt_scene *s, Context *c, const rt_options *o, const void *camera, std::vector<rt::TileDev> &tab,
                                             uint32_t blocks16, uint64_t total_px, uint32_t step, uint32_t prev_step, uint8_t *d_out, hipStream_t stream,
                                             bool counting)
{
    if (step == 1 && prev_step == 0) return enqueue_camera(s, c, o, camera, tab, blocks16, total_px, d_out, stream, counting);
    const void *nodes = nullptr;
    uint32_t n_nodes = 0;
    rt_status st = query_stream(s, stream, &nodes, &n_nodes);
    if (st != RT_OK) return st;
    uint32_t blocks = 0;
    if ((st = undersample_blocks(tab, step, prev_step != 0, &blocks)) != RT_OK) return st;
    const rt::TileDev *d_tab = nullptr;
    if ((st = upload_tiles(c, tab, stream, 0, &d_tab)) != RT_OK) return st;
    if (counting) {
        HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof(rt::Counters) * rt::kCounterStripes, stream));
        HIP_TRY(hipEventRecord(c->ev0, stream));
    }
    rt::Counters *const counters = counting ? c->d_counters : nullptr;
    st = s->precision == RT_F32
             ? enqueue_undersampled<float>(s, nodes, n_nodes, o, camera, d_tab, (uint32_t)tab.size(), blocks, step, prev_step != 0, d_out, counters, stream)
             : enqueue_undersampled<double>(s, nodes, n_nodes, o, camera, d_tab, (uint32_t)tab.size(), blocks, step, prev_step != 0, d_out, counters, stream);
    if (st != RT_OK) return st;
    HIP_TRY(hipEventRecord(c->ev1, stream));
    return RT_OK;
}

rt_status rt_render_camera_undersampled_device(rt_scene *s, const rt_options *o, const void *camera, const rt_region *tiles, uint32_t n, uint32_t step,
                                               uint32_t prev_step, void *rgba_inout_device, void *hip_stream, rt_stats *stats)
{
    if (!undersample_args_ok(step, prev_step, "rt_render_camera_undersampled_device")) return RT_ERR_INVALID_ARGUMENT;
    if (!camera_args_ok(s, o, camera, tiles, n, rgba_inout_device, "rt_render_camera_undersampled_device")) return RT_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(rgba_inout_device) & 3u) != 0) {
        snprintf(g_err, sizeof g_err, "the device output buffer must be 4-byte aligned");
        return RT_ERR_INVALID_ARGUMENT;
    }
    std::vector<rt::TileDev> tab;
    uint64_t total_px = 0; uint32_t total_blocks = 0;
    rt_status st = build_tile_table(o, tiles, n, tab, &total_px, &total_blocks);
    if (st != RT_OK) return st;
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    st = enqueue_camera_undersampled(s, c, o, camera, tab, total_blocks, total_px, step, prev_step, static_cast<uint8_t *>(rgba_inout_device), stream,
                                     stats != nullptr);
    if (st != RT_OK) {
        (void)hipEventRecord(c->ev1, stream);           // (the context goes back behind what is enqueued)
        (void)hipGetLastError();
        lease.inflight = true;
        return st;
    }
    if (stats) return read_trace_stats(c, stream, stats);
    lease.inflight = true;                              // the tile table is in use until ev1: asynchronous return
    return RT_OK;
}

rt_status rt_render_camera_undersampled(rt_scene *s, const rt_options *o, const void *camera, const rt_region *tiles, uint32_t n, uint32_t step,
                                        uint32_t prev_step, uint8_t *rgba_inout, rt_stats *stats)
{
    if (!undersample_args_ok(step, prev_step, "rt_render_camera_undersampled")) return RT_ERR_INVALID_ARGUMENT;
    if (!camera_args_ok(s, o, camera, tiles, n, rgba_inout, "rt_render_camera_undersampled")) return RT_ERR_INVALID_ARGUMENT;
    std::vector<rt::TileDev> tab;
    uint64_t total_px = 0; uint32_t total_blocks = 0;
    rt_status st = build_tile_table(o, tiles, n, tab, &total_px, &total_blocks);
    if (st != RT_OK) return st;
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    const HostDest dest = classify_host_pointer(rgba_inout);
    if (dest.bad) {
        snprintf(g_err, sizeof g_err, "rt_render_camera_undersampled: rgba_inout is device memory; use rt_render_camera_undersampled_device");
        return RT_ERR_INVALID_ARGUMENT;
    }
    const size_t bytes = (size_t)total_px * 4;
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    // pinned memory is refined by the kernel in place; anything else goes through the context's device output: up first when the pass
    // keeps cells of the frame it finds (prev_step != 0), and one copy back
    const bool direct = dest.pinned && dest.dev_alias && dest.room >= bytes;
    if (!direct && c->out_cap < bytes) {
        if (c->d_out) HIP_TRY(hipFree(c->d_out));
        c->d_out = nullptr; c->out_cap = 0;
        HIP_TRY(hipMalloc(&c->d_out, bytes));
        c->out_cap = bytes;
    }
    if (!direct && prev_step != 0) {
        const hipError_t e = hipMemcpyAsync(c->d_out, rgba_inout, bytes, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return hip_fail(e, "hipMemcpyAsync", __LINE__); }
    }
    st = enqueue_camera_undersampled(s, c, o, camera, tab, total_blocks, total_px, step, prev_step, direct ? dest.dev_alias : c->d_out, c->stream,
                                     stats != nullptr);
    if (st != RT_OK) { (void)hipStreamSynchronize(c->stream); (void)hipGetLastError(); return st; }
    if (!direct) {
        const hipError_t e = hipMemcpyAsync(rgba_inout, c->d_out, bytes, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return hip_fail(e, "hipMemcpyAsync", __LINE__); }
    }
    if (stats) return read_trace_stats(c, c->stream, stats);          // synchronises the stream
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RT_OK;
}

rt_status rt_host_alloc(size_t bytes, void **out)
{
    if (!out || bytes == 0) { snprintf(g_err, sizeof g_err, "rt_host_alloc: NULL argument or 0 bytes"); return RT_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    int ndev = 0;
    rt_status st = rt_device_count(&ndev);
    if (st != RT_OK) return st;
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocPortable | hipHostMallocMapped));
    void *alias = nullptr;
    if (hipHostGetDevicePointer(&alias, *out, 0) != hipSuccess) { (void)hipGetLastError(); alias = nullptr; }
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    g_pinned[reinterpret_cast<uintptr_t>(*out)] = PinnedRange{ bytes, static_cast<uint8_t *>(alias) };
    return RT_OK;
}

rt_status rt_host_free(void *p)
{
    if (!p) return RT_OK;
    {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        if (g_pinned.erase(reinterpret_cast<uintptr_t>(p)) == 0) {
            snprintf(g_err, sizeof g_err, "rt_host_free: not a pointer rt_host_alloc returned");
            return RT_ERR_INVALID_ARGUMENT;
        }
    }
    HIP_TRY(hipHostFree(p));
    return RT_OK;
}

rt_status rt_host_register(void *p, size_t bytes)
{
    if (!p || bytes == 0) { snprintf(g_err, sizeof g_err, "rt_host_register: NULL argument or 0 bytes"); return RT_ERR_INVALID_ARGUMENT; }
    int ndev = 0;
    rt_status st = rt_device_count(&ndev);
    if (st != RT_OK) return st;
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped));
    void *alias = nullptr;
    if (hipHostGetDevicePointer(&alias, p, 0) != hipSuccess) { (void)hipGetLastError(); alias = nullptr; }
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    g_pinned[reinterpret_cast<uintptr_t>(p)] = PinnedRange{ bytes, static_cast<uint8_t *>(alias) };
    return RT_OK;
}

rt_status rt_host_unregister(void *p)
{
    if (!p) return RT_OK;
    {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        if (g_pinned.erase(reinterpret_cast<uintptr_t>(p)) == 0) {
            snprintf(g_err, sizeof g_err, "rt_host_unregister: not a pointer rt_host_register was given");
            return RT_ERR_INVALID_ARGUMENT;
        }
    }
    HIP_TRY(hipHostUnregister(p));
    return RT_OK;
}

rt_status rt_blit_tiles_device(rt_scene *s, const rt_options *o, const rt_region *tiles, uint32_t n, const uint32_t *src_px_offset,
                               const void *src, void *frame, void *hip_stream)
{
    if (!check_common(s, o, tiles, n, frame) || !src) { snprintf(g_err, sizeof g_err, "rt_blit_tiles_device: NULL argument"); return RT_ERR_INVALID_ARGUMENT; }
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(frame)) & 3u) != 0) {
        snprintf(g_err, sizeof g_err, "rt_blit_tiles_device: buffers must be 4-byte aligned");
        return RT_ERR_INVALID_ARGUMENT;
    }
    std::vector<rt::TileDev> tab;
    uint64_t total_px = 0; uint32_t total_blocks = 0;
    rt_status st = build_tile_table(o, tiles, n, tab, &total_px, &total_blocks);
    if (st != RT_OK) return st;
    if (src_px_offset)
        for (uint32_t i = 0; i < n; ++i) tab[i].out_px = src_px_offset[i];
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const rt::TileDev *d_tab = nullptr;
    if ((st = device_table(s, nullptr, tab, stream, &d_tab)) != RT_OK) return st;
    if (d_tab) {                                                    // cached table: one kernel, nothing else
        hipLaunchKernelGGL(rt::k_blit_tiles, dim3(total_blocks), dim3(rt::kBlockThreads), 0, stream, (unsigned)o->width, d_tab, (unsigned)n,
                           static_cast<const unsigned *>(src), static_cast<unsigned *>(frame));
        HIP_TRY(hipGetLastError());
        return RT_OK;
    }
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    if ((st = device_table(s, c, tab, stream, &d_tab)) != RT_OK) return st;
    hipLaunchKernelGGL(rt::k_blit_tiles, dim3(total_blocks), dim3(rt::kBlockThreads), 0, stream, (unsigned)o->width, d_tab,
                       (unsigned)n, static_cast<const unsigned *>(src), static_cast<unsigned *>(frame));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, stream));
    lease.inflight = true;
    return RT_OK;
}

rt_status rt_scene_traits(const rt_scene *s, uint32_t *traits)
{
    if (!s || !traits) { snprintf(g_err, sizeof g_err, "NULL argument"); return RT_ERR_INVALID_ARGUMENT; }
    *traits = (s->n_nodes ? RT_SCENE_HAS_BOUNDS : 0u) | (s->fused ? RT_SCENE_CONCENTRIC : 0u) | (s->dynamic ? RT_SCENE_DYNAMIC : 0u);
    return RT_OK;
}

rt_status rt_scene_setup_cost(const rt_scene *s, double *total_ms, double *stream_ms)
{
    if (!s || !total_ms || !stream_ms) { snprintf(g_err, sizeof g_err, "NULL argument"); return RT_ERR_INVALID_ARGUMENT; }
    *total_ms = s->setup_total_ms;
    *stream_ms = s->setup_first_stream_ms;
    return RT_OK;
}

typedef void (*selftest_kernel)(unsigned, unsigned long long, unsigned long long *, unsigned *);
static rt_status selftest_all_f32(int device, selftest_kernel kernel, const char *what, uint64_t *mismatches, uint32_t *first_bad_bits)
{
    if (!mismatches || !first_bad_bits) return RT_ERR_INVALID_ARGUMENT;
    int ndev = 0;
    rt_status st = rt_device_count(&ndev);
    if (st != RT_OK) return st;
    if (device < 0 || device >= ndev) return RT_ERR_NO_DEVICE;
    HIP_TRY(hipSetDevice(device));
    unsigned long long *d_bad = nullptr;
    unsigned *d_first = nullptr;
    HIP_TRY(hipMalloc(&d_bad, sizeof *d_bad));
    HIP_TRY(hipMalloc(&d_first, sizeof *d_first));
    HIP_TRY(hipMemset(d_bad, 0, sizeof *d_bad));
    HIP_TRY(hipMemset(d_first, 0xFF, sizeof *d_first));
    // all 2^32 bit patterns: non-negative values, negatives, infinities and NaNs
    hipLaunchKernelGGL(kernel, dim3(256 * 32), dim3(256), 0, nullptr, 0u, 1ull << 32, d_bad, d_first);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned long long bad = 0; unsigned first = 0;
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&first, d_first, sizeof first, hipMemcpyDeviceToHost);
    (void)hipFree(d_bad); (void)hipFree(d_first);
    if (e != hipSuccess) return hip_fail(e, what, __LINE__);
    *mismatches = bad; *first_bad_bits = first;
    return RT_OK;
}

rt_status rt_selftest_sqrt(int device, uint64_t *mismatches, uint32_t *first_bad_bits)
{
    return selftest_all_f32(device, rt::k_selftest_sqrt, "rt_selftest_sqrt", mismatches, first_bad_bits);
}

rt_status rt_selftest_rcp(int device, uint64_t *mismatches, uint32_t *first_bad_bits)
{
    return selftest_all_f32(device, rt::k_selftest_rcp, "rt_selftest_rcp", mismatches, first_bad_bits);
}

constexpr int kMaxRegionLeaders = 2;

// Renders every request of `batch` in ONE pass and delivers each tile to its caller's buffer.
static void run_region_batch(rt_scene *s, const std::vector<rt_scene::RegionReq *> &batch)
{
    std::vector<rt_region> regs(batch.size());
    std::vector<uint8_t *> outs(batch.size());
    for (size_t i = 0; i < batch.size(); ++i) { regs[i] = batch[i]->region; outs[i] = batch[i]->out; }
    count_event(RT_DEBUG_COUNT_REGION_CALLS, (long long)batch.size());
    count_event(RT_DEBUG_COUNT_REGION_PASSES);
    g_err[0] = '\0';
    rt_status st = RT_OK;
    if (batch.size() == 1) {
        st = render_tiles_host(s, &batch[0]->o, batch[0]->trav, regs.data(), 1, outs[0], outs.data(), nullptr, false);
    } else {
        st = render_tiles_host(s, &batch[0]->o, batch[0]->trav, regs.data(), (uint32_t)regs.size(), outs[0], outs.data(), nullptr, false);
        if (st == RT_ERR_INVALID_REGION) {
            // one caller's bad region must not fail its neighbours: everyone on their own
            for (rt_scene::RegionReq *r : batch) {
                g_err[0] = '\0';
                r->st = render_tiles_host(s, &r->o, r->trav, &r->region, 1, r->out, &r->out, nullptr, false);
                snprintf(r->err, sizeof r->err, "%s", g_err);
            }
            return;
        }
    }
    for (rt_scene::RegionReq *r : batch) { r->st = st; snprintf(r->err, sizeof r->err, "%s", g_err); }
}

// rt_render_region through the scene's frame-ahead (rt_scene::FrameAhead).  false: the request is not a bucket of the scheduler's
// grid (render.rs:273-298: 64x64, edge buckets clipped) or the frame is too large to keep -- the caller renders it on its own.
constexpr unsigned kBucket = 64;
constexpr size_t kFrameAheadMaxBytes = (size_t)1 << 28;
constexpr uint64_t kFrameAheadMaxSampleBytes = 1ull << 30;
static bool region_from_frame_ahead(rt_scene *s, const rt_options *o, rt_traversal trav, const rt_region *region, uint8_t *out, rt_status *st)
{
    const unsigned w = o->width, h = o->height;
    if (region->l % kBucket || region->b % kBucket || region->r != std::min<unsigned>(region->l + kBucket, w) ||
        region->t != std::min<unsigned>(region->b + kBucket, h) || region->l >= w || region->b >= h)
        return false;
    const size_t frame_bytes = (size_t)w * h * 4;
    // a whole-grid pass of a sample-parallel frame also needs its per-sample buffers (spp >= 2: a word or more per sample), twice with the
    // pass rendered ahead: the bucket on its own needs a few MB -- leave large frames to the per-bucket path
    const uint64_t ns = (uint64_t)o->samples_per_pixel * o->samples_per_pixel;
    const uint64_t sample_bytes = use_split(o->samples_per_pixel) ? (uint64_t)w * h * ns * (s->precision == RT_F32 ? 5u : 9u) : 0u;
    if (frame_bytes > kFrameAheadMaxBytes || sample_bytes > kFrameAheadMaxSampleBytes || check_traversal(s, trav) != RT_OK) return false;
    const unsigned nbx = (w + kBucket - 1) / kBucket, idx = (region->b / kBucket) * nbx + region->l / kBucket;
    rt_scene::FrameAhead &a = s->ahead;
    std::unique_lock<std::mutex> lk(a.mu);
    auto drain_next = [&] { if (a.next_inflight) { (void)hipEventSynchronize(a.ev); (void)hipGetLastError(); a.next_inflight = false; } };
    // The copies out of the staging run OUTSIDE the lock (the reference's pool threads call this concurrently, render.rs:283-294), so
    // a new pass -- which replaces the staging the readers copy from -- waits until the last of them is done, and whoever was waiting
    // looks again afterwards: another caller may have brought the new pass in meanwhile.
    for (;;) {
        const bool same = a.valid && a.trav == trav && a.o.width == o->width && a.o.height == o->height && a.o.samples_per_pixel == o->samples_per_pixel;
        if (same && !a.served[idx]) break;
        if (!same) {
            // Whole-grid passes are for a caller that walks the grid (the scheduler, render.rs:273-298).  A lone request -- a partial redraw,
            // a tool, a test -- is rendered on its own: the frame-ahead engages with the SECOND distinct bucket asked for with the same options.
            const bool seen = a.seen_idx >= 0 && a.seen_trav == trav && a.seen_o.width == o->width && a.seen_o.height == o->height &&
                              a.seen_o.samples_per_pixel == o->samples_per_pixel;
            if (!seen || a.seen_idx == (int)idx) { a.seen_o = *o; a.seen_trav = trav; a.seen_idx = (int)idx; return false; }
        }
        if (a.readers != 0) { a.cv.wait(lk); continue; }
        bool have = false;
        if (!same) {
            drain_next();                                   // a pass for other options may still be writing h_next
            a.valid = false;
            a.grid.clear(); a.off.clear();
            size_t off = 0;
            for (unsigned y = 0; y < h; y += kBucket)
                for (unsigned x = 0; x < w; x += kBucket) {
                    const rt_region r{ (uint16_t)x, (uint16_t)std::min(y + kBucket, h), (uint16_t)std::min(x + kBucket, w), (uint16_t)y };
                    a.grid.push_back(r);
                    a.off.push_back(off);
                    off += (size_t)(r.r - r.l) * (r.t - r.b) * 4;
                }
            if (a.cap < frame_bytes) {
                if (a.h) (void)rt_host_free(a.h);
                if (a.h_next) (void)rt_host_free(a.h_next);
                a.h = a.h_next = nullptr; a.cap = 0;
                void *p = nullptr, *q = nullptr;
                // whatever fails in here: the caller renders its bucket on its own (the per-bucket path needs a few MB, not two pinned frames)
                if (rt_host_alloc(frame_bytes, &p) != RT_OK) { a.valid = false; return false; }
                if (rt_host_alloc(frame_bytes, &q) != RT_OK) { (void)rt_host_free(p); a.valid = false; return false; }
                a.h = static_cast<uint8_t *>(p); a.h_next = static_cast<uint8_t *>(q); a.cap = frame_bytes;
            }
            a.o = *o; a.trav = trav;
        } else if (a.next_inflight) {
            // the pass that was started when the previous frame was first asked for
            const hipError_t e = hipEventSynchronize(a.ev);
            a.next_inflight = false;
            if (e == hipSuccess) { std::swap(a.h, a.h_next); have = true; } else (void)hipGetLastError();
        }
        if (!have) {
            // the whole grid in one pass, the kernel storing into the pinned staging (rt_host_alloc'd memory is recognised by address)
            if (render_tiles_host(s, o, trav, a.grid.data(), (uint32_t)a.grid.size(), a.h, nullptr, nullptr, true) != RT_OK) {
                a.valid = false; a.seen_idx = -1;          // e.g. out of memory for the whole grid: the bucket alone may still fit
                return false;
            }
        }
        a.served.assign(a.grid.size(), 0);
        a.valid = true;
        count_event(RT_DEBUG_COUNT_FRAME_AHEAD_PASSES);
        if (knob(RT_DEBUG_FRAME_AHEAD) != 1 && sample_bytes <= kFrameAheadMaxSampleBytes / 4) {
            // the next frame's pass, asynchronously, on a stream of its own; whatever fails here only costs the overlap
            hipError_t e = hipSuccess;
            if (!a.stream) e = hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking);
            if (e == hipSuccess && !a.ev) e = hipEventCreateWithFlags(&a.ev, hipEventDisableTiming);
            const HostDest next = classify_host_pointer(a.h_next);
            if (e == hipSuccess && next.pinned && next.dev_alias && next.room >= frame_bytes &&
                rt_render_tiles_device(s, o, trav, a.grid.data(), (uint32_t)a.grid.size(), next.dev_alias, a.stream, nullptr) == RT_OK &&
                hipEventRecord(a.ev, a.stream) == hipSuccess)
                a.next_inflight = true;
            else if (a.stream) { (void)hipStreamSynchronize(a.stream); (void)hipGetLastError(); }
        }
        break;
    }
    const uint8_t *src = a.h + a.off[idx];
    a.served[idx] = 1;
    ++a.readers;
    lk.unlock();
    memcpy(out, src, (size_t)(region->r - region->l) * (region->t - region->b) * 4);
    lk.lock();
    if (--a.readers == 0) a.cv.notify_all();
    *st = RT_OK;
    return true;
}

rt_status rt_render_region(rt_scene *s, const rt_options *o, rt_traversal trav, const rt_region *region, uint8_t *rgba_out,
                           rt_stats *stats)
{
    if (!check_common(s, o, region, 1, rgba_out)) return RT_ERR_INVALID_ARGUMENT;
    if (rt_status dst = refuse_dynamic(s, "rt_render_region"); dst != RT_OK) return dst;
    if (!stats && knob(RT_DEBUG_FRAME_AHEAD) != 0) {
        if (classify_host_pointer(rgba_out).bad) {              // the frame-ahead path copies with the CPU: same answer as rt_render_tiles gives
            snprintf(g_err, sizeof g_err, "rt_render_region: rgba_out is device memory; use rt_render_tiles_device");
            return RT_ERR_INVALID_ARGUMENT;
        }
        rt_status fst = RT_OK;
        if (region_from_frame_ahead(s, o, trav, region, rgba_out, &fst)) return fst;
    }
    if (stats || knob(RT_DEBUG_COALESCE) == 0) return render_tiles_host(s, o, trav, region, 1, rgba_out, &rgba_out, stats, false);
    // Group commit: the reference calls this from up to RTRACEMAXPROCS pool threads at once (render.rs:283-294), and one
    // 64x64 bucket per device pass would leave 255 of 256 CUs idle.  A caller that finds no pass running leads the next
    // one and renders every request waiting at that moment (same options and traversal) together; the others sleep until
    // their bytes are in their buffer.  A lone caller degenerates to one pass per call.
    rt_scene::RegionReq me;
    me.o = *o; me.trav = trav; me.region = *region; me.out = rgba_out;
    const long long k = knob(RT_DEBUG_COALESCE);
    const int max_leaders = k > 0 ? (int)std::min<long long>(k, 8) : kMaxRegionLeaders;
    std::unique_lock<std::mutex> lk(s->comb_mu);
    s->comb_pending.push_back(&me);
    while (!me.done) {
        // up to max_leaders passes at once: while one leader waits for its kernel or hands out bytes, the next batch is
        // already being set up and rendered on another stream.  Sleepers are woken one by one (their request is done, or it
        // is their turn to lead), never all at once.
        if (me.taken || s->comb_leaders >= max_leaders) { me.cv.wait(lk); continue; }
        ++s->comb_leaders;
        std::vector<rt_scene::RegionReq *> batch, rest;
        const rt_scene::RegionReq *head = s->comb_pending.front();
        for (rt_scene::RegionReq *r : s->comb_pending) {
            const bool same = r->trav == head->trav && r->o.width == head->o.width && r->o.height == head->o.height &&
                              r->o.samples_per_pixel == head->o.samples_per_pixel;
            (same ? batch : rest).push_back(r);
            if (same) r->taken = true;
        }
        s->comb_pending.swap(rest);
        lk.unlock();
        run_region_batch(s, batch);
        lk.lock();
        --s->comb_leaders;
        if (!s->comb_pending.empty()) s->comb_pending.front()->cv.notify_one();      // someone whose request is still waiting leads next
        for (rt_scene::RegionReq *r : batch) {
            r->done = true;
            if (r != &me) r->cv.notify_one();
        }
    }
    lk.unlock();
    if (me.st != RT_OK) snprintf(g_err, sizeof g_err, "%s", me.err);
    return me.st;
}


