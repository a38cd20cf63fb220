// rt_capi_launch.hpp -- part of rt_capi.hip: which kernel a pass runs (loop flavours, k_render_skip_fast, two rays per lane, the flat
// pipeline), enqueueing a pass, reading its counters.
// (included by rt_capi.hip where its text used to stand: nothing here is a header of its own)
// Variant of k_render_skip (rt_skip.hpp VAR bits): the generated assembly loops, fused where the scene allows it.
// rt_debug.h overrides it for A/B runs (read per call so one process can interleave variants, tools/ab.py); the fused bit
// is dropped for scenes that are not fused.
int skip_variant(const rt_scene *s)
{
    int v = 1 | 2 | 4 | 16;
    if (const long long o = knob(RT_DEBUG_SKIP_VARIANT); o >= 0) v = (int)o & 23;
    if (v & 2) v |= 1;                                  // the assembly loops imply the lean sqrt in what C++ remains
    if (!s->fused || !(v & 2)) v &= ~4;
    if (!s->d_xprim || !(v & 2)) v &= ~16;      // the filtered loops (f32: both walks; f64: the primary walk) need their streams
#ifdef RT_TEST_HOOKS
    if ((v & 3) == 3 && g_trace_on.load(std::memory_order_relaxed)) v |= 8;      // diagnostic build of the assembly variants
#endif
    return v;
}


// (Re)allocates the context's per-sample buffers {n.light, state} for `samples` samples of REAL size `esz`.
rt_status ensure_sample_buffers(Context *c, size_t samples, size_t esz)
{
    const size_t need = samples * esz;
    if (c->sample_cap >= need) return RT_OK;
    if (c->d_sample_gdot) HIP_TRY(hipFree(c->d_sample_gdot));
    if (c->d_sample_state) HIP_TRY(hipFree(c->d_sample_state));
    c->d_sample_gdot = nullptr; c->d_sample_state = nullptr; c->sample_cap = 0;
    HIP_TRY(hipMalloc(&c->d_sample_gdot, need));
    HIP_TRY(hipMalloc(&c->d_sample_state, samples));
    c->sample_cap = need;
    return RT_OK;
}

// rt_flat_wf.hpp: primary+shade -> shadow pass over the largest spheres -> shadow pass over the rest -> ordered resolve.
template <typename T, int CHUNK>
rt_status launch_flat_wavefront(const rt_scene *s, Context *c, hipStream_t stream, unsigned w, unsigned h, unsigned spp, const rt::TileDev *d_tab32,
                                unsigned nt, uint32_t blocks32, const rt::TileDev *d_tab16, uint32_t blocks16, uint64_t total_px, uint8_t *d_out,
                                rt::Counters *cnt, unsigned frame_w)
{
    const size_t ns = (size_t)spp * spp, samples = ns * total_px;
    if (ns > 65535 || samples > 0xFFFFFFFFull) {
        snprintf(g_err, sizeof g_err, "flat traversal: too many samples for one pass");
        return RT_ERR_INVALID_ARGUMENT;
    }
    rt_status st = ensure_sample_buffers(c, samples, sizeof(T));
    if (st != RT_OK) return st;
    const size_t qbytes = samples * sizeof(rt::Quad<T>);
    if (c->queue_cap < qbytes) {
        if (c->d_queue1) HIP_TRY(hipFree(c->d_queue1));
        if (c->d_queue2) HIP_TRY(hipFree(c->d_queue2));
        c->d_queue1 = c->d_queue2 = nullptr; c->queue_cap = 0;
        HIP_TRY(hipMalloc(&c->d_queue1, qbytes));
        HIP_TRY(hipMalloc(&c->d_queue2, qbytes));
        c->queue_cap = qbytes;
    }
    if (!c->d_queues) HIP_TRY(hipMalloc(&c->d_queues, sizeof(rt::FlatQueues)));
    HIP_TRY(hipMemsetAsync(c->d_queues, 0, sizeof(rt::FlatQueues), stream));
    rt::SampleBuf<T> sb{ static_cast<T *>(c->d_sample_gdot), c->d_sample_state, (unsigned)total_px };
    rt::Quad<T> *q1 = static_cast<rt::Quad<T> *>(c->d_queue1), *q2 = static_cast<rt::Quad<T> *>(c->d_queue2);
    const dim3 b(rt::kBlockThreads);
    if constexpr (sizeof(T) == 4) {
        if (knob(RT_DEBUG_FLAT_KERNELS) != 0) {
            // f32: the scalar-fed scan (rt_flat_sc.hpp): two rays per lane, a workgroup = two 16x16-pixel blocks of two waves each (the resolve table serves both)
            constexpr unsigned kFirstPassGroups = 342;                  // the 1,026 largest spheres (an even number of groups)
            const rt::FlatScView sv = flat_sc_view_of(s);
            const unsigned first_bytes = std::min(kFirstPassGroups * 64u, sv.n_sbytes);
            c->flat_first_pass_items = first_bytes / 64u * rt::kFlatShadowItems;
            hipLaunchKernelGGL(rt::k_flat_primary_sc, dim3((blocks16 + 1) / 2, (unsigned)ns), dim3(rt::kFlatScPrimaryThreads), 0, stream, sv, w, h, spp,
                               d_tab16, nt, blocks16, sb, q1, c->d_queues, cnt);
            HIP_TRY(hipGetLastError());
            const size_t rays_per_wg = (size_t)rt::kBlockThreads * rt::kFlatScRays;
            const dim3 gsh((unsigned)((samples + rays_per_wg - 1) / rays_per_wg));      // worst case; surplus waves leave at once
            hipLaunchKernelGGL(rt::k_flat_shadow_sc, gsh, b, 0, stream, sv, 0u, first_bytes, q1, &c->d_queues->n1, q2, &c->d_queues->n2, sb, cnt);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(rt::k_flat_shadow_sc, gsh, b, 0, stream, sv, first_bytes, 0xFFFFFF80u, q2, &c->d_queues->n2,
                               (rt::Quad<T> *)nullptr, (unsigned *)nullptr, sb, cnt);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL((rt::k_resolve_samples<T>), dim3(blocks16), b, 0, stream, sb, spp, d_tab16, nt, d_out, frame_w, false);
            return RT_OK;
        }
    }
    c->flat_first_pass_items = (unsigned)CHUNK;
    const rt::FlatView<T> view = flat_view_of<T>(s);
    if constexpr (sizeof(T) == 8) {
        if (knob(RT_DEBUG_FLAT_KERNELS) != 0) {
            // f64: the same pipeline with the conservative bound in front of the exact test (rt_flat_f64.hpp)
            const rt::FlatF64View fx = flat_f64_view_of(s);
            hipLaunchKernelGGL((rt::k_flat_primary_f64<CHUNK>), dim3(blocks32, (unsigned)ns), b, 0, stream, view, fx, w, h, spp, d_tab32, nt, sb, q1, c->d_queues, cnt);
            HIP_TRY(hipGetLastError());
            const unsigned rays_per_wg = rt::kBlockThreads * rt::kFlatR;
            const dim3 gsh((unsigned)((samples + rays_per_wg - 1) / rays_per_wg));
            hipLaunchKernelGGL((rt::k_flat_shadow_f64<CHUNK>), gsh, b, 0, stream, view, fx, 0u, (unsigned)CHUNK, q1, &c->d_queues->n1, q2, &c->d_queues->n2, sb, cnt);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL((rt::k_flat_shadow_f64<CHUNK>), gsh, b, 0, stream, view, fx, (unsigned)CHUNK, 0xFFFFFFFFu, q2, &c->d_queues->n2,
                               (rt::Quad<T> *)nullptr, (unsigned *)nullptr, sb, cnt);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL((rt::k_resolve_samples<T>), dim3(blocks16), b, 0, stream, sb, spp, d_tab16, nt, d_out, frame_w, false);
            return RT_OK;
        }
    }
#ifndef RT_TEST_HOOKS
    // (round 1's unfiltered LDS kernels, rt_flat_wf.hpp: only rt_debug.h's RT_DEBUG_FLAT_KERNELS = 0 selects them)
    (void)d_tab32; (void)blocks32; (void)view;
    snprintf(g_err, sizeof g_err, "internal: no flat-scan kernels for this precision");
    return RT_ERR_UNSUPPORTED;
#else
    hipLaunchKernelGGL((rt::k_flat_primary<T, CHUNK>), dim3(blocks32, (unsigned)ns), b, 0, stream, view, w, h, spp, d_tab32, nt, sb, q1, c->d_queues, cnt);
    HIP_TRY(hipGetLastError());
    const unsigned rays_per_block = rt::kBlockThreads * rt::kFlatR;
    const dim3 gshadow((unsigned)((samples + rays_per_block - 1) / rays_per_block));      // worst case; surplus workgroups leave at once
    hipLaunchKernelGGL((rt::k_flat_shadow<T, CHUNK>), gshadow, b, 0, stream, view, 0u, (unsigned)CHUNK, q1, &c->d_queues->n1, q2, &c->d_queues->n2, sb, cnt);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((rt::k_flat_shadow<T, CHUNK>), gshadow, b, 0, stream, view, (unsigned)CHUNK, 0xFFFFFFFFu, q2, &c->d_queues->n2,
                       (rt::Quad<T> *)nullptr, (unsigned *)nullptr, sb, cnt);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((rt::k_resolve_samples<T>), dim3(blocks16), b, 0, stream, sb, spp, d_tab16, nt, d_out, frame_w, false);
    return RT_OK;
#endif
}

// The render kernel of a hierarchy-walk launch: f32 launches that do not count run the build held to 8 waves per SIMD (rt_skip.hpp).
template <typename T, bool COUNT, int VAR, int MODE, bool COOP = false>
constexpr auto skip_kernel()
{
    if constexpr (sizeof(T) == 4 && !COUNT && COOP) return &rt::k_render_skip_f32_coop<COUNT, VAR, MODE>;
    else if constexpr (sizeof(T) == 4 && !COUNT) return &rt::k_render_skip_f32<COUNT, VAR, MODE>;
    else if constexpr (sizeof(T) == 8 && !COUNT && (VAR & 18) == 18 && COOP) return &rt::k_render_skip_f64_coop<VAR, MODE>;
    else if constexpr (sizeof(T) == 8 && !COUNT && (VAR & 18) == 18) return &rt::k_render_skip_f64<VAR, MODE>;
    else return &rt::k_render_skip<T, COUNT, VAR, MODE, COOP>;
}

// The arguments of k_render_skip2_fast (rt_skip2_fast.hpp): the two-ray kernel's, in the order it reads them
template <bool FUSED>
rt::Fast2Args fast2_args(const rt_scene *s, const rt::BlockList &order, unsigned w, unsigned h, unsigned spp, unsigned frame_w, void *dst)
{
    const rt::SkipView<float> sv = skip_view_of<float>(s);
    rt::Fast2Args a{};
    a.order = order.d; a.wg_first = order.wg_first;
    a.width = w; a.height = h; a.spp = spp;
    a.nb = (FUSED ? sv.n_fnodes : sv.n_nodes) * (unsigned)sizeof(rt::Node<float>);
    a.walk_prim = FUSED ? static_cast<const void *>(sv.xfprim) : static_cast<const void *>(sv.xprim);
    a.frame_w = frame_w;
    a.items = sv.items; a.own = sv.xown;
    a.eye[0] = sv.eye.x; a.eye[1] = sv.eye.y; a.eye[2] = sv.eye.z; a.light[0] = sv.light.x; a.light[1] = sv.light.y; a.light[2] = sv.light.z;
    a.walk_shad = FUSED ? static_cast<const void *>(sv.xfshad) : static_cast<const void *>(sv.xshad);
    a.exact_shad = FUSED ? static_cast<const void *>(sv.fshad) : static_cast<const void *>(sv.shad);
    a.fc = sv.fc;
    a.dst = dst;
    return a;
}

// Does this launch walk the scene's TIGHT streams (walks_tight_with, rt_capi_dispatch.hpp)?  A question only: whoever wants the streams
// made at the launch (RT_DEBUG_TIGHT_BOUNDS at 1 or 2: tests, tools) calls ensure_tight first -- launch_render does.
bool walks_tight(const rt_scene *s, int v, uint64_t total_px, unsigned spp) { return walks_tight_with(s, v, total_px, spp, knob(RT_DEBUG_TIGHT_BOUNDS)); }
// ... and does such a launch read the scene's PER-WALK filter streams in their places (rt_tight.hpp build_walk)?  RT_DEBUG_WALK_BOUNDS: 0 never,
// 1 the rule, 2 wherever the scene has them; default: the rule (kWalkByRule, DESIGN.md 4.1: what the A/B against the parent said).
constexpr bool kWalkByRule = true;
bool walks_per_walk(const rt_scene *s)
{
    const long long wb = knob(RT_DEBUG_WALK_BOUNDS);
    if (wb == 0 || !s->walk_ready.load(std::memory_order_acquire)) return false;
    return wb == 2 || kWalkByRule;
}

template <typename T, bool COUNT, int VAR>
rt_status launch_skip_one(const rt_scene *s, Context *c, dim3 grid, hipStream_t stream, unsigned w, unsigned h, unsigned spp,
                          const rt::TileDev *d_tab, unsigned nt, uint64_t total_px, uint8_t *d_out, rt::Counters *cnt, unsigned frame_w,
                          rt::BlockList order, [[maybe_unused]] int tight = 0)      // (skip_view_of: 0 given, 1 tight, 2 per-walk)
{
    // two rays per lane (rt_skip2.hpp): f32, fused assembly loops, launches that neither count nor trace
    bool two_rays = false;
    // (fused scenes: the fused assembly loops, filtered or not; other scenes: the filtered assembly loops over the plain streams)
    constexpr bool kTwoRayFlavour = !COUNT && sizeof(T) == 4 && ((VAR & 15) == 7 || (VAR & 31) == 19);
    if constexpr (kTwoRayFlavour) {
        const long long k = knob(RT_DEBUG_SKIP_RAYS);
        two_rays = k < 0 ? skip2_by_default(total_px, spp, (VAR & 4) ? s->n_fnodes : s->n_nodes) : k == 2;
        two_rays = two_rays && (spp == 1 || (use_split(spp) && packed_samples(spp))) && !tight;      // (walks_tight has asked the same question)
    }
    // an order with cooperative quads needs the COOP flavour of k_render_skip: everything else renders the plain order of the same list
    constexpr bool kCoopFlavour = !COUNT && (VAR == 19 || VAR == 23 || VAR == 31);       // (f32, and since round 6 f64: the filtered assembly loops)
    if (order.holes && !(kCoopFlavour && spp == 1 && !two_rays && !order.wg_first)) {
        order.d = order.plain_d; order.n = order.plain_n; order.wg_first = order.plain_wg_first; order.n_wg = order.plain_n_wg;
        order.holes = nullptr; order.n_holes = 0;
    }
    const dim3 b(rt::kBlockThreads);
    const unsigned lds = (unsigned)std::max(0ll, knob(RT_DEBUG_LDS_BYTES));
    uint32_t *no_cost = nullptr;
    // rt_debug_wave_trace(<file>) (diagnostic, tools/wave_timeline.py): the launch records every wave's start / end /
    // placement and the records are written to <file> -- synchronous, one file per launch (overwritten).
    std::string trace_file;
#ifdef RT_TEST_HOOKS
    if (VAR & 8) { std::lock_guard<std::mutex> lk(g_trace_mu); trace_file = g_trace_path; }
#endif
    const char *trace_path = trace_file.empty() ? nullptr : trace_file.c_str();
    const dim3 rgrid(order.d ? (order.wg_first ? order.n_wg : order.n) : grid.x);      // render workgroups: one per descriptor, or dealt
    const size_t trace_words = (size_t)(order.d ? order.n : grid.x) * 4 * 8 * (use_split(spp) ? (size_t)spp * spp : 1);
    struct Trace {
        uint32_t *d = nullptr; const char *path; size_t words; hipStream_t stream;
        ~Trace()
        {
            if (!d) return;
            std::vector<uint32_t> h(words);
            if (hipStreamSynchronize(stream) == hipSuccess && hipMemcpy(h.data(), d, words * 4, hipMemcpyDeviceToHost) == hipSuccess) {
                if (FILE *f = fopen(path, "wb")) { fwrite(h.data(), 4, words, f); fclose(f); }
            }
            (void)hipFree(d);
        }
    } tr{ nullptr, trace_path, trace_words, stream };
    if (trace_path && hipMalloc(&tr.d, trace_words * 4) == hipSuccess) {
        (void)hipMemsetAsync(tr.d, 0, trace_words * 4, stream);
        no_cost = tr.d;
    }
    rt::SampleBuf<T> sb{ nullptr, nullptr, (unsigned)total_px };
    const dim3 b2(rt::kSkip2Threads);
    if (!use_split(spp)) {
        if constexpr (kTwoRayFlavour) {
            if (two_rays) {
                count_event(RT_DEBUG_COUNT_TWO_RAY_LAUNCHES); g_launch_flags |= RT_LAUNCH_TWO_RAYS;
                if constexpr ((VAR & 16) != 0) {
                    if (order.d && knob(RT_DEBUG_FAST_KERNEL) != 0) {      // the same kernel with its arguments fetched where they are needed (rt_skip2_fast.hpp; spp 1: lists are not dealt)
                        g_launch_flags |= RT_LAUNCH_FAST_KERNEL;
                        hipLaunchKernelGGL((rt::k_render_skip2_fast<rt::kSkipOne, (VAR & 4) != 0>), rgrid, b2, 0, stream, fast2_args<(VAR & 4) != 0>(s, order, w, h, spp, frame_w, d_out));
                        return RT_OK;
                    }
                }
                hipLaunchKernelGGL((rt::k_render_skip2<rt::kSkipOne, (VAR & 16) != 0, (VAR & 4) != 0>), rgrid, b2, 0, stream, skip_view_of<float>(s), w, h, spp, d_tab, nt, d_out, sb, frame_w,
                                   order.d, order.wg_first);
                return RT_OK;
            }
        }
        // Steady-state frames -- f32, one sample per pixel, a dispatch list, the filtered assembly loops -- run the kernel that was written
        // around a wave's fixed costs (rt_skip_fast.hpp), with or without cooperative quads; everything else the generic one.
        if constexpr (!COUNT && sizeof(T) == 4 && ((VAR & ~8) == 19 || (VAR & ~8) == 23)) {
            // (measured, one box, interleaved -- profiles/r06_ab_fast_vs_generic.log: WITHOUT cooperative quads the lean kernel is the generic one's
            // equal, 1 - 2 % behind it at 1080p, 1 % ahead at 2560x1440 -- a wave's shorter start does not shorten a frame that is as long as its
            // longest chain, and the late batch is a round trip the generic kernel's parked values do not make --; WITH them it is 39.8 against
            // 43.5 us at 1080p and 38.4 against 40.5 at 1600x900: eight workgroups per CU where the generic cooperative flavour has seven.  So it runs
            // where a list has holes; RT_DEBUG_FAST_KERNEL = 2 forces it for every ordered f32 spp-1 launch (tests, A/B))
            const long long fk = knob(RT_DEBUG_FAST_KERNEL);
            if (spp == 1 && order.d && !order.wg_first && lds == 0 && fk != 0 && (order.holes || fk == 2)) {
                rt::FastArgs fa{};
                const rt::SkipView<float> sv = skip_view_of<float>(s, tight);
                constexpr bool kFused = (VAR & 4) != 0;
                fa.order = order.d;
                fa.walk_prim = kFused ? sv.xfprim : sv.xprim;
                fa.width = w; fa.height = h; fa.nb = (kFused ? sv.n_fnodes : sv.n_nodes) * (unsigned)sizeof(rt::Node<float>); fa.frame_w = frame_w; fa.out = d_out;
                fa.eye[0] = sv.eye.x; fa.eye[1] = sv.eye.y; fa.eye[2] = sv.eye.z; fa.light[0] = sv.light.x; fa.light[1] = sv.light.y; fa.light[2] = sv.light.z;
                fa.items = sv.items; fa.own = sv.xown; fa.walk_shad = kFused ? sv.xfshad : sv.xshad; fa.exact_shad = kFused ? sv.fshad : sv.shad;
                memcpy(fa.fc, &s->fc, sizeof fa.fc);
                fa.trace = no_cost;
                g_launch_flags |= RT_LAUNCH_FAST_KERNEL;
                if (order.holes) {
                    fa.holes = order.holes; fa.n_holes = order.n_holes; fa.cv = s->coop;
                    count_event(RT_DEBUG_COUNT_COOP_LAUNCHES); g_launch_flags |= RT_LAUNCH_COOPERATIVE;
                    hipLaunchKernelGGL((rt::k_render_skip_fast_coop<(VAR & ~8), (VAR & 8) != 0>), rgrid, b, 0, stream, fa);
                } else hipLaunchKernelGGL((rt::k_render_skip_fast<(VAR & ~8), (VAR & 8) != 0>), rgrid, b, 0, stream, fa);
                return RT_OK;
            }
        }
        // ... and the f64 twin of the lean kernel (rt_skip_fast64.hpp): 80 scalar / 61 vector registers and no scratch -- EIGHT waves per SIMD -- where
        // k_render_skip_f64 has 96 / 72 and 12 - 36 bytes (seven) and k_render_skip_f64_coop 96 vector registers (five): measured ahead of the generic
        // kernels with AND without cooperative quads (profiles/r06_f64_lean_kernel.log: 2560x1440 91.6 -> 82 us without, 1280x720 42.0 -> 34.5 with,
        // 1080p 55.2 -> 50.2), so every ordered f64 spp-1 launch takes it (RT_DEBUG_FAST_KERNEL = 0: never)
        if constexpr (!COUNT && sizeof(T) == 8 && ((VAR & ~8) == 19 || (VAR & ~8) == 23)) {
            const long long fk = knob(RT_DEBUG_FAST_KERNEL);
            if (spp == 1 && order.d && !order.wg_first && lds == 0 && fk != 0 && (!order.holes || s->coop.fanout != 0u)) {
                rt::FastArgs64 fa{};
                const rt::SkipView<double> sv = skip_view_of<double>(s);
                constexpr bool kFused = (VAR & 4) != 0;
                fa.order = order.d;
                fa.walk_prim = kFused ? sv.xfprim : sv.xprim;
                fa.exact_prim = kFused ? sv.fprim : sv.prim;
                fa.width = w; fa.height = h; fa.nbf = (kFused ? sv.n_fnodes : sv.n_nodes) * (unsigned)sizeof(rt::FNode); fa.frame_w = frame_w; fa.out = d_out;
                fa.items = sv.items; fa.own = sv.xown;
                fa.eye[0] = sv.eye.x; fa.eye[1] = sv.eye.y; fa.eye[2] = sv.eye.z; fa.light[0] = sv.light.x; fa.light[1] = sv.light.y; fa.light[2] = sv.light.z;
                fa.walk_shad = kFused ? sv.xfshad : sv.xshad; fa.exact_shad = kFused ? sv.fshad : sv.shad;
                memcpy(fa.fc, &s->fc, sizeof fa.fc);
                fa.trace = no_cost;
                fa.holes = order.holes; fa.n_holes = order.holes ? order.n_holes : 0u; fa.cv = s->coop;
                g_launch_flags |= RT_LAUNCH_FAST_KERNEL;
                if (order.holes) { count_event(RT_DEBUG_COUNT_COOP_LAUNCHES); g_launch_flags |= RT_LAUNCH_COOPERATIVE; }
                hipLaunchKernelGGL((rt::k_render_skip_fast64_coop<(VAR & ~8), (VAR & 8) != 0>), rgrid, b, 0, stream, fa);
                return RT_OK;
            }
        }
        if constexpr (!COUNT && (VAR == 19 || VAR == 23 || VAR == 31)) {
            if (spp == 1 && order.d && order.holes && !order.wg_first) {        // some quads of the pass are walked cooperatively (rt_coop.hpp)
                count_event(RT_DEBUG_COUNT_COOP_LAUNCHES); g_launch_flags |= RT_LAUNCH_COOPERATIVE;
                hipLaunchKernelGGL((skip_kernel<T, COUNT, VAR, rt::kSkipOne, true>()), rgrid, b, lds, stream, 
                                   skip_args_of<T>(s, tight, order.d, order.wg_first, w, h, frame_w, d_out, d_tab, nt, spp, cnt, no_cost, sb, s->coop, order.holes, order.n_holes));
                return RT_OK;
            }
        }
        if (spp == 1)
            hipLaunchKernelGGL((skip_kernel<T, COUNT, VAR, rt::kSkipOne>()), rgrid, b, lds, stream, 
                               skip_args_of<T>(s, tight, order.d, order.wg_first, w, h, frame_w, d_out, d_tab, nt, spp, cnt, no_cost, sb));
        else
            hipLaunchKernelGGL((skip_kernel<T, COUNT, VAR, rt::kSkipLoop>()), rgrid, b, lds, stream, 
                               skip_args_of<T>(s, tight, order.d, order.wg_first, w, h, frame_w, d_out, d_tab, nt, spp, cnt, no_cost, sb));
        return RT_OK;
    }
    const size_t ns = (size_t)spp * spp;
    {
        rt_status bst = ensure_sample_buffers(c, ns * total_px, sizeof(T));
        if (bst != RT_OK) return bst;
    }
    sb.gdot = static_cast<T *>(c->d_sample_gdot);
    sb.state = c->d_sample_state;
    const bool packed = packed_samples(spp);
    bool done2 = false;
    if constexpr (kTwoRayFlavour) {
        if (two_rays) {
            count_event(RT_DEBUG_COUNT_TWO_RAY_LAUNCHES); g_launch_flags |= RT_LAUNCH_TWO_RAYS;
            bool lean2 = false;
            if constexpr ((VAR & 16) != 0) {
                // (measured, profiles/r06_two_ray_lean_kernel.log: ahead by 2 - 8 % on the pyramid scenes -- 3840x2160 127 -> 117 us, 1080p spp 4 473 -> 458,
                // 4096^2 spp 4 L8 2.656 -> 2.608 ms; config 5 itself the same, 2.873 / 2.881 --, behind by 1.4 % on a plain-stream scene whose list is
                // dealt to workgroups on the host, several descriptors each (100,000 arbitrary spheres, 15.87 / 16.09 ms: k_render_skip2 parks its
                // arguments once per workgroup, this kernel fetches them once per descriptor): that case keeps k_render_skip2)
                if (order.d && knob(RT_DEBUG_FAST_KERNEL) != 0 && ((VAR & 4) != 0 || !order.wg_first || knob(RT_DEBUG_FAST_KERNEL) == 2)) {
                    g_launch_flags |= RT_LAUNCH_FAST_KERNEL;
                    hipLaunchKernelGGL((rt::k_render_skip2_fast<rt::kSkipPacked, (VAR & 4) != 0>), dim3(rgrid.x, (unsigned)ns), b2, 0, stream,
                                       fast2_args<(VAR & 4) != 0>(s, order, w, h, spp, frame_w, sb.gdot));
                    lean2 = true;
                }
            }
            if (!lean2)
            hipLaunchKernelGGL((rt::k_render_skip2<rt::kSkipPacked, (VAR & 16) != 0, (VAR & 4) != 0>), dim3(rgrid.x, (unsigned)ns), b2, 0, stream, skip_view_of<float>(s), w, h, spp, d_tab, nt,
                               d_out, sb, frame_w, order.d, order.wg_first);
            done2 = true;
        }
    }
    if (done2) {
    } else if (packed)
        hipLaunchKernelGGL((skip_kernel<T, COUNT, VAR, rt::kSkipPacked>()), dim3(rgrid.x, (unsigned)ns), b, lds, stream, 
                           skip_args_of<T>(s, tight, order.d, order.wg_first, w, h, frame_w, d_out, d_tab, nt, spp, cnt, no_cost, sb));
    else
        hipLaunchKernelGGL((skip_kernel<T, COUNT, VAR, rt::kSkipSplit>()), dim3(rgrid.x, (unsigned)ns), b, lds, stream, 
                           skip_args_of<T>(s, tight, order.d, order.wg_first, w, h, frame_w, d_out, d_tab, nt, spp, cnt, no_cost, sb));
    HIP_TRY(hipGetLastError());
    if constexpr (sizeof(T) == 4) {
        if (packed) {        // one word per sample, [pixel][sample] (rt_kernels.hpp sample_word)
            const uint4 *words = reinterpret_cast<const uint4 *>(sb.gdot);
            if (ns == 4) hipLaunchKernelGGL((rt::k_resolve_words<4>), grid, b, 0, stream, words, d_tab, nt, d_out, frame_w);
            else if (ns == 16) hipLaunchKernelGGL((rt::k_resolve_words<16>), grid, b, 0, stream, words, d_tab, nt, d_out, frame_w);
            else hipLaunchKernelGGL((rt::k_resolve_words<64>), grid, b, 0, stream, words, d_tab, nt, d_out, frame_w);
            return RT_OK;
        }
    }
    hipLaunchKernelGGL((rt::k_resolve_samples<T>), grid, b, 0, stream, sb, spp, d_tab, nt, d_out, frame_w, packed);
    return RT_OK;
}

template <typename T, bool COUNT>
rt_status launch_skip_var(const rt_scene *s, Context *c, dim3 grid, hipStream_t stream, unsigned w, unsigned h, unsigned spp,
                          const rt::TileDev *d_tab, unsigned nt, uint64_t total_px, uint8_t *d_out, rt::Counters *cnt, unsigned frame_w,
                          rt::BlockList order)
{
    // a counting launch always runs the C++ loops: the assembly bits would only duplicate kernels
    const int v = skip_variant(s);
    if constexpr (COUNT) {
#ifdef RT_TEST_HOOKS
        if (!(v & 1)) return launch_skip_one<T, true, 0>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
#endif
        return launch_skip_one<T, true, 1>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
    } else {
        if constexpr (sizeof(T) == 4) {
            if (walks_tight(s, v, total_px, spp)) {
                g_launch_flags |= RT_LAUNCH_TIGHT_BOUNDS;
                if (order.d && order.tight_costs) g_launch_flags |= RT_LAUNCH_TIGHT_COSTS;
                const int streams = walks_per_walk(s) ? 2 : 1;          // (skip_view_of: the tight streams, or the per-walk filter streams over them)
                if (streams == 2) g_launch_flags |= RT_LAUNCH_WALK_BOUNDS;
                if (streams == 2 && s->walk_lean) g_launch_flags |= RT_LAUNCH_LEAN_BOUNDS;      // (the flag is data: the loops take the lean step where a node says so)
#ifdef RT_TEST_HOOKS
                if (v & 8) return launch_skip_one<T, false, 27>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order, streams);
#endif
                return launch_skip_one<T, false, 19>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order, streams);
            }
        }
        switch (v) {
        // what a scene gets by itself: the filtered assembly loops, fused where the scene is concentric (f64 scenes too large for the
        // filter streams' 32-bit offsets: the unfiltered ones)
        case 19: return launch_skip_one<T, false, 19>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
        case 23: return launch_skip_one<T, false, 23>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
        case 3: if constexpr (sizeof(T) == 8) return launch_skip_one<T, false, 3>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order); else break;
        case 7: if constexpr (sizeof(T) == 8) return launch_skip_one<T, false, 7>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order); else break;
#ifdef RT_TEST_HOOKS
        // flavours only rt_debug.h's RT_DEBUG_SKIP_VARIANT / rt_debug_wave_trace can ask for
        case 0: return launch_skip_one<T, false, 0>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
        case 27: if constexpr (sizeof(T) == 4) return launch_skip_one<T, false, 27>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order); else break;
        case 31: if constexpr (sizeof(T) == 4) return launch_skip_one<T, false, 31>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order); else break;
        case 11: return launch_skip_one<T, false, 11>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
        case 15: return launch_skip_one<T, false, 15>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
#endif
        default: break;
        }
#ifdef RT_TEST_HOOKS
        if constexpr (sizeof(T) == 4) {
            if (v == 3) return launch_skip_one<T, false, 3>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
            if (v == 7) return launch_skip_one<T, false, 7>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
        }
        return launch_skip_one<T, false, 1>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
#else
        snprintf(g_err, sizeof g_err, "internal: no traversal loops for variant %d", v);      // (skip_variant cannot return anything else without a control)
        return RT_ERR_UNSUPPORTED;
#endif
    }
}

rt_status launch_skip(const rt_scene *s, Context *c, dim3 grid, hipStream_t stream, unsigned w, unsigned h, unsigned spp,
                      const rt::TileDev *d_tab, unsigned nt, uint64_t total_px, uint8_t *d_out, rt::Counters *cnt, unsigned frame_w,
                      rt::BlockList order)
{
    if (s->precision == RT_F32)
        return cnt ? launch_skip_var<float, true>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order)
                   : launch_skip_var<float, false>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
    return cnt ? launch_skip_var<double, true>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order)
               : launch_skip_var<double, false>(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
}

rt_status ensure_flat(rt_scene *s)
{
    if (rt_status dst = refuse_dynamic(s, "the flat scan"); dst != RT_OK) return dst;
    std::lock_guard<std::mutex> lk(s->flat_mu);
    if (s->flat_ready) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    rt_status st = s->precision == RT_F32 ? upload_flat<float>(s, s->h_items.data()) : upload_flat<double>(s, s->h_items.data());
    if (st != RT_OK) {
        // a later call tries again from nothing: what this attempt had already allocated goes back (nothing was launched against it
        // that has not been waited for: the failing call was an allocation, a launch or the synchronise itself)
        (void)hipDeviceSynchronize(); (void)hipGetLastError();
        for (void **p : { &s->d_fprim, &s->d_fprim_rr, &s->d_fshad, &s->d_pf, &s->d_pe, &s->d_sg, &s->d_se, &s->d_f64_pf, &s->d_f64_sf, &s->d_f64_sg })
            if (*p) { (void)hipFree(*p); *p = nullptr; }
        return st;
    }
    s->flat_ready = true;
    std::vector<unsigned char>().swap(s->h_items);
    return RT_OK;
}

rt_status check_traversal(rt_scene *s, rt_traversal trav)
{
    if (trav != RT_TRAVERSAL_FLAT && trav != RT_TRAVERSAL_SKIP) {
        snprintf(g_err, sizeof g_err, "unknown traversal %d", (int)trav);
        return RT_ERR_INVALID_ARGUMENT;
    }
    if (rt_status dst = refuse_dynamic(s, "rt_render_tiles / rt_render_frame"); dst != RT_OK) return dst;
    if (trav == RT_TRAVERSAL_FLAT) return ensure_flat(s);
    if (trav == RT_TRAVERSAL_SKIP && s->n_nodes == 0) {
        snprintf(g_err, sizeof g_err, "the hierarchy (skip) traversal needs a scene created with subtree bounds");
        return RT_ERR_UNSUPPORTED;
    }
    return RT_OK;
}

// The render kernels of one pass.  c may be NULL when the pass needs no per-call device state (no counters, no
// sample buffers): then nothing but the kernel itself is enqueued.
rt_status launch_render(rt_scene *s, Context *c, const rt_options *o, rt_traversal trav, const rt::TileDev *d_tab, unsigned nt,
                        uint32_t total_blocks, uint64_t total_px, uint8_t *d_out, unsigned frame_w, hipStream_t stream, rt::Counters *cnt,
                        const rt::TileDev *d_tab16 = nullptr, uint32_t blocks16 = 0, rt::BlockList order = rt::BlockList{})
{
    const dim3 grid(total_blocks);
    const unsigned w = o->width, h = o->height, spp = o->samples_per_pixel;
    // RT_DEBUG_TIGHT_BOUNDS 1 / 2 (tests, tools): the tight streams are made here and now if the scene's worker has not made them yet
    if (trav == RT_TRAVERSAL_SKIP && !cnt && knob(RT_DEBUG_TIGHT_BOUNDS) >= 1) (void)ensure_tight(s);
    // ... and RT_DEBUG_WALK_BOUNDS 1 / 2 the per-walk streams over them
    if (trav == RT_TRAVERSAL_SKIP && !cnt && knob(RT_DEBUG_WALK_BOUNDS) >= 1 && knob(RT_DEBUG_TIGHT_BOUNDS) != 0 && ensure_tight(s)) (void)ensure_walk(s);
    if (spp == 0) {
        // render.rs:219-250 with no sample to take: 0 * inf = NaN in every channel, and `NaN as u8` is 0 (set_pixel_from_vector, render.rs:96-108)
        g_launch_flags = cnt ? RT_LAUNCH_COUNTING : 0u;
        if (frame_w == 0) HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)total_px * 4, stream));
        else hipLaunchKernelGGL(rt::k_zero_tiles, dim3(nt), dim3(rt::kBlockThreads), 0, stream, frame_w, d_tab, reinterpret_cast<unsigned *>(d_out));
        HIP_TRY(hipGetLastError());
        return RT_OK;
    }
    g_launch_flags = (trav == RT_TRAVERSAL_FLAT ? RT_LAUNCH_FLAT_PIPELINE : 0u) | (order.d ? RT_LAUNCH_ORDERED : 0u) |
                     (trav == RT_TRAVERSAL_SKIP && use_split(spp) ? RT_LAUNCH_SAMPLE_PARALLEL : 0u) | (cnt ? RT_LAUNCH_COUNTING : 0u);
    // a dispatch order that is being timed against others (pick_order); never a counting launch: its loops are different ones
    const bool timed = order.ev0 && order.ev1 && !cnt && trav == RT_TRAVERSAL_SKIP;
    if (timed) HIP_TRY(hipEventRecord(order.ev0, stream));
    struct Stop { hipEvent_t e; hipStream_t s; ~Stop() { if (e) (void)hipEventRecord(e, s); } } stop{ timed ? order.ev1 : nullptr, stream };
    if (trav == RT_TRAVERSAL_FLAT && d_tab16) {                     // wavefront pipeline (needs a context and the 16x16 table)
        rt_status fst = s->precision == RT_F32
            ? launch_flat_wavefront<float, 1024>(s, c, stream, w, h, spp, d_tab, nt, total_blocks, d_tab16, blocks16, total_px, d_out, cnt, frame_w)
            : launch_flat_wavefront<double, 512>(s, c, stream, w, h, spp, d_tab, nt, total_blocks, d_tab16, blocks16, total_px, d_out, cnt, frame_w);
        if (fst != RT_OK) return fst;
    } else if (trav == RT_TRAVERSAL_FLAT) {
        snprintf(g_err, sizeof g_err, "flat traversal launched without its resolve table");
        return RT_ERR_INVALID_ARGUMENT;
    } else {
        rt_status lst = launch_skip(s, c, grid, stream, w, h, spp, d_tab, nt, total_px, d_out, cnt, frame_w, order);
        if (lst != RT_OK) return lst;
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// Enqueues every kernel of one pass on `stream` through a leased context.  d_out must hold 4 * total_px bytes
// (tile-major) or the whole frame (frame_w != 0).
rt_status enqueue_pass(rt_scene *s, Context *c, const rt_options *o, rt_traversal trav, const std::vector<rt::TileDev> &tab,
                       uint32_t total_blocks, uint64_t total_px, uint8_t *d_out, unsigned frame_w, hipStream_t stream, bool want_counters,
                       const std::vector<rt::TileDev> *tab16 = nullptr, uint32_t blocks16 = 0, bool cacheable = true,
                       const rt::TileDev **d_tab_out = nullptr)       // the device copy of `tab` the pass was launched with
{
    const rt::TileDev *d_tab = nullptr, *d_tab16 = nullptr;
    rt::BlockList order;
    {
        // (will_be_timed: launch_render records the trial's event pair -- a pass without samples launches nothing and records none)
        rt_status ust = trav == RT_TRAVERSAL_SKIP ? device_table(s, c, tab, stream, &d_tab, 0, o, &order, cacheable, !want_counters && o->samples_per_pixel != 0)
                                                  : device_table(s, c, tab, stream, &d_tab, 0, nullptr, nullptr, cacheable);
        if (ust != RT_OK) return ust;
        if (tab16) {
            if ((ust = device_table(s, c, *tab16, stream, &d_tab16, 1, nullptr, nullptr, cacheable)) != RT_OK) return ust;
        }
        if (d_tab_out) *d_tab_out = d_tab;
    }
    if (want_counters) {
        HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof(rt::Counters) * rt::kCounterStripes, stream));
        HIP_TRY(hipEventRecord(c->ev0, stream));
    }
    rt_status st = launch_render(s, c, o, trav, d_tab, (unsigned)tab.size(), total_blocks, total_px, d_out, frame_w, stream,
                                 want_counters ? c->d_counters : nullptr, d_tab16, blocks16, order);
    if (st != RT_OK) return st;
    HIP_TRY(hipEventRecord(c->ev1, stream));
    return RT_OK;
}

rt_status read_stats(rt_scene *s, Context *c, hipStream_t stream, rt_traversal trav, rt_stats *st)
{
    std::vector<rt::Counters> stripes(rt::kCounterStripes);
    HIP_TRY(hipMemcpyAsync(stripes.data(), c->d_counters, sizeof(rt::Counters) * rt::kCounterStripes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    rt::Counters h{};
    for (const rt::Counters &k : stripes) {
        h.primary += k.primary; h.hits += k.hits; h.shadow += k.shadow; h.occluded += k.occluded;
        h.sphere_tests += k.sphere_tests; h.bound_tests += k.bound_tests; h.wave_steps += k.wave_steps;
        h.max_wave_steps = std::max(h.max_wave_steps, k.max_wave_steps);
        h.max_wave_cycles = std::max(h.max_wave_cycles, k.max_wave_cycles);
        h.max_wave_ref100mhz = std::max(h.max_wave_ref100mhz, k.max_wave_ref100mhz);
        h.wave_item_steps += k.wave_item_steps;
        h.filter_pass += k.filter_pass; h.filter_violations += k.filter_violations; h.primary_tests += k.primary_tests;
        h.tight_violations += k.tight_violations;
    }
    count_event(RT_DEBUG_COUNT_FILTER_PASS, (long long)h.filter_pass);
    // (a tight-stream violation is a bound's verdict violated like the others: it counts there too, so that whoever asserts that counter asserts this one)
    count_event(RT_DEBUG_COUNT_FILTER_VIOLATIONS, (long long)(h.filter_violations + h.tight_violations));
    count_event(RT_DEBUG_COUNT_TIGHT_VIOLATIONS, (long long)h.tight_violations);
    count_store(RT_DEBUG_COUNT_PRIMARY_TESTS, (long long)h.primary_tests);
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    st->primary = h.primary; st->hits = h.hits; st->shadow = h.shadow; st->occluded = h.occluded;
    st->primary_tests = trav == RT_TRAVERSAL_FLAT ? h.primary * (uint64_t)s->n_items : h.primary_tests;
    if (trav == RT_TRAVERSAL_FLAT) {
        st->sphere_tests = (h.primary + h.shadow) * (uint64_t)s->n_items;
        st->bound_tests = 0;
        st->tests_executed = st->sphere_tests;
        if (c->d_queues) {                                          // the shadow queues' lengths say what actually ran
            rt::FlatQueues q{};
            HIP_TRY(hipMemcpy(&q, c->d_queues, sizeof q, hipMemcpyDeviceToHost));
            const uint64_t chunk = c->flat_first_pass_items, n = s->n_items;
            st->tests_executed = h.primary * n + (uint64_t)q.n1 * std::min<uint64_t>(chunk, n) + (uint64_t)q.n2 * (n > chunk ? n - chunk : 0);
        }
    } else {
        st->sphere_tests = h.sphere_tests; st->bound_tests = h.bound_tests;
        st->tests_executed = h.sphere_tests + h.bound_tests;
    }
    if (knob(RT_DEBUG_PRINT_STEPS) > 0)
        fprintf(stderr, "[rtrace_hip] wave_steps %llu (%llu at ITEM nodes) max_wave_steps %llu longest wave: %llu cycles, %.2f us, %.0f MHz\n",
                h.wave_steps, h.wave_item_steps, h.max_wave_steps, h.max_wave_cycles, h.max_wave_ref100mhz / 100.0,
                h.max_wave_ref100mhz ? 100.0 * h.max_wave_cycles / h.max_wave_ref100mhz : 0.0);
    st->device_ms = ms;
    st->longest_wave_cycles = trav == RT_TRAVERSAL_FLAT ? 0 : h.max_wave_cycles; st->longest_wave_ref100mhz = trav == RT_TRAVERSAL_FLAT ? 0 : h.max_wave_ref100mhz;
    return RT_OK;
}

bool check_common(rt_scene *s, const rt_options *o, const rt_region *tiles, uint32_t n, const void *out)
{
    if (!s || !o || !tiles || !out || n == 0) { snprintf(g_err, sizeof g_err, "NULL argument or n_tiles == 0"); return false; }
    if (o->width == 0 || o->height == 0) {       // (samples_per_pixel == 0 is the reference's black frame: launch_render)
        snprintf(g_err, sizeof g_err, "width and height must be >= 1");
        return false;
    }
    return true;
}

template <typename T>
bool items_valid(const void *p, uint32_t n, bool need_positive_radius)
{
    const T *v = static_cast<const T *>(p);
    for (uint64_t i = 0; i < (uint64_t)n * 4; ++i) {
        if (!std::isfinite(v[i]) || std::fabs((double)v[i]) > 1e15) return false;
        if (need_positive_radius && (i & 3) == 3 && !(v[i] > T(0))) return false;
    }
    return true;
}

// ... over the live slots alone (rt_scene_update_live): a dead slot may hold any bits
template <typename T>
bool live_items_valid(const void *items, const uint8_t *live, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i)
        if (live[i] && !items_valid<T>(static_cast<const T *>(items) + 4 * (size_t)i, 1, true)) return false;
    return true;
}

// ---- what the queries' checks and launches share: one precision switch, one flavour switch, one alignment check, three
// domain predicates.  A query brings its argument struct, its NULL / mode / capacity rules, its table of pointers, its composition of the
// predicates and one launch lambda per kernel ----

inline size_t real_size(const rt_scene *s) { return s->precision == RT_F32 ? sizeof(float) : sizeof(double); }

// The precision switch: f(float{}) or f(double{}) by the scene's REAL, and what it returns.  Inside, `using T = decltype(real)`.
template <typename F>
auto by_precision(const rt_scene *s, F &&f) { return s->precision == RT_F32 ? f(float{}) : f(double{}); }

// The flavour switch: runtime flags as template arguments.  with_flags(f, a, b) calls f(std::bool_constant<a>{}, std::bool_constant<b>{});
// a generic lambda that launches kernel<T, a(), b()> is instantiated for every combination of its flags.  So this is for kernels that
// exist in every combination: where only some do (the list queries' <COUNT, false> and <false, true>), spell those.
template <typename F>
void with_flags(F &&f) { f(); }
template <typename F, typename... Rest>
void with_flags(F &&f, bool first, Rest... rest)
{
    if (first) with_flags([&](auto... r) { f(std::true_type{}, r...); }, rest...);
    else with_flags([&](auto... r) { f(std::false_type{}, r...); }, rest...);
}

// ... and the capacity of a k-list kernel's lists: f(std::integral_constant<int, B>{}), B the smallest bucket >= k
// (RT_DEBUG_MULTIHIT_BUCKET: a larger one).
template <typename F>
void with_list_bucket(uint32_t k, F &&f)
{
    static_assert(sizeof rt::kMultiBuckets == 4 * sizeof(unsigned) && rt::kMultiBuckets[3] == 16u, "the cases below are rt::kMultiBuckets");
    unsigned bucket = 0;
    for (unsigned b : rt::kMultiBuckets)
        if (bucket == 0 && b >= k) bucket = b;
    const long long forced = knob(RT_DEBUG_MULTIHIT_BUCKET);
    for (unsigned b : rt::kMultiBuckets)
        if (forced == (long long)b && b >= k) bucket = b;
    switch (bucket) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
    }
}

// One thread per query, in blocks of rt::kBlockThreads.
inline dim3 query_grid(uint32_t n) { return dim3((unsigned)(((uint64_t)n + rt::kBlockThreads - 1) / rt::kBlockThreads)); }
inline dim3 query_block() { return dim3(rt::kBlockThreads); }

// The alignment check: the first pointer of the table that is not `alignment`-byte aligned is named (NULL is aligned).
struct NamedPointer { const void *p; const char *name; };
bool aligned_ok(const char *what, size_t alignment, std::initializer_list<NamedPointer> table)
{
    for (const NamedPointer &x : table)
        if ((reinterpret_cast<uintptr_t>(x.p) % alignment) != 0) {
            snprintf(g_err, sizeof g_err, "%s: %s must be %u-byte aligned", what, x.name, (unsigned)alignment);
            return false;
        }
    return true;
}

// The domain predicates of the host entries, each for element i of a REAL array, with the variable parts of its message passed in.  A
// query's *_valid composes them element by element (each_valid): of two violations the one at the lower index is reported.
// 1. a ray {pos, dir}: finite, |pos| <= 1e15 and a unit direction (squared length within 2e-3 of 1) -- the bounds rt_scene_create puts on
//    the light and the eye: no intermediate of the walk overflows.  `infix`: what stands between `what` and ": ray i"
template <typename T>
bool ray_ok(const T *rays, uint32_t i, const char *what, const char *infix)
{
    const T *r = rays + 6 * (size_t)i;
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(r[k]) || (k < 3 && std::fabs((double)r[k]) > 1e15)) {
            snprintf(g_err, sizeof g_err, "%s%s: ray %u has a non-finite component or |pos| > 1e15", what, infix, i);
            return false;
        }
    const double d2 = (double)r[3] * r[3] + (double)r[4] * r[4] + (double)r[5] * r[5];
    if (std::fabs(d2 - 1.0) > 2e-3) {
        snprintf(g_err, sizeof g_err, "%s%s: ray %u's direction is not a unit vector (its squared length is %.6g)", what, infix, i, d2);
        return false;
    }
    return true;
}

// ... with a tmax that is not NaN; a proximity radius is held to no more.  v == NULL: none was given
template <typename T>
bool not_nan_ok(const T *v, uint32_t i, const char *what, const char *name)
{
    if (v && std::isnan(v[i])) { snprintf(g_err, sizeof g_err, "%s: %s[%u] is NaN", what, name, i); return false; }
    return true;
}

// 2. a triple: every component finite and within +-1e15, the scene's own bound on a length (vv stays finite).  `subject`, `noun`: "point"
//    and "coordinate", "disp of slot" and "component"
template <typename T>
bool triple_ok(const T *v, uint32_t i, const char *what, const char *subject, const char *noun)
{
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(v[c]) || std::fabs((double)v[c]) > 1e15) {
            snprintf(g_err, sizeof g_err, "%s: %s %u has a non-finite %s or one beyond +-1e15", what, subject, i, noun);
            return false;
        }
    return true;
}

// 3. a radius in 0 .. 1e15, the scene's own bound on a radius: no intermediate of the inflated test overflows.  `before`, `after`: what
//    stands around i, "radius[" and "] =" or "query " and "'s radius"
template <typename T>
bool radius_ok(T r, uint32_t i, const char *what, const char *before, const char *after)
{
    if (!(r >= T(0.0) && (double)r <= 1e15)) {                     // (NaN fails the first comparison)
        snprintf(g_err, sizeof g_err, "%s: %s%u%s %g is not in 0 .. 1e15", what, before, i, after, (double)r);
        return false;
    }
    return true;
}

// ok(real, i) for every element 0 .. n-1, in the scene's REAL
template <typename F>
bool each_valid(const rt_scene *s, uint32_t n, F &&ok)
{
    return by_precision(s, [&](auto real) {
        for (uint32_t i = 0; i < n; ++i)
            if (!ok(real, i)) return false;
        return true;
    });
}

// ---- ray queries (rt_intersect_rays*, rt_query.hpp) ----

// The stream a ray query walks: the scene's plain per-origin stream, or -- for a scene created without bounds -- its items as a stream of
// ITEM nodes, derived by the first query on that query's own stream (no other caller's work is waited for).  Until the derivation's
// event has completed, every later query makes its stream wait for it.
rt_status query_stream(rt_scene *s, hipStream_t stream, const void **nodes, uint32_t *n_nodes)
{
    if (s->n_nodes) { *nodes = s->d_shad; *n_nodes = s->n_nodes; return RT_OK; }
    std::lock_guard<std::mutex> lk(s->query_mu);
    if (!s->d_query_items) {
        const bool f32 = s->precision == RT_F32;
        const unsigned total = s->n_items + rt::kNodePad;
        void *p = nullptr;
        hipEvent_t ev = nullptr;
        HIP_TRY(hipMalloc(&p, (f32 ? sizeof(rt::Node<float>) : sizeof(rt::Node<double>)) * total));
        hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) {
            by_precision(s, [&](auto real) {
                using T = decltype(real);
                hipLaunchKernelGGL(rt::k_items_stream<T>, dim3((total + 255) / 256), dim3(256), 0, stream, static_cast<const rt::Item<T> *>(s->d_items), s->n_items,
                                   static_cast<rt::Node<T> *>(p));
            });
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ev, stream);
        if (e != hipSuccess) {
            if (ev) (void)hipEventDestroy(ev);
            (void)hipStreamSynchronize(stream);          // (a launched derivation must not write freed memory)
            (void)hipFree(p);
            return hip_fail(e, "k_items_stream", __LINE__);
        }
        s->d_query_items = p; s->query_items_ev = ev;
    } else if (s->query_items_ev) {
        const hipError_t q = hipEventQuery(s->query_items_ev);
        if (q == hipSuccess) { (void)hipEventDestroy(s->query_items_ev); s->query_items_ev = nullptr; }
        else {
            (void)hipGetLastError();
            HIP_TRY(hipStreamWaitEvent(stream, s->query_items_ev, 0));
        }
    }
    *nodes = s->d_query_items; *n_nodes = s->n_items;
    return RT_OK;
}

// Pointers and sizes every query entry checks (device pointers are not dereferenced here).
bool query_args_ok(const rt_scene *s, rt_query mode, const void *rays, const void *tmax, uint32_t n, const void *dist, const void *normal, const int32_t *item,
                   const char *what)
{
    if (!s || !rays || !dist || n == 0 || (mode != RT_QUERY_NEAREST && mode != RT_QUERY_ANY)) {
        snprintf(g_err, sizeof g_err, "%s: NULL scene, rays or distance_out, n == 0 or unknown mode", what);
        return false;
    }
    return aligned_ok(what, real_size(s), { { rays, "REAL buffers" }, { tmax, "REAL buffers" }, { dist, "REAL buffers" }, { normal, "REAL buffers" } })
           && aligned_ok(what, 4, { { item, "item_out" } });
}

// The host entry's domain: rays, and a tmax that is not NaN.  (The multi-hit, trace and order entries share it, message and all.)
bool query_rays_valid(const rt_scene *s, const void *rays, const void *tmax, uint32_t n)
{
    return each_valid(s, n, [&](auto real, uint32_t i) {
        using T = decltype(real);
        return ray_ok(static_cast<const T *>(rays), i, "rt_intersect_rays", "") && not_nan_ok(static_cast<const T *>(tmax), i, "rt_intersect_rays", "tmax");
    });
}

// One query launch on `stream`: counters != NULL runs the counting flavour (same bytes); with an order, the rays in that order
// (rt_order.hpp): the same walk, ray order[j] in lane j.
rt_status enqueue_query(const rt_scene *s, const void *nodes, uint32_t n_nodes, rt_query mode, const void *rays, const void *tmax, uint32_t n,
                        void *dist, void *normal, int32_t *item, rt::Counters *counters, hipStream_t stream, const uint32_t *order = nullptr)
{
    by_precision(s, [&](auto real) {
        using T = decltype(real);
        const rt::QueryArgs<T> a{ static_cast<const rt::Node<T> *>(nodes), static_cast<const rt::Item<T> *>(s->d_items), static_cast<const T *>(rays),
                                  static_cast<const T *>(tmax), static_cast<T *>(dist), static_cast<T *>(normal), item, counters, n_nodes, n };
        with_flags([&](auto count, auto any, auto ordered) {
            if constexpr (ordered()) hipLaunchKernelGGL((rt::k_query_rays_ordered<T, count(), any()>), query_grid(n), query_block(), 0, stream, a, order);
            else hipLaunchKernelGGL((rt::k_query_rays<T, count(), any()>), query_grid(n), query_block(), 0, stream, a);
        }, counters != nullptr, mode == RT_QUERY_ANY, order != nullptr);
    });
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// A counting call's counters, their stripes summed into *h, and what every query reports of them in *st: primary = rays, hits = results
// below tmax, the tests, the interval; every other field 0.  Synchronises `stream`.
rt_status read_counters(Context *c, hipStream_t stream, rt::Counters *h, rt_stats *st)
{
    std::vector<rt::Counters> stripes(rt::kCounterStripes);
    HIP_TRY(hipMemcpyAsync(stripes.data(), c->d_counters, sizeof(rt::Counters) * rt::kCounterStripes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *h = rt::Counters{};
    for (const rt::Counters &k : stripes) {
        h->primary += k.primary; h->hits += k.hits; h->shadow += k.shadow; h->occluded += k.occluded;
        h->sphere_tests += k.sphere_tests; h->bound_tests += k.bound_tests; h->primary_tests += k.primary_tests;
    }
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *st = rt_stats{};
    st->primary = h->primary; st->hits = h->hits;
    st->sphere_tests = h->sphere_tests; st->bound_tests = h->bound_tests; st->tests_executed = h->sphere_tests + h->bound_tests;
    st->device_ms = ms;
    return RT_OK;
}

rt_status read_query_stats(Context *c, hipStream_t stream, rt_stats *st)
{
    rt::Counters h;
    return read_counters(c, stream, &h, st);
}

// ---- multi-hit ray queries (rt_intersect_rays_multi*, rt_multihit.hpp) ----

// What both multi-hit entries check besides query_args_ok: k, the mode and hits_out's alignment.
bool multihit_args_ok(rt_multihit mode, uint32_t k, const uint32_t *hits, const char *what)
{
    if (k == 0 || k > RT_MULTIHIT_MAX_K || (mode != RT_MULTIHIT_CLOSEST && mode != RT_MULTIHIT_ALL)) {
        snprintf(g_err, sizeof g_err, "%s: k must be 1 .. %d and the mode closest (0) or all (1)", what, RT_MULTIHIT_MAX_K);
        return false;
    }
    return aligned_ok(what, 4, { { hits, "hits_out" } });
}

// One multi-hit launch on `stream`: the list capacity is the smallest bucket >= k; counters != NULL runs the counting flavour (same
// bytes); with an order, the rays in that order (rt_order.hpp).
rt_status enqueue_multihit(const rt_scene *s, const void *nodes, uint32_t n_nodes, rt_multihit mode, uint32_t k, const void *rays, const void *tmax,
                           uint32_t n, void *dist, void *normal, int32_t *item, uint32_t *hits, rt::Counters *counters, hipStream_t stream,
                           const uint32_t *order = nullptr)
{
    by_precision(s, [&](auto real) {
        using T = decltype(real);
        const rt::MultiArgs<T> a{ static_cast<const rt::Node<T> *>(nodes), static_cast<const rt::Item<T> *>(s->d_items), static_cast<const T *>(rays),
                                  static_cast<const T *>(tmax), static_cast<T *>(dist), static_cast<T *>(normal), item, hits, counters, n_nodes, n, k };
        with_list_bucket(k, [&](auto bucket) {
            constexpr int B = bucket();
            with_flags([&](auto count, auto all, auto ordered) {
                if constexpr (ordered()) hipLaunchKernelGGL((rt::k_multihit_rays_ordered<T, count(), all(), B>), query_grid(n), query_block(), 0, stream, a, order);
                else hipLaunchKernelGGL((rt::k_multihit_rays<T, count(), all(), B>), query_grid(n), query_block(), 0, stream, a);
            }, counters != nullptr, mode == RT_MULTIHIT_ALL, order != nullptr);
        });
    });
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- proximity queries (rt_near_spheres*, rt_near.hpp) ----

// What both proximity entries check (device pointers are not dereferenced here).
bool near_args_ok(const rt_scene *s, rt_near mode, uint32_t k, const void *points, const void *radius, uint32_t n, const int32_t *exclude,
                  const uint32_t *order, const void *gap, const int32_t *item, const uint32_t *found, const char *what)
{
    if (!s || !points || !gap || n == 0) { snprintf(g_err, sizeof g_err, "%s: NULL scene, points or gap_out, or n == 0", what); return false; }
    if (k == 0 || k > RT_NEAR_MAX_K) { snprintf(g_err, sizeof g_err, "%s: k must be 1 .. %d, not %u", what, RT_NEAR_MAX_K, k); return false; }
    if (mode != RT_NEAR_CLOSEST && mode != RT_NEAR_ALL) { snprintf(g_err, sizeof g_err, "%s: unknown mode %d (closest is 0, all is 1)", what, (int)mode); return false; }
    return aligned_ok(what, 4, { { item, "item_out" }, { found, "found_out" }, { exclude, "exclude" }, { order, "order" } })
           && aligned_ok(what, real_size(s), { { points, "REAL buffers" }, { radius, "REAL buffers" }, { gap, "REAL buffers" } });
}

// The host entry's domain: points, and a radius that is not NaN.
bool near_points_valid(const rt_scene *s, const void *points, const void *radius, uint32_t n, const char *what)
{
    return each_valid(s, n, [&](auto real, uint32_t i) {
        using T = decltype(real);
        return triple_ok(static_cast<const T *>(points) + 3 * (size_t)i, i, what, "point", "coordinate") && not_nan_ok(static_cast<const T *>(radius), i, what, "radius");
    });
}

// One proximity launch on `stream`: the list capacity as for the multi-hit lists; counters != NULL runs the counting flavour (same bytes).
rt_status enqueue_near(const rt_scene *s, const void *nodes, uint32_t n_nodes, rt_near mode, uint32_t k, const void *points, const void *radius, uint32_t n,
                       const int32_t *exclude, const uint32_t *order, void *gap, int32_t *item, uint32_t *found, rt::Counters *counters, hipStream_t stream)
{
    by_precision(s, [&](auto real) {
        using T = decltype(real);
        const rt::NearArgs<T> a{ static_cast<const rt::Node<T> *>(nodes), static_cast<const T *>(points), static_cast<const T *>(radius), exclude, order,
                                 static_cast<T *>(gap), item, found, counters, n_nodes, n, k };
        with_list_bucket(k, [&](auto bucket) {
            constexpr int B = bucket();
            with_flags([&](auto count, auto all, auto ordered) {
                hipLaunchKernelGGL((rt::k_near_spheres<T, count(), all(), ordered(), B>), query_grid(n), query_block(), 0, stream, a);
            }, counters != nullptr, mode == RT_NEAR_ALL, order != nullptr);
        });
    });
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- sphere casts (rt_sweep_spheres*, rt_sweep.hpp) ----

// What both cast entries check (device pointers are not dereferenced here).
bool sweep_args_ok(const rt_scene *s, rt_sweep mode, const void *rays, const void *radius, const void *tmax, uint32_t n, const int32_t *exclude,
                   const uint32_t *order, const void *dist, const void *normal, const int32_t *item, const char *what)
{
    if (!s || !rays || !dist || n == 0) { snprintf(g_err, sizeof g_err, "%s: NULL scene, rays or distance_out, or n == 0", what); return false; }
    if (mode != RT_SWEEP_NEAREST && mode != RT_SWEEP_ANY) { snprintf(g_err, sizeof g_err, "%s: unknown mode %d (nearest is 0, any is 1)", what, (int)mode); return false; }
    return aligned_ok(what, 4, { { item, "item_out" }, { exclude, "exclude" }, { order, "order" } })
           && aligned_ok(what, real_size(s), { { rays, "rays" }, { radius, "radius" }, { tmax, "tmax" }, { dist, "distance_out" }, { normal, "normal_out" } });
}

// The host entry's domain: per cast the ray, a radius in 0 .. 1e15 and a tmax that is not NaN.
bool sweep_casts_valid(const rt_scene *s, const void *rays, const void *radius, const void *tmax, uint32_t n, const char *what)
{
    return each_valid(s, n, [&](auto real, uint32_t i) {
        using T = decltype(real);
        return ray_ok(static_cast<const T *>(rays), i, what, ": rays") && (!radius || radius_ok(static_cast<const T *>(radius)[i], i, what, "radius[", "] ="))
               && not_nan_ok(static_cast<const T *>(tmax), i, what, "tmax");
    });
}

// One cast launch on `stream`: counters != NULL runs the counting flavour (same bytes).
rt_status enqueue_sweep(const rt_scene *s, const void *nodes, uint32_t n_nodes, rt_sweep mode, const void *rays, const void *radius, const void *tmax, uint32_t n,
                        const int32_t *exclude, const uint32_t *order, void *dist, void *normal, int32_t *item, rt::Counters *counters, hipStream_t stream)
{
    by_precision(s, [&](auto real) {
        using T = decltype(real);
        const rt::SweepArgs<T> a{ static_cast<const rt::Node<T> *>(nodes), static_cast<const rt::Item<T> *>(s->d_items), static_cast<const T *>(rays),
                                  static_cast<const T *>(radius), static_cast<const T *>(tmax), exclude, order, static_cast<T *>(dist), static_cast<T *>(normal),
                                  item, counters, n_nodes, n };
        with_flags([&](auto count, auto any, auto ordered) {
            hipLaunchKernelGGL((rt::k_sweep_spheres<T, count(), any(), ordered()>), query_grid(n), query_block(), 0, stream, a);
        }, counters != nullptr, mode == RT_SWEEP_ANY, order != nullptr);
    });
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- contact pairs (rt_scene_contacts*, rt_contacts.hpp) ----

// What both contacts entries check (device pointers are not dereferenced here).
bool contacts_args_ok(const rt_scene *s, double margin, uint32_t capacity, const int32_t *pairs, const void *gap, const uint64_t *offsets, const uint64_t *total,
                      const char *what)
{
    if (!s || !total) { snprintf(g_err, sizeof g_err, "%s: NULL scene or total_out", what); return false; }
    if (std::isnan(margin)) { snprintf(g_err, sizeof g_err, "%s: margin is NaN", what); return false; }
    if (capacity > 0x7FFFFFFFu) { snprintf(g_err, sizeof g_err, "%s: capacity %u is above 2^31 - 1", what, capacity); return false; }
    if (gap && !pairs) { snprintf(g_err, sizeof g_err, "%s: gap_out without pairs_out", what); return false; }
    return aligned_ok(what, 4, { { pairs, "pairs_out" } }) && aligned_ok(what, 8, { { offsets, "offsets_out" }, { total, "total_out" } })
           && aligned_ok(what, real_size(s), { { gap, "gap_out" } });
}

// The three launches of the scan on `stream`: the counts of `n` lists into offsets[n + 1] in the workspace and, where given, in the caller's
// device memory; the total also into *total_out.
rt_status enqueue_list_scan(const ListSpace &w, uint32_t n, uint64_t *offsets_out, uint64_t *total_out, hipStream_t stream)
{
    const unsigned n_sums = (unsigned)(((uint64_t)n + rt::kScanBlock - 1) / rt::kScanBlock);
    const dim3 sgrid(n_sums), sblock(rt::kScanBlock);
    hipLaunchKernelGGL(rt::k_contact_scan_sums, sgrid, sblock, 0, stream, w.counts, n, w.sums);
    hipLaunchKernelGGL(rt::k_contact_scan_spine, dim3(1), sblock, 0, stream, w.sums, n_sums, w.offsets + n, offsets_out ? offsets_out + n : nullptr, total_out);
    hipLaunchKernelGGL(rt::k_contact_scan_offsets, sgrid, sblock, 0, stream, w.counts, n, w.sums, w.offsets, offsets_out);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The scene's contacts workspace, made by the first call, and this call's place behind the one before it.  Under s->contacts.mu.  A scene
// that is not dynamic gets its item-to-node table here, on `stream`: every later call waits for contacts.ev, so for it too.
rt_status contacts_begin(rt_scene *s, const void *nodes, uint32_t n_nodes, hipStream_t stream)
{
    ListSpace &w = s->contacts;
    if (!w.ev) HIP_TRY(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
    if (w.recorded) HIP_TRY(hipStreamWaitEvent(stream, w.ev, 0));
    if (w.d) return RT_OK;
    const size_t n = s->n_items;
    const bool table = s->n_nodes != 0 && !s->d_item_node;
    if (const rt_status st = w.make_total(); st != RT_OK) return st;
    uint8_t *behind = nullptr;
    if (const rt_status st = w.make_room(n, (table ? sizeof(uint32_t) * n : 0) + 256, &behind); st != RT_OK) return st;
    if (table) {
        uint32_t *const item_node = reinterpret_cast<uint32_t *>(behind);
        hipError_t e = hipMemsetAsync(item_node, 0xFF, sizeof(uint32_t) * n, stream);
        if (e != hipSuccess) { (void)hipFree(w.d); w.d = nullptr; return hip_fail(e, "hipMemsetAsync(item_node)", __LINE__); }
        by_precision(s, [&](auto real) {
            using T = decltype(real);
            hipLaunchKernelGGL(rt::k_contact_item_nodes<T>, dim3((n_nodes + 255) / 256), dim3(256), 0, stream, static_cast<const rt::Node<T> *>(nodes), n_nodes, s->n_items, item_node);
        });
        if ((e = hipGetLastError()) != hipSuccess) { (void)hipFree(w.d); w.d = nullptr; return hip_fail(e, "k_contact_item_nodes", __LINE__); }
        s->d_contacts_item_node = item_node;
    }
    return RT_OK;
}

// Where item i's own node lies in the stream the contacts and impacts walks skip from: the dynamic scene's table, or contacts_begin's.
inline const uint32_t *contact_item_node(const rt_scene *s) { return s->n_nodes ? (s->d_item_node ? s->d_item_node : s->d_contacts_item_node) : nullptr; }

// One pass of the walk on `stream`.  The first (fill == false) counts; counters != NULL runs its counting flavour (same counts).  The
// second is the same walk, pair offsets[i] + rank written where it lies below `capacity`.
rt_status enqueue_contacts_pass(const rt_scene *s, const void *nodes, uint32_t n_nodes, double margin, bool fill, uint32_t capacity, int32_t *pairs, void *gap,
                                rt::Counters *counters, hipStream_t stream)
{
    by_precision(s, [&](auto real) {
        using T = decltype(real);
        const ListSpace &w = s->contacts;
        const rt::ContactArgs<T> a{ static_cast<const rt::Node<T> *>(nodes), contact_item_node(s), fill ? nullptr : w.counts, fill ? w.offsets : nullptr, pairs,
                                    static_cast<T *>(gap), counters, (T)margin, n_nodes, s->n_items, capacity };
        if (fill) hipLaunchKernelGGL((rt::k_contact_pairs<T, false, true>), query_grid(s->n_items), query_block(), 0, stream, a);
        else with_flags([&](auto count) { hipLaunchKernelGGL((rt::k_contact_pairs<T, count(), false>), query_grid(s->n_items), query_block(), 0, stream, a); }, counters != nullptr);
    });
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The first pass and the scan: counts, then offsets[n_items + 1] in the workspace and, where given, in the caller's device memory.
rt_status enqueue_contacts_count(const rt_scene *s, const void *nodes, uint32_t n_nodes, double margin, uint64_t *offsets_out, uint64_t *total_out,
                                 rt::Counters *counters, hipStream_t stream)
{
    const rt_status st = enqueue_contacts_pass(s, nodes, n_nodes, margin, false, 0u, nullptr, nullptr, counters, stream);
    return st != RT_OK ? st : enqueue_list_scan(s->contacts, s->n_items, offsets_out, total_out, stream);
}

rt_status enqueue_contacts_fill(const rt_scene *s, const void *nodes, uint32_t n_nodes, double margin, uint32_t capacity, int32_t *pairs, void *gap, hipStream_t stream)
{
    return enqueue_contacts_pass(s, nodes, n_nodes, margin, true, capacity, pairs, gap, nullptr, stream);
}

// ---- impact pairs (rt_scene_impacts*, rt_impacts.hpp) ----

// What both impacts entries check (device pointers are not dereferenced here).
bool impacts_args_ok(const rt_scene *s, const void *disp, uint32_t capacity, const int32_t *pairs, const void *time, const uint64_t *offsets, const uint64_t *total,
                     const char *what)
{
    if (!s || !disp || !total) { snprintf(g_err, sizeof g_err, "%s: NULL scene, disp or total_out", what); return false; }
    if (capacity > 0x7FFFFFFFu) { snprintf(g_err, sizeof g_err, "%s: capacity %u is above 2^31 - 1", what, capacity); return false; }
    if (time && !pairs) { snprintf(g_err, sizeof g_err, "%s: time_out without pairs_out", what); return false; }
    return aligned_ok(what, 4, { { pairs, "pairs_out" } }) && aligned_ok(what, 8, { { offsets, "offsets_out" }, { total, "total_out" } })
           && aligned_ok(what, real_size(s), { { disp, "disp" }, { time, "time_out" } });
}

// The host entry's domain: the displacement of every slot.
bool impacts_disp_valid(const rt_scene *s, const void *disp, uint32_t n_items, const char *what)
{
    return each_valid(s, n_items, [&](auto real, uint32_t i) {
        return triple_ok(static_cast<const decltype(real) *>(disp) + 3 * (size_t)i, i, what, "disp of slot", "component");
    });
}

// Where the parts of a motion table of `cap` nodes lie, in bytes: the nodes' motions at 0, their lengths, the lengths' chunk maxima, the
// call's magnitude (a word of its own) and the bound nodes' radii.
struct MotionLayout { size_t length, chunk, magnitude, radius, bytes; };
MotionLayout motion_table_layout(size_t esz, uint32_t cap)
{
    const auto padded = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t n = cap ? cap : 1, n_chunks = (n + rt::kMotionChunk - 1) / rt::kMotionChunk;
    MotionLayout l{};
    l.length = padded(4 * esz * n);
    l.chunk = l.length + padded(esz * n);
    l.magnitude = l.chunk + padded(esz * n_chunks);
    l.radius = l.magnitude + 256;
    l.bytes = l.radius + padded(esz * n);
    return l;
}

// Room for a motion table of `n_nodes` nodes in *table.  `w`: the workspace behind whose event the calls that use this table run -- a
// table that has to grow waits for it.
rt_status motion_table_begin(rt_scene *s, const ListSpace &w, void **table, uint32_t *cap, uint32_t n_nodes, const char *what)
{
    if (n_nodes <= *cap && *table) return RT_OK;
    if (*table) {
        if (w.recorded) HIP_TRY(hipEventSynchronize(w.ev));
        HIP_TRY(hipFree(*table));
        *table = nullptr; *cap = 0;
    }
    const size_t esz = real_size(s);
    const MotionLayout l = motion_table_layout(esz, n_nodes);
    HIP_TRY(hipMalloc(table, l.bytes));
    *cap = n_nodes;
    // the radii of the bound nodes: a static scene's never change and go up once; a dynamic scene's are gathered per call
    if (!s->dynamic && s->n_nodes != 0u) {
        if (s->h_node_radius.size() != esz * (size_t)s->n_nodes || n_nodes != s->n_nodes) {
            snprintf(g_err, sizeof g_err, "%s: internal: the scene kept no radii for its %u nodes", what, s->n_nodes);
            return RT_ERR_INVALID_ARGUMENT;
        }
        HIP_TRY(hipMemcpy(static_cast<uint8_t *>(*table) + l.radius, s->h_node_radius.data(), s->h_node_radius.size(), hipMemcpyHostToDevice));
    }
    return RT_OK;
}

// contacts_begin, and room for the motion table of `n_nodes` nodes.  Under s->contacts.mu.
rt_status impacts_begin(rt_scene *s, const void *nodes, uint32_t n_nodes, hipStream_t stream)
{
    const rt_status st = contacts_begin(s, nodes, n_nodes, stream);
    if (st != RT_OK) return st;
    return motion_table_begin(s, s->contacts, &s->d_impacts, &s->impacts_cap, n_nodes, "rt_scene_impacts");
}

template <typename T> struct ImpactsSpace { rt::Motion<T> *motion; T *length, *chunk, *magnitude, *radius; };
template <typename T>
ImpactsSpace<T> motion_table_space(void *table, uint32_t cap)
{
    const MotionLayout l = motion_table_layout(sizeof(T), cap);
    uint8_t *const d = static_cast<uint8_t *>(table);
    return { reinterpret_cast<rt::Motion<T> *>(d), reinterpret_cast<T *>(d + l.length), reinterpret_cast<T *>(d + l.chunk), reinterpret_cast<T *>(d + l.magnitude),
             reinterpret_cast<T *>(d + l.radius) };
}

// The motion table of one call into `w`, on `stream`: *w.magnitude must already be 0 or hold what the call folds in besides the scene.
// disp == NULL: the scene stands still (every e and D is 0).
template <typename T>
rt_status enqueue_motion_table(const rt_scene *s, const rt::Node<T> *st, uint32_t n_nodes, const T *disp, const ImpactsSpace<T> &w, hipStream_t stream)
{
    if (n_nodes == 0u) return RT_OK;
    const unsigned n_chunks = (n_nodes + rt::kMotionChunk - 1) / rt::kMotionChunk;
    if (s->dynamic && s->n_nodes != 0u && s->n_bounds != 0u)
        hipLaunchKernelGGL(rt::k_impact_bound_radii<T>, dim3((s->n_bounds + 255) / 256), dim3(256), 0, stream, static_cast<const rt::Item<T> *>(s->d_bounds), s->d_bound_node,
                           s->n_bounds, n_nodes, w.radius);
    hipLaunchKernelGGL(rt::k_impact_motion_items<T>, dim3(n_chunks), dim3(rt::kMotionChunk), 0, stream, st, static_cast<const rt::Item<T> *>(s->d_items),
                       s->n_nodes != 0u ? w.radius : nullptr, disp, n_nodes, s->n_items, w.motion, w.length, w.chunk, w.magnitude);
    hipLaunchKernelGGL(rt::k_impact_motion_bounds<T>, dim3((n_nodes + 255) / 256), dim3(256), 0, stream, st, n_nodes, w.length, w.chunk, w.magnitude, w.motion);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// One pass of the walk on `stream`.  The first (fill == false) makes the motion table and counts; counters != NULL runs its counting
// flavour (same counts).  The second is the same walk over the table the first left, pair offsets[i] + rank written below `capacity`.
rt_status enqueue_impacts_pass(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *disp, bool fill, uint32_t capacity, int32_t *pairs, void *time,
                               rt::Counters *counters, hipStream_t stream)
{
    return by_precision(s, [&](auto real) -> rt_status {
        using T = decltype(real);
        const ImpactsSpace<T> w = motion_table_space<T>(s->d_impacts, s->impacts_cap);
        const rt::Node<T> *const st = static_cast<const rt::Node<T> *>(nodes);
        if (!fill) {
            HIP_TRY(hipMemsetAsync(w.magnitude, 0, sizeof(T), stream));
            if (const rt_status mt = enqueue_motion_table<T>(s, st, n_nodes, static_cast<const T *>(disp), w, stream); mt != RT_OK) return mt;
        }
        const rt::ImpactArgs<T> a{ st, w.motion, w.magnitude, contact_item_node(s), fill ? nullptr : s->contacts.counts, fill ? s->contacts.offsets : nullptr, pairs,
                                   static_cast<T *>(time), counters, n_nodes, s->n_items, capacity };
        if (fill) hipLaunchKernelGGL((rt::k_impact_pairs<T, false, true>), query_grid(s->n_items), query_block(), 0, stream, a);
        else with_flags([&](auto count) { hipLaunchKernelGGL((rt::k_impact_pairs<T, count(), false>), query_grid(s->n_items), query_block(), 0, stream, a); }, counters != nullptr);
        HIP_TRY(hipGetLastError());
        return RT_OK;
    });
}

// The motion table, the first pass and the scan.
rt_status enqueue_impacts_count(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *disp, uint64_t *offsets_out, uint64_t *total_out,
                                rt::Counters *counters, hipStream_t stream)
{
    const rt_status st = enqueue_impacts_pass(s, nodes, n_nodes, disp, false, 0u, nullptr, nullptr, counters, stream);
    return st != RT_OK ? st : enqueue_list_scan(s->contacts, s->n_items, offsets_out, total_out, stream);
}

rt_status enqueue_impacts_fill(const rt_scene *s, const void *nodes, uint32_t n_nodes, uint32_t capacity, int32_t *pairs, void *time, hipStream_t stream)
{
    return enqueue_impacts_pass(s, nodes, n_nodes, nullptr, true, capacity, pairs, time, nullptr, stream);
}

// ---- contact islands (rt_scene_islands*, rt_scene_impact_islands*, rt_islands.hpp) ----

// What the four islands entries check (device pointers are not dereferenced here).  moving: the impact form, which takes disp and no margin.
bool islands_args_ok(const rt_scene *s, bool moving, double margin, const void *disp, const int32_t *label, const int32_t *index, const uint32_t *size,
                     const uint64_t *n_islands, const char *what)
{
    if (!s || !label || (moving && !disp)) { snprintf(g_err, sizeof g_err, "%s: NULL scene%s or label_out", what, moving ? ", disp" : ""); return false; }
    if (!moving && std::isnan(margin)) { snprintf(g_err, sizeof g_err, "%s: margin is NaN", what); return false; }
    return aligned_ok(what, 4, { { label, "label_out" }, { index, "index_out" }, { size, "size_out" } }) && aligned_ok(what, 8, { { n_islands, "n_islands_out" } })
           && aligned_ok(what, real_size(s), { { disp, "disp" } });
}

// contacts_begin (moving: impacts_begin), and the scene's forest: parent[n_items] and size_root[n_items] behind it, made by the first
// islands call.  Under s->contacts.mu: islands calls take their turn with the contacts and impacts calls, whose counts and offsets they use.
rt_status islands_begin(rt_scene *s, bool moving, const void *nodes, uint32_t n_nodes, hipStream_t stream)
{
    const rt_status st = moving ? impacts_begin(s, nodes, n_nodes, stream) : contacts_begin(s, nodes, n_nodes, stream);
    if (st != RT_OK || s->d_islands) return st;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_islands), 2 * sizeof(uint32_t) * (size_t)s->n_items));
    return RT_OK;
}

// One islands call on `stream`: the forest's start, the hook walk (moving: behind its motion table), the labels, the scan of the roots --
// whose total is n_islands -- and, where index or size is wanted, the last kernel.  counters != NULL runs the walk's counting flavour (same
// labels).  label: required; index, size, n_islands: device pointers or NULL.
rt_status enqueue_islands(const rt_scene *s, const void *nodes, uint32_t n_nodes, bool moving, double margin, const void *disp, int32_t *label, int32_t *index,
                          uint32_t *size, uint64_t *n_islands, rt::Counters *counters, hipStream_t stream)
{
    const uint32_t n = s->n_items;
    uint32_t *const parent = s->d_islands, *const size_root = size ? s->d_islands + n : nullptr;
    const dim3 grid((n + 255) / 256), block(256);
    const ListSpace &w = s->contacts;
    const rt_status st = by_precision(s, [&](auto real) -> rt_status {
        using T = decltype(real);
        const rt::Node<T> *const stn = static_cast<const rt::Node<T> *>(nodes);
        hipLaunchKernelGGL(rt::k_island_init, grid, block, 0, stream, parent, size_root, n);
        rt::IslandArgs<T> a{ nullptr, contact_item_node(s), counters, moving ? T(0.0) : (T)margin, n_nodes, n };
        const rt::Motion<T> *motion = nullptr;
        if (moving) {
            const ImpactsSpace<T> m = motion_table_space<T>(s->d_impacts, s->impacts_cap);
            HIP_TRY(hipMemsetAsync(m.magnitude, 0, sizeof(T), stream));
            if (const rt_status mt = enqueue_motion_table<T>(s, stn, n_nodes, static_cast<const T *>(disp), m, stream); mt != RT_OK) return mt;
            motion = m.motion;
            a.magnitude = m.magnitude;
        }
        with_flags([&](auto count, auto mov) { hipLaunchKernelGGL((rt::k_island_hook<T, count(), mov()>), query_grid(n), query_block(), 0, stream, a, stn, motion, parent); },
                   counters != nullptr, moving);
        hipLaunchKernelGGL(rt::k_island_labels<T>, grid, block, 0, stream, stn, contact_item_node(s), parent, n_nodes, n, label, w.counts, size_root);
        HIP_TRY(hipGetLastError());
        return RT_OK;
    });
    if (st != RT_OK) return st;
    if (const rt_status sc = enqueue_list_scan(w, n, nullptr, n_islands, stream); sc != RT_OK) return sc;
    if (index || size) {
        hipLaunchKernelGGL(rt::k_island_finish, grid, block, 0, stream, label, w.offsets, size_root, n, index, size);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}

// ---- overlap lists (rt_overlap_spheres*, rt_overlap.hpp) ----

// What both overlap entries check (device pointers are not dereferenced here).
bool overlap_args_ok(const rt_scene *s, const void *queries, uint32_t n, double margin, const int32_t *exclude, const uint32_t *order, uint32_t capacity,
                     const int32_t *items, const void *gap, const uint64_t *offsets, const uint64_t *total, const char *what)
{
    if (!s || !queries || !total || n == 0) { snprintf(g_err, sizeof g_err, "%s: NULL scene, queries or total_out, or n == 0", what); return false; }
    if (std::isnan(margin)) { snprintf(g_err, sizeof g_err, "%s: margin is NaN", what); return false; }
    if (capacity > 0x7FFFFFFFu) { snprintf(g_err, sizeof g_err, "%s: capacity %u is above 2^31 - 1", what, capacity); return false; }
    if (gap && !items) { snprintf(g_err, sizeof g_err, "%s: gap_out without items_out", what); return false; }
    return aligned_ok(what, 4, { { items, "items_out" }, { exclude, "exclude" }, { order, "order" } })
           && aligned_ok(what, 8, { { offsets, "offsets_out" }, { total, "total_out" } }) && aligned_ok(what, real_size(s), { { queries, "queries" }, { gap, "gap_out" } });
}

// The host entry's domain: per query sphere its centre (rt_near_spheres's points) and a radius in 0 .. 1e15 (rt_sweep_spheres's).
bool overlap_queries_valid(const rt_scene *s, const void *queries, uint32_t n, const char *what)
{
    return each_valid(s, n, [&](auto real, uint32_t i) {
        const decltype(real) *rec = static_cast<const decltype(real) *>(queries) + 4 * (size_t)i;
        return triple_ok(rec, i, what, "query", "coordinate") && radius_ok(rec[3], i, what, "query ", "'s radius");
    });
}

// The scene's overlap workspace for `n` queries, and this call's place behind the one before it.  Under s->overlap.mu.  The first call
// makes the workspace; a call with more queries than any before it makes a larger one, once the call before it is through with the old.
rt_status overlap_begin(rt_scene *s, uint32_t n, hipStream_t stream)
{
    ListSpace &w = s->overlap;
    if (!w.ev) HIP_TRY(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
    if (const rt_status st = w.make_total(); st != RT_OK) return st;
    if (n > w.cap) {
        if (w.recorded) HIP_TRY(hipEventSynchronize(w.ev));
        if (const rt_status st = w.make_room(n, 0, nullptr); st != RT_OK) return st;
    }
    if (w.recorded) HIP_TRY(hipStreamWaitEvent(stream, w.ev, 0));
    return RT_OK;
}

// One pass of the walk on `stream`.  The first (fill == false) counts; counters != NULL runs its counting flavour (same counts); with an
// order a query that no thread carries keeps the count 0.  The second is the same walk by the queries that counted something, entry
// offsets[g] + rank written where it lies below `capacity`.
rt_status enqueue_overlap_pass(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *queries, uint32_t n, double margin, const int32_t *exclude,
                               const uint32_t *order, bool fill, uint32_t capacity, int32_t *items, void *gap, rt::Counters *counters, hipStream_t stream)
{
    if (!fill && order) HIP_TRY(hipMemsetAsync(s->overlap.counts, 0, sizeof(uint32_t) * (size_t)n, stream));
    by_precision(s, [&](auto real) {
        using T = decltype(real);
        const rt::OverlapArgs<T> a{ static_cast<const rt::Node<T> *>(nodes), static_cast<const T *>(queries), exclude, order, s->overlap.counts,
                                    fill ? s->overlap.offsets : nullptr, items, static_cast<T *>(gap), counters, (T)margin, n_nodes, n, capacity };
        if (fill) hipLaunchKernelGGL((rt::k_overlap_spheres<T, false, true>), query_grid(n), query_block(), 0, stream, a);
        else with_flags([&](auto count) { hipLaunchKernelGGL((rt::k_overlap_spheres<T, count(), false>), query_grid(n), query_block(), 0, stream, a); }, counters != nullptr);
    });
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The first pass and the scan: counts, then offsets[n + 1] in the workspace and, where given, in the caller's device memory.
rt_status enqueue_overlap_count(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *queries, uint32_t n, double margin, const int32_t *exclude,
                                const uint32_t *order, uint64_t *offsets_out, uint64_t *total_out, rt::Counters *counters, hipStream_t stream)
{
    const rt_status st = enqueue_overlap_pass(s, nodes, n_nodes, queries, n, margin, exclude, order, false, 0u, nullptr, nullptr, counters, stream);
    return st != RT_OK ? st : enqueue_list_scan(s->overlap, n, offsets_out, total_out, stream);
}

rt_status enqueue_overlap_fill(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *queries, uint32_t n, double margin, const int32_t *exclude,
                               const uint32_t *order, uint32_t capacity, int32_t *items, void *gap, hipStream_t stream)
{
    return enqueue_overlap_pass(s, nodes, n_nodes, queries, n, margin, exclude, order, true, capacity, items, gap, nullptr, stream);
}

// ---- box overlap lists (rt_overlap_boxes*, rt_box.hpp): the overlap lists' workspace (overlap_begin) and their turn ----

// What both box entries check (device pointers are not dereferenced here).
bool boxes_args_ok(const rt_scene *s, const void *boxes, uint32_t n, double margin, const int32_t *exclude, const uint32_t *order, uint32_t capacity,
                   const int32_t *items, const void *gap, const uint64_t *offsets, const uint64_t *total, const char *what)
{
    if (!s) { snprintf(g_err, sizeof g_err, "%s: NULL scene", what); return false; }
    if (!boxes) { snprintf(g_err, sizeof g_err, "%s: NULL boxes", what); return false; }
    if (!total) { snprintf(g_err, sizeof g_err, "%s: NULL total_out", what); return false; }
    if (n == 0) { snprintf(g_err, sizeof g_err, "%s: n == 0", what); return false; }
    if (std::isnan(margin)) { snprintf(g_err, sizeof g_err, "%s: margin is NaN", what); return false; }
    if (capacity > 0x7FFFFFFFu) { snprintf(g_err, sizeof g_err, "%s: capacity %u is above 2^31 - 1", what, capacity); return false; }
    if (gap && !items) { snprintf(g_err, sizeof g_err, "%s: gap_out without items_out", what); return false; }
    return aligned_ok(what, 4, { { items, "items_out" }, { exclude, "exclude" }, { order, "order" } })
           && aligned_ok(what, 8, { { offsets, "offsets_out" }, { total, "total_out" } }) && aligned_ok(what, real_size(s), { { boxes, "boxes" }, { gap, "gap_out" } });
}

// The host entry's domain: no coordinate is NaN, a finite one lies within +-1e15 (an infinite side is a slab's or a half-space's), and
// lo <= hi on every axis.
bool boxes_valid(const rt_scene *s, const void *boxes, uint32_t n, const char *what)
{
    return each_valid(s, n, [&](auto real, uint32_t i) {
        const decltype(real) *b = static_cast<const decltype(real) *>(boxes) + 6 * (size_t)i;
        for (int k = 0; k < 6; ++k)
            if (std::isnan(b[k]) || (std::isfinite(b[k]) && std::fabs((double)b[k]) > 1e15)) {
                snprintf(g_err, sizeof g_err, "%s: box %u has a NaN coordinate or a finite one beyond +-1e15", what, i);
                return false;
            }
        for (int k = 0; k < 3; ++k)
            if (b[k] > b[k + 3]) {
                snprintf(g_err, sizeof g_err, "%s: box %u is inverted: lo %g > hi %g on axis %d", what, i, (double)b[k], (double)b[k + 3], k);
                return false;
            }
        return true;
    });
}

// One pass of the walk on `stream`, as enqueue_overlap_pass: the first (fill == false) counts, counters != NULL runs its counting flavour
// (same counts), and with an order a box that no thread carries keeps the count 0; the second is the same walk by the boxes that counted
// something, entry offsets[g] + rank written where it lies below `capacity`.
rt_status enqueue_boxes_pass(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *boxes, uint32_t n, double margin, const int32_t *exclude,
                             const uint32_t *order, bool fill, uint32_t capacity, int32_t *items, void *gap, rt::Counters *counters, hipStream_t stream)
{
    if (!fill && order) HIP_TRY(hipMemsetAsync(s->overlap.counts, 0, sizeof(uint32_t) * (size_t)n, stream));
    by_precision(s, [&](auto real) {
        using T = decltype(real);
        const rt::BoxArgs<T> a{ static_cast<const rt::Node<T> *>(nodes), static_cast<const T *>(boxes), exclude, order, s->overlap.counts,
                                fill ? s->overlap.offsets : nullptr, items, static_cast<T *>(gap), counters, (T)margin, n_nodes, n, capacity };
        if (fill) hipLaunchKernelGGL((rt::k_overlap_boxes<T, false, true>), query_grid(n), query_block(), 0, stream, a);
        else with_flags([&](auto count) { hipLaunchKernelGGL((rt::k_overlap_boxes<T, count(), false>), query_grid(n), query_block(), 0, stream, a); }, counters != nullptr);
    });
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The first pass and the scan: counts, then offsets[n + 1] in the workspace and, where given, in the caller's device memory.
rt_status enqueue_boxes_count(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *boxes, uint32_t n, double margin, const int32_t *exclude,
                              const uint32_t *order, uint64_t *offsets_out, uint64_t *total_out, rt::Counters *counters, hipStream_t stream)
{
    const rt_status st = enqueue_boxes_pass(s, nodes, n_nodes, boxes, n, margin, exclude, order, false, 0u, nullptr, nullptr, counters, stream);
    return st != RT_OK ? st : enqueue_list_scan(s->overlap, n, offsets_out, total_out, stream);
}

rt_status enqueue_boxes_fill(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *boxes, uint32_t n, double margin, const int32_t *exclude,
                             const uint32_t *order, uint32_t capacity, int32_t *items, void *gap, hipStream_t stream)
{
    return enqueue_boxes_pass(s, nodes, n_nodes, boxes, n, margin, exclude, order, true, capacity, items, gap, nullptr, stream);
}

// ---- region overlap lists (rt_overlap_regions*, rt_region.hpp): the overlap lists' workspace (overlap_begin) for n J counts, and their turn ----

// The rule for sections == 0 (include/rtrace_hip.h states it, rust_tracer_amd.region_sections restates it): a pure function of (n, n_nodes).
// As many sections as bring the call to kRegionLanes lanes, none shorter than kRegionSectionNodes nodes.  DESIGN.md 4.23 has the sweep
// (tools/region_rate.py) that chose the two constants.
constexpr uint32_t kRegionLanes = 1u << 18, kRegionSectionNodes = 8u, kRegionMaxCounts = 1u << 26;

inline uint32_t region_sections_rule(uint32_t n, uint32_t n_nodes)
{
    return std::max(1u, std::min(kRegionLanes / std::max(n, 1u), n_nodes / kRegionSectionNodes));
}

// J of a call: the caller's `sections` clamped to 1 .. n_nodes, or the rule's for 0.  The stream a region call walks has s->n_nodes nodes,
// or -- a scene without bounds -- one per item (query_stream); neither changes after the scene is made.
inline uint32_t region_sections_of(const rt_scene *s, uint32_t n, uint32_t sections)
{
    const uint32_t n_nodes = std::max(1u, s->n_nodes ? s->n_nodes : s->n_items);
    return sections == 0u ? region_sections_rule(n, n_nodes) : std::min(sections, n_nodes);
}

// What both region entries check (device pointers are not dereferenced here).
bool regions_args_ok(const rt_scene *s, const void *planes, uint32_t n, double margin, uint32_t sections, uint32_t capacity, const int32_t *items, const void *gap,
                     const uint64_t *offsets, const uint64_t *total, const char *what)
{
    if (!s) { snprintf(g_err, sizeof g_err, "%s: NULL scene", what); return false; }
    if (!planes) { snprintf(g_err, sizeof g_err, "%s: NULL planes", what); return false; }
    if (!total) { snprintf(g_err, sizeof g_err, "%s: NULL total_out", what); return false; }
    if (n == 0) { snprintf(g_err, sizeof g_err, "%s: n == 0", what); return false; }
    if (std::isnan(margin)) { snprintf(g_err, sizeof g_err, "%s: margin is NaN", what); return false; }
    if (capacity > 0x7FFFFFFFu) { snprintf(g_err, sizeof g_err, "%s: capacity %u is above 2^31 - 1", what, capacity); return false; }
    if (gap && !items) { snprintf(g_err, sizeof g_err, "%s: gap_out without items_out", what); return false; }
    if (!(aligned_ok(what, 4, { { items, "items_out" } }) && aligned_ok(what, 8, { { offsets, "offsets_out" }, { total, "total_out" } })
          && aligned_ok(what, real_size(s), { { planes, "planes" }, { gap, "gap_out" } })))
        return false;
    const uint32_t J = region_sections_of(s, n, sections);
    if ((uint64_t)n * J > kRegionMaxCounts) {
        snprintf(g_err, sizeof g_err, "%s: n * sections = %u * %u is above 2^26", what, n, J);
        return false;
    }
    return true;
}

// The host entry's domain, plane k of region i: no NaN; a normal that is finite and of length 1 (|n.n - 1| <= 2^-10: what catches input
// that was never normalised, no tolerance of the metric) with a d that is -inf or finite within +-1e15; or the absent plane, a zero normal
// with d = -inf.
bool regions_valid(const rt_scene *s, const void *planes, uint32_t n, const char *what)
{
    return each_valid(s, n, [&](auto real, uint32_t i) {
        const decltype(real) *r = static_cast<const decltype(real) *>(planes) + 24 * (size_t)i;
        for (int k = 0; k < 6; ++k) {
            const double x = (double)r[4 * k], y = (double)r[4 * k + 1], z = (double)r[4 * k + 2], d = (double)r[4 * k + 3];
            const char *bad = nullptr;
            const double nn = (x * x + y * y) + z * z;
            if (std::isnan(x) || std::isnan(y) || std::isnan(z) || std::isnan(d)) bad = "holds a NaN";
            else if (std::isinf(x) || std::isinf(y) || std::isinf(z)) bad = "has an infinite normal component";
            else if (d == std::numeric_limits<double>::infinity()) bad = "has d = +inf";
            else if (std::isfinite(d) && std::fabs(d) > 1e15) bad = "has a finite |d| above 1e15";
            else if (nn == 0.0 && std::isfinite(d)) bad = "has a zero normal and a d that is not -inf";
            else if (nn != 0.0 && std::fabs(nn - 1.0) > 0x1p-10) bad = "has a normal that is not of length 1";
            if (bad) {
                snprintf(g_err, sizeof g_err, "%s: region %u, plane %d %s", what, i, k, bad);
                return false;
            }
        }
        return true;
    });
}

// One pass of the sectioned walk on `stream` (rt_region.hpp): ceil(J / 64) waves per region.  The first (fill == false) writes every one of
// the n J counts; counters != NULL runs its counting flavour (same counts).  The second is the same walk by the sections that counted
// something, entry offsets[g J + j] + rank written where it lies below `capacity`.
rt_status enqueue_regions_pass(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *planes, uint32_t n, double margin, uint32_t J, bool fill,
                               uint32_t capacity, int32_t *items, void *gap, rt::Counters *counters, hipStream_t stream)
{
    const uint64_t waves = (uint64_t)n * ((J + 63u) / 64u);                    // <= n J <= 2^26
    const dim3 grid((unsigned)((waves * 64u + rt::kBlockThreads - 1) / rt::kBlockThreads));
    by_precision(s, [&](auto real) {
        using T = decltype(real);
        const rt::RegionArgs<T> a{ static_cast<const rt::Node<T> *>(nodes), static_cast<const T *>(planes), s->overlap.counts, fill ? s->overlap.offsets : nullptr,
                                   items, static_cast<T *>(gap), counters, (T)margin, n_nodes, n, J, capacity };
        if (fill) hipLaunchKernelGGL((rt::k_overlap_regions<T, false, true>), grid, query_block(), 0, stream, a);
        else with_flags([&](auto count) { hipLaunchKernelGGL((rt::k_overlap_regions<T, count(), false>), grid, query_block(), 0, stream, a); }, counters != nullptr);
    });
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The first pass, the scan over the n J counts -- offsets[n J + 1] in the workspace, the total where the caller wants it -- and the rows:
// offsets_out[g] = offsets[g J] where given, and the regions with an entry into the counters' hits.
rt_status enqueue_regions_count(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *planes, uint32_t n, double margin, uint32_t J,
                                uint64_t *offsets_out, uint64_t *total_out, rt::Counters *counters, hipStream_t stream)
{
    rt_status st = enqueue_regions_pass(s, nodes, n_nodes, planes, n, margin, J, false, 0u, nullptr, nullptr, counters, stream);
    if (st == RT_OK) st = enqueue_list_scan(s->overlap, n * J, nullptr, total_out, stream);
    if (st != RT_OK || (!offsets_out && !counters)) return st;
    hipLaunchKernelGGL(rt::k_region_rows, query_grid(n + 1u), query_block(), 0, stream, s->overlap.offsets, n, J, offsets_out, counters);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

rt_status enqueue_regions_fill(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *planes, uint32_t n, double margin, uint32_t J, uint32_t capacity,
                               int32_t *items, void *gap, hipStream_t stream)
{
    return enqueue_regions_pass(s, nodes, n_nodes, planes, n, margin, J, true, capacity, items, gap, nullptr, stream);
}

// ---- swept overlap lists (rt_swept_overlaps*, rt_swept.hpp) ----

// What both swept entries check (device pointers are not dereferenced here).
bool swept_args_ok(const rt_scene *s, const void *queries, const void *qdisp, uint32_t n, const void *disp, const int32_t *exclude, const uint32_t *order,
                   uint32_t capacity, const int32_t *items, const void *time, const void *normal, const uint64_t *offsets, const uint64_t *total, const char *what)
{
    if (!s) { snprintf(g_err, sizeof g_err, "%s: NULL scene", what); return false; }
    if (!queries) { snprintf(g_err, sizeof g_err, "%s: NULL queries", what); return false; }
    if (!qdisp) { snprintf(g_err, sizeof g_err, "%s: NULL qdisp", what); return false; }
    if (!total) { snprintf(g_err, sizeof g_err, "%s: NULL total_out", what); return false; }
    if (n == 0) { snprintf(g_err, sizeof g_err, "%s: n == 0", what); return false; }
    if (capacity > 0x7FFFFFFFu) { snprintf(g_err, sizeof g_err, "%s: capacity %u is above 2^31 - 1", what, capacity); return false; }
    if (time && !items) { snprintf(g_err, sizeof g_err, "%s: time_out without items_out", what); return false; }
    if (normal && !items) { snprintf(g_err, sizeof g_err, "%s: normal_out without items_out", what); return false; }
    return aligned_ok(what, 4, { { items, "items_out" }, { exclude, "exclude" }, { order, "order" } })
           && aligned_ok(what, 8, { { offsets, "offsets_out" }, { total, "total_out" } })
           && aligned_ok(what, real_size(s), { { queries, "queries" }, { qdisp, "qdisp" }, { disp, "disp" }, { time, "time_out" }, { normal, "normal_out" } });
}

// The host entry's domain for the queries' displacements.
bool swept_qdisp_valid(const rt_scene *s, const void *qdisp, uint32_t n, const char *what)
{
    return each_valid(s, n, [&](auto real, uint32_t i) {
        return triple_ok(static_cast<const decltype(real) *>(qdisp) + 3 * (size_t)i, i, what, "qdisp of query", "component");
    });
}

// overlap_begin, and room for this entry's motion table of `n_nodes` nodes.  Under s->overlap.mu.
rt_status swept_begin(rt_scene *s, uint32_t n, uint32_t n_nodes, hipStream_t stream)
{
    const rt_status st = overlap_begin(s, n, stream);
    if (st != RT_OK) return st;
    return motion_table_begin(s, s->overlap, &s->d_swept, &s->swept_cap, n_nodes, "rt_swept_overlaps");
}

// What a walk of moving queries runs first on `stream`: the queries' magnitude into *w.magnitude, then the motion table.
template <typename T>
rt_status enqueue_query_motion(const rt_scene *s, const rt::Node<T> *st, uint32_t n_nodes, const T *queries, const T *qdisp, uint32_t n, const T *disp,
                               const ImpactsSpace<T> &w, hipStream_t stream)
{
    HIP_TRY(hipMemsetAsync(w.magnitude, 0, sizeof(T), stream));
    hipLaunchKernelGGL(rt::k_swept_query_magnitude<T>, dim3((unsigned)(((uint64_t)n + 255) / 256)), dim3(256), 0, stream, queries, qdisp, n, w.magnitude);
    HIP_TRY(hipGetLastError());
    return enqueue_motion_table<T>(s, st, n_nodes, disp, w, stream);
}

// One pass of the walk on `stream`.  The first (fill == false) runs enqueue_query_motion and counts; counters != NULL runs its counting
// flavour (same counts); with an order a query that no thread carries keeps the count 0.  The second is the same walk over the table the
// first left, by the queries that counted something; entry offsets[g] + rank written where it lies below `capacity`.
rt_status enqueue_swept_pass(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *queries, const void *qdisp, uint32_t n, const void *disp,
                             const int32_t *exclude, const uint32_t *order, bool fill, uint32_t capacity, int32_t *items, void *time, void *normal,
                             rt::Counters *counters, hipStream_t stream)
{
    return by_precision(s, [&](auto real) -> rt_status {
        using T = decltype(real);
        const ImpactsSpace<T> w = motion_table_space<T>(s->d_swept, s->swept_cap);
        const rt::Node<T> *const st = static_cast<const rt::Node<T> *>(nodes);
        const T *const q = static_cast<const T *>(queries), *const qd = static_cast<const T *>(qdisp);
        if (!fill) {
            if (const rt_status mt = enqueue_query_motion<T>(s, st, n_nodes, q, qd, n, static_cast<const T *>(disp), w, stream); mt != RT_OK) return mt;
            if (order) HIP_TRY(hipMemsetAsync(s->overlap.counts, 0, sizeof(uint32_t) * (size_t)n, stream));
        }
        const rt::SweptArgs<T> a{ st, w.motion, w.magnitude, q, qd, exclude, order, s->overlap.counts, fill ? s->overlap.offsets : nullptr, items,
                                  static_cast<T *>(time), static_cast<T *>(normal), counters, n_nodes, n, capacity };
        if (fill) hipLaunchKernelGGL((rt::k_swept_overlaps<T, false, true>), query_grid(n), query_block(), 0, stream, a);
        else with_flags([&](auto count) { hipLaunchKernelGGL((rt::k_swept_overlaps<T, count(), false>), query_grid(n), query_block(), 0, stream, a); }, counters != nullptr);
        HIP_TRY(hipGetLastError());
        return RT_OK;
    });
}

// The queries' magnitude, the motion table, the first pass and the scan.
rt_status enqueue_swept_count(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *queries, const void *qdisp, uint32_t n, const void *disp,
                              const int32_t *exclude, const uint32_t *order, uint64_t *offsets_out, uint64_t *total_out, rt::Counters *counters, hipStream_t stream)
{
    const rt_status st = enqueue_swept_pass(s, nodes, n_nodes, queries, qdisp, n, disp, exclude, order, false, 0u, nullptr, nullptr, nullptr, counters, stream);
    return st != RT_OK ? st : enqueue_list_scan(s->overlap, n, offsets_out, total_out, stream);
}

rt_status enqueue_swept_fill(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *queries, const void *qdisp, uint32_t n, const int32_t *exclude,
                             const uint32_t *order, uint32_t capacity, int32_t *items, void *time, void *normal, hipStream_t stream)
{
    return enqueue_swept_pass(s, nodes, n_nodes, queries, qdisp, n, nullptr, exclude, order, true, capacity, items, time, normal, nullptr, stream);
}

// ---- first contacts (rt_first_contacts*, rt_first.hpp) ----

// What both first-contact entries check (device pointers are not dereferenced here).
bool first_args_ok(const rt_scene *s, rt_sweep mode, const void *queries, const void *qdisp, uint32_t n, const void *disp, const int32_t *exclude,
                   const uint32_t *order, const void *time, const int32_t *item, const void *normal, const char *what)
{
    if (!s) { snprintf(g_err, sizeof g_err, "%s: NULL scene", what); return false; }
    if (mode != RT_SWEEP_NEAREST && mode != RT_SWEEP_ANY) { snprintf(g_err, sizeof g_err, "%s: unknown mode %d (nearest is 0, any is 1)", what, (int)mode); return false; }
    if (!queries) { snprintf(g_err, sizeof g_err, "%s: NULL queries", what); return false; }
    if (!qdisp) { snprintf(g_err, sizeof g_err, "%s: NULL qdisp", what); return false; }
    if (!time) { snprintf(g_err, sizeof g_err, "%s: NULL time_out", what); return false; }
    if (n == 0) { snprintf(g_err, sizeof g_err, "%s: n == 0", what); return false; }
    return aligned_ok(what, 4, { { item, "item_out" }, { exclude, "exclude" }, { order, "order" } })
           && aligned_ok(what, real_size(s), { { queries, "queries" }, { qdisp, "qdisp" }, { disp, "disp" }, { time, "time_out" }, { normal, "normal_out" } });
}

// One first-contacts call's place among the overlap and swept calls of its scene, and its kernels: under s->overlap.mu it goes behind
// the call before it (swept_begin; it brings no counts, so the list workspace does not grow for it), uses the swept entry's motion table
// (enqueue_query_motion, then the one walk; counters != NULL runs the counting flavour, same bytes), and leaves the event the next call
// waits for -- host calls too: the outputs are the call's own, only the table is shared, so the call need not hold the mutex until its
// stream is drained.
rt_status enqueue_first(rt_scene *s, const void *nodes, uint32_t n_nodes, rt_sweep mode, const void *queries, const void *qdisp, uint32_t n, const void *disp,
                        const int32_t *exclude, const uint32_t *order, void *time, int32_t *item, void *normal, rt::Counters *counters, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(s->overlap.mu);
    rt_status st = swept_begin(s, 0u, n_nodes, stream);
    if (st != RT_OK) return st;
    st = by_precision(s, [&](auto real) -> rt_status {
        using T = decltype(real);
        const ImpactsSpace<T> w = motion_table_space<T>(s->d_swept, s->swept_cap);
        const rt::Node<T> *const stream_nodes = static_cast<const rt::Node<T> *>(nodes);
        const T *const q = static_cast<const T *>(queries), *const qd = static_cast<const T *>(qdisp);
        if (const rt_status mt = enqueue_query_motion<T>(s, stream_nodes, n_nodes, q, qd, n, static_cast<const T *>(disp), w, stream); mt != RT_OK) return mt;
        const rt::FirstArgs<T> a{ stream_nodes, w.motion, w.magnitude, q, qd, exclude, order, static_cast<T *>(time), item, static_cast<T *>(normal), counters, n_nodes, n };
        with_flags([&](auto count, auto any) {
            hipLaunchKernelGGL((rt::k_first_contacts<T, count(), any()>), query_grid(n), query_block(), 0, stream, a);
        }, counters != nullptr, mode == RT_SWEEP_ANY);
        HIP_TRY(hipGetLastError());
        return RT_OK;
    });
    // whatever was enqueued uses the table: the next call goes behind it
    if (hipEventRecord(s->overlap.ev, stream) == hipSuccess) s->overlap.recorded = true;
    else { (void)hipGetLastError(); (void)hipStreamSynchronize(stream); }
    return st;
}

// ---- traced rays and camera frames (rt_trace_rays*, rt_render_camera*, rt_trace.hpp) ----

// The camera domain both rt_render_camera entries check (in double, before the device is touched): 12 finite values, |eye coordinate|
// <= 1e15 (rt_scene_create's eye), every axis of length within [1e-2, 1e2] and |det(right, up, forward)| >= 1e-2 |right| |up| |forward|.
// Within it no sample direction is zero, underflows or overflows, so every normalised direction lies in the ray queries' domain.
bool camera_valid(const rt_scene *s, const void *cam, const char *what)
{
    double v[12];
    for (int k = 0; k < 12; ++k) {
        v[k] = by_precision(s, [&](auto real) { return (double)static_cast<const decltype(real) *>(cam)[k]; });
        if (!std::isfinite(v[k])) { snprintf(g_err, sizeof g_err, "%s: camera value %d is not finite", what, k); return false; }
    }
    for (int k = 0; k < 3; ++k)
        if (std::fabs(v[k]) > 1e15) { snprintf(g_err, sizeof g_err, "%s: |camera eye coordinate| > 1e15", what); return false; }
    double len[3];
    for (int a = 0; a < 3; ++a) {
        const double *p = v + 3 + 3 * a;
        len[a] = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        if (!(len[a] >= 1e-2 && len[a] <= 1e2)) {
            snprintf(g_err, sizeof g_err, "%s: camera axis %d has length %.6g, outside [1e-2, 1e2]", what, a, len[a]);
            return false;
        }
    }
    const double *r = v + 3, *u = v + 6, *f = v + 9;
    const double det = r[0] * (u[1] * f[2] - u[2] * f[1]) - r[1] * (u[0] * f[2] - u[2] * f[0]) + r[2] * (u[0] * f[1] - u[1] * f[0]);
    if (!(std::fabs(det) >= 1e-2 * len[0] * len[1] * len[2])) {
        snprintf(g_err, sizeof g_err, "%s: the camera's right, up and forward axes are (nearly) coplanar", what);
        return false;
    }
    return true;
}

// Pointers and sizes both rt_trace_rays entries check (device pointers are not dereferenced here).
bool trace_args_ok(const rt_scene *s, const void *rays, uint32_t n, const void *color, const void *alpha, const char *what)
{
    if (!s || !rays || !color || n == 0) {
        snprintf(g_err, sizeof g_err, "%s: NULL scene, rays or color_out, or n == 0", what);
        return false;
    }
    return aligned_ok(what, real_size(s), { { rays, "REAL buffers" }, { color, "REAL buffers" }, { alpha, "REAL buffers" } });
}

// One rt_trace_rays launch (rays != NULL; with an order, the rays in that order, rt_order.hpp) or one camera frame over a device tile
// table on `stream`; counters != NULL runs the counting flavour (same bytes).
rt_status enqueue_trace(const rt_scene *s, const void *nodes, uint32_t n_nodes, const void *rays, uint32_t n, void *color, void *alpha,
                        const rt_options *o, const void *cam, const rt::TileDev *d_tab, uint32_t n_tiles, uint32_t blocks, uint8_t *d_out,
                        rt::Counters *counters, hipStream_t stream, const uint32_t *order = nullptr)
{
    by_precision(s, [&](auto real) {
        using T = decltype(real);
        rt::TraceArgs<T> a{};
        a.stream = static_cast<const rt::Node<T> *>(nodes);
        a.items = static_cast<const rt::Item<T> *>(s->d_items);
        a.counters = counters;
        a.rays = static_cast<const T *>(rays);
        a.color = static_cast<T *>(color);
        a.alpha = static_cast<T *>(alpha);
        a.tiles = d_tab;
        a.out = d_out;
        if (cam) for (int k = 0; k < 12; ++k) a.cam[k] = static_cast<const T *>(cam)[k];
        for (int k = 0; k < 3; ++k) a.light[k] = (T)s->light[k];
        a.n_nodes = n_nodes;
        if (rays) {
            a.n = n;
            with_flags([&](auto count, auto ordered) {
                if constexpr (ordered()) hipLaunchKernelGGL((rt::k_trace_rays_ordered<T, count()>), query_grid(n), query_block(), 0, stream, a, order);
                else hipLaunchKernelGGL((rt::k_trace_rays<T, count(), rt::kTraceRays>), query_grid(n), query_block(), 0, stream, a);
            }, counters != nullptr, order != nullptr);
        } else {
            a.n = n_tiles;
            a.width = o->width; a.height = o->height; a.spp = o->samples_per_pixel;
            with_flags([&](auto count) { hipLaunchKernelGGL((rt::k_trace_rays<T, count(), rt::kTraceCamera>), dim3(blocks), query_block(), 0, stream, a); }, counters != nullptr);
        }
    });
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// A counting trace's rt_stats: read_counters's (primary = rays or samples), shadow / occluded as the render counts them and the primary
// walks' share of the tests; the longest-wave fields 0.  Synchronises `stream`.
rt_status read_trace_stats(Context *c, hipStream_t stream, rt_stats *st)
{
    rt::Counters h;
    if (const rt_status rst = read_counters(c, stream, &h, st); rst != RT_OK) return rst;
    st->shadow = h.shadow; st->occluded = h.occluded;
    st->primary_tests = h.primary_tests;
    return RT_OK;
}

// ---- coherent ray batches (rt_ray_order*, rt_*_ordered*; rt_order.hpp) ----

// Where the pieces of a sort of n rays lie in a context's d_sort.  The head (digit totals, plan, box) is what one memset clears.
struct SortLayout {
    unsigned per_block = 0, n_blocks = 0;
    size_t totals = 0, plan = 0, box = 0, head_bytes = 0, table = 0, keys[2] = { 0, 0 }, idx[2] = { 0, 0 }, order = 0, bytes = 0;
};

SortLayout sort_layout(uint32_t n)
{
    SortLayout l;
    uint64_t per = ((uint64_t)n + rt::kSortMaxBlocks - 1) / rt::kSortMaxBlocks;
    per = std::max<uint64_t>(per, rt::kSortTile);
    per = (per + rt::kSortThreads - 1) / rt::kSortThreads * rt::kSortThreads;
    l.per_block = (unsigned)per;
    l.n_blocks = (unsigned)(((uint64_t)n + per - 1) / per);
    auto take = [&](size_t bytes) { const size_t at = l.bytes; l.bytes += (bytes + 255) & ~(size_t)255; return at; };
    l.totals = take(4 * 256 * sizeof(unsigned));
    l.plan = take(sizeof(rt::SortPlan));
    l.box = take(sizeof(rt::RayBox));
    l.head_bytes = l.bytes;
    l.table = take((size_t)256 * l.n_blocks * sizeof(unsigned));
    for (int k = 0; k < 2; ++k) l.keys[k] = take((size_t)n * sizeof(unsigned));
    for (int k = 0; k < 2; ++k) l.idx[k] = take((size_t)n * sizeof(unsigned));
    l.order = take((size_t)n * sizeof(unsigned));
    return l;
}

// rays and order_out as both rt_ray_order entries check them (device pointers are not dereferenced here).
bool order_args_ok(const rt_scene *s, const void *rays, uint32_t n, const uint32_t *order_out, const char *what)
{
    if (!s || !rays || !order_out || n == 0) { snprintf(g_err, sizeof g_err, "%s: NULL scene, rays or order_out, or n == 0", what); return false; }
    const uintptr_t esz = s->precision == RT_F32 ? sizeof(float) : sizeof(double);
    if ((reinterpret_cast<uintptr_t>(rays) % esz) != 0) { snprintf(g_err, sizeof g_err, "%s: REAL buffers must be %u-byte aligned", what, (unsigned)esz); return false; }
    if ((reinterpret_cast<uintptr_t>(order_out) & 3u) != 0) { snprintf(g_err, sizeof g_err, "%s: order_out must be 4-byte aligned", what); return false; }
    return true;
}

// A host order must be a permutation of 0 .. n-1.
bool order_is_permutation(const uint32_t *order, uint32_t n, const char *what)
{
    std::vector<bool> seen;
    try { seen.assign(n, false); } catch (const std::exception &) { snprintf(g_err, sizeof g_err, "%s: out of memory checking the order", what); return false; }
    for (uint32_t j = 0; j < n; ++j) {
        if (order[j] >= n || seen[order[j]]) {
            snprintf(g_err, sizeof g_err, "%s: order[%u] = %u is %s: the order must be a permutation of 0 .. n-1", what, j, order[j],
                     order[j] >= n ? "out of range" : "repeated");
            return false;
        }
        seen[order[j]] = true;
    }
    return true;
}

// The order of n device rays on `stream`, through the context's sort workspace (grown on demand: the context is leased, nothing that is
// enqueued uses it).  order_out: device memory, or NULL for the workspace's own slot; *order_used is where the order ends up.
rt_status enqueue_ray_order(const rt_scene *s, Context *c, const void *rays, uint32_t n, uint32_t *order_out, hipStream_t stream, const uint32_t **order_used)
{
    const SortLayout l = sort_layout(n);
    if (c->sort_cap < l.bytes) {
        if (c->d_sort) HIP_TRY(hipFree(c->d_sort));
        c->d_sort = nullptr; c->sort_cap = 0;
        HIP_TRY(hipMalloc(&c->d_sort, l.bytes));
        c->sort_cap = l.bytes;
    }
    uint8_t *const w = static_cast<uint8_t *>(c->d_sort);
    rt::SortArgs a{};
    for (int k = 0; k < 2; ++k) { a.keys[k] = reinterpret_cast<unsigned *>(w + l.keys[k]); a.idx[k] = reinterpret_cast<unsigned *>(w + l.idx[k]); }
    a.table = reinterpret_cast<unsigned *>(w + l.table);
    rt::SortPlan *const plan = reinterpret_cast<rt::SortPlan *>(w + l.plan);
    a.plan = plan;
    a.order_out = order_out ? order_out : reinterpret_cast<unsigned *>(w + l.order);
    a.n = n; a.per_block = l.per_block; a.n_blocks = l.n_blocks;
    unsigned *const totals = reinterpret_cast<unsigned *>(w + l.totals);
    a.totals = totals;
    rt::RayBox *const box = reinterpret_cast<rt::RayBox *>(w + l.box);
    HIP_TRY(hipMemsetAsync(w, 0, l.head_bytes, stream));
    const dim3 wide((unsigned)std::min<uint64_t>(((uint64_t)n + rt::kSortThreads - 1) / rt::kSortThreads, rt::kSortMaxBlocks)), block(rt::kSortThreads);
    if (s->precision == RT_F32) {
        hipLaunchKernelGGL(rt::k_ray_box<float>, wide, block, 0, stream, static_cast<const float *>(rays), n, box);
        hipLaunchKernelGGL(rt::k_ray_keys<float>, wide, block, 0, stream, static_cast<const float *>(rays), n, box, a.keys[0], totals);
    } else {
        hipLaunchKernelGGL(rt::k_ray_box<double>, wide, block, 0, stream, static_cast<const double *>(rays), n, box);
        hipLaunchKernelGGL(rt::k_ray_keys<double>, wide, block, 0, stream, static_cast<const double *>(rays), n, box, a.keys[0], totals);
    }
    hipLaunchKernelGGL(rt::k_sort_plan, dim3(1), block, 0, stream, totals, n, plan);
    for (unsigned pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(rt::k_sort_hist, dim3(l.n_blocks), block, 0, stream, a, pass);
        hipLaunchKernelGGL(rt::k_sort_scan, dim3(256), block, 0, stream, a, pass);
        hipLaunchKernelGGL(rt::k_sort_scatter, dim3(l.n_blocks), block, 0, stream, a, pass);
    }
    HIP_TRY(hipGetLastError());
    *order_used = a.order_out;
    return RT_OK;
}

// ---- sphere orders and rebuilds (rt_sphere_order*, rt_scene_rebuild*; rt_rebuild.hpp) ----

// The Morton order of n device spheres on `stream`, through `workspace` (sort_layout(n).bytes of device memory: a context's d_sort or a
// scene's rebuild workspace).  order_out: device memory, or NULL for the workspace's own slot; *order_used is where the order ends up.
template <typename T>
rt_status enqueue_sphere_order(void *workspace, const void *spheres, uint32_t n, uint32_t *order_out, hipStream_t stream, const uint32_t **order_used)
{
    const SortLayout l = sort_layout(n);
    uint8_t *const w = static_cast<uint8_t *>(workspace);
    rt::SortArgs a{};
    for (int k = 0; k < 2; ++k) { a.keys[k] = reinterpret_cast<unsigned *>(w + l.keys[k]); a.idx[k] = reinterpret_cast<unsigned *>(w + l.idx[k]); }
    a.table = reinterpret_cast<unsigned *>(w + l.table);
    rt::SortPlan *const plan = reinterpret_cast<rt::SortPlan *>(w + l.plan);
    a.plan = plan;
    a.order_out = order_out ? order_out : reinterpret_cast<unsigned *>(w + l.order);
    a.n = n; a.per_block = l.per_block; a.n_blocks = l.n_blocks;
    unsigned *const totals = reinterpret_cast<unsigned *>(w + l.totals);
    a.totals = totals;
    rt::RayBox *const box = reinterpret_cast<rt::RayBox *>(w + l.box);
    HIP_TRY(hipMemsetAsync(w, 0, l.head_bytes, stream));
    const dim3 wide((unsigned)std::min<uint64_t>(((uint64_t)n + rt::kSortThreads - 1) / rt::kSortThreads, rt::kSortMaxBlocks)), block(rt::kSortThreads);
    hipLaunchKernelGGL(rt::k_sphere_box<T>, wide, block, 0, stream, static_cast<const rt::Item<T> *>(spheres), n, box);
    hipLaunchKernelGGL(rt::k_sphere_keys<T>, wide, block, 0, stream, static_cast<const rt::Item<T> *>(spheres), n, box, a.keys[0], totals);
    hipLaunchKernelGGL(rt::k_sort_plan, dim3(1), block, 0, stream, totals, n, plan);
    for (unsigned pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(rt::k_sort_hist, dim3(l.n_blocks), block, 0, stream, a, pass);
        hipLaunchKernelGGL(rt::k_sort_scan, dim3(256), block, 0, stream, a, pass);
        hipLaunchKernelGGL(rt::k_sort_scatter, dim3(l.n_blocks), block, 0, stream, a, pass);
    }
    HIP_TRY(hipGetLastError());
    *order_used = a.order_out;
    return RT_OK;
}

// The same through a leased context's sort workspace, grown on demand (as enqueue_ray_order grows it).
rt_status enqueue_sphere_order(const rt_scene *s, Context *c, const void *spheres, uint32_t n, uint32_t *order_out, hipStream_t stream, const uint32_t **order_used)
{
    const size_t bytes = sort_layout(n).bytes;
    if (c->sort_cap < bytes) {
        if (c->d_sort) HIP_TRY(hipFree(c->d_sort));
        c->d_sort = nullptr; c->sort_cap = 0;
        HIP_TRY(hipMalloc(&c->d_sort, bytes));
        c->sort_cap = bytes;
    }
    return s->precision == RT_F32 ? enqueue_sphere_order<float>(c->d_sort, spheres, n, order_out, stream, order_used)
                                  : enqueue_sphere_order<double>(c->d_sort, spheres, n, order_out, stream, order_used);
}

// What both rebuild entries check of the scene: a dynamic scene with groups to refit.
rt_status rebuild_scene_ok(const rt_scene *s, const void *spheres, const char *what)
{
    if (!s || !spheres) { snprintf(g_err, sizeof g_err, "%s: NULL scene or spheres", what); return RT_ERR_INVALID_ARGUMENT; }
    if (!s->dynamic) {
        snprintf(g_err, sizeof g_err, "%s: the scene was made by rt_scene_create and is immutable; rt_scene_create_dynamic makes one that can be rebuilt", what);
        return RT_ERR_UNSUPPORTED;
    }
    if (s->n_bounds == 0) {
        snprintf(g_err, sizeof g_err, "%s: the scene was created with n_bounds == 0: a flat scene has no group to refit, so an order changes nothing it walks", what);
        return RT_ERR_UNSUPPORTED;
    }
    return RT_OK;
}

// The sort's part of a scene's rebuild workspace: room for the sort of any n <= n_items keys (rt_scene_rebuild_n*).  Every piece of
// sort_layout grows with n while a slice holds kSortTile keys; past that the digit table may shrink as n grows, so a scene that large
// gets room for the largest table there is.
size_t rebuild_sort_bytes(uint32_t n_items)
{
    size_t bytes = sort_layout(n_items).bytes;
    if ((uint64_t)n_items > (uint64_t)rt::kSortTile * rt::kSortMaxBlocks) bytes += (size_t)256 * rt::kSortMaxBlocks * sizeof(unsigned);
    return bytes;
}

// One rebuild on `stream`: the order of the spheres at `src` (device memory), the gather into the scene's rebuild staging, the refit
// update over the gathered items.  The scene's rebuild workspace -- the sort's, sized by n_items alone, and the staging behind it -- is
// made by the first rebuild and freed with the scene; from then on nothing is allocated and nothing waited for.
template <typename T>
rt_status enqueue_rebuild(rt_scene *s, const void *src, uint32_t *order_out, hipStream_t stream, const uint32_t **order_used)
{
    const size_t sort_bytes = rebuild_sort_bytes(s->n_items);
    {
        std::lock_guard<std::mutex> lk(s->rebuild_mu);
        if (!s->d_rebuild) HIP_TRY(hipMalloc(&s->d_rebuild, sort_bytes + sizeof(rt::Item<T>) * s->n_items));
    }
    rt::Item<T> *const staged = reinterpret_cast<rt::Item<T> *>(static_cast<uint8_t *>(s->d_rebuild) + sort_bytes);      // (sort_bytes is a multiple of 256)
    if (rt_status st = enqueue_sphere_order<T>(s->d_rebuild, src, s->n_items, order_out, stream, order_used); st != RT_OK) return st;
    hipLaunchKernelGGL(rt::k_gather_items<T>, dim3((s->n_items + rt::kBlockThreads - 1) / rt::kBlockThreads), dim3(rt::kBlockThreads), 0, stream,
                       static_cast<const rt::Item<T> *>(src), *order_used, s->n_items, staged);
    HIP_TRY(hipGetLastError());
    return enqueue_dynamic_update<T>(s, staged, nullptr, stream);
}

rt_status enqueue_rebuild(rt_scene *s, const void *src, uint32_t *order_out, hipStream_t stream, const uint32_t **order_used)
{
    return s->precision == RT_F32 ? enqueue_rebuild<float>(s, src, order_out, stream, order_used)
                                  : enqueue_rebuild<double>(s, src, order_out, stream, order_used);
}

// A rebuild of n <= n_items spheres (rt_scene_rebuild_n*): order and gather over n, the live update over the capacity
// with the predicate slot < n for liveness.  The sort of n keys lies inside the workspace of n_items keys (rebuild_sort_bytes).
template <typename T>
rt_status enqueue_rebuild_n(rt_scene *s, const void *src, uint32_t n, uint32_t *order_out, hipStream_t stream, const uint32_t **order_used)
{
    const size_t sort_bytes = rebuild_sort_bytes(s->n_items);
    {
        std::lock_guard<std::mutex> lk(s->rebuild_mu);
        if (!s->d_rebuild) HIP_TRY(hipMalloc(&s->d_rebuild, sort_bytes + sizeof(rt::Item<T>) * s->n_items));
    }
    rt::Item<T> *const staged = reinterpret_cast<rt::Item<T> *>(static_cast<uint8_t *>(s->d_rebuild) + sort_bytes);
    *order_used = nullptr;
    if (n != 0u) {
        if (rt_status st = enqueue_sphere_order<T>(s->d_rebuild, src, n, order_out, stream, order_used); st != RT_OK) return st;
        hipLaunchKernelGGL(rt::k_gather_items<T>, dim3((n + rt::kBlockThreads - 1) / rt::kBlockThreads), dim3(rt::kBlockThreads), 0, stream,
                           static_cast<const rt::Item<T> *>(src), *order_used, n, staged);
        HIP_TRY(hipGetLastError());
    }
    return enqueue_dynamic_update_live<T, true>(s, staged, nullptr, nullptr, n, stream);
}

rt_status enqueue_rebuild_n(rt_scene *s, const void *src, uint32_t n, uint32_t *order_out, hipStream_t stream, const uint32_t **order_used)
{
    return s->precision == RT_F32 ? enqueue_rebuild_n<float>(s, src, n, order_out, stream, order_used)
                                  : enqueue_rebuild_n<double>(s, src, n, order_out, stream, order_used);
}

// ---- undersampled camera frames (rt_render_camera_undersampled*, rt_undersample.hpp) ----

// step in [1, RT_UNDERSAMPLE_MAX_STEP]; prev_step 0 (a fresh frame) or exactly 2 * step (a refinement of the step-2s frame in the buffer).
bool undersample_args_ok(uint32_t step, uint32_t prev_step, const char *what)
{
    if (step < 1 || step > RT_UNDERSAMPLE_MAX_STEP) {
        snprintf(g_err, sizeof g_err, "%s: step is %u, outside 1 .. %d", what, step, RT_UNDERSAMPLE_MAX_STEP);
        return false;
    }
    if (prev_step != 0 && prev_step != 2 * step) {
        snprintf(g_err, sizeof g_err, "%s: prev_step is %u; it must be 0 (a fresh frame) or 2 * step = %u", what, prev_step, 2 * step);
        return false;
    }
    return true;
}

// The blocks of an undersampled pass over a validated tile table (rt_undersample.hpp): per tile, 16 x 16 cells of its step grid (fresh)
// or 8 x 8 cells of its 2 * step grid (refinement), counted in blk_first / blks_x.
rt_status undersample_blocks(std::vector<rt::TileDev> &tab, uint32_t step, bool refine, uint32_t *total_blocks)
{
    const uint32_t unit = refine ? 2 * step : step, per_block = refine ? 8 : (uint32_t)rt::kBlockW;
    uint64_t blocks = 0;
    for (rt::TileDev &t : tab) {
        const uint32_t nx = (t.r - 1u) / unit - t.l / unit + 1u, ny = (t.t - 1u) / unit - t.b / unit + 1u;
        const uint32_t bxs = (nx + per_block - 1) / per_block, bys = (ny + per_block - 1) / per_block;
        t.blk_first = (uint32_t)blocks;
        t.blks_x = bxs;
        blocks += (uint64_t)bxs * bys;
    }
    *total_blocks = (uint32_t)blocks;          // (never more than build_tile_table's 16 x 16 pixel blocks)
    return RT_OK;
}

// One undersampled pass over a device tile table (blocks as undersample_blocks counts them) on `stream`; counters != NULL runs the
// counting flavour (same bytes).
template <typename T>
rt_status enqueue_undersampled(const rt_scene *s, const void *nodes, uint32_t n_nodes, const rt_options *o, const void *cam, const rt::TileDev *d_tab,
                               uint32_t n_tiles, uint32_t blocks, uint32_t step, bool refine, uint8_t *d_out, rt::Counters *counters, hipStream_t stream)
{
    rt::UnderArgs<T> a{};
    a.t.stream = static_cast<const rt::Node<T> *>(nodes);
    a.t.items = static_cast<const rt::Item<T> *>(s->d_items);
    a.t.counters = counters;
    a.t.tiles = d_tab;
    a.t.out = d_out;
    for (int k = 0; k < 12; ++k) a.t.cam[k] = static_cast<const T *>(cam)[k];
    for (int k = 0; k < 3; ++k) a.t.light[k] = (T)s->light[k];
    a.t.n_nodes = n_nodes;
    a.t.n = n_tiles;
    a.t.width = o->width; a.t.height = o->height; a.t.spp = o->samples_per_pixel;
    a.step = step;
    a.refine = refine ? 1u : 0u;
    while ((1u << a.lg_pw) < step) ++a.lg_pw;
    a.lg_p = std::min(6u, 2 * a.lg_pw);
    const dim3 grid(blocks), block(refine ? 192 : rt::kBlockThreads);
    if (counters) hipLaunchKernelGGL((rt::k_trace_undersampled<T, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((rt::k_trace_undersampled<T, false>), grid, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
