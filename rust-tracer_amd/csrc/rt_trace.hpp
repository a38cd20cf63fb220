// rt_trace.hpp -- rt_trace_rays* / rt_render_camera*: Renderer::raytrace (render.rs:171-215) for arbitrary rays, and the reference's whole
// per-pixel pipeline (render.rs:218-255) for a pinhole camera of the caller's choice.
//
// Each ray makes two walks over the scene's PLAIN per-origin stream (the shadow walk's stream of rt_skip.hpp; a scene without bounds:
// its items-only stream, rt_query.hpp k_items_stream), both the loop of k_query_rays: a wave-uniform stream index (node records arrive
// through the scalar cache), one `resume` index per lane, the tests in the reference's order.
//   primary  nearest hit from pos, hit.distance = +inf going in: BOUND culls at d >= best (group.rs:73), ITEM updates at !(d >= best)
//   shade    render_skip_body's: nrm, g = nrm . light, the ambient exit at g >= 0, sp = (pos + dir*best) + nrm*(best*sqrt(EPSILON))
//   shadow   any hit from sp along -light: a BOUND culls the lanes its sphere misses, the first ITEM hit retires the lane (only
//            has_missed() is asked afterwards); lanes without a shadow ray sit the walk out
// The walks make the reference's tests one for one, so the counters mean what the render's counting launches report.
//
// SRC = kTraceRays:   ray i = rays[6i .. 6i+6], one per lane in the caller's order -> the colour raytrace() leaves in a c = {0, 0, 0} and
//                     its return value (alpha 0 or 1).
// SRC = kTraceCamera: one thread per pixel of a tile list, laid out as the render kernels lay it out (a 16x16 block per workgroup, an 8x8
//                     patch per wave): the camera's rays of neighbouring pixels stay coherent.  The thread takes its samples in the
//                     reference's order (ssx outer, ssy inner), accumulates g and alpha term by term as the non-SPLIT render does, scales
//                     by 1 / (ssf*ssf) and stores scale_u8 RGBA tile-major (out_index) -- no sample buffer, no resolve pass.
//   The sample ray of a camera {eye, right, up, forward} (REAL[12]): u = xres - w/2, v = (h - yres) - h/2, f = w (render.rs:238-242) and
//   dir = normalized((right*u + up*v) + forward*f) component by component, every operation rounded once; pos = eye.  With the identity
//   basis that is the reference's (u, v, f) bit for bit (times 0 or 1 and plus +-0 change nothing: f >= 1, u and v are never -0).
#pragma once
#include "rt_skip.hpp"

namespace rt {

enum { kTraceRays = 0, kTraceCamera = 1 };

template <typename T> struct TraceArgs {
    const Node<T> *stream;      // plain per-origin stream (or the items-only one), END-padded
    const Item<T> *items;       // DFS items (the winner's centre for the normal)
    Counters *counters;         // COUNT: kCounterStripes slots
    // kTraceRays
    const T *rays;              // [6 n]: pos.xyz, dir.xyz
    T *color;                   // [3 n]
    T *alpha;                   // [n] or NULL
    // kTraceCamera
    const TileDev *tiles;
    uint8_t *out;               // tile-major RGBA
    T cam[12];                  // eye, right, up, forward
    T light[3];
    uint32_t n_nodes;           // nodes in front of END
    uint32_t n;                 // rays (kTraceRays) / tiles (kTraceCamera)
    uint32_t width, height, spp;
};

// Per-lane counts of one thread's rays.
struct TraceCounts { unsigned hits = 0, shadow = 0, occ = 0, items = 0, bounds = 0, ptests = 0; };

// raytrace (render.rs:186-213) for one ray per lane: the exit it takes (SampleState) and n.light where it got that far.
template <typename T, bool COUNT>
__device__ __forceinline__ uint8_t trace_ray(const TraceArgs<T> &a, V3<T> o, V3<T> d, bool live, T &gdot, TraceCounts &c)
{
    constexpr unsigned kNone = 0xFFFFFFFFu;
    const unsigned n = a.n_nodes;
    // ---------------- primary ray: s.group.intersect(&mut h, r)  render.rs:188-189 ----------------
    T best = inf<T>();
    unsigned best_item = kNone;
    unsigned resume = live ? 0u : kNever;
    const unsigned t_before = c.items + c.bounds;
    if (n != 0u) {
        unsigned i = 0;
        Node<T> nd = a.stream[0];
        for (;;) {
            const bool active = i >= resume;
            // Sphere::distance_from_ray (primitive.rs:55-72) in the reference's order, every operation rounded once
            const V3<T> v = { nd.a0 - o.x, nd.a1 - o.y, nd.a2 - o.z };
            const T b = dot(v, d);
            const T disc = (b * b - dot(v, v)) + nd.a3;
            T t = inf<T>();
            if (!(disc < T(0.0))) {
                const T s = sqrt_rn_lean(disc);
                const T t2 = b + s;
                if (!(t2 < T(0.0))) {
                    const T t1 = b - s;
                    t = t1 > T(0.0) ? t1 : t2;
                }
            }
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  group.rs:73
                const bool cull = active && (t >= best);
                if (cull) resume = nd.skip();
                if (COUNT) c.bounds += active ? 1u : 0u;
                ni = (__ballot(active && !cull) == 0) ? nd.skip() : i + 1;
            } else {                                                 // ITEM   primitive.rs:78-83
                if (active && !(t >= best)) { best = t; best_item = nd.index(); }
                if (COUNT) c.items += active ? 1u : 0u;
                ni = i + 1;
            }
            if (ni >= n) break;
            i = (unsigned)__builtin_amdgcn_readfirstlane((int)ni);
            nd = a.stream[i];
        }
    }
    if (COUNT) c.ptests += c.items + c.bounds - t_before;
    // ---------------- shade  render.rs:190-199 ----------------
    const V3<T> light = { a.light[0], a.light[1], a.light[2] };
    uint8_t state = kMiss;
    bool need_shadow = false;
    V3<T> sp = { T(0.0), T(0.0), T(0.0) };
    gdot = T(0.0);
    if (live && best_item != kNone) {
        if (COUNT) ++c.hits;
        const Item<T> it = a.items[best_item];
        const V3<T> nrm = normalized(add(o, sub(mulf(d, best), V3<T>{ it.cx, it.cy, it.cz })));      // primitive.rs:83
        gdot = dot(nrm, light);
        if (gdot >= T(0.0)) {
            state = kAmbient;
        } else {
            need_shadow = true;
            if (COUNT) ++c.shadow;
            sp = add(add(o, mulf(d, best)), mulf(nrm, best * rsqrt_exact(eps<T>())));
        }
    }
    // ---------------- shadow ray: any hit  render.rs:202-208 ----------------
    // hit.distance stays INF until the first hit, so a bound culls iff the ray misses it; the lane retires at its first item hit.
    bool occluded = false;
    if (n != 0u && __ballot(need_shadow) != 0) {
        const V3<T> sdir = mulf(light, T(-1.0));                     // render.rs:206
        resume = need_shadow ? 0u : kNever;
        unsigned i = 0;
        Node<T> nd = a.stream[0];
        for (;;) {
            const bool active = i >= resume;
            const V3<T> v = { nd.a0 - sp.x, nd.a1 - sp.y, nd.a2 - sp.z };
            const T b = dot(v, sdir);
            const T disc = (b * b - dot(v, v)) + nd.a3;
            const bool hit = !(disc < T(0.0)) && !((b + sqrt_rn_lean(disc)) < T(0.0));
            unsigned ni;
            if (nd.is_bound()) {
                const bool cull = active && !hit;
                if (cull) resume = nd.skip();
                if (COUNT) c.bounds += active ? 1u : 0u;
                ni = (__ballot(active && hit) == 0) ? nd.skip() : i + 1;
            } else {
                const bool fin = active && hit;
                if (COUNT) c.items += active ? 1u : 0u;
                if (fin) { occluded = true; resume = kNever; }
                // some lane retired: go straight to the next node any lane still wants
                ni = (__ballot(fin) != 0) ? wave_min_u32(resume == kNever ? kNever : (resume > i ? resume : i + 1)) : i + 1;
            }
            if (ni >= n) break;                                      // also kNever: every lane retired
            i = (unsigned)__builtin_amdgcn_readfirstlane((int)ni);
            nd = a.stream[i];
        }
    }
    if (need_shadow) {
        state = occluded ? kShadowed : kLit;
        if (COUNT && occluded) ++c.occ;
    }
    return state;
}

// *c = *c + ... as raytrace() adds its exit's colour (render.rs:191-213); returns raytrace()'s value.
template <typename T>
__device__ __forceinline__ T accumulate(V3<T> &g, uint8_t state, T gdot)
{
    const V3<T> OBJECT = { T(0xae) / T(255.0), T(0x31) / T(255.0), T(0x31) / T(255.0) };
    const V3<T> BACKGROUND = { T(0x22) / T(255.0), T(0x0a) / T(255.0), T(0x0a) / T(255.0) };
    const V3<T> AMBIENT = { BACKGROUND.x * T(0.8), BACKGROUND.y * T(0.8), BACKGROUND.z * T(0.8) };
    if (state == kMiss) g = add(g, BACKGROUND);
    else if (state == kAmbient) g = add(g, AMBIENT);
    else if (state == kLit) { g = add(add(g, mulf(OBJECT, -gdot)), AMBIENT); return T(1.0); }          // render.rs:209
    else g = add(add(g, BACKGROUND), mulf(AMBIENT, -gdot));                                              // render.rs:212
    return T(0.0);
}

// Eight waves per SIMD (64 VGPRs, no scratch) for the product flavours; the counting ones keep seven more per-lane counts and may take the
// registers of fewer waves instead of spilling.
template <typename T, bool COUNT, int SRC>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(COUNT ? 4 : 8))) void k_trace_rays(TraceArgs<T> a)
{
    TraceCounts c;
    unsigned rays_here = 0;
    unsigned stripe_of = blockIdx.x;
    if constexpr (SRC == kTraceRays) {
        const unsigned gid = blockIdx.x * kBlockThreads + threadIdx.x;
        const bool live = gid < a.n;
        const size_t k = live ? gid : 0u;
        V3<T> o = { T(0.0), T(0.0), T(0.0) }, d = { T(0.0), T(0.0), T(0.0) };
        if (live) {
            const T *r = a.rays + 6 * k;
            o = { r[0], r[1], r[2] };
            d = { r[3], r[4], r[5] };
        }
        T gdot;
        const uint8_t state = trace_ray<T, COUNT>(a, o, d, live, gdot, c);
        if (live) {
            V3<T> g = { T(0.0), T(0.0), T(0.0) };
            const T alpha = accumulate(g, state, gdot);
            T *p = a.color + 3 * k;
            p[0] = g.x; p[1] = g.y; p[2] = g.z;
            if (a.alpha) a.alpha[k] = alpha;
            rays_here = 1;
        }
    } else {
        // the block's tile: the last one whose first block is <= blockIdx.x (block-uniform)
        unsigned lo = 0, hi = a.n - 1;
        while (lo < hi) {
            const unsigned mid = (lo + hi + 1) >> 1;
            if (a.tiles[mid].blk_first <= blockIdx.x) lo = mid; else hi = mid - 1;
        }
        const TileDev tile = a.tiles[lo];
        const unsigned lb = blockIdx.x - tile.blk_first;
        const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const unsigned x = tile.l + (lb % tile.blks_x) * kBlockW + (wave & 1) * 8u + (lane & 7u);
        const unsigned y = tile.b + (lb / tile.blks_x) * kBlockH + (wave >> 1) * 8u + (lane >> 3);
        const bool inside = x < tile.r && y < tile.t;
        if (__ballot(inside) == 0) return;          // (waves are independent: no LDS, no barrier)
        const unsigned spp = a.spp;
        const T ssf = T(spp);
        const T total_recip = T(1.0) / (ssf * ssf);
        const T fw = T(a.width), fh = T(a.height);
        const T half_w = fw / T(2.0), half_h = fh / T(2.0);
        const V3<T> eye = { a.cam[0], a.cam[1], a.cam[2] };
        V3<T> g = { T(0.0), T(0.0), T(0.0) };
        T alpha = T(0.0);
        for (unsigned ssx = 0; ssx < spp; ++ssx) {
            for (unsigned ssy = 0; ssy < spp; ++ssy) {
                const T xres = T(x) + T(ssx) / ssf;                  // render.rs:238-242
                const T yres = T(y) + T(ssy) / ssf;
                const T u = xres - half_w, v = (fh - yres) - half_h;
                const V3<T> dir = normalized(V3<T>{ (a.cam[3] * u + a.cam[6] * v) + a.cam[9] * fw,
                                                    (a.cam[4] * u + a.cam[7] * v) + a.cam[10] * fw,
                                                    (a.cam[5] * u + a.cam[8] * v) + a.cam[11] * fw });
                T gdot;
                const uint8_t state = trace_ray<T, COUNT>(a, eye, dir, inside, gdot, c);
                if (inside) alpha += accumulate(g, state, gdot);
            }
        }
        if (inside) {
            g = mulf(g, total_recip);                                // render.rs:251-253
            alpha *= total_recip;
            const unsigned rgba = scale_u8(g.x) | (scale_u8(g.y) << 8) | (scale_u8(g.z) << 16) | (scale_u8(alpha) << 24);
            reinterpret_cast<unsigned *>(a.out)[out_index(tile, x, y, 0)] = rgba;
            rays_here = spp * spp;
        }
    }
    if constexpr (COUNT) {
        const unsigned long long prim = wave_sum(rays_here), hits = wave_sum(c.hits), sh = wave_sum(c.shadow), oc = wave_sum(c.occ);
        const unsigned long long its = wave_sum(c.items), bds = wave_sum(c.bounds), ptot = wave_sum(c.ptests);
        if ((threadIdx.x & 63u) == 0u) {
            Counters *const stripe = a.counters + stripe_of % kCounterStripes;
            atomicAdd(&stripe->primary, prim);
            atomicAdd(&stripe->hits, hits);
            atomicAdd(&stripe->shadow, sh);
            atomicAdd(&stripe->occluded, oc);
            atomicAdd(&stripe->sphere_tests, its);
            atomicAdd(&stripe->bound_tests, bds);
            atomicAdd(&stripe->primary_tests, ptot);
        }
    }
}

// k_trace_rays<T, COUNT, kTraceRays> with the rays taken in a given order (rt_trace_rays_ordered*; rt_order.hpp): thread j
// carries ray order[j] -- it reads that ray and writes its colour and alpha at that index; an order[j] >= n carries no ray.
template <typename T, bool COUNT>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(COUNT ? 4 : 8))) void k_trace_rays_ordered(TraceArgs<T> a, const uint32_t *order)
{
    TraceCounts c;
    unsigned rays_here = 0;
    const unsigned gid = blockIdx.x * kBlockThreads + threadIdx.x;
    bool live = gid < a.n;
    size_t k = 0u;
    if (live) {
        const unsigned q = order[gid];
        live = q < a.n;
        k = live ? q : 0u;
    }
    V3<T> o = { T(0.0), T(0.0), T(0.0) }, d = { T(0.0), T(0.0), T(0.0) };
    if (live) {
        const T *r = a.rays + 6 * k;
        o = { r[0], r[1], r[2] };
        d = { r[3], r[4], r[5] };
    }
    T gdot;
    const uint8_t state = trace_ray<T, COUNT>(a, o, d, live, gdot, c);
    if (live) {
        V3<T> g = { T(0.0), T(0.0), T(0.0) };
        const T alpha = accumulate(g, state, gdot);
        T *p = a.color + 3 * k;
        p[0] = g.x; p[1] = g.y; p[2] = g.z;
        if (a.alpha) a.alpha[k] = alpha;
        rays_here = 1;
    }
    if constexpr (COUNT) {
        const unsigned long long prim = wave_sum(rays_here), hits = wave_sum(c.hits), sh = wave_sum(c.shadow), oc = wave_sum(c.occ);
        const unsigned long long its = wave_sum(c.items), bds = wave_sum(c.bounds), ptot = wave_sum(c.ptests);
        if ((threadIdx.x & 63u) == 0u) {
            Counters *const stripe = a.counters + blockIdx.x % kCounterStripes;
            atomicAdd(&stripe->primary, prim);
            atomicAdd(&stripe->hits, hits);
            atomicAdd(&stripe->shadow, sh);
            atomicAdd(&stripe->occluded, oc);
            atomicAdd(&stripe->sphere_tests, its);
            atomicAdd(&stripe->bound_tests, bds);
            atomicAdd(&stripe->primary_tests, ptot);
        }
    }
}

}  // namespace rt
