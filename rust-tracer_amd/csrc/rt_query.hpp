// rt_query.hpp -- rt_intersect_rays / rt_intersect_rays_device: TypedGroup::intersect(&mut hit, &ray) (group.rs:72-83 over
// primitive.rs:55-84) for a batch of arbitrary rays, one ray per lane, in the caller's order.
//
// The walk is the generic skip-pointer loop of rt_skip.hpp (render_skip_body) over the scene's PLAIN per-origin stream (Node<T>
// {cx, cy, cz, rr, item, skip_off}: the shadow walk's stream, never the compacted one, so no own-sphere bookkeeping), put together
// from the pieces of rt_walk.hpp: ray_sphere_t is the metric, every lane keeps its own hit.distance and one `resume` index,
// bound_step_skip puts a culling lane to sleep until the skip target and takes the wave there once no live lane wants to enter.
//
// hit.distance starts at the caller's tmax (+inf = Hit::missed()).  NEAREST: BOUND culls when d >= best (group.rs:73), ITEM
// updates when !(d >= best) (primitive.rs:79: strict `<`, the first item in DFS order wins a tie); the normal is formed once,
// from the winning item, as primitive.rs:82 forms it.  ANY: best stays tmax, the first ITEM with d < tmax retires the lane, and a
// wave with a newly retired lane goes straight to the smallest `resume` still wanted (item_step_retire).  Until a lane's
// first hit both walks make the same tests as the reference, so "something < tmax" is the reference's own answer.
#pragma once
#include "rt_walk.hpp"

namespace rt {

template <typename T> struct QueryArgs {
    const Node<T> *stream;      // plain per-origin stream, END-padded
    const Item<T> *items;       // DFS items (the winner's centre for the normal)
    const T *rays;              // [6 n]: pos.xyz, dir.xyz
    const T *tmax;              // [n] or NULL (+inf)
    T *dist;                    // [n]
    T *normal;                  // [3 n] or NULL
    int32_t *item;              // [n] or NULL
    Counters *counters;         // COUNT: kCounterStripes slots
    uint32_t n_nodes;           // nodes in front of END
    uint32_t n;                 // rays
};

template <typename T, bool COUNT, bool ANY>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_query_rays(QueryArgs<T> a)
{
    const unsigned gid = lane_query(false, nullptr, a.n);
    const bool live = gid < a.n;
    const size_t g = live ? gid : 0u;
    V3<T> o = { T(0.0), T(0.0), T(0.0) }, d = { T(0.0), T(0.0), T(0.0) };
    T best = inf<T>();
    if (live) {
        const T *r = a.rays + 6 * g;
        o = { r[0], r[1], r[2] };
        d = { r[3], r[4], r[5] };
        if (a.tmax) best = a.tmax[g];
    }
    unsigned best_item = kNone;
    unsigned resume = live ? 0u : kNever;        // a lane without a ray never wakes
    unsigned c_items = 0, c_bounds = 0;
    const unsigned n = a.n_nodes;
    unsigned i = 0;
    if (n != 0u) {
        Node<T> nd = a.stream[0];
        for (;;) {
            const bool active = i >= resume;
            const T t = ray_sphere_t(nd, o, d);
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  group.rs:73
                const bool cull = active && (t >= best);
                ni = bound_step_skip<COUNT>(active, cull, nd, i, resume, c_bounds);
            } else if constexpr (!ANY) {                             // ITEM   primitive.rs:78-83
                if (active && !(t >= best)) { best = t; best_item = nd.index(); }
                if (COUNT) c_items += active ? 1u : 0u;
                ni = i + 1;
            } else {                                                 // ITEM, any hit below tmax retires the lane
                const bool fin = active && !(t >= best);
                if (COUNT) c_items += active ? 1u : 0u;
                if (fin) { best = t; best_item = nd.index(); }
                ni = item_step_retire(fin, i, resume);
            }
            if (ni >= n) break;                                      // also kNever: every lane retired
            i = (unsigned)__builtin_amdgcn_readfirstlane((int)ni);
            nd = a.stream[i];
        }
    }
    if (live) {
        a.dist[g] = best;                                            // (ANY: the retiring item's distance, else tmax)
        if (a.item) a.item[g] = best_item != kNone ? (int32_t)best_item : -1;
        if (a.normal) {
            V3<T> nrm = { T(0.0), T(0.0), T(0.0) };                  // Hit.pos stays at its default when nothing was closer
            if (best_item != kNone) {
                const Item<T> it = a.items[best_item];
                nrm = normalized(add(o, sub(mulf(d, best), V3<T>{ it.cx, it.cy, it.cz })));     // primitive.rs:82
            }
            T *p = a.normal + 3 * g;
            p[0] = nrm.x; p[1] = nrm.y; p[2] = nrm.z;
        }
    }
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum((live && best_item != kNone) ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

// k_query_rays with the rays taken in a given order (rt_intersect_rays_ordered*; rt_order.hpp): thread j carries ray
// order[j] -- it reads that ray and its tmax and writes every result at that index; an order[j] >= n carries no ray (one comparison in
// front of the first load).  The kernel has its own text, made of the same pieces of rt_walk.hpp: one force-inlined body under both
// kernels renamed registers and rescheduled all sixteen flavours, and the any-hit shadow query measured 1 to 2 % slower with it.
template <typename T, bool COUNT, bool ANY>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_query_rays_ordered(QueryArgs<T> a, const uint32_t *order)
{
    const unsigned gid = lane_query(true, order, a.n);
    const bool live = gid < a.n;
    const size_t g = live ? gid : 0u;
    V3<T> o = { T(0.0), T(0.0), T(0.0) }, d = { T(0.0), T(0.0), T(0.0) };
    T best = inf<T>();
    if (live) {
        const T *r = a.rays + 6 * g;
        o = { r[0], r[1], r[2] };
        d = { r[3], r[4], r[5] };
        if (a.tmax) best = a.tmax[g];
    }
    unsigned best_item = kNone;
    unsigned resume = live ? 0u : kNever;        // a lane without a ray never wakes
    unsigned c_items = 0, c_bounds = 0;
    const unsigned n = a.n_nodes;
    unsigned i = 0;
    if (n != 0u) {
        Node<T> nd = a.stream[0];
        for (;;) {
            const bool active = i >= resume;
            const T t = ray_sphere_t(nd, o, d);
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  group.rs:73
                const bool cull = active && (t >= best);
                ni = bound_step_skip<COUNT>(active, cull, nd, i, resume, c_bounds);
            } else if constexpr (!ANY) {                             // ITEM   primitive.rs:78-83
                if (active && !(t >= best)) { best = t; best_item = nd.index(); }
                if (COUNT) c_items += active ? 1u : 0u;
                ni = i + 1;
            } else {                                                 // ITEM, any hit below tmax retires the lane
                const bool fin = active && !(t >= best);
                if (COUNT) c_items += active ? 1u : 0u;
                if (fin) { best = t; best_item = nd.index(); }
                ni = item_step_retire(fin, i, resume);
            }
            if (ni >= n) break;                                      // also kNever: every lane retired
            i = (unsigned)__builtin_amdgcn_readfirstlane((int)ni);
            nd = a.stream[i];
        }
    }
    if (live) {
        a.dist[g] = best;                                            // (ANY: the retiring item's distance, else tmax)
        if (a.item) a.item[g] = best_item != kNone ? (int32_t)best_item : -1;
        if (a.normal) {
            V3<T> nrm = { T(0.0), T(0.0), T(0.0) };                  // Hit.pos stays at its default when nothing was closer
            if (best_item != kNone) {
                const Item<T> it = a.items[best_item];
                nrm = normalized(add(o, sub(mulf(d, best), V3<T>{ it.cx, it.cy, it.cz })));     // primitive.rs:82
            }
            T *p = a.normal + 3 * g;
            p[0] = nrm.x; p[1] = nrm.y; p[2] = nrm.z;
        }
    }
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum((live && best_item != kNone) ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

// A scene created without bounds has no hierarchy stream: the query walks its items as a stream of ITEM nodes (the flat nearest hit
// over all items), built once on first use -- the same records k_build_streams writes for an item of the shadow stream, END-padded.
template <typename T>
__global__ void k_items_stream(const Item<T> *__restrict__ items, unsigned n, Node<T> *__restrict__ out)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n + kNodePad) return;
    constexpr unsigned kStride = (unsigned)sizeof(Node<T>);
    Node<T> s;
    if (i >= n) {
        per_origin_end(s, n);
    } else {
        const Item<T> it = items[i];
        per_origin_terms(s, it.cx, it.cy, it.cz, it.r);
        s.item = i | kNodeItem;
        s.skip_off = (i + 1u) * kStride;
    }
    out[i] = s;
}

}  // namespace rt
