// rt_multihit.hpp -- rt_intersect_rays_multi / rt_intersect_rays_multi_device: the k closest hits along each ray, or every hit below
// tmax, for a batch of arbitrary rays -- TypedGroup::intersect (group.rs:72-83 over primitive.rs:55-84) with its single best hit widened
// to a sorted list of k (distance, item) slots.
//
// The walk is made of k_query_rays's pieces (rt_walk.hpp: ray_sphere_t, bound_step_skip): the scene's PLAIN per-origin stream, one ray
// per lane, a per-lane `resume` and a jump to the subtree's skip target once no live lane wants to enter.  Every slot starts as
// (tmax, -1).  A BOUND culls when d >= cut, the lane's own cutoff: the last slot's distance (CLOSEST) or tmax (ALL).  An ITEM with
// !(d >= last slot) (primitive.rs:79's strict `<`) is inserted behind every slot whose distance is <= d and the last slot drops out, so
// equal distances keep DFS order; ALL also counts every ITEM with d < tmax.  With k = 1, CLOSEST is TypedGroup::intersect test for test:
// the bytes and counters of RT_QUERY_NEAREST.
//
// The list lives in registers (a runtime-indexed array would go to scratch): its capacity B is a template parameter, every access
// uses a compile-time slot index and the insertion is a fully unrolled compare-and-shift.  A runtime k < B is served by the first
// B - k slots, which hold -inf: nothing is ever inserted in front of them, they are never reported, and slot B-1 is always the k-th
// real slot -- the cutoff is the last register.
#pragma once
#include "rt_query.hpp"

namespace rt {

template <typename T> struct MultiArgs {
    const Node<T> *stream;      // plain per-origin stream, END-padded
    const Item<T> *items;       // DFS items (the centres for the normals)
    const T *rays;              // [6 n]: pos.xyz, dir.xyz
    const T *tmax;              // [n] or NULL (+inf)
    T *dist;                    // [n k]
    T *normal;                  // [3 n k] or NULL
    int32_t *item;              // [n k] or NULL
    uint32_t *hits;             // [n] or NULL
    Counters *counters;         // COUNT: kCounterStripes slots
    uint32_t n_nodes;           // nodes in front of END
    uint32_t n;                 // rays
    uint32_t k;                 // slots per ray, 1 <= k <= B
};

// The list capacities a launch can pick (the smallest one >= k).
constexpr unsigned kMultiBuckets[] = { 1u, 4u, 8u, 16u };

template <typename T, bool COUNT, bool ALL, int B>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(B <= 4 ? 8 : 4))) void k_multihit_rays(MultiArgs<T> a)
{
    const unsigned gid = lane_query(false, nullptr, a.n);
    const bool live = gid < a.n;
    const size_t g = live ? gid : 0u;
    V3<T> o = { T(0.0), T(0.0), T(0.0) }, d = { T(0.0), T(0.0), T(0.0) };
    T tmax = inf<T>();
    if (live) {
        const T *r = a.rays + 6 * g;
        o = { r[0], r[1], r[2] };
        d = { r[3], r[4], r[5] };
        if (a.tmax) tmax = a.tmax[g];
    }
    const unsigned pad = (unsigned)B - a.k;      // slots [0, pad) are never reported
    T ld[B];
    unsigned li[B];
#pragma unroll
    for (int j = 0; j < B; ++j) { ld[j] = (unsigned)j < pad ? -inf<T>() : tmax; li[j] = kNone; }
    unsigned count = 0;                          // ALL: items below tmax
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
            if (nd.is_bound()) {                                     // BOUND  group.rs:73 against the lane's cutoff
                const bool cull = active && (t >= (ALL ? tmax : ld[B - 1]));
                ni = bound_step_skip<COUNT>(active, cull, nd, i, resume, c_bounds);
            } else {                                                 // ITEM   primitive.rs:78-83, into the list
                if (ALL) count += (active && !(t >= tmax)) ? 1u : 0u;
                // Branch-free, in place from the last slot down: slot j takes slot j-1's entry, or the new one, or keeps its own.  An
                // inactive lane inserts +inf, which is below no slot (and a t >= the last slot is below none either: the list is sorted).
                const T tt = active ? t : inf<T>();
                const unsigned it = nd.index();
#pragma unroll
                for (int j = B - 1; j > 0; --j) {
                    const bool shift = tt < ld[j - 1];
                    const bool here = tt < ld[j];
                    ld[j] = shift ? ld[j - 1] : here ? tt : ld[j];
                    li[j] = shift ? li[j - 1] : here ? it : li[j];
                }
                if (tt < ld[0]) { ld[0] = tt; li[0] = it; }
                if (COUNT) c_items += active ? 1u : 0u;
                ni = i + 1;
            }
            if (ni >= n) break;                                      // also kNever: every lane retired
            i = (unsigned)__builtin_amdgcn_readfirstlane((int)ni);
            nd = a.stream[i];
        }
    }
    unsigned filled = 0;
#pragma unroll
    for (int j = 0; j < B; ++j) filled += ((unsigned)j >= pad && li[j] != kNone) ? 1u : 0u;
    const unsigned hits = ALL ? count : filled;
    if (live) {
        const size_t base = g * a.k - pad;                           // slot j of the list is output slot j - pad
#pragma unroll
        for (int j = 0; j < B; ++j) {
            if ((unsigned)j < pad) continue;
            const size_t q = base + (unsigned)j;
            a.dist[q] = ld[j];                                       // an empty slot: tmax
            if (a.item) a.item[q] = li[j] != kNone ? (int32_t)li[j] : -1;
            if (a.normal) {
                V3<T> nrm = { T(0.0), T(0.0), T(0.0) };
                if (li[j] != kNone) {
                    const Item<T> it = a.items[li[j]];
                    nrm = normalized(add(o, sub(mulf(d, ld[j]), V3<T>{ it.cx, it.cy, it.cz })));     // primitive.rs:82
                }
                T *p = a.normal + 3 * q;
                p[0] = nrm.x; p[1] = nrm.y; p[2] = nrm.z;
            }
        }
        if (a.hits) a.hits[g] = hits;
    }
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum((live && hits > 0u) ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

// k_multihit_rays with the rays taken in a given order (rt_intersect_rays_multi_ordered*; rt_order.hpp): thread j carries
// ray order[j] -- it reads that ray and its tmax and writes every result at that index; an order[j] >= n carries no ray.  The kernel has
// its own text: with one force-inlined body under both kernels the f32 flavours with B >= 4 came out up to 30 instructions longer.
template <typename T, bool COUNT, bool ALL, int B>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(B <= 4 ? 8 : 4))) void k_multihit_rays_ordered(MultiArgs<T> a, const uint32_t *order)
{
    const unsigned gid = lane_query(true, order, a.n);
    const bool live = gid < a.n;
    const size_t g = live ? gid : 0u;
    V3<T> o = { T(0.0), T(0.0), T(0.0) }, d = { T(0.0), T(0.0), T(0.0) };
    T tmax = inf<T>();
    if (live) {
        const T *r = a.rays + 6 * g;
        o = { r[0], r[1], r[2] };
        d = { r[3], r[4], r[5] };
        if (a.tmax) tmax = a.tmax[g];
    }
    const unsigned pad = (unsigned)B - a.k;      // slots [0, pad) are never reported
    T ld[B];
    unsigned li[B];
#pragma unroll
    for (int j = 0; j < B; ++j) { ld[j] = (unsigned)j < pad ? -inf<T>() : tmax; li[j] = kNone; }
    unsigned count = 0;                          // ALL: items below tmax
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
            if (nd.is_bound()) {                                     // BOUND  group.rs:73 against the lane's cutoff
                const bool cull = active && (t >= (ALL ? tmax : ld[B - 1]));
                ni = bound_step_skip<COUNT>(active, cull, nd, i, resume, c_bounds);
            } else {                                                 // ITEM   primitive.rs:78-83, into the list
                if (ALL) count += (active && !(t >= tmax)) ? 1u : 0u;
                // Branch-free, in place from the last slot down: slot j takes slot j-1's entry, or the new one, or keeps its own.  An
                // inactive lane inserts +inf, which is below no slot (and a t >= the last slot is below none either: the list is sorted).
                const T tt = active ? t : inf<T>();
                const unsigned it = nd.index();
#pragma unroll
                for (int j = B - 1; j > 0; --j) {
                    const bool shift = tt < ld[j - 1];
                    const bool here = tt < ld[j];
                    ld[j] = shift ? ld[j - 1] : here ? tt : ld[j];
                    li[j] = shift ? li[j - 1] : here ? it : li[j];
                }
                if (tt < ld[0]) { ld[0] = tt; li[0] = it; }
                if (COUNT) c_items += active ? 1u : 0u;
                ni = i + 1;
            }
            if (ni >= n) break;                                      // also kNever: every lane retired
            i = (unsigned)__builtin_amdgcn_readfirstlane((int)ni);
            nd = a.stream[i];
        }
    }
    unsigned filled = 0;
#pragma unroll
    for (int j = 0; j < B; ++j) filled += ((unsigned)j >= pad && li[j] != kNone) ? 1u : 0u;
    const unsigned hits = ALL ? count : filled;
    if (live) {
        const size_t base = g * a.k - pad;                           // slot j of the list is output slot j - pad
#pragma unroll
        for (int j = 0; j < B; ++j) {
            if ((unsigned)j < pad) continue;
            const size_t q = base + (unsigned)j;
            a.dist[q] = ld[j];                                       // an empty slot: tmax
            if (a.item) a.item[q] = li[j] != kNone ? (int32_t)li[j] : -1;
            if (a.normal) {
                V3<T> nrm = { T(0.0), T(0.0), T(0.0) };
                if (li[j] != kNone) {
                    const Item<T> it = a.items[li[j]];
                    nrm = normalized(add(o, sub(mulf(d, ld[j]), V3<T>{ it.cx, it.cy, it.cz })));     // primitive.rs:82
                }
                T *p = a.normal + 3 * q;
                p[0] = nrm.x; p[1] = nrm.y; p[2] = nrm.z;
            }
        }
        if (a.hits) a.hits[g] = hits;
    }
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum((live && hits > 0u) ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

}  // namespace rt
