// rt_sweep.hpp -- rt_sweep_spheres / rt_sweep_spheres_device: the first contact of a moving sphere with the scene, for a batch of casts
// (DESIGN.md 4.15).  Cast g is a ray {pos, dir} (dir a unit vector), a radius q and a cutoff tmax: how far can a sphere of radius q whose
// centre starts at pos move along dir before it touches something?
//
// A sphere of radius q moving along a ray touches a sphere {c, r} exactly where the ray hits {c, r + q}.  The cast distance of a stream
// record {c, rr} (rr = the radius squared, rounded once: per_origin_terms, rt_skip.hpp), in REAL, every operation rounded once, no FMA
// contraction, both roots correctly rounded (sqrt_rn_lean):
//     rad  = sqrt(rr)                                  the same value in every lane
//     RR   = (rr + (q + q) * rad) + q * q              (r + q)^2 expanded; q = 0 gives RR == rr bit for bit
//     v    = c - pos ;  b = dot(v, dir) ;  disc = (b*b - dot(v, v)) + RR            rt_query.hpp's order
//     t    = +inf                   if !(rr > 0)  or  disc < 0  or  b + sqrt(disc) < 0
//          = b - sqrt(disc)         if that is > 0
//          = 0                      otherwise: the moving sphere touches or overlaps the record at its start
// The start case is 0, not the ray query's exit distance: the inflated bound's distance is then a lower bound of its inflated items'
// distances, and a cast that starts in contact reports 0 and that item.  The guard rr > 0 is rt_near.hpp's: the dead record of DESIGN.md
// 4.13 is {0, 0, 0, -inf}, whose root would be NaN; with the guard a dead ITEM is at +inf (never below a cutoff) and a dead BOUND culls
// for every cast.
//
// The walk is made of k_query_rays's pieces (rt_walk.hpp: bound_step_skip, item_step_retire) over the same plain per-origin stream: one
// cast per lane, a per-lane `resume`, a jump to the skip target once no live lane wants to enter; the metric above has its one copy in
// the loop below.  `best` starts at tmax.  A BOUND culls when t >= best.  NEAREST: an ITEM with !(t >= best) becomes the result (the
// first item in DFS order wins a tie, several items at 0 included).  ANY: the first ITEM with !(t >= tmax) retires the lane, and the wave
// goes to the smallest `resume` still wanted.  The cast's `exclude` slot is tested and counted as a test, but can never win or retire
// the lane.  The index only grows, so the walk ends whatever bits the casts carry.
#pragma once
#include "rt_walk.hpp"

namespace rt {

template <typename T> struct SweepArgs {
    const Node<T> *stream;      // plain per-origin stream, END-padded
    const Item<T> *items;       // DFS items (the winner's centre for the normal)
    const T *rays;              // [6 n]: pos.xyz, dir.xyz
    const T *radius;            // [n] or NULL (0)
    const T *tmax;              // [n] or NULL (+inf)
    const int32_t *exclude;     // [n] or NULL: the item slot cast g ignores (-1, or any slot outside the scene: none)
    const uint32_t *order;      // ORDERED: [n], thread j carries cast order[j]; an entry >= n carries none
    T *dist;                    // [n]
    T *normal;                  // [3 n] or NULL
    int32_t *item;              // [n] or NULL
    Counters *counters;         // COUNT: kCounterStripes slots
    uint32_t n_nodes;           // nodes in front of END
    uint32_t n;                 // casts
};

template <typename T, bool COUNT, bool ANY, bool ORDERED>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_sweep_spheres(SweepArgs<T> a)
{
    const unsigned gid = lane_query(ORDERED, a.order, a.n);
    const bool live = gid < a.n;
    const size_t g = live ? gid : 0u;
    V3<T> o = { T(0.0), T(0.0), T(0.0) }, d = { T(0.0), T(0.0), T(0.0) };
    T best = inf<T>(), q = T(0.0);
    unsigned excl = kNone;
    if (live) {
        const T *r = a.rays + 6 * g;
        o = { r[0], r[1], r[2] };
        d = { r[3], r[4], r[5] };
        if (a.radius) q = a.radius[g];
        if (a.tmax) best = a.tmax[g];
        if (a.exclude) excl = (unsigned)a.exclude[g];
    }
    const T q2 = q + q, qq = q * q;              // the lane's part of (r + q)^2
    unsigned best_item = kNone;
    unsigned resume = live ? 0u : kNever;        // a lane without a cast never wakes
    unsigned c_items = 0, c_bounds = 0;
    const unsigned n = a.n_nodes;
    unsigned i = 0;
    if (n != 0u) {
        Node<T> nd = a.stream[0];
        for (;;) {
            const bool active = i >= resume;
            // the record inflated by the lane's radius, then Sphere::distance_from_ray's order with 0 for a start in contact
            const T RR = (nd.a3 + q2 * sqrt_rn_lean(nd.a3)) + qq;
            const V3<T> v = { nd.a0 - o.x, nd.a1 - o.y, nd.a2 - o.z };
            const T b = dot(v, d);
            const T disc = (b * b - dot(v, v)) + RR;
            T t = inf<T>();
            if (nd.a3 > T(0.0) && !(disc < T(0.0))) {
                const T s = sqrt_rn_lean(disc);
                if (!(b + s < T(0.0))) {
                    const T t1 = b - s;
                    t = t1 > T(0.0) ? t1 : T(0.0);
                }
            }
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND
                const bool cull = active && (t >= best);
                ni = bound_step_skip<COUNT>(active, cull, nd, i, resume, c_bounds);
            } else if constexpr (!ANY) {                             // ITEM, the nearest so far
                const unsigned it = nd.index();
                if (active && it != excl && !(t >= best)) { best = t; best_item = it; }
                if (COUNT) c_items += active ? 1u : 0u;
                ni = i + 1;
            } else {                                                 // ITEM, any contact below tmax retires the lane
                const unsigned it = nd.index();
                const bool fin = active && it != excl && !(t >= best);
                if (COUNT) c_items += active ? 1u : 0u;
                if (fin) { best = t; best_item = it; }
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
            V3<T> nrm = { T(0.0), T(0.0), T(0.0) };
            if (best_item != kNone) {                                // from the touched sphere to the moving sphere's centre at contact
                const Item<T> it = a.items[best_item];
                nrm = normalized(add(o, sub(mulf(d, best), V3<T>{ it.cx, it.cy, it.cz })));     // rt_query.hpp's expression
            }
            T *p = a.normal + 3 * g;
            p[0] = nrm.x; p[1] = nrm.y; p[2] = nrm.z;
        }
    }
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum((live && best_item != kNone) ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

}  // namespace rt
