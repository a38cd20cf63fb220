// rt_near.hpp -- rt_near_spheres / rt_near_spheres_device: the k nearest spheres of a point, or every sphere within a radius, for a batch
// of points.  No ray: the metric is the surface GAP between the point p and a sphere {c, r}.
//
// The gap of a stream record {c, rr} (rr = the radius squared, rounded once: per_origin_terms, rt_skip.hpp), in REAL, every operation
// rounded once, no FMA contraction:
//     v   = c - p
//     vv  = (v.x*v.x + v.y*v.y) + v.z*v.z                 dot()'s order
//     gap = rr > 0 ? sqrt(vv) - sqrt(rr) : +inf           both roots correctly rounded (sqrt_rn_lean)
// negative when p is inside the sphere.  A bound encloses its items, so its gap is a lower bound of theirs -- what a bound's ray distance
// is to the ray queries.  The guard belongs to the definition: the dead record of DESIGN.md 4.13 is {0, 0, 0, -inf}, whose root would be
// NaN; with the guard a dead ITEM has gap +inf (never below a cutoff: never listed, never counted) and a dead BOUND culls for every query.
//
// The walk is k_multihit_rays's (rt_multihit.hpp; the shared pieces are rt_walk.hpp's) over the same plain per-origin stream: one query
// per lane, a per-lane `resume`, a jump to the skip target once no live lane wants to enter.  The gap and the BOUND step stand in this
// kernel's own text -- rt_walk.hpp's centre_gap with q = 0 and bound_step_skip, which made the f64 B = 4 flavours 30 to 40 instructions
// longer when called from here.  Every slot starts as (rho, -1).  A BOUND culls when gap >= cut: the last slot's gap (CLOSEST) or rho
// (ALL).  An ITEM with !(gap >= last slot) is inserted behind every slot whose gap is <= its own, so equal gaps keep DFS order; ALL also
// counts every ITEM with !(gap >= rho).  The query's `exclude` slot is tested and counted as a test, but neither inserted nor counted as
// found.
//
// The list lives in registers as multihit's does: capacity B is a template parameter (kMultiBuckets), a runtime k < B leaves the first
// B - k slots at -inf, every access has a compile-time index and the insertion is the branch-free compare-and-shift.
#pragma once
#include "rt_multihit.hpp"

namespace rt {

template <typename T> struct NearArgs {
    const Node<T> *stream;      // plain per-origin stream, END-padded
    const T *points;            // [3 n]
    const T *radius;            // [n] or NULL (+inf)
    const int32_t *exclude;     // [n] or NULL: the item slot query g ignores (-1, or any slot outside the scene: none)
    const uint32_t *order;      // ORDERED: [n], thread j carries query order[j]; an entry >= n carries none
    T *gap;                     // [n k]
    int32_t *item;              // [n k] or NULL
    uint32_t *found;            // [n] or NULL
    Counters *counters;         // COUNT: kCounterStripes slots
    uint32_t n_nodes;           // nodes in front of END
    uint32_t n;                 // queries
    uint32_t k;                 // slots per query, 1 <= k <= B
};

template <typename T, bool COUNT, bool ALL, bool ORDERED, int B>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(B <= 4 ? 8 : 4))) void k_near_spheres(NearArgs<T> a)
{
    const unsigned gid = lane_query(ORDERED, a.order, a.n);
    const bool live = gid < a.n;
    const size_t g = live ? gid : 0u;
    V3<T> p = { T(0.0), T(0.0), T(0.0) };
    T rho = inf<T>();
    unsigned excl = kNone;
    if (live) {
        const T *q = a.points + 3 * g;
        p = { q[0], q[1], q[2] };
        if (a.radius) rho = a.radius[g];
        if (a.exclude) excl = (unsigned)a.exclude[g];
    }
    const unsigned pad = (unsigned)B - a.k;      // slots [0, pad) are never reported
    T ld[B];
    unsigned li[B];
#pragma unroll
    for (int j = 0; j < B; ++j) { ld[j] = (unsigned)j < pad ? -inf<T>() : rho; li[j] = kNone; }
    unsigned count = 0;                          // ALL: items below rho
    unsigned resume = live ? 0u : kNever;        // a lane without a query never wakes
    unsigned c_items = 0, c_bounds = 0;
    const unsigned n = a.n_nodes;
    unsigned i = 0;
    if (n != 0u) {
        Node<T> nd = a.stream[0];
        for (;;) {
            const bool active = i >= resume;
            // the gap, every operation rounded once; the record's root is the same value in every lane
            const V3<T> v = { nd.a0 - p.x, nd.a1 - p.y, nd.a2 - p.z };
            const T vv = dot(v, v);
            T t = inf<T>();
            if (nd.a3 > T(0.0)) t = sqrt_rn_lean(vv) - sqrt_rn_lean(nd.a3);
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  against the lane's cutoff
                const bool cull = active && (t >= (ALL ? rho : ld[B - 1]));
                if (cull) resume = nd.skip();
                if (COUNT) c_bounds += active ? 1u : 0u;
                ni = (__ballot(active && !cull) == 0) ? nd.skip() : i + 1;
            } else {                                                 // ITEM   into the list
                const unsigned it = nd.index();
                const bool take = active && it != excl;
                if (ALL) count += (take && !(t >= rho)) ? 1u : 0u;
                // Branch-free, in place from the last slot down (rt_multihit.hpp): a lane that is inactive or excludes this item inserts
                // +inf, which is below no slot.
                const T tt = take ? t : inf<T>();
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
    const unsigned found = ALL ? count : filled;
    if (live) {
        const size_t base = g * a.k - pad;                           // slot j of the list is output slot j - pad
#pragma unroll
        for (int j = 0; j < B; ++j) {
            if ((unsigned)j < pad) continue;
            const size_t q = base + (unsigned)j;
            a.gap[q] = ld[j];                                        // an empty slot: rho
            if (a.item) a.item[q] = li[j] != kNone ? (int32_t)li[j] : -1;
        }
        if (a.found) a.found[g] = found;
    }
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum((live && found > 0u) ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

}  // namespace rt
